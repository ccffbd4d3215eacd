"""What tests/test_bf16_launches_gpu.py covers, checked without a GPU (engine.plan_layout: the host-only planner on 256 compute units, built first as
for tests/test_plan_layout.py), and that its half-ulp grade and its copy identity can tell a wrong launch from a right one.

The bf16 aortic U-Net runs on persistent "walker" kernels: the weight-stationary convs / transposed convs of kernels_ws.hip (tilings 400, 401, 402,
410, 411, the ring form 422), the fused stem (kernels_stem.hip) and the fused tail (kernels_tail.hip).  Each launcher sizes its grid to the chip and
never starts more workgroups than the tiles need; each wave then takes tiles worker, worker + nworkers, ...  A launch's SITUATION -- how many rounds its
waves make and whether the last one is ragged, the tile order, whole or ragged 32-column tiles, the workgroup placement -- is computed here from the
plan op's map and the launchers' own arithmetic, whose constants and lines are read from the sources and asserted
(test_launcher_constants_are_the_ones_assumed).  Round classes, ntiles against nworkers = waves of the grid:

    below     ntiles <= nworkers             every wave at most one tile
    between   nworkers < ntiles < 2 nworkers  some waves two tiles, some one
    two+      ntiles >= 2 nworkers            'exact' (ntiles % nworkers == 0) or 'ragged'

REQUIREMENTS (requirements()):
  a. every (layer, tiling) combination of the recorded default bf16 plans of UNet_ao (tests/golden/plan_layouts.json, knob '': 61, the fused stem and
     tail among them) is planned by some case; a tile-per-workgroup tiling (below 400) counts only on a map its tiles divide, or do not divide, as some
     recorded plan of that combination has it (the rule of tests/test_fp32_launch_coverage.py, here for every such tiling);
  b. every weight-stationary (layer, tiling, tile order) of the plans of the two benchmark batches, 100 x 256 x 256 and 100 x 192 x 208, in each round
     class those batches put it in and in the class below it; and per tiling: every round class (422: below and between only -- two+ needs more than
     100 x 256 x 256 pixels, which the benchmark does not reach either), wave-major and XCD-local order where the benchmark batches reach both (401, 410),
     whole and ragged 32-column tiles, a grid that is and is not a multiple of 8 nG (the two placements of ws_place);
  c. the stem and the tail below one round, between one and two, and at two or more; the tail with one segment per strip, with several, and with a
     ragged last segment;
  d. no case is idle: dropping any one leaves a requirement unmet.
The cases were found by a greedy cover over N <= 129, H and W multiples of 16 up to 256 and at most 100 x 256 x 256 pixels, cheapest first
(pixels + 25 x float64 pixels), then reduced until (d) held.

The bound tells a defect (e): on the three distinct images at 144 x 208 (a batch of six copies), a float32 numpy evaluation of the specified arithmetic
stands in for the engine and passes every launch with no element outside the half-ulp grade; each planted defect -- folded weights not rounded to bf16,
one zeroed tap, the input shifted by a pixel, truncation instead of round-to-nearest-even on the store -- fails the grade at every launch it touches;
one 2 x 32 tile of a slice >= 3 left at the poison pattern, or taken from the neighbouring copy, fails the copy identity at every stored map; and
channels 16..31 of the zero-padded up0_0 (UNet-LSTM_ao on 401: 16 real channels on the 32-row MFMA) stored non-zero land on the next image's plane of
the channel-blocked map and fail the grade or the copy identity."""
import collections
import os
import re

import numpy as np
import pytest

import launch_grading as G
import test_bf16_launches_gpu as L
from oracle import fcn_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = G.CUS
BENCH = [(100, 256, 256), (100, 192, 208)]
WS_TILINGS = (400, 401, 402, 410, 411, 422)
BELOW = {'between': 'below', 'two+ ragged': 'between', 'two+ exact': 'between'}


def source(name):
    with open(os.path.join(ROOT, 'ukbb_cardiac_amd', 'csrc', name)) as f:
        return f.read()


def plan(n, H, W, model='UNet_ao'):
    from ukbb_cardiac_amd import engine
    from ukbb_cardiac_amd.arch import MODELS
    return engine.plan_layout(MODELS[model], 'bf16', n, H, W, CUS)


def reached(n, H, W):
    """Everything one case reaches: ('combo', layer, tiling, fit), ('ws', layer, tiling, order, class), ('tiling', id, situation), ('stem' | 'tail', state)."""
    p = plan(n, H, W)
    out = set()
    for o in p['ops']:
        if o['kind'] == 'logits':
            continue
        cfg = o['cfg'] if o['kind'] in ('conv', 'tconv') else -1
        # a tile-per-workgroup tiling 'div' | 'nodiv' (G.fit_of's 'ragged' and 'partial' taken together), None for the walkers and the fused launches
        out.add(('combo', o['name'], cfg, None if not 0 <= cfg < 400 else 'div' if G.fit_of(o) == 'div' else 'nodiv'))
        if o['kind'] == 'stem':
            out.add(('stem', G.stem_launch(n, H, W)['cls'].split(' ')[0]))
        elif o['kind'] == 'tail':
            t = G.tail_launch(n, H, W)
            out.add(('tail', t['cls'].split(' ')[0]))
            out.add(('tail', 'one segment per strip' if t['segs'] == 1 else 'several segments per strip'))
            if t['ragged']:
                out.add(('tail', 'ragged last segment'))
        elif cfg >= 400:
            w = G.ws_launch(o, p['acts'], n)
            out.add(('ws', o['name'], cfg, w['order'], w['cls']))
            for s in (w['cls'], w['order'], w['cols'], w['place']):
                out.add(('tiling', cfg, s))
    return out


@pytest.fixture(scope='module')
def recorded():
    """{(layer, tiling): set of fits} over the recorded default bf16 plans of UNet_ao (G.replay_records)."""
    assert not [k for k in G.LAUNCHER_KNOBS if k in os.environ], 'the launchers\' own knobs change the situations counted here'
    rec = collections.defaultdict(set)
    for _, _, _, got in G.replay_records('UNet_ao', 'bf16', reached):
        for k in got:
            if k[0] == 'combo':
                rec[k[1:3]].add(k[3])
    return dict(rec)


def requirements(rec):
    want = {('combo',) + k for k in rec}
    both_orders = collections.defaultdict(set)
    for c in BENCH:
        for k in reached(*c):
            if k[0] == 'ws':
                _, layer, cfg, order, cls = k
                want.add(k)
                if cls != 'below':
                    want.add(('ws', layer, cfg, order, BELOW[cls]))
                both_orders[cfg].add(order)
    for cfg in WS_TILINGS:
        for s in ('below', 'between', 'two+ exact', 'two+ ragged', 'whole columns', 'ragged columns', 'grid 8 nG', 'grid not 8 nG') + tuple(sorted(both_orders[cfg])):
            if not (cfg == 422 and s.startswith('two+')):
                want.add(('tiling', cfg, s))
    want |= {(k, s) for k in ('stem', 'tail') for s in ('below', 'between', 'two+')}
    want |= {('tail', s) for s in ('one segment per strip', 'several segments per strip', 'ragged last segment')}
    return want


def covered(cases, rec):
    got = set()
    for c in cases:
        for k in reached(*c):
            if k[0] == 'combo':
                if k[1:3] in rec and k[3] in rec[k[1:3]]:
                    got.add(k[:3])
            else:
                got.add(k)
    return got


# ---- the launchers hold what L's arithmetic assumes ------------------------------------------------------------------------------------------------
def test_launcher_constants_are_the_ones_assumed():
    ws, stem, tail = source('kernels_ws.hip'), source('kernels_stem.hip'), source('kernels_tail.hip')
    assert int(re.search(r'constexpr int WS_TW = (\d+);', ws).group(1)) == G.WS_TW
    # rows / cb / waves of each tiling: the registry macros against the names ws_shape reads them from
    reg = {int(m.group(1)): m.group(2) for m in re.finditer(r'^    ([WST])\((4\d\d), (\d+)(?:, (\d+))?, (\d+)\)', ws, re.M) for m in [re.match(r'(?s).*\((4\d\d), (.*)\)', m.group(0))]}
    for cfg in WS_TILINGS:
        R, cb, wn, transposed = G.ws_shape(cfg)
        assert reg[cfg] == ('%d, %d' % (R, wn) if transposed else '%d, %d, %d' % (R, cb, wn)), (cfg, reg[cfg])
        assert not transposed or cb == 2
    assert {c for c in WS_TILINGS if G.ws_shape(c)[3]} == {410, 411} and 'convBF16wr' in G.config_name(422)
    lw = ws[ws.index('hipError_t launch_conv_ws('):]
    assert 'a.tiles_y = (a.Ho + c->th - 1) / c->th; a.tiles_x = (a.Wo + WS_TW - 1) / WS_TW;' in lw
    assert 'a.xcd_local = force ? atoi(force) : ((long long)a.H * a.W >= 128ll * 128);' in lw
    assert 'const int nG = a.Cout / (32 * c->cb);' in lw and 'const long long ntiles = (long long)a.N * a.tiles_y * a.tiles_x;' in lw
    assert 'long long want = ((ntiles + c->wn - 1) / c->wn) * nG;' in lw
    assert 'int grid = cus >= 8 * nG ? cus / (8 * nG) * (8 * nG) : cus / nG * nG;' in lw and 'if (grid < nG) grid = nG;' in lw
    assert 'if (want < grid) grid = (int)((want + nG - 1) / nG * nG);' in lw
    assert 'a.Cout != 4 * a.up2' in lw and 'a.Ho != a.H || a.Wo != a.W' in lw           # transposed: 4 x up2 virtual channels; every walker walks its input map
    # the walkers: tile t of a round on worker t, nworkers = workgroups per group x waves, in both orders; the two placements
    assert ws.count('const int worker = a.xcd_local ? chunk_ * NW + wave : wave * nwalk + walker, nworkers = nwalk * NW;') == 2
    assert ws.count('const int t = valid ? worker + k * nworkers : 0;') == 2
    assert 'if ((int)gridDim.x % (8 * nG) == 0) {' in ws and 'nwalk = (int)gridDim.x / nG;' in ws
    assert 'ws_place(a.Cout / (32 * CB), grp, walker, nwalk);' in ws and 'ws_place(a.Cout / 64, grp, walker, nwalk);' in ws
    # stem: 8 rows x 30 columns per tile, 4 waves, at most two workgroups per CU
    assert 'constexpr int ST_TW = %d,' % G.STEM_TW in stem and 'constexpr int R = %d, NW = %d;' % (G.STEM_R, G.STEM_NW) in stem
    ls = stem[stem.index('hipError_t launch_unet_stem('):]
    assert 'const long long ntiles = (long long)a.N * ((a.H + R - 1) / R) * ((a.W + ST_TW - 1) / ST_TW);' in ls and 'const long long want = (ntiles + NW - 1) / NW;' in ls
    assert 'const long long cap = (long long)cus * %d;' % G.STEM_WG_PER_CU in ls and 'const int grid = (int)(want < cap ? want : cap);' in ls
    # tail: 8 rows x 14 columns per tile, 8 waves, one workgroup per CU; segments per strip
    assert 'constexpr int R = %d, NW = %d, NB = 1;' % (G.TAIL_R, G.TAIL_NW) in tail and 'constexpr int tl_tw(int nb) { return 16 * nb - 2; }' in tail and G.TAIL_TW == 16 * 1 - 2
    lt = tail[tail.index('hipError_t launch_unet_tail('):]
    assert 'const long long ntiles = (long long)a.N * ((a.H + R - 1) / R) * ((a.W + TL_TW - 1) / TL_TW);' in lt
    assert 'const long long want = (ntiles + NW - 1) / NW;' in lt and 'const int grid = (int)(want < cus ? want : cus);' in lt
    assert 'const bool strips = !es || atoi(es) != 0;' in lt
    for line in ('for (int segs = 1; segs <= tiles_y; ++segs) {', 'const int seg = (tiles_y + segs - 1) / segs;', 'if ((tiles_y + seg - 1) / seg != segs) continue;',
                 'const long long units = nstrips * segs, cost = (units + workers - 1) / workers * seg;', 'if (best < 0 || cost < best) { best = cost; best_seg = seg; }',
                 'const long long nstrips = (long long)a.N * tiles_x, workers = (long long)grid * NW;'):
        assert line in lt, line


def test_launch_arithmetic_on_the_figures_the_benchmark_batches_give():
    """12800 tiles on 1024 workers, 6400 on 2048, 1600 on 512 at 100 x 256 x 256; one-tile-per-wave launches at 1 x 256 x 256."""
    p = plan(100, 256, 256)
    w = {o['name']: G.ws_launch(o, p['acts'], 100) for o in p['ops'] if o['kind'] in ('conv', 'tconv') and o['cfg'] >= 400}
    assert (w['conv1_1']['ntiles'], w['conv1_1']['nworkers']) == (12800, 1024) and (w['conv2_1']['ntiles'], w['conv2_1']['nworkers']) == (6400, 2048)
    assert (w['conv3_1']['ntiles'], w['conv3_1']['nworkers']) == (1600, 512) and len(w) == 12
    assert {v['cls'] for k, v in w.items() if k != 'up3_0'} == {'two+ ragged'} and w['up3_0']['cls'] == 'between'
    p = plan(1, 256, 256)
    w = [G.ws_launch(o, p['acts'], 1) for o in p['ops'] if o['kind'] in ('conv', 'tconv') and o['cfg'] >= 400]
    assert len(w) == 12 and all(v['ntiles'] == v['nworkers'] and v['cols'] == 'whole columns' for v in w)
    assert sorted({(v['ntiles'], v['nworkers']) for v in w}) == [(16, 16), (64, 64), (128, 128)]
    assert G.stem_launch(100, 256, 256)['cls'] == 'two+ ragged' and G.tail_launch(100, 256, 256)['cls'] == 'two+ ragged'


# ---- (a) - (d) ---------------------------------------------------------------------------------------------------------------------------------------
def test_cases_reach_every_recorded_combination(recorded):
    assert len(recorded) == 61
    assert len(set(L.CASES)) == len(L.CASES) and all(H % 16 == 0 and W % 16 == 0 and n <= 129 and n * H * W <= 100 * 256 * 256 for n, H, W in L.CASES)
    assert not set(L.CASES) & set(BENCH), 'the smallest case that reaches a situation, not the workload\'s own sizes'
    missing = {('combo',) + k for k in recorded} - covered(L.CASES, recorded)
    assert not missing, sorted(missing, key=str)
    # the fifteen combinations the three shapes of tests/test_bf16_layers_gpu.py do not reach are among them
    old = covered([(1, 256, 256), (3, 64, 96), (2, 48, 16)], recorded)
    assert len({k for k in old if k[0] == 'combo'}) == 46


def test_cases_reach_every_walker_situation(recorded):
    want = {r for r in requirements(recorded) if r[0] != 'combo'}
    # 12 weight-stationary launches: the four on 128 x 128 / 96 x 104 maps (401, 410) in both orders, the seven of levels 2-3 wave-major, each
    # 'two+ ragged' and 'between'; up3_0 on 422 'between' and 'below'
    assert len([r for r in want if r[0] == 'ws']) == 4 * 2 * 2 + 7 * 2 + 2 and len(requirements(recorded)) == 156
    got = covered(L.CASES, recorded)
    assert not want - got, sorted(want - got, key=str)
    # what the three shapes of tests/test_bf16_layers_gpu.py reach of it: one tile per wave only
    old = covered([(1, 256, 256), (3, 64, 96), (2, 48, 16)], recorded)
    assert {k[4] for k in old if k[0] == 'ws'} == {'below'} and {k[1] for k in old if k[0] in ('stem', 'tail')} <= {'below', 'one segment per strip', 'several segments per strip', 'ragged last segment'}


def test_no_case_is_idle(recorded):
    only = G.no_case_is_idle(L.CASES, lambda c: covered([c], recorded), requirements(recorded))
    for c, mine in zip(L.CASES, only):
        print('%-16s %8d pixels; only it reaches %s' % (c, c[0] * c[1] * c[2], mine))
    assert sum(n * H * W for n, H, W in L.CASES) == 10680064 and sum(min(n, 3) * H * W for n, H, W in L.CASES) == 633344     # the docstring's table


def test_sequence_cases_plan_the_up0_tilings_named():
    got = set()
    for N, H, W, cfg0, cfg1 in L.SEQ_CASES:
        p = plan(9 * N, H, W, 'UNet-LSTM_ao')
        ops = {o['name']: o for o in p['ops']}
        assert (ops['up0_0']['cfg'], ops['up0_1']['cfg']) == (cfg0, cfg1) and p['acts'][ops['up0_0']['out']]['channels'] == 16
        assert {'conv0', 'up0_t', 'up0_0', 'up0'} <= {a['name'] for a in p['acts']}
        if cfg0 == 401:
            w = G.ws_launch(ops['up0_0'], p['acts'], 9 * N)
            assert w['nG'] == 1 and w['grid'] > 1                      # 16 channels padded to one 32-row group; more than one workgroup
            got.add((cfg0, cfg1, w['cols']))
        else:
            got.add((cfg0, cfg1))
    assert got == {(232, 232), (401, 236, 'whole columns'), (401, 236, 'ragged columns')}


def test_graph_lists_every_planned_launch():
    """launches() of tests/launch_grading.py names exactly the launches of the bf16 plans, and every map grade_unet fetches is stored."""
    from ukbb_cardiac_amd.arch import MODELS
    for n, H, W in L.CASES:
        p = plan(n, H, W)
        planned = [part for o in p['ops'] for part in o['name'].split('+')]
        graph = G.launches(MODELS['UNet_ao'])
        assert planned == [g[0] for g in graph], (planned, graph)
        assert [o['kind'] for o in p['ops'] if '+' in o['name']] == ['stem', 'tail']
        stored = {a['name'] for a in p['acts']}
        assert {g[1] for g in graph if g[0] not in ('conv0_0', 'up0_0', 'up0_1', 'logits')} <= stored


# ---- (e) the bound tells a defect ----------------------------------------------------------------------------------------------------------------------
H, W = 144, 208
DEFECTS = ('folded weights not rounded to bf16', 'one zeroed tap', 'input shifted by a pixel', 'truncation on the store')


def launch32(x, p, stride=1, transposed=False, relu=True, defect=None, round_w=True):
    """One launch as the engine is specified to run it, in float32 numpy, storing bf16 -- with one planted defect, if any."""
    w, b = G.fold(p, transposed)
    if round_w and defect != DEFECTS[0]:
        w = G.bf16_round(w)
    if defect == DEFECTS[1]:
        w = w.copy()
        w[0, 2] = 0
    x = np.asarray(x, np.float32)
    if defect == DEFECTS[2]:
        x = np.concatenate([np.zeros_like(x[:, :, :1]), x[:, :, :-1]], axis=2)
    y = (O.conv2d_transpose_same(x, w, stride) if transposed else O.conv2d_same(x, w, stride)) + b
    assert y.dtype == np.float32
    if relu:
        y = np.maximum(y, np.float32(0))
    if defect == DEFECTS[3]:
        return (np.ascontiguousarray(y).view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    return G.bf16_round(y)


def logits32(a, params):
    pl = params['logits']
    lg = O.conv2d_same(a, pl['kernel'].astype(np.float32), 1) + pl['bias'].astype(np.float32)
    assert lg.dtype == np.float32
    return lg, np.argmax(lg, -1)


def fails(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except AssertionError:
        return True
    return False


@pytest.fixture(scope='module')
def stand_in():
    """The float32 stand-in's stored maps of the three distinct images at 144 x 208 (the whole bf16 rounding model), graded launch by launch exactly as
    the GPU test grades the engine; and per launch the grade of the same launch with each planted defect.  Returns (stored, logits, pred, rows)."""
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.weights import synthetic_params
    arch = MODELS['UNet_ao']
    params = synthetic_params(arch, G.SEEDS[0])
    img, nd = G.normalised_copies(0, 6, H, W)
    img = img[:nd]
    stored, rows = {}, []
    for lname, sname, l, srcs, stride, transposed, relu in G.launches(arch):
        if lname in ('conv0_0', 'up0_0', 'up0_1', 'logits'):
            continue
        if lname == 'conv0_1':                                            # the stem as a unit; the defect sits in its second layer
            a00 = launch32(G.bf16_round(img), params['conv0_0'])
            ex, slack, n_amb = L.stem_reference(img, params, 'stem')
            sc = float(np.abs(ex).max())
            stored[sname] = launch32(a00, params[lname])
            L.grade_stem(stored[sname], ex, sc, slack)
            rows.append((lname, G.measure(stored[sname], ex, sc)[0], {d: fails(L.grade_stem, launch32(a00, params[lname], defect=d), ex, sc, slack) for d in DEFECTS}))
            continue
        x = np.concatenate([stored[s] for s in srcs], axis=-1)
        ex = G.layer(x, params[lname], stride, transposed, relu, round_w=True)
        sc = float(np.abs(ex).max())
        stored[sname] = launch32(x, params[lname], stride, transposed, relu)
        share = G.grade(lname, stored[sname], ex, sc, ulps=0.5, fraction=1.0)
        rows.append((lname, share, {d: fails(G.grade, lname, launch32(x, params[lname], stride, transposed, relu, defect=d), ex, sc, ulps=0.5, fraction=1.0) for d in DEFECTS}))
    x = np.concatenate([stored['conv0'], stored['up0_t']], axis=-1)       # the tail as a unit; the defect sits in up0_1
    ex = L.tail_reference(x, params)
    a = launch32(x, params['up0_0'])
    logits, pred = logits32(launch32(a, params['up0_1']), params)
    L.grade_tail(logits, pred, ex)
    rows.append(('up0_0+up0_1+logits', 1.0, {d: fails(L.grade_tail, *logits32(launch32(a, params['up0_1'], defect=d), params), ex) for d in DEFECTS}))
    return stored, logits, pred, rows


def test_float32_stand_in_passes_every_launch(stand_in):
    """Every element of every single launch inside the half-ulp grade (the share a boundary rule would be capped by is 0), the stem and the tail
    inside their figures."""
    stored, logits, pred, rows = stand_in
    assert len(rows) == 20 and sum(v.size for v in stored.values()) > 9e6           # 18 single launches, the stem and the tail: 21 layers and the logits
    for lname, share, _ in rows:
        print('stand-in %-20s share within half an ulp %.7f' % (lname, share))
        assert share == 1.0 or lname == 'conv0_1', (lname, share)
    for k, v in stored.items():
        G.check_bf16(k, v)


def test_each_planted_arithmetic_defect_fails_at_every_launch(stand_in):
    rows = stand_in[3]
    for lname, _, caught in rows:
        print('%-20s %s' % (lname, caught))
        assert set(caught) == set(DEFECTS) and all(caught.values()), (lname, caught)


def test_a_lost_or_misdirected_tile_breaks_the_copy_identity(stand_in):
    """One 2 x 32 tile of slice 4 of a batch of six copies left at the poison pattern, or taken from the neighbouring copy (another image): every
    stored map and the logits; the unchanged batch passes."""
    stored, logits, pred, _ = stand_in
    nan = np.array([int(G.POISON, 16) & 0xffff0000], np.uint32).view(np.float32)[0]
    assert np.isnan(nan) and np.isnan(np.array([int(G.POISON, 16)], np.uint32).view(np.float32)[0])
    for name, a in list(stored.items()) + [('logits', logits)]:
        six = np.concatenate([a, a])
        G.check_copies(name, six, 3)
        tile = (4, slice(2, 4), slice(0, 32))
        for what, value in (('poison', nan), ('neighbouring copy', six[5][tile[1:]])):
            bad = six.copy()
            assert not np.array_equal(bad[tile], value)
            bad[tile] = value
            assert fails(G.check_copies, name, bad, 3), (name, what)
    labels = np.concatenate([pred, pred])
    G.check_copies('pred', labels, 3)
    labels[4, 2:4, :32] = labels[5, 2:4, :32] + 1
    assert fails(G.check_copies, 'pred', labels, 3)


def test_nonzero_padding_channels_of_up0_0_are_caught():
    """up0_0 of UNet-LSTM_ao on 401: 16 real output channels on one 32-row MFMA group whose rows 16..31 are zero weights, never stored
    (cout_store = 16).  If they were stored they would be channel block 1 of image n, which in the channel-blocked map [N][C/16][H][W][16] with
    C = 16 is the plane of image n + 1.  Planted: rows 16..31 hold a non-zero filter and land on the next image in every second 4-row tile."""
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.weights import synthetic_params
    params = synthetic_params(MODELS['UNet-LSTM_ao'], G.SEEDS[0])
    rng = np.random.default_rng(3)
    three = G.bf16_round(np.maximum(rng.standard_normal((3, 16, 64, 32)), 0.0).astype(np.float32))
    x = np.concatenate([three, three])
    ex = G.layer(x[:3], params['up0_0'], round_w=True)
    sc = float(np.abs(ex).max())
    clean = launch32(x, params['up0_0'])
    assert G.grade('up0_0', clean[:3], ex, sc, ulps=0.5, fraction=1.0) == 1.0
    G.check_copies('up0_0', clean, 3)
    pad = dict(params['up0_0'])
    pad['kernel'] = pad['kernel'][..., ::-1]
    spilled = launch32(x, pad)
    assert spilled.max() > 0
    bad = clean.copy()
    for n in range(5):
        for y0 in range(4, 16, 8):
            bad[n + 1, y0:y0 + 4] = spilled[n, y0:y0 + 4]
    assert fails(G.grade, 'up0_0', bad[:3], ex, sc, ulps=0.5, fraction=1.0) and fails(G.check_copies, 'up0_0', bad, 3)
