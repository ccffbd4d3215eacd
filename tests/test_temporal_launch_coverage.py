"""What tests/test_temporal_launches_gpu.py covers, checked without a GPU (engine.plan_layout: the host-only planner), and that its bound can tell a
wrong launch from a right one.

Every 3x3x3 unit of the Temporal-UNet but the first runs on conv3d_kernel<CB> (kernels_conv3d.hip): one wave = one ITEM = 32 pixels of one frame x
32 CB output channels, item -> (channel group, pixel tile, frame), four items per workgroup.  A launch's SITUATION is computed here from the plan op's
map and a mirror of launch_conv3d's arithmetic (launch_grading.conv3d_launch; its constants and lines are read from the source and asserted):

    kind      stride-1, stride-2, two-source (skip concat) or transposed (4 sub-pixel phases over the INPUT map)
    CB        2 where the padded channel count is a multiple of 64, else 1; and the number of channel groups (CB 1: 1, 3, 5 on the 'wide' architecture)
    padded    Cout < Cout_pad (16 channels on the 32-row MFMA: level 0) or not
    fit       the map's pixels in 32-pixel tiles: divides / whole tiles and a partial one / one partial tile / a single pixel
    idle      items % 4: the waves of the last workgroup that return at once
    T         windows of 1 frame (only the middle time tap runs), of 3 (every frame but one at a window edge), of 5 or more
    windows   one, or several (a window edge inside the batch)

The full cross product is not reachable by a dozen small cases; SITUATIONS counted per launch are, for its (kind, CB): (fit, T), (idle, windows),
(T, windows), the number of channel groups, and per kind whether the channels are padded; for the first layer (T, windows); for the logits launch the
class count.  SEARCHED: the four architectures of the GPU file (the default one; windows of 3 frames with 2 classes; windows of 1 frame with 4
classes; n_filter (16, 32, 96, 160, 96) with a three-block level) x 1, 2, 4, 5 windows x the maps 16 x 16 (a 1 x 1 deepest map, up3_t from a single
pixel), 16 x 48 and 48 x 16 (asymmetric: a deepest map of one partial tile), 32 x 48, 48 x 48 (12 x 12 at level 2: whole tiles and a partial one) and
48 x 80.  CASES reaches every situation any searched case holds, and dropping any one case leaves some situation unreached.

The bound tells a defect: at 2 windows x 3 frames x 16 x 32 a float32 numpy evaluation of the graph stands in for the engine and passes every launch
at 1e-5 of the layer's scale; each planted defect -- transposed time taps not reversed, a window-edge tap taken from the neighbouring window instead
of skipped, [up, skip] instead of [skip, up], one zeroed tap, the input shifted by a pixel -- fails the bound at every launch it touches and nowhere
else (every launch is graded on its own stored input)."""
import os
import re

import numpy as np
import pytest

import launch_grading as G
import temporal_unet_ref as R
import test_temporal_launches_gpu as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS = (1, 2, 4, 5)
MAPS = ((16, 16), (16, 48), (48, 16), (32, 48), (48, 48), (48, 80))


def plan(key, N, H, W):
    from ukbb_cardiac_amd import engine
    arch = L.arch_of(key)
    return arch, engine.plan_layout(arch, 'fp32', N * arch.fc, H, W, G.CUS)


def reached(case):
    key, N, H, W = case
    arch, p = plan(key, N, H, W)
    T = arch.fc
    out = set()
    for o in p['ops']:
        if o['kind'] in ('conv3d', 'tconv3d'):
            d = G.conv3d_launch(o, p['acts'], N * T, T)
            k = (d['kind'], d['cb'])
            out |= {('fit',) + k + (d['fit'], d['T']), ('idle',) + k + (d['idle'], d['windows']), ('T',) + k + (d['T'], d['windows']),
                    ('groups',) + k + (d['cgroups'],), ('padded', d['kind'], d['padded'])}
        elif o['kind'] == 'first3d':
            d = G.conv3d_launch(dict(o, kind='conv3d'), p['acts'], N * T, T)
            out.add(('first', d['T'], d['windows']))
        else:
            assert o['kind'] == 'logits', o
            out.add(('logits', arch.n_class))
    return out


@pytest.fixture(scope='module')
def searched():
    return {c: reached(c) for c in [(key, N, H, W) for key in L.ARCH_CHANGES for N in WINDOWS for H, W in MAPS]}


def test_launcher_lines_are_the_ones_mirrored():
    with open(os.path.join(ROOT, 'ukbb_cardiac_amd', 'csrc', 'kernels_conv3d.hip')) as f:
        src = f.read()
    assert G.grid_caps_3d() == (256 * 64 * 256, 256 * 16 * 256)
    body = re.search(r'hipError_t launch_conv3d\(.*?\n}\n', src, re.S).group(0)
    assert 'const int cb = a.Cout_pad %% %d == 0 ? 2 : 1;' % (2 * G.C3D_COB) in body
    assert 'const long long items = (long long)a.N * ((a.Hg * a.Wg + %d) / %d) * (a.Cout_pad / %d / cb);' % (G.C3D_PIX - 1, G.C3D_PIX, G.C3D_COB) in body
    assert 'const long long blocks = (items + %d) / %d;' % (G.C3D_WAVES - 1, G.C3D_WAVES) in body and 'dim3 g((unsigned)blocks, (unsigned)a.nph), t(256)' in body
    kern = re.search(r'void conv3d_kernel\(.*?\n}\n', src, re.S).group(0)
    assert 'ptiles = (npix + 31) / 32, ncob = a.Cout_pad / 32, cgroups = ncob / CB;' in kern
    assert 'const long long item = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);' in kern
    assert 'if (item >= (long long)a.N * ptiles * cgroups) return;' in kern
    # the engine hands launch_conv3d the map the mirror takes: the output map of a conv, the INPUT map of a transposed conv
    with open(os.path.join(ROOT, 'ukbb_cardiac_amd', 'csrc', 'engine.cpp')) as f:
        eng = f.read()
    assert 'ca.Hg = op.Ho; ca.Wg = op.Wo; ca.stride = op.stride;' in eng and 'ca.Hg = op.H; ca.Wg = op.W; ca.stride = 1; ca.up = 2;' in eng
    assert 'ca.Cout = L.cout; ca.Cout_pad = round_up(L.cout, 32);' in eng


def test_the_architectures_are_accepted_and_span_the_windows_and_class_counts():
    archs = {k: L.arch_of(k) for k in L.ARCH_CHANGES}
    assert {a.fc for a in archs.values()} == {1, 3, 9} and {a.n_class for a in archs.values()} == {2, 3, 4}
    assert archs['wide'].n_filter == (16, 32, 96, 160, 96) and archs['wide'].n_block == (2, 2, 3, 2, 2)
    assert {c[0] for c in L.CASES} == set(archs) and {c[0] for c in L.SMALL_CINES} == {'fc3c2', 'fc1c4'}
    _, p = plan('wide', 1, 16, 48)
    by = {o['name']: G.conv3d_launch(o, p['acts'], 9, 9) for o in p['ops'] if o['kind'] in ('conv3d', 'tconv3d')}
    assert {(d['cb'], d['cgroups']) for d in by.values()} >= {(1, 1), (1, 3), (1, 5)}       # conv3d_kernel<1> with odd group counts above level 1
    assert by['up2_0']['kind'] == 'two-source' and (by['up2_0']['cb'], by['up2_0']['cgroups']) == (1, 3)        # 96 + 96 channels in
    assert by['conv2_2']['kind'] == 'stride-1' and 'up2_2' in by and 'conv3_2' not in by                     # the three-block level


def test_launches_names_the_plans_launches_and_stored_maps():
    for key in L.ARCH_CHANGES:
        arch, p = plan(key, 2, 32, 48)
        graph = G.launches(arch)
        assert [g[0] for g in graph] == [o['name'] for o in p['ops']]
        stored = {a['name']: a for a in p['acts']}
        for lname, sname, l, srcs, stride, transposed, relu in graph[:-1]:
            o = [o for o in p['ops'] if o['name'] == lname][0]
            assert stored[sname]['per_image'] == (32 >> l) * (48 >> l) * arch.n_filter[l] and p['acts'][o['out']]['name'] == sname
            assert [p['acts'][i]['name'] for i in (o['in0'], o['in1']) if i >= 0] == [s for s in srcs if s]
            assert (o['kind'] == 'tconv3d') == transposed and (o['stride'] == 2) == (stride == 2 and not transposed)


def test_cases_reach_every_searched_situation_and_none_is_idle(searched):
    assert len(set(L.CASES)) == len(L.CASES) and set(L.CASES) <= set(searched)
    want = set().union(*searched.values())
    only = G.no_case_is_idle(L.CASES, searched.__getitem__, want)
    for c, mine in zip(L.CASES, only):
        print('temporal-coverage %-7s %d x %2d x %2d alone reaches %d of %d situations, e.g. %s' % (c + (len(mine), len(want), mine[0])))
    # what the list must hold whatever the search finds: the shapes, window counts and seeds the grader's docstring names
    assert {(H, W) for _, _, H, W in L.CASES} >= {(16, 16), (16, 48), (32, 48), (48, 48)}
    assert {N for _, N, _, _ in L.CASES} >= {1, 2, 5}
    assert {k[3] for k in want if k[0] == 'fit'} == {'divides', 'whole tiles and a partial one', 'one partial tile', 'single pixel'}
    assert {k[3] for k in want if k[0] == 'idle'} == {0, 1, 2, 3} and {k[3] for k in want if k[0] == 'groups' and k[2] == 1} == {1, 3, 5}
    assert {k[1] for k in want if k[0] == 'logits'} == {2, 3, 4} and {k[1] for k in want if k[0] == 'first'} == {'T=1', 'T=3', 'T>=5'}
    # graded maps stay small: at most 48 x 80 and 9 frames
    assert all(H * W <= 48 * 80 and L.arch_of(k).fc <= 9 for k, _, H, W in L.CASES)


def test_the_full_size_cases_wrap_the_loops_they_are_meant_to():
    first_cap, tile_cap = G.grid_caps_3d()
    N, H, W = L.FULL_SEQ
    assert first_cap < N * 9 * H * W < 2 * first_cap and (N * 9 * H * W) % first_cap and 3 * 9 * H * W <= first_cap
    F, H, W = L.FULL_CINE
    from ukbb_cardiac_amd import engine
    cw = engine.cine_chunk_windows(L.arch_of('default'), 'fp32', F, H, W, 1)
    assert tile_cap < F * H * W and first_cap < cw * 9 * H * W and 1 < -(-F // cw)
    for key, F, H, W, step in L.SMALL_CINES:
        T = L.arch_of(key).fc
        assert step > T and F > step                                      # frames no window reaches, more than one window


# ---- the bound tells a defect -----------------------------------------------------------------------------------------------------------------------
DEFECTS = ('tconv taps not reversed', 'edge tap from the neighbouring window', 'up before skip', 'one zeroed tap', 'input shifted by a pixel')


def stand_in(x, params, graph, defect=None):
    """The graph in float32 numpy (the engine's folded float32 weights, float32 accumulation), every launch on the stand-in's own stored input.
    Returns {stored name: map}."""
    stored = {}
    for lname, sname, l, srcs, stride, transposed, relu in graph:
        srcs = srcs[::-1] if defect == 'up before skip' else srcs
        xin = x if srcs == [''] else np.concatenate([stored[s] for s in srcs], axis=-1)
        w, b = G.fold(params[lname], transposed)
        if w.shape[0] == 3:                                              # the 3x3x3 units; the 1x1x1 logits conv has no taps to plant these in
            if defect == 'tconv taps not reversed' and transposed:
                w = w[::-1]
            if defect == 'one zeroed tap':
                w = w.copy()
                w[1, 1, 1] = 0
            if defect == 'input shifted by a pixel':
                xin = np.roll(xin, 1, axis=3)
        n, t = xin.shape[:2]
        if defect == 'edge tap from the neighbouring window' and w.shape[0] == 3:
            xin = xin.reshape((1, n * t) + xin.shape[2:])                # the windows end to end: only the batch's two ends see the zero frame
        xin = np.ascontiguousarray(xin, np.float32)
        y = R.conv3d_transpose_same(xin, w, stride) if transposed else R.conv3d_same(xin, w, stride)
        assert y.dtype == np.float32
        y = y.reshape((n, t) + y.shape[2:]) + b
        stored[sname] = np.maximum(y, np.float32(0)) if relu else y
    return stored


def failing(x, params, graph, stored):
    out = set()
    for lname, sname, l, srcs, stride, transposed, relu in graph:
        xin = x if srcs == [''] else np.concatenate([stored[s] for s in srcs], axis=-1)
        err, _ = G.rel_err(stored[sname], G.layer3d(xin, params[lname], stride, transposed, relu))
        if not err <= L.BOUND:
            out.add(lname)
    return out


def test_the_bound_tells_planted_defects():
    from ukbb_cardiac_amd.weights import synthetic_params
    arch = L.arch_of('fc3c2')
    params = synthetic_params(arch, G.SEEDS[0])
    graph = G.launches(arch)
    x, nd = G.window_batch(0, 2, arch.fc, 16, 32)
    assert nd == 2
    assert failing(x, params, graph, stand_in(x, params, graph)) == set()
    units = {g[0] for g in graph if g[0] != 'logits'}
    touched = {'tconv taps not reversed': {g[0] for g in graph if g[5]}, 'edge tap from the neighbouring window': units,
               'up before skip': {g[0] for g in graph if len(g[3]) == 2}, 'one zeroed tap': units, 'input shifted by a pixel': units}
    assert set(touched) == set(DEFECTS) and all(touched.values())
    for defect in DEFECTS:
        assert failing(x, params, graph, stand_in(x, params, graph, defect)) == touched[defect], defect
