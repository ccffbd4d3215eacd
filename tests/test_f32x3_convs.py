"""ukbb_fcn_set_f32x3_convs without a GPU: the interface (C export, Engine method, plan_layout keyword, deploy_network.py flag), the plan the switch
makes (engine.plan_layout on the host-only planner, 256 compute units), the numpy model of the three-piece launch against the two grades and against
planted defects, the constant R of tests/f32x3_convs_grading.py, and what the cases of tests/test_f32x3_convs_launches_gpu.py reach.

The plan.  With the switch on under 'f32x3' an FCN plan is the f32x3 plan -- ops, maps, split range -- except for the tilings of the eleven layers
conv1_0 .. conv4_2, which all come from ConvFamily::F32x3Operands (330-345: eight tilings); it does not depend on the batch.  With the switch off, under any other
precision, and on every other kind (where the handle call and the debug export refuse with UKBB_EARCH) plan_layout gives what it gave before.

The model and R.  On the three rough images at 32 x 48, the eleven layers each fed by the layer before (weights of seeds 1234 and 7), the numpy model
x3_launch passes grade 1 (every element within 1e-5 of the scale) and grade 2 (RMS error <= R x the fp32 model's) at every layer, and each planted
defect -- each single term dropped, the l pieces absent, h.h only, the activations left as one piece, a zeroed tap, a one-pixel shift -- misses at
least one grade at every layer.  Per layer the worst ratio of the correct model, the mildest defect's ratio and R are printed and held against the
section of profiles/f32x3_convs.txt that records them (rewritten only with UKBB_F32X3_WRITE_PROFILE=1 in the environment).  Measured: correct 1.92 .. 2.59,
mildest defect (h.l, l.h or m.m dropped) 12.9 .. 40, R = 5.79 a factor 2.24 from either side; grade 1 alone sees none of those three (2e-6 .. 5e-6).

Coverage.  The chooser (plan.cpp choose_x3_cfg) takes the tiling that issues the fewest 32-pixel blocks, so over the legal shapes it puts every one
of the eight tilings on maps its tiles divide, on ragged edge tiles and on single partial tiles (launch_grading.fit_of) -- 12 x 13 and 11 x 13 too, e.g.
on the 12 x 20 level 2 of a 48 x 80 input.  The requirements are those 8 x 3 fits at both batch classes (up to plan.h SMALL_BATCH, above it) and the 92
(layer, tiling, fit, batch class) situations of the switch-on plans at the recorded shapes of tests/golden/plan_layouts.json: 140.  CASES of
tests/f32x3_convs_grading.py reach every one, and no case added to the six specified shapes is idle."""
import json
import os
import re

import numpy as np
import pytest

import f32x3_convs_grading as X
import launch_grading as G

ROOT = G.ROOT
FCN_MODELS = ('FCN_sa', 'FCN_la_2ch', 'FCN_la_4ch', 'FCN_la_4ch_seg4')
UNET_KINDS = ('UNet_ao', 'UNet-LSTM_ao', 'Temporal-UNet_ao')
PLAN_SHAPES = [(n, H, W) for n in (1, 17, 64) for H, W in ((32, 48), (80, 112), (176, 208), (192, 208), (256, 256))]


# ---- interface -------------------------------------------------------------------------------------------------------------------------------------------
def test_export_is_declared_listed_and_bound():
    from ukbb_cardiac_amd import _lib, engine
    with open(os.path.join(ROOT, 'include', 'ukbb_fcn.h')) as f:
        hdr = f.read()
    assert 'int ukbb_fcn_set_f32x3_convs(ukbb_fcn_handle *h, int on);' in hdr
    assert int(re.search(r'#define UKBB_FCN_ABI_VERSION (\d+)', hdr).group(1)) == 11          # additive: no ABI bump
    # listed: in EXPORTS_NUMBERED, the list of declared symbols whose names hold digits (tests/test_abi.py holds EXPORTS to a header scan that reads
    # letters and underscores only); every name with a digit the header declares is there, and the library exports it
    plain = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    numbered = sorted(n for n in set(re.findall(r'\b(ukbb_fcn_[a-z0-9_]+)\s*\(', plain)) if re.search(r'\d', n))
    assert numbered == sorted(_lib.EXPORTS_NUMBERED) == ['ukbb_fcn_set_f32x3_convs'] and not set(_lib.EXPORTS_NUMBERED) & set(_lib.EXPORTS)
    assert all(hasattr(_lib.lib, n) for n in _lib.EXPORTS_NUMBERED)
    assert hasattr(_lib.lib, 'ukbb_fcn_debug_plan_layout') and hasattr(_lib.lib, 'ukbb_fcn_debug_plan_layout_x3')
    assert callable(engine.Engine.set_f32x3_convs)
    # the header says where the arithmetic splits, what is dropped and what stays fp32
    doc = hdr[hdr.index('/* The FCN\'s 3x3 conv stack on three bf16 pieces'):hdr.index('int ukbb_fcn_set_f32x3_convs')]
    for word in ('Where the arithmetic splits', 'bf16(x - h - m)', 'l.h, h.l, m.m, m.h, h.m, h.h', 'What is dropped', 'm.l, l.m and l.l', 'What stays fp32',
                 'logits, prob and pred', 'UKBB_EARCH', 're-plans', 'kept and', 'ignored'):
        assert word in doc, word


def test_flag_exists_and_is_refused_without_precision_f32x3(monkeypatch):
    from ukbb_cardiac_amd import deploy_network
    fs = deploy_network.define_flags()
    assert fs.parse([])[0].f32x3_convs is False
    assert fs.parse(['--f32x3_convs', '--precision', 'f32x3'])[0].f32x3_convs is True
    for argv in (['--f32x3_convs'], ['--f32x3_convs', '--precision', 'fp32'], ['--f32x3_convs', '--precision', 'bf16_store'],
                 ['--f32x3_convs', '--precision', 'bf16_full']):
        with pytest.raises(SystemExit) as e:                       # a flag error, before any engine exists
            deploy_network.main(argv)
        assert 'Flags parsing error' in str(e.value) and '--f32x3_convs needs --precision f32x3' in str(e.value)


@pytest.mark.parametrize('model', UNET_KINDS)
def test_unet_kinds_refuse_the_switch_with_EARCH(model):
    from ukbb_cardiac_amd import _lib, engine
    from ukbb_cardiac_amd.arch import MODELS
    prec = 'fp32'
    with pytest.raises(_lib.UkbbFcnError) as e:                    # the debug export refuses as the handle call does (one check in engine.cpp)
        engine.plan_layout(MODELS[model], prec, 1, 64, 96, G.CUS, f32x3_convs=True)
    assert '(-2)' in str(e.value) and 'FCN models only' in str(e.value)
    assert engine.plan_layout(MODELS[model], prec, 1, 64, 96, G.CUS) == engine.plan_layout(MODELS[model], prec, 1, 64, 96, G.CUS, f32x3_convs=False)


# ---- plan ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('model', FCN_MODELS)
def test_switch_on_plan_is_the_f32x3_plan_on_the_new_family(model):
    seen = set()
    for n, H, W in PLAN_SHAPES:
        on, off = X.plan(model, n, H, W), X.plan(model, n, H, W, on=False)
        assert on.pop('conv_x3') is True and 'conv_x3' not in off
        assert on['acts'] == off['acts'] and on['split'] == off['split'] and {k: v for k, v in on.items() if k != 'ops'} == {k: v for k, v in off.items() if k != 'ops'}
        assert [o['name'] for o in on['ops']] == [o['name'] for o in off['ops']] and len(on['ops']) == 14
        for a, b in zip(on['ops'], off['ops']):
            if a['name'] in X.LAYERS:
                assert a['cfg'] in X.X3_TILINGS and b['cfg'] not in X.X3_TILINGS
                assert G.config_name(a['cfg']).startswith('convF32x3_3x3s%d_' % a['stride'])
                assert {k: v for k, v in a.items() if k not in ('cfg', 'mfma_macs', 'issued_macs')} == {k: v for k, v in b.items() if k not in ('cfg', 'mfma_macs', 'issued_macs')}
                assert a['mfma_macs'] == 6 * a['macs'] and a['issued_macs'] >= a['mfma_macs']
                seen.add(a['cfg'])
            else:
                assert a == b                                      # the fp32 stem (134 / 130), the squeeze launches, the head
        assert on['ops'][0]['cfg'] in (130, 134) and [o['kind'] for o in on['ops']][-2:] == ['sqg_multi', 'head']
        assert on['acts'] == X.plan(model, n, H, W, on=False, precision='fp32')['acts']       # maps and workspace of the fp32 plan
    assert seen == set(X.X3_TILINGS)
    # the plan does not depend on the batch
    for H, W in {(H, W) for _, H, W in PLAN_SHAPES}:
        assert len({json.dumps(X.plan(model, n, H, W)['ops'], sort_keys=True) for n in (1, 10, 16, 17, 64, 100)}) == 1


@pytest.mark.parametrize('model', FCN_MODELS)
def test_switch_off_or_any_other_precision_plans_as_before(model):
    from ukbb_cardiac_amd import engine
    from ukbb_cardiac_amd.arch import MODELS
    for n, H, W in PLAN_SHAPES[::2]:
        for prec in ('fp32', 'bf16', 'f32x3', 'bf16_store', 'bf16_full'):
            base = engine.plan_layout(MODELS[model], prec, n, H, W, G.CUS)
            assert 'conv_x3' not in base and not [o for o in base['ops'] if o['cfg'] in X.X3_TILINGS]
            assert engine.plan_layout(MODELS[model], prec, n, H, W, G.CUS, f32x3_convs=False) == base
            if prec != 'f32x3':                                    # kept and ignored
                assert engine.plan_layout(MODELS[model], prec, n, H, W, G.CUS, f32x3_convs=True) == base


def test_recorded_plans_replay_unchanged():
    """The switch is off by default: every recorded f32x3 plan of tests/golden/plan_layouts.json replays to its own names and tilings."""
    for model in FCN_MODELS:
        assert len(G.replay_records(model, 'f32x3', lambda n, H, W: None)) == 48


def test_new_tilings_enter_no_other_plan(monkeypatch):
    """cfg_valid admits the family in conv_x3 plans only: forced on every layer (UKBB_CONV_CFG) of a plain f32x3 / fp32 / bf16 plan it is ignored, and in
    a conv_x3 plan an override naming another family is ignored for the eleven layers."""
    from ukbb_cardiac_amd import engine
    from ukbb_cardiac_amd.arch import MODELS
    arch = MODELS[X.MODEL]
    monkeypatch.setenv('UKBB_CONV_CFG', ','.join('%s:330' % k for k in X.LAYERS))
    for prec in ('fp32', 'bf16', 'f32x3'):
        assert not [o for o in engine.plan_layout(arch, prec, 1, 192, 208, G.CUS)['ops'] if o['cfg'] in X.X3_TILINGS]
    forced = {o['name']: o['cfg'] for o in X.plan(X.MODEL, 1, 192, 208)['ops'] if o['name'] in X.LAYERS}
    assert {forced[k] for k in X.LAYERS if k not in ('conv1_0', 'conv1_1') and not k.endswith('_0')} == {330}          # valid there: 3x3 s1, Cout % 64 == 0
    assert forced['conv1_1'] == 335 and forced['conv2_0'] == 340                                                       # not valid there: the table's choice
    monkeypatch.setenv('UKBB_CONV_CFG', ','.join('%s:300' % k for k in X.LAYERS))
    assert {o['cfg'] for o in X.plan(X.MODEL, 1, 192, 208)['ops'] if o['name'] in X.LAYERS} <= set(X.X3_TILINGS)


def test_lds_of_a_tiling_is_three_times_the_bf16_operand_tilings():
    """ConvConfig::lds_bytes is not exported; the formula of kernels_conv_x3.hip is held against conv_bf_lds_bytes of kernels_conv.hip in the sources, and
    every tiling fits the 160 KB of a gfx950 compute unit (12 x 13 stride 1, 64 channels: 85 536 bytes, one workgroup per CU)."""
    with open(os.path.join(ROOT, 'ukbb_cardiac_amd', 'csrc', 'kernels_conv_x3.hip')) as f:
        src = f.read()
    assert 'return 3 * ((16 / 2 + 4) * x3_halo(th, s) * x3_halo(tw, s) + wm * cb * 9 * 64 * 4) * 4;' in src
    with open(os.path.join(ROOT, 'ukbb_cardiac_amd', 'csrc', 'kernels_conv.hip')) as f:
        assert 'return ((16 / 2 + 4) * ((th - 1) * s + ks) * ((tw - 1) * s + ks) + wm * cb * ks * ks * 64 * 4) * 4;' in f.read()
    rows = re.findall(r'X\((\d+), (\d), (\d+), (\d+), (\d), (\d), (\d)\)', src)
    assert sorted(int(r[0]) for r in rows) == list(X.X3_TILINGS)
    for cfg, s, th, tw, wm, wn, cb in (tuple(map(int, r)) for r in rows):
        lds = 3 * (12 * ((th - 1) * s + 3) * ((tw - 1) * s + 3) + wm * cb * 9 * 64 * 4) * 4
        assert lds <= 160 * 1024 and wm * wn == 4, (cfg, lds)
        assert G.config_name(cfg) == 'convF32x3_3x3s%d_t%dx%d_w%dx%d_cb%d' % (s, th, tw, wm, wn, cb) and G.tile_of(cfg) == (th, tw)
        if (cfg, s, th, tw, wm) == (330, 1, 12, 13, 2):
            assert lds == 85536
    assert len(rows) == 8


# ---- the model, the grades, R ----------------------------------------------------------------------------------------------------------------------------
H, W = 32, 48


@pytest.fixture(scope='module')
def chain():
    """Per seed and layer conv1_0 .. conv4_2: (seed, layer, grades of the model, {defect: grades}), against float64 on the model's own stored input."""
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.weights import synthetic_params
    arch = MODELS[X.MODEL]
    rows = []
    for seed in G.SEEDS:
        params = synthetic_params(arch, seed)
        img = G.distinct_images(H, W)
        x = G.layer(G.layer(img, params['conv0_0']), params['conv0_1']).astype(np.float32)       # the fused first layer: fp32
        for lname, sname, l, srcs, stride, transposed, relu in G.launches(arch):
            if lname not in X.LAYERS:
                continue
            ex = G.layer(x, params[lname], stride)
            assert ex.shape[1:3] == (H >> l, W >> l) and ex.max() > 0
            f32 = X.fp32_launch(x, params[lname], stride)
            got = X.x3_launch(x, params[lname], stride)
            rows.append((seed, lname, X.grades(got, ex, f32), {d: X.grades(X.x3_launch(x, params[lname], stride, d), ex, f32) for d in X.DEFECTS}))
            x = got
    return rows


def test_split_is_exact_and_three_pieces_leave_less_than_2_to_the_minus_24():
    v = (np.random.default_rng(3).standard_normal(4096) * np.exp2(np.random.default_rng(4).integers(-12, 12, 4096))).astype(np.float32)
    h, m, l = X.split3(v)
    for p in (h, m, l):
        assert not (p.view(np.uint32) & np.uint32(0xffff)).any()
    rest = v.astype(np.float64) - h - m - l
    assert np.abs(rest).max() <= np.abs(v).max() * 2.0 ** -24 and (np.abs(rest) <= np.abs(v) * 2.0 ** -24).all()


def test_model_passes_both_grades_at_every_layer(chain):
    assert len(chain) == 11 * len(G.SEEDS) and [r[1] for r in chain[:11]] == list(X.LAYERS)
    for seed, lname, (err, ratio), _ in chain:
        print('f32x3-model seed %4d %-8s err/scale %.2e  rms ratio to the fp32 model %.2f' % (seed, lname, err, ratio))
        assert err <= X.BOUND and ratio <= X.R, (seed, lname, err, ratio)


def test_each_planted_defect_misses_a_grade_at_every_layer(chain):
    assert len(X.DEFECTS) == 11
    for seed, lname, _, caught in chain:
        print('seed %4d %-8s %s' % (seed, lname, '  '.join('%s %.1e / %.1f' % ((d,) + v) for d, v in caught.items())))
        for d, (err, ratio) in caught.items():
            assert err > X.BOUND or ratio > X.R, (seed, lname, d, err, ratio)
    # grade 2 is needed: grade 1 alone passes a dropped small term somewhere
    assert any(caught[d][0] <= X.BOUND for _, _, _, caught in chain for d in X.DEFECTS[:3])


def test_R_is_the_geometric_mean_and_a_factor_two_from_either_side(chain):
    lines = []
    for lname in X.LAYERS:
        rows = [r for r in chain if r[1] == lname]
        correct = max(r[2][1] for r in rows)
        mildest = min(v[1] for r in rows for v in r[3].values())
        lines.append('%-8s worst ratio of the correct model %.2f  mildest defect %.2f  R %.2f' % (lname, correct, mildest, X.R))
    worst = max(r[2][1] for r in chain)
    mildest = min(v[1] for r in chain for v in r[3].values())
    geo = float(np.sqrt(worst * mildest))
    lines.append('all      worst ratio of the correct model %.3f  mildest defect %.3f  geometric mean %.3f  R %.2f' % (worst, mildest, geo, X.R))
    print('\n'.join(lines))
    if os.environ.get('UKBB_F32X3_WRITE_PROFILE'):                 # the record's section: rewritten on request, never by a plain test run
        with open(X.PROFILE) as f:
            text = f.read()
        a, b = '# ---- grade 2: per layer (tests/test_f32x3_convs.py) ----\n', '# ---- end of grade 2 ----\n'
        body = a + '\n'.join(lines) + '\n' + b
        text = text[:text.index(a)] + body + text[text.index(b) + len(b):] if a in text else text + body
        with open(X.PROFILE, 'w') as f:
            f.write(text)
    # the committed record holds these lines: same layers in the same order, every figure within 2 % (another BLAS may sum a float64 product in
    # another order and move a float32 rounding of the model)
    with open(X.PROFILE) as f:
        text = f.read()
    a, b = '# ---- grade 2: per layer (tests/test_f32x3_convs.py) ----\n', '# ---- end of grade 2 ----\n'
    kept = text[text.index(a) + len(a):text.index(b)].splitlines()
    assert [ln.split()[0] for ln in kept] == [ln.split()[0] for ln in lines]
    number = re.compile(r'-?\d+\.\d+')
    for old_ln, new_ln in zip(kept, lines):
        assert number.sub('#', old_ln) == number.sub('#', new_ln), (old_ln, new_ln)
        for u, v in zip(map(float, number.findall(old_ln)), map(float, number.findall(new_ln))):
            assert abs(u - v) <= 0.02 * abs(v) + 0.006, (old_ln, new_ln)
    assert abs(X.R - geo) <= 0.01 * geo, (X.R, geo)
    assert X.R >= 2 * worst and mildest >= 2 * X.R, (worst, X.R, mildest)


# ---- coverage --------------------------------------------------------------------------------------------------------------------------------------------
BOTH = ('small', 'large')


def recorded_shapes():
    with open(G.GOLDEN) as f:
        g = json.load(f)
    return sorted({(r[4], r[2], r[3]) for r in g['records'] if r[0] == X.MODEL and r[1] == 'f32x3' and r[5] == '' and r[6] == 0})


def reach(n, H_, W_):
    """What a case reaches: its (layer, tiling, fit, batch class) tuples and, per tiling, (tiling, fit, batch class)."""
    r = X.reached(X.MODEL, n, H_, W_)                              # (the four models plan alike: counted as FCN_sa)
    return r | {x[1:] for x in r}


@pytest.fixture(scope='module')
def recorded():
    """{(layer, tiling, fit, batch class)} of the switch-on plans at the recorded shapes and batches."""
    shapes = recorded_shapes()
    assert len(shapes) == 48
    want = set().union(*(X.reached(X.MODEL, *s) for s in shapes))
    for model in FCN_MODELS[1:]:                                   # the four models plan alike: grading two of them grades all
        assert set().union(*(X.reached(model, *s) for s in shapes)) == want
    return want


@pytest.fixture(scope='module')
def wanted(recorded):
    """The requirements: every tiling of the family on a map its tiles divide, on ragged edge tiles and on a single partial tile, at both batch
    classes (48), and every (layer, tiling, fit, batch class) of the recorded shapes (92)."""
    return recorded | {(t, f, b) for t in X.X3_TILINGS for f in X.FITS for b in BOTH}


def test_the_chooser_gives_every_tiling_every_fit():
    """choose_x3_cfg decides by the 32-pixel blocks a launch issues, so each tiling is planned in each fit on some legal shape -- not only on the recorded
    ones: e.g. 48 x 80 has a 12 x 20 level 2, which two 12 x 13 tiles cover in 12 block slots (8 x 16: 16, 11 x 13: 24), the second tile ragged."""
    seen = {}
    for H_ in range(16, 209, 16):
        for W_ in range(16, 209, 16):
            for _, t, f, _ in X.reached(X.MODEL, 1, H_, W_):
                seen.setdefault((t, f), (H_, W_))
    assert set(seen) == {(t, f) for t in X.X3_TILINGS for f in X.FITS}, sorted(set(seen))
    by_name = {o['name']: o for o in X.plan(X.MODEL, 1, 48, 80)['ops']}
    assert [(by_name[k]['cfg'], by_name[k]['Ho'], by_name[k]['Wo'], G.fit_of(by_name[k])) for k in ('conv2_0', 'conv2_1')] == [(340, 12, 20, 'ragged'), (330, 12, 20, 'ragged')]
    by_name = {o['name']: o for o in X.plan(X.MODEL, 1, 80, 144)['ops']}
    assert [(by_name[k]['cfg'], by_name[k]['Ho'], by_name[k]['Wo'], G.fit_of(by_name[k])) for k in ('conv3_0', 'conv3_1')] == [(342, 10, 18, 'ragged'), (332, 10, 18, 'ragged')]


def test_recorded_shapes_hold_92_situations(recorded):
    assert len(recorded) == 92 and {w[0] for w in recorded} == set(X.LAYERS) and {w[1] for w in recorded} == set(X.X3_TILINGS)


def test_cases_reach_every_tiling_in_every_fit_at_both_batch_classes_and_every_recorded_situation(wanted):
    assert len(set(X.CASES)) == len(X.CASES) and all(H_ % 16 == 0 and W_ % 16 == 0 for _, _, H_, W_ in X.CASES)
    assert {n for _, n, _, _ in X.CASES} == {1, X.small_batch() + 1}
    assert X.SPECIFIED == [('FCN_sa', 1, 32, 48), ('FCN_sa', 17, 32, 48), ('FCN_sa', 1, 80, 112), ('FCN_sa', 17, 80, 112), ('FCN_la_2ch', 1, 192, 208),
                           ('FCN_la_2ch', 1, 176, 208)]
    assert not [c for c in X.CASES if c[1:] == (64, 192, 208)]     # the smallest case that reaches a situation, not the workload's own batch
    assert len(wanted) == 140
    got = set().union(*(reach(*c[1:]) for c in X.CASES))
    assert not wanted - got, sorted(wanted - got, key=str)
    assert {(t, f, b) for t in X.X3_TILINGS for f in X.FITS for b in BOTH} <= got       # all eight tilings: div, ragged, partial; small, large
    # the kernel's delicate walk among them: 13-column tiles (330 / 332 / 340 / 342), several per map, the last ragged along x
    for n in (1, X.small_batch() + 1):
        ragged_x = {o['cfg'] for c in X.CASES if c[1] == n for o in X.plan(X.MODEL, *c[1:])['ops']
                    if o['cfg'] in (330, 332, 340, 342) and o['Wo'] > 13 and o['Wo'] % 13}
        assert ragged_x == {330, 332, 340, 342}, (n, ragged_x)


def test_no_added_case_is_idle(wanted):
    """The six specified shapes stay as specified (the ragged situations of 80 x 112 are also reached by other cases); every case added to them reaches
    a requirement that no other case does.  No case is larger than the largest recorded map at the first batch above plan.h SMALL_BATCH."""
    per = [reach(*c[1:]) & wanted for c in X.CASES]
    assert set().union(*per) == wanted
    for i, c in enumerate(X.CASES):
        mine = sorted(wanted - set().union(*(per[:i] + per[i + 1:])), key=str)
        print('%-32s %8d pixels; only it reaches %d requirements, e.g. %s' % (c, c[1] * c[2] * c[3], len(mine), mine[:2]))
        assert mine or c in X.SPECIFIED, 'case %s adds nothing' % (c,)
    assert max(c[1] * c[2] * c[3] for c in X.CASES) <= 17 * 256 * 256
