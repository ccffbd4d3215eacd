"""What tests/test_bf16_operand_launches_gpu.py covers, checked without a GPU (engine.plan_layout: the host-only planner on 256 compute units, built
first as for tests/test_plan_layout.py), and that its bound can tell a wrong bf16-operand launch from a right one.

Completeness: the recorded knob-less bf16 plans of FCN_sa (tests/golden/plan_layouts.json: 8 shapes x 6 batches) replay to their own names and
tilings and hold exactly 25 (layer, tiling) combinations on the tilings {130, 200, 201, 202, 210, 211}.  Every one is planned by some entry of CASES,
and counts only where the case reaches it on a map its tiles divide, or do not divide, as some recorded plan of that combination has it (the rule of
tests/test_bf16_launch_coverage.py for tile-per-workgroup tilings; tile sizes from the tiling's name, "..._t<rows>x<columns>_...", and the op's
Ho / Wo).  "Do not divide" is told apart further (fit_of of tests/launch_grading.py): 'ragged', whole tiles and a partial last one along an axis, and 'partial', one partial tile
only -- a ragged edge tile takes its halo from a neighbouring tile's pixels on one side and from the padding on the other.  Per tiling CASES also
reaches every (fit, batch class) the records hold, the batch classes being up to plan.h SMALL_BATCH and above it: the bf16 plans do not depend on the
batch, but the grids do, and the copy identity of the GPU file needs several images.  That is 53 requirements.  The recorded bf16 plans of FCN_la_2ch,
FCN_la_4ch and FCN_la_4ch_seg4 give the same set of (layer, tiling, fit, batch class) -- the encoders are the same graph -- which is why grading
FCN_sa grades them.  No case is idle, none is the benchmark's batch, and the batch sizes are 1 and plan.h SMALL_BATCH + 1.

Tilings 203 and 212 are registered but taken by no recorded plan; the GPU file forces them in a child process (UKBB_CONV_CFG), and
test_forced_tilings_are_planned_where_they_are_valid replays that plan here.  Tilings 220 and 221, the 2 x 2 (transposed-conv) kernels with bf16
operands and fp32 storage, are UNREACHABLE: cfg_valid admits a ConvFamily::Bf16Operands tiling only in Bf16Mode::Operands, plan_mode gives that mode to
UKBB_KIND_FCN alone (every other kind takes Bf16Mode::Storage), and the FCN graph has no 2 x 2 layer; forced on every layer (UKBB_CONV_CFG) of every
model in every precision it accepts they enter no plan, and no record of any model, precision or knob holds them
(test_tilings_220_and_221_are_unreachable).  They are left as they are.

The bound tells a defect: on the three rough images at 32 x 48, the eleven layers conv1_0 .. conv4_2 each fed by the layer before, a float32 numpy
evaluation of the rounding model stands in for the engine and passes BOUND at every layer, while weights or activations (or both: the layer on an
fp32 tiling) left unrounded, weights or activations truncated instead of rounded to nearest even, and an input shifted by a pixel each miss it by at
least 10 x, one zeroed tap by at least 100 x, at every layer; and the fp32 model of a launch is itself >= 10 x BOUND from the rounding model, which is
what the "really bf16" assertion of the GPU file rests on."""
import collections
import json
import os
import re

import numpy as np
import pytest

import launch_grading as G
import test_bf16_operand_launches_gpu as L
from oracle import fcn_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = G.GOLDEN
LA_MODELS = ('FCN_la_2ch', 'FCN_la_4ch', 'FCN_la_4ch_seg4')
TILINGS = {130, 200, 201, 202, 210, 211}
BENCH = (64, 192, 208)                  # bench.py BATCH, H, W


def small_batch():
    with open(os.path.join(ROOT, 'ukbb_cardiac_amd', 'csrc', 'plan.h')) as f:
        return int(re.search(r'constexpr int SMALL_BATCH = (\d+);', f.read()).group(1))


def batch_class(n):
    """The plans do not depend on the batch, the launch grids do (one workgroup per tile, image and Cout group), and batch independence can only
    fail with several images: up to plan.h SMALL_BATCH, or above it."""
    return 'small' if n <= small_batch() else 'large'


def conv_ops(n, H, W, model=L.MODEL):
    from ukbb_cardiac_amd import engine
    from ukbb_cardiac_amd.arch import MODELS
    return [o for o in engine.plan_layout(MODELS[model], 'bf16', n, H, W, G.CUS)['ops']]


def reached(n, H, W, model=L.MODEL):
    """{(layer, tiling): fit} of the bf16 plan's conv launches (the fused first layer as 'conv0_0+conv0_1')."""
    return {(o['name'], o['cfg']): G.fit_of(o) for o in conv_ops(n, H, W, model) if o['kind'] == 'conv'}


def replay_records(model):
    """{(layer, tiling): set of (fit, batch class)} over the recorded knob-less bf16 plans of one model (G.replay_records)."""
    replayed = G.replay_records(model, 'bf16', lambda n, H, W: reached(n, H, W, model))
    assert len(replayed) == 48, (model, len(replayed))
    rec = collections.defaultdict(set)
    for n, _, _, got in replayed:
        for k, fit in got.items():
            rec[k].add((fit, batch_class(n)))
    return dict(rec)


@pytest.fixture(scope='module')
def recorded():
    return replay_records(L.MODEL)


def requirements(rec):
    """Every combination, and per tiling every (fit, batch class) the recorded plans hold."""
    return set(rec) | {(k[1],) + fb for k, fbs in rec.items() for fb in fbs}


def covered(cases, rec):
    got = set()
    for c in cases:
        for k, fit in reached(*c).items():
            if k in rec and fit in {f for f, _ in rec[k]}:
                got.add(k)
                if (fit, batch_class(c[0])) in rec[k]:
                    got.add((k[1], fit, batch_class(c[0])))
    return got


def test_recorded_plans_hold_25_combinations_on_six_tilings(recorded):
    assert len(recorded) == 25 and {k[1] for k in recorded} == TILINGS
    by_layer = collections.defaultdict(set)
    for (layer, cfg) in recorded:
        by_layer[layer].add(cfg)
    assert by_layer.pop('conv0_0+conv0_1') == {130}
    assert all(cfgs <= ({210, 211} if layer.endswith('_0') else {200, 201, 202}) for layer, cfgs in by_layer.items()) and len(by_layer) == 11
    assert all(L.is_bf16_tiling(c) for c in TILINGS - {130}) and not L.is_bf16_tiling(130)


def test_the_long_axis_models_record_the_same_combinations_and_fits(recorded):
    for model in LA_MODELS:
        assert replay_records(model) == recorded, model


def test_cases_reach_every_recorded_combination_and_fit(recorded):
    assert len(set(L.CASES)) == len(L.CASES) and all(H % 16 == 0 and W % 16 == 0 for n, H, W in L.CASES)
    assert BENCH not in L.CASES, 'the smallest case that reaches a situation, not the workload\'s own batch'
    with open(os.path.join(ROOT, 'bench.py')) as f:
        assert 'BATCH, H, W = %d, %d, %d' % BENCH in f.read()
    assert len(requirements(recorded)) == 53
    missing = requirements(recorded) - covered(L.CASES, recorded)
    assert not missing, sorted(missing, key=str)
    # the situations the defects of a tile walk hide in are among them: ragged edge tiles of 201, 202, 210 and 211, whole tilings of 200, 201 and 210
    assert {(t, 'ragged', b) for t in (201, 202, 210, 211) for b in ('small', 'large')} | {(t, 'div', 'large') for t in (200, 201, 210)} <= requirements(recorded)


def test_no_case_is_idle(recorded):
    only = G.no_case_is_idle(L.CASES, lambda c: covered([c], recorded), requirements(recorded))
    for c, mine in zip(L.CASES, only):
        print('%-14s %7d pixels; only it reaches %s' % (c, c[0] * c[1] * c[2], mine))
    assert sum(n * H * W for n, H, W in L.CASES) == 854016 and sum(min(n, 3) * H * W for n, H, W in L.CASES) == 190976        # the docstring's table


def test_batch_sizes_are_one_and_the_first_above_the_small_batch_threshold():
    assert {n for n, _, _ in L.CASES} == {1, small_batch() + 1} and {batch_class(n) for n, _, _ in L.CASES} == {'small', 'large'}


def test_graph_lists_every_planned_conv_launch():
    """launches() names exactly the conv launches of the plans, and every map the GPU test reads is stored; the squeeze and head stay out."""
    from ukbb_cardiac_amd import engine
    from ukbb_cardiac_amd.arch import MODELS
    arch = MODELS[L.MODEL]
    graph = [g for g in G.launches(arch) if g[0] != 'logits']
    assert all(not g[5] and g[6] and len(g[3]) == 1 for g in graph)          # no transposed conv, ReLU everywhere, one source
    for n, H, W in L.CASES + L.FORCED_CASES:
        ops = conv_ops(n, H, W)
        assert [part for o in ops if o['kind'] == 'conv' for part in o['name'].split('+')] == [g[0] for g in graph]
        assert [o['name'] for o in ops if o['kind'] != 'conv'] == ['sqg1-4', 'head']
        stored = {a['name'] for a in engine.plan_layout(arch, 'bf16', n, H, W, G.CUS)['acts']}
        assert {g[1] for g in graph if g[0] != 'conv0_0'} <= stored


def test_forced_tilings_are_planned_where_they_are_valid(monkeypatch):
    """The child's plan: 212 / 203 on the layers with Cout % 64 == 0, the override ignored at the 32-channel level 1; on FORCED_CASES[0] their tiles
    divide every map, on FORCED_CASES[1] none; no recorded plan holds either tiling."""
    with open(GOLDEN) as f:
        g = json.load(f)
    assert not {L.FORCED_S1, L.FORCED_S2} & {c for cfgs in g['cfgs'] for c in cfgs}
    assert G.config_name(L.FORCED_S1) == 'convBF16_3x3s1_t16x16_w2x2_cb1' and G.config_name(L.FORCED_S2) == 'convBF16_3x3s2_t8x16_w2x2_cb1'
    monkeypatch.setenv('UKBB_CONV_CFG', L.forced_spec())                  # read at every plan build (plan.cpp override_cfg)
    for index, (n, H, W) in enumerate(L.FORCED_CASES):
        got = reached(n, H, W)
        want = L.forced_expectation()
        ran = {k[0]: k[1] for k in got}
        assert [ran[k] for k in ('conv1_0', 'conv1_1')] == [211, 202] and want['conv1_0'] is None and want['conv1_1'] is None
        assert all(ran[k] == v for k, v in want.items() if v is not None)
        assert sorted(ran.values()).count(L.FORCED_S2) == 3 and sorted(ran.values()).count(L.FORCED_S1) == 6
        assert {fit for k, fit in got.items() if k[1] in (L.FORCED_S1, L.FORCED_S2)} == ({'div'} if index == 0 else {'ragged', 'partial'})
        assert max(-(-o['Ho'] // 16) * -(-o['Wo'] // 16) for o in conv_ops(n, H, W) if o['cfg'] == L.FORCED_S1) > 1      # more than one workgroup


def test_tilings_220_and_221_are_unreachable(monkeypatch):
    from ukbb_cardiac_amd import _lib, engine
    from ukbb_cardiac_amd.arch import KIND_FCN, KIND_TEMPORAL_UNET, MODELS
    # a bf16-operand tiling only in a bf16-operand plan, and such a plan only for FCN handles: forced on every layer of every model in
    # every precision the model accepts, neither tiling is planned anywhere
    layers = ['up%d_t' % l for l in range(4)] + ['%s%d_%d' % (p, l, i) for p in ('conv', 'up') for l in range(5)
                                                     for i in range(max(max(a.n_block) for a in MODELS.values()))]
    n_plans, refused = 0, set()
    for forced in (220, 221):
        monkeypatch.setenv('UKBB_CONV_CFG', ','.join('%s:%d' % (k, forced) for k in layers))      # read at every plan build
        for name, arch in MODELS.items():
            for prec in ('fp32', 'bf16', 'f32x3', 'bf16_store'):
                for n, H, W in ((1, 64, 96), (17, 48, 16)):
                    try:
                        ops = engine.plan_layout(arch, prec, n, H, W, G.CUS)['ops']
                    except _lib.UkbbFcnError:
                        refused.add((name, prec))
                        continue
                    assert forced not in [o['cfg'] for o in ops], (forced, name, prec, n, H, W)
                    n_plans += 1
    assert refused == ({(k, 'bf16') for k, a in MODELS.items() if a.kind == KIND_TEMPORAL_UNET} |
                       {(k, 'bf16_store') for k, a in MODELS.items() if a.kind != KIND_FCN}), refused
    assert n_plans == 96
    monkeypatch.delenv('UKBB_CONV_CFG')
    assert G.config_name(220).startswith('convBF16_2x2s1_') and G.config_name(221).startswith('convBF16_2x2s1_')
    # the FCN graph has no 2 x 2 layer: no transposed conv among its launches, nor in any of its plans; the other kinds plan bf16 storage
    for name, arch in MODELS.items():
        if arch.kind == KIND_FCN:
            assert not [g for g in G.launches(arch) if g[5]], name
            assert {o['kind'] for o in conv_ops(1, 64, 96, name)} == {'conv', 'sqg_multi', 'head'}
    with open(GOLDEN) as f:
        g = json.load(f)
    assert not {220, 221} & {c for cfgs in g['cfgs'] for c in cfgs}
    kinds = {r[0]: set() for r in g['records']}
    for r in g['records']:
        if r[1] == 'bf16' and r[6] == 0:
            kinds[r[0]] |= {c for c in g['cfgs'][r[9]] if 200 <= c < 230}
    assert all(bool(v) == (MODELS[k].kind == KIND_FCN) for k, v in kinds.items()), kinds


# ---- the bound tells a defect ----------------------------------------------------------------------------------------------------------------------------
H, W = 32, 48
DEFECTS = ('weights left in fp32', 'activations left in fp32', 'both left in fp32', 'weights truncated', 'activations truncated', 'one zeroed tap',
           'input shifted by a pixel')


def truncate(x):
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)


def launch32(x, p, stride, defect=None):
    """One bf16-operand launch as the engine is specified to run it, in float32 numpy (products of bf16 values are exact in float32, the sum is
    float32) -- with one planted defect, if any."""
    w, b = G.fold(p)
    x = np.ascontiguousarray(x, np.float32)
    if defect == DEFECTS[6]:
        x = np.concatenate([np.zeros_like(x[:, :, :1]), x[:, :, :-1]], axis=2)
    xr = truncate(x) if defect == DEFECTS[4] else x if defect in (DEFECTS[1], DEFECTS[2]) else G.bf16_round(x)
    wr = truncate(w) if defect == DEFECTS[3] else w if defect in (DEFECTS[0], DEFECTS[2]) else G.bf16_round(w)
    if defect == DEFECTS[5]:
        wr = wr.copy()
        wr[0, 2] = 0
    y = np.maximum(O.conv2d_same(xr, wr, stride) + b, np.float32(0))
    assert y.dtype == np.float32
    return y


@pytest.fixture(scope='module')
def chain():
    """Per seed and layer conv1_0 .. conv4_2: (layer, err of the float32 stand-in, {defect: err}, distance of the fp32 model), all against the
    float64 rounding model on the stand-in's own stored input."""
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.weights import synthetic_params
    arch = MODELS[L.MODEL]
    rows = []
    for seed in G.SEEDS:
        params = synthetic_params(arch, seed)
        img = G.distinct_images(H, W)
        x = G.layer(G.layer(img, params['conv0_0']), params['conv0_1']).astype(np.float32)       # the fused first layer: fp32
        for lname, sname, l, srcs, stride, transposed, relu in G.launches(arch):
            if lname in ('conv0_0', 'conv0_1', 'logits'):
                continue
            ex = G.layer(x, params[lname], stride, round_w=True, round_x=True)
            assert ex.shape[1:3] == (H >> l, W >> l) and ex.max() > 0
            got = launch32(x, params[lname], stride)
            rows.append((seed, lname, G.rel_err(got, ex)[0], {d: G.rel_err(launch32(x, params[lname], stride, d), ex)[0] for d in DEFECTS},
                         G.rel_err(G.layer(x, params[lname], stride), ex)[0]))
            x = got
    return rows


def test_float32_stand_in_passes_the_bound_at_every_layer(chain):
    assert len(chain) == 11 * len(G.SEEDS)
    for seed, lname, err, _, _ in chain:
        print('stand-in seed %4d %-8s err/scale %.2e' % (seed, lname, err))
        assert err <= L.BOUND, (seed, lname, err)


def test_each_planted_defect_fails_the_bound_at_every_layer(chain):
    for seed, lname, _, caught, _ in chain:
        print('seed %4d %-8s %s' % (seed, lname, '  '.join('%s %.1e' % kv for kv in caught.items())))
        for d, err in caught.items():
            assert err >= (100 if d == DEFECTS[5] else 10) * L.BOUND, (seed, lname, d, err)


def test_fp32_model_is_far_from_the_rounding_model(chain):
    """What the GPU file's "at least 10 x BOUND from the fp32 model" assertion rests on: a correct bf16-operand launch is within BOUND of the rounding
    model, the fp32 model >= 11 x BOUND from it at every layer, so the launch is >= 10 x BOUND from the fp32 model."""
    assert L.APART == 10 * L.BOUND
    for seed, lname, _, _, apart in chain:
        assert apart >= L.APART + L.BOUND, (seed, lname, apart)
