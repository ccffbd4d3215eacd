"""--precision bf16_store (UKBB_PREC_BF16_STORE) without a GPU: the plans the host-only planner makes for it, what tests/test_fcn_bf16_store_launches_gpu.py
covers of them, and that its grades tell planted defects.

Plans (engine.plan_layout on 256 compute units, the four FCN models over the SHAPES x BATCHES of tests/test_plan_layout.py): the fused stem, the eleven
convs conv1_0 .. conv4_2 each on a bf16-STORAGE tiling (a row of g_tuned_bfio in plan.cpp or a fallback: names convBF16io_ / convBF16ws_ / convBF16wr_),
never on an fp32 tiling or on a bf16-operand one (200-series, convBF16_), then the squeeze launch(es) and the head; encoder maps take 2 bytes per
element, the G_l maps 4, and the workspace is smaller than the fp32 plan's.  The U-Net kinds refuse the code.  fp32, bf16 and f32x3 plans are pinned
by tests/test_plan_layout.py and do not move.

Coverage: every (layer, tiling, fit, walker round class) those 192 plans hold -- fit: the tiles divide the map / whole tiles and a ragged last one /
a single partial tile; round class of the weight-stationary walkers and of the stem: below one round, between one and two, two or more exact / ragged,
in wave-major or XCD-local tile order (tests/launch_grading.py ws_launch, stem_launch) -- is reached by some case of the GPU file, no case is
idle, and the four models hold the same set (one encoder graph), which is why the cases take the models in turn.

The grades tell a defect: on the three rough images at 64 x 96 a float32 numpy evaluation of the rounding model (kernels rounded to bf16, every
encoder map rounded once as stored, fp32 accumulation, squeeze and head in fp32 on the stored values) stands in for the engine and passes every
launch; folded weights left unrounded, a truncating store, one zeroed tap and an input shifted by a pixel each miss the grade at every encoder launch
they touch; a squeeze that reads the stored bf16 blocks as if they were fp32 NHWC misses its bound at every level."""
import os
import re

import numpy as np
import pytest

import test_bf16_launch_coverage as C                              # its float32 stand-in launch32 and DEFECTS
import test_bf16_launches_gpu as B                                 # the stem as a unit: stem_reference, grade_stem
import test_fcn_bf16_store_launches_gpu as L
import test_head_launches_gpu as HL                                # the squeeze and head models
from launch_grading import SEEDS, bf16_round, check_bf16, config_name, distinct_images, grade, launches, layer, no_case_is_idle, rel_err
from test_plan_layout import BATCHES, SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FCN_MODELS = L.MODELS_IN_TURN
STORAGE_PREFIXES = ('convBF16io_', 'convBF16ws_', 'convBF16wr_')
BENCH = (64, 192, 208)


def plan(model, prec, n, H, W):
    from ukbb_cardiac_amd import engine
    from ukbb_cardiac_amd.arch import MODELS
    return engine.plan_layout(MODELS[model], prec, n, H, W, L.CUS)


def workspace_bytes(p, n):
    return n * sum(a['per_image'] * a['bytes_per_element'] for a in p['acts'])


def tuned_bfio_rows():
    """{(ks, stride, cin, cout): [tilings in order]} of g_tuned_bfio, read from plan.cpp."""
    with open(os.path.join(ROOT, 'ukbb_cardiac_amd', 'csrc', 'plan.cpp')) as f:
        src = f.read()
    body = src[src.index('const Tuned g_tuned_bfio[] = {'):]
    body = body[:body.index('};')]
    return {tuple(map(int, m.groups()[:4])): [int(v) for v in m.groups()[4:] if int(v) >= 0] for m in re.finditer(r'\{(\d), (\d), (\d+), (\d+), (-?\d+), (-?\d+), (-?\d+)\}', body)}


# ---- the plans ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('model', FCN_MODELS)
def test_bf16_store_plans_of_the_fcn_models(model):
    from ukbb_cardiac_amd.arch import MODELS
    arch = MODELS[model]
    tuned = tuned_bfio_rows()
    convs = [gr for gr in launches(arch) if gr[0] not in ('conv0_0', 'conv0_1', 'logits')]
    assert len(convs) == 11
    n_plans, on_tuned = 0, 0
    for H, W in SHAPES:
        for n in BATCHES:
            p, f = plan(model, 'bf16_store', n, H, W), plan(model, 'fp32', n, H, W)
            ops = p['ops']
            # stem, encoder convs, the squeeze launch, the head
            assert [o['name'] for o in ops] == ['conv0_0+conv0_1'] + [gr[0] for gr in convs] + ['sqg1-4', 'head'], [o['name'] for o in ops]
            assert [o['kind'] for o in ops] == ['stem'] + ['conv'] * 11 + ['sqg_multi', 'head']
            assert p['bfio'] and p['split'] == (-1, -2)                      # UKBB_SPLIT_FROM keeps its FCN default of 0
            for o, gr in zip(ops[1:12], convs):
                name = config_name(o['cfg'])
                assert name.startswith(STORAGE_PREFIXES), (o['name'], o['cfg'], name)      # no fp32 tiling, no 200-series (convBF16_) tiling
                assert not 200 <= o['cfg'] < 230 and o['cfg'] >= 230
                assert '_3x3s%d_' % gr[4] in name and o['stride'] == gr[4]
                row = tuned[(3, gr[4], arch.n_filter[gr[2] - 1] if gr[4] == 2 else arch.n_filter[gr[2]], arch.n_filter[gr[2]])]
                on_tuned += o['cfg'] in row
            # encoder maps 2 bytes per element, G_l 4; smaller than the fp32 plan's workspace, which holds the same maps at 4
            assert [(a['name'], a['per_image']) for a in p['acts']] == [(a['name'], a['per_image']) for a in f['acts']]
            assert all(a['bytes_per_element'] == (4 if a['name'].startswith('g') else 2) for a in p['acts']), p['acts']
            assert all(a['bytes_per_element'] == 4 for a in f['acts'])
            assert {a['name'] for a in p['acts'] if a['bytes_per_element'] == 4} == {'g1', 'g2', 'g3', 'g4'}
            assert workspace_bytes(p, n) < workspace_bytes(f, n)
            g_bytes = n * sum(a['per_image'] * 4 for a in p['acts'] if a['name'].startswith('g'))
            assert workspace_bytes(p, n) - g_bytes == (workspace_bytes(f, n) - g_bytes) // 2
            n_plans += 1
    assert n_plans == 48
    assert on_tuned >= 48 * 11 // 2, on_tuned                                # most launches sit on a measured row, the rest on a fallback that fits the map


def test_the_other_precisions_of_an_fcn_plan_are_untouched_by_the_new_code():
    """bf16 on an FCN handle stays the bf16-OPERAND mode (fp32 storage, 200-series tilings, the fused first layer 130)."""
    p = plan('FCN_sa', 'bf16', *BENCH)
    assert not p['bfio'] and all(a['bytes_per_element'] == 4 for a in p['acts'])
    assert [o['cfg'] for o in p['ops'] if o['kind'] == 'conv'][0] == 130 and all(200 <= o['cfg'] < 230 for o in p['ops'][1:12])
    u = plan('UNet_ao', 'bf16', 10, 256, 256)
    assert u['bfio'] and all(a['bytes_per_element'] == 4 for a in u['acts'])      # the U-Net kinds allocate floats in either precision (plan.h act_alloc_esz)


@pytest.mark.parametrize('model', ['UNet_ao', 'UNet-LSTM_ao', 'Temporal-UNet_ao'])
def test_the_unet_kinds_refuse_the_code(model):
    from ukbb_cardiac_amd import _lib
    with pytest.raises(_lib.UkbbFcnError) as e:
        plan(model, 'bf16_store', 10, 64, 96)
    assert 'failed (-2)' in str(e.value) and 'already store bf16 under UKBB_PREC_BF16' in str(e.value)       # UKBB_EARCH


def test_cine_planners_answer_zero_for_the_code():
    import ctypes as Ct
    from ukbb_cardiac_amd import _lib
    from ukbb_cardiac_amd.arch import MODELS
    for model in ('UNet-LSTM_ao', 'Temporal-UNet_ao', 'FCN_sa'):
        a = _lib.arch_struct(MODELS[model])
        assert _lib.lib.ukbb_fcn_cine_scratch_bytes(Ct.byref(a), 3, 50, 64, 96, 1, 0) == 0
        assert _lib.lib.ukbb_fcn_cine_min_scratch_bytes(Ct.byref(a), 3, 50, 64, 96, 1) == 0
        assert _lib.lib.ukbb_fcn_cine_chunk_windows(Ct.byref(a), 3, 50, 64, 96, 1, 0) == 0


# ---- coverage ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def wanted():
    """Every (layer, tiling, fit, walker round class) of the bf16_store plans over SHAPES x BATCHES; the same set for each of the four models."""
    want = {m: set() for m in FCN_MODELS}
    for m in FCN_MODELS:
        for H, W in SHAPES:
            for n in BATCHES:
                want[m] |= L.situations(n, H, W, m)
    assert all(want[m] == want[FCN_MODELS[0]] for m in FCN_MODELS)
    return want[FCN_MODELS[0]]


def test_the_plans_hold_88_situations_on_14_tilings(wanted):
    assert len(wanted) == 88
    assert {k[1] for k in wanted} == {-1, 230, 232, 234, 239, 240, 241, 242, 244, 245, 248, 400, 401, 402}
    assert {k[2] for k in wanted if k[1] >= 0} == {'div', 'ragged', 'partial'}
    walkers = {k[3].split(' ')[0] + (' ' + k[3].split(' ')[1] if k[3].startswith('two+') else '') for k in wanted if k[1] >= 400}
    assert walkers == {'below', 'between', 'two+ exact', 'two+ ragged'}
    assert {k[3].split(' ')[-1] for k in wanted if k[1] == 401} == {'wave', 'xcd'}
    for k in sorted(wanted, key=str):
        print('%-16s tiling %3d  %-8s %s' % k)


def test_cases_reach_every_situation_and_none_is_idle(wanted):
    cases = L.CASES
    assert len(set(cases)) == len(cases) and all(H % 16 == 0 and W % 16 == 0 and n <= 129 and n * H * W <= 100 * 256 * 256 for n, H, W in cases)
    assert BENCH not in cases, 'the smallest case that reaches a situation, not the workload\'s own batch'
    only = no_case_is_idle(list(enumerate(cases)), lambda ic: L.situations(*ic[1], L.model_of(ic[0])), wanted)
    for (i, c), mine in zip(enumerate(cases), only):
        print('%-16s %-16s %8d pixels; only it reaches %s' % (c, L.model_of(i), c[0] * c[1] * c[2], mine))
    # all four class counts appear, with both seeds
    from ukbb_cardiac_amd.arch import MODELS
    assert {MODELS[L.model_of(i)].n_class for i in range(len(cases))} == {MODELS[m].n_class for m in FCN_MODELS} and len({MODELS[m].n_class for m in FCN_MODELS}) == 4
    assert {SEEDS[i % 2] for i in range(len(cases))} == {1234, 7}


# ---- the grades tell a defect ---------------------------------------------------------------------------------------------------------------------------
H, W = 64, 96
DEFECTS = C.DEFECTS          # folded weights not rounded to bf16, one zeroed tap, input shifted by a pixel, truncation on the store


def fails(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except AssertionError:
        return True
    return False


def to_blocked_bf16(a):
    """NHWC float32 holding bf16 values -> the uint16 words of the engine's channel-blocked map [N][C/16][H][W][16]."""
    n, h, w, c = a.shape
    u = (np.ascontiguousarray(a, np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)
    return np.ascontiguousarray(u.reshape(n, h, w, c // 16, 16).transpose(0, 3, 1, 2, 4))


def read_undecoded(a):
    """What a squeeze launch that ignored the input format would read: the map's bytes taken as fp32 [npix][cin] (the map is half as long; the rest of
    the read lies past it -- here it wraps around)."""
    raw = to_blocked_bf16(a).reshape(-1).view(np.float32)
    return np.resize(raw, a.size).reshape(a.shape)


@pytest.fixture(scope='module', params=SEEDS)
def stand_in(request):
    """The float32 stand-in's maps of the three rough images, graded launch by launch as the GPU file grades the engine; per encoder launch, whether
    each planted defect fails the grade.  -> (stored maps, g, rows [(layer, {defect: failed})])."""
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.weights import synthetic_params
    arch = MODELS['FCN_sa']
    params = synthetic_params(arch, request.param)
    img = ((distinct_images(H, W) - np.float32(0.3)) / np.float32(0.25)).astype(np.float32)
    stored, rows = {}, []
    for lname, sname, l, srcs, stride, transposed, relu in launches(arch):
        if lname in ('conv0_0', 'logits'):
            continue
        if lname == 'conv0_1':                                            # the stem as a unit; the defect sits in its second layer
            a00 = C.launch32(bf16_round(img), params['conv0_0'])
            ex, slack, n_amb = B.stem_reference(img, params, 'stem')
            sc = float(np.abs(ex).max())
            stored[sname] = C.launch32(a00, params[lname])
            B.grade_stem(stored[sname], ex, sc, slack)
            rows.append((lname, {d: fails(B.grade_stem, C.launch32(a00, params[lname], defect=d), ex, sc, slack) for d in DEFECTS}))
            continue
        x = stored[srcs[0]]
        ex = layer(x, params[lname], stride, round_w=True)
        sc = float(np.abs(ex).max())
        stored[sname] = C.launch32(x, params[lname], stride)
        assert grade(lname, stored[sname], ex, sc, ulps=0.5, fraction=1.0) == 1.0
        rows.append((lname, {d: fails(grade, lname, C.launch32(x, params[lname], stride, defect=d), ex, sc, ulps=0.5, fraction=1.0) for d in DEFECTS}))
    g = {l: HL.squeeze_map(stored['conv%d' % l], params, l, np.float32) for l in range(1, 5)}
    return params, stored, g, rows


def test_stand_in_passes_every_launch(stand_in):
    params, stored, g, rows = stand_in
    from ukbb_cardiac_amd.arch import MODELS
    assert [r[0] for r in rows] == [gr[0] for gr in launches(MODELS['FCN_sa']) if gr[0] not in ('conv0_0', 'logits')]
    for a in stored.values():
        check_bf16('stand-in', a)
    for l in range(1, 5):
        assert g[l].dtype == np.float32
        assert rel_err(g[l], HL.squeeze_map(stored['conv%d' % l], params, l))[0] <= L.BOUND
    lg32 = HL.head_logits(stored['conv0'], g, params, np.float32)
    assert lg32.dtype == np.float32 and rel_err(lg32, HL.head_logits(stored['conv0'], g, params))[0] <= L.BOUND


def test_each_planted_defect_fails_at_every_encoder_launch(stand_in):
    params, stored, g, rows = stand_in
    assert len(rows) == 12
    for lname, failed in rows:
        print('%-8s %s' % (lname, failed))
        assert all(failed[d] for d in DEFECTS), (lname, failed)


def test_an_undecoded_squeeze_input_misses_the_bound_at_every_level(stand_in):
    params, stored, g, rows = stand_in
    for l in range(1, 5):
        x = stored['conv%d' % l]
        ex = HL.squeeze_map(x, params, l)
        with np.errstate(all='ignore'):
            bad = HL.squeeze_map(read_undecoded(x), params, l, np.float32)
            err = rel_err(np.nan_to_num(bad, nan=np.float32(3e38), posinf=np.float32(3e38), neginf=np.float32(-3e38)), ex)[0]
        print('g%d: undecoded input err/scale %.3g' % (l, err))
        assert not err <= 100 * L.BOUND, (l, err)
        # the channel-blocked layout itself matters as well: the decoded values in blocked order, taken as NHWC, miss it too (levels with C > 16)
        n, h, w, c = x.shape
        scrambled = x.reshape(n, h, w, c // 16, 16).transpose(0, 3, 1, 2, 4).reshape(n, h, w, c)
        assert not rel_err(HL.squeeze_map(scrambled, params, l, np.float32), ex)[0] <= 100 * L.BOUND
