"""The Temporal-UNet's bf16 mode (precision 'bf16_3d', UKBB_PREC_BF16_3D 4) on the host: the plan, the refusals, the cine scratch arithmetic, and that
the grade of tests/test_temporal_bf16_launches_gpu.py tells a wrong launch from a right one.  No GPU.

The plan is the fp32 one, op for op (first3d, conv3d / tconv3d, logits), on maps of 2 bytes per element; the code is valid on the Temporal-UNet only,
and 'bf16' / 'bf16_store' stay refused there.  The cine planners answer for the code: the activation term of a window follows the element size, the
window probabilities stay fp32, so the scratch of a call is below the fp32 figure and no fewer windows fit a chunk.

The grade tells a defect: at 2 windows x 3 frames x 16 x 32 a float32 numpy evaluation of the rounding model (temporal_bf16_grading: bf16-rounded
folded kernels, bf16-valued stored maps, float32 accumulation, one rounding of what is stored) stands in for the engine and passes every launch within
half a bf16 ulp; each planted defect -- unrounded weights, a truncating store, a zeroed time tap, a time tap read across a window edge, a one-pixel
shift -- misses the grade at every launch it touches."""
import numpy as np
import pytest

import launch_grading as G
import temporal_bf16_grading as B
import temporal_unet_ref as R

MODEL = 'Temporal-UNet_ao'


def model(name=MODEL):
    from ukbb_cardiac_amd.arch import MODELS
    return MODELS[name]


def test_the_plan_is_the_fp32_op_sequence_on_two_byte_maps():
    from ukbb_cardiac_amd import engine
    arch = model()
    p32 = engine.plan_layout(arch, 'fp32', 18, 64, 96)
    p16 = engine.plan_layout(arch, B.PRECISION, 18, 64, 96)
    assert [(o['name'], o['kind']) for o in p16['ops']] == [(o['name'], o['kind']) for o in p32['ops']]
    kinds = [o['kind'] for o in p16['ops']]
    assert kinds[0] == 'first3d' and kinds[-1] == 'logits' and set(kinds[1:-1]) == {'conv3d', 'tconv3d'}
    for k in ('H', 'W', 'Ho', 'Wo', 'stride', 'in0', 'in1', 'out', 'macs', 'mfma_macs', 'issued_macs'):
        assert [o[k] for o in p16['ops']] == [o[k] for o in p32['ops']], k            # the same tiling: the same MACs, issued ones included
    assert [(a['name'], a['per_image'], a['channels']) for a in p16['acts']] == [(a['name'], a['per_image'], a['channels']) for a in p32['acts']]
    assert p16['bfio'] and not p32['bfio']
    assert all(a['bytes_per_element'] == 2 for a in p16['acts']) and all(a['bytes_per_element'] == 4 for a in p32['acts'])
    assert all(a['channels'] % 16 == 0 and a['channels'] > 0 for a in p16['acts'])     # the channel-blocked format holds whole 16-channel blocks
    ws = lambda p: sum(a['per_image'] * a['bytes_per_element'] for a in p['acts'])
    assert 2 * ws(p16) == ws(p32)


@pytest.mark.parametrize('name', ['FCN_sa', 'UNet_ao', 'UNet-LSTM_ao'])
def test_every_other_kind_refuses_the_code(name):
    from ukbb_cardiac_amd import _lib, engine
    with pytest.raises(_lib.UkbbFcnError) as e:
        engine.plan_layout(model(name), B.PRECISION, 10, 64, 96)
    assert 'failed (-2)' in str(e.value) and 'Temporal-UNet' in str(e.value)          # UKBB_EARCH, and why


@pytest.mark.parametrize('precision', ['bf16', 'bf16_store'])
def test_the_other_bf16_codes_stay_refused_on_the_temporal_unet(precision):
    from ukbb_cardiac_amd import _lib, engine
    with pytest.raises(_lib.UkbbFcnError) as e:
        engine.plan_layout(model(), precision, 18, 64, 96)
    assert 'failed (-2)' in str(e.value) and 'fp32 only' in str(e.value) and 'bf16_3d' in str(e.value)


def test_the_abi_names_the_code():
    from ukbb_cardiac_amd import _lib, engine
    assert engine._PLAN_PREC[B.PRECISION] == 4 and engine._PREC[B.PRECISION] == 4
    with open(G.os.path.join(G.ROOT, 'include', 'ukbb_fcn.h')) as f:
        assert '#define UKBB_PREC_BF16_3D 4' in f.read()
    assert _lib.lib.ukbb_fcn_abi_version() == _lib.ABI_VERSION            # the code is additive: header, library and binding agree (tests/test_abi.py)


def test_the_cine_planners_answer_for_the_code():
    from ukbb_cardiac_amd import engine
    arch = model()
    F, H, W = 50, 256, 256
    # a cine whose windows all fit one chunk in either precision (50 windows of 64 x 96): the same windows take fewer bytes
    assert engine.cine_chunk_windows(arch, 'fp32', F, 64, 96) == engine.cine_chunk_windows(arch, B.PRECISION, F, 64, 96) == F
    assert 0 < engine.cine_scratch_bytes(arch, B.PRECISION, F, 64, 96) < engine.cine_scratch_bytes(arch, 'fp32', F, 64, 96)
    # 256 x 256: the 4e9-byte rule admits more windows per chunk, so a chunk may hold MORE bytes than the fp32 one (both within the rule); at the
    # same number of windows it holds fewer (the budgeted calls below)
    b32 = engine.cine_scratch_bytes(arch, 'fp32', F, H, W)
    b16 = engine.cine_scratch_bytes(arch, B.PRECISION, F, H, W)
    assert 0 < b32 < 4.0e9 + 1e6 and 0 < b16 < 4.0e9 + 1e6
    w32 = engine.cine_chunk_windows(arch, 'fp32', F, H, W)
    w16 = engine.cine_chunk_windows(arch, B.PRECISION, F, H, W)
    assert w16 >= w32 >= 1
    assert (w32, w16) == (10, 21)                                                     # the 4e9-byte rule: 152 HW (4 | 2) + 3 HW 4 bytes per frame, T = 9
    # the activation term follows the element size, the probability term stays 4 bytes: per window T HW (152 e + 4 C)
    p = engine.plan_layout(arch, B.PRECISION, 9, H, W)
    per_frame = sum(a['per_image'] for a in p['acts'])
    tables = lambda Wn, T: ((T * Wn * 4 + 7) // 8 * 8 + (F * T * 4 + 7) // 8 * 8 + T * 8 + F * 8 + 3) // 4 * 4
    assert b16 == w16 * 9 * (per_frame * 2 + H * W * arch.n_class * 4) + tables(F, 9)
    assert b32 == w32 * 9 * (per_frame * 4 + H * W * arch.n_class * 4) + tables(F, 9)
    # under a budget: the minimum is one window, a budget below it answers 0, a budget between the two precisions' minima runs bf16_3d alone
    m32 = engine.cine_min_scratch_bytes(arch, 'fp32', F, H, W)
    m16 = engine.cine_min_scratch_bytes(arch, B.PRECISION, F, H, W)
    assert 0 < m16 < m32
    assert engine.cine_scratch_bytes(arch, B.PRECISION, F, H, W, budget=m16 - 1) == 0 and engine.cine_chunk_windows(arch, B.PRECISION, F, H, W, budget=m16 - 1) == 0
    assert engine.cine_chunk_windows(arch, B.PRECISION, F, H, W, budget=m16) == 1 and engine.cine_chunk_windows(arch, 'fp32', F, H, W, budget=m16) == 0
    budget = int(1.0e9)
    assert engine.cine_chunk_windows(arch, B.PRECISION, F, H, W, budget=budget) >= engine.cine_chunk_windows(arch, 'fp32', F, H, W, budget=budget) >= 1
    assert engine.cine_scratch_bytes(arch, B.PRECISION, F, H, W, budget=budget) <= budget
    # the codes the kind refuses keep answering 0
    assert engine.cine_scratch_bytes(arch, 'bf16', F, H, W) == 0
    assert engine.cine_scratch_bytes(model('UNet-LSTM_ao'), B.PRECISION, F, H, W) == 0


# ---- the grade tells a defect -----------------------------------------------------------------------------------------------------------------------
DEFECTS = ('unrounded weights', 'truncating store', 'zeroed time tap', 'time tap across a window edge', 'one-pixel shift')


def truncate_bf16(x):
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)


def stand_in(x, params, graph, defect=None):
    """The rounding model in float32 numpy, every launch on the stand-in's own stored input.  Returns {stored name: map}; the defects are planted in
    the bf16 launches (every 3x3x3 unit but conv0_0)."""
    stored = {}
    for lname, sname, l, srcs, stride, transposed, relu in graph:
        xin = x if srcs == [''] else np.concatenate([stored[s] for s in srcs], axis=-1)
        w, b = G.fold(params[lname], transposed)
        bf = lname not in ('conv0_0', 'logits')
        if bf and defect != 'unrounded weights':
            w = G.bf16_round(w)
        n, t = xin.shape[:2]
        if bf and defect == 'zeroed time tap':
            w = w.copy()
            w[0] = 0
        if bf and defect == 'one-pixel shift':
            xin = np.roll(xin, 1, axis=3)
        if bf and defect == 'time tap across a window edge':
            xin = xin.reshape((1, n * t) + xin.shape[2:])                # the windows end to end: only the batch's two ends see the zero frame
        xin = np.ascontiguousarray(xin, np.float32)
        y = R.conv3d_transpose_same(xin, w, stride) if transposed else R.conv3d_same(xin, w, stride)
        assert y.dtype == np.float32
        y = y.reshape((n, t) + y.shape[2:]) + b
        y = np.maximum(y, np.float32(0)) if relu else y
        if lname != 'logits':                                            # every 3-D map is stored as bf16, rounded once; the logits stay float32
            y = truncate_bf16(y) if bf and defect == 'truncating store' else G.bf16_round(y)
        stored[sname] = y
    return stored


def failing(x, params, graph, stored):
    out = set()
    for lname, sname, l, srcs, stride, transposed, relu in graph:
        if lname == 'logits':
            continue
        xin = x if srcs == [''] else np.concatenate([stored[s] for s in srcs], axis=-1)
        ex = B.exact_of(lname, xin, params[lname], stride, transposed, relu)
        G.check_bf16(sname, stored[sname])
        try:
            G.grade(lname, stored[sname], ex, float(np.abs(ex).max()), ulps=0.5, fraction=1.0)
        except AssertionError:
            out.add(lname)
    return out


def test_the_grade_passes_the_rounding_model_and_tells_planted_defects():
    from ukbb_cardiac_amd.weights import synthetic_params
    arch = B.arch_of('fc3c2')
    params = synthetic_params(arch, G.SEEDS[0])
    graph = G.launches(arch)
    x, nd = G.window_batch(0, 2, arch.fc, 16, 32)
    assert nd == 2
    assert failing(x, params, graph, stand_in(x, params, graph)) == set()
    units = {g[0] for g in graph if g[0] not in ('conv0_0', 'logits')}
    assert len(units) == len(graph) - 2
    for defect in DEFECTS:
        assert failing(x, params, graph, stand_in(x, params, graph, defect)) == units, defect
