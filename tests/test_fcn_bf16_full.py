"""--precision bf16_full (UKBB_PREC_BF16_FULL) without a GPU: the code and its refusals, the plan the host-only planner makes for it, the host packer of
the head's bf16 weight blocks, and that the head's grade (tests/fcn_bf16_full_grading.py) passes a correct evaluation and tells planted defects.

Plan: bf16_store's, op for op, tiling for tiling and map for map, plus the head flag (plan_layout's 'head_bf16'); every other precision keeps the flag
off.  The U-Net, UNet-LSTM and Temporal-UNet kinds refuse the code with UKBB_EARCH.

Packer: ukbb_fcn_debug_pack_head_bf16 (pack_head_bf16 of pack.cpp, host arithmetic only) against a numpy restatement of the A-fragment order of
v_mfma_f32_32x32x16_bf16 -- lane (m = lane & 31, g = lane >> 5) holds A[row m][k = 8 g + e], e = 0..7, two bf16 per dword, low half first -- with
same_dim0's k in the order of the stored conv0 half-block and out0's / out1's k in the order the registers of a 32 x 32 accumulator tile supply it
(register r of lane half g = row (r & 3) + 8 (r >> 2) + 4 g), every weight rounded to bf16 once, ties to even.

Grade: for every case of the GPU grader, on what a float64 rounding model of the encoder stores for the case's own images and weights, a float32 numpy
stand-in of the head's specification passes with the zero-slack floor (40 %) met, and each planted defect -- weights not rounded, S not rounded, P not
rounded, truncation instead of round-to-nearest-even, a dropped K chunk of out1, bf16_store's fp32 head run in its place -- misses the grade.  No case
is idle: each reaches a situation of the head's tile walk that no other case reaches.

Measured here (profiles/fcn_bf16_full.txt): the stand-in's worst error on zero-slack pixels 2.3e-7 of the logits' scale, no pixel outside the bound, smallest
zero-slack share 0.574; the weakest planted defect (unrounded P at 17 x 240 x 256) misses the bound by 229 x, with 13 % of its pixels inside.  The module
takes 40 s, nearly all of it the float64 encoder model of the 11 cases, computed once."""
import ctypes as Ct
import os
import re

import numpy as np
import pytest

import fcn_bf16_full_grading as F
from launch_grading import CUS, no_case_is_idle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FCN_MODELS = ('FCN_sa', 'FCN_la_2ch', 'FCN_la_4ch', 'FCN_la_4ch_seg4')
PLAN_SHAPES = [(1, 16, 16), (1, 192, 208), (17, 256, 256), (64, 192, 208), (64, 176, 208), (100, 80, 112)]


def plan(model, prec, n, H, W):
    from ukbb_cardiac_amd import engine
    from ukbb_cardiac_amd.arch import MODELS
    return engine.plan_layout(MODELS[model], prec, n, H, W, CUS)


# ---- the code ------------------------------------------------------------------------------------------------------------------------------------------
def test_header_define_and_flag_enum():
    from ukbb_cardiac_amd import deploy_network, engine
    with open(os.path.join(ROOT, 'include', 'ukbb_fcn.h')) as f:
        hdr = f.read()
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r'^#define UKBB_PREC_(\w+) (\d+)$', hdr, re.M)}
    assert codes == {'FP32': 0, 'BF16': 1, 'F32X3': 2, 'BF16_STORE': 3, 'BF16_3D': 4, 'BF16_FULL': 5}
    assert engine._PLAN_PREC['bf16_full'] == 5 and sorted(engine._PLAN_PREC.values()) == list(range(6))
    assert int(re.search(r'#define UKBB_FCN_ABI_VERSION (\d+)', hdr).group(1)) == 11          # additive: no ABI bump
    with open(deploy_network.__file__) as f:
        src = f.read()
    m = re.search(r"DEFINE_enum\('precision', 'fp32', \[([^\]]*)\]", src)
    assert m and [v.strip(" '") for v in m.group(1).split(',')] == ['fp32', 'f32x3', 'bf16_store', 'bf16_full']
    # the header and the flag's help say where the mode rounds and what stays fp32
    doc = hdr[hdr.index('/* UKBB_PREC_BF16_FULL'):hdr.index('#define UKBB_PREC_BF16_FULL')]
    for word in ('bf16(W_s0)', 'bf16(S)', 'bf16(P)', 'RNE', 'logits, prob and pred', 'UKBB_EARCH'):
        assert word in doc, word


@pytest.mark.parametrize('model', FCN_MODELS)
def test_the_plan_is_bf16_stores_plus_the_head_flag(model):
    for n, H, W in PLAN_SHAPES:
        p, s = plan(model, 'bf16_full', n, H, W), plan(model, 'bf16_store', n, H, W)
        assert p['head_bf16'] and p['bfio'] and s['bfio'] and not s['head_bf16']
        assert p['ops'] == s['ops'] and p['acts'] == s['acts'] and p['split'] == s['split']
        assert [o['name'] for o in p['ops']][-2:] == list(F.TAIL_OPS) and [o['kind'] for o in p['ops']][-2:] == ['sqg_multi', 'head']
        for prec in ('fp32', 'bf16', 'f32x3'):
            assert not plan(model, prec, n, H, W)['head_bf16']


@pytest.mark.parametrize('model', ['UNet_ao', 'UNet-LSTM_ao', 'Temporal-UNet_ao'])
def test_the_other_kinds_refuse_the_code(model):
    from ukbb_cardiac_amd import _lib
    with pytest.raises(_lib.UkbbFcnError) as e:
        plan(model, 'bf16_full', 10, 64, 96)
    assert 'failed (-2)' in str(e.value) and "UKBB_PREC_BF16_FULL is the FCN's bf16-storage mode with its head on the bf16 matrix instruction" in str(e.value)   # UKBB_EARCH
    for a in ('UNet-LSTM_ao', 'Temporal-UNet_ao', 'FCN_sa'):                                  # no cine plan under the code
        from ukbb_cardiac_amd.arch import MODELS
        s = _lib.arch_struct(MODELS[a])
        assert _lib.lib.ukbb_fcn_cine_scratch_bytes(Ct.byref(s), 5, 50, 64, 96, 1, 0) == 0


# ---- the packer ----------------------------------------------------------------------------------------------------------------------------------------
def rowmap(r, g):
    return (r & 3) + 8 * (r >> 2) + 4 * g


def bf16_bits(w):
    """The 16-bit patterns of w rounded to bf16, ties to even."""
    u = np.ascontiguousarray(w, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint32) & 0xffff


def fragments_numpy(w, acc_k):
    """The restatement: uint32 [n_out / 32][k_in / 16][64 lanes][4] of the bf16 (ties to even) of w [k_in, n_out]."""
    k_in, n_out = w.shape
    b = bf16_bits(w)
    out = np.zeros((n_out // 32, k_in // 16, 64, 4), np.uint32)
    for cb in range(n_out // 32):
        for kc in range(k_in // 16):
            for lane in range(64):
                m, g = lane & 31, lane >> 5
                for e in range(8):
                    row = 32 * (kc // 2) + rowmap(8 * (kc & 1) + e, g) if acc_k else 16 * kc + 8 * g + e
                    out[cb, kc, lane, e // 2] |= b[row, 32 * cb + m] << np.uint32(16 * (e & 1))
    return out


@pytest.mark.parametrize('k_in,n_out,acc_k', [(16, 32, 0), (32, 64, 1), (64, 64, 1)])
def test_packer_against_the_fragment_order(k_in, n_out, acc_k):
    from ukbb_cardiac_amd import _lib
    fn = _lib.lib.ukbb_fcn_debug_pack_head_bf16
    fn.argtypes = [Ct.POINTER(Ct.c_float), Ct.c_int, Ct.c_int, Ct.c_int, Ct.POINTER(Ct.c_uint32)]
    rng = np.random.default_rng(k_in + n_out)
    w = rng.standard_normal((k_in, n_out)).astype(np.float32)
    w[0, 0], w[1, 1], w[2, 2] = np.float32(1 + 2.0 ** -8), np.float32(1 + 3 * 2.0 ** -8), np.float32(-(1 + 2.0 ** -8 + 2.0 ** -20))    # ties: to even, down and up; past a tie
    want = fragments_numpy(w, acc_k)
    got = np.full(want.shape, 0xdeadbeef, np.uint32)
    assert fn(w.ctypes.data_as(Ct.POINTER(Ct.c_float)), k_in, n_out, acc_k, got.ctypes.data_as(Ct.POINTER(Ct.c_uint32))) == 0
    assert np.array_equal(got, want)
    assert got[0, 0, 0, 0] & 0xffff == 0x3f80                               # 1 + 2^-8 rounds to the even neighbour 1.0
    # every weight appears exactly once, and the accumulator order differs from the natural one (a natural-order pack would not pass for it)
    assert sorted((got & 0xffff).ravel().tolist() + (got >> 16).ravel().tolist()) == sorted(bf16_bits(w).ravel().tolist())
    if acc_k:
        assert not np.array_equal(want, fragments_numpy(w, 0))
    assert fn(w.ctypes.data_as(Ct.POINTER(Ct.c_float)), 24, n_out, acc_k, got.ctypes.data_as(Ct.POINTER(Ct.c_uint32))) == -1       # UKBB_EINVAL


# ---- the grade -----------------------------------------------------------------------------------------------------------------------------------------
def fails(fn, *args):
    try:
        fn(*args)
    except AssertionError:
        return True
    return False


@pytest.fixture(scope='module')
def graded():
    """Per case: (model of the head on the stand-in's inputs, the stand-in's logits, {defect: its logits})."""
    out = []
    for index in range(len(F.CASES)):
        params, conv0, g = F.stand_in_inputs(index)
        model = F.head_model(conv0, g, params)
        out.append((model, F.head_stand_in(conv0, g, params), {d: F.head_stand_in(conv0, g, params, d) for d in F.DEFECTS}))
    return out


def test_stand_in_passes_with_the_floor_met(graded):
    worst = [0.0, 0.0, 1.0]
    for cid, (model, logits, bad) in zip(F.CASE_IDS, graded):
        share, worst_zero, over = F.grade_head(cid, logits, model)
        assert share >= F.ZERO_SLACK_FLOOR and worst_zero <= F.BOUND and over <= F.BOUND
        worst = [max(worst[0], worst_zero), max(worst[1], over), min(worst[2], share)]
    print('stand-in, worst over the cases: err/scale on zero-slack pixels %.2e, (err - slack)/scale %.2e, smallest zero-slack share %.3f' % tuple(worst))


def test_each_planted_defect_misses_the_grade_at_every_case(graded):
    for cid, (model, logits, bad) in zip(F.CASE_IDS, graded):
        for d in F.DEFECTS:
            share, worst_zero, over, inside = F.measure_head(bad[d], model)
            print('%-28s %-26s worst (err - slack)/scale %.2e = %.0f x the bound, %.3f of the pixels inside' % (cid, d, over, over / F.BOUND, inside))
            assert fails(F.grade_head, cid + ' ' + d, bad[d], model), (cid, d)
            assert not worst_zero <= F.BOUND, (cid, d, worst_zero)          # the zero-slack pixels alone tell it: the slack hides nothing


def test_no_case_is_idle():
    want = set().union(*(F.situations(*c) for c in F.CASES))
    only = no_case_is_idle(F.CASES, lambda c: F.situations(*c), want)
    for c, mine in zip(F.CASES, only):
        print('%-36s only it reaches %s' % (c, mine))
    from ukbb_cardiac_amd.arch import MODELS
    assert {MODELS[c[0]].n_class for c in F.CASES} == {2, 3, 4, 6}
    assert {F.seed_of(i) for i in range(len(F.CASES))} == {1234, 7}
    assert all(c[2] % 16 == 0 and c[3] % 16 == 0 for c in F.CASES)
