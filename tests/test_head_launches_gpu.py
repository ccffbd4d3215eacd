"""The FCN squeeze launches (sqg1-4: sqg_multi_kernel, sqg_body / sqg_stream_body) and the head launch (fcn_head_pc_kernel, kernels_head.hip), one launch
at a time, against float64 on the engine's OWN stored inputs -- the graders' common method (tests/launch_grading.py) and the bound of
tests/test_fp32_launches_gpu.py, which stops in front of them.

One forward per case and mode.  From what the engine stored (Engine.activation), in numpy float64 with the float32 BN fold of engine.cpp create():

    g_l     expected  relu(BN(Ws_l * conv_l)) @ (W0[32 l : 32 l + 32, :] * sc0)  from the stored conv_l, l = 1..4       max |engine - f64| <= 1e-5 max |f64|
    logits  expected  out0 pre-activation  b0' + W0'[0:32] relu(BN(Ws_0 * conv0)) + sum_l up_l(g_l)  from the stored conv0 and the stored g_1..g_4
            (up_l: oracle/fcn_oracle.py transpose_upsample2d_separable, the reference's un-normalised bilinear transposed convolution, in float64),
            then ReLU, out1, ReLU, logits + bias: the head as a unit, the map between same_dim0 and out0 never being stored     <= 1e-5 of the logits' scale
    prob    against a float64 softmax of the engine's own float32 logits, <= 1e-6 absolute.  p <= 1; the rounding of l - m enters as
            |x| e^-|x| 2^-24 <= 0.37 x 2^-24; expf, the sum, the reciprocal and the product cost a few ulp each: 16 x 2^-24 covers that for up to 6
            classes (tests/test_head_launch_coverage.py: a float32 numpy softmax of the same form passes, one bf16 ulp in one exponential does not)
    pred    == argmax(prob) over the engine's float32 prob, lowest index on ties, exactly;  == argmax(logits) wherever the engine's top-two logit gap
            is >= 4e-7 (the contract at softmax_argmax, kernels.h);  the pred-only call (want_logits=False, want_prob=False) gives the same map bit for
            bit;  against the float64 logits a label may differ only where the float64 top-two margin is <= 2e-5 of the logits' scale

Every case runs in fp32, in f32x3 and in bf16 on the same handle, with the same bounds (include/ukbb_fcn.h promises fp32-grade results for f32x3).  In
bf16 (UKBB_PREC_BF16 on an FCN handle: bf16-operand convs, fp32 maps in HBM; engine.cpp switches the head for f32x3 only) the squeeze and the head are
the fp32 launches, fed by maps the bf16-operand convs stored (those are graded in tests/test_bf16_operand_launches_gpu.py); everything here is graded
from the engine's own stored conv0..4 and g1..4, so the same bounds hold.  Inputs as in
the fp32 launch test (batch_of_copies): slices 0-2 are graded in float64 and every other slice of g1..g4, logits, prob and pred must be BIT-IDENTICAL
to the graded copy of its image; weights from seeds 1234 and 7 in turn.
Each case asserts that the plan it ran holds sqg1-4 and head.

CASES: the smallest maps that reach each situation of the squeeze launcher (launch_sqg_multi: one wave per 32-pixel block, four per workgroup, at most
2048 workgroups per level, above which the bodies loop) and of the head's tile walk (one workgroup per CU, 256 here; workgroup b takes tiles b,
b + 256, ...; two stages per 16 x 16 tile; windows of 9 / 6 / 4 / 3 source rows and columns with out-of-map rows zero-filled).  The situations are
computed on the host by tests/test_head_launch_coverage.py, which also shows that dropping any one case leaves a situation unreached ([*] = the
situation only this case reaches):

    case  model             N    H    W  tiles  reaches
       0  FCN_sa            1   16   16      1  [*] single tile (level maps of 64, 16, 4, 1 pixels; most of the 3 x 3 level-4 window outside the map);
                                                partial 32-pixel blocks (`valid` mask) in sqg_stream_body (level 2) and in sqg_body (levels 3, 4), as in 1-5 and 7
       1  FCN_sa            1   48   16      3  [*] one tile column, three tile rows: window columns outside the map on both sides at levels 2-4 (level-4 map 3 x 1)
       2  FCN_sa            1   16  144      9  [*] one tile row, nine tile columns: window rows outside on both sides at levels 2-4 (level-4 map 1 x 9)
       3  FCN_la_2ch        3   80  112    105  [*] 2 classes; a 32-pixel squeeze block spanning two images (level 4: 35 pixels per image); odd level-4 map (5 x 7)
       4  FCN_la_4ch        3   80  112    105  [*] 3 classes
       5  FCN_la_4ch_seg4   3   80  112    105  [*] 6 classes
       6  FCN_sa            1  256  256    256  [*] as many tiles as workgroups
       7  FCN_sa            1  272  304    323  odd level-4 map (17 x 19); more tiles than workgroups at N = 1: [*] workgroups with two tiles (even) and, in the
                                                same launch, with exactly one (the flush after the loop, next to workgroups still in it)
       8  FCN_sa           17  256  256   4352  [*] squeeze loop past the cap (level 1: 278 528 pixels against 2048 x 4 x 32 = 262 144); 17 tiles per workgroup
                                                (odd, >= 3), consecutive tiles of a workgroup in different images; large-batch conv plan in front
       9  FCN_sa           17  240  256   4080  [*] squeeze grid just under the cap, no loop (level 1: 261 120 pixels, 2040 workgroups); workgroups with 16 and
                                                with 15 tiles in one launch, consecutive tiles at different positions of different images
      10  FCN_sa           17   32   32     68  [*] large-batch conv plan in front of a map with fewer tiles than workgroups; squeeze blocks spanning 2 and 8
                                                images (levels 3 and 4: 16 and 4 pixels per image)
    4 classes, fewer tiles than workgroups and workgroups with exactly one tile are reached by cases 0-2 and 10 alike.

Non-default launches: the knobs are latched per process, so for each of UKBB_SIDE_STREAM=1 (stand-alone sqg_stream_kernel<32/64> and
sqg_kernel<128/256>), UKBB_HEAD_DIRECT_GATHER=1 and UKBB_HEAD_INLINE_TAIL=1 one fresh child process grades cases 0, 2 and 5 in the same way with the same
bounds, after asserting that it ran the form meant (kernel_names() / ukbb_fcn_head_tail_form()).  If the A/B tests ever fail, this tells which side is
wrong.

Measured on an MI355X (profiles/head_launches.txt, one row per graded launch and mode, worst per launch kind, level and mode in its last block), worst
over the 11 cases, fp32 / f32x3: g1 3.2e-7, g2 3.1e-7, g3 3.6e-7, g4 6.8e-7 of the map's scale (the squeeze is the same launch in both modes); logits
5.7e-7 / 6.7e-7 of their scale; prob 1.6e-7 / 1.6e-7 absolute; no label differing from the float64 argmax, no copy differing, no defect found.  The
three children measure the same or less on their cases.  In bf16 (behind the bf16-operand encoder): g1 3.4e-7, g2 2.9e-7, g3 3.5e-7, g4 4.8e-7, logits
5.6e-7, prob 1.6e-7, no label differing.  The 11 cases take 3 s together in fp32 and f32x3 (0.34 s of forwards and read-back, 1.6 s of float64; the
largest 0.8 s) and 4.5 s with bf16 (the largest 1.3 s), each child 3 s, most of it starting Python."""
import json
import os
import time

import numpy as np
import pytest

from launch_grading import SEEDS, batch_of_copies, check_copies, config_name, fold, rel_err, run_in_child
from oracle import fcn_oracle as O

pytestmark = pytest.mark.gpu
BOUND = 1e-5                            # g_l and logits: the project's fp32 launch bound, of the launch's scale
PROB_ATOL = 1e-6                        # 16 x 2^-24 = 9.5e-7, see above
NEAR_TIE_GAP = 4e-7                     # kernels.h softmax_argmax
LABEL_MARGIN = 2e-5                     # of the float64 logits' scale: two fp32-grade evaluations, 1e-5 each
MODES = ('fp32', 'f32x3', 'bf16')
CHILD_MODES = ('fp32', 'f32x3')         # the knob children stay on the two modes whose head launches differ

CASES = [
    ('FCN_sa', 1, 16, 16), ('FCN_sa', 1, 48, 16), ('FCN_sa', 1, 16, 144),
    ('FCN_la_2ch', 3, 80, 112), ('FCN_la_4ch', 3, 80, 112), ('FCN_la_4ch_seg4', 3, 80, 112),
    ('FCN_sa', 1, 256, 256), ('FCN_sa', 1, 272, 304), ('FCN_sa', 17, 256, 256), ('FCN_sa', 17, 240, 256), ('FCN_sa', 17, 32, 32),
]
CHILD_CASES = (0, 2, 5)                 # the reduced list of the non-default launches
KNOBS = ('UKBB_SIDE_STREAM', 'UKBB_HEAD_DIRECT_GATHER', 'UKBB_HEAD_INLINE_TAIL')


# ---- the float64 reference of the squeeze and of the head, from stored maps -------------------------------------------------------------------------
def folded(params, name, dtype=np.float64):
    """The 1 x 1 layer's [Cin, Cout] matrix and bias after the float32 BN fold of engine.cpp create() (tests/launch_grading.py fold)."""
    w, b = fold(params[name])
    assert w.shape[:2] == (1, 1)
    return w[0, 0].astype(dtype), b.astype(dtype)


def same_dim(x, params, l, dtype=np.float64):
    """relu(BN(Ws_l * x)): common/network.py:201-204 on the given conv_l."""
    w, b = folded(params, 'same_dim%d' % l, dtype)
    return np.maximum(np.asarray(x, dtype) @ w + b, 0)


def out0_slice(params, l, dtype=np.float64):
    """out0's rows of level l after the fold: W0[32 l : 32 l + 32, :] * sc0."""
    return folded(params, 'out0', dtype)[0][32 * l:32 * l + 32]


def squeeze_map(conv_l, params, l, dtype=np.float64):
    """g_l: out0's level-l slice applied at low resolution (it commutes with the channel-diagonal upsampling)."""
    return same_dim(conv_l, params, l, dtype) @ out0_slice(params, l, dtype)


def upsample(g, l):
    """up_l: the reference's un-normalised bilinear transposed convolution by 2^l, in g's own type (exact weights k / 2^l)."""
    return O.transpose_upsample2d_separable(g, 2 ** l)


def head_logits(conv0, g, params, dtype=np.float64, up=upsample, term0=None):
    """The head as a unit: logits from conv0 and g = {1: g_1, .., 4: g_4}.  ``up`` and ``term0`` (level 0's out0 term) exist so that
    tests/test_head_launch_coverage.py can plant defects."""
    pre = same_dim(conv0, params, 0, dtype) @ out0_slice(params, 0, dtype) if term0 is None else np.asarray(term0, dtype)
    pre = pre + folded(params, 'out0', dtype)[1]
    for l in range(1, 5):
        pre = pre + up(np.asarray(g[l], dtype), l)
    x = np.maximum(pre, 0)
    w1, b1 = folded(params, 'out1', dtype)
    x = np.maximum(x @ w1 + b1, 0)
    wl, bl = folded(params, 'logits', dtype)
    return x @ wl + bl


def softmax64(logits):
    return O.softmax(np.asarray(logits, np.float64))


def top2_gap(logits):
    srt = np.sort(logits, axis=-1)
    return srt[..., -1] - srt[..., -2]


# ---- one case, every mode, on one handle ---------------------------------------------------------------------------------------------------------------
def grade_case(index, want_names=('sqg1-4', 'head'), tail_form=None, modes=MODES):
    """Runs case ``index`` in every mode of ``modes``, prints one line per graded launch and mode, asserts everything the module docstring lists.
    Returns the rows [(mode, launch, figure, where)]."""
    from ukbb_cardiac_amd import _lib, engine
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.weights import synthetic_params
    model, n, H, W = CASES[index]
    seed = SEEDS[index % 2]
    arch = MODELS[model]
    params = synthetic_params(arch, seed)
    img, nd = batch_of_copies(index, n, H, W)
    tag = 'head-launch %-15s %2dx%3dx%3d seed %4d' % (model, n, H, W, seed)
    rows, failures = [], []
    t_gpu = t_ref = 0.0
    prev = None                                                          # (stored inputs, expected maps) of the mode before: same inputs, same reference
    with engine.Engine(arch, params) as eng:
        for mode in modes:
            t0 = time.perf_counter()
            eng.set_precision(mode)
            out = eng.run(img, want_logits=True, want_prob=True, want_pred=True)
            names, cfgs = eng.kernel_names(), eng.kernel_configs()
            form = int(_lib.lib.ukbb_fcn_head_tail_form())
            conv = {l: eng.activation('conv%d' % l).reshape(n, H >> l, W >> l, -1) for l in range(5)}
            g = {l: eng.activation('g%d' % l).reshape(n, H >> l, W >> l, 64) for l in range(1, 5)}
            only = eng.run(img, want_logits=False, want_prob=False, want_pred=True)
            t_gpu += time.perf_counter() - t0
            for nm in want_names:
                assert nm in names, (mode, nm, names)
            # bf16: the maps the squeeze and the head read were stored by bf16-operand convs, every one from conv1_0 on
            on_bf16 = [config_name(c).startswith('convBF16_') for nm, c in zip(names, cfgs) if nm.startswith('conv') and '+' not in nm]
            assert len(on_bf16) == 11 and all(v == (mode == 'bf16') for v in on_bf16), (mode, list(zip(names, cfgs)))
            if tail_form is not None and mode == 'fp32':                 # f32x3 keeps the in-stage tail in every form
                assert form == tail_form, (form, tail_form)
            logits, prob, pred = out['logits'], out['prob'], out['pred']
            assert logits.shape == (n, H, W, arch.n_class) and prob.shape == logits.shape and pred.shape == (n, H, W)
            assert [conv[l].shape[-1] for l in range(5)] == list(arch.n_filter)
            # every slice is a bit-identical copy of the graded slice of its image
            for sname, a in [('g%d' % l, g[l]) for l in range(1, 5)] + [('logits', logits), ('prob', prob), ('pred', pred)]:
                check_copies('%s %s' % (mode, sname), a, nd)
            # pred: exact statements on the engine's own outputs, all N slices
            assert np.array_equal(pred, np.argmax(prob, axis=-1).astype(np.int32)), mode + ': pred != argmax(prob)'
            clear = top2_gap(logits) >= np.float32(NEAR_TIE_GAP)
            assert np.array_equal(pred[clear], np.argmax(logits, axis=-1).astype(np.int32)[clear]), mode + ': pred != argmax(logits) away from a near-tie'
            assert only['pred'].dtype == pred.dtype and np.array_equal(only['pred'], pred), mode + ': the pred-only call gives another label map'
            t0 = time.perf_counter()
            stored = [conv[l][:nd] for l in range(5)] + [g[l][:nd] for l in range(1, 5)]
            if prev is not None and all(np.array_equal(a, b) for a, b in zip(stored, prev[0])):
                ex_g, ex_logits = prev[1]
            else:
                ex_g = {l: squeeze_map(conv[l][:nd], params, l) for l in range(1, 5)}
                ex_logits = head_logits(conv[0][:nd], {l: g[l][:nd] for l in range(1, 5)}, params)
                prev = (stored, (ex_g, ex_logits))
            for l in range(1, 5):
                err, where = rel_err(g[l][:nd], ex_g[l])
                rows.append((mode, 'g%d' % l, err, where, BOUND))
            err, where = rel_err(logits[:nd], ex_logits)
            rows.append((mode, 'logits', err, where, BOUND))
            d = np.abs(prob.astype(np.float64) - softmax64(logits))
            rows.append((mode, 'prob', float(d.max()), tuple(int(v) for v in np.unravel_index(int(d.argmax()), d.shape)), PROB_ATOL))
            # labels against the float64 logits: only inside the margin two fp32-grade evaluations leave
            differ = pred[:nd] != np.argmax(ex_logits, axis=-1)
            margin = top2_gap(ex_logits) / float(np.abs(ex_logits).max())
            worst = float(margin[differ].max()) if differ.any() else 0.0
            rows.append((mode, 'pred', worst, (int(differ.sum()),), LABEL_MARGIN))
            t_ref += time.perf_counter() - t0
    for mode, launch, fig, where, bound in rows:
        if launch == 'pred':
            print('%s %-5s pred    %d labels differ from argmax(float64 logits), largest float64 margin / scale there %.2e' % (tag, mode, where[0], fig))
        elif launch == 'prob':
            print('%s %-5s prob    max |engine - float64 softmax of its logits| %.2e  worst at %s' % (tag, mode, fig, where))
        else:
            print('%s %-5s %-7s err/scale %.2e  worst at %s' % (tag, mode, launch, fig, where))
        if not fig <= bound:
            failures.append((mode, launch, fig, where, bound))
    print('%s forward + read-back %.2f s, float64 reference %.2f s' % (tag, t_gpu, t_ref))
    assert not failures, 'over the bound (mode, launch, figure, worst element [slice, y, x, channel], bound): %s' % (failures,)
    return rows


@pytest.mark.parametrize('index', range(len(CASES)), ids=['%s-%dx%dx%d' % c for c in CASES])
def test_squeeze_and_head_launches_against_float64_on_their_own_inputs(index):
    grade_case(index)


# ---- non-default launches: one child process per knob --------------------------------------------------------------------------------------------------
def run_child(knob, path):
    """In a process started with ``knob``=1: grade CHILD_CASES, after checking that the form meant is the one that runs."""
    assert os.environ.get(knob) == '1' and not [k for k in os.environ if k.startswith('UKBB_') and k != knob]
    want = ('sqg1', 'sqg2', 'sqg3', 'sqg4', 'head') if knob == 'UKBB_SIDE_STREAM' else ('sqg1-4', 'head')
    # the fp32 head reports the in-stage form (1) under either head knob, the deferred default (0) otherwise (kernels_head.hip launch_head_pc_nc)
    form = 0 if knob == 'UKBB_SIDE_STREAM' else 1
    rows = []
    for index in CHILD_CASES:
        rows += [(index,) + r[:3] for r in grade_case(index, want, form, CHILD_MODES)]
    with open(path, 'w') as f:
        json.dump(rows, f)


@pytest.mark.parametrize('knob', KNOBS)
def test_non_default_launches_against_float64(knob, tmp_path):
    path = str(tmp_path / 'rows.json')
    r = run_in_child('test_head_launches_gpu', 'run_child', [knob, path], {knob: '1'})
    print(''.join(knob + '=1 ' + ln + '\n' for ln in r.stdout.splitlines() if ln.startswith('head-launch')), end='')
    assert r.returncode == 0, r.stdout[-3000:]
    with open(path) as f:
        rows = json.load(f)
    assert len(rows) == len(CHILD_CASES) * len(CHILD_MODES) * 7 and {r[0] for r in rows} == set(CHILD_CASES)
