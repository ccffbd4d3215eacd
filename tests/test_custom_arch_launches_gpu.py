"""Every launch of the 2-D architectures ukbb_fcn_create accepts beyond the named models (tests/custom_archs.py: other class counts, blocks per level
and pyramids of the FCN, the U-Net and the UNet-LSTM -- what tf_checkpoint.infer_arch builds from a user's checkpoint), one launch at a time, against
float64 on the engine's OWN stored inputs.  The other launch graders run the entries of arch.MODELS only.

The method is the graders' common one (tests/launch_grading.py): one forward per case on an engine created under UKBB_DEBUG_GUARD and poisoned in front
of the forward, inputs from batch_of_copies (fp32 maps) or normalised_copies (bf16 maps), weights from seeds 1234 and 7 in turn, the plan that ran being
the plan tests/test_custom_arch_launch_coverage.py counted (assert_plan_ran), every stored map read back, slices 0..2 recomputed alone in float64 from
the map or maps the engine stored in front of the launch, every further slice bit-identical to its copy, bf16 maps holding bf16 values only, no poison
left and no guard damaged.  Each launch is held to the bound of the grader of its precision, imported and not restated:

    fp32 conv / transposed conv / logits / first, the fused first layer as a unit     1e-5 of the layer's scale (tests/test_fp32_launches_gpu.py BOUND)
    bf16-storage conv / transposed conv / first (U-Net kinds under bf16; FCN bf16_store, bf16_full)   grade(ulps = 0.5, fraction = 1.0): EVERY element
    the fused stem and the fused tail as units                                        stem_reference / grade_stem, tail_reference / grade_tail of
                                                                                      tests/test_bf16_launches_gpu.py
    FCN bf16 (operands)                                                               1e-5 against the rounded-operand model and >= 1e-4 from the fp32 model
                                                                                      (tests/test_bf16_operand_launches_gpu.py BOUND, APART)
    FCN f32x3 with set_f32x3_convs                                                    1e-5 and the RMS ratio R of tests/f32x3_convs_grading.py
    g1..g4 (sqg1-4 or the per-level sqg launches), the head's logits                  squeeze_map / head_logits and BOUND of tests/test_head_launches_gpu.py;
                                                                                      bf16_full: head_model / grade_outputs of tests/fcn_bf16_full_grading.py
    prob, pred (FCN and U-Net)                                                        PROB_ATOL of a float64 softmax of the engine's own logits; pred == argmax(prob)
                                                                                      exactly, over all slices

Two launches no named model's default plan holds have no grader of their own:
  * the separate bf16 `logits` launch (n_block[0] == 1: logits_kernel<16, C, IBF>) widens the stored bf16 up0 exactly and is an fp32 launch on it: 1e-5;
  * the conv with the logits in its epilogue (n_block[0] == 3 under bf16: tilings 325 and 404) never stores its own output: it rounds it to bf16 "as a store
    would have" and multiplies by the logits weights (404: entered as bf16 hi + lo pieces).  It is graded as a unit against exactly that in float64:
    |logits - model| <= 1e-5 of the logits' scale + slack, the slack being (one bf16 ulp of an up0 value) x |w| summed over the values whose float64
    pre-rounding result lies within the fp32 accumulation allowance of tolerance() (2^-18 |exact| + 2^-20 scale) of a rounding boundary, where a correct
    kernel may hold either neighbour -- zero everywhere else; and to grade_tail's figures, the tail being the same unit one layer longer.

UNet-LSTM cases run run_seq; their U-Net part is graded as above.  In fp32 the sequence's logits are compared with O.unet_lstm in float64 end to end,
within 1e-3 of the oracle's scale (the figure of tests/test_gpu_parity.py).  Under bf16 no end-to-end figure separates a right engine from a wrong one (see
below), so the ConvLSTM behind the custom U-Net is graded launch by launch as well (grade_convlstm), with the models and the bf16 conditions of
tests/test_lstm_launches_gpu.py, from the engine's own stored up0, lstm:gx, lstm:h1 and lstm:hall: the x pass from the stored up0 of every frame (the
hand-off from the U-Net: decoded gx within half a bf16 ulp on every element; h1 within one ulp + 1e-5 on every element and 99.9 % within half an ulp),
every step launch of both directions from the stored previous hidden map (the same two conditions), lstm_out's logits from the stored hidden maps within
1e-5 of their scale.  The end-to-end deviation under bf16 is printed: it is the accumulation of the specified roundings of some forty bf16-stored maps,
2e-2 .. 1.1e-1 of the scale on these cases (the largest at LSTM-wide 9 x 144 x 144, where every launch from the stem to lstm_out is inside its bound on
its own input); the NAMED UNet-LSTM_ao on the same rough copies measures 2.5e-2 .. 7.3e-2, on a smooth phantom cine 1.7e-2 .. 5.5e-2 (the 0.08 of
tests/test_unidirectional_lstm.py is for such a cine at 48 x 64), with 99.3 % of the labels equal to the float64 argmax.

End to end, one test per architecture in fp32: logits within 1e-3 of the float64 oracle's scale (O.build_FCN / O.UNet / O.unet_lstm with the
descriptor's n_filter and n_block), labels identical except where the float64 top-two margin is below 1e-4 (tests/test_gpu_parity.py).
FCN-wide and FCN-big are refusal cases: plan.cpp supported() refuses an FCN pyramid the squeeze kernels have no instance for, Engine raises with the
reason, and a named model runs afterwards in the same process.

CASES: a greedy cover, cheapest first (pixels + 25 x float64 pixels; 32 x 48 and 64 x 96 preferred), of the situations (tests/custom_archs.py) the plans of
ARCHS hold over the SHAPES of tests/test_plan_layout.py at batches 1 and 17 and the named models' plans do not; N = 1 or 17 (UNet-LSTM: one or two
sequences of 9 frames), H and W multiples of 16 up to 96 x 128 -- except for the 71 situations no such map reaches (tilings the planner takes only on large
maps: 5, 23, 29, 31, 200, 210, 211, 230, 240, 241, 250, 251, 330-344 at the new channel pairs), which take the smallest map that does (40 cases, up to
192 x 208 and 128 x 256 at N = 1, nine frames of them for the UNet-LSTM); maps below 32 x 48 (deepest map 2 x 3) only where nothing larger within the
limit reaches the situation (5 cases); reduced until no case is idle.  The coverage file prints what only each case reaches.

Measured on an MI355X: profiles/custom_arch_launches.txt, one row per launch (case, layer, tiling, channels, deviation over its bound).  Every launch
inside its imported bound, none widened: fp32 convs / transposed convs / first / logits <= 1.5e-6 of their scale (worst: tilings 23, 5, 305, 29 at
96 and 160 channels), the three- and five-group Winograd launches 301 / 303 <= 1e-6, the two-source convs of K = 9 x 192 and 9 x 320 and the transposed
convs 160 -> 96, 96 -> 160, 96 -> 32 likewise; every element of every bf16-storing launch within the half-ulp grade (worst / tolerance 0.999); bf16
operands <= 4.2e-7; f32x3 convs at most 0.66 of their two bounds; g1..g4 <= 4.5e-7, head logits <= 7.9e-7, prob <= 2.1e-7; the fused-logits convs 325 /
404 within 8e-8 of the logits' scale beyond their slack, 91-94 % of the pixels carrying none; the tail <= 0.09 of its 2e-2; no copy differing, no guard
damaged; the bf16 ConvLSTM behind the custom U-Nets: no gx element outside half an ulp, h1 and every step map at most 0.5 of the one-ulp condition,
lstm_out 2.2e-7.  The 93 cases, 12 end-to-end tests and the refusal test take 30 s together; the largest cases are LSTM-wide bf16 9 x 128 x 256 (3.9 s,
3.5 s of it float64) and 9 x 208 x 144 (3.6 s), then LSTM-wide fp32 9 x 192 x 208 (2.4 s)."""
import time

import numpy as np
import pytest

import custom_archs as A
import f32x3_convs_grading as X
import fcn_bf16_full_grading as F
import launch_grading as G
import test_bf16_launches_gpu as B                                  # the stem and the tail as units
import test_bf16_operand_launches_gpu as OP                         # BOUND, APART, is_bf16_tiling
import test_fp32_launches_gpu as FP                                 # BOUND
import test_head_launches_gpu as HL                                 # the squeeze and head models and their bounds
import test_lstm_launches_gpu as LL                                 # the ConvLSTM's launch models, its bf16 conditions and PROB_ATOL
from oracle import fcn_oracle as O

pytestmark = pytest.mark.gpu
BOUND = FP.BOUND
E2E_LOGITS, E2E_MARGIN = 1e-3, 1e-4                                 # tests/test_gpu_parity.py

CASES = [
    ('FCN-c5', 'bf16', 1, 32, 48), ('FCN-c5', 'bf16_full', 1, 80, 64), ('FCN-c5', 'bf16_store', 1, 80, 64), ('FCN-c5', 'f32x3c', 1, 32, 48),
    ('FCN-c5', 'fp32', 17, 32, 64), ('FCN-nb1', 'bf16', 1, 32, 48), ('FCN-nb1', 'bf16_full', 1, 32, 48), ('FCN-nb1', 'bf16_store', 1, 32, 48),
    ('FCN-nb1', 'f32x3c', 1, 32, 48), ('FCN-nb1', 'fp32', 1, 32, 48), ('FCN-nb3', 'bf16', 1, 32, 48), ('FCN-nb3', 'bf16_full', 1, 32, 48),
    ('FCN-nb3', 'bf16_full', 1, 32, 64), ('FCN-nb3', 'bf16_full', 1, 48, 80), ('FCN-nb3', 'bf16_store', 1, 32, 48),
    ('FCN-nb3', 'bf16_store', 1, 32, 64), ('FCN-nb3', 'bf16_store', 1, 48, 80), ('FCN-nb3', 'f32x3c', 1, 32, 48), ('FCN-nb3', 'fp32', 1, 32, 48),
    ('FCN-flat', 'bf16', 1, 32, 48), ('FCN-flat', 'bf16', 1, 128, 256), ('FCN-flat', 'bf16', 1, 144, 16), ('FCN-flat', 'bf16', 1, 192, 208),
    ('FCN-flat', 'bf16_full', 1, 32, 48), ('FCN-flat', 'bf16_full', 1, 80, 144), ('FCN-flat', 'bf16_full', 1, 128, 256),
    ('FCN-flat', 'bf16_full', 1, 144, 144), ('FCN-flat', 'bf16_full', 1, 192, 208), ('FCN-flat', 'bf16_store', 1, 32, 48),
    ('FCN-flat', 'bf16_store', 1, 80, 144), ('FCN-flat', 'bf16_store', 1, 128, 256), ('FCN-flat', 'bf16_store', 1, 144, 144),
    ('FCN-flat', 'bf16_store', 1, 192, 208), ('FCN-flat', 'f32x3c', 1, 32, 48), ('FCN-flat', 'f32x3c', 1, 128, 256),
    ('FCN-flat', 'f32x3c', 1, 176, 208), ('FCN-flat', 'f32x3c', 1, 192, 208), ('FCN-flat', 'fp32', 1, 32, 48), ('FCN-flat', 'fp32', 1, 128, 128),
    ('FCN-flat', 'fp32', 1, 144, 144), ('FCN-flat', 'fp32', 1, 192, 208), ('UNet-c2', 'bf16', 1, 80, 64), ('UNet-c2', 'fp32', 17, 32, 64),
    ('UNet-c4', 'bf16', 1, 32, 48), ('UNet-c4', 'fp32', 1, 32, 48), ('UNet-nb1', 'bf16', 1, 32, 48), ('UNet-nb1', 'fp32', 1, 32, 48),
    ('UNet-nb3', 'bf16', 1, 32, 48), ('UNet-nb3', 'bf16', 1, 32, 64), ('UNet-nb3', 'bf16', 1, 48, 80), ('UNet-wide', 'bf16', 1, 16, 144),
    ('UNet-wide', 'bf16', 1, 32, 48), ('UNet-wide', 'bf16', 1, 48, 80), ('UNet-wide', 'bf16', 1, 64, 48), ('UNet-wide', 'bf16', 1, 80, 80),
    ('UNet-wide', 'bf16', 1, 128, 256), ('UNet-wide', 'bf16', 1, 144, 144), ('UNet-wide', 'bf16', 1, 208, 144), ('UNet-wide', 'fp32', 1, 32, 48),
    ('UNet-wide', 'fp32', 1, 64, 96), ('UNet-wide', 'fp32', 1, 80, 80), ('UNet-wide', 'fp32', 1, 128, 128), ('UNet-wide', 'fp32', 1, 144, 16),
    ('UNet-wide', 'fp32', 1, 144, 144), ('UNet-wide', 'fp32', 1, 192, 208), ('UNet-flat', 'bf16', 1, 32, 48), ('UNet-flat', 'bf16', 1, 32, 80),
    ('UNet-flat', 'bf16', 1, 48, 64), ('UNet-flat', 'bf16', 1, 128, 256), ('UNet-flat', 'bf16', 1, 144, 144), ('UNet-flat', 'bf16', 1, 192, 208),
    ('UNet-flat', 'bf16', 1, 208, 144), ('UNet-flat', 'fp32', 1, 32, 48), ('UNet-flat', 'fp32', 1, 128, 128), ('UNet-flat', 'fp32', 1, 144, 144),
    ('UNet-flat', 'fp32', 1, 192, 208), ('LSTM-wide', 'bf16', 9, 16, 144), ('LSTM-wide', 'bf16', 9, 32, 48), ('LSTM-wide', 'bf16', 9, 48, 80),
    ('LSTM-wide', 'bf16', 9, 64, 48), ('LSTM-wide', 'bf16', 9, 80, 80), ('LSTM-wide', 'bf16', 9, 128, 256), ('LSTM-wide', 'bf16', 9, 144, 144),
    ('LSTM-wide', 'bf16', 9, 208, 144), ('LSTM-wide', 'fp32', 9, 32, 48), ('LSTM-wide', 'fp32', 9, 64, 96), ('LSTM-wide', 'fp32', 9, 80, 80),
    ('LSTM-wide', 'fp32', 9, 128, 128), ('LSTM-wide', 'fp32', 9, 144, 16), ('LSTM-wide', 'fp32', 9, 144, 144), ('LSTM-wide', 'fp32', 9, 192, 208),
    ('LSTM-nb', 'bf16', 9, 32, 48), ('LSTM-nb', 'fp32', 9, 32, 48),
]
E2E_ARCHS = [k for k in A.ARCHS if k not in A.REFUSED]


def engine_precision(prec):
    return 'f32x3' if prec == 'f32x3c' else prec


# ---- the conv with the logits in its epilogue, as a unit --------------------------------------------------------------------------------------------
def fused_logits_reference(x, params, lname, split):
    """(float64 logits of the specified arithmetic, slack) of `lname` + logits on the stored input x: the conv's result rounded to bf16 and never
    stored, then the 1 x 1 logits conv on it with fp32 weights (325) or with the weights entered as bf16 hi + lo pieces (split: 404, kernels_ws.hip LG)."""
    pre = G.layer(x, params[lname], round_w=True)
    sc = float(np.abs(pre).max())
    r = G.bf16_round(pre.astype(np.float32)).astype(np.float64)
    w = params['logits']['kernel'].astype(np.float32).reshape(pre.shape[-1], -1)
    if split:
        hi = G.bf16_round(w)
        w = hi.astype(np.float64) + G.bf16_round(w - hi).astype(np.float64)
    w = w.astype(np.float64)
    ulp = 2 * G.half_ulp(pre)
    q = pre / ulp
    amb = (np.abs(q - np.floor(q) - 0.5) * ulp <= np.abs(pre) * 2.0 ** -18 + sc * 2.0 ** -20) & (pre > 0)
    return r @ w + params['logits']['bias'].astype(np.float64), np.where(amb, ulp, 0.0) @ np.abs(w)


# ---- one case -----------------------------------------------------------------------------------------------------------------------------------------
class Rows:
    """One printed row per launch, as measured; the failures are raised after the last one."""

    def __init__(self, tag, acts):
        self.tag, self.acts, self.rows, self.failures = tag, acts, [], []

    def channels(self, o):
        def ch(i):
            return self.acts[i]['channels'] if i >= 0 else 0
        return '%3d+%3d->%3d' % (ch(o['in0']), ch(o['in1']), ch(o['out']))

    def add(self, o, what, dev, note='', ok=True):
        cfg = o['cfg'] if o['kind'] in ('conv', 'tconv') else -1
        self.rows.append((what, cfg, dev))
        print('custom-arch %-32s %-20s %-9s tiling %3d  %s  deviation / bound %.3f  %s' % (self.tag, what, o['kind'], cfg, self.channels(o), dev, note))
        if not (dev <= 1.0 and ok):
            self.failures.append((what, cfg, dev, note))

    def note(self, what, dev, note='', ok=True):
        """A launch that is no op of the U-Net's plan (the ConvLSTM behind it)."""
        self.rows.append((what, -1, dev))
        print('custom-arch %-32s %-20s %-9s deviation / bound %.3f  %s' % (self.tag, what, 'convlstm', dev, note))
        if not (dev <= 1.0 and ok):
            self.failures.append((what, dev, note))

    def guard(self, o, what, fn, *args):
        """An imported grade that asserts: run it, keep its message as a failure."""
        try:
            fn(*args)
        except AssertionError as e:
            self.failures.append((what, o['cfg'], str(e)[:300]))


def grade_conv(rows, o, lname, x, got, p, stride, transposed, relu, prec, bfio):
    cfg = o['cfg']
    if bfio:                                                             # a bf16-storing launch: half a bf16 ulp of the specified arithmetic, every element
        ex = G.layer(x, p, stride, transposed, relu, round_w=True)
        share, worst = G.measure(got, ex, float(np.abs(ex).max()))
        rows.add(o, lname, worst, 'within half an ulp %.6f' % share)
    elif prec == 'bf16' and OP.is_bf16_tiling(cfg):                      # bf16 operands, fp32 maps
        err = G.rel_err(got, G.layer(x, p, stride, transposed, relu, round_w=True, round_x=True))[0]
        apart = G.rel_err(got, G.layer(x, p, stride, transposed, relu))[0]
        rows.add(o, lname, err / OP.BOUND, 'from the fp32 model %.2e' % apart, apart >= OP.APART)
    elif prec == 'f32x3c' and cfg in X.X3_TILINGS:                       # three bf16 pieces per operand
        err, ratio = X.grades(got, G.layer(x, p, stride), X.fp32_launch(x, p, stride))
        rows.add(o, lname, max(err / X.BOUND, ratio / X.R), 'err/scale %.2e rms ratio %.2f' % (err, ratio))
    else:
        rows.add(o, lname, G.rel_err(got, G.layer(x, p, stride, transposed, relu))[0] / BOUND)


STEP_BAND = 48                                                       # rows of a step launch graded on a map taller than this


def read_convlstm(eng, lp, NF, T, H, W):
    """What the bf16 ConvLSTM stored behind the U-Net (tests/test_lstm_launches_gpu.py run_engine): the features of every frame, h1, hall, the decoded gx."""
    Wn = NF // T
    r = dict(feat=eng.activation('up0').reshape(NF, H, W, LL.NH))
    r['h1'] = LL.widen(eng.activation('lstm:h1'), 2 * NF * H * W * LL.NH, True).reshape(2, NF, H, W, LL.NH)
    r['hall'] = LL.widen(eng.activation('lstm:hall'), 2 * T * Wn * H * W * LL.NH, True).reshape(2, T, Wn, H, W, LL.NH)
    r['hall'][0, 0] = r['hall'][1, T - 1] = 0.0                         # never written: those first steps live in h1
    r['gx'] = None
    if lp['bf_hoist']:
        raw = eng.activation('lstm:gx')
        r['gx'] = LL.decode_gx_wino(raw, NF, H, W, lp['tile_cols']) if lp['bf_wino'] else LL.decode_gx_ws(raw, NF, H, W)
    return r


def grade_convlstm(rows, r, params, lp, out, T):
    """The bf16 ConvLSTM behind a custom U-Net, each launch alone in float64 from the engine's own stored maps, with the models and the bf16 conditions of
    tests/test_lstm_launches_gpu.py: the x pass from the stored up0 of EVERY frame over the whole map (the hand-off from the U-Net: decoded gx within half
    a bf16 ulp on every element, h1 holding the two conditions of holds() against the model that applies -- gates rounded first where gx is kept); each
    step launch of both directions from the stored previous hidden map (every element within one ulp + 1e-5, 99.9 % within half an ulp); lstm_out's
    logits from the stored hidden maps within 1e-5 of their scale.  On a map taller than STEP_BAND rows the step launches are graded on rows
    0 .. STEP_BAND - 1, recomputed from rows 0 .. STEP_BAND of the stored maps -- exact, every input being a stored map and the cell state being carried
    per pixel -- which keeps the float64 cost of the large cases at a second; the x pass and lstm_out cover the whole map."""
    feat = r['feat'].astype(np.float64)
    NF, H, W = feat.shape[:3]
    Wn = NF // T
    wmap = np.arange(T)[:, None] + T * np.arange(Wn)[None, :]           # run_seq: step k of window w is frame w T + k
    assert np.array_equal(r['feat'], G.bf16_round(r['feat']))
    R = min(H, STEP_BAND)
    Rin = min(H, R + 1)
    for d, name in enumerate(('lstm_fw', 'lstm_bw')):
        kernel, bias = G.fold(params[name])
        if not lp['bf_wino']:
            kernel = G.bf16_round(kernel)
        kernel, bias = kernel.astype(np.float64), bias.astype(np.float64)
        gx_exact = LL.gate_conv(feat, kernel[:, :, :LL.NH]) + bias
        gxs = None if r['gx'] is None else r['gx'][d].astype(np.float64)
        if gxs is not None:
            sc = float(np.abs(gx_exact).max())
            share, worst = G.measure(gxs, gx_exact, sc)
            rows.note('gx dir %d' % d, worst, 'within half an ulp %.6f' % share, LL.passes('gx', gxs, gx_exact, sc, 1.0))
        ex = LL.cell(gx_exact if gxs is None else gxs, 0.0)[0]
        dev = float((np.abs(r['h1'][d].astype(np.float64) - ex) / (2 * G.half_ulp(ex) + LL.ULP_ATOL)).max())
        rows.note('h1 dir %d' % d, dev, 'outside half an ulp %.2e' % (1.0 - LL.share_half_ulp(r['h1'][d], ex)), LL.holds('h1', r['h1'][d], ex))
        steps = LL.direction_launches(d, feat[:, :Rin], r['h1'][d][:, :Rin].astype(np.float64), r['hall'][d][:, :, :Rin].astype(np.float64), wmap, kernel, bias,
                                      gx_stored=None if gxs is None else gxs[:, :Rin], first_from_stored=True)
        for kind, n_, k, exact, got, S in steps:
            if kind != 'step':
                continue
            got32, ex = r['hall'][d][k][:, :R], exact[:, :R]
            dev = float((np.abs(got32.astype(np.float64) - ex) / (2 * G.half_ulp(ex) + LL.ULP_ATOL)).max())
            rows.note('step %d dir %d' % (n_, d), dev, 'outside half an ulp %.2e' % (1.0 - LL.share_half_ulp(got32, ex)), LL.passes('step', got32, ex))
    hf, hb = LL.step_maps(r['h1'].astype(np.float64), r['hall'].astype(np.float64), wmap)
    lg64 = LL.out_logits(hf, hb, params['lstm_out']).transpose(1, 0, 2, 3, 4)            # [Wn][T][H][W][C]
    rows.note('lstm_out', float(np.abs(out['logits'] - lg64).max() / np.abs(lg64).max()) / LL.BOUND)


def run_case(index, monkeypatch):
    from ukbb_cardiac_amd.weights import synthetic_params
    name, prec, n, H, W = CASES[index]
    arch, kind = A.arch_of(name), A.kind_of(name)
    params = synthetic_params(arch, G.SEEDS[index % 2])
    plan = A.plan(name, prec, n, H, W)
    ops, acts, bfio = plan['ops'], plan['acts'], plan['bfio']
    assert bfio == (prec in ('bf16_store', 'bf16_full') or (prec == 'bf16' and kind != 'FCN')) and plan['head_bf16'] == (prec == 'bf16_full')
    assert plan.get('conv_x3', False) == (prec == 'f32x3c')
    img, nd = (G.normalised_copies if bfio else G.batch_of_copies)(index, n, H, W)
    graph = G.launches(arch)
    by_name = {gr[0]: gr for gr in graph}
    stored_names = {a['name'] for a in acts}
    tag = '%s %s %dx%dx%d' % (name, prec, n, H, W)
    maps, g = {}, {}
    t0 = time.perf_counter()
    with G.guarded_engine(monkeypatch, arch, params, engine_precision(prec)) as eng:
        if prec == 'f32x3c':
            eng.set_f32x3_convs(True)
        eng.reserve(n, H, W)
        eng.poison(G.POISON)
        if kind == 'UNet-LSTM':
            out = eng.run_seq(img.reshape(n // arch.fc, arch.fc, H, W, 1), want_logits=True, want_prob=True, want_pred=True)
        else:
            out = eng.run(img, want_logits=True, want_prob=True, want_pred=True)
        G.assert_plan_ran(eng, plan)                                     # the plan tests/test_custom_arch_launch_coverage.py counted for this case
        for lname, sname, l, _, _, _, _ in graph:
            if sname in stored_names and sname not in maps:
                a = eng.activation(sname).reshape(n, H >> l, W >> l, -1)
                if bfio:
                    G.check_bf16(sname, a)
                G.check_copies(sname, a, nd, tag)                        # no poison left, every further slice bit-identical to its copy
                maps[sname] = a[:nd].copy()
        if kind == 'FCN':
            for l in range(1, 5):
                a = eng.activation('g%d' % l).reshape(n, H >> l, W >> l, 64)
                G.check_copies('g%d' % l, a, nd, tag)
                g[l] = a[:nd].copy()
        lstm = read_convlstm(eng, plan['lstm'], n, arch.fc, H, W) if kind == 'UNet-LSTM' and bfio else None
        damaged, where = eng.check_guards()
        assert damaged == 0, where
    for k in ('logits', 'prob', 'pred'):
        assert np.isfinite(out[k]).all(), (tag, k)
        if kind != 'UNet-LSTM':                                          # a frame's output depends on its place in the sequence
            G.check_copies(k, out[k], nd, tag)
    t_gpu = time.perf_counter() - t0
    t0 = time.perf_counter()
    rows = Rows(tag, acts)
    x0 = img[:nd]
    for o in ops:
        parts = o['name'].split('+')
        if o['kind'] == 'first':                                         # conv0_0 as a launch of its own (n_block[0] == 1): fp32 arithmetic on the image
            got = maps[by_name['conv0_0'][1]]
            if bfio:
                ex = G.layer(x0, params['conv0_0'])
                share, worst = G.measure(got, ex, float(np.abs(ex).max()))
                rows.add(o, 'conv0_0', worst, 'within half an ulp %.6f' % share)
            else:
                rows.add(o, 'conv0_0', G.rel_err(got, G.layer(x0, params['conv0_0']))[0] / BOUND)
        elif parts[:2] == ['conv0_0', 'conv0_1']:                        # the first two layers as a unit
            assert len(parts) == 2 and o['kind'] in ('stem', 'conv')
            got = maps[by_name['conv0_1'][1]]
            if bfio:
                ex, slack, _ = B.stem_reference(x0, params, o['kind'])
                sc = float(np.abs(ex).max())
                rows.add(o, o['name'], float((np.abs(got.astype(np.float64) - ex) / (G.tolerance(ex, sc, 4.0) + slack)).max()),
                         'within half an ulp %.6f' % G.measure(got, ex, sc)[0])
                rows.guard(o, o['name'], B.grade_stem, got, ex, sc, slack)
            else:
                rows.add(o, o['name'], G.rel_err(got, G.layer(G.layer(x0, params['conv0_0']), params['conv0_1']))[0] / BOUND)
        elif o['kind'] in ('conv', 'tconv') and parts[-1] == 'logits':  # up0_k + logits: the conv's own output is never stored
            assert len(parts) == 2 and bfio and kind == 'UNet'
            _, _, _, srcs, stride, transposed, relu = by_name[parts[0]]
            ex, slack = fused_logits_reference(np.concatenate([maps[s] for s in srcs], axis=-1), params, parts[0], split=o['cfg'] >= 400)
            lsc = float(np.abs(ex).max())
            err = np.abs(out['logits'][:nd].astype(np.float64) - ex)
            rows.add(o, o['name'], float(((err - slack) / (BOUND * lsc)).max()), 'pixels with zero slack %.3f' % float(np.mean(slack.max(-1) == 0)))
            rows.guard(o, o['name'], B.grade_tail, out['logits'][:nd], out['pred'][:nd], ex)
        elif o['kind'] in ('conv', 'tconv'):
            _, sname, _, srcs, stride, transposed, relu = by_name[o['name']]
            if kind == 'FCN' and prec == 'bf16' and not o['name'].startswith('conv0_'):
                assert OP.is_bf16_tiling(o['cfg']), o
            grade_conv(rows, o, o['name'], np.concatenate([maps[s] for s in srcs], axis=-1), maps[sname], params[o['name']], stride, transposed, relu, prec, bfio)
        elif o['kind'] == 'logits':                                      # the U-Net's 1 x 1 logits launch, from the stored up0 (bf16 values widened exactly)
            x = maps[by_name['logits'][3][0]]
            rows.add(o, 'logits', G.rel_err(out['logits'][:nd], G.layer(x, params['logits'], relu=False))[0] / BOUND)
        elif o['kind'] == 'tail':
            ex = B.tail_reference(np.concatenate([maps['conv0'], maps['up0_t']], axis=-1), params)
            lsc = float(np.abs(ex).max())
            err = np.abs(out['logits'][:nd].astype(np.float64) - ex)
            rows.add(o, o['name'], float(err.max() / (2e-2 * lsc)), 'logits within 2e-4 %.6f' % float(np.mean(err <= 2e-4 * lsc)))
            rows.guard(o, o['name'], B.grade_tail, out['logits'][:nd], out['pred'][:nd], ex)
        elif o['kind'] in ('sqg', 'sqg_multi'):
            levels = range(1, 5) if o['kind'] == 'sqg_multi' else [int(o['name'][3:])]
            for l in levels:
                rows.add(o, 'g%d' % l, G.rel_err(g[l], HL.squeeze_map(maps['conv%d' % l], params, l))[0] / HL.BOUND)
        elif o['kind'] == 'head':
            if prec == 'bf16_full':
                model = F.head_model(maps['conv0'], g, params)
                share, worst_zero, worst, inside = F.measure_head(out['logits'][:nd], model)
                rows.add(o, 'head', worst / F.BOUND, 'zero-slack pixels %.3f' % share, share >= F.ZERO_SLACK_FLOOR)
            else:
                rows.add(o, 'head', G.rel_err(out['logits'][:nd], HL.head_logits(maps['conv0'], g, params))[0] / HL.BOUND)
        else:
            raise AssertionError('a launch this grader does not know: %s' % (o,))
    # prob and pred, over all slices
    atol = LL.PROB_ATOL if kind == 'UNet-LSTM' else HL.PROB_ATOL
    perr = float(np.abs(out['prob'].astype(np.float64) - HL.softmax64(out['logits'])).max())
    print('custom-arch %-32s prob %.2e (bound %.0e)' % (tag, perr, atol))
    if not perr <= atol:
        rows.failures.append(('prob', perr, atol))
    assert np.array_equal(out['pred'], np.argmax(out['prob'], axis=-1).astype(np.int32)), tag + ': pred != argmax(prob)'
    if lstm is not None:
        grade_convlstm(rows, lstm, params, plan['lstm'], out, arch.fc)
    if kind == 'UNet-LSTM':                                              # the sequence end to end against float64
        ref = O.unet_lstm(img.reshape(n // arch.fc, arch.fc, H, W, 1), params, arch.n_hidden, n_filter=arch.n_filter, n_block=arch.n_block, dtype=np.float64)
        dev = float(np.abs(out['logits'] - ref).max() / np.abs(ref).max())
        print('custom-arch %-32s sequence logits against float64, err/scale %.2e%s' % (tag, dev, '' if bfio else ' (bound %.0e)' % E2E_LOGITS))
        if not bfio and not dev <= E2E_LOGITS:
            rows.failures.append(('sequence logits', dev, E2E_LOGITS))
    print('custom-arch %-32s forward, read-back and identity %.2f s, float64 %.2f s' % (tag, t_gpu, time.perf_counter() - t0))
    assert not rows.failures, 'launches outside their bound: %s' % (rows.failures,)
    return plan, rows.rows


@pytest.mark.parametrize('index', range(len(CASES)), ids=['%s-%s-%dx%dx%d' % c for c in CASES])
def test_each_launch_of_a_custom_architecture_against_float64_on_its_own_input(index, monkeypatch):
    plan, rows = run_case(index, monkeypatch)
    graded = {r[0] for r in rows}
    for o in plan['ops']:                                                # every launch of the plan has its row
        want = ['g%d' % l for l in range(1, 5)] if o['kind'] == 'sqg_multi' else ['g' + o['name'][3:]] if o['kind'] == 'sqg' else \
            ['conv0_0'] if o['kind'] == 'first' else [o['name']]
        assert set(want) <= graded, (o, sorted(graded))


# ---- end to end, fp32 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', E2E_ARCHS)
def test_custom_architecture_end_to_end_against_the_float64_oracle(name):
    from ukbb_cardiac_amd.engine import Engine
    from ukbb_cardiac_amd.weights import synthetic_params
    arch, kind = A.arch_of(name), A.kind_of(name)
    params = synthetic_params(arch, 1234)
    H, W = 32, 48
    with Engine(arch, params) as eng:
        if kind == 'UNet-LSTM':
            img = G.batch_of_copies(0, arch.fc, H, W)[0].reshape(1, arch.fc, H, W, 1)
            out = eng.run_seq(img, want_logits=True)
            ref = O.unet_lstm(img, params, arch.n_hidden, n_filter=arch.n_filter, n_block=arch.n_block, dtype=np.float64)
        else:
            img = G.batch_of_copies(0, 3, H, W)[0]
            out = eng.run(img, want_logits=True)
            ref = O.build_FCN(img, params, arch.n_class, n_filter=arch.n_filter, n_block=arch.n_block, dtype=np.float64) if kind == 'FCN' else \
                O.UNet(img, params, arch.n_class, n_filter=arch.n_filter, n_block=arch.n_block, dtype=np.float64)
    scale = float(np.abs(ref).max())
    err = float(np.abs(out['logits'] - ref).max())
    bad = out['pred'] != O.argmax_pred(ref)
    print('custom-arch %-10s end to end: logits err/scale %.2e, %d labels differ, largest float64 margin there %.2e' % (
        name, err / scale, int(bad.sum()), float(O.top2_margin(ref)[bad].max()) if bad.any() else 0.0))
    assert out['logits'].shape == ref.shape and err <= E2E_LOGITS * scale, (err, scale)
    assert np.all(O.top2_margin(ref)[bad] < E2E_MARGIN), 'labels differ from the float64 oracle away from a tie'


# ---- the refused FCN pyramids ---------------------------------------------------------------------------------------------------------------------------
def test_refused_fcn_pyramids_raise_with_the_reason_and_a_named_model_still_runs():
    from ukbb_cardiac_amd import _lib
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.engine import Engine
    from ukbb_cardiac_amd.weights import synthetic_params
    for name, why in A.REFUSED.items():
        arch = A.arch_of(name)
        with pytest.raises(_lib.UkbbFcnError) as e:
            Engine(arch, synthetic_params(arch, 1234))
        assert why in str(e.value), str(e.value)
    arch = MODELS['FCN_sa']
    params = synthetic_params(arch, 1234)
    img = G.batch_of_copies(0, 2, 32, 48)[0]
    with Engine(arch, params) as eng:
        out = eng.run(img, want_logits=True)
    ref = O.build_FCN(img, params, arch.n_class, dtype=np.float64)
    assert float(np.abs(out['logits'] - ref).max()) <= E2E_LOGITS * float(np.abs(ref).max())
