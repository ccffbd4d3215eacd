"""What the graders of the FCN's --precision bf16_full share (UKBB_PREC_BF16_FULL, include/ukbb_fcn.h; the BM instance of fcn_head_pc_kernel in
kernels_head.hip): the cases, the grades of the encoder and squeeze launches, the float64 interval model of the head, a float32 stand-in of the head with
its planted defects, and the head's tile-walk situations.  A helper module like tests/launch_grading.py (which it imports, and nothing else of tests/):
no tests of its own, ukbb_cardiac_amd imported inside the functions that need it.

THE ENCODER AND THE SQUEEZE are bf16_store's launches, so they are held to bf16_store's grades, restated here: the stem as a unit (stem_reference,
grade_stem: every element within 4 bf16 ulps + the slack of an ambiguous conv0_0 value, 99.5 % within half an ulp), conv1_0 .. conv4_2 within half a
bf16 ulp + 2^-18 |exact| + 2^-20 scale for EVERY element (launch_grading.grade on layer(round_w=True)), g1 .. g4 within 1e-5 of the map's scale of the
fp32 squeeze model in float64 on the stored conv_l.

THE HEAD is graded as a unit against a float64 model of the header's specification, evaluated on the engine's own stored conv0 and g1..g4:

    S = relu(b_s0 + bf16(W_s0) . conv0)             P = relu(T + bf16(W_o0[:, 0:32]) . bf16(S)),  T = b_o0 + sum_l up_l(g_l)
    Q = relu(b_o1 + bf16(W_o1) . bf16(P))           logits = W_lg . Q + b_lg

S and P never reach memory, so an element whose exact value lies next to a bf16 rounding midpoint may round either way in a correct fp32 evaluation.
The model carries an interval (head_model).  A pre-activation is uncertain by  u = slack_in . |bf16(W)| + 2^-18 (|acc| + |x| . |bf16(W)|),  slack_in the
slack of the stage's input x (zero for conv0), the second term K <= 64 exact products accumulated in fp32 plus the fp32 evaluation of T.  An element is
AMBIGUOUS when relu(acc - u) and relu(acc + u) round to different bf16 values; its slack is then the larger distance of the two to the model's rounded
value, and zero otherwise (rounding is monotone: every value of the interval rounds to the model's).  Slack propagates through |bf16(W_o1)|, ReLU
(1-Lipschitz) and |W_lg| to a slack per pixel and class.  Every pixel is graded with  |logits - model| <= 1e-5 scale + slack  (1e-5: the project's fp32
launch bound, of the largest model logit), and at least 40 % of the graded pixels of every case must carry zero slack: those are held to the plain 1e-5.

THE STAND-IN (head_stand_in) is a float32 numpy evaluation of the same specification; tests/test_fcn_bf16_full.py shows that it passes the grade at every
case with the floor met and that each planted defect (DEFECTS) misses it at every case, on the inputs a float64 rounding model of the encoder stores
for the case's own images and weights (stand_in_inputs)."""
import numpy as np

import launch_grading as G
from oracle import fcn_oracle as O

PREC = 'bf16_full'
BOUND = 1e-5                            # g_l and logits: the project's fp32 launch bound, of the launch's scale
PROB_ATOL = 1e-6                        # 16 x 2^-24 = 9.5e-7 (tests/test_head_launches_gpu.py derives it)
ZERO_SLACK_FLOOR = 0.40
ACC_REL = 2.0 ** -18                    # fp32 accumulation of K <= 64 exact products (+ the fp32 evaluation of T), relative to the terms' magnitudes
HEAD_CUS = 256                          # one head workgroup per compute unit of an MI355X
TAIL_OPS = ('sqg1-4', 'head')

# the launcher situations of tests/test_head_launches_gpu.py, restated: model, N, H, W
CASES = [
    ('FCN_sa', 1, 16, 16), ('FCN_sa', 1, 48, 16), ('FCN_sa', 1, 16, 144),
    ('FCN_la_2ch', 3, 80, 112), ('FCN_la_4ch', 3, 80, 112), ('FCN_la_4ch_seg4', 3, 80, 112),
    ('FCN_sa', 1, 256, 256), ('FCN_sa', 1, 272, 304), ('FCN_sa', 17, 256, 256), ('FCN_sa', 17, 240, 256), ('FCN_sa', 17, 32, 32),
]
CASE_IDS = ['%s-%dx%dx%d' % c for c in CASES]
DEFECTS = ('unrounded weights', 'unrounded S', 'unrounded P', 'truncating rounding', 'dropped K chunk of out1', 'fp32 head')


def seed_of(index):
    return G.SEEDS[index % 2]


# ---- the head's tile walk (launch_head_pc: 16 x 16 tiles, one workgroup per compute unit, workgroup b takes tiles b, b + grid, ...) ------------------
def situations(model, n, H, W, cus=HEAD_CUS):
    """What a case reaches of the head launcher: the class count, a lone tile / one tile column / one tile row (windows outside the map on both
    sides), and the fewest and most tiles a workgroup takes behind the small- or the large-batch encoder plan."""
    from ukbb_cardiac_amd.arch import MODELS
    ty, tx = H // 16, W // 16
    ntiles = n * ty * tx
    out = {('classes', MODELS[model].n_class), ('walk', ntiles // cus, -(-ntiles // cus), 'large batch' if n > 16 else 'small batch')}
    if ty == 1 and tx == 1:
        out.add(('map', 'single tile'))
    elif tx == 1:
        out.add(('map', 'one tile column'))
    elif ty == 1:
        out.add(('map', 'one tile row'))
    return out


# ---- float64 pieces of the squeeze and of the head, from stored maps (the float32 BN fold of engine.cpp create()) ------------------------------------
def folded(params, name, dtype=np.float64):
    """The 1 x 1 layer's [Cin, Cout] matrix and bias after launch_grading.fold."""
    w, b = G.fold(params[name])
    assert w.shape[:2] == (1, 1)
    return w[0, 0].astype(dtype), b.astype(dtype)


def squeeze_map(conv_l, params, l, dtype=np.float64):
    """g_l = relu(BN(Ws_l * conv_l)) @ (W0[32 l : 32 l + 32, :] * sc0): the fp32 squeeze launch's specification."""
    w, b = folded(params, 'same_dim%d' % l, dtype)
    return np.maximum(np.asarray(conv_l, dtype) @ w + b, 0) @ folded(params, 'out0', dtype)[0][32 * l:32 * l + 32]


def handed_tile(g, params, dtype=np.float64):
    """T = b_o0 + sum_l up_l(g_l): the reference's un-normalised bilinear transposed convolution (exact weights k / 2^l), in `dtype`."""
    t = None
    for l in range(1, 5):
        u = O.transpose_upsample2d_separable(np.asarray(g[l], dtype), 2 ** l)
        t = u if t is None else t + u
    return t + folded(params, 'out0', dtype)[1]


def softmax64(logits):
    return O.softmax(np.asarray(logits, np.float64))


def bf16_rne64(x):
    """float64 -> the nearest bf16 value (ties to even), as float64, with no float32 step in between."""
    x = np.asarray(x, np.float64)
    a = np.maximum(np.abs(x), 2.0 ** -120)
    ulp = np.exp2(np.floor(np.log2(a)) - 7)
    return np.round(x / ulp) * ulp                                  # numpy rounds halves to even


def bf16_trunc(x):
    """float32 -> bf16 by dropping the low 16 bits (the planted rounding defect)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return (u & np.uint32(0xffff0000)).view(np.float32)


def head_weights(params):
    """(W_s0, b_s0, W_o0[0:32], W_o1, b_o1, W_lg, b_lg) after the fold, float32; the first, third and fourth are what pack_head_bf16 rounds."""
    ws, bs = folded(params, 'same_dim0', np.float32)
    w0 = folded(params, 'out0', np.float32)[0][:32]
    w1, b1 = folded(params, 'out1', np.float32)
    wl, bl = folded(params, 'logits', np.float32)
    return ws, bs, w0, w1, b1, wl, bl


# ---- the interval model ----------------------------------------------------------------------------------------------------------------------------
def _stage(x, slack_in, wb, add):
    """One rounded stage: (model's rounded value, slack).  x the stage's input (float64), wb = bf16(W) as float64, add the bias or T."""
    aw = np.abs(wb)
    acc = x @ wb + add
    u = ACC_REL * (np.abs(acc) + np.abs(x) @ aw)
    if slack_in is not None:
        u = u + slack_in @ aw
    r = bf16_rne64(np.maximum(acc, 0))
    lo, hi = bf16_rne64(np.maximum(acc - u, 0)), bf16_rne64(np.maximum(acc + u, 0))
    return r, np.where(lo != hi, np.maximum(np.abs(lo - r), np.abs(hi - r)), 0.0)


def head_model(conv0, g, params):
    """The float64 model of the specification on stored conv0 [nd,H,W,16] (bf16 values) and g = {l: g_l}: dict(logits, slack [nd,H,W,n_class],
    zero [nd,H,W] = the pixel carries no slack, scale = the largest |logit|, amb = (ambiguous S elements, ambiguous P elements))."""
    ws, bs, w0, w1, b1, wl, bl = head_weights(params)
    f8 = np.float64
    wsb, w0b, w1b = (G.bf16_round(w).astype(f8) for w in (ws, w0, w1))
    s, slack_s = _stage(np.asarray(conv0, f8), None, wsb, bs.astype(f8))
    p, slack_p = _stage(s, slack_s, w0b, handed_tile(g, params))
    q = np.maximum(p @ w1b + b1.astype(f8), 0)
    slack_q = slack_p @ np.abs(w1b)                                 # ReLU is 1-Lipschitz
    logits = q @ wl.astype(f8) + bl.astype(f8)
    slack = slack_q @ np.abs(wl.astype(f8))
    return dict(logits=logits, slack=slack, zero=~(slack_p != 0).any(axis=-1), scale=float(np.abs(logits).max()),
                amb=(int((slack_s != 0).sum()), int((slack_p != 0).sum())))


def measure_head(logits, model):
    """(share of zero-slack pixels, worst |err| / scale on them, worst (|err| - slack) / scale over all pixels, share of pixels inside the bound)."""
    d = np.abs(np.asarray(logits, np.float64) - model['logits'])
    zero = model['zero']
    over = (d - model['slack']) / model['scale']
    inside = (over <= BOUND).all(axis=-1)
    return float(zero.mean()), float(d[zero].max() / model['scale']) if zero.any() else 0.0, float(over.max()), float(inside.mean())


def grade_head(tag, logits, model):
    """Prints the figures, then asserts the grade: the floor of zero-slack pixels and |logits - model| <= 1e-5 scale + slack at every pixel."""
    share, worst_zero, worst, inside = measure_head(logits, model)
    print('fcn-bf16-full %-30s head    zero-slack pixels %.3f, worst err/scale on them %.2e, worst (err - slack)/scale %.2e, inside %.5f '
          '(ambiguous S %d, P %d)' % ((tag, share, worst_zero, worst, inside) + model['amb']))
    assert share >= ZERO_SLACK_FLOOR, '%s: only %.3f of the graded pixels carry zero slack (floor %.2f)' % (tag, share, ZERO_SLACK_FLOOR)
    assert worst <= BOUND, '%s: logits outside 1e-5 scale + slack: worst (err - slack)/scale %.3g, %.5f of the pixels inside' % (tag, worst, inside)
    return share, worst_zero, worst


def grade_outputs(tag, out, nd, model):
    """logits of the graded slices against the model; prob against a float64 softmax of the engine's own logits; pred == argmax(prob) exactly."""
    figs = grade_head(tag, out['logits'][:nd], model)
    perr = float(np.abs(out['prob'].astype(np.float64) - softmax64(out['logits'])).max())
    print('fcn-bf16-full %-30s prob    %.2e (bound %.0e)' % (tag, perr, PROB_ATOL))
    assert perr <= PROB_ATOL, (tag, perr)
    assert np.array_equal(out['pred'], np.argmax(out['prob'], axis=-1).astype(np.int32)), tag + ': pred != argmax(prob)'
    return figs + (perr,)


# ---- the encoder and the squeeze: bf16_store's grades ------------------------------------------------------------------------------------------------
def stem_reference(img, params):
    """The fused stem (kernels_stem.hip) as a unit: image -> bf16, conv0_0 with the bf16 kernel -> bf16 (never stored), conv0_1.  Returns (exact
    conv0_1 output in float64 from the bf16-rounded conv0_0 output, slack).  Where conv0_0's float64 value lies within the worst-case error of an fp32
    sum of its 10 terms (10 x 2^-24 (sum |x||w| + |b|)) of a bf16 rounding boundary a correct kernel may hold either neighbour; slack is one ulp of
    that value x |w| of the tap that reads it, zero elsewhere."""
    w0, b0 = G.fold(params['conv0_0'])
    x, w0 = G.bf16_round(img).astype(np.float64), G.bf16_round(w0).astype(np.float64)
    pre = np.maximum(O.conv2d_same(x, w0, 1) + b0.astype(np.float64), 0.0)
    mag = O.conv2d_same(np.abs(x), np.abs(w0), 1) + np.abs(b0).astype(np.float64)
    ulp = 2 * G.half_ulp(pre)
    q = pre / ulp
    amb = (np.abs(q - np.floor(q) - 0.5) * ulp <= 10 * 2.0 ** -24 * mag) & (pre > 0)
    w1 = G.bf16_round(G.fold(params['conv0_1'])[0]).astype(np.float64)
    slack = O.conv2d_same(np.where(amb, ulp, 0.0), np.abs(w1), 1)
    return G.layer(G.bf16_round(pre.astype(np.float32)), params['conv0_1'], round_w=True), slack


def grade_stem(got, ex, sc, slack):
    got = np.asarray(got, np.float64).reshape(ex.shape)
    tol = G.tolerance(ex, sc, 4.0) + slack
    bad = np.abs(got - ex) > tol
    assert not bad.any(), 'conv0_0+conv0_1: %d elements further than 4 bf16 ulps from the specified result, worst %.3g x the bound' % (
        int(bad.sum()), float((np.abs(got - ex) / tol).max()))
    G.grade('conv0_0+conv0_1 (half ulp)', got, ex, sc, ulps=0.5, fraction=0.995)


def grade_encoder_and_squeeze(arch, params, img, conv, g, report):
    """Every encoder launch and g1..g4 on the graded slices.  Returns the squeeze rows [(launch, figure, bound)]."""
    for lname, sname, l, srcs, stride, transposed, relu in G.launches(arch):
        if lname in ('conv0_0', 'logits'):
            continue
        if lname == 'conv0_1':
            ex, slack = stem_reference(img, params)
            sc = float(np.abs(ex).max())
            report.row(lname, conv[sname], ex, sc)
            grade_stem(conv[sname], ex, sc, slack)
            continue
        ex = G.layer(conv[srcs[0]], params[lname], stride, round_w=True)
        sc = float(np.abs(ex).max())
        report.row(lname, conv[sname], ex, sc)
        G.grade('%s (tiling %d)' % (lname, report.op_of[lname]['cfg']), conv[sname], ex, sc, ulps=0.5, fraction=1.0)
    rows = [('g%d' % l, G.rel_err(g[l], squeeze_map(conv['conv%d' % l], params, l))[0], BOUND) for l in range(1, 5)]
    for launch, fig, bound in rows:
        print('fcn-bf16-full %-30s %-7s %.2e (bound %.0e)' % (report.tag, launch, fig, bound))
    bad = [r for r in rows if not r[1] <= r[2]]
    assert not bad, 'squeeze launches over their bound (launch, figure, bound): %s' % (bad,)
    return rows


# ---- the stand-in ------------------------------------------------------------------------------------------------------------------------------------
def case_inputs(index):
    """(arch, params, normalised batch, number of distinct images) of case `index`, as the GPU grader feeds it."""
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.weights import synthetic_params
    model, n, H, W = CASES[index]
    arch = MODELS[model]
    img, nd = G.normalised_copies(index, n, H, W)
    return arch, synthetic_params(arch, seed_of(index)), img, nd


def stand_in_inputs(index):
    """What the mode's encoder and squeeze store in front of the head for case `index`, by their rounding model on the CPU: every encoder map the
    float64 result of layer(round_w=True) on the map before it, rounded once to bf16; g_l the fp32 squeeze in float32.  -> (params, conv0, g)."""
    arch, params, img, nd = case_inputs(index)
    w0, b0 = G.fold(params['conv0_0'])
    x = G.bf16_round(img[:nd]).astype(np.float64)
    a00 = np.maximum(O.conv2d_same(x, G.bf16_round(w0).astype(np.float64), 1) + b0.astype(np.float64), 0.0)
    stored = {}
    for lname, sname, l, srcs, stride, transposed, relu in G.launches(arch):
        if lname in ('conv0_0', 'logits'):
            continue
        src = G.bf16_round(a00.astype(np.float32)) if lname == 'conv0_1' else stored[srcs[0]]
        stored[sname] = G.bf16_round(G.layer(src, params[lname], stride, round_w=True).astype(np.float32))
    g = {l: squeeze_map(stored['conv%d' % l], params, l, np.float32) for l in range(1, 5)}
    assert all(v.dtype == np.float32 for v in g.values())
    return params, stored['conv0'], g


def head_stand_in(conv0, g, params, defect=None):
    """A float32 numpy evaluation of the head's specification (every sum in float32, in numpy's order), or of one planted defect of DEFECTS."""
    assert defect is None or defect in DEFECTS
    f4 = np.float32
    ws, bs, w0, w1, b1, wl, bl = head_weights(params)
    rw = (lambda w: w) if defect in ('unrounded weights', 'fp32 head') else G.bf16_round
    rnd = bf16_trunc if defect == 'truncating rounding' else G.bf16_round
    x = np.asarray(conv0, f4)
    s = np.maximum(x @ rw(ws) + bs, f4(0))
    if defect not in ('unrounded S', 'fp32 head'):
        s = rnd(s)
    p = np.maximum(handed_tile(g, params, f4) + s @ rw(w0), f4(0))
    if defect not in ('unrounded P', 'fp32 head'):
        p = rnd(p)
    w1r = rw(w1)
    if defect == 'dropped K chunk of out1':
        w1r = w1r.copy()
        w1r[16:32] = 0                                              # chunk 1 of P0: the rows its registers 8..15 hold
    q = np.maximum(p @ w1r + b1, f4(0))
    out = q @ wl + bl
    assert out.dtype == f4
    return out
