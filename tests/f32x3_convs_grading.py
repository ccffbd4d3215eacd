"""What the tests of ukbb_fcn_set_f32x3_convs share (tests/test_f32x3_convs.py on the CPU, tests/test_f32x3_convs_launches_gpu.py and
tests/test_f32x3_convs_gpu.py on the GPU): the numpy model of the three-piece launch (kernels_conv_x3.hip), its planted defects, the fp32 model of the
same launch, the two grades, the cases of the launch grader and the planner side of their coverage count.  Built on tests/launch_grading.py.

THE MODEL (x3_launch).  The folded kernel and the stored fp32 input are each split into three bf16 pieces, h = bf16(v), m = bf16(v - h),
l = bf16(v - h - m), round to nearest even, the residuals formed in float32 (exact).  Per 16-channel chunk (outer) and filter tap (inner) six terms
add into one float32 accumulator in the kernel's order -- weight piece . activation piece: l.h, h.l, m.m, m.h, h.m, h.h -- each term the EXACT sum of
its 16 products (a product of two bf16 values is exact in float32; the sum is formed in float64) rounded into the accumulator once, as one matrix
instruction does.  Then + bias, ReLU, in float32.  fp32_launch is the same walk with unsplit operands: one term per (chunk, tap).

THE GRADES of one launch, both against float64 on the launch's own stored input (launch_grading.layer):
  1. every element within BOUND = 1e-5 of the layer's scale max |float64| -- the bound of the fp32 launch graders;
  2. the RMS error at most R times the RMS error of fp32_launch on the same input.
Grade 1 cannot see a dropped small term (a dropped l.h, h.l or m.m moves an element by some 1e-6 of the scale); grade 2 can.  R is not taken from
what the engine gives: tests/test_f32x3_convs.py computes, on the chain of real layers below, the worst ratio of the correct model and the mildest
planted defect's ratio, asserts that R is their geometric mean and lies a factor >= 2 from either, and the GPU tests read the constant here."""
import os

import numpy as np

import launch_grading as G

BOUND = 1e-5
R = 5.79                                # asserted by tests/test_f32x3_convs.py::test_R_is_the_geometric_mean_and_a_factor_two_from_either_side
PIECES = ('h', 'm', 'l')
TERMS = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))          # (weight piece, activation piece): l.h h.l m.m m.h h.m h.h
TERM_NAMES = tuple('%s.%s' % (PIECES[a], PIECES[b]) for a, b in TERMS)
DEFECTS = tuple('%s dropped' % t for t in TERM_NAMES) + ('l pieces absent', 'h.h only', 'weights split but activations not', 'one zeroed tap',
                                                           'input shifted by a pixel')
MODEL = 'FCN_sa'
LAYERS = tuple('conv%d_%d' % (l, i) for l, nb in ((1, 2), (2, 3), (3, 3), (4, 3)) for i in range(nb))       # the eleven launches
X3_TILINGS = (330, 332, 334, 335, 340, 342, 344, 345)
PROFILE = os.path.join(G.ROOT, 'profiles', 'f32x3_convs.txt')

# The cases of tests/test_f32x3_convs_launches_gpu.py: (model, N, H, W), batches of 1 and of plan.h SMALL_BATCH + 1.  The first six are the shapes the
# feature was specified with and stay as specified; the rest is what the coverage count of tests/test_f32x3_convs.py asks for on top of them -- the
# smallest maps on which the chooser puts EVERY tiling of the family on a map its tiles divide, on ragged edge tiles and on a single partial tile,
# at both batch classes, and that reach every (layer, tiling, fit, batch class) of the switch-on plans at the recorded shapes.  No added case is idle
# (test_no_added_case_is_idle prints what only each reaches).
CASES = [
    ('FCN_sa', 1, 32, 48), ('FCN_sa', 17, 32, 48),                # 8 x 16: ragged at level 1, the deep levels single partial tiles
    ('FCN_sa', 1, 80, 112), ('FCN_sa', 17, 80, 112),              # 8 x 16: ragged at levels 1-3, a single partial tile at level 4
    ('FCN_la_2ch', 1, 192, 208), ('FCN_la_2ch', 1, 176, 208),     # 8 x 16 dividing / ragged at levels 1-3, 12 x 13 / 11 x 13 dividing (one tile) at level 4
    ('FCN_sa', 1, 48, 16), ('FCN_sa', 17, 48, 16),                # level 1 a single partial 8 x 16 tile, level 2 a single partial 12 x 13 tile
    ('FCN_sa', 1, 48, 80), ('FCN_sa', 17, 48, 80),                # level 2 is 12 x 20: two 12 x 13 tiles (330 / 340), the second ragged along x
    ('FCN_sa', 1, 80, 16), ('FCN_sa', 17, 80, 16),                # 11 x 13 as a single partial tile (level 3, 10 x 2) and ragged along y (342 at level 2, 20 x 4)
    ('FCN_sa', 1, 80, 144), ('FCN_sa', 17, 80, 144),              # level 3 is 10 x 18: two 11 x 13 tiles (332 / 342), partial along y and ragged along x
    ('FCN_sa', 1, 208, 16), ('FCN_sa', 17, 208, 16),              # one tile column: ragged along y alone
    ('FCN_sa', 1, 128, 256), ('FCN_sa', 17, 128, 256),            # 8 x 16 tiles divide every map
    ('FCN_sa', 17, 192, 208), ('FCN_sa', 17, 176, 208),           # the first six's dividing tiles in the large batch class
]
SPECIFIED = CASES[:6]
FITS = ('div', 'ragged', 'partial')


# ---- the arithmetic ------------------------------------------------------------------------------------------------------------------------------------
def split3(v):
    """(h, m, l) as float32 arrays: split_pair of device_prims.h / pack_conv_x3."""
    v = np.ascontiguousarray(v, np.float32)
    h = G.bf16_round(v)
    r = (v - h).astype(np.float32)
    m = G.bf16_round(r)
    q = (r - m).astype(np.float32)
    return h, m, G.bf16_round(q)


def taps_of(x, stride):
    """[(kh, kw, the input patch of every output pixel at that tap [N, Ho, Wo, C])] under TF 'SAME' zero padding, 3 x 3."""
    n, H, W, c = x.shape
    Ho, Wo = -(-H // stride), -(-W // stride)
    ph, pw = max((Ho - 1) * stride + 3 - H, 0), max((Wo - 1) * stride + 3 - W, 0)
    xp = np.pad(x, ((0, 0), (ph // 2, ph - ph // 2), (pw // 2, pw - pw // 2), (0, 0)))
    return [(kh, kw, xp[:, kh:kh + (Ho - 1) * stride + 1:stride, kw:kw + (Wo - 1) * stride + 1:stride, :]) for kh in range(3) for kw in range(3)]


def accumulate(x_pieces, w_pieces, terms, stride, zero_tap=None):
    """The float32 accumulator after every (chunk, tap, term): each term's 16 products summed exactly, one float32 rounding per term."""
    cin, cout = w_pieces[0].shape[2:]
    taps = [taps_of(np.asarray(xp, np.float64), stride) for xp in x_pieces]
    w64 = [np.asarray(wp, np.float64) for wp in w_pieces]
    acc = np.zeros(taps[0][0][2].shape[:3] + (cout,), np.float32)
    for c0 in range(0, cin, 16):
        for t in range(9):
            kh, kw = t // 3, t % 3
            if (kh, kw) == zero_tap:
                continue
            for wi, xi in terms:
                part = taps[xi][t][2][..., c0:c0 + 16] @ w64[wi][kh, kw, c0:c0 + 16, :]
                acc = (acc.astype(np.float64) + part).astype(np.float32)
    return acc


def finish(acc, b):
    y = np.maximum((acc + b).astype(np.float32), np.float32(0))
    assert y.dtype == np.float32
    return y


def x3_launch(x, p, stride, defect=None):
    """One three-piece launch in float32 numpy as the engine is specified to run it -- with one planted defect, if any."""
    w, b = G.fold(p)
    x = np.ascontiguousarray(x, np.float32)
    if defect == 'input shifted by a pixel':
        x = np.concatenate([np.zeros_like(x[:, :, :1]), x[:, :, :-1]], axis=2)
    terms = list(TERMS)
    if defect in DEFECTS[:6]:
        terms.pop(DEFECTS.index(defect))
    elif defect == 'l pieces absent':
        terms = [t for t in TERMS if 2 not in t]
    elif defect == 'h.h only':
        terms = [(0, 0)]
    elif defect == 'weights split but activations not':           # the activations as their first piece alone
        terms = [t for t in TERMS if t[1] == 0]
    return finish(accumulate(split3(x), split3(w), terms, stride, (0, 2) if defect == 'one zeroed tap' else None), b)


def fp32_launch(x, p, stride):
    """The fp32 model of the same launch: unsplit float32 operands, float32 accumulation per 16-channel chunk and tap."""
    w, b = G.fold(p)
    return finish(accumulate([np.ascontiguousarray(x, np.float32)], [w], [(0, 0)], stride), b)


def rms(d):
    return float(np.sqrt(np.mean(np.square(np.asarray(d, np.float64)))))


def grades(got, exact, fp32_model):
    """(max |got - exact| / scale, rms(got - exact) / rms(fp32_model - exact)): grade 1 holds the first to BOUND, grade 2 the second to R."""
    scale = float(np.abs(exact).max())
    return float(np.abs(np.asarray(got, np.float64) - exact).max()) / scale, rms(np.asarray(got, np.float64) - exact) / rms(np.asarray(fp32_model, np.float64) - exact)


# ---- the planner side ----------------------------------------------------------------------------------------------------------------------------------
def plan(model, n, H, W, on=True, precision='f32x3'):
    from ukbb_cardiac_amd import engine
    from ukbb_cardiac_amd.arch import MODELS
    return engine.plan_layout(MODELS[model], precision, n, H, W, G.CUS, f32x3_convs=on)


def small_batch():
    import re
    with open(os.path.join(G.ROOT, 'ukbb_cardiac_amd', 'csrc', 'plan.h')) as f:
        return int(re.search(r'constexpr int SMALL_BATCH = (\d+);', f.read()).group(1))


def batch_class(n):
    return 'small' if n <= small_batch() else 'large'


def reached(model, n, H, W):
    """{(layer, tiling, fit, batch class)} of the switch-on plan's eleven three-piece launches."""
    ops = [o for o in plan(model, n, H, W)['ops'] if o['kind'] == 'conv' and o['name'] in LAYERS]
    assert len(ops) == 11 and all(o['cfg'] in X3_TILINGS for o in ops), ops
    return {(o['name'], o['cfg'], G.fit_of(o), batch_class(n)) for o in ops}
