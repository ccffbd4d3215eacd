"""Every ConvLSTM launch of UNet-LSTM_ao (the reference's default aortic model), fp32 and bf16, one launch at a time, against float64 on the engine's
OWN stored input -- what tests/test_fp32_launches_gpu.py and tests/test_bf16_layers_gpu.py do for the conv launches in front of it.

One run_seq or run_cine per case on synthetic weights.  Read back: 'up0' (the features the ConvLSTM consumed), 'lstm:h1' ([dir][NF][H][W][16], the x
pass's per-frame first step), 'lstm:hall' ([dir][T][Wn][H][W][16]; slot k = 0 of the forward and k = T - 1 of the backward direction are never written:
those first steps live in h1 and are gathered through the window map) and, in bf16, 'lstm:gx' (lane-native, decoded here).  Each launch is then
recomputed ALONE in numpy float64 (reference common/network_ao.py:255-319, tf.contrib.rnn.Conv2DLSTMCell: gate order i, j, f, o, forget bias 1):

    x pass          z = W_x * feat + b per frame and direction; c1, h1 from the zero state.
    step launch n   (n = 2..T of a direction, all windows w, frame = map[k][w]):  z = gx[frame] + W_h * h_prev, h_prev being the ENGINE's stored
                    previous hidden map (step 2: h1 gathered through the map, later: hall);  c' = sigmoid(f + 1) c + sigmoid(i) tanh(j),
                    h' = tanh(c') sigmoid(o).
    cell state      the engine keeps only the last c, so it cannot be read back per step: it is carried in float64 along the same chain of
                    engine-stored h's.  A launch's c' shows in that launch's own h'; c IS GRADED THROUGH h ONLY.
    window map      written here with oracle aortic_window_indices (run_cine) or w T + k (run_seq), not copied from the engine's cine_tables.
    lstm_out        (run_seq) logits = W_out . concat(h_fw[k][w], h_bw[k][w]) + b from the stored h1 / hall; prob, pred.
    lstm_tile       (run_cine) prob against a float64 restatement of deploy_network_ao.py:129-183 fed with float64 softmax(out_conv(stored h)).

The gate conv is one float64 im2col product (gate_conv; test_gate_conv_is_conv2d_same holds it to oracle conv2d_same): conv2d_same takes 0.5 s per
step launch of case D.

Bounds.  fp32: max |h - h64| <= n x 1e-5 x S for the direction's n-th cell update (n = 1: the x pass), S = max(1, max |z64|) the scale of that launch's
gate pre-activations; 1e-5 is the project's per-launch fp32 bound (test_fp32_launches_gpu.BOUND); sigmoid and tanh have slope <= 1, so a
pre-activation error reaches h at most unchanged; the factor n because the engine's fp32 cell state carries the earlier launches' contributions (each
multiplied by sigmoid(f + 1) < 1) while the reference chain is float64.  In fp32 gx is recomputed in float64, not decoded: its fp32 error is charged
to the step launch that adds it.  Logits within 1e-5 x their scale; prob within 1e-5 x max(1, logits scale) (softmax moves by at most half the largest
logit change; the tiling adds at most T float32 roundings); pred == argmax(prob) exactly.
bf16 (inputs: the engine's stored bf16 values, gate kernels rounded to bf16, fp32 bias): decoded gx within half a bf16 ulp on every element (grade(),
as for the conv layers); h1 and every hall map: every element within one bf16 ulp + 1e-5 of the exact value, and >= 99.9 % of them within half an ulp
(+ grade()'s slack).  First step: h1 is graded against BOTH models -- gates rounded to bf16 first (what gx holds), and un-rounded -- and exactly one
must pass: the kernel's x pass rounds the gates whenever gx is kept (kernels_ws.hip mode 1, kernels_wino24.hip LS 1 BF), and uses the fp32
accumulator in the un-hoisted form (UKBB_LSTM_BF16_UNHOIST, mode 3), where no gx exists.  UKBB_LSTM_BF16_WINOGRAD: fp32 (un-rounded) gate kernels on
bf16 storage, gx in the F(2x4) kernel's lane order.

Cases (regimes(): the launchers' grid arithmetic; tests/test_lstm_launch_coverage.py shows that every regime is reached and every case needed):

    A     run_seq 1x9x16x16               one region column; W below the bf16 32-column tile
    B     run_seq 2x9x48x48               the 32-column regions the planner picks in production, ragged; a two-sequence map
    B64   run_seq 2x9x48x64               32-column regions that divide the map
    C     run_seq 1x9x128x128             the XCD-local tile order of launch_lstm_ws (H W >= 128^2)
    D     run_cine F = 13, 64x80          workgroups with one and with several items in one launch; the window-map gathers
    D32   D, UKBB_LSTM_TILE_COLS=32       (fp32, child process) ragged 32-column regions with second items
    E     run_cine F = 5, 32x48           F < T: a frame twice in one window
    F10   run_cine F = 12, time_step 10   frames no window reaches: NaN, pred 0; h1 of unused frames
    F2    run_cine F = 12, time_step 2    fewer windows than frames, every frame reached
    G1 G3 G13   run_seq 2xTx32x48, (T, classes) = (1, 3), (3, 4), (13, 3): no step launch at all; four classes; the longest chain
    H     B in bf16 under UKBB_LSTM_BF16_UNHOIST=1 / UKBB_LSTM_BF16_WINOGRAD=1 (child processes)

Measured on an MI355X (profiles/lstm_launches.txt, one row per launch, the worst per kind, form and step in its last block): fp32 hidden maps
1.4e-7 .. 3.8e-7 of S at every step, the 13th as the 2nd (the factor n is not used up), logits <= 2.2e-7 of their scale, prob <= 1.5e-7; bf16: no element
of any gx or hidden map outside half an ulp, in the three forms; the first-step model that does not apply misses on 28 - 36 % of the elements.  The 26
tests take 17 s together: the largest case 1.5 s (0.02 s of it the run and read-back), a child 2.5 - 3.1 s, most of it starting Python."""
import dataclasses
import json
import os
import time

import numpy as np
import pytest

from launch_grading import bf16_round, fold, grade, half_ulp, run_in_child, tolerance
from oracle import fcn_oracle as O

pytestmark = pytest.mark.gpu
BOUND = 1e-5                             # the project's per-launch fp32 bound (tests/test_fp32_launches_gpu.py BOUND)
MODEL = 'UNet-LSTM_ao'
NH = 16                                  # hidden channels
PROB_ATOL = 1e-5
ULP_ATOL = 1e-5                          # bf16: absolute part of the every-element condition
HALF_ULP_SHARE = 0.999

# name -> (call, sequences or frames, H, W, time_step, T, classes)
CASES = {
    'A': ('seq', 1, 16, 16, 1, 9, 3), 'B': ('seq', 2, 48, 48, 1, 9, 3), 'B64': ('seq', 2, 48, 64, 1, 9, 3), 'C': ('seq', 1, 128, 128, 1, 9, 3),
    'D': ('cine', 13, 64, 80, 1, 9, 3), 'E': ('cine', 5, 32, 48, 1, 9, 3), 'F10': ('cine', 12, 32, 48, 10, 9, 3), 'F2': ('cine', 12, 32, 48, 2, 9, 3),
    'G1': ('seq', 2, 32, 48, 1, 1, 3), 'G3': ('seq', 2, 32, 48, 1, 3, 4), 'G13': ('seq', 2, 32, 48, 1, 13, 3),
}
# (case, precision, knob or None): the forms behind environment variables run in child processes
CHILDREN = [('D', 'fp32', 'UKBB_LSTM_TILE_COLS=32'), ('B', 'bf16', 'UKBB_LSTM_BF16_UNHOIST=1'), ('B', 'bf16', 'UKBB_LSTM_BF16_WINOGRAD=1')]
RUNS = [(c, p, None) for c in CASES for p in ('fp32', 'bf16')] + CHILDREN
# what each run must reach, in regimes()'s words, for 256 compute units
EXPECT = {
    ('A', 'fp32', None): {'regions of 16 columns', 'one region column', 'step items below the grid'},
    ('A', 'bf16', None): {'map narrower than a tile', 'step workgroups below the grid', 'wave-major tile order'},
    ('B', 'fp32', None): {'regions of 32 columns, ragged', 'the default model on planned 32-column regions, ragged', 'step items below the grid', 'two-sequence map'},
    ('B', 'bf16', None): {'ragged tile', 'step workgroups below the grid', 'two-sequence map of the default model'},
    ('B64', 'fp32', None): {'regions of 32 columns', 'planned 32-column regions'},
    ('B64', 'bf16', None): {'two sequences on whole tiles'},
    ('C', 'fp32', None): {'regions of 16 columns', 'step items below the grid', 'a map of 128 x 128'},
    ('C', 'bf16', None): {'XCD-local tile order', 'step workgroups below the grid'},
    ('D', 'fp32', None): {'regions of 16 columns', 'step items above two rounds', 'x pass items above two rounds', 'cine window map'},
    ('D', 'bf16', None): {'ragged tile', 'step workgroups above the grid', 'x pass workgroups above the grid', 'cine window map'},
    ('D', 'fp32', 'UKBB_LSTM_TILE_COLS=32'): {'regions of 32 columns, ragged', 'step items between one and two rounds', 'ragged 32-column regions with second items'},
    ('E', 'fp32', None): {'F < T'}, ('E', 'bf16', None): {'F < T'},
    ('F10', 'fp32', None): {'frames no window reaches'}, ('F10', 'bf16', None): {'frames no window reaches'},
    ('F2', 'fp32', None): {'fewer windows than frames, every frame reached'}, ('F2', 'bf16', None): {'fewer windows than frames, every frame reached'},
    ('G1', 'fp32', None): {'T = 1'}, ('G1', 'bf16', None): {'T = 1'},
    ('G3', 'fp32', None): {'4 classes'}, ('G3', 'bf16', None): {'4 classes'},
    ('G13', 'fp32', None): {'T = 13'}, ('G13', 'bf16', None): {'T = 13'},
    ('B', 'bf16', 'UKBB_LSTM_BF16_UNHOIST=1'): {'un-hoisted steps (mode 3)', 'ragged tile'},
    ('B', 'bf16', 'UKBB_LSTM_BF16_WINOGRAD=1'): {'fp32 Winograd arithmetic on bf16 storage', 'regions of 32 columns, ragged'},
}
EXPECT = {k: {k[1] + ': ' + s for s in v} for k, v in EXPECT.items()}
WS_TW, WS_R, WS_NW = 32, 2, 4            # kernels_ws.hip WS_TW, LSW_R, LSW_NW (tests/test_lstm_launch_coverage.py reads them from the source)
W24_ROWS = 8                             # kernels_wino24.hip: 2 * TRY pixel rows per region


def arch_of(case):
    from ukbb_cardiac_amd.arch import MODELS
    _, _, _, _, _, T, c = CASES[case]
    return dataclasses.replace(MODELS[MODEL], fc=T, n_class=c)


def frames_windows(case):
    """(NF feature frames, Wn windows, T steps) of the case's run_bilstm call."""
    call, n, _, _, ts, T, _ = CASES[case]
    return (n * T, n, T) if call == 'seq' else (n, (n + ts - 1) // ts, T)


def window_map(case):
    """map[k][w] = feature frame of step k of window w: w T + k for run_seq (ukbb_fcn_forward_seq), the circular windows of
    deploy_network_ao.py:147-158 centred on range(0, F, time_step) for run_cine."""
    call, n, _, _, ts, T, _ = CASES[case]
    if call == 'seq':
        return np.array([[w * T + k for w in range(n)] for k in range(T)], np.int64).reshape(T, n)
    return np.array([O.aortic_window_indices(t, n, (T + 1) // 2) for t in range(0, n, ts)], np.int64).T.reshape(T, -1)


def regimes(case, precision, lstm_plan, planned_cols, cus=256):
    """The situations a run reaches, each prefixed with its precision, from the launchers' grid arithmetic (launch_wino24_lstm_t: min(items, CUs)
    persistent workgroups, items = ceil(H / 8) x N x ceil(W / tile_cols) x Cout / 64; launch_lstm_ws: ceil(tiles / 4) x Cout / 64 workgroups wanted on
    a grid of at most the CUs).  lstm_plan: plan_layout(...)['lstm'] of the run; planned_cols: the fp32 plan's tile_cols without any knob."""
    call, n, H, W, ts, T, ncls = CASES[case]
    NF, Wn, _ = frames_windows(case)
    out = set()
    add = lambda s: out.add(precision + ': ' + s)
    default_model = (T, ncls) == (9, 3)
    add('%d classes' % ncls)
    if T in (1, 13):
        add('T = %d' % T)
    wino = precision == 'fp32' or lstm_plan['bf_wino']
    launches = [('x pass', NF, 2)] + ([('step', Wn, 1)] if T > 1 else [])
    if wino:
        cols = lstm_plan['tile_cols']
        ragged = W % cols != 0
        add('regions of %d columns%s' % (cols, ', ragged' if ragged else ''))
        if cols == 32 and planned_cols == 32:
            add('planned 32-column regions')
            if ragged and default_model:
                add('the default model on planned 32-column regions, ragged')
        regs_x = (W + cols - 1) // cols
        if regs_x == 1:
            add('one region column')
        if (H, W) == (128, 128):
            add('a map of 128 x 128')
        for kind, N, groups in launches:
            items = ((H + W24_ROWS - 1) // W24_ROWS) * N * regs_x * groups
            where = 'below the grid' if items < cus else 'equal to the grid' if items == cus else 'between one and two rounds' if items <= 2 * cus else 'above two rounds'
            add('%s items %s' % (kind, where))
            if items > cus and cols == 32 and ragged:
                add('ragged 32-column regions with second items')
        if precision == 'bf16':
            add('fp32 Winograd arithmetic on bf16 storage')
    else:
        if W < WS_TW:
            add('map narrower than a tile')
        if W % WS_TW:
            add('ragged tile')
        add('XCD-local tile order' if H * W >= 128 * 128 else 'wave-major tile order')
        tiles = ((H + WS_R - 1) // WS_R) * ((W + WS_TW - 1) // WS_TW)
        for kind, N, groups in launches:
            want = (N * tiles + WS_NW - 1) // WS_NW * groups
            grid = cus // (8 * groups) * (8 * groups) if cus >= 8 * groups else max(cus // groups * groups, groups)
            add('%s workgroups %s the grid' % (kind, 'below' if want < grid else 'above' if want > grid else 'equal to'))
        if not lstm_plan['bf_hoist']:
            add('un-hoisted steps (mode 3)')
        elif call == 'seq' and n == 2 and default_model:
            add('two-sequence map of the default model' if W % WS_TW else 'two sequences on whole tiles')
    if call == 'seq' and n == 2:
        add('two-sequence map')
    if call == 'cine':
        add('cine window map')
        m = window_map(case)
        if n < T:
            add('F < T')
        if len(set(m.ravel())) < n:
            add('frames no window reaches')
        elif Wn < n:
            add('fewer windows than frames, every frame reached')
    return out


# ---- the float64 restatement of one launch ---------------------------------------------------------------------------------------------------------
def gate_conv(x, w):
    """3 x 3 SAME cross-correlation as one im2col product: x [N, H, W, Cin], w [3, 3, Cin, Cout] -> [N, H, W, Cout], in x's dtype."""
    n, h, wd, cin = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    cols = np.concatenate([xp[:, i:i + h, j:j + wd, :] for i in range(3) for j in range(3)], axis=-1)
    return (cols.reshape(-1, 9 * cin) @ np.asarray(w, x.dtype).reshape(9 * cin, -1)).reshape(n, h, wd, -1)


def sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def cell(z, c, forget_bias=1.0):
    """Conv2DLSTMCell's update from the gate pre-activations z (i | j | f | o, 16 channels each) and the cell state c: (h', c')."""
    i, j, f, o = np.split(z, 4, axis=-1)
    c = sig(f + forget_bias) * c + sig(i) * np.tanh(j)
    return np.tanh(c) * sig(o), c


def direction_launches(d, feat, h1, hall, wmap, kernel, bias, gx_stored=None, first_from_stored=False, tweak=None):
    """The launches of direction d (0 forward, 1 backward), each evaluated alone in float64 from the stored maps in front of it.  Yields
    (kind, n, k, exact, got, S): kind 'gx' (exact W_x * feat + b of every frame), 'h1' (n = 1), 'step' (n = 2..T at window position k); got = the
    stored map graded against exact (None for 'gx' when nothing is stored), S = max(1, max |z|) of the launch.
    feat [NF, H, W, 16], h1 [NF, H, W, 16], hall [T, Wn, H, W, 16] (this direction's), kernel [3, 3, 32, 64] (x rows first), bias [64], float64.
    gx_stored: the stored gx (bf16 plans), which the steps then add instead of the exact one; first_from_stored: the first step takes it too (the
    rounded-gates model).  tweak: planted defects (tests/test_lstm_launch_coverage.py)."""
    tweak = tweak or {}
    T, Wn = wmap.shape
    kx, kh = kernel[:, :, :NH], tweak.get('kh', kernel[:, :, NH:])
    post = tweak.get('z', lambda z: z)
    fb = tweak.get('forget_bias', 1.0)
    gx = gate_conv(feat, kx) + bias
    yield 'gx', 0, -1, gx, gx_stored, max(1.0, float(np.abs(gx).max()))
    zin = gx if gx_stored is None else gx_stored
    z1 = post(zin if first_from_stored else gx)
    hx, c1 = cell(z1, 0.0, fb)
    yield 'h1', 1, -1, hx, h1, max(1.0, float(np.abs(z1).max()))
    order = list(range(T)) if d == 0 else list(range(T - 1, -1, -1))
    c = c1[wmap[order[0]]]
    hprev = tweak.get('h1', h1)[wmap[order[0]]]
    older = [c, c]                                                       # the cell states of one and of two steps back (a planted defect reads the latter)
    for n, k in enumerate(order[1:], 2):
        frames = tweak.get('gx_frame', lambda f: f)(wmap[k])
        z = post(zin[frames] + gate_conv(tweak.get('hprev', lambda h: h)(hprev), kh))
        h, c = cell(z, older[0] if tweak.get('stale_c') else c, fb)
        older = [older[1], c]
        yield 'step', n, k, h, hall[k], max(1.0, float(np.abs(z).max()))
        hprev = hall[k]


def out_logits(hf, hb, po, swap=False):
    """The 1 x 1 output conv over concat([h_fw, h_bw]) + bias (network_ao.py:305-312), float64."""
    k = po['kernel'].astype(np.float64).reshape(2 * NH, -1)
    if swap:
        k = np.concatenate([k[NH:], k[:NH]])
    return np.concatenate([hf, hb], axis=-1).astype(np.float64) @ k + po['bias'].astype(np.float64)


def step_maps(h1, hall, wmap):
    """([T][Wn][H][W][16] forward, backward) hidden maps as the output kernels read them: a direction's first step from h1 through the map."""
    T = wmap.shape[0]
    hf = np.stack([h1[0][wmap[0]] if k == 0 else hall[0, k] for k in range(T)])
    hb = np.stack([h1[1][wmap[T - 1]] if k == T - 1 else hall[1, k] for k in range(T)])
    return hf, hb


def tile_prob(p, F, T, time_step, weight_r=0.1):
    """deploy_network_ao.py:129-183 in float64: p [Wn][T][H][W][C] window probabilities -> [F][H][W][C].  `prob[idx] += p * w` with fancy indexing
    keeps the LAST of a frame's occurrences in one window (F < T); a frame no window reaches ends as 0 / 0 = NaN."""
    weight_R = (T + 1) // 2
    prob = np.zeros((F,) + p.shape[2:], np.float64)
    weight = np.zeros((F, 1, 1, 1), np.float64)
    w = O.aortic_window_weights(weight_R, weight_r).reshape(T, 1, 1, 1)
    for wi, t in enumerate(range(0, F, time_step)):
        idx = O.aortic_window_indices(t, F, weight_R)
        prob[idx] += p[wi] * w
        weight[idx] += w
    with np.errstate(invalid='ignore', divide='ignore'):
        return prob / weight


# ---- reading the engine's buffers --------------------------------------------------------------------------------------------------------------------
def widen(raw, count, bf):
    """The first ``count`` stored elements of a raw 'lstm:*' buffer (handed out as float32 words) as float32 values."""
    if not bf:
        return raw[:count]
    return (raw.view(np.uint16)[:count].astype(np.uint32) << 16).view(np.float32)


def decode_gx_ws(raw, NF, H, W):
    """kernels_ws.hip mode 1's lane-native gx -> [dir][NF][H][W][64] (i | j | f | o).  Per frame: tiles of 2 rows x 32 columns, each
    [row][gate][lane half g][pixel][hidden channel 8 g + m] bf16 (the decoder of tools/debug_lstm.py, vectorised)."""
    ty_n, tx_n = (H + WS_R - 1) // WS_R, (W + WS_TW - 1) // WS_TW
    v = widen(raw, 2 * NF * ty_n * tx_n * WS_R * 2048, True).reshape(2, NF, ty_n, tx_n, 2, 4, 2, 32, 8)
    v = v.transpose(0, 1, 2, 4, 3, 7, 5, 6, 8).reshape(2, NF, ty_n * 2, tx_n * 32, 64)
    return np.ascontiguousarray(v[:, :, :H, :W])


def decode_gx_wino(raw, NF, H, W, cols):
    """kernels_wino24.hip LS 1 BF's gx -> [dir][NF][H][W][64].  Per frame and 8 x cols region: [wave][tile block][row i of the 2 x 4 tile][column j]
    [lane = 16 g + t16][gate] bf16; tile q = 16 tb + t16 of the region's 4 x (cols / 4) tiles, hidden channel 4 wave + g."""
    tbw, trx = cols // 16, cols // 4
    regs_y, regs_x = (H + 7) // 8, (W + cols - 1) // cols
    v = widen(raw, 2 * NF * regs_y * regs_x * 4 * tbw * 8 * 64 * 4, True).reshape(2, NF, regs_y, regs_x, 4, tbw, 2, 4, 4, 16, 4)
    ry, rx, wave, tb, i, j, g, t16, gate = np.meshgrid(*[np.arange(s) for s in v.shape[2:]], indexing='ij')
    q = tb * 16 + t16
    y, x = (ry * 4 + q // trx) * 2 + i, (rx * trx + q % trx) * 4 + j
    ok = (y < H) & (x < W)
    out = np.full((2, NF, H, W, 64), np.nan, np.float32)
    out[:, :, y[ok], x[ok], (gate * 16 + 4 * wave + g)[ok]] = v[:, :, ok]
    assert not np.isnan(out).any()
    return out


def run_engine(case, precision, seed):
    """One call; returns everything the grades need, the stored maps as float32 arrays of their stored values."""
    import torch
    from ukbb_cardiac_amd import engine
    from ukbb_cardiac_amd.weights import synthetic_params
    call, n, H, W, ts, T, ncls = CASES[case]
    arch = arch_of(case)
    params = synthetic_params(arch, seed)
    NF, Wn, _ = frames_windows(case)
    bf = precision == 'bf16'
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    plan = engine.plan_layout(arch, precision, NF, H, W, cus)['lstm']
    x = np.random.default_rng(seed + 1).standard_normal((NF, H, W)).astype(np.float32)
    r = dict(arch=arch, params=params, plan=plan, cus=cus, bf=bf)
    t0 = time.perf_counter()
    with engine.Engine(arch, params) as eng:
        if bf:
            eng.set_precision('bf16')
        if call == 'seq':
            r['out'] = eng.run_seq(x.reshape(n, T, H, W, 1), want_logits=True)
        else:
            r['prob'], r['pred'] = eng.run_cine(x, weight_R=(T + 1) // 2, weight_r=0.1, time_step=ts)
        r['feat'] = eng.activation('up0').reshape(NF, H, W, 16)
        r['h1'] = widen(eng.activation('lstm:h1'), 2 * NF * H * W * NH, bf).reshape(2, NF, H, W, NH)
        r['hall'] = widen(eng.activation('lstm:hall'), 2 * T * Wn * H * W * NH, bf).reshape(2, T, Wn, H, W, NH)
        r['hall'][0, 0] = r['hall'][1, T - 1] = 0.0                       # never written (those first steps live in h1): whatever the buffer held
        r['gx'] = None
        if bf and plan['bf_hoist']:
            raw = eng.activation('lstm:gx')
            r['gx'] = decode_gx_wino(raw, NF, H, W, plan['tile_cols']) if plan['bf_wino'] else decode_gx_ws(raw, NF, H, W)
    r['t_gpu'] = time.perf_counter() - t0
    return r


def share_half_ulp(got, exact, scale=1.0):
    """Share of the elements inside grade()'s half-ulp tolerance (a hidden map: |h| < 1, scale 1)."""
    return float(np.mean(np.abs(np.asarray(got, np.float64) - exact) <= tolerance(exact, scale, 0.5)))


def share_one_ulp(got, exact):
    """Share of the elements within one bf16 ulp of the exact value + 1e-5."""
    return float(np.mean(np.abs(np.asarray(got, np.float64) - exact) <= 2 * half_ulp(exact) + ULP_ATOL))


def passes(name, got, exact, scale=1.0, fraction=HALF_ULP_SHARE):
    try:
        grade(name, got, exact, scale, ulps=0.5, fraction=fraction)
    except AssertionError:
        return False
    return True


def holds(name, got, exact):
    """The two bf16 conditions on a hidden map: every element within one ulp + 1e-5, 99.9 % within half an ulp (grade())."""
    return share_one_ulp(got, exact) == 1.0 and passes(name, got, exact)


def grade_run(case, precision, knob=None, seed=1234):
    """Runs the case and grades every launch; returns the profile rows (dicts).  Asserts after printing every figure."""
    from ukbb_cardiac_amd import engine
    call, n, H, W, ts, T, ncls = CASES[case]
    NF, Wn, _ = frames_windows(case)
    assert {k: v for k, v in os.environ.items() if k.startswith('UKBB_LSTM_')} == (dict([knob.split('=')]) if knob else {})
    r = run_engine(case, precision, seed)
    bf, plan, params = r['bf'], r['plan'], r['params']
    # ---- the form and the grid regime the case is listed for are the ones that ran ----
    env = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith('UKBB_LSTM_')}     # the plan without the knob
    try:
        planned = engine.plan_layout(r['arch'], 'fp32', NF, H, W, r['cus'])['lstm']['tile_cols']
    finally:
        os.environ.update(env)
    reached = regimes(case, precision, plan, planned, r['cus'])
    assert reached >= EXPECT.get((case, precision, knob), set()), (sorted(EXPECT[(case, precision, knob)] - reached), plan, r['cus'])
    form = ('wino24 %d cols' % plan['tile_cols'] + (' ragged' if W % plan['tile_cols'] else '')) if (not bf or plan['bf_wino']) else \
        ('ws mode %d' % (2 if plan['bf_hoist'] else 3) + (' ragged' if W % WS_TW else ''))
    tag = 'lstm-launch %-3s %-4s %-26s %-18s' % (case, precision, knob or '-', form)
    wmap = window_map(case)
    assert wmap.shape == (T, Wn) and wmap.min() >= 0 and wmap.max() < NF
    feat = r['feat'].astype(np.float64)
    if bf:
        for k in ('feat', 'h1'):
            assert np.array_equal(r[k], bf16_round(r[k])), k
    t0 = time.perf_counter()
    rows, failures = [], []

    def row(kind, d, n_, figure, ok, what):
        rows.append(dict(case=case, precision=precision, knob=knob, form=form, kind=kind, dir=d, n=n_, figure=figure, what=what))
        print('%s %-8s dir %d n %2d  %s %.3e%s' % (tag, kind, d, n_, what, figure, '' if ok else '   <-- MISSES'))
        if not ok:
            failures.append((kind, d, n_, what, figure))

    first_model = set()
    for d, name in enumerate(('lstm_fw', 'lstm_bw')):
        kernel, bias = fold(params[name])
        if bf and not plan['bf_wino']:
            kernel = bf16_round(kernel)
        kernel, bias = kernel.astype(np.float64), bias.astype(np.float64)
        h1, hall = r['h1'][d].astype(np.float64), r['hall'][d].astype(np.float64)
        if not bf:
            for kind, n_, k, exact, got, S in direction_launches(d, feat, h1, hall, wmap, kernel, bias):
                if kind != 'gx':
                    err = float(np.abs(got - exact).max()) / S
                    row(kind, d, n_, err, err <= n_ * BOUND, 'err/S (bound %de-5)' % n_)
            continue
        gxs = None if r['gx'] is None else r['gx'][d].astype(np.float64)
        for kind, n_, k, exact, got, S in direction_launches(d, feat, h1, hall, wmap, kernel, bias, gx_stored=gxs, first_from_stored=True):
            if kind == 'gx':
                gx_exact = exact
                if got is not None:                                  # half an ulp on every element, as for the conv layers
                    sc = float(np.abs(exact).max())
                    row('gx', d, 0, 1.0 - share_half_ulp(got, exact, sc), passes('gx', got, exact, sc, 1.0), 'share outside half an ulp')
            elif kind == 'h1':
                # the first step against both models: gates rounded to bf16 first (gx kept: the stored gx holds them) | un-rounded
                ex_r = exact if gxs is not None else cell(bf16_round(gx_exact.astype(np.float32)).astype(np.float64), 0.0)[0]
                ex_u = cell(gx_exact, 0.0)[0]
                ok_r, ok_u = holds('h1, gates rounded first', r['h1'][d], ex_r), holds('h1, gates un-rounded', r['h1'][d], ex_u)
                want_r = gxs is not None                             # gx kept: the x pass rounds its gates; un-hoisted: it does not
                row('h1', d, 1, 1.0 - share_half_ulp(r['h1'][d], ex_r), ok_r == want_r, 'share outside half an ulp, gates rounded first')
                row('h1', d, 1, 1.0 - share_half_ulp(r['h1'][d], ex_u), ok_u == (not want_r), 'share outside half an ulp, gates un-rounded')
                row('h1', d, 1, 1.0 - share_one_ulp(r['h1'][d], ex_r if want_r else ex_u), True, 'share outside one ulp + 1e-5, its model')
                first_model.add('both' if ok_r and ok_u else 'rounded' if ok_r else 'un-rounded' if ok_u else 'neither')
            else:
                got32 = r['hall'][d][k]
                assert np.array_equal(got32, bf16_round(got32))
                row('step', d, n_, 1.0 - share_half_ulp(got32, exact), passes('step', got32, exact), 'share outside half an ulp')
                row('step', d, n_, 1.0 - share_one_ulp(got32, exact), share_one_ulp(got32, exact) == 1.0, 'share outside one ulp + 1e-5')
    # ---- output conv, softmax / argmax, tiling: from the stored hidden maps ----
    hf, hb = step_maps(r['h1'].astype(np.float64), r['hall'].astype(np.float64), wmap)
    lg64 = out_logits(hf, hb, params['lstm_out']).transpose(1, 0, 2, 3, 4)               # [Wn][T][H][W][C]
    lsc = float(np.abs(lg64).max())
    p64 = O.softmax(lg64)
    if call == 'seq':
        out = r['out']
        e = float(np.abs(out['logits'] - lg64).max()) / lsc
        row('lstm_out', 2, T, e, e <= BOUND, 'logits err/scale')
        e = float(np.abs(out['prob'] - p64).max())
        row('lstm_out', 2, T, e, e <= PROB_ATOL * max(1.0, lsc), 'prob abs err')
        assert np.array_equal(out['pred'], out['prob'].argmax(-1)), 'pred != argmax(prob)'
        flips = out['pred'] != lg64.argmax(-1)
        assert np.all(O.top2_margin(lg64)[flips] <= 2 * BOUND * lsc), 'pred differs from the float64 argmax away from a tie'
    else:
        want = tile_prob(p64, n, T, ts)
        prob, pred = r['prob'], r['pred']
        dead = np.isnan(want)
        assert np.array_equal(np.isnan(prob), dead), 'NaN frames differ'
        assert dead.reshape(n, -1).all(axis=1).sum() == n - len(set(wmap.ravel())) and np.array_equal(dead.all(axis=(1, 2, 3)), dead.any(axis=(1, 2, 3)))
        e = float(np.abs(prob - want)[~dead].max())
        row('lstm_tile', 2, T, e, e <= PROB_ATOL * max(1.0, lsc), 'prob abs err')
        assert np.all(pred[dead.all(axis=-1)] == 0), 'pred of a frame no window reaches'
        live = ~dead.all(axis=-1)
        assert np.array_equal(pred[live], prob.argmax(-1)[live]), 'pred != argmax(prob)'
    print('%s run + read-back %.2f s, float64 reference %.2f s%s' % (tag, r['t_gpu'], time.perf_counter() - t0,
                                                                   '' if not bf else ', first step passes with: %s gates' % '/'.join(sorted(first_model))))
    assert not failures, failures
    assert not bf or first_model in ({'rounded'}, {'un-rounded'}), 'first step: exactly one of the two models must pass, the same in both directions: %s' % first_model
    return rows


def test_gate_conv_is_conv2d_same():
    rng = np.random.default_rng(0)
    x, w = rng.standard_normal((2, 9, 13, 16)), rng.standard_normal((3, 3, 16, 64))
    ex = O.conv2d_same(x, w, 1)
    assert np.abs(gate_conv(x, w) - ex).max() <= 1e-12 * np.abs(ex).max()


@pytest.mark.parametrize('case,precision', [(c, p) for c, p, k in RUNS if k is None], ids=['%s-%s' % (c, p) for c, p, k in RUNS if k is None])
def test_each_lstm_launch_against_float64_on_its_own_input(case, precision):
    grade_run(case, precision)


def run_child(case, precision, knob, path):
    """In a process started with ``knob``: grade the run, leave the rows at ``path``."""
    rows = grade_run(case, precision, knob)
    with open(path, 'w') as f:
        json.dump(rows, f)


@pytest.mark.parametrize('case,precision,knob', CHILDREN, ids=['%s-%s-%s' % c for c in CHILDREN])
def test_lstm_launches_behind_a_knob_against_float64(case, precision, knob, tmp_path):
    path = str(tmp_path / 'rows.json')
    r = run_in_child('test_lstm_launches_gpu', 'run_child', [case, precision, knob, path], dict([knob.split('=')]), timeout=120)
    print(''.join(ln + '\n' for ln in r.stdout.splitlines() if ln.startswith('lstm-launch')), end='')
    assert r.returncode == 0, r.stdout[-3000:]
    with open(path) as f:
        rows = json.load(f)
    assert {(x['case'], x['precision'], x['knob']) for x in rows} == {(case, precision, knob)} and any(x['kind'] == 'step' for x in rows)
