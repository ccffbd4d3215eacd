"""What tests/test_lstm_launches_gpu.py covers, checked without a GPU, and that its bounds can tell a wrong ConvLSTM launch from a right one.

Coverage: the situations of the two gate-conv launchers are computed on the host from the case's shape, the planner's region choice
(engine.plan_layout, 256 compute units) and the launchers' constants, which are read from kernels_wino24.hip and kernels_ws.hip.  RUNS reaches every
situation in REQUIRED, each run reaches what the GPU test lists for it (EXPECT), and dropping any one run leaves a situation unreached.

The bounds can tell a defect: on one 32 x 48 window of nine frames, with a float32 (or bf16-storing) numpy evaluation of the unchanged reference
standing in for the engine, every launch passes; the float64 reference with ONE planted defect (a zeroed W_h tap, h_prev shifted by a pixel, gates i
and j swapped, forget bias 0, the cell state of two steps back, gx of the neighbouring frame, the backward direction reading the forward h1, the
output conv's halves swapped) is further than 100 x the fp32 bound from the unchanged one at every launch it touches, and its bf16 rounding has fewer
than 99.9 % of its elements within half an ulp.  The first step with gates rounded to bf16 first and with un-rounded gates tell each other apart the
same way (share of agreement printed: 0.7 - 0.8)."""
import os
import re

import numpy as np
import pytest

import test_lstm_launches_gpu as G
from launch_grading import CUS, bf16_round, fold, no_case_is_idle
from oracle import fcn_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = G.BOUND

REQUIRED = {
    'fp32: regions of 16 columns', 'fp32: regions of 32 columns', 'fp32: regions of 32 columns, ragged', 'fp32: planned 32-column regions',
    'fp32: the default model on planned 32-column regions, ragged', 'fp32: one region column', 'fp32: ragged 32-column regions with second items',
    'fp32: step items below the grid', 'fp32: step items between one and two rounds', 'fp32: step items above two rounds',
    'fp32: x pass items below the grid', 'fp32: x pass items between one and two rounds', 'fp32: x pass items above two rounds',
    'bf16: step workgroups below the grid', 'bf16: step workgroups above the grid', 'bf16: x pass workgroups below the grid', 'bf16: x pass workgroups above the grid',
    'bf16: ragged tile', 'bf16: map narrower than a tile', 'bf16: two sequences on whole tiles', 'bf16: wave-major tile order', 'bf16: XCD-local tile order',
    'bf16: un-hoisted steps (mode 3)', 'bf16: fp32 Winograd arithmetic on bf16 storage', 'fp32: a map of 128 x 128', 'bf16: two-sequence map of the default model',
} | {p + s for p in ('fp32: ', 'bf16: ') for s in ('F < T', 'frames no window reaches', 'fewer windows than frames, every frame reached', 'T = 1', 'T = 13',
                                                     '3 classes', '4 classes', 'two-sequence map', 'cine window map')}


def source(name):
    with open(os.path.join(ROOT, 'ukbb_cardiac_amd', 'csrc', name)) as f:
        return f.read()


def test_launcher_constants_are_the_ones_assumed():
    w24, ws = source('kernels_wino24.hip'), source('kernels_ws.hip')
    assert 2 * int(re.search(r'constexpr int TRY = (\d+);', w24).group(1)) == G.W24_ROWS
    # items and grid of launch_wino24_lstm_t; regions of 4 * TRX = 16 * TBW columns (TBW = 2: 32 columns, 1: 16)
    assert 'const long long nitems = (long long)((a.Ho + 2 * TRY - 1) / (2 * TRY)) * a.N * regs_x * (a.Cout / 64);' in w24
    assert 'const int regs_x = (a.Wo + 4 * G::TRX - 1) / (4 * G::TRX);' in w24 and 'static constexpr int NT = 16 * TBW, TRX = 4 * TBW;' in w24
    assert 'dim3 grid((unsigned)(nitems < n_cu ? nitems : n_cu));' in w24
    assert 'tile_cols == 32 ? launch_wino24_lstm_t<2, 2, false>(a, s) : launch_wino24_lstm_t<1, 2, false>(a, s)' in w24
    assert int(re.search(r'constexpr int WS_TW = (\d+);', ws).group(1)) == G.WS_TW
    assert tuple(map(int, re.search(r'constexpr int LSW_R = (\d+), LSW_NW = (\d+);', ws).groups())) == (G.WS_R, G.WS_NW)
    lw = ws[ws.index('hipError_t launch_lstm_ws('):ws.index('hipError_t launch_conv_ws(')]
    assert 'a.xcd_local = force ? atoi(force) : ((long long)a.H * a.W >= 128ll * 128);' in lw
    assert 'long long want = ((ntiles + LSW_NW - 1) / LSW_NW) * nG;' in lw and 'const int nG = a.Cout / 64;' in lw
    assert 'int grid = cus >= 8 * nG ? cus / (8 * nG) * (8 * nG) : cus / nG * nG;' in lw and 'if (want < grid) grid = (int)((want + nG - 1) / nG * nG);' in lw


def plan_of(case, precision, knob):
    from ukbb_cardiac_amd import engine
    NF, _, _ = G.frames_windows(case)
    _, _, H, W, _, _, _ = G.CASES[case]
    assert not [k for k in os.environ if k.startswith('UKBB_LSTM_')]
    planned = engine.plan_layout(G.arch_of(case), 'fp32', NF, H, W, CUS)['lstm']['tile_cols']
    if knob:
        os.environ[knob.split('=')[0]] = knob.split('=')[1]
    try:
        return engine.plan_layout(G.arch_of(case), precision, NF, H, W, CUS)['lstm'], planned
    finally:
        if knob:
            del os.environ[knob.split('=')[0]]


def test_runs_reach_every_regime_and_none_is_idle():
    assert len(set(G.RUNS)) == len(G.RUNS) and set(G.EXPECT) <= set(G.RUNS)
    per_run = {(c, p, k): G.regimes(c, p, *plan_of(c, p, k), cus=CUS) for c, p, k in G.RUNS}
    for run, s in per_run.items():
        print(run, sorted(s))
        assert s >= G.EXPECT.get(run, set()), (run, G.EXPECT[run] - s)
    no_case_is_idle(G.RUNS, per_run.__getitem__, REQUIRED)
    # every case in both precisions; the figures the case table of the GPU test's docstring rests on
    assert {(c, p) for c, p, k in G.RUNS if k is None} == {(c, p) for c in G.CASES for p in ('fp32', 'bf16')}
    cols = {c: plan_of(c, 'fp32', None)[0]['tile_cols'] for c in G.CASES}
    assert cols == {'A': 16, 'B': 32, 'B64': 32, 'C': 16, 'D': 16, 'E': 16, 'F10': 16, 'F2': 16, 'G1': 16, 'G3': 16, 'G13': 32}
    assert plan_of('D', 'fp32', 'UKBB_LSTM_TILE_COLS=32')[0]['tile_cols'] == 32
    items = lambda c, co, N, g: ((G.CASES[c][2] + 7) // 8) * N * ((G.CASES[c][3] + co - 1) // co) * g
    assert (items('A', 16, 1, 1), items('B', 32, 2, 1), items('C', 16, 1, 1), items('D', 16, 13, 1), items('D', 16, 13, 2), items('D', 32, 13, 1)) == (2, 24, 128, 520, 1040, 312)


def test_window_maps():
    """run_seq: w T + k.  run_cine: circular windows; F < T puts a frame twice into one window; time_step 10 leaves frames 5 of 12 unreached."""
    assert G.window_map('B').tolist() == [[k, 9 + k] for k in range(9)]
    e = G.window_map('E')
    assert e.shape == (9, 5) and e[:, 0].tolist() == [1, 2, 3, 4, 0, 1, 2, 3, 4] and all(e[4, w] == w for w in range(5))
    f = G.window_map('F10')
    assert f.shape == (9, 2) and sorted(set(range(12)) - set(f.ravel())) == [5] and f[4].tolist() == [0, 10]
    assert G.window_map('F2').shape == (9, 6) and set(G.window_map('F2').ravel()) == set(range(12))
    assert G.window_map('D')[:, 0].tolist() == [9, 10, 11, 12, 0, 1, 2, 3, 4]


def test_tile_prob_is_the_reference_loop():
    """tile_prob against oracle aortic_lstm_prob_sequence (the reference's loop on a padded volume) fed with the same window probabilities."""
    rng = np.random.default_rng(5)
    for F, ts in ((13, 1), (5, 1), (12, 2)):
        Wn = (F + ts - 1) // ts
        p = O.softmax(rng.standard_normal((Wn, 9, 4, 6, 3))).astype(np.float32)
        full = np.zeros((Wn, 9, 256, 256, 3), np.float32)
        full[:, :, :4, :6] = p
        calls = iter(range(Wn))
        ref = O.aortic_lstm_prob_sequence(np.zeros((256, 256, 1, F)), lambda x: full[next(calls)][None], time_step=ts)[:4, :6, 0]     # [X][Y][F][C]
        got = G.tile_prob(p.astype(np.float64), F, 9, ts)
        assert np.abs(got - ref.transpose(2, 0, 1, 3)).max() <= 1e-6


# ---- the bounds can tell a defect ---------------------------------------------------------------------------------------------------------------------
H, W, T = 32, 48, 9


def stand_in(feat, params, wmap, bf, round_first=True):
    """The unchanged reference in float32 numpy, storing what the engine stores (bf: bf16 features, gate kernels, gx and hidden maps; fp32 cell
    state): (h1 [2][NF].., hall [2][T][Wn].., gx [2][NF]..64 or None)."""
    f32 = np.float32
    NF = feat.shape[0]
    Wn = wmap.shape[1]
    h1 = np.zeros((2, NF, H, W, G.NH), f32)
    hall = np.zeros((2, T, Wn, H, W, G.NH), f32)
    gxs = np.zeros((2, NF, H, W, 4 * G.NH), f32)
    for d, name in enumerate(('lstm_fw', 'lstm_bw')):
        k, b = fold(params[name])
        if bf:
            k = bf16_round(k)
        gx = (G.gate_conv(feat.astype(f32), k[:, :, :G.NH]) + b).astype(f32)
        gxs[d] = bf16_round(gx) if bf else gx
        h, c = G.cell(gxs[d] if round_first else gx, f32(0), f32(1))
        assert h.dtype == f32 and c.dtype == f32
        h1[d] = bf16_round(h) if bf else h
        order = list(range(T)) if d == 0 else list(range(T - 1, -1, -1))
        c, hp = c[wmap[order[0]]], h1[d][wmap[order[0]]]
        for kk in order[1:]:
            h, c = G.cell(gxs[d][wmap[kk]] + G.gate_conv(hp, k[:, :, G.NH:]), c, f32(1))
            assert h.dtype == f32 and c.dtype == f32
            hp = hall[d, kk] = bf16_round(h) if bf else h
    return h1, hall, (gxs if bf else None)


@pytest.fixture(scope='module')
def window():
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.weights import synthetic_params
    params = synthetic_params(MODELS[G.MODEL], 1234)
    feat = np.maximum(np.random.default_rng(11).standard_normal((T, H, W, G.NH)), 0.0).astype(np.float32)
    wmap = np.arange(T, dtype=np.int64).reshape(T, 1)
    return params, feat, wmap


def kernels(params, d, bf):
    k, b = fold(params[('lstm_fw', 'lstm_bw')[d]])
    return (bf16_round(k) if bf else k).astype(np.float64), b.astype(np.float64)


def launches(window, stored, d, bf, **kw):
    params, feat, wmap = window
    h1, hall, gxs = stored
    k, b = kernels(params, d, bf)
    feat = bf16_round(feat) if bf else feat
    return {(kind, n): (exact, got, S) for kind, n, _, exact, got, S in G.direction_launches(
        d, feat.astype(np.float64), h1[d].astype(np.float64), hall[d].astype(np.float64), wmap, k, b,
        gx_stored=None if gxs is None else gxs[d].astype(np.float64), first_from_stored=bf, **kw)}


def test_unchanged_reference_in_float32_and_bf16_passes(window):
    params, feat, wmap = window
    for bf in (False, True):
        stored = stand_in(bf16_round(feat) if bf else feat, params, wmap, bf)
        for d in (0, 1):
            for (kind, n), (exact, got, S) in launches(window, stored, d, bf).items():
                if kind == 'gx':
                    if bf:
                        assert G.passes('gx', got, exact, float(np.abs(exact).max()), 1.0)
                elif bf:
                    g32 = got.astype(np.float32)
                    assert G.holds(kind, g32, exact), (d, kind, n, G.share_half_ulp(g32, exact), G.share_one_ulp(g32, exact))
                else:
                    assert np.abs(got - exact).max() <= n * BOUND * S, (d, kind, n)
    h1, hall, _ = stand_in(feat, params, wmap, False)
    hf, hb = G.step_maps(h1.astype(np.float64), hall.astype(np.float64), wmap)
    po = params['lstm_out']
    lg32 = np.concatenate([hf, hb], -1).astype(np.float32) @ po['kernel'].astype(np.float32).reshape(2 * G.NH, -1) + po['bias'].astype(np.float32)
    lg64 = G.out_logits(hf, hb, po)
    assert lg32.dtype == np.float32 and np.abs(lg32 - lg64).max() <= BOUND * np.abs(lg64).max()
    e = np.exp(lg32 - lg32.max(-1, keepdims=True))
    p32 = e * (np.float32(1) / e.sum(-1, keepdims=True, dtype=np.float32))
    assert p32.dtype == np.float32 and np.abs(p32 - O.softmax(lg64)).max() <= G.PROB_ATOL * max(1.0, np.abs(lg64).max())


def shifted(h):
    out = np.zeros_like(h)
    out[:, :, 1:] = h[:, :, :-1]
    return out


def swap_ij(z):
    i, j, f, o = np.split(z, 4, axis=-1)
    return np.concatenate([j, i, f, o], axis=-1)


def test_bounds_tell_each_planted_defect(window):
    """(defect, the launches it touches): at each of them the defective float64 reference is > 100 x the fp32 bound from the unchanged one, and its
    bf16 rounding has < 99.9 % of the elements within half an ulp of the unchanged one."""
    params, feat, wmap = window
    for bf in (False, True):
        stored = stand_in(bf16_round(feat) if bf else feat, params, wmap, bf)
        for d in (0, 1):
            clean = launches(window, stored, d, bf)
            k, _ = kernels(params, d, bf)
            kh0 = k[:, :, G.NH:].copy()
            kh0[0, 2] = 0.0
            steps = [('step', n) for n in range(2, T + 1)]
            defects = [
                ('a zeroed W_h tap', dict(kh=kh0), steps),
                ('h_prev shifted by one pixel', dict(hprev=shifted), steps),
                ('gates i and j swapped', dict(z=swap_ij), [('h1', 1)] + steps),
                ('forget bias 0', dict(forget_bias=0.0), steps),
                ('the cell state of two steps back', dict(stale_c=True), steps[1:]),
                ('gx of the neighbouring frame', dict(gx_frame=lambda f: (f + 1) % T), steps),
            ]
            if d == 1:
                defects.append(('the backward direction reading the forward h1', dict(h1=stored[0][0].astype(np.float64)), steps[:1]))
            for name, tweak, touched in defects:
                bad = launches(window, stored, d, bf, tweak=tweak)
                for key in touched:
                    exact, _, S = clean[key]
                    wrong = bad[key][0]
                    if bf:
                        share = G.share_half_ulp(bf16_round(wrong.astype(np.float32)), exact)
                        print('bf16 dir %d %-46s %-5s n %d  share within half an ulp %.4f' % (d, name, key[0], key[1], share))
                        assert share < G.HALF_ULP_SHARE and not G.holds(name, bf16_round(wrong.astype(np.float32)), exact), (name, d, key, share)
                    else:
                        err = float(np.abs(wrong - exact).max()) / S
                        print('fp32 dir %d %-46s %-5s n %d  err/S %.2e (bound %.0e)' % (d, name, key[0], key[1], err, key[1] * BOUND))
                        assert err > 100 * key[1] * BOUND, (name, d, key, err)
    h1, hall, _ = stand_in(feat, params, wmap, False)
    hf, hb = G.step_maps(h1.astype(np.float64), hall.astype(np.float64), wmap)
    lg = G.out_logits(hf, hb, params['lstm_out'])
    err = float(np.abs(G.out_logits(hf, hb, params['lstm_out'], swap=True) - lg).max() / np.abs(lg).max())
    print('output conv halves swapped: logits err/scale %.2e' % err)
    assert err > 100 * BOUND


def test_first_step_models_tell_each_other_apart(window):
    """A bf16 x pass that rounds its gates first passes the rounded-gates model and misses the un-rounded one, and the other way round."""
    params, feat, wmap = window
    fb = bf16_round(feat)
    for round_first in (True, False):
        h1, hall, gxs = stand_in(fb, params, wmap, True, round_first)
        for d in (0, 1):
            k, b = kernels(params, d, True)
            gx = G.gate_conv(fb.astype(np.float64), k[:, :, :G.NH]) + b
            ex_r, ex_u = G.cell(gxs[d].astype(np.float64), 0.0)[0], G.cell(gx, 0.0)[0]
            ok_r, ok_u = G.holds('rounded', h1[d], ex_r), G.holds('un-rounded', h1[d], ex_u)
            share = G.share_half_ulp(h1[d], ex_u if round_first else ex_r)
            print('x pass %s its gates, dir %d: passes rounded model %s, un-rounded model %s; share within half an ulp of the other model %.3f' % (
                'rounds' if round_first else 'does not round', d, ok_r, ok_u, share))
            assert (ok_r, ok_u) == (round_first, not round_first) and 0.5 < share < 0.9
