"""The scratch budget of ukbb_fcn_forward_cine (ABI 11), the parts that need no GPU: the three entry points exist, the host-only
planner ukbb_fcn_cine_scratch_bytes reproduces the footprint include/ukbb_fcn.h documents, its chunk plans respect the budget, and
the aortic script takes --cine_scratch_gb.  (The planner is the function the engine itself plans with; tests/test_cine_budget_gpu.py
checks that what a handle allocates is what it predicts.)"""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['ukbb_fcn_set_scratch_budget', 'ukbb_fcn_scratch_bytes', 'ukbb_fcn_cine_scratch_bytes']


def _header():
    with open(os.path.join(ROOT, 'include', 'ukbb_fcn.h')) as f:
        return f.read()


def test_header_library_and_binding_agree_on_abi_11():
    from ukbb_cardiac_amd import _lib
    h = _header()
    assert int(re.search(r'#define\s+UKBB_FCN_ABI_VERSION\s+(\d+)', h).group(1)) == 11
    assert _lib.ABI_VERSION == 11 and _lib.lib.ukbb_fcn_abi_version() == 11
    for name in NEW:
        assert re.search(r'\b%s\s*\(' % name, h), name + ' not declared'
        assert name in _lib.EXPORTS
        assert getattr(_lib.lib, name) is not None
    assert re.search(r'int\s+ukbb_fcn_set_scratch_budget\(ukbb_fcn_handle \*h, uint64_t bytes\)', h)
    assert re.search(r'uint64_t\s+ukbb_fcn_scratch_bytes\(const ukbb_fcn_handle \*h\)', h)


# ---- the header's formula, in Python ---------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def _unet_floats_per_frame(arch, H, W):
    """Every activation map of the UNet-LSTM's U-Net plan (conv0_0 is evaluated inside conv0_1's launch and has none)."""
    hs = [(H, W)]
    for _ in range(1, arch.n_level):
        hs.append((_cdiv(hs[-1][0], 2), _cdiv(hs[-1][1], 2)))
    n = 0
    for l, (h, w) in enumerate(hs):
        n += (arch.n_block[l] - (1 if l == 0 else 0)) * h * w * arch.n_filter[l]
    for l in range(arch.n_level - 2, -1, -1):
        n += 4 * hs[l + 1][0] * hs[l + 1][1] * arch.n_filter[l] + arch.n_block[l] * hs[l][0] * hs[l][1] * arch.n_filter[l]
    return n


def _fp32_region_cols(F, H, W, cus=256):
    """The region shape of the fused gate-conv / cell kernel: 8 x 32 or 8 x 16 pixels, whichever wastes less of the last round of
    work items on 256 compute units (the wider on a tie; the finer for small batches; a shape must fill 70 % of its regions)."""
    best, best_eff = None, -1.0
    for tw in (32, 16):
        if H * W < 0.7 * _cdiv(H, 8) * 8 * _cdiv(W, tw) * tw:
            continue
        rounds = _cdiv(F * _cdiv(H, 8) * _cdiv(W, tw), cus)
        eff = 1.0 / (rounds * (tw // 16))
        if F <= 16:
            eff = 2.0 if tw == 16 else 1.0
        if eff > best_eff + 1e-12:
            best, best_eff = tw, eff
    return best


def _table_bytes(F, T, Wn):
    al8 = lambda v: _cdiv(v, 8) * 8
    off_ord = al8(4 * T * Wn)
    off_wk = al8(off_ord + 4 * F * T)
    return _cdiv(off_wk + 8 * T + 8 * F, 4) * 4


def _unchunked_bytes(arch, prec, F, H, W, ts):
    """include/ukbb_fcn.h, forward_cine:  2*T*Wn*HW*16*e + 2*F*HWp*64*e + 2*F*HW*16*e + (2*F + Wn)*HWp*16*4 + the U-Net's activations
    for F frames + the tables, HWp = the map padded to the kernels' tiles."""
    T, HW, Wn = arch.fc, H * W, _cdiv(F, ts)
    if prec == 'fp32':
        e, tc = 4, _fp32_region_cols(F, H, W)
        HWp = _cdiv(H, 8) * 8 * _cdiv(W, tc) * tc
    else:
        e = 2
        HWp = _cdiv(H, 2) * 2 * _cdiv(W, 32) * 32
    return (2 * T * Wn * HW * 16 * e + 2 * F * HWp * 64 * e + 2 * F * HW * 16 * e + (2 * F + Wn) * HWp * 16 * 4
            + F * _unet_floats_per_frame(arch, H, W) * 4 + _table_bytes(F, T, Wn))


CASES = [(100, 256, 256, 1), (4, 64, 64, 1), (25, 48, 80, 2), (25, 240, 208, 1), (50, 64, 64, 3), (10, 48, 80, 12), (9, 240, 208, 1),
         (400, 256, 256, 1)]


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('F,H,W,ts', CASES)
def test_budget_0_is_the_documented_unchunked_footprint(prec, F, H, W, ts):
    from ukbb_cardiac_amd import engine
    from ukbb_cardiac_amd.arch import MODELS
    arch = MODELS['UNet-LSTM_ao']
    got = engine.cine_scratch_bytes(arch, prec, F, H, W, ts, 0)
    assert got == _unchunked_bytes(arch, prec, F, H, W, ts)
    assert engine.cine_chunk_windows(arch, prec, F, H, W, ts, 0) == _cdiv(F, ts)
    if (F, H, W, ts) == (100, 256, 256, 1):
        # the header's 13.0 GB (fp32) / 7.2 GB (bf16) of ConvLSTM scratch + 136 floats per pixel and frame of U-Net maps
        lstm = got - 100 * 136 * 65536 * 4
        assert abs(lstm - (13.0e9 if prec == 'fp32' else 7.2e9)) < 0.1e9
    if (H, W) == (240, 208):                                                         # 208 = 6.5 x 32 columns: the tile-padded terms exceed the plain formula
        T, Wn, e = arch.fc, _cdiv(F, ts), 4 if prec == 'fp32' else 2
        plain = (2 * T * Wn * 16 * e + 2 * F * 64 * e + 2 * F * 16 * e + (2 * F + Wn) * 16 * 4 + F * 136 * 4) * H * W + _table_bytes(F, T, Wn)
        assert got > plain if (prec == 'bf16' or _fp32_region_cols(F, H, W) == 32) else got == plain


def test_temporal_unet_footprint():
    """Wc*T*(152 + C)*HW*4 bytes + tables, Wc from the 4e9-byte rule without a budget (include/ukbb_fcn.h)."""
    from ukbb_cardiac_amd import engine
    from ukbb_cardiac_amd.arch import MODELS
    arch = MODELS['Temporal-UNet_ao']
    per_window = 9 * (152 + 3) * 65536 * 4
    assert engine.cine_chunk_windows(arch, 'fp32', 50, 256, 256, 1, 0) == 10
    assert engine.cine_scratch_bytes(arch, 'fp32', 50, 256, 256, 1, 0) == 10 * per_window + _table_bytes(50, 9, 50)
    assert engine.cine_scratch_bytes(arch, 'fp32', 50, 256, 256, 1, int(1.2e9)) == 3 * per_window + _table_bytes(50, 9, 50)
    assert engine.cine_min_scratch_bytes(arch, 'fp32', 50, 256, 256, 1) == per_window + _table_bytes(50, 9, 50)
    assert engine.cine_scratch_bytes(arch, 'fp32', 50, 256, 256, 1, per_window) == 0
    assert engine.cine_scratch_bytes(arch, 'bf16', 50, 256, 256, 1, 0) == 0              # no bf16 Temporal-UNet


def test_planner_properties():
    from ukbb_cardiac_amd import engine
    from ukbb_cardiac_amd.arch import MODELS
    rng = np.random.default_rng(20261016)
    archs = [MODELS['UNet-LSTM_ao'], MODELS['Temporal-UNet_ao']]
    chunked = 0
    for _ in range(300):
        arch = archs[int(rng.integers(0, 4) == 0)]
        prec = 'fp32' if arch.kind == 3 else ('fp32', 'bf16')[int(rng.integers(0, 2))]
        F, ts = int(rng.integers(4, 420)), int(rng.integers(1, 14))
        H, W = 16 * int(rng.integers(1, 17)), 16 * int(rng.integers(1, 17))
        req = (arch, prec, F, H, W, ts)
        whole = engine.cine_scratch_bytes(*req, 0)
        low = engine.cine_min_scratch_bytes(*req)
        Wn = _cdiv(F, ts)
        assert whole > 0 and 0 < low
        if arch.kind == 2:
            assert low <= whole
            assert engine.cine_scratch_bytes(*req, whole) == whole                       # a budget at the unchunked size: unchunked
            assert engine.cine_scratch_bytes(*req, whole + int(rng.integers(1, 1 << 40))) == whole
            assert engine.cine_chunk_windows(*req, whole) == Wn
        assert engine.cine_scratch_bytes(*req, low - 1) == 0                             # below the minimum: refused
        assert engine.cine_chunk_windows(*req, low - 1) == 0
        assert engine.cine_scratch_bytes(*req, low) == low
        top = max(whole, low)
        budgets = sorted({low, top} | {int(b) for b in rng.integers(low, top + 1, size=6)})
        prev_bytes, prev_wc = 0, 0
        for b in budgets:
            got, wc = engine.cine_scratch_bytes(*req, b), engine.cine_chunk_windows(*req, b)
            assert 0 < got <= b, (req[1:], b, got)
            assert 1 <= wc <= Wn
            assert got >= prev_bytes and wc >= prev_wc, 'not monotonic in the budget'
            prev_bytes, prev_wc = got, wc
            chunked += wc < Wn
    assert chunked > 300                                                                 # the sweep does exercise chunk plans


@pytest.mark.parametrize('bad', [dict(F=0), dict(F=3), dict(H=40), dict(W=8), dict(ts=0), dict(ts=-2), dict(prec_code=2), dict(prec_code=-1),
                                 dict(model='UNet_ao'), dict(model='FCN_sa'), dict(F=1 << 20, H=256, W=256)])
def test_malformed_requests_give_0(bad):
    import ctypes as C
    from ukbb_cardiac_amd import _lib
    from ukbb_cardiac_amd.arch import MODELS
    a = _lib.arch_struct(MODELS[bad.get('model', 'UNet-LSTM_ao')])
    q = (C.byref(a), bad.get('prec_code', 0), bad.get('F', 20), bad.get('H', 64), bad.get('W', 64), bad.get('ts', 1))
    good = _lib.arch_struct(MODELS['UNet-LSTM_ao'])
    assert _lib.lib.ukbb_fcn_cine_scratch_bytes(C.byref(good), 0, 20, 64, 64, 1, 0) > 0
    assert _lib.lib.ukbb_fcn_cine_scratch_bytes(*q, 0) == 0
    assert _lib.lib.ukbb_fcn_cine_scratch_bytes(*q, 1 << 40) == 0
    assert _lib.lib.ukbb_fcn_cine_min_scratch_bytes(*q) == 0
    assert _lib.lib.ukbb_fcn_cine_scratch_bytes(None, 0, 20, 64, 64, 1, 0) == 0
    bad_arch = _lib.arch_struct(MODELS['UNet-LSTM_ao'])
    bad_arch.n_level = 0
    assert _lib.lib.ukbb_fcn_cine_scratch_bytes(C.byref(bad_arch), 0, 20, 64, 64, 1, 0) == 0


def test_chunk_terms_follow_the_window_order():
    """The chunk form of the tiling adds, per frame, the terms of windows [w0, w1) in ascending w: over ascending chunks that is the
    one-pass order, whatever Wc -- checked on the numpy restatement of the reference's loop (fancy-indexed `+=`, last write wins)."""
    from oracle import fcn_oracle as O
    rng = np.random.default_rng(5)
    for F, ts, Wc in [(13, 1, 2), (25, 2, 3), (4, 1, 1), (9, 3, 2), (12, 10, 1), (50, 1, 7)]:
        Wn, T = _cdiv(F, ts), 9
        p = rng.random((Wn, T)).astype(np.float32)                           # one "pixel" per (window, step)
        w = O.aortic_window_weights(5, 0.1)
        one = np.zeros(F, np.float32)
        for i, t in enumerate(range(0, F, ts)):
            one[O.aortic_window_indices(t, F, 5)] += p[i] * w
        acc = np.zeros(F, np.float32)
        for w0 in range(0, Wn, Wc):                                          # the float32 accumulator is carried between chunks
            part = acc.copy()
            for i in range(w0, min(w0 + Wc, Wn)):
                part[O.aortic_window_indices(i * ts, F, 5)] += p[i] * w
            acc = part
        assert np.array_equal(one.view(np.uint32), acc.view(np.uint32))


def test_cine_scratch_gb_flag():
    from ukbb_cardiac_amd import deploy_network_ao
    from ukbb_cardiac_amd.flags import FlagError
    fs = deploy_network_ao.define_flags()
    assert fs.parse([])[0].cine_scratch_gb == 0
    assert fs.parse(['--cine_scratch_gb', '4'])[0].cine_scratch_gb == 4.0
    assert fs.parse(['--cine_scratch_gb=0.5'])[0].cine_scratch_gb == 0.5
    for argv in (['--cine_scratch_gb', '-1'], ['--cine_scratch_gb=-0.25'], ['--cine_scratch_gb', 'nan'], ['--cine_scratch_gb', 'lots']):
        with pytest.raises(FlagError):
            fs.parse(argv)
    assert 'cine_scratch_gb' in fs.usage()
