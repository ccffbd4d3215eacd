"""What tests/test_head_launches_gpu.py covers, checked without a GPU, and that its bounds can tell a wrong squeeze or head from a right one.

Coverage: the situations of the squeeze launcher and of the head's tile walk are computed on the host from N, H, W, the launcher's constants (read
from kernels_head.hip) and 256 compute units (plan_layout's default; one head workgroup per CU).  CASES reaches every one of them, and dropping any one
case leaves a situation unreached.

The reference can tell a defect: on rough 48 x 32 inputs, conv0..conv4 from a float64 encoder forward, a head reference with one planted defect
(border taps renormalised, up_l's source shifted by a pixel, pad-before f/2, a level's term left out, two out0 slices swapped, a same_dim channel
zeroed) misses 1e-5 of the logits' scale by more than 100x, per level; the unchanged reference evaluated in float32 passes.

Softmax bound: the float32 numpy softmax passes 1e-6 on these logits; one bf16 ulp (2^-8 relative) in one exponential does not."""
import os
import re

import numpy as np
import pytest

import launch_grading as G
import test_head_launches_gpu as HL
from oracle import fcn_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = G.CUS                             # 256, engine.plan_layout's default; launch_head_pc: one workgroup per CU
HT = 16
WIN = {1: 9, 2: 6, 3: 4, 4: 3}          # kernels_head.hip win_n


def launcher_constants():
    with open(os.path.join(ROOT, 'ukbb_cardiac_amd', 'csrc', 'kernels_head.hip')) as f:
        src = f.read()
    cap = int(re.search(r'hipError_t launch_sqg_multi\(.*?if \(wg > (\d+)\) wg = \1;', src, re.S).group(1))
    ht = int(re.search(r'constexpr int HT = (\d+);', src).group(1))
    win = re.search(r'int win_n\(int l\) \{ return l == 1 \? (\d+) : l == 2 \? (\d+) : l == 3 \? (\d+) : (\d+); \}', src).groups()
    assert 'blk += (long long)vgrid * 4' in src and '(a.npix + 31) >> 5' in src       # four waves per workgroup, 32 pixels per wave
    return cap, ht, {l + 1: int(v) for l, v in enumerate(win)}


def window(l, origin, size):
    """(first, one past the last) window row or column of level l that lies inside the map, for a tile at ``origin`` of an axis of ``size`` pixels
    (fcn_head_pc_kernel g_load: ylo / yhi)."""
    n, s0 = size >> l, (origin >> l) - 1
    return (-s0 if s0 < 0 else 0), min(n - s0, WIN[l])


def situations(model, n, H, W, cap=2048):
    from ukbb_cardiac_amd import engine
    from ukbb_cardiac_amd.arch import MODELS
    out = {'%d classes' % MODELS[model].n_class}
    ty, tx = H // HT, W // HT
    ntiles = n * ty * tx
    grid = min(ntiles, CUS)
    per_wg = [(ntiles - b + grid - 1) // grid for b in range(grid)]
    # ---- head ----
    if ntiles == 1:
        out.add('single tile')
    out.add('fewer tiles than workgroups' if ntiles < CUS else 'as many tiles as workgroups' if ntiles == CUS else 'more tiles than workgroups')
    if 1 in per_wg:
        out.add('a workgroup with exactly one tile')
    if 1 in per_wg and max(per_wg) > 1:
        out.add('workgroups with one tile and with more in one launch')
    if any(t >= 2 and t % 2 == 0 for t in per_wg):
        out.add('a workgroup with an even number of tiles')
    if any(t >= 3 and t % 2 == 1 for t in per_wg):
        out.add('a workgroup with an odd number of tiles >= 3')
    if n > 1 and max(per_wg) > 1 and any(b // (ty * tx) != (b + grid) // (ty * tx) for b in range(grid) if b + grid < ntiles):
        out.add('consecutive tiles of a workgroup in different images')
        if grid % (ty * tx):
            out.add('consecutive tiles of a workgroup at different positions of different images')
    both = lambda size, origin: all(lo > 0 and hi < WIN[l] for l in (2, 3, 4) for lo, hi in [window(l, origin, size)])
    if ntiles > 1 and all(both(W, x0) for x0 in range(0, W, HT)):
        out.add('every tile: window columns outside the map on both sides, levels 2-4')
    if ntiles > 1 and all(both(H, y0) for y0 in range(0, H, HT)):
        out.add('every tile: window rows outside the map on both sides, levels 2-4')
    if (H >> 4) % 2 == 1 and (W >> 4) % 2 == 1 and min(H >> 4, W >> 4) > 1:
        out.add('odd level-4 map')
    # ---- squeeze ----
    for l in range(1, 5):
        per_image = (H >> l) * (W >> l)
        npix = n * per_image
        body = 'sqg_stream_body' if l <= 2 else 'sqg_body'
        if npix % 32:
            out.add('partial 32-pixel block in ' + body)
        if n > 1 and per_image % 32:
            out.add('a 32-pixel squeeze block spanning images')
        wg = ((npix + 31) // 32 + 3) // 4
        if wg > cap:
            out.add('squeeze loop past the cap')
        elif wg > cap - cap // 100:
            out.add('squeeze grid just under the cap, no loop')
    # ---- the conv plan in front ----
    arch = MODELS[model]
    if n > 1 and [o['cfg'] for o in engine.plan_layout(arch, 'fp32', n, H, W)['ops']] != [o['cfg'] for o in engine.plan_layout(arch, 'fp32', 1, H, W)['ops']]:
        out.add('large-batch conv plan in front')
        if ntiles < CUS:
            out.add('large-batch conv plan in front, fewer tiles than workgroups')
    return out


REQUIRED = {
    '2 classes', '3 classes', '4 classes', '6 classes',
    'single tile', 'partial 32-pixel block in sqg_stream_body', 'partial 32-pixel block in sqg_body',
    'every tile: window columns outside the map on both sides, levels 2-4', 'every tile: window rows outside the map on both sides, levels 2-4',
    'odd level-4 map',
    'fewer tiles than workgroups', 'as many tiles as workgroups', 'more tiles than workgroups',
    'a workgroup with exactly one tile', 'workgroups with one tile and with more in one launch',
    'a workgroup with an even number of tiles', 'a workgroup with an odd number of tiles >= 3',
    'consecutive tiles of a workgroup in different images', 'consecutive tiles of a workgroup at different positions of different images',
    'a 32-pixel squeeze block spanning images',
    'squeeze loop past the cap', 'squeeze grid just under the cap, no loop',
    'large-batch conv plan in front', 'large-batch conv plan in front, fewer tiles than workgroups',
}


def test_launcher_constants_are_the_ones_assumed():
    cap, ht, win = launcher_constants()
    assert (cap, ht, win) == (2048, HT, WIN)
    assert cap * 4 * 32 == 262144 < 17 * 128 * 128


def test_cases_reach_every_situation_and_none_is_idle():
    from ukbb_cardiac_amd.arch import KIND_FCN, MODELS
    assert len(set(HL.CASES)) == len(HL.CASES)
    assert {m for m, _, _, _ in HL.CASES} == {k for k, a in MODELS.items() if a.kind == KIND_FCN}        # all four class-count instantiations
    assert all(H % 16 == 0 and W % 16 == 0 and H >= 16 and W >= 16 and n >= 1 for _, n, H, W in HL.CASES)  # 16 x 16 tiling, integral level sizes
    at = {c: situations(*c) for c in HL.CASES}
    for c, s in at.items():
        print(c, sorted(s))
    G.no_case_is_idle(HL.CASES, at.__getitem__, REQUIRED)
    # the cases the docstring names, where it names them
    assert 'single tile' in at[('FCN_sa', 1, 16, 16)] and 'squeeze loop past the cap' in at[('FCN_sa', 17, 256, 256)]
    assert 'squeeze loop past the cap' not in at[('FCN_sa', 17, 240, 256)]
    assert [n * (H // 16) * (W // 16) for _, n, H, W in HL.CASES] == [1, 3, 9, 105, 105, 105, 256, 323, 4352, 4080, 68]
    assert all(HL.CASES[i][1] <= 3 and HL.CASES[i][2] * HL.CASES[i][3] <= 80 * 112 for i in HL.CHILD_CASES)


def test_modes_and_the_plans_behind_them():
    """Every case runs in the three precisions; in each the plan ends in the same sqg1-4 and head launches on the same maps (engine.cpp switches the
    head's arithmetic for f32x3 only), and in bf16 every conv in front of them from conv1_0 on is a bf16-operand tiling storing fp32 maps, so the
    squeeze and head of that mode are fp32 launches on maps another kernel family stored.  The knob children keep fp32 and f32x3."""
    from ukbb_cardiac_amd import engine
    from ukbb_cardiac_amd.arch import MODELS
    assert HL.MODES == ('fp32', 'f32x3', 'bf16') and set(HL.CHILD_MODES) == {'fp32', 'f32x3'}
    for model, n, H, W in HL.CASES:
        tails = {}
        for mode in HL.MODES:
            p = engine.plan_layout(MODELS[model], mode, n, H, W)
            assert not p['bfio'], (model, mode)                                         # fp32 maps in HBM in every mode
            tails[mode] = [(o['name'], o['kind'], o['H'], o['W']) for o in p['ops'] if o['kind'] != 'conv']
            acts = [(a['name'], a['per_image'], a['channels']) for a in p['acts']]
            assert [t[0] for t in tails[mode]] == ['sqg1-4', 'head'] and {'conv%d' % l for l in range(5)} | {'g%d' % l for l in range(1, 5)} <= {a[0] for a in acts}
            on_bf16 = [G.config_name(o['cfg']).startswith('convBF16_') for o in p['ops'] if o['kind'] == 'conv' and '+' not in o['name']]
            assert len(on_bf16) == 11 and all(v == (mode == 'bf16') for v in on_bf16), (model, mode)
        assert tails['fp32'] == tails['f32x3'] == tails['bf16']


def test_window_arithmetic_against_the_taps_of_the_reference():
    """window() marks as inside exactly the source rows that the reference's taps of a tile's 16 output rows read with a non-zero weight or
    would read inside the map: rows (y + pb) >> l and one less, pb = (2^l - 1) // 2."""
    for size in (16, 48, 144, 272):
        for l in (1, 2, 3, 4):
            f, n = 1 << l, size >> l
            for origin in range(0, size, HT):
                y = np.arange(origin, origin + HT)
                i1 = (y + (f - 1) // 2) >> l
                rows = set(i1) | set(i1 - 1)
                s0 = (origin >> l) - 1
                assert min(rows) >= s0 and max(rows) < s0 + WIN[l]
                lo, hi = window(l, origin, size)
                assert {r for r in rows if 0 <= r < n} == {r for r in range(s0 + lo, s0 + hi)} & rows
                assert all(0 <= r < n for r in range(s0 + lo, s0 + hi))


# ---- the reference can tell a defect ----------------------------------------------------------------------------------------------------------------------
def up_variant(x, l, pad_before=None, renorm=False):
    """transpose_upsample2d_separable with a planted defect: another pad-before, or border taps renormalised to sum to one."""
    f = 1 << l
    pb = (f - 1) // 2 if pad_before is None else pad_before

    def taps(n_in):
        o = np.arange(n_in * f)
        i1 = (o + pb) // f
        j1 = (o + pb) - i1 * f
        w1 = np.where(i1 < n_in, (j1 + 1) / f, 0.0)
        w0 = np.where(i1 - 1 >= 0, (f - 1 - j1) / f, 0.0)
        if renorm:
            s = w0 + w1
            w0, w1 = w0 / s, w1 / s
        return np.clip(i1 - 1, 0, n_in - 1), w0, np.clip(i1, 0, n_in - 1), w1

    y0, wy0, y1, wy1 = taps(x.shape[1])
    x0, wx0, x1, wx1 = taps(x.shape[2])
    rows = x[:, y0] * wy0[None, :, None, None] + x[:, y1] * wy1[None, :, None, None]
    return rows[:, :, x0] * wx0[None, None, :, None] + rows[:, :, x1] * wx1[None, None, :, None]


def shifted(x, axis):
    out = np.zeros_like(x)
    dst, src = [slice(None)] * 4, [slice(None)] * 4
    dst[axis], src[axis] = slice(1, None), slice(0, -1)
    out[tuple(dst)] = x[tuple(src)]
    return out


@pytest.fixture(scope='module')
def small():
    """conv0..conv4 of the three rough 48 x 32 images from a float64 encoder forward (rounded to float32, as the engine stores them), per seed."""
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.weights import synthetic_params
    out = []
    for seed in G.SEEDS:
        params = synthetic_params(MODELS['FCN_sa'], seed)
        _, net = O.build_FCN(G.distinct_images(48, 32), params, 4, dtype=np.float64, return_net=True)
        conv = {l: net['conv%d' % l].astype(np.float32) for l in range(5)}
        g = {l: HL.squeeze_map(conv[l], params, l) for l in range(1, 5)}
        out.append((params, conv, g, HL.head_logits(conv[0], g, params)))
    return out


def test_up_variant_without_a_defect_is_the_oracle(small):
    _, _, g, _ = small[0]
    for l in range(1, 5):
        assert np.array_equal(up_variant(g[l], l), O.transpose_upsample2d_separable(g[l], 1 << l))
        dense = O.transpose_upsample2d(g[l][:1, :, :, :3], 1 << l)                       # the reference's own dense form, float64 input
        assert np.abs(dense - up_variant(g[l][:1, :, :, :3], l)).max() <= 1e-12 * np.abs(dense).max()


def test_float32_reference_passes_the_bounds(small):
    for params, conv, g, full in small:
        for l in range(1, 5):
            g32 = HL.squeeze_map(conv[l], params, l, np.float32)
            assert g32.dtype == np.float32 and G.rel_err(g32, g[l])[0] <= HL.BOUND
        lg32 = HL.head_logits(conv[0], {l: g[l].astype(np.float32) for l in g}, params, np.float32)
        assert lg32.dtype == np.float32 and G.rel_err(lg32, full)[0] <= HL.BOUND


def _defects(params, conv, g):
    """(name, level, logits of the head reference with the defect planted)."""
    H = HL.head_logits
    sd = {l: HL.same_dim(conv[l], params, l) for l in range(5)}
    proj = lambda l, m, s=None: (sd[l] if s is None else s) @ HL.out0_slice(params, m)     # level l's same_dim map through level m's out0 slice
    for l in range(1, 5):
        only = lambda fn, l=l: (lambda x, k: fn(x, k) if k == l else HL.upsample(x, k))
        yield 'border taps renormalised', l, H(conv[0], g, params, up=only(lambda x, k: up_variant(x, k, renorm=True)))
        yield 'source shifted along y', l, H(conv[0], g, params, up=only(lambda x, k: HL.upsample(shifted(x, 1), k)))
        yield 'source shifted along x', l, H(conv[0], g, params, up=only(lambda x, k: HL.upsample(shifted(x, 2), k)))
        yield 'pad-before f/2', l, H(conv[0], g, params, up=only(lambda x, k: up_variant(x, k, pad_before=(1 << k) // 2)))
        yield 'term left out', l, H(conv[0], g, params, up=only(lambda x, k: np.zeros((x.shape[0], x.shape[1] << k, x.shape[2] << k, 64))))
    for l in range(5):
        for m in range(l + 1, 5):                                                         # out0 slices of levels l and m swapped
            gs = dict(g)
            gs[m] = proj(m, l)
            if l:
                gs[l] = proj(l, m)
            yield 'out0 slices swapped with level %d' % l, m, H(conv[0], gs, params, term0=None if l else proj(0, m))
    for l in range(5):
        live = np.flatnonzero(sd[l].reshape(-1, 32).max(axis=0) > 0)
        c = int(live[len(live) // 2])                                                    # one channel that is not dead at these weights
        z = sd[l].copy()
        z[..., c] = 0.0
        if l:
            yield 'same_dim channel %d zeroed' % c, l, H(conv[0], {**g, l: proj(l, l, z)}, params)
        else:
            yield 'same_dim channel %d zeroed' % c, l, H(conv[0], g, params, term0=proj(0, 0, z))


def test_bound_tells_each_planted_defect(small):
    """Every defect, at every level it can be planted at, misses the logits bound by more than 100x: a head with it cannot pass."""
    for seed, (params, conv, g, full) in zip(G.SEEDS, small):
        for name, l, bad in _defects(params, conv, g):
            err, _ = G.rel_err(bad, full)
            print('seed %4d level %d %-36s logits error / scale %.2e' % (seed, l, name, err))
            assert err > 100 * HL.BOUND, (seed, name, l, err)


def test_squeeze_bound_tells_a_defect(small):
    """g_l with the out0 slice of another level, a same_dim channel zeroed, or its input pixel one off, misses 1e-5 of g_l's scale by more than 100x."""
    for params, conv, g, _ in small:
        for l in range(1, 5):
            sd = HL.same_dim(conv[l], params, l)
            for m in range(5):
                if m != l:
                    assert G.rel_err(sd @ HL.out0_slice(params, m), g[l])[0] > 100 * HL.BOUND, (l, m)
            z = sd.copy()
            z[..., int(np.argmax(sd.reshape(-1, 32).max(axis=0)))] = 0.0
            assert G.rel_err(z @ HL.out0_slice(params, l), g[l])[0] > 100 * HL.BOUND, l
            flat = conv[l].reshape(-1, conv[l].shape[-1])
            off = HL.squeeze_map(np.roll(flat, 1, axis=0), params, l).reshape(g[l].shape)
            assert G.rel_err(off, g[l])[0] > 100 * HL.BOUND, l


# ---- softmax ------------------------------------------------------------------------------------------------------------------------------------------------
def softmax32(lg, spoil=None):
    """The engine's form (kernels.h softmax_argmax) in float32 numpy: e = exp(l - m), p = e * (1 / sum e)."""
    lg = np.asarray(lg, np.float32)
    e = np.exp(lg - lg.max(axis=-1, keepdims=True))
    assert e.dtype == np.float32
    if spoil is not None:
        e[spoil] = e[spoil] * np.float32(1 + 2.0 ** -8)
    return e * (np.float32(1) / e.sum(axis=-1, keepdims=True, dtype=np.float32))


def test_softmax_bound(small):
    rng = np.random.default_rng(3)
    for n_class in (2, 3, 4, 6):
        for _, _, _, full in small:
            lg = full.astype(np.float32)
            if n_class != lg.shape[-1]:                                  # other class counts: these logits' range, resampled over the channel axis
                lg = np.concatenate([lg, lg[:, ::-1], lg[:, :, ::-1]], axis=-1)[..., rng.permutation(12)[:n_class]]
            p = softmax32(lg)
            assert p.dtype == np.float32
            assert np.abs(p.astype(np.float64) - HL.softmax64(lg)).max() <= HL.PROB_ATOL
            idx = np.unravel_index(int(np.argmax(HL.top2_gap(lg) * -1)), lg.shape[:-1])      # the pixel nearest a tie: both top classes near 1/2
            bad = softmax32(lg, idx + (int(np.argmax(lg[idx])),))
            assert np.abs(bad.astype(np.float64) - HL.softmax64(lg)).max() > HL.PROB_ATOL
