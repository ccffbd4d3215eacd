"""What the float64 launch graders share (tests/test_*_launches_gpu.py, tests/test_*_layers_gpu.py and their CPU coverage files
tests/test_*_launch_coverage.py, tests/test_fcn_bf16_store.py), each written once.  A plain helper module: functions and constants, imported with
numpy and the oracle alone; ukbb_cardiac_amd is imported inside the functions that need it, so a CPU test reaches a helper without a `gpu` module.

THE METHOD the graders share.  One forward per case.  Every stored map is read back (Engine.activation) and recomputed ALONE in numpy float64
(oracle/fcn_oracle.py conv2d_same / conv2d_transpose_same, the float32 BN fold of engine.cpp create(): fold, layer) from the map or maps the
engine ITSELF stored in front of it, so a launch's deviation is its kernel's own and no error is carried from layer to layer.  A batch is made of
copies of at most three distinct rough images, img[i] = distinct[i % 3] (distinct_images: a phantom slice, a uniform-noise slice, standard-normal
noise scaled to the phantom's range -- rough, so that a wrong tap is not hidden by a smooth image; batch_of_copies, normalised_copies).  Slices
0, 1, 2 are graded in float64 -- the float64 cost does not grow with the batch -- and every other slice of every stored map and output must be
BIT-IDENTICAL to the graded copy of its image and hold no NaN (check_copies): that grades all N slices and asserts batch independence inside every
large-batch tiling.  A batch of one takes the three images in turn over the case list; weights come from seeds 1234 and 7 in turn.  The plan that
ran must be the plan the CPU coverage file counted for the case (assert_plan_ran: kernel_names() / kernel_configs() equal plan_layout's).

fp32 launches are held to a share of the layer's largest activation (rel_err); bf16-storing launches to half a bf16 ulp of the exact value of the
specified arithmetic, + 2^-18 |exact| for the fp32 accumulation, + 2^-20 of the layer's scale for values ReLU brings next to zero (tolerance,
grade, measure).  The bf16-storage graders run on an engine created under UKBB_DEBUG_GUARD and poisoned in front of the forward (guarded_engine,
POISON): a tile nobody wrote holds NaN, not a leftover.  Forms behind environment variables that a process latches run in a fresh child process
with a scrubbed environment (run_in_child).

The planner side (config_name, tile_of, fit_of, replay_records, no_case_is_idle) and the mirror of the walker launchers' grid arithmetic (ws_launch,
stem_launch, tail_launch, launch_class; its constants are asserted against the sources in tests/test_bf16_launch_coverage.py) are what the coverage
files count situations with, and what the graders name a launch's situation with in the rows they print.

The Temporal-UNet (tests/test_temporal_launches_gpu.py, tests/test_temporal_launch_coverage.py) takes the same graph (launches) on 3-D units: layer3d
on tests/temporal_unet_ref.py, batches of windows (distinct_windows, window_batch), the mirror of launch_conv3d's arithmetic (conv3d_launch) and the
grid caps of the kind's two grid-stride kernels read from the source (grid_caps_3d)."""
import json
import os
import re
import subprocess
import sys

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
if ROOT not in sys.path:                                            # the oracle, when imported outside pytest (tests/conftest.py does the same)
    sys.path.insert(0, ROOT)
if TESTS not in sys.path:                                           # tests/temporal_unet_ref.py, likewise
    sys.path.insert(0, TESTS)

from oracle import fcn_oracle as O                                  # noqa: E402

GOLDEN = os.path.join(TESTS, 'golden', 'plan_layouts.json')
SEEDS = (1234, 7)
BN_EPS = np.float32(1e-3)
CUS = 256                                                          # the plans are counted for an MI355X
POISON = '7FC07FC0'                                                # bf16 NaN pairs (one fp32 NaN): no layer produces it from finite inputs


# ---- the arithmetic of one launch -------------------------------------------------------------------------------------------------------------------
def bf16_round(x):
    """float32 -> nearest bf16 (ties to even), returned as float32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7fff)
    return ((u + r) & np.uint32(0xffff0000)).view(np.float32)


def fold(p, transposed=False):
    """engine.cpp create(): sc = gamma / sqrtf(var + eps); W' = W * sc; b' = beta - mean * sc, all float32, no contraction.  A layer without BN
    keeps its kernel and bias.  2-D ([kh,kw,Cin,Cout], transposed [kh,kw,Cout,Cin]) and 3-D kernels ([kd,kh,kw,Cin,Cout], [kd,kh,kw,Cout,Cin]) alike."""
    k = p['kernel'].astype(np.float32)
    if 'gamma' not in p:
        return k, p['bias'].astype(np.float32)
    sc = (p['gamma'].astype(np.float32) / np.sqrt(p['var'].astype(np.float32) + BN_EPS)).astype(np.float32)
    ms = (p['mean'].astype(np.float32) * sc).astype(np.float32)
    b = (p['beta'].astype(np.float32) - ms).astype(np.float32)
    return (k * (sc[:, None] if transposed else sc)).astype(np.float32), b          # the scale runs over Cout: the last axis, or the one before it


def layer(x, p, stride=1, transposed=False, relu=True, round_w=False, round_x=False):
    """One conv2d_bn_relu / conv2d_transpose_bn_relu / biased conv in float64 on the given input: the exact result of the launch's specified
    arithmetic before any rounding of the output.  No flag: an fp32 launch.  round_w: the folded kernel rounded to bf16 (a bf16-storage launch, on
    its bf16-valued stored input).  round_w and round_x: the input rounded to bf16 as well (a bf16-operand launch on fp32 maps)."""
    w, b = fold(p, transposed)
    if round_w:
        w = bf16_round(w)
    if round_x:
        x = bf16_round(x)
    x, w = np.asarray(x, np.float64), w.astype(np.float64)
    y = (O.conv2d_transpose_same(x, w, stride) if transposed else O.conv2d_same(x, w, stride)) + b.astype(np.float64)
    return np.maximum(y, 0.0) if relu else y


def layer3d(x, p, stride=1, transposed=False, relu=True):
    """One conv3d_bn_relu / conv3d_transpose_bn_relu / biased 1x1x1 conv of the Temporal-UNet in float64 on x [N,T,H,W,C] (tests/temporal_unet_ref.py
    conv3d_same / conv3d_transpose_same; time stride 1, `stride` in space), with the engine's float32 fold applied to float64 copies."""
    import temporal_unet_ref as R3
    w, b = fold(p, transposed)
    x, w = np.asarray(x, np.float64), w.astype(np.float64)
    y = (R3.conv3d_transpose_same(x, w, stride) if transposed else R3.conv3d_same(x, w, stride)) + b.astype(np.float64)
    return np.maximum(y, 0.0) if relu else y


def half_ulp(v):
    """Half a bf16 ulp at |v| (float64 array): bf16 keeps 8 significant bits."""
    a = np.maximum(np.abs(v), 1e-30)
    return np.exp2(np.floor(np.log2(a)) - 8)


def tolerance(exact, scale, ulps):
    """`ulps` bf16 ulps of the exact value, + a 2^-18 relative slack for the fp32 accumulation, + an absolute floor for values next to zero."""
    return 2 * ulps * half_ulp(exact) + np.abs(exact) * 2.0 ** -18 + scale * 2.0 ** -20


def grade(name, got, exact, scale, ulps=0.5, fraction=1.0):
    """got: the engine's stored bf16 values; exact: float64 result of the specified arithmetic before the final rounding."""
    got = np.asarray(got, np.float64).reshape(exact.shape)
    ok = np.abs(got - exact) <= tolerance(exact, scale, ulps)
    assert ok.mean() >= fraction, '%s: %.5f of the elements within %.1f bf16 ulp of the specified result (asked %.5f); worst %.3g at value %.3g' % (
        name, ok.mean(), ulps, fraction, float(np.abs(got - exact).max()), float(exact.flat[np.abs(got - exact).argmax()]))
    return float(ok.mean())


def measure(got, exact, scale, ulps=0.5):
    """(share of the elements inside grade()'s tolerance at `ulps`, worst |got - exact| over that tolerance)."""
    got = np.asarray(got, np.float64).reshape(exact.shape)
    r = np.abs(got - exact) / tolerance(exact, scale, ulps)
    return float(np.mean(r <= 1.0)), float(r.max())


def rel_err(got, ex):
    """(max |got - ex| / max |ex|, index of the worst element)."""
    d = np.abs(np.asarray(got, np.float64) - ex)
    return float(d.max()) / float(np.abs(ex).max()), tuple(int(v) for v in np.unravel_index(int(d.argmax()), d.shape))


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------------
def distinct_images(H, W):
    """The three input kinds, [3, H, W, 1] float32: a phantom slice, a uniform-noise slice, standard-normal noise scaled to the phantom's range."""
    from ukbb_cardiac_amd.phantom import cine_phantom, uniform_slices
    ph = cine_phantom(1, H, W, seed=17)[0]
    un = uniform_slices(1, H, W, seed=5)[0]
    z = np.random.default_rng(29).standard_normal((H, W, 1))
    lo, hi = float(ph.min()), float(ph.max())
    nz = (lo + (z - z.min()) / (z.max() - z.min()) * (hi - lo)).astype(np.float32)
    return np.stack([ph, un, nz]).astype(np.float32)


def batch_of_copies(index, n, H, W):
    """img[i] = distinct[i % 3]; a batch of one takes the three kinds in turn over the case list.  Returns (batch, number of distinct images)."""
    d = distinct_images(H, W)
    if n == 1:
        return d[index % 3:index % 3 + 1].copy(), 1
    return np.stack([d[i % 3] for i in range(n)]), min(n, 3)


def normalised_copies(index, n, H, W):
    """batch_of_copies, normalised as tests/test_bf16_layers_gpu.py normalises its phantom."""
    img, nd = batch_of_copies(index, n, H, W)
    return ((img - np.float32(0.3)) / np.float32(0.25)).astype(np.float32), nd


def distinct_windows(T, H, W):
    """The three input kinds as windows of T frames, [3, T, H, W, 1] float32, normalised as normalised_copies does: a cine_phantom window, a
    uniform-noise window, standard-normal noise scaled to the phantom's range.  The two noise windows are independent from frame to frame, so a wrong
    or reversed time tap is not hidden by a cine that is smooth in time."""
    from ukbb_cardiac_amd.phantom import cine_phantom, uniform_slices
    ph = cine_phantom(T, H, W, seed=17)
    un = uniform_slices(T, H, W, seed=5)
    z = np.random.default_rng(29).standard_normal((T, H, W, 1))
    lo, hi = float(ph.min()), float(ph.max())
    nz = (lo + (z - z.min()) / (z.max() - z.min()) * (hi - lo)).astype(np.float32)
    return ((np.stack([ph, un, nz]).astype(np.float32) - np.float32(0.3)) / np.float32(0.25)).astype(np.float32)


def window_batch(index, n, T, H, W):
    """batch_of_copies for windows: window i = distinct[i % 3]; a batch of one takes the three kinds in turn over the case list.  Returns
    (batch [n, T, H, W, 1], number of distinct windows)."""
    d = distinct_windows(T, H, W)
    if n == 1:
        return d[index % 3:index % 3 + 1].copy(), 1
    return np.stack([d[i % 3] for i in range(n)]), min(n, 3)


# ---- the graph --------------------------------------------------------------------------------------------------------------------------------------
def launches(arch):
    """The graph, launch by launch, as the reference defines it (common/network.py build_FCN's encoder, network_ao.py build_UNet; the Temporal-UNet
    is the same graph on 3-D units): (layer name, stored name, level, input stored names, stride, transposed, relu).  '' as the input is the image."""
    from ukbb_cardiac_amd.arch import KIND_FCN, KIND_TEMPORAL_UNET
    nb = arch.n_block

    def stored(kind, l, i):                                         # the 2-D plans name a level's last map after the level, the 3-D plan after its layer
        return '%s%d' % (kind, l) if i == nb[l] - 1 and arch.kind != KIND_TEMPORAL_UNET else '%s%d_%d' % (kind, l, i)
    out = []
    for l in range(arch.n_level):
        for i in range(nb[l]):
            src = '' if (l, i) == (0, 0) else stored('conv', l - 1, nb[l - 1] - 1) if i == 0 else stored('conv', l, i - 1)
            out.append(('conv%d_%d' % (l, i), stored('conv', l, i), l, [src], 2 if (l > 0 and i == 0) else 1, False, True))
    if arch.kind != KIND_FCN:                                       # UNet, UNet-LSTM, Temporal-UNet: the decoder and conv_out
        below = stored('conv', arch.n_level - 1, nb[-1] - 1)
        for l in range(arch.n_level - 2, -1, -1):
            out.append(('up%d_t' % l, 'up%d_t' % l, l, [below], 2, True, True))
            for i in range(nb[l]):
                src = [stored('conv', l, nb[l] - 1), 'up%d_t' % l] if i == 0 else [stored('up', l, i - 1)]      # skip first (network_ao.py:51)
                out.append(('up%d_%d' % (l, i), stored('up', l, i), l, src, 1, False, True))
            below = stored('up', l, nb[l] - 1)
        out.append(('logits', 'logits', 0, [below], 1, False, False))
    return out


# ---- identity checks --------------------------------------------------------------------------------------------------------------------------------
def check_copies(name, a, nd, what=''):
    """a[i] for i >= nd must be bit-identical to a[i % nd]; no NaN (the poison pattern) anywhere."""
    bits = a.view(np.uint32 if a.dtype.itemsize == 4 else a.dtype)
    if a.dtype.kind == 'f':
        assert not np.isnan(a).any(), '%s: holds the poison pattern (NaN) at slice, y, x, channel %s %s' % (name, tuple(int(v[0]) for v in np.nonzero(np.isnan(a))), what)
    for i in range(nd):
        same = bits[i + nd::nd] == bits[i]
        if not same.all():
            k = tuple(int(v[0]) for v in np.nonzero(~same))
            raise AssertionError('%s: slice %d differs from slice %d of the same image at y, x, channel %s %s' % (name, i + nd * (k[0] + 1), i, k[1:], what))


def check_bf16(name, a):
    assert not (a.view(np.uint32) & np.uint32(0xffff)).any(), '%s: stored values are not bf16' % name


def plan_cfgs(ops):
    """kernel_configs() of a plan's ops: the tiling of a conv / transposed conv, -1 for every other launch."""
    return [o['cfg'] if o['kind'] in ('conv', 'tconv') else -1 for o in ops]


def assert_plan_ran(eng, plan):
    """The plan that ran is the one the CPU coverage file counted for the case.  Returns (kernel_names(), kernel_configs())."""
    names, cfgs = eng.kernel_names(), eng.kernel_configs()
    assert names == [o['name'] for o in plan['ops']], (names, [o['name'] for o in plan['ops']])
    assert cfgs == plan_cfgs(plan['ops']), (cfgs, plan['ops'])
    return names, cfgs


# ---- the planner side -------------------------------------------------------------------------------------------------------------------------------
def config_name(cfg):
    from ukbb_cardiac_amd import _lib
    return _lib.lib.ukbb_fcn_conv_config_name(cfg).decode()


def tile_of(cfg):
    """(rows, columns) of a tiling's tile: from its name, "..._t<rows>x<columns>..." (tile per workgroup) or "..._r<rows>x32_..." (walkers)."""
    if cfg >= 400:
        return ws_shape(cfg)[0], WS_TW
    return tuple(map(int, re.search(r'_t(\d+)x(\d+)', config_name(cfg)).groups()))


def fit_of(op):
    """How the tiling's tile fits the op's output map: 'div' (it divides both axes), 'ragged' (some axis has whole tiles AND a partial last one: an
    edge tile whose halo comes from a neighbour on one side and from the zero padding on the other) or 'partial' (it does not divide, and every axis
    it does not divide holds one partial tile only).  Callers that count two situations take 'ragged' and 'partial' together as 'nodiv'."""
    th, tw = tile_of(op['cfg'])
    if op['Ho'] % th == 0 and op['Wo'] % tw == 0:
        return 'div'
    return 'ragged' if (op['Ho'] % th and op['Ho'] > th) or (op['Wo'] % tw and op['Wo'] > tw) else 'partial'


def replay_records(model, precision, reached):
    """[(n, H, W, reached(n, H, W))] over the recorded knob-less plans (tests/golden/plan_layouts.json: knob '', rc 0) of one model and precision.
    The records hold no map sizes per op, so each is replayed on the host planner, and the replay is checked against the record's own names and
    tilings (as tests/test_plan_layout.py does for all of them)."""
    from ukbb_cardiac_amd import engine
    from ukbb_cardiac_amd.arch import MODELS
    assert 'UKBB_CONV_CFG' not in os.environ
    with open(GOLDEN) as f:
        g = json.load(f)
    out = []
    for r in g['records']:
        name, prec, H, W, n, knob, rc = r[:7]
        if (name, prec, knob, rc) != (model, precision, '', 0):
            continue
        ops = engine.plan_layout(MODELS[model], precision, n, H, W, CUS)['ops']
        assert [o['name'] for o in ops] == g['names'][r[8]] and plan_cfgs(ops) == g['cfgs'][r[9]], r[:6]
        out.append((n, H, W, reached(n, H, W)))
    return out


def no_case_is_idle(cases, covered_of, want):
    """The cases reach all of `want` together, and dropping any one leaves some of it unreached.  Returns, per case, what only it reaches."""
    per_case = [covered_of(c) & want for c in cases]
    assert set().union(*per_case) == want, sorted(want - set().union(*per_case), key=str)
    only = []
    for i, c in enumerate(cases):
        rest = set().union(*(per_case[:i] + per_case[i + 1:]))
        assert want - rest, 'case %s adds nothing' % (c,)
        only.append(sorted(want - rest, key=str))
    return only


# ---- the walker launchers' grid arithmetic (constants asserted against the sources in tests/test_bf16_launch_coverage.py) ---------------------------
WS_TW = 32
STEM_R, STEM_NW, STEM_TW, STEM_WG_PER_CU = 8, 4, 30, 2
TAIL_R, TAIL_NW, TAIL_TW = 8, 8, 14
LAUNCHER_KNOBS = ('UKBB_WS_XCD_LOCAL', 'UKBB_TAIL_STRIPS', 'UKBB_TAIL_SEG')      # A/B switches of launch_conv_ws / launch_unet_tail: unset in the graders


def ws_shape(cfg):
    """(rows, cb, waves, transposed) of a weight-stationary tiling, from its name: "..._r<rows>x32_cb<cb>_w<waves>"."""
    name = config_name(cfg)
    m = re.search(r'^(t?)convBF16w[sr]_\dx\d(?:s1)?_r(\d+)x%d_cb(\d+)_w(\d+)$' % WS_TW, name)
    assert m, name
    return int(m.group(2)), int(m.group(3)), int(m.group(4)), m.group(1) == 't'


def round_class(ntiles, nworkers):
    if ntiles <= nworkers:
        return 'below'
    if ntiles < 2 * nworkers:
        return 'between'
    return 'two+ exact' if ntiles % nworkers == 0 else 'two+ ragged'


def ws_launch(op, acts, n, cus=CUS):
    """launch_conv_ws's arithmetic for one plan op: tiles, grid, workers, round class, tile order, columns, placement."""
    R, cb, wn, transposed = ws_shape(op['cfg'])
    ch = acts[op['out']]['channels']
    cout = 4 * ch if transposed else -(-ch // 32) * 32             # transposed: 4 phases x up2 virtual channels; up0_0 of UNet-LSTM: 16 padded to 32
    per_group = 64 if transposed else 32 * cb
    assert cout % per_group == 0, (op, ch)
    nG = cout // per_group
    H, W = op['H'], op['W']                                         # a transposed conv walks its INPUT map
    ntiles = n * -(-H // R) * -(-W // WS_TW)
    want = -(-ntiles // wn) * nG
    grid = cus // (8 * nG) * (8 * nG) if cus >= 8 * nG else cus // nG * nG
    grid = max(grid, nG)
    if want < grid:
        grid = -(-want // nG) * nG
    nworkers = grid // nG * wn
    return dict(ntiles=ntiles, nworkers=nworkers, grid=grid, nG=nG, cls=round_class(ntiles, nworkers), order='xcd' if H * W >= 128 * 128 else 'wave',
                cols='ragged columns' if W % WS_TW else 'whole columns', place='grid 8 nG' if grid % (8 * nG) == 0 else 'grid not 8 nG')


def stem_launch(n, H, W, cus=CUS):
    ntiles = n * -(-H // STEM_R) * -(-W // STEM_TW)
    grid = min(-(-ntiles // STEM_NW), STEM_WG_PER_CU * cus)
    return dict(ntiles=ntiles, nworkers=grid * STEM_NW, cls=round_class(ntiles, grid * STEM_NW))


def tail_launch(n, H, W, cus=CUS):
    """launch_unet_tail: grid, and the segment length of the strip walk (the split whose busiest worker has the fewest tiles; the longest among equals)."""
    tiles_y, tiles_x = -(-H // TAIL_R), -(-W // TAIL_TW)
    ntiles = n * tiles_y * tiles_x
    grid = min(-(-ntiles // TAIL_NW), cus)
    workers = grid * TAIL_NW
    best, best_seg = -1, tiles_y
    for segs in range(1, tiles_y + 1):
        seg = -(-tiles_y // segs)
        if -(-tiles_y // seg) != segs:
            continue
        cost = -(-(n * tiles_x * segs) // workers) * seg
        if best < 0 or cost < best:
            best, best_seg = cost, seg
    return dict(ntiles=ntiles, nworkers=workers, cls=round_class(ntiles, workers), seg=best_seg, segs=-(-tiles_y // best_seg), ragged=tiles_y % best_seg != 0)


def launch_class(op, acts, n):
    """The round class of a plan op as the record's rows name it ('-' for a tile-per-workgroup launch)."""
    if op['kind'] == 'stem':
        return stem_launch(n, op['H'], op['W'])['cls']
    if op['kind'] == 'tail':
        return tail_launch(n, op['H'], op['W'])['cls']
    if op['kind'] in ('conv', 'tconv') and op['cfg'] >= 400:
        w = ws_launch(op, acts, n)
        return '%s %s' % (w['cls'], w['order'])
    return '-'


# ---- the Temporal-UNet's launchers (kernels_conv3d.hip; constants asserted against the source in tests/test_temporal_launch_coverage.py) -------------
C3D_PIX, C3D_COB, C3D_WAVES = 32, 32, 4                            # pixels and output channels of one MFMA tile; items (waves) per workgroup
C3D_FIRST_CAP = 256 * 64 * 256                                     # threads launch_conv3d_first starts at most: beyond, conv3d_first_kernel's loop wraps
T3D_TILE_CAP = 256 * 16 * 256                                      # the same for launch_t3d_tile / t3d_tile_kernel


def grid_caps_3d():
    """(C3D_FIRST_CAP, T3D_TILE_CAP) as kernels_conv3d.hip holds them: the workgroup cap of launch_conv3d_first / launch_t3d_tile x 256 threads, each
    kernel's loop advancing by gridDim.x * 256.  A graded case that relies on a loop wrapping asserts these, so that a later change of a cap fails the
    test and does not silently void it."""
    with open(os.path.join(ROOT, 'ukbb_cardiac_amd', 'csrc', 'kernels_conv3d.hip')) as f:
        src = f.read()
    caps = []
    for launcher, kernel in (('launch_conv3d_first', 'conv3d_first_kernel'), ('launch_t3d_tile', 't3d_tile_kernel')):
        body = re.search(r'hipError_t %s\(.*?\n}\n' % launcher, src, re.S).group(0)
        m = re.search(r'long long blocks = \(total \+ 255\) / 256;\n    if \(blocks > (\d+) \* (\d+)\) blocks = \1 \* \2;', body)
        assert m and re.search(r'dim3\(\(unsigned\)blocks\), dim3\(256\)|dim3 g\(\(unsigned\)blocks\), t\(256\)', body), body     # a 1-D grid of 256 threads
        loop = re.search(r'void %s\(.*?\n}\n' % kernel, src, re.S).group(0)
        assert 'for (long long id = (long long)blockIdx.x * 256 + threadIdx.x; id < total; id += (long long)gridDim.x * 256)' in loop, loop
        caps.append(int(m.group(1)) * int(m.group(2)) * 256)
    assert tuple(caps) == (C3D_FIRST_CAP, T3D_TILE_CAP), caps
    return tuple(caps)


def conv3d_launch(op, acts, n_images, T):
    """launch_conv3d's arithmetic for one 'conv3d' / 'tconv3d' plan op on n_images = windows x T frames: the kernel's item count and the facets of the
    launch's situation.  A transposed conv walks its INPUT map, once per sub-pixel phase."""
    cout = acts[op['out']]['channels']
    cout_pad = -(-cout // C3D_COB) * C3D_COB
    cb = 2 if cout_pad % (2 * C3D_COB) == 0 else 1
    npix = op['H'] * op['W'] if op['kind'] == 'tconv3d' else op['Ho'] * op['Wo']
    ptiles, cgroups = -(-npix // C3D_PIX), cout_pad // C3D_COB // cb
    items = n_images * ptiles * cgroups
    kind = 'transposed' if op['kind'] == 'tconv3d' else 'two-source' if op['in1'] >= 0 else 'stride-%d' % op['stride']
    fit = 'divides' if npix % C3D_PIX == 0 else 'single pixel' if npix == 1 else 'one partial tile' if npix < C3D_PIX else 'whole tiles and a partial one'
    return dict(kind=kind, cb=cb, cgroups=cgroups, padded=cout < cout_pad, fit=fit, items=items, idle=items % C3D_WAVES,
                T='T=1' if T == 1 else 'T=3' if T == 3 else 'T>=5', windows='one window' if n_images == T else 'several windows')


class Report:
    """Rows of one case, printed as they are measured (before the assertion that may end the test)."""

    def __init__(self, tag, ops, acts, n):
        self.tag, self.n, self.acts, self.rows = tag, n, acts, []
        self.op_of = {part: o for o in ops for part in o['name'].split('+')}

    def row(self, lname, got, exact, scale):
        o = self.op_of[lname]
        share, worst = measure(got, exact, scale)
        cfg = o['cfg'] if o['kind'] in ('conv', 'tconv') else -1
        r = (self.tag, o['name'], cfg, launch_class(o, self.acts, self.n), share, worst)
        self.rows.append(r)
        print('bf16-launch %-22s %-18s tiling %3d  %-18s within half an ulp %.6f  worst / bound %.3f' % r)


# ---- the engine and the child process ---------------------------------------------------------------------------------------------------------------
def guarded_engine(monkeypatch, arch, params, precision):
    """A fresh engine created under UKBB_DEBUG_GUARD (every buffer filled with the poison pattern as it is allocated), the launchers' knobs unset."""
    from ukbb_cardiac_amd.engine import Engine
    for k in LAUNCHER_KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('UKBB_DEBUG_GUARD', POISON)                   # read in ukbb_fcn_create only
    eng = Engine(arch, params)
    eng.set_precision(precision)
    return eng


def fetcher(eng, shape_of, nd, cache, what):
    """fetch(stored name): one activation read back, checked (bf16 values, no poison, copies identical), slices 0..nd-1 kept."""
    def fetch(sname):
        if sname not in cache:
            a = eng.activation(sname).reshape(shape_of(sname))
            check_bf16(sname, a)
            check_copies(sname, a, nd, what)
            cache[sname] = a[:nd].copy()
        return cache[sname]
    return fetch


CHILD_PROGRAM = '''import importlib, json, sys
sys.path.insert(0, sys.argv[1])
getattr(importlib.import_module(sys.argv[2]), sys.argv[3])(*json.loads(sys.argv[4]))
'''


def run_in_child(module, function, args, knobs, timeout=300):
    """`module`.`function`(*args) of tests/ in a fresh child process whose environment is this one's without any UKBB_* variable, plus `knobs`
    ({name: value}) and the repository on PYTHONPATH; args must be JSON values.  Returns the CompletedProcess, stderr folded into stdout."""
    env = {k: v for k, v in os.environ.items() if not k.startswith('UKBB_')}
    env.update(knobs)
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    return subprocess.run([sys.executable, '-c', CHILD_PROGRAM, TESTS, module, function, json.dumps(list(args))], env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
