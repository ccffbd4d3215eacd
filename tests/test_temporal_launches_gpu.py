"""Every launch of the aortic Temporal-UNet (kernels_conv3d.hip, kind 3), one launch at a time, against float64 on the engine's OWN stored input; and the
two grid-stride loops of the kind, conv3d_first_kernel and t3d_tile_kernel, past their first pass.

tests/test_temporal_unet_gpu.py grades the launches of one case (the default architecture, 2 windows x 9 frames x 32 x 48, Gaussian noise).  This file
does it over the architectures plan.cpp supported() admits beyond that one -- windows of 1, 3 and 9 frames, 2, 3 and 4 classes, channel counts whose
padded count is no multiple of 64 above level 1 (conv3d_kernel<1> with 3 and 5 channel groups, a two-source conv of 96 + 96 channels, a three-block
level) -- and over the maps and window counts at which the item decomposition of conv3d_kernel changes: ARCH_CHANGES, CASES.
tests/test_temporal_launch_coverage.py computes each launch's situation on the CPU and shows that CASES reaches all of them, none idle.

The method is the graders' common one (tests/launch_grading.py): one run_seq per case on an engine created under UKBB_DEBUG_GUARD and poisoned first;
every stored map (conv*, up*_t, up*) and the logits read back; for windows 0..2 each launch recomputed alone in float64 (layer3d: conv3d_same /
conv3d_transpose_same of tests/temporal_unet_ref.py on the engine's float32 BN fold) from the map or maps the engine stored in front of it -- conv0_0
from the image, the skip-concat convs from concatenate([skip, upL_t]), the logits from the stored up0_1 with bias and no ReLU.  A batch is window i =
distinct[i % 3] (window_batch: a phantom window and two noise windows independent from frame to frame); every further window of every map and of
logits, prob and pred is bit-identical to its copy and holds no NaN; no guard is damaged; prob is within PROB_ATOL (1e-6, as
tests/test_head_launches_gpu.py) of a float64 softmax of the engine's own logits; pred == argmax(prob) exactly; the plan that ran is the host
planner's.  Weights come from seeds 1234 and 7 in turn.
Bound, as in tests/test_fp32_launches_gpu.py: max |engine - float64| <= 1e-5 x the layer's largest activation, for every launch.

    case  architecture  windows  T   H   W  weights  one-window input
       0  fc1c4               1  1  16  16     1234  phantom
       1  fc3c2               5  3  16  16        7  -
       2  wide                1  9  16  16     1234  normal
       3  default             2  9  16  16        7  -
       4  fc3c2               1  3  48  48     1234  uniform
       5  fc1c4               5  1  48  48        7  -
       6  fc3c2               1  3  32  48     1234  phantom
       7  fc1c4               5  1  32  48        7  -
       8  wide                5  9  16  16     1234  -
       9  default             1  9  32  48        7  phantom
      10  wide                1  9  16  48     1234  uniform
      11  default             1  9  48  48        7  normal

THE FIRST LAYER PAST ONE GRID PASS (test_first_layer_past_one_grid_pass): launch_conv3d_first starts at most 256 * 64 workgroups of 256 threads and
conv3d_first_kernel walks on by gridDim.x * 256.  One run_seq of 8 windows x 9 x 256 x 256 = 4 718 592 pixels is 1.125 passes, the last one partial.
conv0_0 of windows 0..2 is graded in float64; conv0_0, the last decoder map and the outputs of windows 3..7 are copies, and windows 0..2 are
bit-identical to a 3-window run_seq (one pass; a conv3d_kernel item does not depend on N) on the same handle.

THE CINE PAST ONE PASS, BOTH LOOPS, THROUGH THE FRAME TABLE (test_cine_past_one_pass_of_both_loops): run_cine of 17 frames x 256 x 256, time_step 1:
F H W = 1 114 112 > 256 * 16 * 256, so t3d_tile_kernel wraps in every chunk; with the default chunking (10 windows: 5 898 240 pixels, then 7) the first layer
wraps while it reads through the window -> frame table.  Once so and once under UKBB_TEMPORAL_CHUNK_WINDOWS=5 (chunks of 5, 5, 5 and 2), bit for bit
against tests/temporal_unet_ref.py deploy_tiling driven by single-window run_seq calls.  Two small cines (12 frames x 32 x 32, time_step 10: frames no
window reaches) on the 2- and 4-class architectures, the same comparison (t3d_tile_kernel<2> and <4>, windows of 3 frames and of 1).

Both caps are read from the launchers' source and asserted (launch_grading.grid_caps_3d), and the cases print the pass counts they asserted.

Measured on an MI355X (profiles/temporal_launches.txt, one row per launch): 5e-8 .. 4.2e-7 of the layer's scale over the 12 cases and the full-size
first layer, prob within 1.5e-7 of the float64 softmax, no copy differing, both cines bit-identical to the deploy loop.  Each of the 12 cases takes
0.2 - 0.3 s (0.1 s of forward and read-back, up to 0.1 s of float64); the first-layer case 2 s (0.7 s of forwards and read-back, 1.2 s of float64);
the 17 single-window forwards of the cine 0.2 s, each of its two chunkings 0.1 s, each small cine 0.1 s."""
import dataclasses
import time

import numpy as np
import pytest

import temporal_unet_ref as R
from launch_grading import (POISON, SEEDS, assert_plan_ran, check_copies, conv3d_launch, grid_caps_3d, guarded_engine, launches, layer3d, rel_err,
                            window_batch)
from oracle import fcn_oracle as O

pytestmark = pytest.mark.gpu
BOUND = 1e-5
PROB_ATOL = 1e-6                        # tests/test_head_launches_gpu.py

WIDE = dict(n_filter=(16, 32, 96, 160, 96), n_block=(2, 2, 3, 2, 2))
ARCH_CHANGES = {'default': {}, 'fc3c2': dict(fc=3, n_class=2), 'fc1c4': dict(fc=1, n_class=4), 'wide': WIDE}

CASES = [
    ('fc1c4', 1, 16, 16), ('fc3c2', 5, 16, 16), ('wide', 1, 16, 16), ('default', 2, 16, 16), ('fc3c2', 1, 48, 48), ('fc1c4', 5, 48, 48),
    ('fc3c2', 1, 32, 48), ('fc1c4', 5, 32, 48), ('wide', 5, 16, 16), ('default', 1, 32, 48), ('wide', 1, 16, 48), ('default', 1, 48, 48),
]
FULL_SEQ = (8, 256, 256)                # windows, H, W of the first-layer case
FULL_CINE = (17, 256, 256)              # frames, H, W of the cine case
SMALL_CINES = [('fc3c2', 12, 32, 32, 10), ('fc1c4', 12, 32, 32, 10)]       # architecture, frames, H, W, time_step


def arch_of(key):
    from ukbb_cardiac_amd.arch import MODELS
    return dataclasses.replace(MODELS['Temporal-UNet_ao'], **ARCH_CHANGES[key])


def softmax64(logits):
    return O.softmax(np.asarray(logits, np.float64))


def check_outputs(tag, out, nd):
    """prob against the float64 softmax of the engine's own logits, pred == argmax(prob), every window a copy.  Returns the prob figure."""
    for k in ('logits', 'prob', 'pred'):
        check_copies('%s %s' % (tag, k), out[k], nd)
    d = float(np.abs(out['prob'].astype(np.float64) - softmax64(out['logits'])).max())
    print('%s prob    max |engine - float64 softmax of its logits| %.2e' % (tag, d))
    assert d <= PROB_ATOL, (tag, d)
    assert out['pred'].dtype == np.int32 and np.array_equal(out['pred'], np.argmax(out['prob'], axis=-1).astype(np.int32)), tag + ': pred != argmax(prob)'
    return d


@pytest.mark.parametrize('index', range(len(CASES)), ids=['%s-%dx%dx%d' % c for c in CASES])
def test_each_3d_launch_against_float64_on_its_own_input(index, monkeypatch):
    from ukbb_cardiac_amd import engine
    from ukbb_cardiac_amd.weights import synthetic_params
    key, N, H, W = CASES[index]
    seed = SEEDS[index % 2]
    arch = arch_of(key)
    T = arch.fc
    params = synthetic_params(arch, seed)
    x, nd = window_batch(index, N, T, H, W)
    plan = engine.plan_layout(arch, 'fp32', N * T, H, W)
    graph = launches(arch)
    tag = 'temporal-launch %-7s %dx%dx%2dx%2d seed %4d' % (key, N, T, H, W, seed)
    t0 = time.perf_counter()
    with guarded_engine(monkeypatch, arch, params, 'fp32') as eng:
        eng.reserve(N * T, H, W)
        eng.poison(POISON)
        out = eng.run_seq(x, want_logits=True)
        assert_plan_ran(eng, plan)                                       # the plan tests/test_temporal_launch_coverage.py counted for this case
        stored = {'logits': out['logits']}
        for lname, sname, l, _, _, _, _ in graph:
            if lname != 'logits':
                stored[sname] = eng.activation(sname).reshape(N, T, H >> l, W >> l, -1)
        damaged, where = eng.check_guards()
        assert damaged == 0, where
    t_gpu = time.perf_counter() - t0
    assert [o['kind'] for o in plan['ops']] == ['first3d'] + ['tconv3d' if g[5] else 'conv3d' for g in graph[1:-1]] + ['logits']
    assert out['logits'].shape == (N, T, H, W, arch.n_class) and out['prob'].shape == out['logits'].shape and out['pred'].shape == (N, T, H, W)
    for sname, a in stored.items():
        check_copies('%s %s' % (tag, sname), a, nd)
    check_outputs(tag, out, nd)
    t0 = time.perf_counter()
    op_of = {o['name']: o for o in plan['ops']}
    rows = []
    for lname, sname, l, srcs, stride, transposed, relu in graph:
        xin = x[:nd] if srcs == [''] else np.concatenate([stored[s][:nd] for s in srcs], axis=-1)
        ex = layer3d(xin, params[lname], stride, transposed, relu)
        err, where = rel_err(stored[sname][:nd], ex)
        o = op_of[lname]
        if o['kind'] in ('conv3d', 'tconv3d'):
            d = conv3d_launch(o, plan['acts'], N * T, T)
            what = '%-10s CB %d x %d groups  %-29s items %% 4 = %d' % (d['kind'], d['cb'], d['cgroups'], d['fit'], d['idle'])
        else:
            what = o['kind']
        rows.append((lname, what, err, where))
    t_ref = time.perf_counter() - t0
    for lname, what, err, where in rows:
        print('%s  %-7s %-72s err/scale %.2e  worst at %s' % (tag, lname, what, err, where))
    print('%s forward + read-back %.2f s, float64 reference %.2f s' % (tag, t_gpu, t_ref))
    bad = [r for r in rows if not r[2] <= BOUND]
    assert not bad, 'launches over %g of their layer\'s scale (layer, situation, error, worst element [window, frame, y, x, channel]): %s' % (BOUND, bad)


def test_first_layer_past_one_grid_pass(monkeypatch):
    from ukbb_cardiac_amd.weights import synthetic_params
    N, H, W = FULL_SEQ
    arch = arch_of('default')
    T = arch.fc
    cap, _ = grid_caps_3d()
    pixels = N * T * H * W
    assert pixels > cap and pixels % cap and 3 * T * H * W <= cap, (pixels, cap)        # a partial last pass; the 3-window call stays within one
    print('temporal-launch first layer: %d pixels over a cap of %d threads = %.3f passes; 3 windows %.3f' % (pixels, cap, pixels / cap, 3 * T * H * W / cap))
    params = synthetic_params(arch, SEEDS[0])
    x, nd = window_batch(0, N, T, H, W)
    names = ('conv0_0', 'up0_1')
    t0 = time.perf_counter()
    with guarded_engine(monkeypatch, arch, params, 'fp32') as eng:
        eng.reserve(N * T, H, W)
        eng.poison(POISON)
        out = eng.run_seq(x, want_logits=True)
        maps = {s: eng.activation(s).reshape(N, T, H, W, -1) for s in names}
        damaged, where = eng.check_guards()
        assert damaged == 0, where
        for s, a in maps.items():
            check_copies('8 windows ' + s, a, nd)
            maps[s] = a[:nd].copy()
        check_outputs('temporal-launch first layer, 8 windows', out, nd)
        out = {k: v[:nd].copy() for k, v in out.items()}
        eng.poison(POISON)
        few = eng.run_seq(x[:nd], want_logits=True)
        for s in names:
            assert np.array_equal(maps[s].view(np.uint32), eng.activation(s).reshape(nd, T, H, W, -1).view(np.uint32)), s + ': 8 windows and 3 windows differ'
        for k in ('logits', 'prob', 'pred'):
            assert np.array_equal(out[k].view(np.uint32), few[k].view(np.uint32)), k + ': 8 windows and 3 windows differ'
        damaged, where = eng.check_guards()
        assert damaged == 0, where
    t_gpu = time.perf_counter() - t0
    t0 = time.perf_counter()
    worst = 0.0
    for i in range(nd):                                                  # window by window: the float64 map of one window is 75 MB
        err, where = rel_err(maps['conv0_0'][i:i + 1], layer3d(x[i:i + 1], params['conv0_0']))
        print('temporal-launch default %dx%dx%dx%d seed %4d  conv0_0 window %d past one pass  err/scale %.2e  worst at %s' % (N, T, H, W, SEEDS[0], i, err, where))
        worst = max(worst, err)
    print('temporal-launch first layer: forward + read-back %.2f s, float64 reference %.2f s' % (t_gpu, time.perf_counter() - t0))
    assert worst <= BOUND, worst


# ---- cines ----------------------------------------------------------------------------------------------------------------------------------------
def exact_loop(eng, frames, time_step, weight_R):
    """the reference's deploy loop with this engine's single-window run_seq standing for sess.run (tests/test_temporal_unet_gpu.py _exact_loop)"""
    return R.deploy_tiling(frames, lambda w: eng.run_seq(w)['prob'], time_step, weight_R=weight_R)


def assert_cine(prob, pred, exact):
    np.testing.assert_array_equal(prob, exact)                           # NaNs (frames no window reaches) compare equal here
    np.testing.assert_array_equal(pred, np.argmax(exact, -1).astype(np.int32))


@pytest.fixture(scope='module')
def full_cine():
    """(engine, frames, the deploy loop's prob) of the 17-frame cine: 17 single-window forwards, shared by the two chunkings."""
    from ukbb_cardiac_amd.engine import Engine
    from ukbb_cardiac_amd.weights import synthetic_params
    F, H, W = FULL_CINE
    arch = arch_of('default')
    frames = np.random.default_rng(17).standard_normal((F, H, W)).astype(np.float32)    # independent from frame to frame
    with Engine(arch, synthetic_params(arch, SEEDS[1])) as eng:
        yield arch, eng, frames, exact_loop(eng, frames, 1, 5)


@pytest.mark.parametrize('chunk', [None, 5], ids=['default-chunks', 'chunks-of-5'])
def test_cine_past_one_pass_of_both_loops(full_cine, chunk, monkeypatch):
    from ukbb_cardiac_amd import engine
    arch, eng, frames, exact = full_cine
    F, H, W = FULL_CINE
    T = arch.fc
    first_cap, tile_cap = grid_caps_3d()
    monkeypatch.delenv('UKBB_TEMPORAL_CHUNK_WINDOWS', raising=False)
    planned = engine.cine_chunk_windows(arch, 'fp32', F, H, W, 1)         # the planner's host query: windows per chunk without a budget
    assert F * H * W > tile_cap, (F * H * W, tile_cap)
    assert planned * T * H * W > first_cap and planned < F, (planned, first_cap)        # the default chunking wraps the first layer, in two unequal chunks
    if chunk is not None:
        monkeypatch.setenv('UKBB_TEMPORAL_CHUNK_WINDOWS', str(chunk))
        assert F % chunk and F > 2 * chunk                               # the first and the last chunk differ
    cw = chunk or planned
    print('temporal-launch cine %dx%dx%d in chunks of %d windows: tiling %d pixels over a cap of %d threads = %.3f passes; first layer %d pixels per chunk '
          'over %d = %.3f passes' % (F, H, W, cw, F * H * W, tile_cap, F * H * W / tile_cap, cw * T * H * W, first_cap, cw * T * H * W / first_cap))
    prob, pred = eng.run_cine(frames, time_step=1)
    assert not np.isnan(prob).any()
    assert_cine(prob, pred, exact)


@pytest.mark.parametrize('index', range(len(SMALL_CINES)), ids=['%s-%dx%dx%d-step%d' % c for c in SMALL_CINES])
def test_small_cines_of_the_2_and_4_class_architectures(index, monkeypatch):
    from ukbb_cardiac_amd.engine import Engine
    from ukbb_cardiac_amd.weights import synthetic_params
    key, F, H, W, time_step = SMALL_CINES[index]
    arch = arch_of(key)
    weight_R = (arch.fc + 1) // 2
    monkeypatch.delenv('UKBB_TEMPORAL_CHUNK_WINDOWS', raising=False)
    frames = np.random.default_rng(F + index).standard_normal((F, H, W)).astype(np.float32)
    with Engine(arch, synthetic_params(arch, SEEDS[index % 2])) as eng:
        prob, pred = eng.run_cine(frames, weight_R=weight_R, time_step=time_step)
        exact = exact_loop(eng, frames, time_step, weight_R)
    assert prob.shape == (F, H, W, arch.n_class)
    reached = ~np.isnan(exact).any(axis=(1, 2, 3))
    assert reached.any() and not reached.all() and (pred[~reached] == 0).all()          # time_step 10 leaves frames no window reaches: NaN, label 0
    assert_cine(prob, pred, exact)
    assert len(np.unique(pred[reached])) > 1
