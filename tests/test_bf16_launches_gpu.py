"""Every launch of the bf16 aortic U-Net (--precision bf16), one launch at a time, against float64 on the engine's OWN stored input, at the batches where
its persistent "walker" kernels take several rounds.

tests/test_bf16_layers_gpu.py grades three shapes this way, (1, 256, 256), (3, 64, 96) and (2, 48, 16): 46 of the 61 (layer, tiling) combinations of
the recorded default plans, and the weight-stationary walkers of kernels_ws.hip only with exactly one tile per wave.  This file grades every
combination, and every weight-stationary launch of the benchmark's batches in the round classes those batches put it in: several rounds with a ragged
last one, the round in which only some waves take a second tile, XCD-local and wave-major tile order, ragged 32-column tiles, both workgroup
placements; the fused stem and tail below, between and above one and two rounds, the tail's strip segments whole and ragged.
tests/test_bf16_launch_coverage.py computes all of that on the CPU from the host planner and the launchers' constants, shows that CASES reaches it
with no case idle, and that the grade and the copy identity used here tell a planted defect.

The method is the graders' common one (tests/launch_grading.py), on a guarded, poisoned engine: one forward per case on a fresh engine created
under UKBB_DEBUG_GUARD and poisoned again by Engine.poison() in front of the forward, so a tile no walker wrote holds NaN, not a leftover; the plan
that ran must be the plan the CPU test counted (engine.plan_layout on 256 compute units); inputs are normalised_copies.  The worker of tile t differs
between the copies of an image, so a dropped, duplicated or misdirected tile breaks either the grade of slices 0..2 or the identity of a later slice
with them.
  * slices 0..2 of every stored map are graded in float64 from the engine's stored input map(s) of that launch with the bf16-rounded folded kernel
    (layer(round_w=True) and grade of tests/launch_grading.py): grade(ulps = 0.5, fraction = 1.0) -- half a bf16 ulp + 2^-18 |exact| +
    2^-20 scale, for EVERY element;
  * the fused stem (image -> conv0_0 -> conv0_1) and the fused tail (up0_0 -> up0_1 -> logits, argmax) are graded as units with their intermediate
    rounding and the figures of tests/test_bf16_layers_gpu.py: 4 ulps for every element and half an ulp for 99.5 % (stem); logits within 2e-2 of their scale, 99 % within 2e-4,
    label flips only next to a tie (tail).  The stem's un-stored conv0_0 value may legitimately round either way where it lies within fp32 error of
    a rounding boundary; on these rough inputs that moves an output the other taps cancel by more than 4 of ITS ulps (measured: 2 elements of 3.1 M
    at 17 x 256 x 256 on the MI355X at 5.4 ulps, and a float32 numpy evaluation of the same arithmetic shows the same), so exactly those outputs get
    the movement such a value can cause added to their bound (stem_reference);  The stem's form -- the fused stem kernel, or an fp32 first layer inside conv0_1's staging -- is taken from
    the plan op's kind;
  * every other slice of every stored map and of the logits and labels must be bit-identical to the graded copy of its image;
  * every stored map holds bf16 values only, and no NaN.
One activation is fetched at a time and only slices 0..2 are kept after the identity check (the largest case's maps are 1.5 GB as float32).

SEQ_CASES: the bf16 U-Net of UNet-LSTM_ao stores up0_0 and up0_1 (its tail is the ConvLSTM): up0_0 on 401 with its 16 output channels zero-padded to
the 32-row MFMA and up0_1 on the tile-per-workgroup 236, on whole and on ragged 32-column tiles, and the pair the small-map plans take instead
(232 / 232), each graded from the stored conv0 / up0_t / up0_0 of a run_seq call.

    case   N    H    W    pixels   what only it reaches (tests/test_bf16_launch_coverage.py prints the full table)
       0   1   32   48      1536   conv1_1 / up1_* on 232, conv2_0 on 241, conv2_1 / up2_* on 234, up1_t on 253
       1   1   48   32      1536   conv2_1 / up2_* on 230, up0_t on 253
       2   1   16  112      1792   up2_t on 257; 401 and 410 below one round on a grid that is no multiple of 8 nG
       3   1  112   16      1792   conv2_1 .. up3_1 on 232
       4   1   48   80      3840   conv3_0 on 241, up2_t on 253
       5 129   16  208    429312   401 / 410 wave-major between one and two rounds; tail between, one segment per strip
       6   9  256  256    589824   401 / 410 XCD-local between one and two rounds; stem between
       7  17  256  256   1114112   401 / 410 XCD-local two rounds and a ragged third; up1_t 411 and up2_0 400 between
       8 103   80  208   1713920   400 / 402 / 411 of levels 2-3 between one and two rounds; conv3_0 on 240
       9 128  128  208   3407872   400 / 401 / 402 / 410 / 411 at an exact multiple of their workers
      10 114  144  208   3414528   400 / 402 / 411 of levels 2-3 in two+ rounds with a ragged last one; 422 between; conv4_0 240, conv4_1 230, up3_t 250
    all                 10680064   float64 on min(N, 3) x H x W = 633344 pixels

Measured on an MI355X: profiles/bf16_launches.txt (one row per launch: case, layer, tiling, round class, share of elements within the half-ulp
grade, worst deviation over the bound; per case the seconds of forward + read-back + identity and of float64)."""
import time

import numpy as np
import pytest

from launch_grading import (CUS, POISON, SEEDS, Report, assert_plan_ran, bf16_round, check_copies, fetcher, fold, grade, guarded_engine, half_ulp, launch_class,
                            launches, layer, normalised_copies, tolerance)
from oracle import fcn_oracle as O

pytestmark = pytest.mark.gpu

CASES = [(1, 32, 48), (1, 48, 32), (1, 16, 112), (1, 112, 16), (1, 48, 80), (129, 16, 208), (9, 256, 256), (17, 256, 256), (103, 80, 208),
         (128, 128, 208), (114, 144, 208)]
# (sequences, H, W, tiling of up0_0, tiling of up0_1): T = 9 frames each
SEQ_CASES = [(1, 16, 48, 232, 232), (2, 32, 64, 401, 236), (1, 48, 80, 401, 236)]


def stem_reference(img, params, kind):
    """The fused first two layers as a unit: (exact conv0_1 output in float64 from the bf16-rounded conv0_0 output, slack, ambiguous intermediates).

    kind 'stem' (kernels_stem.hip): image -> bf16, conv0_0 with the bf16 kernel -> bf16; kind 'conv': conv0_0 in fp32 on the un-rounded image inside
    conv0_1's staging (conv_mfma_kernel<..., FUSE = 1>) -> bf16.  conv0_0's output is never stored, so where its float64 value lies within the
    worst-case error of an fp32 sum of its K = 10 terms (nine taps and the bias: K 2^-24 (sum |x||w| + |b|)) of a bf16 rounding boundary, a correct
    kernel may hold either neighbour -- a float32 numpy evaluation does, once to three times in 3 x 256 x 256 values -- and the outputs it feeds move by
    up to (one bf16 ulp of that value) x |w|, many ulps of an output the other taps cancel.  slack is exactly that: sum over the ambiguous values of
    ulp x |w| of the tap that reads them; it is zero everywhere else.  About one conv0_0 value in 600 is ambiguous by this worst-case figure and each
    feeds 9 x 16 outputs, so about one output in six carries a slack, of the size of a few of its own ulps; the half-ulp share asked of the unit
    (99.5 %) is not touched by it."""
    w0, b0 = fold(params['conv0_0'])
    x = img.astype(np.float64)
    if kind == 'stem':
        x, w0 = bf16_round(img).astype(np.float64), bf16_round(w0)
    w0 = w0.astype(np.float64)
    pre = np.maximum(O.conv2d_same(x, w0, 1) + b0.astype(np.float64), 0.0)
    mag = O.conv2d_same(np.abs(x), np.abs(w0), 1) + np.abs(b0).astype(np.float64)
    ulp = 2 * half_ulp(pre)
    q = pre / ulp
    amb = (np.abs(q - np.floor(q) - 0.5) * ulp <= 10 * 2.0 ** -24 * mag) & (pre > 0)
    w1 = bf16_round(fold(params['conv0_1'])[0]).astype(np.float64)
    slack = O.conv2d_same(np.where(amb, ulp, 0.0), np.abs(w1), 1)
    ex = layer(bf16_round(pre.astype(np.float32)), params['conv0_1'], round_w=True)
    return ex, slack, int(amb.sum())


def grade_stem(got, ex, sc, slack):
    """The figures of tests/test_bf16_layers_gpu.py for the stem: every element within 4 bf16 ulps (+ slack where an ambiguous conv0_0 value feeds it),
    99.5 % within half an ulp."""
    got = np.asarray(got, np.float64).reshape(ex.shape)
    tol = tolerance(ex, sc, 4.0) + slack
    bad = np.abs(got - ex) > tol
    assert not bad.any(), 'conv0_0+conv0_1: %d elements further than 4 bf16 ulps from the specified result, worst %.3g x the bound at slice, y, x, channel %s' % (
        int(bad.sum()), float((np.abs(got - ex) / tol).max()), np.unravel_index(int((np.abs(got - ex) / tol).argmax()), ex.shape))
    grade('conv0_0+conv0_1 (half ulp)', got, ex, sc, ulps=0.5, fraction=0.995)


def grade_unet(arch, params, ops, img, fetch, logits, pred, report):
    """Every launch of a UNet_ao bf16 plan on the graded slices.  img [nd, H, W, 1]; fetch(stored name) -> [nd, h, w, c] float32 (bf16 values);
    logits [nd, H, W, classes], pred [nd, H, W]."""
    first = [o for o in ops if 'conv0_0' in o['name'].split('+')]
    assert len(first) == 1 and first[0]['name'] == 'conv0_0+conv0_1' and first[0]['kind'] in ('stem', 'conv'), first
    tails = [o for o in ops if o['kind'] == 'tail']
    assert len(tails) == 1 and tails[0]['name'] == 'up0_0+up0_1+logits', [o['name'] for o in ops]
    for lname, sname, l, srcs, stride, transposed, relu in launches(arch):
        if lname in ('conv0_0', 'up0_0', 'up0_1', 'logits'):
            continue
        if lname == 'conv0_1':
            ex, slack, n_amb = stem_reference(img, params, first[0]['kind'])
            sc = float(np.abs(ex).max())
            got = fetch(sname)
            report.row(lname, got, ex, sc)
            print('bf16-launch %-22s stem: %d of %d conv0_0 values within fp32 error of a rounding boundary; they reach %d of %d outputs' % (
                report.tag, n_amb, ex.size, int((slack > 0).sum()), ex.size))
            grade_stem(got, ex, sc, slack)
            continue
        x = np.concatenate([fetch(s) for s in srcs], axis=-1)
        ex = layer(x, params[lname], stride, transposed, relu, round_w=True)
        sc = float(np.abs(ex).max())
        got = fetch(sname)
        report.row(lname, got, ex, sc)
        grade('%s (tiling %d)' % (lname, report.op_of[lname]['cfg']), got, ex, sc, ulps=0.5, fraction=1.0)
    ex = tail_reference(np.concatenate([fetch('conv0'), fetch('up0_t')], axis=-1), params)
    lsc = float(np.abs(ex).max())
    err = np.abs(logits.astype(np.float64) - ex)
    r = (report.tag, tails[0]['name'], -1, launch_class(tails[0], report.acts, report.n), float(np.mean(err <= 2e-4 * lsc)), float(err.max() / (2e-2 * lsc)))
    report.rows.append(r)
    print('bf16-launch %-22s %-18s tiling %3d  %-18s logits within 2e-4   %.6f  worst / bound %.3f' % r)
    grade_tail(logits, pred, ex)


def tail_reference(a, params):
    """The fused tail as a unit, float64 logits: up0_0 -> bf16 -> up0_1 -> bf16 -> logits (fp32 kernel; the engine enters it as bf16 hi + lo)."""
    for nm in ('up0_0', 'up0_1'):
        a = bf16_round(layer(a, params[nm], round_w=True).astype(np.float32))
    pl = params['logits']
    return O.conv2d_same(a.astype(np.float64), pl['kernel'].astype(np.float64), 1) + pl['bias'].astype(np.float64)


def grade_tail(logits, pred, ex):
    """The figures of tests/test_bf16_layers_gpu.py: a flipped rounding of one up0_0 / up0_1 value moves a logit by (one bf16 ulp of that value) x a few
    weights, a few 1e-3 of the scale at worst; labels differ from the float64 argmax only next to a tie."""
    lsc = float(np.abs(ex).max())
    err = np.abs(logits.astype(np.float64) - ex)
    assert err.max() <= 2e-2 * lsc and np.mean(err <= 2e-4 * lsc) >= 0.99, (float(err.max() / lsc), float(np.mean(err <= 2e-4 * lsc)))
    flips = pred != np.argmax(ex, -1)
    assert np.all(O.top2_margin(ex)[flips] <= 4e-2 * lsc) and flips.mean() < 2e-3, (int(flips.sum()), float(flips.mean()))


def grade_up0(params, fetch, report):
    """up0_0 and up0_1 of the UNet-LSTM's U-Net, each from the stored map(s) in front of it."""
    x = np.concatenate([fetch('conv0'), fetch('up0_t')], axis=-1)          # skip first (network_ao.py:51)
    for lname, sname in (('up0_0', 'up0_0'), ('up0_1', 'up0')):
        ex = layer(x, params[lname], round_w=True)
        sc = float(np.abs(ex).max())
        got = fetch(sname)
        report.row(lname, got, ex, sc)
        grade('%s (tiling %d)' % (lname, report.op_of[lname]['cfg']), got, ex, sc, ulps=0.5, fraction=1.0)
        x = got


@pytest.mark.parametrize('index', range(len(CASES)), ids=['%dx%dx%d' % c for c in CASES])
def test_each_bf16_launch_against_its_specified_arithmetic(index, monkeypatch):
    from ukbb_cardiac_amd import engine
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.weights import synthetic_params
    n, H, W = CASES[index]
    arch = MODELS['UNet_ao']
    params = synthetic_params(arch, SEEDS[index % 2])
    img, nd = normalised_copies(index, n, H, W)
    plan = engine.plan_layout(arch, 'bf16', n, H, W, CUS)
    ops = plan['ops']
    tag = 'UNet_ao %dx%dx%d' % (n, H, W)
    t0 = time.perf_counter()
    cache = {}
    with guarded_engine(monkeypatch, arch, params, 'bf16') as eng:
        eng.reserve(n, H, W)
        eng.poison(POISON)
        out = eng.run(img, want_logits=True, want_prob=False)
        t_fwd = time.perf_counter() - t0
        assert_plan_ran(eng, plan)                                    # the plan tests/test_bf16_launch_coverage.py counted for this case
        level = {g[1]: g[2] for g in launches(arch)}
        fetch = fetcher(eng, lambda s: (n, H >> level[s], W >> level[s], -1), nd, cache, tag)
        for g in launches(arch):                                  # every stored map read back and checked once, in graph order
            if g[0] not in ('conv0_0', 'up0_0', 'up0_1', 'logits'):
                fetch(g[1])
        damaged, where = eng.check_guards()
        assert damaged == 0, where
    assert out['logits'].shape == (n, H, W, arch.n_class)
    check_copies('logits', out['logits'], nd, tag)
    check_copies('pred', out['pred'], nd, tag)
    t_gpu = time.perf_counter() - t0
    t0 = time.perf_counter()
    report = Report(tag, ops, plan['acts'], n)
    try:
        grade_unet(arch, params, ops, img[:nd], fetch, out['logits'][:nd], out['pred'][:nd], report)
    finally:
        print('bf16-launch %-22s forward %.2f s, + read-back and identity %.2f s, float64 %.2f s' % (tag, t_fwd, t_gpu, time.perf_counter() - t0))


@pytest.mark.parametrize('index', range(len(SEQ_CASES)), ids=['%dx9x%dx%d-%d-%d' % c for c in SEQ_CASES])
def test_up0_launches_of_the_unet_lstm(index, monkeypatch):
    from ukbb_cardiac_amd import engine
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.weights import synthetic_params
    N, H, W, cfg0, cfg1 = SEQ_CASES[index]
    arch = MODELS['UNet-LSTM_ao']
    T = arch.fc
    params = synthetic_params(arch, SEEDS[index % 2])
    img, nd = normalised_copies(index, N * T, H, W)
    plan = engine.plan_layout(arch, 'bf16', N * T, H, W, CUS)
    ops = plan['ops']
    assert {o['name']: o['cfg'] for o in ops if o['name'] in ('up0_0', 'up0_1')} == {'up0_0': cfg0, 'up0_1': cfg1}
    tag = 'UNet-LSTM_ao %dx%dx%dx%d' % (N, T, H, W)
    cache = {}
    t0 = time.perf_counter()
    with guarded_engine(monkeypatch, arch, params, 'bf16') as eng:
        eng.reserve(N * T, H, W)
        eng.poison(POISON)
        eng.run_seq(img.reshape(N, T, H, W, 1), want_prob=False)   # the U-Net's maps are per frame; the ConvLSTM behind them is graded in tests/test_lstm_launches_gpu.py
        assert_plan_ran(eng, plan)
        fetch = fetcher(eng, lambda s: (N * T, H, W, -1), nd, cache, tag)
        for s in ('conv0', 'up0_t', 'up0_0', 'up0'):
            fetch(s)
        damaged, where = eng.check_guards()
        assert damaged == 0, where
    t_gpu = time.perf_counter() - t0
    t0 = time.perf_counter()
    report = Report(tag, ops, plan['acts'], N * T)
    try:
        grade_up0(params, fetch, report)
    finally:
        print('bf16-launch %-22s forward + read-back %.2f s, float64 %.2f s' % (tag, t_gpu, time.perf_counter() - t0))
