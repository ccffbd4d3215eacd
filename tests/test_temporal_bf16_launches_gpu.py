"""Every launch of the aortic Temporal-UNet under precision 'bf16_3d' (UKBB_PREC_BF16_3D, kernels_conv3d_bf16.hip), one launch at a time, against
float64 on the engine's OWN stored input.

The method is the graders' common one (tests/launch_grading.py), as tests/test_temporal_launches_gpu.py applies it to the fp32 kernels: one run_seq
per case on an engine created under UKBB_DEBUG_GUARD and poisoned first; every stored map (conv*, up*_t, up*) and the logits read back; for windows
0..2 each launch recomputed alone in float64 from the map or maps the engine stored in front of it, in the rounding model of
tests/temporal_bf16_grading.py:

    conv0_0        launch_grading.layer3d on the fp32 image with the UNROUNDED float32 fold (the vector-ALU first layer), stored bf16
    every other    layer3d_bf16: the folded kernel rounded once to bf16, the stored bf16-valued input as it is (the skip-concat convs from
    3-D launch     concatenate([skip, upL_t])), stored bf16
    logits         launch_grading.layer3d on the stored up0_1 with bias and no ReLU, float32

Every element of a stored 3-D map must lie within half a bf16 ulp of the exact value (launch_grading.grade, ulps=0.5, fraction=1.0: the bound of the
bf16 U-Net graders) and be bf16-representable.  The logits are held within 1e-5 of their scale, prob within 1e-6 of a float64 softmax of the engine's
own logits, pred == argmax(prob) exactly (the bounds of tests/test_head_launches_gpu.py).  A batch is window i = distinct[i % 3] (window_batch); every
further window of every map and of logits, prob and pred is bit-identical to its copy and holds no NaN (the poison); no guard is damaged; the plan
that ran is the host planner's (tests/test_temporal_bf16_launch_coverage.py counts its situations).  Weights come from seeds 1234 and 7 in turn.

The cases are temporal_bf16_grading.CASES, the twelve of the fp32 grader: the new launcher keeps that launcher's item decomposition.  No kernel of
the mode walks a capped grid (the first layer starts one thread per pixel), so there is no case past a cap.

Measured on an MI355X (profiles/temporal_bf16.txt): every element of all 270 graded 3-D launches inside the bound, the worst at 0.999 of it (a
correctly rounded value lies up to half an ulp from the exact one); logits within 0.016 of their bound, prob within 1.4e-7 of the float64 softmax;
each case takes 0.2 - 0.4 s."""
import time

import numpy as np
import pytest

import temporal_bf16_grading as B
from launch_grading import POISON, SEEDS, assert_plan_ran, check_bf16, check_copies, conv3d_launch, grade, guarded_engine, launches, measure, rel_err, window_batch
from oracle import fcn_oracle as O

pytestmark = pytest.mark.gpu
LOGITS_BOUND = 1e-5                     # of the logits' scale
PROB_ATOL = 1e-6                        # tests/test_head_launches_gpu.py


def check_outputs(tag, out, nd):
    for k in ('logits', 'prob', 'pred'):
        check_copies('%s %s' % (tag, k), out[k], nd)
    d = float(np.abs(out['prob'].astype(np.float64) - O.softmax(np.asarray(out['logits'], np.float64))).max())
    print('%s prob    max |engine - float64 softmax of its logits| %.2e' % (tag, d))
    assert d <= PROB_ATOL, (tag, d)
    assert out['pred'].dtype == np.int32 and np.array_equal(out['pred'], np.argmax(out['prob'], axis=-1).astype(np.int32)), tag + ': pred != argmax(prob)'


@pytest.mark.parametrize('index', range(len(B.CASES)), ids=['%s-%dx%dx%d' % c for c in B.CASES])
def test_each_bf16_3d_launch_against_float64_on_its_own_input(index, monkeypatch):
    from ukbb_cardiac_amd import engine
    from ukbb_cardiac_amd.weights import synthetic_params
    key, N, H, W = B.CASES[index]
    seed = SEEDS[index % 2]
    arch = B.arch_of(key)
    T = arch.fc
    params = synthetic_params(arch, seed)
    x, nd = window_batch(index, N, T, H, W)
    plan = engine.plan_layout(arch, B.PRECISION, N * T, H, W)
    graph = launches(arch)
    tag = 'temporal-bf16-launch %-7s %dx%dx%2dx%2d seed %4d' % (key, N, T, H, W, seed)
    t0 = time.perf_counter()
    with guarded_engine(monkeypatch, arch, params, B.PRECISION) as eng:
        eng.reserve(N * T, H, W)
        eng.poison(POISON)
        out = eng.run_seq(x, want_logits=True)
        assert_plan_ran(eng, plan)
        stored = {'logits': out['logits']}
        for lname, sname, l, _, _, _, _ in graph:
            if lname != 'logits':
                stored[sname] = eng.activation(sname).reshape(N, T, H >> l, W >> l, -1)
        damaged, where = eng.check_guards()
        assert damaged == 0, where
    t_gpu = time.perf_counter() - t0
    assert [o['kind'] for o in plan['ops']] == ['first3d'] + ['tconv3d' if g[5] else 'conv3d' for g in graph[1:-1]] + ['logits']
    assert all(a['bytes_per_element'] == 2 for a in plan['acts'])
    assert out['logits'].shape == (N, T, H, W, arch.n_class) and out['prob'].shape == out['logits'].shape and out['pred'].shape == (N, T, H, W)
    for sname, a in stored.items():
        check_copies('%s %s' % (tag, sname), a, nd)                      # no poison left, every further window a copy
        if sname != 'logits':
            check_bf16('%s %s' % (tag, sname), a)
    check_outputs(tag, out, nd)
    t0 = time.perf_counter()
    op_of = {o['name']: o for o in plan['ops']}
    rows, exact = [], {}
    for lname, sname, l, srcs, stride, transposed, relu in graph:
        xin = x[:nd] if srcs == [''] else np.concatenate([stored[s][:nd] for s in srcs], axis=-1)
        ex = B.exact_of(lname, xin, params[lname], stride, transposed, relu)
        scale = float(np.abs(ex).max())
        exact[lname] = (sname, ex, scale)
        o = op_of[lname]
        if lname == 'logits':
            err, where = rel_err(stored[sname][:nd], ex)
            rows.append((lname, 'logits (fp32)', 1.0 if err <= LOGITS_BOUND else 0.0, err / LOGITS_BOUND))
            continue
        share, worst = measure(stored[sname][:nd], ex, scale)
        if o['kind'] in ('conv3d', 'tconv3d'):
            d = conv3d_launch(o, plan['acts'], N * T, T)
            what = '%-10s CB %d x %d groups  %-29s items %% 4 = %d' % (d['kind'], d['cb'], d['cgroups'], d['fit'], d['idle'])
        else:
            what = o['kind']
        rows.append((lname, what, share, worst))
    t_ref = time.perf_counter() - t0
    for lname, what, share, worst in rows:
        print('%s  %-7s %-72s within the bound %.6f  worst / bound %.3f' % (tag, lname, what, share, worst))
    print('%s forward + read-back %.2f s, float64 reference %.2f s' % (tag, t_gpu, t_ref))
    for lname, (sname, ex, scale) in exact.items():                    # the assertions, after every row is printed
        if lname != 'logits':
            grade('%s %s' % (tag, lname), stored[sname][:nd], ex, scale, ulps=0.5, fraction=1.0)
    bad = [r for r in rows if r[0] == 'logits' and not r[3] <= 1.0]
    assert not bad, 'logits over %g of their scale: %s' % (LOGITS_BOUND, bad)
