"""The FCN head's separable bilinear gather (kernels_head.hip, fcn_head_pc_kernel, r08) against the direct 2-D gather it replaced
(UKBB_HEAD_DIRECT_GATHER=1) and against the float64 oracle.

The knob is latched at the head's first launch, so each gather runs in a child process of its own.  Every child evaluates the same
batches: four image sizes (the headline 192 x 208, the long-axis 176 x 208, 208 x 256 and the unusual 272 x 304, whose level-4 map
is 17 x 19, so tiles on the right and bottom border read window rows and columns outside the map at every level), N = 1, 10 and 64
(the first slices of one batch of 64), fp32 and f32x3.  The separable form rounds its sums in another order, so the two gathers agree
to ordinary fp32 rounding, not bit for bit.  Within one gather the logits of a slice do not depend on the batch it is in."""
import numpy as np
import pytest

from launch_grading import run_in_child

pytestmark = pytest.mark.gpu
LOGIT_RTOL = 1e-3                       # north-star tolerance (tests/test_gpu_parity.py)
AB_RTOL = 1e-6                          # separable vs direct gather: a few fp32 roundings of out0's pre-activation
CASES = [('FCN_sa', 192, 208), ('FCN_la_2ch', 176, 208), ('FCN_sa', 208, 256), ('FCN_sa', 272, 304)]
BATCHES = (1, 10, 64)
MODES = ('fp32', 'f32x3')


def images(H, W):
    from ukbb_cardiac_amd.phantom import cine_phantom
    return cine_phantom(max(BATCHES), H, W, seed=H + W)


def run_cases(path):
    """Logits of every (mode, case, batch) with the gather this process latched, saved to one .npz."""
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.engine import Engine
    from ukbb_cardiac_amd.weights import synthetic_params
    out = {}
    for model in sorted({c[0] for c in CASES}):
        arch = MODELS[model]
        with Engine(arch, synthetic_params(arch, 1234)) as eng:
            for mode in MODES:
                eng.set_precision(mode)
                for m, H, W in CASES:
                    if m != model:
                        continue
                    img = images(H, W)
                    for n in BATCHES:
                        out['%s_%s_%dx%d_n%d' % (mode, model, H, W, n)] = eng.run(img[:n], want_logits=True)['logits']
    np.savez(path, **out)


@pytest.fixture(scope='module')
def logits(tmp_path_factory):
    res = {}
    for tag, knob in (('separable', None), ('direct', '1')):
        path = str(tmp_path_factory.mktemp('head_gather') / (tag + '.npz'))
        r = run_in_child('test_head_gather_gpu', 'run_cases', [path], {'UKBB_HEAD_DIRECT_GATHER': knob} if knob else {}, timeout=900)
        assert r.returncode == 0, r.stdout[-3000:]
        with np.load(path) as z:
            res[tag] = {k: z[k] for k in z.files}
    return res


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('model,H,W', CASES)
def test_separable_gather_against_direct(logits, mode, model, H, W):
    worst, zero = 0.0, True
    for n in BATCHES:
        k = '%s_%s_%dx%d_n%d' % (mode, model, H, W, n)
        new, old = logits['separable'][k].astype(np.float64), logits['direct'][k].astype(np.float64)
        d = float(np.abs(new - old).max()) / float(np.abs(old).max())
        print('%s %s %dx%d N=%d: separable vs direct gather, max logit difference / scale %.2g' % (mode, model, H, W, n, d))
        worst, zero = max(worst, d), zero and d == 0.0
    assert worst <= AB_RTOL, worst
    assert not zero                                     # two summation orders: the knob really switched gathers


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('model,H,W', CASES)
def test_separable_gather_is_batch_independent(logits, mode, model, H, W):
    for tag in ('separable', 'direct'):
        full = logits[tag]['%s_%s_%dx%d_n%d' % (mode, model, H, W, max(BATCHES))]
        for n in BATCHES[:-1]:
            assert np.array_equal(logits[tag]['%s_%s_%dx%d_n%d' % (mode, model, H, W, n)], full[:n]), (tag, n)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('model,H,W', CASES)
def test_separable_gather_against_float64(logits, mode, model, H, W):
    """First and last slice of the N = 10 batch against oracle/fcn_oracle.py in float64."""
    from oracle import fcn_oracle as O
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.weights import synthetic_params
    arch = MODELS[model]
    params = synthetic_params(arch, 1234)
    img = images(H, W)
    got = logits['separable']['%s_%s_%dx%d_n10' % (mode, model, H, W)]
    for i in (0, 9):
        ref = O.build_FCN(img[i:i + 1], params, arch.n_class, dtype=np.float64)[0]
        sc = float(np.abs(ref).max())
        err = float(np.abs(got[i].astype(np.float64) - ref).max()) / sc
        print('%s %s %dx%d slice %d: logits vs float64, max error / scale %.2g' % (mode, model, H, W, i, err))
        assert err <= LOGIT_RTOL, err
