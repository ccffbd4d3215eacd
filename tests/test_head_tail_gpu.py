"""The FCN head's deferred logits tail (kernels_head.hip, fcn_head_pc_kernel, r11) against the in-stage tail it replaced
(UKBB_HEAD_INLINE_TAIL=1).

The deferred form moves instructions: a block's second half of the logits product, the exchange between the lane halves, the
soft-max / arg-max and the stores issue between the MFMAs of the next block.  Every sum keeps its order, so `logits`, `prob` and
`pred` must be bit-identical between the two forms; no tolerance applies.  The knob is latched at the head's first launch, so each
form runs in a child process of its own.  Cases: the headline 192 x 208 at N = 1 (156 tiles on 256 CUs: workgroups with exactly one
tile, i.e. two stages and the flush after the loop), 10 and 64; 176 x 208 with two classes; 208 x 256; three and six classes at
80 x 112; each with only `pred` requested (the call shape of bench.py) and with all three outputs.  Every case also runs with the
last layer scaled to 1e-7, which puts part of the pixels on the near-tie path of softmax_argmax (kernels.h): the test asserts that
some but not all pixels have a top-two logit gap below 4e-7, so both paths ran.  The f32x3 instance keeps the in-stage tail and is
not a case."""
import copy

import numpy as np
import pytest

from launch_grading import run_in_child

pytestmark = pytest.mark.gpu
CASES = [('FCN_sa', 192, 208, 1), ('FCN_sa', 192, 208, 10), ('FCN_sa', 192, 208, 64), ('FCN_la_2ch', 176, 208, 10),
         ('FCN_sa', 208, 256, 10), ('FCN_la_4ch', 80, 112, 3), ('FCN_la_4ch_seg4', 80, 112, 3)]
SCALES = (1.0, 1e-7)
NEAR_TIE_GAP = 4e-7


def key(model, H, W, n, scale):
    return '%s_%dx%d_n%d_%s' % (model, H, W, n, 'full' if scale == 1.0 else 'neartie')


def run_cases(path):
    """Outputs of every case with the tail this process latched, saved to one .npz."""
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.engine import Engine
    from ukbb_cardiac_amd.phantom import cine_phantom
    from ukbb_cardiac_amd.weights import synthetic_params
    out = {}
    for model in sorted({c[0] for c in CASES}):
        arch = MODELS[model]
        for scale in SCALES:
            params = copy.deepcopy(synthetic_params(arch, 1234))
            if scale != 1.0:
                params['logits']['kernel'] = (params['logits']['kernel'] * scale).astype(np.float32)
                params['logits']['bias'] = (params['logits']['bias'] * scale).astype(np.float32)
            with Engine(arch, params) as eng:
                for m, H, W, n in CASES:
                    if m != model:
                        continue
                    img = cine_phantom(n, H, W, seed=H + W + n)
                    k = key(model, H, W, n, scale)
                    only = eng.run(img, want_logits=False, want_prob=False, want_pred=True)     # the pred-only path of the bench
                    full = eng.run(img, want_logits=True, want_prob=True, want_pred=True)
                    out[k + '/pred_only'] = only['pred']
                    for name in ('logits', 'prob', 'pred'):
                        out[k + '/' + name] = full[name]
    from ukbb_cardiac_amd import _lib
    out['tail_form'] = np.int32(_lib.lib.ukbb_fcn_head_tail_form())      # what the last head launch ran: 0 deferred, 1 in-stage
    np.savez(path, **out)


@pytest.fixture(scope='module')
def outputs(tmp_path_factory):
    res = {}
    for tag, knob in (('deferred', None), ('inline', '1')):
        path = str(tmp_path_factory.mktemp('head_tail') / (tag + '.npz'))
        r = run_in_child('test_head_tail_gpu', 'run_cases', [path], {'UKBB_HEAD_INLINE_TAIL': knob} if knob else {}, timeout=900)
        assert r.returncode == 0, r.stdout[-3000:]
        with np.load(path) as z:
            res[tag] = {k: z[k] for k in z.files}
    # the two children really ran different kernels (a knob that was misspelt or not read would make every comparison pass)
    assert int(res['deferred']['tail_form']) == 0 and int(res['inline']['tail_form']) == 1, (res['deferred']['tail_form'], res['inline']['tail_form'])
    return res


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


@pytest.mark.parametrize('scale', SCALES, ids=('full', 'neartie'))
@pytest.mark.parametrize('model,H,W,n', CASES)
def test_deferred_tail_is_bit_identical_to_the_inline_tail(outputs, model, H, W, n, scale):
    k = key(model, H, W, n, scale)
    new, old = outputs['deferred'], outputs['inline']
    for name in ('logits', 'prob', 'pred', 'pred_only'):
        a, b = new[k + '/' + name], old[k + '/' + name]
        differ = int((bits(a) != bits(b)).sum())
        print('%s %s: %d of %d words differ between the deferred and the in-stage tail' % (k, name, differ, a.size))
        assert a.shape == b.shape and a.dtype == b.dtype and differ == 0, (k, name, differ)
    assert np.array_equal(new[k + '/pred_only'], new[k + '/pred'])      # one label map whichever outputs were requested
    srt = np.sort(new[k + '/logits'], axis=-1)
    near = (srt[..., -1] - srt[..., -2]) < NEAR_TIE_GAP
    print('%s: %d of %d pixels have a top-two logit gap below %g' % (k, int(near.sum()), near.size, NEAR_TIE_GAP))
    if scale != 1.0:
        assert near.any() and not near.all(), (int(near.sum()), near.size)      # both paths of softmax_argmax ran


def test_outputs_are_not_trivial(outputs):
    """The comparison above means something only if the head wrote every pixel: more than one label occurs in each full-scale case."""
    for model, H, W, n in CASES:
        pred = outputs['deferred'][key(model, H, W, n, 1.0) + '/pred']
        assert pred.shape == (n, H, W) and len(np.unique(pred)) > 1, (model, H, W, n)
