"""Every launch of the UKBB_PREC_BF16 aortic U-Net plan against an INDEPENDENT emulation of what it is specified to compute (r06).

The bf16 path is defined by where it rounds (include/ukbb_fcn.h UKBB_PREC_BF16): BN folded in fp32, the folded kernel rounded to bf16
(RNE), bf16 x bf16 products accumulated in fp32, + fp32 bias, ReLU, the activation rounded to bf16 ONCE as it is stored; the fused stem rounds the image and
conv0_0's output the same way, the fused tail up0_0's and up0_1's outputs, and the logits use the fp32 logits kernel on those bf16 activations.

For every layer the engine stores, this test takes the ENGINE's own stored input map(s) -- exact bf16 values -- and evaluates that one layer in numpy
float64 with the bf16-rounded folded kernel (oracle/fcn_oracle.py conv2d_same / conv2d_transpose_same: the reference's op, reference
common/network.py:19-34, network_ao.py:31-58): the exact result of the specified arithmetic.  The engine's stored output must then be that value
rounded to bf16, up to fp32 accumulation error near a rounding boundary: |engine - exact| <= half a bf16 ulp of the exact value (+ a 2^-18 relative slack
for the fp32 accumulation, + an absolute floor for values ReLU brings next to zero).  No error is carried from layer to layer, so the bound is the same at
conv1_0 and at up1_1.  The fused stem (two layers) and tail (two layers + logits) are emulated as units with their intermediate rounding; there an
intermediate value that lands within fp32 accumulation error of ITS rounding boundary may round the other way and move the outputs it feeds by a bf16
ulp of one product, so those are graded at 4 ulps for every element and half an ulp for 99.5 % of them.

This replaces comparing the r04 kernels with the kernels they replaced (tests/test_bf16_kernels_gpu.py: regression guards) as the parity statement of
the bf16 kernels: kernels_ws.hip (conv / transposed conv walkers, the K = 2304 ring form), the bf16 tile-per-workgroup tilings, kernels_stem.hip and
kernels_tail.hip are each checked against numpy, at the tuned 256 x 256 shape and at a shape where the small-map fall-backs run.
tests/test_bf16_launches_gpu.py does the same for every (layer, tiling) combination of the default plans and at the batches where the walkers take several rounds."""
import numpy as np
import pytest

from launch_grading import bf16_round, grade, layer, tolerance
from oracle import fcn_oracle as O

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('shape,seed', [((1, 256, 256), 1234), ((3, 64, 96), 7), ((2, 48, 16), 11)])
def test_every_bf16_launch_against_its_specified_arithmetic(shape, seed):
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.engine import Engine
    from ukbb_cardiac_amd.phantom import cine_phantom
    from ukbb_cardiac_amd.weights import synthetic_params
    arch = MODELS['UNet_ao']
    params = synthetic_params(arch, seed)
    n, H, W = shape
    img = ((cine_phantom(n, H, W, seed=seed) - 0.3) / 0.25).astype(np.float32)
    with Engine(arch, params) as eng:
        eng.set_precision('bf16')
        out = eng.run(img, want_logits=True)
        names = eng.kernel_names()

        def act(name, l):
            # the last map of a level is registered under the level's name (include/ukbb_fcn.h ukbb_fcn_get_activation: "conv0".."conv4", "up3".."up0")
            kind, i = name.split('_')
            if i != 't' and int(i) == arch.n_block[l] - 1:
                name = kind
            return eng.activation(name).reshape(n, H >> l, W >> l, -1)
        stored = {}
        for l in range(5):
            for i in range(arch.n_block[l]):
                if not (l == 0 and i == 0):
                    stored['conv%d_%d' % (l, i)] = act('conv%d_%d' % (l, i), l)
        for l in (3, 2, 1, 0):
            stored['up%d_t' % l] = act('up%d_t' % l, l)
            for i in range(arch.n_block[l]):
                try:
                    stored['up%d_%d' % (l, i)] = act('up%d_%d' % (l, i), l)
                except Exception:                                        # up0_0 / up0_1 inside the fused tail: never stored
                    assert l == 0, (l, i)
    if shape[1] >= 64:
        assert any('+' in k for k in names), 'the fused stem / tail are expected in this plan: %s' % names
    for k, v in stored.items():                                          # what is stored really is bf16
        assert np.array_equal(v, bf16_round(v)), k
    report = {}
    # ---- stem: image -> bf16; conv0_0 -> bf16; conv0_1 -> bf16 (kernels_stem.hip, or the fused-first tile kernel on small maps: fp32 first layer) ----
    a00 = bf16_round(layer(bf16_round(img), params['conv0_0'], round_w=True).astype(np.float32))
    ex = layer(a00, params['conv0_1'], round_w=True)
    sc = float(np.abs(ex).max())
    try:
        report['stem'] = grade('conv0_0+conv0_1', stored['conv0_1'], ex, sc, ulps=4.0)
        grade('conv0_0+conv0_1 (half ulp)', stored['conv0_1'], ex, sc, ulps=0.5, fraction=0.995)
    except AssertionError:
        # small maps: conv0_0 evaluated in fp32 on the un-rounded image inside conv0_1's staging (conv_mfma_kernel<..., FUSE = 1>)
        a00 = bf16_round(layer(img, params['conv0_0']).astype(np.float32))
        ex = layer(a00, params['conv0_1'], round_w=True)
        report['stem(fp32 first layer)'] = grade('conv0_0+conv0_1', stored['conv0_1'], ex, sc, ulps=4.0)
        grade('conv0_0+conv0_1 (half ulp)', stored['conv0_1'], ex, sc, ulps=0.5, fraction=0.995)
    # ---- every stored layer from the engine's own stored inputs: half an ulp, every element ----
    for l in range(1, 5):
        x = stored['conv%d_%d' % (l - 1, arch.n_block[l - 1] - 1)]
        for i in range(arch.n_block[l]):
            nm = 'conv%d_%d' % (l, i)
            ex = layer(x, params[nm], stride=2 if i == 0 else 1, round_w=True)
            report[nm] = grade(nm, stored[nm], ex, float(np.abs(ex).max()))
            x = stored[nm]
    # the grade is not vacuous: the same layer with the folded kernel NOT rounded to bf16 (what an fp32-weight path would compute) misses it
    wrong = layer(stored['conv2_0'], params['conv2_1'])
    tol = tolerance(wrong, float(np.abs(wrong).max()), 0.5)
    assert np.mean(np.abs(stored['conv2_1'].astype(np.float64) - wrong) <= tol) < 0.9
    up = stored['conv4_%d' % (arch.n_block[4] - 1)]
    for l in (3, 2, 1, 0):
        nm = 'up%d_t' % l
        ex = layer(up, params[nm], stride=2, transposed=True, round_w=True)
        report[nm] = grade(nm, stored[nm], ex, float(np.abs(ex).max()))
        x = np.concatenate([stored['conv%d_%d' % (l, arch.n_block[l] - 1)], stored[nm]], axis=-1)      # skip first (network_ao.py:51)
        for i in range(arch.n_block[l]):
            nm = 'up%d_%d' % (l, i)
            if nm not in stored:
                break
            ex = layer(x, params[nm], round_w=True)
            report[nm] = grade(nm, stored[nm], ex, float(np.abs(ex).max()))
            x = stored[nm]
        up = x
    # ---- tail: up0_0 -> bf16 -> up0_1 -> bf16 -> logits (fp32 kernel as bf16 hi + lo), softmax / argmax; x = the last stored map(s) in front of it ----
    a = x
    for i in range(arch.n_block[0]):
        if 'up0_%d' % i not in stored:
            a = bf16_round(layer(a, params['up0_%d' % i], round_w=True).astype(np.float32))
    pl = params['logits']
    logits = O.conv2d_same(a.astype(np.float64), pl['kernel'].astype(np.float64), 1) + pl['bias'].astype(np.float64)
    lsc = float(np.abs(logits).max())
    err = np.abs(out['logits'].astype(np.float64) - logits)
    # a flipped rounding of one up0_0 / up0_1 value moves a logit by (one bf16 ulp of that value) x a few weights: a few 1e-3 of the scale at worst
    assert err.max() <= 2e-2 * lsc and np.mean(err <= 2e-4 * lsc) >= 0.99, (float(err.max() / lsc), float(np.mean(err <= 2e-4 * lsc)))
    report['tail logits rel'] = float(err.max() / lsc)
    flips = out['pred'] != np.argmax(logits, -1)
    assert np.all(O.top2_margin(logits)[flips] <= 4e-2 * lsc) and flips.mean() < 2e-3, (int(flips.sum()), float(flips.mean()))
    print('bf16 layers vs specified arithmetic %s: %s' % (shape, {k: round(v, 6) for k, v in report.items()}))


def test_bf16_conv_lstm_against_its_rounding_model():
    """The bf16 ConvLSTM (kernels_ws.hip LS forms; reference common/network_ao.py:255-319) against numpy float64 with the roundings the header specifies
    (include/ukbb_fcn.h UKBB_PREC_BF16 on a UNet-LSTM handle): gate kernels rounded to bf16; gx = the x half of the gates ROUNDED TO bf16 (it is stored);
    per direction the first step from that rounded gx (the x pass's epilogue rounds before its cell update: tests/test_lstm_launches_gpu.py holds h1
    against both models and only this one passes), later steps from gx + W_h * h; cell state fp32; every hidden map rounded to bf16 as stored; the output conv in
    fp32 weights on those maps.  Input: the engine's own stored U-Net features (bf16).  A flipped rounding of one gx / h value (its exact value within fp32
    error of a rounding boundary) moves what it feeds by a bf16 ulp, and nine steps carry it on, so the bound is on the logits, not per element of every
    map: measured max 1.5e-3 of the logits' scale, 99.9 % within 2.7e-4, median 1.3e-8 (with the first step taken from the un-rounded gates, as this model
    once did: 2.2e-3, 1.2e-3, 6e-5) -- five to thirteen times closer than to the un-rounded float64 graph on the same features (7.8e-3 / 3.6e-3), which is what says the roundings sit where they are specified."""
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.engine import Engine
    from ukbb_cardiac_amd.phantom import cine_phantom
    from ukbb_cardiac_amd.weights import synthetic_params
    arch = MODELS['UNet-LSTM_ao']
    params = synthetic_params(arch, 1234)
    T, nh = arch.fc, arch.same_dim
    N, H, W = 2, 64, 80
    img = ((cine_phantom(N * T, H, W, seed=3) - 0.3) / 0.25).astype(np.float32).reshape(N, T, H, W, 1)
    with Engine(arch, params) as eng:
        eng.set_precision('bf16')
        out = eng.run_seq(img, want_logits=True)
        feats = eng.activation('up0').reshape(N, T, H, W, -1)
    assert np.array_equal(feats, bf16_round(feats))
    feats = feats.astype(np.float64)

    def sig(x):
        return 1.0 / (1.0 + np.exp(-x))

    def direction(p, order):
        k, b = bf16_round(p['kernel']).astype(np.float64), p['bias'].astype(np.float64)
        kx, kh = k[:, :, :arch.n_filter[0]], k[:, :, arch.n_filter[0]:]
        h = c = None
        hs = {}
        for step, t in enumerate(order):
            gx = O.conv2d_same(feats[:, t], kx, 1) + b
            gx = bf16_round(gx.astype(np.float32)).astype(np.float64)
            z = gx if step == 0 else gx + O.conv2d_same(h, kh, 1)
            i, j, f, o = np.split(z, 4, axis=-1)                          # gate order i, j, f, o; forget bias 1 (conv_lstm_cell in the oracle)
            c = (sig(f + 1.0) * (0.0 if step == 0 else c) + sig(i) * np.tanh(j)).astype(np.float32).astype(np.float64)
            h = bf16_round((np.tanh(c) * sig(o)).astype(np.float32)).astype(np.float64)
            hs[t] = h
        return hs
    fw, bw = direction(params['lstm_fw'], list(range(T))), direction(params['lstm_bw'], list(range(T - 1, -1, -1)))
    po = params['lstm_out']
    model = np.stack([O.conv2d_same(np.concatenate([fw[t], bw[t]], -1), po['kernel'].astype(np.float64), 1) + po['bias'] for t in range(T)], 1)
    sc = float(np.abs(model).max())
    err = np.abs(out['logits'] - model) / sc
    unrounded = np.abs(out['logits'] - O.biconv_lstm(feats, params, nh)) / sc
    print('bf16 ConvLSTM vs its rounding model: max %.2e, 99.9 %% %.2e, median %.2e of the scale; vs the un-rounded graph: max %.2e, 99.9 %% %.2e' % (
        err.max(), np.percentile(err, 99.9), np.median(err), unrounded.max(), np.percentile(unrounded, 99.9)))
    assert err.max() <= 6e-3 and np.percentile(err, 99.9) <= 3e-3 and np.median(err) <= 2e-4
    assert np.percentile(err, 99.9) < 0.6 * np.percentile(unrounded, 99.9)
    assert (out['pred'] == model.argmax(-1)).mean() >= 0.999
