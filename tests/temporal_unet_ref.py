"""Float64 numpy restatement of the aortic Temporal-UNet (reference common/network_ao.py:67-114 Temporal_UNet,
common/network.py:37-52 conv3d_bn_relu / conv3d_transpose_bn_relu) and of the windowed deploy loop
(common/deploy_network_ao.py:129-183), written from those semantics for the tests of the 3-D kernels.
[TF-recall]: tf.layers.conv3d / conv3d_transpose with padding 'same' -- kernels DHWIO [3,3,3,Cin,Cout] and
[3,3,3,Cout,Cin], TF 'SAME' pads in every dim (along time: one zero frame at each WINDOW edge), BN epsilon 1e-3.
Helper module, no tests of its own."""
import numpy as np

from oracle.fcn_oracle import aortic_window_indices, aortic_window_weights, batch_norm_infer, relu, same_pads, softmax


def conv3d_same(x, w, stride=1):
    """tf.layers.conv3d(padding='same', strides=(1, stride, stride), use_bias=False).
    x: [N,T,H,W,Cin]; w: [kd,kh,kw,Cin,Cout] (cross-correlation, no flip)."""
    n, t, h, wd, cin = x.shape
    kd, kh, kw, cin2, cout = w.shape
    assert cin == cin2
    to, tpb, tpa = same_pads(t, kd, 1)
    ho, pt, pb = same_pads(h, kh, stride)
    wo, pl, pr = same_pads(wd, kw, stride)
    xp = np.pad(x, ((0, 0), (tpb, tpa), (pt, pb), (pl, pr), (0, 0)))
    out = np.zeros((n, to, ho, wo, cout), dtype=x.dtype)
    for a in range(kd):
        for i in range(kh):
            for j in range(kw):
                patch = xp[:, a:a + to, i:i + (ho - 1) * stride + 1:stride, j:j + (wo - 1) * stride + 1:stride, :]
                out += np.tensordot(patch, w[a, i, j].astype(x.dtype), axes=([4], [0]))
    return out


def conv3d_transpose_same(x, w, stride=2):
    """tf.layers.conv3d_transpose(padding='same', strides=(1, stride, stride)): output T x (H*stride) x (W*stride).
    x: [N,T,h,w,Cin]; w: [kd,kh,kw,Cout,Cin].  The gradient of the forward SAME conv: full scatter of length
    (in-1)*s+k per dim, cropped from the forward conv's pad_before -- along time (stride 1) out[t] = sum_k x[t+1-k] W[k]."""
    n, t, h, wd, cin = x.shape
    kd, kh, kw, cout, cin2 = w.shape
    assert cin == cin2
    s = stride
    H, W = h * s, wd * s
    _, tb, _ = same_pads(t, kd, 1)
    _, pt, _ = same_pads(H, kh, s)
    _, pl, _ = same_pads(W, kw, s)
    full = np.zeros((n, t + kd - 1, max((h - 1) * s + kh, pt + H), max((wd - 1) * s + kw, pl + W), cout), dtype=x.dtype)
    for a in range(kd):
        for i in range(kh):
            for j in range(kw):
                full[:, a:a + t, i:i + (h - 1) * s + 1:s, j:j + (wd - 1) * s + 1:s, :] += \
                    np.tensordot(x, w[a, i, j].astype(x.dtype), axes=([4], [1]))
    return full[:, tb:tb + t, pt:pt + H, pl:pl + W, :]


def conv3d_bn_relu(x, p, stride=1):
    y = conv3d_same(x, p['kernel'], stride)
    return relu(batch_norm_infer(y, p['gamma'], p['beta'], p['mean'], p['var']))


def conv3d_transpose_bn_relu(x, p, stride=2):
    y = conv3d_transpose_same(x, p['kernel'], stride)
    return relu(batch_norm_infer(y, p['gamma'], p['beta'], p['mean'], p['var']))


def temporal_unet(x, params, n_level=5, n_block=(2, 2, 2, 2, 2), dtype=np.float64, return_maps=False):
    """Temporal_UNet (network_ao.py:67-114): x [N,T,H,W,1] -> logits [N,T,H,W,n_class] (conv_out: 1x1x1 conv3d + bias).
    return_maps: also {layer name: output map} with the engine's layer names (conv{l}_{i}, up{l}_t, up{l}_{i})."""
    maps = {}
    h = np.asarray(x, dtype)
    skips = []
    for l in range(n_level):
        for i in range(n_block[l]):
            name = 'conv%d_%d' % (l, i)
            h = conv3d_bn_relu(h, params[name], 2 if (l > 0 and i == 0) else 1)
            maps[name] = h
        skips.append(h)
    for l in range(n_level - 2, -1, -1):
        up = conv3d_transpose_bn_relu(h, params['up%d_t' % l], 2)
        maps['up%d_t' % l] = up
        h = np.concatenate([skips[l], up], axis=-1)              # skip first, as in UNet (network_ao.py:51)
        for i in range(n_block[l]):
            name = 'up%d_%d' % (l, i)
            h = conv3d_bn_relu(h, params[name], 1)
            maps[name] = h
    p = params['logits']
    logits = np.tensordot(h, p['kernel'][0, 0, 0].astype(dtype), axes=([4], [0])) + p['bias'].astype(dtype)
    return (logits, maps) if return_maps else logits


def deploy_tiling(frames, window_prob, time_step=1, weight_R=5, weight_r=0.1):
    """deploy_network_ao.py:129-183 for one slice position, in numpy as the reference writes it (fancy-indexed `+=` on a
    float32 accumulator with float64 weights, then `prob /= weight`): frames [F,H,W]; window_prob(x [1,T,H,W,1]) ->
    float32 probabilities [1,T,H,W,C] of one window.  Returns prob [F,H,W,C] (NaN where no window reaches a frame)."""
    F, H, W = frames.shape
    K = 2 * weight_R - 1
    prob = None
    weight = np.zeros((F, 1, 1, 1))
    w = np.reshape(aortic_window_weights(weight_R, weight_r), (K, 1, 1, 1))
    for t in range(0, F, time_step):
        idx = aortic_window_indices(t, F, weight_R)
        p = np.asarray(window_prob(frames[idx][None, ..., None].astype(np.float32)))[0]
        if prob is None:
            prob = np.zeros((F,) + p.shape[1:], np.float32)
        prob[idx] += p * w
        weight[idx] += w
    with np.errstate(invalid='ignore', divide='ignore'):
        prob /= weight
    return prob


def window_prob_float64(params, n_block=(2, 2, 2, 2, 2)):
    """window_prob for deploy_tiling from the float64 network (softmax in float64, rounded to float32 as TF's prob:0 is)."""
    return lambda x: softmax(temporal_unet(x, params, n_block=n_block)).astype(np.float32)
