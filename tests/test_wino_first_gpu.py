"""The fused first layer with conv0_1 as Winograd F(2x2,3x3) (kernels_conv.hip, conv_pc_kernel WINO; config 134, the fp32 FCN default).

conv0_0 + conv0_1 is one launch, so the stored conv0_1 map is checked against float64 from the image: numpy through the reference's op
(oracle/fcn_oracle.py conv2d_same, reference common/network.py:19-25) with the BN fold of ukbb_fcn_create, at the headline size, the other
model sizes, N = 1, a map of odd tile counts and a map of a single 16 x 16 tile (every halo pixel on the border is zero padding).  Then the
A/B knob UKBB_NO_WINOGRAD_FIRST=1 (the direct fused kernel) against the default: same outputs to ordinary fp32 rounding (the transforms
reorder the sums), not bit for bit."""
import numpy as np
import pytest

from launch_grading import layer, run_in_child

pytestmark = pytest.mark.gpu
WINO_FIRST = 134


def conv0_1_map(model, n, H, W):
    """(stored conv0_1 map, config id of the conv0_0+conv0_1 launch) of the engine's fp32 plan."""
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.engine import Engine
    from ukbb_cardiac_amd.phantom import cine_phantom
    from ukbb_cardiac_amd.weights import synthetic_params
    arch = MODELS[model]
    params = synthetic_params(arch, 1234)
    img = cine_phantom(n, H, W, seed=17)
    with Engine(arch, params) as eng:
        eng.run(img)
        cfgs = dict(zip(eng.kernel_names(), eng.kernel_configs()))
        name = 'conv0' if arch.n_block[0] == 2 else 'conv0_1'
        got = eng.activation(name).reshape(n, H, W, -1)
    return got, cfgs.get('conv0_0+conv0_1'), img, params


@pytest.mark.parametrize('model,shape', [('FCN_sa', (2, 192, 208)), ('FCN_sa', (3, 80, 112)), ('FCN_la_2ch', (2, 176, 208)),
                                         ('FCN_sa', (1, 192, 208)), ('FCN_sa', (2, 48, 272)), ('FCN_sa', (1, 16, 48))])
def test_winograd_first_layer_against_float64(model, shape):
    n, H, W = shape
    got, cfg, img, params = conv0_1_map(model, n, H, W)
    assert cfg == WINO_FIRST, cfg
    x = img.astype(np.float64)
    ex = layer(layer(x[..., None] if x.ndim == 3 else x, params['conv0_0']), params['conv0_1'])
    sc = float(np.abs(ex).max())
    err = float(np.abs(got.astype(np.float64) - ex).max()) / sc
    print('%s %s: conv0_1 max error / layer scale %.2g' % (model, shape, err))
    assert err <= 1e-5, err


def save_headline_map(path):
    """The stored conv0_1 map of FCN_sa 2 x 192 x 208 with the first layer this process's environment selects, saved; the launch's tiling printed."""
    got, cfg, _, _ = conv0_1_map('FCN_sa', 2, 192, 208)
    np.save(path, got)
    print('cfg', cfg)


def test_direct_knob_against_winograd(tmp_path):
    out = {}
    for tag, knob in (('wino', None), ('direct', '1')):
        path = str(tmp_path / (tag + '.npy'))
        r = run_in_child('test_wino_first_gpu', 'save_headline_map', [path], {'UKBB_NO_WINOGRAD_FIRST': knob} if knob else {}, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:]
        cfg = int(r.stdout.split('cfg')[-1].split()[0])
        assert (cfg == WINO_FIRST) == (knob is None), cfg
        out[tag] = np.load(path).astype(np.float64)
    sc = float(np.abs(out['direct']).max())
    diff = float(np.abs(out['wino'] - out['direct']).max()) / sc
    print('Winograd vs direct conv0_1: max difference / scale %.2g' % diff)
    assert diff <= 1e-5, diff
    assert diff > 0.0                                   # two different summation orders: the knob really switched kernels


@pytest.mark.parametrize('model,precision,want', [('UNet_ao', 'fp32', 'direct'), ('UNet-LSTM_ao', 'fp32', 'direct'),
                                                  ('FCN_sa', 'bf16', 'direct'), ('FCN_sa', 'f32x3', 'winograd')])
def test_winograd_first_layer_only_in_fp32_fcn_plans(model, precision, want):
    """Tiling 134 is taken by the fp32-conv FCN plans only (UKBB_PREC_F32X3 changes the head alone); the U-Net, UNet-LSTM and bf16-operand
    FCN plans keep the direct fused kernel (tilings 130-133)."""
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.engine import Engine
    from ukbb_cardiac_amd.phantom import cine_phantom
    from ukbb_cardiac_amd.weights import synthetic_params
    arch = MODELS[model]
    params = synthetic_params(arch, 1234)
    H, W = 64, 96
    with Engine(arch, params) as eng:
        eng.set_precision(precision)
        if arch.kind == 2:                               # UNet-LSTM: one window of arch.fc frames
            eng.run_seq(cine_phantom(arch.fc, H, W, seed=3).reshape(1, arch.fc, H, W, 1))
        else:
            eng.run(cine_phantom(2, H, W, seed=3))
        cfgs = dict(zip(eng.kernel_names(), eng.kernel_configs()))
    cfg = cfgs.get('conv0_0+conv0_1')
    if want == 'winograd':
        assert cfg == WINO_FIRST, cfgs
    else:
        assert cfg in (130, 131, 132, 133), cfgs
