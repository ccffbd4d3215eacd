"""The aortic Temporal-UNet (network_ao.py:67-114) without a GPU: the float64 restatement of its 3-D convolutions
against torch-CPU (second source), weight layout and count (ctypes), checkpoint import, weight blob, and the deploy
script's windowed branch driven by a stub."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import temporal_unet_ref as R
from tf_bundle_writer import write_checkpoint
from ukbb_cardiac_amd import tf_checkpoint as tfc
from ukbb_cardiac_amd.arch import KIND_TEMPORAL_UNET, MODELS
from ukbb_cardiac_amd.weights import load_blob, pack_flat, save_blob, synthetic_params

ARCH = MODELS['Temporal-UNet_ao']


def _tf_tensors(arch, params):
    return {tf: params[layer][key] for layer, names in tfc.variable_names(arch).items() for key, tf in names.items()}


@pytest.mark.parametrize('stride,shape', [(1, (2, 5, 8, 12, 3)), (2, (1, 4, 8, 12, 3)), (2, (1, 3, 6, 10, 2))])
def test_conv3d_same_matches_torch(stride, shape):
    rng = np.random.default_rng(stride + shape[3])
    x = rng.standard_normal(shape)
    w = rng.standard_normal((3, 3, 3, shape[-1], 4))
    got = R.conv3d_same(x, w, stride)
    # TF SAME: time pads 1/1; spatial pad_before = total // 2, extra pixel after
    pads = []
    for n in (shape[3], shape[2]):                                     # F.pad order: W then H (then T)
        out = -(-n // stride)
        tot = max((out - 1) * stride + 3 - n, 0)
        pads += [tot // 2, tot - tot // 2]
    xt = torch.from_numpy(x).permute(0, 4, 1, 2, 3)                    # NCDHW
    xt = TF.pad(xt, pads + [1, 1])
    want = TF.conv3d(xt, torch.from_numpy(w).permute(4, 3, 0, 1, 2), stride=(1, stride, stride))
    np.testing.assert_allclose(got, want.permute(0, 2, 3, 4, 1).numpy(), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('shape', [(1, 5, 4, 6, 3), (2, 3, 3, 5, 2)])
def test_conv3d_transpose_same_matches_torch(shape):
    rng = np.random.default_rng(shape[2])
    x = rng.standard_normal(shape)
    w = rng.standard_normal((3, 3, 3, 4, shape[-1]))                   # [kd,kh,kw,Cout,Cin]
    got = R.conv3d_transpose_same(x, w, 2)
    # torch: weight [Cin,Cout,kd,kh,kw]; time padding 1 (out = T), spatial 0 (out = 2n + 1), crop the trailing row / column
    want = TF.conv_transpose3d(torch.from_numpy(x).permute(0, 4, 1, 2, 3), torch.from_numpy(w).permute(4, 3, 0, 1, 2),
                               stride=(1, 2, 2), padding=(1, 0, 0))
    want = want[:, :, :, :2 * shape[2], :2 * shape[3]].permute(0, 2, 3, 4, 1).numpy()
    assert got.shape == want.shape == (shape[0], shape[1], 2 * shape[2], 2 * shape[3], 4)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)


def test_transposed_conv_along_time_is_the_reference_formula():
    """out[t] = sum_k in[t + 1 - k] W[k] (stride 1 along time, zero frames at the window edges)."""
    rng = np.random.default_rng(2)
    x = rng.standard_normal((1, 6, 1, 1, 1))
    w = np.zeros((3, 3, 3, 1, 1))
    w[:, 0, 0, 0, 0] = [1.0, 10.0, 100.0]
    got = R.conv3d_transpose_same(x, w, 2)[0, :, 0, 0, 0]
    xs = np.pad(x[0, :, 0, 0, 0], 1)
    want = [sum(xs[t + 1 + 1 - k] * w[k, 0, 0, 0, 0] for k in range(3)) for t in range(6)]
    np.testing.assert_allclose(got, want, rtol=1e-14)


def test_weight_count_matches_the_library():
    from ukbb_cardiac_amd import _lib
    for name, arch in MODELS.items():
        a = _lib.arch_struct(arch)
        assert _lib.lib.ukbb_fcn_weight_count(C.byref(a)) == arch.n_weight_floats(), name
    assert ARCH.kind == KIND_TEMPORAL_UNET == 3 and ARCH.fc == 9
    specs = ARCH.layer_specs()
    assert specs[0].kernel_shape == (3, 3, 3, 1, 16) and specs[0].kd == 3
    assert [s.name for s in specs] == [s.name for s in MODELS['UNet_ao'].layer_specs()]
    ups = {s.name: s for s in specs}
    assert ups['up3_t'].kernel_shape == (3, 3, 3, 128, 256) and ups['up3_t'].transposed
    assert ups['logits'].kernel_shape == (1, 1, 1, 16, 3) and ups['logits'].has_bias
    # three time taps: the kernels hold 3x the 2-D U-Net's 3x3 weights
    unet = MODELS['UNet_ao']
    k2 = sum(int(np.prod(s.kernel_shape)) for s in unet.layer_specs() if s.name != 'logits')
    k3 = sum(int(np.prod(s.kernel_shape)) for s in specs if s.name != 'logits')
    assert k3 == 3 * k2
    # unchanged for the existing kinds (the flat layouts their checkpoints and blobs use)
    assert {m: MODELS[m].n_weight_floats() for m in MODELS if m != 'Temporal-UNet_ao'} == {
        'FCN_sa': 1989012, 'FCN_la_2ch': 1988882, 'FCN_la_4ch': 1988947, 'FCN_la_4ch_seg4': 1989142,
        'UNet_ao': 2163587, 'UNet-LSTM_ao': 2200627}
    assert all(s.kd == 1 for m in MODELS.values() if m.kind != KIND_TEMPORAL_UNET for s in m.layer_specs())


def test_checkpoint_variable_names():
    n = tfc.variable_names(ARCH)
    assert n['conv0_0']['kernel'] == 'Temporal_UNet/conv0/conv3d/kernel'
    assert n['conv0_1']['kernel'] == 'Temporal_UNet/conv0/conv3d_1/kernel'
    assert n['conv2_1']['var'] == 'Temporal_UNet/conv2/batch_normalization_1/moving_variance'
    assert n['up3_t']['kernel'] == 'Temporal_UNet/conv3_up/conv3d_transpose/kernel'
    assert n['up3_t']['gamma'] == 'Temporal_UNet/conv3_up/batch_normalization/gamma'
    assert n['up3_0']['kernel'] == 'Temporal_UNet/conv3_up/conv3d/kernel'
    assert n['up3_1']['mean'] == 'Temporal_UNet/conv3_up/batch_normalization_2/moving_mean'
    assert n['logits'] == {'kernel': 'Temporal_UNet/conv_out/conv3d/kernel', 'bias': 'Temporal_UNet/conv_out/conv3d/bias'}


def test_checkpoint_loads_as_temporal_unet(tmp_path):
    from ukbb_cardiac_amd.engine import load_model
    params = synthetic_params(ARCH, 11)
    prefix = str(tmp_path / 'Temporal-UNet')
    t = _tf_tensors(ARCH, params)
    t['global_step'] = np.int64(1000)
    t['Temporal_UNet/conv0/conv3d/kernel/Adam'] = np.zeros((3, 3, 3, 1, 16), np.float32)   # optimizer slots are ignored
    write_checkpoint(prefix, t, tensor_crc=False)
    arch, got = load_model(prefix)                                    # what Session(model_path) binds
    assert arch == ARCH and arch.kind == KIND_TEMPORAL_UNET
    assert arch.n_filter == (16, 32, 64, 128, 256) and arch.n_class == 3 and arch.fc == 9
    np.testing.assert_array_equal(pack_flat(arch, got), pack_flat(ARCH, params))
    for layer in params:
        for key in params[layer]:
            np.testing.assert_array_equal(got[layer][key], params[layer][key])
    # blob round trip (the converter CLI and save_blob / load_blob)
    assert tfc.main([prefix, '-o', str(tmp_path / 'm.ukbbw')]) == 0
    arch2, p2 = load_blob(str(tmp_path / 'm.ukbbw'))
    assert arch2 == ARCH
    np.testing.assert_array_equal(pack_flat(arch2, p2), pack_flat(ARCH, params))
    save_blob(str(tmp_path / 'n.ukbbw'), ARCH, params)
    arch3, p3 = load_blob(str(tmp_path / 'n.ukbbw'))
    assert arch3 == ARCH
    np.testing.assert_array_equal(pack_flat(arch3, p3), pack_flat(ARCH, params))


def test_checkpoint_with_other_filters_and_classes(tmp_path):
    from ukbb_cardiac_amd.arch import ModelArch
    arch = ModelArch('x', KIND_TEMPORAL_UNET, 2, n_filter=(16, 32, 64, 128, 128), n_block=(2, 2, 3, 2, 2), fc=9)
    params = synthetic_params(arch, 3)
    prefix = str(tmp_path / 'c')
    write_checkpoint(prefix, _tf_tensors(arch, params), tensor_crc=False)
    arch2, got = tfc.checkpoint_to_params(prefix)
    assert arch2.kind == KIND_TEMPORAL_UNET and arch2.n_filter == arch.n_filter and arch2.n_block == arch.n_block
    assert arch2.n_class == 2 and arch2.fc == 9
    np.testing.assert_array_equal(pack_flat(arch2, got), pack_flat(arch, params))


def _subject(tmp_path, shape=(40, 36, 1, 7)):
    from ukbb_cardiac_amd import nifti
    d = tmp_path / 'data' / 's1'
    d.mkdir(parents=True)
    vol = np.round(100 * np.random.default_rng(4).gamma(2.0, 1.0, size=shape)).astype(np.float32)
    nifti.save(vol, str(d / 'ao.nii.gz'), np.diag([1.6, 1.6, 6.0, 1.0]), pixdim=[1, 1.6, 1.6, 6, 0.01, 0, 0, 0])
    return d, vol


def test_deploy_temporal_unet_with_a_stub(tmp_path):
    from ukbb_cardiac_amd import deploy_network_ao as DA, nifti
    d, vol = _subject(tmp_path)
    seen = []

    def cine(frames, weight_R, weight_r, time_step=1):
        seen.append((frames.shape, weight_R, weight_r, time_step))
        p = np.zeros(frames.shape + (3,), np.float32)
        p[..., 2] = 1.0
        p[:, :128, :, 2] = 0.0
        p[:, :128, :, 1] = 1.0                                          # label 1 in the upper half of the padded frame, 2 below
        return p
    F, _ = DA.define_flags().parse(['--data_dir', str(tmp_path / 'data'), '--model', 'Temporal-UNet', '--model_path', 'x',
                                    '--time_step', '3', '--weight_R', '5', '--io_threads', '0'])
    assert DA.run(F, None, log=lambda *_: None, cine_forward=cine) == ['s1']
    assert seen == [((7, 256, 256), 5, 0.1, 3)]
    seg = nifti.load(str(d / 'seg_ao.nii.gz')).get_data()
    assert seg.dtype == np.int32 and seg.shape == vol.shape
    x_pre = (256 - 40) // 2
    want = np.where(np.arange(40)[:, None, None, None] + x_pre < 128, 1, 2) * np.ones(vol.shape, np.int32)
    np.testing.assert_array_equal(seg, want)
    F2, _ = DA.define_flags().parse(['--data_dir', str(tmp_path / 'data'), '--model', 'Temporal-UNet', '--noprocess_seq'])
    assert DA.run(F2, None, log=lambda *_: None, cine_forward=cine) == []      # windowed models need sequence mode


def test_deploy_main_refuses_a_model_of_the_other_kind(tmp_path, monkeypatch):
    """--model Temporal-UNet with a UNet checkpoint, and --model UNet with a Temporal-UNet one: exit with a message
    (the check runs on the loaded architecture, before any forward)."""
    from ukbb_cardiac_amd import deploy_network_ao as DA, engine
    _subject(tmp_path)
    made = []

    class FakeEngine:
        def __init__(self, arch, params, device=0):
            self.arch = arch
            made.append(arch.name)

        def close(self):
            pass
    monkeypatch.setattr(engine, 'Engine', FakeEngine)
    for ckpt_model, flag in (('UNet_ao', 'Temporal-UNet'), ('Temporal-UNet_ao', 'UNet'), ('UNet-LSTM_ao', 'Temporal-UNet'),
                             ('Temporal-UNet_ao', 'UNet-LSTM')):
        arch = MODELS[ckpt_model]
        prefix = str(tmp_path / ckpt_model)
        write_checkpoint(prefix, _tf_tensors(arch, synthetic_params(arch, 1)), tensor_crc=False)
        with pytest.raises(SystemExit) as e:
            DA.main(['--data_dir', str(tmp_path / 'data'), '--model_path', prefix, '--model', flag])
        assert 'holds a' in str(e.value)
    assert made == ['UNet_ao', 'Temporal-UNet_ao', 'UNet-LSTM_ao', 'Temporal-UNet_ao']
    with pytest.raises(SystemExit) as e:
        DA.main(['--data_dir', str(tmp_path / 'data'), '--model_path', prefix, '--model', 'Temporal-UNet', '--precision', 'bf16'])
    assert 'fp32 only' in str(e.value)


def test_macs_table_counts_three_time_taps():
    from ukbb_cardiac_amd.arch import fcn_macs_per_slice
    m3u, m1u = fcn_macs_per_slice(MODELS['UNet_ao'], 256, 256)
    m3, m1 = fcn_macs_per_slice(ARCH, 256, 256)
    assert m3 == 3 * m3u and m1 == m1u
    rows = ARCH.macs_per_pixel_table()
    assert rows[0] == ('conv0_0', 27, 1, 16, False) and rows[-1] == ('logits', 1, 16, 3, False)
