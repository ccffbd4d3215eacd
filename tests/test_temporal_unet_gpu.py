"""The aortic Temporal-UNet (network_ao.py:67-114, 3-D convolutions: kernels_conv3d.hip) on the GPU against the float64
numpy restatement in tests/temporal_unet_ref.py and the windowed deploy loop of deploy_network_ao.py:129-183."""
import numpy as np
import pytest

import temporal_unet_ref as R
from oracle import fcn_oracle as O

pytestmark = pytest.mark.gpu
LOGIT_TOL = 1e-5            # of the logits scale (fp32 arithmetic, 18 layers; float64 reference)
LAYER_TOL = 1e-6            # of the layer's output scale, one launch from its own stored input
NEAR_TIE = 1e-4             # tests/test_gpu_parity.py: a label flip below this fp64 logit margin is a numerical tie


@pytest.fixture(scope='module')
def model():
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.engine import Engine
    from ukbb_cardiac_amd.weights import synthetic_params
    arch = MODELS['Temporal-UNet_ao']
    params = synthetic_params(arch, 1234)
    eng = Engine(arch, params)
    yield arch, params, eng
    eng.close()


def _check_labels(pred, ref_logits):
    bad = pred != O.argmax_pred(ref_logits)
    margin = O.top2_margin(ref_logits)
    assert not np.any(bad & (margin > NEAR_TIE)), 'label flip away from a numerical tie'
    assert bad.sum() <= max(1, int((margin <= NEAR_TIE).sum()))


@pytest.mark.parametrize('shape', [(2, 9, 32, 48), (1, 9, 256, 256), (1, 9, 48, 80)])
def test_forward_seq_vs_float64_reference(model, shape):
    arch, params, eng = model
    if shape[2] == 256:
        from ukbb_cardiac_amd.phantom import cine_phantom
        x = ((cine_phantom(9, 256, 256, seed=71) - 0.3) / 0.25).astype(np.float32)[None]
    else:
        x = np.random.default_rng(shape[3]).standard_normal(shape + (1,)).astype(np.float32)
    out = eng.run_seq(x, want_logits=True)
    ref = R.temporal_unet(x, params, n_block=arch.n_block)
    scale = np.abs(ref).max()
    err = np.abs(out['logits'] - ref).max()
    assert err <= LOGIT_TOL * scale, 'logits err %.3e vs scale %.3e' % (err, scale)
    assert np.abs(out['prob'] - O.softmax(ref)).max() < 1e-4
    assert out['pred'].dtype == np.int32 and out['pred'].shape == shape
    _check_labels(out['pred'], ref)
    assert np.array_equal(out['pred'], np.argmax(out['prob'], -1))
    assert len(np.unique(out['pred'])) > 1


def test_every_3d_launch_vs_float64_on_its_own_input(model):
    """Every conv3d / conv3d_transpose launch recomputed in float64 from the maps the engine stored (Engine.activation),
    with the engine's folded weights (weights.fold_bn)."""
    from ukbb_cardiac_amd.weights import fold_bn
    arch, params, eng = model
    N, T, H, W = 2, 9, 32, 48
    x = np.random.default_rng(5).standard_normal((N, T, H, W, 1)).astype(np.float32)
    eng.run_seq(x)
    nb = arch.n_block

    def act(name, h, w, c):
        return eng.activation(name).reshape(N, T, h, w, c).astype(np.float64)

    checked = 0

    def check(name, inp, stride=1, transposed=False):
        nonlocal checked
        p = params[name]
        scale, shift = fold_bn(p)
        if transposed:
            wf = (p['kernel'] * scale[:, None]).astype(np.float32)
            y = R.conv3d_transpose_same(inp, wf.astype(np.float64), 2)
        else:
            wf = (p['kernel'] * scale).astype(np.float32)
            y = R.conv3d_same(inp, wf.astype(np.float64), stride)
        want = np.maximum(y + shift.astype(np.float64), 0)
        cout = want.shape[-1]
        got = act(name, want.shape[2], want.shape[3], cout)
        err = np.abs(got - want).max()
        assert err <= LAYER_TOL * np.abs(want).max(), '%s: err %.3e of scale %.3e' % (name, err, np.abs(want).max())
        checked += 1
        return got

    cur = x.astype(np.float64)
    level_out = []
    for l in range(arch.n_level):
        for i in range(nb[l]):
            cur = check('conv%d_%d' % (l, i), cur, 2 if (l > 0 and i == 0) else 1)
        level_out.append(cur)
    for l in range(arch.n_level - 2, -1, -1):
        up = check('up%d_t' % l, cur, transposed=True)
        cur = np.concatenate([level_out[l], up], axis=-1)
        for i in range(nb[l]):
            cur = check('up%d_%d' % (l, i), cur)
    assert checked == sum(nb) + 4 + sum(nb[:-1])


def _exact_loop(eng, frames, time_step):
    """the reference's deploy loop with this engine's forward_seq standing for sess.run: same kernels, same arithmetic"""
    return R.deploy_tiling(frames, lambda x: eng.run_seq(x)['prob'], time_step)


@pytest.mark.parametrize('F,time_step', [(12, 1), (12, 3), (5, 1), (12, 10)])
def test_forward_cine_vs_the_deploy_loop(model, F, time_step):
    """forward_cine against deploy_network_ao.py:129-183 in numpy: bit for bit when the window probabilities come from
    forward_seq, within tolerance (labels up to fp64 near-ties) when they come from the float64 network.  F = 5 < T puts
    duplicate frames in a window (last write wins); time_step 10 > 9 leaves frames no window reaches (NaN, label 0)."""
    arch, params, eng = model
    frames = np.random.default_rng(10 * F + time_step).standard_normal((F, 32, 32)).astype(np.float32)
    prob, pred = eng.run_cine(frames, time_step=time_step)
    exact = _exact_loop(eng, frames, time_step)
    np.testing.assert_array_equal(prob, exact)                               # NaNs compare equal here
    np.testing.assert_array_equal(pred, np.argmax(exact, -1).astype(np.int32))
    ref = R.deploy_tiling(frames, R.window_prob_float64(params, arch.n_block), time_step)
    covered = ~np.isnan(ref).any(axis=(1, 2, 3))
    assert np.array_equal(covered, ~np.isnan(prob).any(axis=(1, 2, 3)))
    assert np.abs(prob[covered] - ref[covered]).max() < 1e-5
    lr = np.log(np.maximum(ref[covered], 1e-30))                              # margins in log-probability = logit units
    _check_labels(pred[covered], lr)
    if time_step > 2 * 5 - 1:
        assert (~covered).any() and (pred[~covered] == 0).all()
    else:
        assert covered.all()


def test_chunked_windows_are_bit_identical(model, monkeypatch):
    """UKBB_TEMPORAL_CHUNK_WINDOWS forces small chunks: same prob / pred bits as one chunk."""
    arch, params, eng = model
    frames = np.random.default_rng(3).standard_normal((13, 32, 48)).astype(np.float32)
    monkeypatch.delenv('UKBB_TEMPORAL_CHUNK_WINDOWS', raising=False)
    prob1, pred1 = eng.run_cine(frames, time_step=1)
    for cw in ('1', '4'):
        monkeypatch.setenv('UKBB_TEMPORAL_CHUNK_WINDOWS', cw)
        prob, pred = eng.run_cine(frames, time_step=1)
        np.testing.assert_array_equal(prob, prob1)
        np.testing.assert_array_equal(pred, pred1)
    monkeypatch.setenv('UKBB_TEMPORAL_CHUNK_WINDOWS', '2')
    prob, pred = eng.run_cine(frames, time_step=2)
    monkeypatch.delenv('UKBB_TEMPORAL_CHUNK_WINDOWS')
    prob2, pred2 = eng.run_cine(frames, time_step=2)
    np.testing.assert_array_equal(prob, prob2)
    np.testing.assert_array_equal(pred, pred2)


def test_session_runs_ntxyc_windows(model):
    """Session.run on a Temporal-UNet takes the reference's 5-D image:0 and returns NTXYC prob / NTXY pred."""
    from ukbb_cardiac_amd.engine import Session
    arch, params, eng = model
    x = np.random.default_rng(8).standard_normal((1, 9, 32, 32, 1)).astype(np.float32)
    with Session(arch=arch, params=params) as sess:
        prob, pred = sess.run(['prob:0', 'pred:0'], feed_dict={'image:0': x, 'training:0': False})
    out = eng.run_seq(x)
    assert prob.shape == (1, 9, 32, 32, 3) and pred.shape == (1, 9, 32, 32)
    np.testing.assert_array_equal(prob, out['prob'])
    np.testing.assert_array_equal(pred, out['pred'])


def test_drop_in_script_device_and_host_paths(tmp_path, model):
    """deploy_network_ao.py --model Temporal-UNet on a gzip cine with a checkpoint written under the reference's variable
    names: the device path (z-score, windows, argmax on the GPU) and --nodevice_preproc write the same labels, equal to the
    deploy loop driven by forward_seq."""
    from ukbb_cardiac_amd import deploy_network_ao, nifti, tf_checkpoint as tfc
    from ukbb_cardiac_amd.image_utils import normalise_intensity
    from tf_bundle_writer import write_checkpoint
    arch, params, eng = model
    prefix = str(tmp_path / 'ckpt' / 'model.ckpt-50000')
    (tmp_path / 'ckpt').mkdir()
    write_checkpoint(prefix, {tf: params[layer][key] for layer, names in tfc.variable_names(arch).items()
                              for key, tf in names.items()}, tensor_crc=False)
    rng = np.random.default_rng(41)
    vol = np.round(100 * rng.gamma(2.0, 1.0, size=(70, 90, 1, 11))).astype(np.float32)
    d = tmp_path / 'data' / 'subj1'
    d.mkdir(parents=True)
    nifti.save(vol, str(d / 'ao.nii.gz'), np.diag([1.6, 1.6, 6.0, 1.0]), pixdim=[1, 1.6, 1.6, 6, 0.01, 0, 0, 0])
    segs = {}
    for flag in ('--device_preproc', '--nodevice_preproc'):
        deploy_network_ao.main(['--data_dir', str(tmp_path / 'data'), '--model_path', prefix, '--model', 'Temporal-UNet',
                                '--time_step', '2', flag])
        segs[flag] = nifti.load(str(d / 'seg_ao.nii.gz')).get_data()
    np.testing.assert_array_equal(segs['--device_preproc'], segs['--nodevice_preproc'])
    want = O.aortic_lstm_prob_sequence(normalise_intensity(vol.copy(), 10.0), lambda x: eng.run_seq(x)['prob'], time_step=2)
    np.testing.assert_array_equal(segs['--device_preproc'], np.argmax(want, -1).astype(np.int32))
    assert len(np.unique(segs['--device_preproc'])) > 1
    with pytest.raises(SystemExit):                                          # bf16 is not built for this kind
        deploy_network_ao.main(['--data_dir', str(tmp_path / 'data'), '--model_path', prefix, '--model', 'Temporal-UNet',
                                '--precision', 'bf16'])


def test_precision_and_frame_calls_are_refused(model):
    from ukbb_cardiac_amd import _lib
    arch, params, eng = model
    with pytest.raises(_lib.UkbbFcnError, match=r'fp32 only.*\(-2\)|\(-2\).*fp32 only'):
        eng.set_precision('bf16')
    with pytest.raises(_lib.UkbbFcnError, match='sequences'):
        eng.run(np.zeros((1, 32, 32, 1), np.float32))
    x = np.random.default_rng(1).standard_normal((1, 9, 32, 32, 1)).astype(np.float32)
    assert eng.run_seq(x)['pred'].shape == (1, 9, 32, 32)                    # the handle still works in fp32
