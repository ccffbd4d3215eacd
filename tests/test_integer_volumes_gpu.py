"""uint8 / int16 / uint16 volumes on the device pre-processing path (the *_t entry points of include/ukbb_fcn.h), bit for bit
against the host path, which numpy's integer arithmetic defines: exact selection, the packed network input (clip truncated
toward zero, float64 rescale), the z-score statistics and batch (float64), labels of every sequence model, and the two
deploy scripts end to end with integer gzip files."""
import ctypes as C

import numpy as np
import pytest

from ukbb_cardiac_amd import device_pipeline as dp

pytestmark = pytest.mark.gpu

INT_DTYPES = [np.int16, np.uint16, np.uint8]


def _cuda(a):
    import torch
    return dp._to_device(a, torch.device('cuda', 0))


def _mr_like(shape, dtype, seed, order='F'):
    """MR-like magnitudes in the dtype's range: a gamma body with a heavy tail, background ties; int16 gets negative values
    too and uint16 values above 32767, so a signedness slip shows."""
    rng = np.random.default_rng(seed)
    v = rng.gamma(1.5, 1.0, size=shape)
    v[rng.random(shape) < 0.08] = 0.0
    if dtype == np.uint8:
        v = v * 40.0
    elif dtype == np.int16:
        v = v * 3000.0 - 2000.0
    else:
        v = v * 12000.0
    info = np.iinfo(dtype)
    return np.asarray(np.clip(np.round(v), info.min, info.max).astype(dtype), order=order)


def _engine(model):
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.engine import Engine
    from ukbb_cardiac_amd.weights import synthetic_params
    arch = MODELS[model]
    return Engine(arch, synthetic_params(arch, 1234))


@pytest.fixture(scope='module')
def fcn():
    eng = _engine('FCN_sa')
    yield eng
    eng.close()


# ---- selection ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', INT_DTYPES)
@pytest.mark.parametrize('n', [1, 5, 4096, 1000003])
def test_select_kth_t_equals_partition(dtype, n):
    from ukbb_cardiac_amd import _lib
    a = _mr_like((n,), dtype, n)
    info = np.iinfo(dtype)
    if n > 10:
        a[1], a[2] = info.min, info.max
    if dtype == np.int16:
        assert n < 10 or (a < 0).any()
    if dtype == np.uint16:
        assert n < 10 or (a > 32767).any()
    t = _cuda(a)
    ranks = sorted({0, n // 100, n // 10, (99 * n) // 100, n - 1})
    got = dp._select(t, dtype, ranks, 0)
    want = np.partition(a, ranks)[ranks]
    assert got.dtype == dtype
    np.testing.assert_array_equal(got, want)
    out = np.empty(1, np.float64)
    r = (C.c_uint64 * 1)(0)
    for bad in (16, 8, 256, 0):                                  # float32, int32, int8, unknown: refused with a message
        assert _lib.lib.ukbb_fcn_select_kth_t(t.data_ptr(), bad, n, r, 1, out.ctypes.data_as(C.POINTER(C.c_double)), 0) == -1
        assert 'datatype' in _lib.last_error()


# ---- packed network input ------------------------------------------------------------------------------------------------

def _host_slices(vol, eng):
    """The `slices` pipeline.segment_sequence hands to the network (and its labels), from a copy of vol."""
    from ukbb_cardiac_amd.pipeline import segment_sequence
    seen = []

    def forward(b):
        seen.append(b[..., 0].copy())
        return eng.run(b, want_prob=False)
    host = vol.copy(order='K')
    pred = segment_sequence(host, forward, batch_slices=1 << 20)
    return seen[0], pred, host


def _negative_fraction_bound(shape, seed):
    """int16 volume whose 1 % percentile is -9.35: the clip stores -9 (truncation), floor would give -10."""
    n = int(np.prod(shape))
    k = int((n - 1) * 0.01)
    v = _mr_like(shape, np.int16, seed).reshape(-1, order='F')
    v = np.abs(v)
    rng = np.random.default_rng(seed)
    idx = rng.permutation(n)[:k + 2]
    v[idx[:k + 1]] = -10
    v[idx[k + 1]] = -9
    vol = np.asfortranarray(v.reshape(shape, order='F'))
    lo = np.percentile(vol, (1, 99))[0]
    assert -10 < lo < -9 and lo != np.floor(lo)
    return vol


@pytest.mark.parametrize('dtype', INT_DTYPES)
@pytest.mark.parametrize('shape,order', [((162, 204, 2, 3), 'F'), ((51, 33, 1, 2), 'C'), ((37, 41, 3, 5), 'F')])
def test_rescale_pack_t_equals_host_slices(fcn, dtype, shape, order):
    import torch
    from ukbb_cardiac_amd.pipeline import pad_amounts
    X, Y, Z, T = shape
    vol = _mr_like(shape, dtype, X + Y, order)
    if dtype == np.int16 and shape == (51, 33, 1, 2):
        vol = np.asarray(_negative_fraction_bound(shape, 5), order='C')
    want, _, clipped = _host_slices(vol, fcn)
    t = _cuda(vol)
    lo, hi = dp.device_percentiles(t, (1, 99), 0, dtype)
    assert (lo, hi) == tuple(np.percentile(vol, (1, 99)))
    X2, Y2, x_pre, _, y_pre, _ = pad_amounts(X, Y)
    batch = torch.full((T * Z, X2, Y2), np.nan, dtype=torch.float32, device='cuda')
    dp.pack_rescaled(t.data_ptr(), dtype, shape, t.stride(), lo, hi, (X2, Y2, x_pre, y_pre), batch.data_ptr(), 0)
    got = batch.cpu().numpy()
    assert got.view(np.uint32).tobytes() == want.view(np.uint32).tobytes()
    np.testing.assert_array_equal(dp.clip_like_reference(vol[..., 1], (lo, hi)), clipped[..., 1])   # the saved ED/ES frames


# ---- z-score ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', INT_DTYPES)
@pytest.mark.parametrize('shape,order,seed', [((240, 196, 1, 50), 'F', 1), ((61, 47, 2, 11), 'C', 3), ((33, 250, 1, 9), 'F', 5)])
def test_zscore_t_is_normalise_intensity(dtype, shape, order, seed):
    import torch
    from ukbb_cardiac_amd.image_utils import normalise_intensity
    from ukbb_cardiac_amd.pipeline import pad_amounts_fixed
    img = _mr_like(shape, dtype, seed, order)
    X, Y, Z, T = shape
    t = _cuda(img)
    mu, den, n_roi, val_l = dp.device_zscore_stats(t, 10.0, 0, dtype)
    want_l = np.percentile(img, 10.0)
    roi = img >= want_l
    assert val_l == want_l and n_roi == int(roi.sum())
    assert mu == np.mean(img[roi]) and type(mu) is np.float64
    assert den == np.std(img[roi]) + 1e-6 and type(den) is np.float64
    X2, Y2, x_pre, x_post, y_pre, y_post = pad_amounts_fixed(X, Y)
    batch = torch.empty((T * Z, X2, Y2), dtype=torch.float32, device='cuda')
    dp.zscore_pack(t.data_ptr(), dtype, shape, t.stride(), mu, den, (X2, Y2, x_pre, y_pre), batch.data_ptr(), 0)
    norm = normalise_intensity(img, 10.0)
    assert norm.dtype == np.float64
    padded = np.pad(norm, ((x_pre, x_post), (y_pre, y_post), (0, 0), (0, 0)), 'constant')
    want = np.transpose(padded, (3, 2, 0, 1)).reshape(T * Z, X2, Y2).astype(np.float32)
    assert batch.cpu().numpy().view(np.uint32).tobytes() == want.view(np.uint32).tobytes()


@pytest.mark.parametrize('dtype', INT_DTYPES)
def test_zscore_self_check_is_keyed_by_dtype(fcn, dtype):
    assert dp.device_zscore_matches_numpy(fcn, dtype=dtype)
    assert (fcn.device, np.dtype(dtype)) in dp._ZSCORE_OK


# ---- labels ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', INT_DTYPES)
def test_segment_sequence_device_integer_equals_host_path(fcn, dtype):
    from ukbb_cardiac_amd.phantom import cine_phantom
    Z, T = 3, 5
    v = cine_phantom(Z * T, 162, 204, seed=3)[..., 0].reshape(T, Z, 162, 204).transpose(2, 3, 1, 0)
    info = np.iinfo(dtype)
    v = v * (200.0 if dtype == np.uint8 else 30000.0) + (-3000.0 if dtype == np.int16 else 0.0)
    vol = np.asfortranarray(np.clip(np.round(v), info.min, info.max).astype(dtype))
    keep = vol.copy()
    _, want, clipped = _host_slices(vol, fcn)
    got, aux = dp.segment_sequence_device(vol, fcn, batch_slices=7, return_aux=True)
    assert np.array_equal(vol, keep)                                       # input untouched
    assert got.dtype == np.float64 and got.shape == vol.shape
    np.testing.assert_array_equal(got, want)
    counts = np.stack([[np.sum(want[..., t] == c) for c in range(fcn.arch.n_class)] for t in range(T)])
    np.testing.assert_array_equal(aux['counts'], counts)
    for k in range(T):
        np.testing.assert_array_equal(dp.clip_like_reference(vol[..., k], aux['clip']), clipped[..., k])


@pytest.mark.parametrize('dtype', INT_DTYPES)
def test_aortic_unet_sequence_device_integer_equals_host_path(dtype):
    from ukbb_cardiac_amd import pipeline
    eng = _engine('UNet_ao')
    try:
        shape = (70, 90, 1, 7)
        vol = _mr_like(shape, dtype, 11)
        prob = pipeline.aortic_prob_sequence(vol.copy(), lambda b: eng.run(b), batch_slices=64)
        want = np.argmax(prob, axis=-1).astype(np.int32)
        got, aux = dp.aortic_sequence_device(vol, eng, batch_slices=64, return_aux=True)
        np.testing.assert_array_equal(got, want)
        counts = np.stack([[np.sum(want[..., t] == c) for c in range(3)] for t in range(shape[3])])
        np.testing.assert_array_equal(aux['counts'], counts)
    finally:
        eng.close()


@pytest.mark.parametrize('model', ['UNet-LSTM_ao', 'Temporal-UNet_ao'])
@pytest.mark.parametrize('time_step', [1, 2])
def test_aortic_lstm_sequence_device_integer_equals_host_path(model, time_step):
    from ukbb_cardiac_amd import pipeline
    eng = _engine(model)
    try:
        for i, dtype in enumerate(INT_DTYPES):
            shape = (64, 48, 1, 11)
            vol = _mr_like(shape, dtype, 20 + i + time_step)
            prob = pipeline.aortic_lstm_prob_sequence(vol.copy(), lambda f, R, r, ts=1: eng.run_cine(f, R, r, ts)[0], time_step=time_step)
            want = np.argmax(prob, axis=-1).astype(np.int32)
            got, aux = dp.aortic_sequence_device(vol, eng, window=(5, 0.1, time_step), return_aux=True, prob=True)
            np.testing.assert_array_equal(aux['prob'], prob)
            np.testing.assert_array_equal(got, want)
    finally:
        eng.close()


# ---- deploy scripts -----------------------------------------------------------------------------------------------------------

def test_subject_pipeline_mixed_dtypes(fcn):
    """One SubjectPipeline, subjects of four dtypes in a row (staged and plain arrays): each equals the one-at-a-time device path."""
    from ukbb_cardiac_amd.subject_pipeline import SubjectPipeline, labels_as_float64
    shape = (130, 150, 2, 3)
    vols = [_mr_like(shape, dt, 60 + i) for i, dt in enumerate([np.int16, np.int16, np.uint16, np.uint8, np.int16])]
    vols[1] = np.asfortranarray(vols[1].astype(np.float32))
    want = [dp.segment_sequence_device(v, fcn, batch_slices=5, return_aux=True) for v in vols]
    pipe = SubjectPipeline(fcn, shape, batch_slices=5, depth=3, extra_inputs=2)

    def source():
        for i, v in enumerate(vols):
            if i % 2 == 0:
                st = pipe.stage(v.shape, v.dtype)
                assert st.array.dtype == v.dtype and st.array.flags.f_contiguous
                st.array[...] = v
                yield st.array
            else:
                yield v
    n = 0
    for res, (w_pred, w_aux) in zip(pipe.run(source()), want):
        np.testing.assert_array_equal(labels_as_float64(res.labels), w_pred)
        np.testing.assert_array_equal(res.counts, w_aux['counts'])
        assert res.clip == w_aux['clip']
        np.testing.assert_array_equal(res.image, vols[n])
        n += 1
    assert n == len(vols) and pipe._in_free.qsize() == 5


def test_pipelined_cohort_mixing_float32_and_int16_files(tmp_path, monkeypatch):
    """deploy_network in pipelined sequence mode on gzip subjects of float32 and int16: every output file byte-identical to
    --nodevice_preproc, and no int16 subject takes the sequential fallback."""
    import gzip
    from ukbb_cardiac_amd import deploy_network, nifti
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.phantom import cine_phantom
    from ukbb_cardiac_amd.weights import save_blob, synthetic_params
    arch = MODELS['FCN_sa']
    model = str(tmp_path / 'FCN_sa')
    save_blob(model + '.ukbbw', arch, synthetic_params(arch, 1234))
    X, Y, Z, T = 120, 110, 2, 4
    subjects = {}
    for i, dt in enumerate([np.int16, np.float32, np.int16, np.int16, np.float32]):
        v = cine_phantom(Z * T, X, Y, seed=80 + i)[..., 0].reshape(T, Z, X, Y).transpose(2, 3, 1, 0) * 2500.0 - 150.0
        subjects['s%d' % i] = np.asfortranarray(np.round(v).astype(dt))
    files = ('seg_sa.nii.gz', 'sa_ED.nii.gz', 'sa_ES.nii.gz', 'seg_sa_ED.nii.gz', 'seg_sa_ES.nii.gz')
    outs = {}
    for mode in ('device', 'host'):
        for name, vol in subjects.items():
            d = tmp_path / mode / name
            d.mkdir(parents=True)
            nifti.save(vol, str(d / 'sa.nii.gz'), np.diag([1.8, 1.8, 10.0, 1.0]), pixdim=[1, 1.8, 1.8, 10, 0.03, 0, 0, 0])
            assert nifti.load(str(d / 'sa.nii.gz')).get_data().dtype == vol.dtype
        if mode == 'device':
            def no_fallback(*a, **k):
                raise AssertionError('subject %s left the pipeline' % (a[1][0],))
            monkeypatch.setattr(deploy_network, '_sequence_subject', no_fallback)
        else:
            monkeypatch.undo()
        deploy_network.main(['--seq_name', 'sa', '--data_dir', str(tmp_path / mode), '--model_path', model, '--io_threads', '2',
                             '--device_preproc' if mode == 'device' else '--nodevice_preproc'])
        outs[mode] = {(n, f): gzip.open(str(tmp_path / mode / n / f)).read() for n in subjects for f in files}
    for key in outs['host']:
        assert outs['device'][key] == outs['host'][key], key


def test_aortic_deploy_int16_cine_takes_the_device_path(tmp_path, monkeypatch):
    from ukbb_cardiac_amd import deploy_network_ao, nifti, pipeline
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.weights import save_blob, synthetic_params
    arch = MODELS['UNet-LSTM_ao']
    mp = str(tmp_path / 'UNet-LSTM_ao')
    save_blob(mp + '.ukbbw', arch, synthetic_params(arch, 1234))
    vol = _mr_like((70, 90, 1, 11), np.int16, 31)
    segs = {}
    for mode in ('device', 'host'):
        d = tmp_path / mode / 'subj1'
        d.mkdir(parents=True)
        nifti.save(vol, str(d / 'ao.nii.gz'), np.diag([1.6, 1.6, 6.0, 1.0]), pixdim=[1, 1.6, 1.6, 6, 0.01, 0, 0, 0])
        if mode == 'device':
            def host_path(*a, **k):
                raise AssertionError('the int16 cine took the host path')
            monkeypatch.setattr(pipeline, 'aortic_lstm_prob_sequence', host_path)
        else:
            monkeypatch.undo()
        deploy_network_ao.main(['--seq_name', 'ao', '--data_dir', str(tmp_path / mode), '--model_path', mp,
                                '--device_preproc' if mode == 'device' else '--nodevice_preproc'])
        segs[mode] = nifti.load(str(d / 'seg_ao.nii.gz')).get_data()
    assert segs['device'].dtype == np.int32
    np.testing.assert_array_equal(segs['device'], segs['host'])
