"""The aortic quality-control statistics on the GPU (device_pipeline.device_qc_stats: ukbb_fcn_label_components,
ukbb_fcn_label_max, ukbb_fcn_label_compact + the pairwise sums) equal aorta_qc.stats_host exactly, for every voxel type the
device path takes, and deploy_network_ao.py --aortic_qc_full gives the same table and messages on the device path as on the
host path."""
import re

import numpy as np
import pytest

from ukbb_cardiac_amd import aorta_qc
from ukbb_cardiac_amd import device_pipeline as dp

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.uint8, np.int16, np.uint16]


def _image(shape, dtype, seed, order='F'):
    rng = np.random.default_rng(seed)
    if dtype == np.float32:
        v = (1000.0 * rng.gamma(2.0, 1.0, size=shape)).astype(np.float32)
    else:
        info = np.iinfo(dtype)
        v = rng.integers(info.min, int(info.max) + 1, size=shape).astype(dtype)
    return np.asfortranarray(v) if order == 'F' else np.ascontiguousarray(v)


def _device_stats(image, seg, n_class=3, min_size=None):
    import torch
    dev = torch.device('cuda', 0)
    vol = dp._to_device(image, dev)
    lab = torch.from_numpy(np.ascontiguousarray(seg.reshape(-1, order='F').astype(np.uint8))).to(dev)
    st = dp.device_qc_stats(vol, lab, image.dtype, n_class, torch.cuda.current_stream(dev).cuda_stream, min_size=min_size)
    torch.cuda.synchronize()
    return st


def _assert_equal(image, seg, n_class=3, min_size=None):
    got = _device_stats(image, seg, n_class, min_size)
    want = aorta_qc.stats_host(image, seg, n_class)
    if min_size is not None:
        want['n_large'] = aorta_qc.count_large_components(seg, n_class, min_size)
    assert got['n_large'].tolist() == want['n_large'].tolist()
    assert np.array_equal(got['max'], want['max'], equal_nan=True)
    assert got['mean_ed'].dtype == want['mean_ed'].dtype and got['mean_ed'].tobytes() == want['mean_ed'].tobytes()
    return got


def _blobs(shape, seed):
    """Aorta-like labels: a disc per class per frame plus speckle (small and large components, some frames fragmented)."""
    rng = np.random.default_rng(seed)
    X, Y, Z, T = shape
    seg = np.zeros(shape, np.int32)
    xx, yy = np.meshgrid(np.arange(X), np.arange(Y), indexing='ij')
    for t in range(T):
        for k, (cx, cy) in ((1, (0.35 * X, 0.4 * Y)), (2, (0.65 * X, 0.6 * Y))):
            r = rng.uniform(0.05, 0.12) * min(X, Y) + 1
            for z in range(Z):
                seg[..., z, t][(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = k
        speck = rng.random((X, Y, Z)) < 0.02
        seg[..., t][speck] = rng.integers(0, 3, size=int(speck.sum()))
        if t % 3 == 1:                                   # a second large piece of class 2
            seg[1:6, 1:5, 0, t] = 2
    return seg


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', [(240, 196, 1, 100), (37, 29, 1, 7), (65, 33, 1, 3), (33, 45, 2, 5)])
def test_device_stats_equal_host(dtype, shape):
    image = _image(shape, dtype, 3)
    seg = _blobs(shape, 4)
    got = _assert_equal(image, seg)
    assert (got['n_large'][:, 2] >= 2).any() and (got['n_large'][:, 1] == 1).any()
    if shape[2] == 1:                                    # C-ordered volume: other strides, same statistics
        _assert_equal(_image(shape, dtype, 3, order='C'), seg)


def _serpentine(X, Y):
    """One single-pixel-wide path through the whole frame: every other row, joined at alternating ends."""
    m = np.zeros((X, Y), bool)
    m[::2, :] = True
    for i, x in enumerate(range(1, X, 2)):
        m[x, Y - 1 if i % 2 == 0 else 0] = True
    return m


WORST = {
    'full_frame': lambda X, Y: np.ones((X, Y), np.int32),
    'serpentine': lambda X, Y: _serpentine(X, Y).astype(np.int32),
    'serpentine_diagonal': lambda X, Y: (np.add.outer(np.arange(X), np.arange(Y)) % 4 == 0).astype(np.int32) * 2,
    'checkerboard': lambda X, Y: 1 + (np.add.outer(np.arange(X), np.arange(Y)) % 2),
    'isolated_pixels': lambda X, Y: np.where((np.arange(X)[:, None] % 2 == 0) & (np.arange(Y)[None, :] % 2 == 0), 1, 2),
    'diagonal_joins': lambda X, Y: np.kron(np.eye(max(X, Y) // 4 + 1, dtype=np.int32), np.ones((4, 4), np.int32))[:X, :Y],
}


@pytest.mark.parametrize('case', sorted(WORST))
@pytest.mark.parametrize('dtype', DTYPES)
def test_worst_cases(case, dtype):
    X, Y, T = 240, 196, 4
    frame = WORST[case](X, Y)
    seg = np.repeat(frame[:, :, None, None], T, axis=3).astype(np.int32)
    seg[..., 1] = np.flip(seg[..., 1], axis=(0, 1))
    seg[..., 2] = (seg[..., 2] != 0) * (3 - seg[..., 2])     # swap classes 1 and 2
    image = _image(seg.shape, dtype, 5)
    for min_size in (None, 0):                            # 0: every component counts (isolated pixels: the maximum count)
        got = _assert_equal(image, seg, min_size=min_size)
    if case == 'serpentine':
        assert got['n_large'][:, 1].tolist() == [1, 1, 0, 1]
    if case == 'isolated_pixels':
        assert got['n_large'][0, 1] == 120 * 98


def test_three_d_corners_and_z_edges():
    seg = np.zeros((70, 40, 3, 2), np.int32)
    seg[30:33, 28:32, 0, :] = 1                          # touches the next block only at a 3-D corner: separate
    seg[33:36, 32:36, 1, :] = 1
    seg[33, 31, 1, 1] = 1                                # frame 1: an edge neighbour across z joins them
    seg[60:62, 5:7, :, :] = 2                            # a column through all three planes: one component
    image = _image(seg.shape, np.float32, 6)
    got = _assert_equal(image, seg, min_size=0)
    assert got['n_large'][:, 1].tolist() == [2, 1] and got['n_large'][:, 2].tolist() == [1, 1]


@pytest.mark.parametrize('dtype', [np.float32, np.int16])
def test_nan_and_extremes_under_the_mask(dtype):
    seg = _blobs((50, 40, 1, 4), 7)
    image = _image(seg.shape, dtype, 8)
    if dtype == np.float32:
        image[seg == 1] = -np.inf
        x, y = np.argwhere(seg[:, :, 0, 2] == 1)[0]
        image[x, y, 0, 2] = np.nan
        image[x, y, 0, 0] = -0.0
    else:
        image[seg == 2] = np.iinfo(dtype).min
    got = _assert_equal(image, seg)
    if dtype == np.float32:
        assert np.isnan(got['max'][2, 1]) and got['max'][1, 1] == -np.inf


def test_mean_of_large_masks_follows_numpys_buffers():
    seg = np.zeros((240, 196, 1, 2), np.int32)
    seg[:200, :150, 0, :] = 1                            # 30000 voxels: four 8192-element buffers of numpy's reduction
    seg[200:, :, 0, :] = 2
    for dtype in DTYPES:
        _assert_equal(_image(seg.shape, dtype, 9), seg)


# ---- aux['qc'] and aux['counts'] of the sequence function: both forwards --------------------------------------------------
@pytest.mark.parametrize('name', ['UNet_ao', 'UNet-LSTM_ao'])
def test_sequence_device_qc_and_counts_equal_host(name):
    from test_integer_volumes_gpu import _engine, _mr_like
    eng = _engine(name)
    try:
        vol = _mr_like((64, 48, 2, 11), np.int16, 5)
        pred, aux = dp.aortic_sequence_device(vol, eng, window=None if name == 'UNet_ao' else (5, 0.1, 1), return_aux=True, qc=True)
    finally:
        eng.close()
    got, want = aux['qc'], aorta_qc.stats_host(vol, pred)
    assert got['n_large'].tolist() == want['n_large'].tolist()
    assert np.array_equal(got['max'], want['max'], equal_nan=True)
    assert got['mean_ed'].dtype == want['mean_ed'].dtype and got['mean_ed'].tobytes() == want['mean_ed'].tobytes()
    counts = np.stack([[np.sum(pred[..., t] == c) for c in range(3)] for t in range(vol.shape[3])])
    np.testing.assert_array_equal(aux['counts'], counts)
    assert len(np.unique(pred)) > 1


# ---- deploy_network_ao.py --aortic_qc_full: device path == host path --------------------------------------------------
QC_LINE = re.compile(r'^(The area of|The image becomes|The segmentation has|There is)')


@pytest.mark.parametrize('model,name', [('UNet', 'UNet_ao'), ('UNet-LSTM', 'UNet-LSTM_ao')])
def test_deploy_device_and_host_paths_agree(tmp_path, capsys, model, name):
    import shutil
    from ukbb_cardiac_amd import deploy_network_ao, nifti
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.phantom import cine_phantom
    from ukbb_cardiac_amd.weights import save_blob, synthetic_params
    arch = MODELS[name]
    mp = str(tmp_path / name)
    save_blob(mp + '.ukbbw', arch, synthetic_params(arch, 1234))
    src = tmp_path / 'src'
    names = ['4001', '4002', '4003']
    for i, nm in enumerate(names):
        (src / nm).mkdir(parents=True)
        cine = np.round(cine_phantom(10, 96, 80, seed=90 + i)[..., 0].transpose(1, 2, 0)[:, :, None, :] * 1000.0).astype(np.float32)
        if i == 2:
            cine[..., 4] *= 8.0                          # a noisy frame
        nifti.save(cine, str(src / nm / 'ao.nii.gz'), np.diag([1.6, 1.6, 6.0, 1.0]), np.array([1, 1.6, 1.6, 6.0, 0.01, 0, 0, 0], np.float32))
    out = {}
    for mode in ('device', 'host'):
        work = tmp_path / mode
        shutil.copytree(str(src), str(work))
        csv = str(tmp_path / (mode + '.csv'))
        capsys.readouterr()
        deploy_network_ao.main(['--data_dir', str(work), '--model_path', mp, '--model', model, '--output_csv', csv, '--aortic_qc_full',
                                '--io_threads', '0'] + (['--nodevice_preproc'] if mode == 'host' else []))
        lines = [l for l in capsys.readouterr().out.splitlines() if QC_LINE.match(l) or l in names]
        out[mode] = (open(csv).read(), lines)
    assert out['device'] == out['host']
    assert sum(1 for l in out['device'][1] if l in names) == 3
