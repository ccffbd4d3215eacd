"""ukbb_fcn_atrial_area_length on the GPU equals atrial.frame_stats_host in every one of its 8 columns -- phantom atria around the
32x32 tile of the labeller, planes one voxel wide, an axis-aligned grid full of exact ties, the constructed statuses and clip
branches, carved buffers -- and deploy_network.py --atrial_csv writes the same bytes on the device paths as on the host path."""
import os

import numpy as np
import pytest

import test_atrial as TA
from ukbb_cardiac_amd import atrial
from ukbb_cardiac_amd import device_pipeline as dp

pytestmark = pytest.mark.gpu


def _lab_tensor(planes):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(planes).reshape(-1, order='F').astype(np.uint8))).cuda()


def _device(planes, n_class, affine, long_axis):
    import torch
    X, Y, P = planes.shape
    return dp.device_atrial_stats(_lab_tensor(planes), (X, Y, 1, P), n_class, affine, long_axis, torch.cuda.current_stream().cuda_stream)


def _assert_equal(planes, n_class, g):
    affine, long_axis = TA.geometry(g)
    got = _device(planes, n_class, affine, long_axis)
    want = atrial.frame_stats_host(planes, n_class, affine, long_axis)
    assert got.dtype == np.int32 and got.shape == want.shape == (planes.shape[2], n_class, 8)
    assert np.array_equal(got, want), (g, np.argwhere(got != want)[:8], got[got != want][:8], want[got != want][:8])
    return got


def _atria(shape, n_class, seed):
    """Per plane and class an atrium-like blob where the plane has room for one (runs of labels on a plane one voxel wide), and
    2 % speckle of every label."""
    rng = np.random.default_rng(seed)
    X, Y, P = shape
    seg = np.zeros(shape, np.int32)
    for p in range(P):
        if min(X, Y) >= 16:
            for k in range(1, n_class):
                blob = TA.phantom_atrium(X, Y, seed + 10 * p + k, k, (0.3 + 0.35 * (k - 1) + 0.05 * p, 0.35 + 0.3 * (k - 1)), 0.8)
                seg[..., p] = np.where(blob != 0, blob, seg[..., p])
        else:
            line = seg[..., p].reshape(-1)
            for k in range(1, n_class):
                for _ in range(2):
                    a = int(rng.integers(0, line.size - 4))
                    line[a:a + int(rng.integers(1, 14))] = k
        sp = rng.random((X, Y)) < 0.02
        seg[..., p][sp] = rng.integers(0, n_class, size=int(sp.sum()))
    return seg


@pytest.mark.parametrize('n_class', [2, 3])
@pytest.mark.parametrize('shape', [(40, 56, 4), (57, 33, 5), (1, 64, 2), (64, 1, 2), (208, 176, 3)])
def test_device_stats_equal_host(shape, n_class):
    seg = _atria(shape, n_class, sum(shape) + n_class)
    got = _assert_equal(seg, n_class, sum(shape) % 3)                   # an oblique affine
    _assert_equal(seg, n_class, -1)                                     # the axis-aligned one: d takes few values, ties abound
    if min(shape[:2]) >= 16:
        assert (got[:, 1:, 1] == atrial.MEASURED).all() and (got[:, 1:, 6] > 3).all() and (got[:, 1:, 0] > 30).all()


def _serpentine(X, Y):
    m = np.zeros((X, Y), bool)
    m[::2, :] = True
    for i, x in enumerate(range(1, X, 2)):
        m[x, Y - 1 if i % 2 == 0 else 0] = True
    return m.astype(np.int32)


def _tie(X, Y):
    """Two class-1 components of 12 voxels in different tiles: the one first in C order (small x, large y) is last in the kernels'
    own NIfTI order."""
    f = np.zeros((X, Y), np.int32)
    f[1:4, Y - 6:Y - 2] = 1
    f[X - 5:X - 1, 1:4] = 1
    return f


def _few(X, Y, n):
    f = np.zeros((X, Y), np.int32)
    f[X // 2, 5:5 + n] = 1
    return f


def _border(X, Y, side):
    f = np.zeros((X, Y), np.int32)
    if side == 'x0':
        f[0:6, 8:Y - 8] = 1
    elif side == 'x1':
        f[X - 6:X, 8:Y - 8] = 1
    elif side == 'y0':
        f[8:X - 8, 0:6] = 1
    elif side == 'y1':
        f[8:X - 8, Y - 6:Y] = 1
    else:                                              # a blob cut by a corner
        cx, cy = {'c00': (2, 3), 'c01': (3, Y - 3), 'c10': (X - 3, 2), 'c11': (X - 2, Y - 4)}[side]
        f[TA.ellipse(X, Y, cx, cy, 13.0, 9.0, 0.7)] = 1
    return f


CX, CY = 40, 56
CONSTRUCTED = {
    'tie': lambda: _tie(CX, CY),
    'one_voxel': lambda: _few(CX, CY, 1),
    'two_voxels': lambda: _few(CX, CY, 2),
    'three_voxels': lambda: _few(CX, CY, 3),
    'full_plane': lambda: np.ones((CX, CY), np.int32),
    'serpentine': lambda: _serpentine(CX, CY),
    'absent': lambda: np.where(TA.ellipse(CX, CY, 20, 30, 9, 12, 0.3), 2, 0).astype(np.int32),
}
CONSTRUCTED.update({'border_' + s: (lambda s=s: _border(CX, CY, s)) for s in ('x0', 'x1', 'y0', 'y1', 'c00', 'c01', 'c10', 'c11')})


def test_constructed_planes():
    names = sorted(CONSTRUCTED)
    planes = np.stack([CONSTRUCTED[n]() for n in names], axis=2)
    codes = 0
    for g in (0, 1, 2, -1):
        got = _assert_equal(planes, 3, g)
        row = {n: got[i] for i, n in enumerate(names)}
        assert list(row['tie'][1, :2]) == [12, atrial.MEASURED] and row['tie'][1, 2] < 4          # the component first in C order
        assert list(row['one_voxel'][1]) == [1, atrial.NO_AXIS, 0, 0, 0, 0, 0, 0]
        assert list(row['two_voxels'][1]) == [2, atrial.NO_AXIS, 0, 0, 0, 0, 0, 0]
        assert row['three_voxels'][1, 0] == 3 and row['three_voxels'][1, 1] in (atrial.MEASURED, atrial.NO_HIT)
        assert row['full_plane'][1, 0] == CX * CY and row['full_plane'][1, 1] == atrial.MEASURED
        assert row['serpentine'][1, 0] == _serpentine(CX, CY).sum()
        assert not row['absent'][1].any() and row['absent'][2, 1] == atrial.MEASURED and not got[:, 0].any()
        # which sides of the image the clip moved an end point to, over the border planes
        affine, long_axis = TA.geometry(g)
        for n in names:
            if n.startswith('border_'):
                px, py, qx, qy = atrial.cell_detail(CONSTRUCTED[n](), 1, affine, long_axis)[1]['ends']
                for cvx, cvy in ((int(qy), int(qx)), (int(py), int(px))):
                    codes |= (cvx < 0) + 2 * (cvx > CY - 1) + 4 * (cvy < 0) + 8 * (cvy > CX - 1)
    assert codes == 15                                 # every clip branch ran


def test_crescent_is_missed_by_its_axis_line():
    c = TA.crescent()
    got = _assert_equal(np.stack([c, np.zeros_like(c), c], axis=2), 2, 0)
    assert list(got[0, 1]) == [int(c.sum()), atrial.NO_HIT, 0, 0, 0, 0, 0, 0] and not got[1].any()


def _call(lab_ptr, X, Y, P, n_class, affine, long_axis, work_ptr, out_ptr, stream=0):
    import ctypes as C
    from ukbb_cardiac_amd import _lib
    a = None if affine is None else (C.c_double * 12)(*np.asarray(affine, np.float64)[:3].ravel())
    l = None if long_axis is None else (C.c_double * 3)(*np.asarray(long_axis, np.float64))
    return _lib.lib.ukbb_fcn_atrial_area_length(lab_ptr, X, Y, P, n_class, a, l, work_ptr, out_ptr, stream)


def test_carved_buffers():
    """Labels, work buffer and output inside larger poisoned allocations: the labels stay, nothing beside the work buffer or the
    output changes, every output cell is written (two sentinels), the results are the host's."""
    import torch
    from test_device_memory_gpu import SENTINELS, Carved
    X, Y, P, n_class = 37, 45, 3, 3
    seg = _atria((X, Y, P), n_class, 11).astype(np.uint8)
    affine, long_axis = TA.geometry(1)
    want = atrial.frame_stats_host(seg, n_class, affine, long_axis)
    n = X * Y * P
    n_work, n_out = dp.AtrialStats().sizes((X, Y, 1, P), n_class)
    assert n_work == 2 * P * n_class + 3 * n + (n + 3) // 4 and n_out == P * n_class * 8
    results = []
    for s in SENTINELS:
        labels = Carved(n, 0x01, np.asfortranarray(seg))                        # a label read from beside the planes would count
        work = Carved(4 * n_work, s)
        out = Carved(4 * n_out, s)
        assert work.ptr % 8 == 0
        assert _call(labels.ptr, X, Y, P, n_class, affine, long_axis, work.ptr, out.ptr, torch.cuda.current_stream().cuda_stream) == 0
        results.append(out.read('output').view(np.int32).reshape(P, n_class, 8).copy())
        work.read('work buffer')
        labels.untouched('the labels')
    assert np.array_equal(results[0], want) and np.array_equal(results[1], want)


def test_repeat_run_gives_identical_bits():
    import torch
    seg = _atria((57, 33, 5), 3, 4)
    affine, long_axis = TA.geometry(2)
    lab = _lab_tensor(seg)
    n_work, n_out = dp.AtrialStats().sizes((57, 33, 1, 5), 3)
    work = torch.empty(n_work, dtype=torch.int32, device='cuda')
    outs = [torch.empty(n_out, dtype=torch.int32, device='cuda') for _ in range(2)]
    stream = torch.cuda.current_stream().cuda_stream
    for o in outs:                                     # the same work buffer, dirty from the first call
        dp.AtrialStats().launch(lab.data_ptr(), (57, 33, 1, 5), 3, work.data_ptr(), o.data_ptr(), stream, (affine, long_axis))
    a, b = (o.cpu().numpy() for o in outs)
    assert np.array_equal(a, b) and np.array_equal(a.reshape(5, 3, 8), atrial.frame_stats_host(seg, 3, affine, long_axis))


def test_bad_arguments_are_refused():
    import torch
    from ukbb_cardiac_amd import _lib
    affine, long_axis = TA.geometry(0)
    lab = _lab_tensor(np.ones((8, 8, 1), np.uint8))
    work = torch.empty(1024, dtype=torch.int32, device='cuda')
    out = torch.empty(64, dtype=torch.int32, device='cuda')
    nan_affine = affine.copy()
    nan_affine[1, 3] = np.nan
    good = dict(lab=lab.data_ptr(), X=8, Y=8, P=1, n_class=3, affine=affine, long_axis=long_axis, work=work.data_ptr(), out=out.data_ptr())
    for bad in (dict(lab=None), dict(work=None), dict(out=None), dict(affine=None), dict(long_axis=None), dict(X=0), dict(Y=-1), dict(P=0),
                dict(P=65536), dict(n_class=0), dict(n_class=17), dict(X=1 << 15, Y=1 << 15), dict(work=work.data_ptr() + 4),
                dict(affine=nan_affine), dict(long_axis=np.array([0.0, np.inf, 1.0]))):
        g = dict(good, **bad)
        rc = _call(g['lab'], g['X'], g['Y'], g['P'], g['n_class'], g['affine'], g['long_axis'], g['work'], g['out'])
        assert rc == -1 and 'atrial_area_length: bad argument' in _lib.last_error(), bad        # UKBB_EINVAL
    got = _assert_equal(np.ones((8, 8, 1), np.int32), 3, 0)                    # the library still works
    assert got[0, 1, 0] == 64 and got[0, 1, 1] == atrial.MEASURED


# ---- deploy_network.py --atrial_csv: device paths == host path; eval_atrial_volume over the files == the --frames route ----------
def test_deploy_and_eval_agree(tmp_path, capsys):
    from ukbb_cardiac_amd import deploy_network, eval_atrial_volume, nifti
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.phantom import cine_phantom
    from ukbb_cardiac_amd.weights import save_blob, synthetic_params
    data = tmp_path / 'data'
    names = ['6001', '6002']
    X, Y, T = 48, 40, 4
    for i, nm in enumerate(names):
        (data / nm).mkdir(parents=True)
        nifti.save(np.zeros((4, 4, 2, 1), np.float32), str(data / nm / 'sa.nii.gz'), TA.AFFINES[i][1], np.array([1, 1.8, 1.8, 10, 0.03, 0, 0, 0], np.float32))
    frames = {}
    for j, seq in enumerate(('la_2ch', 'la_4ch')):
        arch = MODELS['FCN_' + seq]
        mp = str(tmp_path / ('FCN_' + seq))
        save_blob(mp + '.ukbbw', arch, synthetic_params(arch, 1234))
        for i, nm in enumerate(names):
            cine = np.round(cine_phantom(T, X, Y, seed=80 + 2 * j + i)[..., 0].reshape(T, 1, X, Y).transpose(2, 3, 1, 0) * 1000.0).astype(np.float32)
            nifti.save(cine, str(data / nm / (seq + '.nii.gz')), TA.AFFINES[(i + j) % 3][0], TA.PIXDIM)
        out = {}
        # --nosave_seg first, so that every mode segments; the last run leaves the label files for eval_atrial_volume
        for mode, extra in (('pipelined', ['--nosave_seg']), ('device', ['--nosave_seg', '--io_threads', '0']),
                            ('host', ['--io_threads', '0', '--nodevice_preproc'])):
            csv = str(tmp_path / ('%s_%s.csv' % (seq, mode)))
            deploy_network.main(['--seq_name', seq, '--data_dir', str(data), '--model_path', mp, '--atrial_csv', csv] + extra)
            out[mode] = open(csv).read()
        assert out['pipelined'] == out['device'] == out['host']
        rows = out['host'].splitlines()
        assert rows[0] == ',' + ','.join(atrial.FRAME_COLUMNS) and len(rows) - 1 == len(names) * T * (arch.n_class - 1)
        frames[seq] = str(tmp_path / ('%s_host.csv' % seq))
        # the labels the run saved, measured again from the files: the same rows
        again = str(tmp_path / (seq + '_again.csv'))
        deploy_network.main(['--seq_name', seq, '--data_dir', str(data), '--model_path', mp, '--atrial_csv', again])
        assert open(again).read() == out['host']
    capsys.readouterr()
    tables = {}
    for mode, args in (('device', ['--data_dir', str(data)]), ('host', ['--data_dir', str(data), '--host']),
                       ('frames', ['--frames_2ch', frames['la_2ch'], '--frames_4ch', frames['la_4ch']])):
        path = str(tmp_path / ('table_%s.csv' % mode))
        eval_atrial_volume.main(args + ['--output_csv', path])
        tables[mode] = open(path).read()
    assert tables['device'] == tables['host'] == tables['frames']
    assert tables['host'].splitlines()[0] == ',' + ','.join(atrial.ATRIAL_COLUMNS)
    assert set(capsys.readouterr().out.splitlines()) >= set(names)
