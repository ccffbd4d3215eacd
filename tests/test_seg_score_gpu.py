"""ukbb_fcn_score_planes on the GPU equals seg_score.stats_host in every int32 field and in the bits of both float64 sums -- the
constructed planes, sizes on both sides of every word and wave boundary of the bit planes, carved buffers -- and the statistic gives
the same through segment_sequence_device, SubjectPipeline and every path of deploy_network.py --score_csv."""
import os

import numpy as np
import pytest

import seg_score_fixtures as F
from test_device_memory_gpu import SENTINELS, Carved
from ukbb_cardiac_amd import device_pipeline as dp
from ukbb_cardiac_amd import seg_score

pytestmark = pytest.mark.gpu


def _bytes(planes):
    """[P, X, Y] planes -> their bytes in the layout ukbb_fcn_unpack_labels leaves behind (x fastest)."""
    return np.ascontiguousarray(np.asarray(planes, np.uint8).transpose(0, 2, 1))


def _call(pred, truth, X, Y, P, n_class, work, cells, sums):
    import torch
    from ukbb_cardiac_amd import _lib
    return _lib.lib.ukbb_fcn_score_planes(pred, truth, X, Y, P, n_class, work, cells, sums, torch.cuda.current_stream().cuda_stream)


def device_stats(pred, truth, n_class, fill):
    """The call on carved buffers filled with ``fill``: inputs unchanged, nothing written outside the two outputs."""
    from ukbb_cardiac_amd import _lib
    P, X, Y = pred.shape
    n_work = int(_lib.lib.ukbb_fcn_score_planes_work(X, Y, P, n_class))
    assert 0 < n_work <= 64 << 20
    d_pred, d_truth = Carved(P * X * Y, fill, _bytes(pred)), Carved(P * X * Y, fill, _bytes(truth))
    work, cells, sums = Carved(n_work, fill), Carved(P * n_class * 32, fill), Carved(P * n_class * 16, fill)
    assert _call(d_pred.ptr, d_truth.ptr, X, Y, P, n_class, work.ptr, cells.ptr, sums.ptr) == 0, _lib.last_error()
    got = {'cells': cells.read('cells').view(np.int32).reshape(P, n_class, 8), 'sums': sums.read('sums').view(np.float64).reshape(P, n_class, 2)}
    work.read('work')
    d_pred.untouched('pred')
    d_truth.untouched('truth')
    return got


def assert_equal(pred, truth, n_class):
    pred, truth = np.asarray(pred, np.uint8), np.asarray(truth, np.uint8)
    want = seg_score.stats_host(F.volume_from_planes(pred), F.volume_from_planes(truth), n_class)
    for fill in SENTINELS:                                 # a cell the kernel leaves unwritten cannot equal the twin under both fills
        got = device_stats(pred, truth, n_class, fill)
        bad = np.argwhere(got['cells'] != want['cells'])
        assert not len(bad), (bad[:8], got['cells'][tuple(bad[0][:2])], want['cells'][tuple(bad[0][:2])])
        assert np.array_equal(got['sums'].view(np.uint64), want['sums'].view(np.uint64)), np.argwhere(got['sums'] != want['sums'])[:8]
    return want


def labels(P, X, Y, n_levels, seed):
    """[P, X, Y] label planes 0..n_levels-1 and a second set: the first shifted, with 3 % of its pixels redrawn."""
    rng = np.random.default_rng(seed)
    if min(X, Y) >= 16:
        a = F.phantom_labels(P, X, Y, seed=seed, n_class=n_levels)
    else:
        a = rng.integers(0, n_levels, size=(P, X, Y), dtype=np.uint8)
    b = np.roll(a, (1 if X > 1 else 0, 2 if Y > 2 else 0), axis=(1, 2))
    flip = rng.random(b.shape) < 0.03
    b[flip] = rng.integers(0, n_levels, size=int(flip.sum()), dtype=np.uint8)
    return a, b


def test_constructed_planes():
    fix = F.fixtures()
    planes = np.stack([fix[n] for n in sorted(fix)]).astype(np.uint8)
    other = np.broadcast_to(F.disc(cx=14, cy=22, r2=60), planes.shape).astype(np.uint8)
    want = assert_equal(planes, other, 2)
    assert want['cells'][:, 1, 0].all() and not want['cells'][:, 0].any()
    assert_equal(other, planes, 2)
    assert_equal(planes, planes[::-1], 2)                  # fixture against fixture: ring against checkerboard, line against serpentine ...


SIZES = [(1, 1), (1, 7), (7, 1), (31, 33), (32, 32), (33, 31), (64, 64), (65, 70), (192, 208), (256, 256), (512, 512)]


@pytest.mark.parametrize('i', range(len(SIZES)), ids=['%dx%d' % s for s in SIZES])
def test_plane_sizes(i):
    X, Y = SIZES[i]
    n_class = (2, 3, 4, 6)[i % 4]
    P = 3 if X * Y <= 65 * 70 else 1
    a, b = labels(P, X, Y, n_class + 1, 100 + i)          # one label more than the call knows: ignored
    if X * Y > 1:
        assert a.max() == n_class
    want = assert_equal(a, b, n_class)
    if min(X, Y) >= 31:
        assert want['cells'][:, 1:, 0].any() and want['sums'].any()


@pytest.mark.parametrize('n_class', [2, 3, 4, 6])
def test_class_counts_and_foreign_labels(n_class):
    a, b = labels(3, 31, 33, 7, 40 + n_class)              # labels up to 6 whatever n_class is
    want = assert_equal(a, b, n_class)
    assert want['cells'][:, 1:, 0].all()


def test_empty_sides():
    a, b = labels(3, 33, 41, 3, 7)
    a[0] = 0
    b[1] = 0
    a[2] = b[2] = 0
    want = assert_equal(a, b, 3)
    assert not want['cells'][:, :, 0].any() and want['cells'][0, 1:, 2].all() and want['cells'][1, 1:, 1].all() and not want['cells'][2].any()
    assert not want['cells'][:, :, 4:].any() and not want['sums'].any()


@pytest.mark.parametrize('P', [1, 3, 1100])
def test_plane_counts(P):
    """1100 one-class planes are more cells than the launch has workgroups (1024): the rest takes the grid-stride loop."""
    a, b = labels(P, 8, 9, 2, P)
    want = assert_equal(a, b, 2)
    assert P < 1100 or want['cells'][1024:, 1, 0].sum() > 20


def test_serpentine_flood_runs_to_its_fixed_point():
    s = F.serpentine(64, 64)
    planes = np.stack([s, s.T]).astype(np.uint8)           # the corridor across the words of a row, and across the rows
    other = np.broadcast_to(F.disc(64, 64, 40, 30, 200), planes.shape).astype(np.uint8)
    want = assert_equal(planes, other, 2)
    assert want['cells'][0, 1, 4] > 64 * 64 // 2 - 200     # nearly every wall pixel borders the outer background


def test_long_contours():
    """More contour pixels than one buffer of numpy's reduction holds (8192): the sums of two and three buffers, against a short
    contour; and the checkerboard and dense noise, whose outer background stops at the rim."""
    X, Y = 192, 208
    planes = np.stack([F.stripes(X, Y), F.noise_labels((X, Y), 10, 12) < 3, F.checkerboard(X, Y), F.noise_labels((X, Y), 2, 12) == 1]).astype(np.uint8)
    other = np.broadcast_to(F.disc(X, Y, 90, 100, 900), planes.shape).astype(np.uint8)
    want = assert_equal(planes, other, 2)
    assert want['cells'][0, 1, 4] == X * Y // 2 > 2 * 8192 and want['cells'][1, 1, 4] > 8192
    assert (want['cells'][2:, 1, 4] < X * Y // 8).all()


def test_worst_case_planes_return():
    """X*Y/2 contour pixels on either side, the most a plane can have (lines of x against lines of y): the launch returns -- the
    two-phase transform has no all-pairs product -- and every field is what the pattern says: a pixel of one is a pixel of the other
    or next to one."""
    import torch
    from ukbb_cardiac_amd import _lib
    X, Y = 192, 208
    a, b = F.stripes(X, Y)[None].astype(np.uint8), np.ascontiguousarray(F.stripes(Y, X).T)[None].astype(np.uint8)
    d_a, d_b = (torch.from_numpy(_bytes(v)).cuda() for v in (a, b))
    work = torch.empty(int(_lib.lib.ukbb_fcn_score_planes_work(X, Y, 1, 2)), dtype=torch.uint8, device='cuda')
    out = torch.empty(2 * 12, dtype=torch.int32, device='cuda')
    assert _call(d_a.data_ptr(), d_b.data_ptr(), X, Y, 1, 2, work.data_ptr(), out.data_ptr(), out.data_ptr() + 64) == 0
    torch.cuda.synchronize()                               # returns
    got = out.cpu().numpy()
    half, quarter = X * Y // 2, X * Y // 4
    assert list(got[8:16]) == [1, half, half, quarter, half, half, 1, 1] and not got[:8].any()
    assert list(got[16:].view(np.float64)) == [0.0, 0.0, float(quarter), float(quarter)]       # sums of 0.0 and 1.0: exact in any order
    assert seg_score.contour_mask(a[0] == 1).sum() == seg_score.contour_mask(b[0] == 1).sum() == half


def test_bad_arguments_and_too_large_planes_are_refused():
    import torch
    from ukbb_cardiac_amd import _lib
    lab = torch.zeros(64, dtype=torch.uint8, device='cuda')
    work = torch.empty(4096, dtype=torch.uint8, device='cuda')
    out = torch.empty(64, dtype=torch.int32, device='cuda')
    good = dict(a=lab.data_ptr(), b=lab.data_ptr(), X=8, Y=8, P=1, n_class=2, work=work.data_ptr(), cells=out.data_ptr(), sums=out.data_ptr() + 64)
    for bad in (dict(a=None), dict(b=None), dict(work=None), dict(cells=None), dict(sums=None), dict(X=0), dict(Y=-1), dict(P=0), dict(P=65536),
                dict(n_class=1), dict(n_class=17), dict(work=work.data_ptr() + 4), dict(sums=out.data_ptr() + 4)):
        g = dict(good, **bad)
        assert _call(g['a'], g['b'], g['X'], g['Y'], g['P'], g['n_class'], g['work'], g['cells'], g['sums']) == -1, bad      # UKBB_EINVAL
        assert 'score_planes: bad argument' in _lib.last_error(), bad
    for X, Y in ((1025, 4), (4, 1025), (520, 512), (512, 513)):
        assert _lib.lib.ukbb_fcn_score_planes_work(X, Y, 1, 2) == 0 and not dp.ScoreStats.fits((X, Y, 1, 1), 2)
        g = dict(good, X=X, Y=Y)                           # refused before any pointer is read
        assert _call(g['a'], g['b'], g['X'], g['Y'], g['P'], g['n_class'], g['work'], g['cells'], g['sums']) == -1
        assert 'does not fit the bit planes' in _lib.last_error() and '%d x %d' % (X, Y) in _lib.last_error()
    assert dp.ScoreStats.fits((512, 512, 1, 1), 4) and dp.ScoreStats.fits((1024, 256, 1, 1), 4)
    assert_equal(np.ones((1, 8, 8)), np.ones((1, 8, 8)), 2)                   # the library still works


# ---- the statistic on the sequence paths ------------------------------------------------------------------------------------------
def _subject(seed, shape=(48, 64, 3, 4)):
    from ukbb_cardiac_amd.phantom import cine_phantom
    X, Y, Z, T = shape
    v = cine_phantom(Z * T, X, Y, seed=seed)[..., 0].reshape(T, Z, X, Y).transpose(2, 3, 1, 0) * 1000.0
    return np.asfortranarray(np.round(v).astype(np.float32))


def _same(got, want):
    assert got['shape'] == want['shape'] and np.array_equal(got['cells'], want['cells'])
    assert np.array_equal(got['sums'].view(np.uint64), want['sums'].view(np.uint64))


def test_statistic_through_the_sequence_paths():
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.engine import Engine
    from ukbb_cardiac_amd.subject_pipeline import SubjectPipeline
    from ukbb_cardiac_amd.weights import synthetic_params
    arch = MODELS['FCN_sa']
    vol = _subject(21)
    with Engine(arch, synthetic_params(arch, 1234), device=0) as eng:
        plain = dp.segment_sequence_device(vol, eng, batch_slices=5)
        truth = np.asfortranarray(np.roll(plain, (2, 1), axis=(0, 1)).astype(np.uint8))
        truth[..., 1] = 0                                  # an un-annotated frame
        pred, aux = dp.segment_sequence_device(vol, eng, batch_slices=5, return_aux=True, stats=[dp.ScoreStats()], stat_args={'score': truth})
        assert np.array_equal(pred, plain) and len(np.unique(pred)) >= 3
        want = seg_score.stats_host(pred, truth, arch.n_class)
        assert want['cells'][:, 1:, 0].any()
        _same(aux['stats']['score'], want)
        pipe = SubjectPipeline(eng, vol.shape, batch_slices=5, depth=3, extra_inputs=1, stats=[dp.ScoreStats()])
        pipe.submit(vol, {'score': truth})
        pipe.submit(vol, None)                             # a subject without a truth file goes without the statistic
        pipe.submit(vol, {'score': np.asfortranarray(pred.astype(np.uint8))})
        res = [pipe.collect() for _ in range(3)]
        for r in res:
            r.done()
            assert np.array_equal(r.labels, pred)
        _same(res[0].stats['score'], want)
        assert 'score' not in res[1].stats
        own = res[2].stats['score']                        # scored against itself
        assert np.array_equal(own['cells'][:, :, 1], own['cells'][:, :, 3]) and not own['cells'][:, :, 6:].any() and not own['sums'].any()
        with pytest.raises(ValueError, match='uint8 array of the shape'):
            dp.ScoreStats().launch(0, vol.shape, 4, 0, 0, 0, truth[:, :, :2])


# ---- deploy_network.py --score_against / --score_csv: every path writes one text, the stand-alone script the same --------------------
def test_deploy_and_eval_agree(tmp_path, capsys):
    from ukbb_cardiac_amd import deploy_network, eval_segmentation, nifti
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.weights import save_blob, synthetic_params
    data = tmp_path / 'data'
    names = ['7001', '7002', '7003']
    pixdim = np.array([1, 1.8, 1.8, 10, 0.03, 0, 0, 0], np.float32)
    arch = MODELS['FCN_sa']
    mp = str(tmp_path / 'FCN_sa')
    save_blob(mp + '.ukbbw', arch, synthetic_params(arch, 1234))
    for i, nm in enumerate(names):
        (data / nm).mkdir(parents=True)
        nifti.save(_subject(30 + i), str(data / nm / 'sa.nii.gz'), np.diag([1.8, 1.8, 10, 1]), pixdim)
    outputs = ('seg_sa.nii.gz', 'seg_sa_ED.nii.gz', 'seg_sa_ES.nii.gz', 'sa_ED.nii.gz', 'sa_ES.nii.gz')

    def written(remove):
        got = {}
        for nm in names:
            for f in outputs:
                path = str(data / nm / f)
                got[nm, f] = open(path, 'rb').read()
                if remove:
                    os.remove(path)
        return got
    base = ['--seq_name', 'sa', '--data_dir', str(data), '--model_path', mp, '--batch_slices', '5']
    deploy_network.main(base)
    # 7001 is scored against its own labels shifted (label 3 present, so that the script below counts the model's 4 classes), 7002 has
    # no truth file, 7003 is scored against the earlier run's own output
    seg = nifti.load(str(data / '7001' / 'seg_sa.nii.gz')).get_data()
    truth = np.roll(seg, (1, 2), axis=(0, 1)).astype(np.uint8)
    truth[0, 0, 0, 0] = 3
    truth[..., 2] = 0
    nifti.save(truth, str(data / '7001' / 'label_sa.nii.gz'), np.diag([1.8, 1.8, 10, 1]), pixdim)
    with open(str(data / '7003' / 'label_sa.nii.gz'), 'wb') as f:
        f.write(open(str(data / '7003' / 'seg_sa.nii.gz'), 'rb').read())
    plain = written(remove=True)
    out = {}
    modes = (('pipelined', []), ('device', ['--io_threads', '0']), ('inflate', ['--device_inflate', '2']), ('host', ['--io_threads', '0', '--nodevice_preproc']))
    for mode, extra in modes:
        csv = str(tmp_path / (mode + '.csv'))
        deploy_network.main(base + ['--score_against', 'label_sa', '--score_csv', csv] + extra)
        out[mode] = open(csv, newline='').read()
        assert written(remove=mode != 'host') == plain, mode                                  # the same files as without the flags
    assert out['pipelined'] == out['device'] == out['inflate'] == out['host']
    rows = [l.split(',') for l in out['host'].splitlines()]
    assert rows[0] == [''] + seg_score.SCORE_COLUMNS
    assert [r[0] for r in rows[1:]] == ['7001'] * 9 + ['7003'] * 12                           # 3 annotated frames, 4 frames; 3 labels
    assert any(r[3] not in ('', '1.0') for r in rows[1:10]) and any(float(r[5]) > 0 for r in rows[1:10] if r[5])
    own = rows[10:]
    assert all(r[3] in ('', '1.0') and r[4] in ('', '0.0') and r[5] in ('', '0.0') for r in own) and sum(r[3] == '1.0' for r in own) >= 8
    assert 'Directory {0} does not contain label_sa.nii.gz'.format(data / '7002') in capsys.readouterr().out
    # a second run segments nothing and scores the three subjects from their files; so does the stand-alone script, on either side
    again = str(tmp_path / 'again.csv')
    deploy_network.main(base + ['--score_against', 'label_sa', '--score_csv', again])
    assert open(again, newline='').read() == out['host']
    for mode, extra in (('host', ['--host']), ('device', [])):
        path = str(tmp_path / ('alone_%s.csv' % mode))
        eval_segmentation.main(['--data_dir', str(data), '--seg_name', 'seg_sa', '--truth_name', 'label_sa', '--output_csv', path, '--n_class', '4'] + extra)
        assert open(path, newline='').read() == out['host'], mode
