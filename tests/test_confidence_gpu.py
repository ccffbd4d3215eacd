"""ukbb_fcn_confidence_cells on the GPU equals confidence.cells_host in every one of the 20 integers of every cell -- padded frames whose
padding would change every field, chunk edges inside frames, every class count with its own load width, planted edge values, sums
beyond 32 bits, a single voxel -- and --confidence_csv writes one text through every path of deploy_network.py and
deploy_network_ao.py, the text of the twin applied to what Engine.run returns."""
import os
import shutil

import numpy as np
import pytest

import confidence_fixtures as F
from test_device_memory_gpu import SENTINELS, Carved
from ukbb_cardiac_amd import confidence

pytestmark = pytest.mark.gpu


def _call(prob, pred, n, shape, pad, C, first, cells):
    import torch
    from ukbb_cardiac_amd import _lib
    X, Y, Z, T = shape
    return _lib.lib.ukbb_fcn_confidence_cells(prob, pred, n, X, Y, Z, T, *pad, C, first, cells, torch.cuda.current_stream().cuda_stream)


def device_cells(prob, pred, shape, pad, chunk, fill):
    """The cells from calls of ``chunk`` slices each on carved buffers filled with ``fill``: inputs unchanged, nothing written but the cells."""
    from ukbb_cardiac_amd import _lib
    n, X2, Y2, C = prob.shape
    T = shape[3]
    d_prob, d_pred = Carved(prob.nbytes, fill, prob), Carved(pred.nbytes, fill, pred)
    d_cells = Carved(T * C * 160, fill, np.zeros(T * C * 20, np.uint64))
    for first in range(0, n, chunk):
        m = min(chunk, n - first)
        rc = _call(d_prob.ptr + first * X2 * Y2 * C * 4, d_pred.ptr + first * X2 * Y2 * 4, m, shape, pad, C, first, d_cells.ptr)
        assert rc == 0, _lib.last_error()
    got = d_cells.read('cells').view(np.uint64).reshape(T, C, 20)
    d_prob.untouched('prob')
    d_pred.untouched('pred')
    return got


def assert_equal(prob, pred, shape, pad, chunk):
    want = confidence.cells_host(prob, pred, shape, pad)
    for fill in SENTINELS:
        got = device_cells(prob, pred, shape, pad, chunk, fill)
        bad = np.argwhere(got != want)
        assert not len(bad), (bad[:8], got[tuple(bad[0][:2])], want[tuple(bad[0][:2])])
    return want


@pytest.mark.parametrize('C', [2, 3, 4, 6])
def test_padded_frames_in_chunks(C):
    """33 x 17 inside 48 x 32 at (7, 8), 3 slices x 5 frames in chunks of 4: chunk edges inside frames; the padding holds values that would
    change every field; the edge values sit in slice 5; two labels the model does not have."""
    shape, pad = (33, 17, 3, 5), (48, 32, 7, 8)
    prob, pred = F.softmax_batch(15, 48, 32, C, seed=20 + C)
    prob, pred = F.spoil_padding(prob, pred, shape, pad)
    planted = F.plant_edges(prob, pred, 5, [(7 + 4, 8 + k) for k in range(17)] + [(7 + 32, 8 + 16), (7, 8), (7 + 32, 8)])
    pred[9, 20, 20], pred[14, 39, 24] = C, -3
    want = assert_equal(prob, pred, shape, pad, 4)
    assert np.array_equal(want, F.loop_cells(prob, pred, shape, pad))
    assert want[:, :, 0].sum() == 15 * 33 * 17 - 2 and want[:, :, 0].all() and len(planted) == F.N_EDGES
    inside = confidence.cells_host(np.ascontiguousarray(prob[:, 7:40, 8:25]), np.ascontiguousarray(pred[:, 7:40, 8:25]), shape)
    assert np.array_equal(want, inside)                    # nothing of the padding in it
    whole = assert_equal(prob, pred, (48, 32, 3, 5), (48, 32, 0, 0), 15)
    assert (whole[:, :, :3] != want[:, :, :3]).all() and (whole[:, :, 19] != want[:, :, 19]).all()     # the padding would have shown


def test_several_workgroups_per_slice():
    """70 x 65 voxels per slice: two workgroups, the second partly filled; rows that do not divide the 256-voxel rounds."""
    shape, pad = (70, 65, 2, 2), (80, 80, 5, 7)
    prob, pred = F.softmax_batch(4, 80, 80, 4, seed=3, sharp=1.0)
    prob[..., 3] *= np.float32(0.01)                       # class 3 is nobody's argmax ...
    pred = np.argmax(prob, axis=-1).astype(np.int32)
    prob, pred = F.spoil_padding(prob, pred, shape, pad)
    pred[:, 30:50, 20:60] = 3                              # ... so these labels are not the argmax: negative margins, added signed
    want = assert_equal(prob, pred, shape, pad, 3)
    assert (want.view(np.int64)[:, 3, 2] < 0).all() and want[:, :, 3:19].sum() == 4 * 70 * 65


def test_sums_beyond_32_bits_and_a_single_voxel():
    X, Y, Z = 200, 208, 2
    prob = np.zeros((Z, 208, 208, 2), np.float32)
    prob[..., 1] = 1.0
    want = assert_equal(prob, np.ones((Z, 208, 208), np.int32), (X, Y, Z, 1), (208, 208, 4, 0), 2)
    n = X * Y * Z
    assert list(want[0, 1]) == [n, 65536 * n, 65536 * n] + [0] * 15 + [n, 65536 * n] and 65536 * n > 1 << 32
    prob, pred = F.softmax_batch(1, 16, 16, 3, seed=5)
    prob, pred = F.spoil_padding(prob, pred, (1, 1, 1, 1), (16, 16, 7, 7))
    want = assert_equal(prob, pred, (1, 1, 1, 1), (16, 16, 7, 7), 1)
    assert want[0, :, 0].sum() == 1 and abs(int(want[0, :, 19].sum()) - 65536) <= 4


def test_bad_arguments_are_refused():
    import torch
    from ukbb_cardiac_amd import _lib
    prob = torch.zeros(4 * 16 * 16 * 3 + 4, dtype=torch.float32, device='cuda')
    pred = torch.zeros(4 * 16 * 16, dtype=torch.int32, device='cuda')
    cells = torch.zeros(2 * 3 * 20 + 1, dtype=torch.int64, device='cuda')
    good = dict(prob=prob.data_ptr(), pred=pred.data_ptr(), n=4, shape=(10, 12, 2, 2), pad=(16, 16, 3, 2), C=3, first=0, cells=cells.data_ptr())

    def rc(**kw):
        g = dict(good, **kw)
        return _call(g['prob'], g['pred'], g['n'], g['shape'], g['pad'], g['C'], g['first'], g['cells'])
    for bad in (dict(prob=None), dict(pred=None), dict(cells=None), dict(n=0), dict(shape=(0, 12, 2, 2)), dict(shape=(10, -1, 2, 2)),
                dict(shape=(10, 12, 0, 2)), dict(shape=(10, 12, 2, 0)), dict(pad=(16, 16, -1, 2)), dict(pad=(16, 16, 7, 2)), dict(pad=(16, 13, 3, 2)),
                dict(C=1), dict(C=17), dict(prob=prob.data_ptr() + 4), dict(cells=cells.data_ptr() + 4), dict(shape=(10, 12, 256, 256), pad=(16, 16, 3, 2))):
        assert rc(**bad) == -1, bad                        # UKBB_EINVAL
        assert 'confidence_cells: bad argument' in _lib.last_error(), bad
    for bad in (dict(first=1), dict(first=-1), dict(n=5), dict(first=3, n=2)):
        assert rc(**bad) == -1, bad
        assert 'lie outside the batch of Z*T = 2 x 2 slices' in _lib.last_error(), bad
    torch.cuda.synchronize()
    assert not cells.cpu().numpy().any()                   # refused before anything was launched
    assert rc() == 0 and rc(first=2, n=2) == 0
    torch.cuda.synchronize()
    assert cells.cpu().numpy()[:120].reshape(2, 3, 20)[:, 0, 0].tolist() == [2 * 120, 4 * 120]


# ---- the statistic on the sequence paths ------------------------------------------------------------------------------------------
def _subject(seed, shape=(48, 64, 3, 4)):
    from ukbb_cardiac_amd.phantom import cine_phantom
    X, Y, Z, T = shape
    v = cine_phantom(Z * T, X, Y, seed=seed)[..., 0].reshape(T, Z, X, Y).transpose(2, 3, 1, 0) * 1000.0
    return np.asfortranarray(np.round(v).astype(np.float32))


def _cells_from_engine(eng, image, batch_slices):
    """confidence.cells_host of what Engine.run(want_prob=True) returns for the subject's packed batch, in the run's chunks."""
    from ukbb_cardiac_amd import pipeline
    outs = []

    def forward(batch):
        outs.append(eng.run(batch, want_prob=True))
        return outs[-1]
    pipeline.segment_sequence(image.copy(), forward, batch_slices)
    X2, Y2, x_pre, _, y_pre, _ = pipeline.pad_amounts(*image.shape[:2])
    prob, pred = np.concatenate([o['prob'] for o in outs]), np.concatenate([o['pred'] for o in outs])
    assert np.array_equal(pred, np.argmax(prob, axis=-1))  # the label is the lowest-index argmax of the float32 probabilities
    return confidence.cells_host(prob, pred, image.shape, (X2, Y2, x_pre, y_pre))


def test_statistic_through_the_sequence_paths():
    from ukbb_cardiac_amd import device_pipeline as dp
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.engine import Engine
    from ukbb_cardiac_amd.subject_pipeline import SubjectPipeline
    from ukbb_cardiac_amd.weights import synthetic_params
    arch = MODELS['FCN_sa']
    vol = _subject(21)
    with Engine(arch, synthetic_params(arch, 1234), device=0) as eng:
        plain = dp.segment_sequence_device(vol, eng, batch_slices=5)
        names = eng.kernel_names()                         # of the run without the statistic
        want = _cells_from_engine(eng, vol, 5)
        assert want[:, 1:, 0].any() and want[:, :, 0].sum() == vol.size
        stats = [dp.GateStats('sa', False), dp.ConfidenceStats(5, arch.n_class)]
        pred, aux = dp.segment_sequence_device(vol, eng, batch_slices=5, return_aux=True, stats=stats)
        assert np.array_equal(pred, plain) and np.array_equal(aux['stats']['confidence'], want) and 'qc' in aux['stats']
        assert np.array_equal(aux['stats']['confidence'][:, :, 0], aux['counts'])
        assert eng.kernel_names() == names and names      # the same forward: its last kernel stores the probabilities as well
        pipe = SubjectPipeline(eng, vol.shape, batch_slices=5, depth=3, extra_inputs=1, stats=stats)
        other = _subject(22)
        for v in (vol, other, vol):                        # a slot's cells are zeroed for every subject
            pipe.submit(v)
        res = [pipe.collect() for _ in range(3)]
        for r in res:
            r.done()
        assert np.array_equal(res[0].labels, pred) and np.array_equal(res[0].stats['confidence'], want)
        assert np.array_equal(res[2].stats['confidence'], want) and np.array_equal(res[1].stats['confidence'], _cells_from_engine(eng, other, 5))


# ---- deploy_network.py --confidence_csv: every path writes one text, the twin's ---------------------------------------------------
def test_deploy_paths_agree(tmp_path, capsys):
    from ukbb_cardiac_amd import deploy_network, nifti
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.engine import Engine
    from ukbb_cardiac_amd.weights import save_blob, synthetic_params
    data = tmp_path / 'data'
    names = ['7001', '7002', '7003']
    pixdim = np.array([1, 1.8, 1.8, 10, 0.03, 0, 0, 0], np.float32)
    arch = MODELS['FCN_sa']
    params = synthetic_params(arch, 1234)
    mp = str(tmp_path / 'FCN_sa')
    save_blob(mp + '.ukbbw', arch, params)
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
    tables = lambda tag: ['--output_csv', str(tmp_path / (tag + '_vol.csv')), '--qc_csv', str(tmp_path / (tag + '_qc.csv'))]
    deploy_network.main(base + tables('plain'))
    plain = written(remove=True)
    plain_tables = [open(str(tmp_path / ('plain_%s.csv' % t)), newline='').read() for t in ('vol', 'qc')]
    out = {}
    modes = (('pipelined', []), ('device', ['--io_threads', '0']), ('inflate', ['--device_inflate', '2']), ('host', ['--io_threads', '0', '--nodevice_preproc']))
    for mode, extra in modes:
        csv = str(tmp_path / (mode + '.csv'))
        deploy_network.main(base + tables(mode) + ['--confidence_csv', csv] + extra)
        out[mode] = open(csv, newline='').read()
        assert written(remove=mode != 'host') == plain, mode                                  # the same files as without the flag
        assert [open(str(tmp_path / ('%s_%s.csv' % (mode, t))), newline='').read() for t in ('vol', 'qc')] == plain_tables, mode
    assert out['pipelined'] == out['device'] == out['inflate'] == out['host']
    with Engine(arch, params, device=0) as eng:
        want = [(nm, r) for nm in names for r in confidence.frame_rows(_cells_from_engine(eng, nifti.load(str(data / nm / 'sa.nii.gz')).get_data(), 5))]
    confidence.write_csv(str(tmp_path / 'want.csv'), want)
    assert out['host'] == open(str(tmp_path / 'want.csv'), newline='').read()
    rows = [l.split(',') for l in out['host'].splitlines()]
    assert rows[0] == [''] + confidence.CONF_COLUMNS and [r[0] for r in rows[1:]] == [nm for nm in names for _ in range(15)]
    assert any(r[3] not in ('', '0') and 0 < float(r[4]) < 1 for r in rows[1:])
    # a second run segments nothing and says that the probabilities are gone
    capsys.readouterr()
    again = str(tmp_path / 'again.csv')
    deploy_network.main(base + ['--confidence_csv', again])
    assert open(again, newline='').read() == out['host'].splitlines()[0] + '\n'
    assert capsys.readouterr().out.count('probabilities are gone') == 3


# ---- deploy_network_ao.py --confidence_csv: the three models, device path and host path ----------------------------------------------
@pytest.mark.parametrize('model,name,prec', [('UNet', 'UNet_ao', 'fp32'), ('UNet', 'UNet_ao', 'bf16'), ('UNet-LSTM', 'UNet-LSTM_ao', 'fp32'),
                                             ('Temporal-UNet', 'Temporal-UNet_ao', 'fp32')])
def test_aortic_paths_agree(tmp_path, model, name, prec):
    from ukbb_cardiac_amd import deploy_network_ao, nifti, pipeline
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.engine import Engine
    from ukbb_cardiac_amd.phantom import cine_phantom
    from ukbb_cardiac_amd.weights import save_blob, synthetic_params
    arch = MODELS[name]
    params = synthetic_params(arch, 1234)
    mp = str(tmp_path / name)
    save_blob(mp + '.ukbbw', arch, params)
    src = tmp_path / 'src'
    names = ['4001']
    for i, nm in enumerate(names):
        (src / nm).mkdir(parents=True)
        cine = np.round(cine_phantom(10, 96, 80, seed=90 + i)[..., 0].transpose(1, 2, 0)[:, :, None, :] * 1000.0).astype(np.float32)
        nifti.save(cine, str(src / nm / 'ao.nii.gz'), np.diag([1.6, 1.6, 6.0, 1.0]), np.array([1, 1.6, 1.6, 6.0, 0.01, 0, 0, 0], np.float32))
    out = {}
    for mode in ('plain', 'device', 'host'):
        work = tmp_path / mode
        shutil.copytree(str(src), str(work))
        csv = str(tmp_path / (mode + '.csv'))
        deploy_network_ao.main(['--data_dir', str(work), '--model_path', mp, '--model', model, '--precision', prec, '--batch_slices', '4',
                                '--output_csv', str(tmp_path / (mode + '_area.csv')), '--io_threads', '0']
                               + ([] if mode == 'plain' else ['--confidence_csv', csv]) + (['--nodevice_preproc'] if mode == 'host' else []))
        out[mode] = ([open(str(work / nm / 'seg_ao.nii.gz'), 'rb').read() for nm in names], open(str(tmp_path / (mode + '_area.csv'))).read(),
                     None if mode == 'plain' else open(csv, newline='').read())
    assert out['device'][:2] == out['plain'][:2] == out['host'][:2]
    assert out['device'][2] == out['host'][2]
    rows = [l.split(',') for l in out['device'][2].splitlines()]
    assert rows[0] == [''] + confidence.CONF_COLUMNS and [r[0] for r in rows[1:]] == [nm for nm in names for _ in range(22)]
    assert any(int(r[3]) > 0 and 0 < float(r[4]) <= 1 for r in rows[1:])
    if model == 'UNet':                                    # the twin on what Engine.run returns for the packed batch
        with Engine(arch, params, device=0) as eng:
            eng.set_precision(prec)
            want = []
            for nm in names:
                prob = pipeline.aortic_prob_sequence(nifti.load(str(src / nm / 'ao.nii.gz')).get_data(), lambda b: eng.run(b, want_prob=True), True, 4)
                want += [(nm, r) for r in confidence.frame_rows(confidence.cells_from_volume(prob, np.argmax(prob, axis=-1)))]
        confidence.write_csv(str(tmp_path / 'want.csv'), want)
        assert out['device'][2] == open(str(tmp_path / 'want.csv'), newline='').read()
