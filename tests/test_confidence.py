"""confidence (per-frame reductions of the softmax behind a label map): the vectorised twin against a plain per-voxel loop and against
hand-made voxels, the table against pandas, the flags, and the host path of both deploy scripts."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import confidence_fixtures as F
from ukbb_cardiac_amd import confidence, deploy_network, deploy_network_ao, nifti, pipeline
from ukbb_cardiac_amd.label_tables import AorticTable, LabelTables

SHAPE, PAD = (5, 7, 2, 3), (8, 9, 2, 1)                   # (X, Y, Z, T) inside (X2, Y2) at (x_pre, y_pre)


@pytest.mark.parametrize('C', [2, 3, 4, 6])
def test_twin_equals_the_per_voxel_loop(C):
    X, Y, Z, T = SHAPE
    prob, pred = F.softmax_batch(Z * T, PAD[0], PAD[1], C, seed=C)
    prob, pred = F.spoil_padding(prob, pred, SHAPE, PAD)
    pred[1, 3, 3] = C                                      # labels the model does not have: soft count only
    pred[2, 4, 5] = -1
    want = F.loop_cells(prob, pred, SHAPE, PAD)
    got = confidence.cells_host(prob, pred, SHAPE, PAD)
    assert got.dtype == np.uint64 and got.shape == (T, C, 20) and np.array_equal(got, want)
    assert want[:, :, 0].sum() == Z * T * X * Y - 2 and want[:, :, 3:19].sum() == want[:, :, 0].sum()
    # chunks whose edges fall inside frames add up to the same cells, in any order
    cells = confidence.new_cells(T, C)
    for first in (4, 0):
        m = min(4, Z * T - first)
        confidence.cells_host(prob[first:first + m], pred[first:first + m], SHAPE, PAD, first, cells)
    assert np.array_equal(cells, want)
    acc = confidence.HostCells(SHAPE, PAD, C)
    for first, m in ((0, 1), (1, 4), (5, 1)):
        acc.add(prob[first:first + m], pred[first:first + m])
    assert np.array_equal(acc.cells, want)
    # the cropped volumes of the aortic host path give the same
    vol_p = prob[:, 2:7, 1:8].reshape(T, Z, X, Y, C).transpose(2, 3, 1, 0, 4)
    vol_l = pred[:, 2:7, 1:8].reshape(T, Z, X, Y).transpose(2, 3, 1, 0)
    assert np.array_equal(confidence.cells_from_volume(vol_p, vol_l), want)


def test_hand_made_voxels():
    X, Y, Z, T, C = 2, 24, 1, 2, 3
    prob = np.zeros((2, X, Y, C), np.float32)
    prob[..., 0] = 1.0                                     # background everywhere: label 0, q1 = margin = 65536
    pred = np.zeros((2, X, Y), np.int32)
    planted = F.plant_edges(prob, pred, 0, [(1, 2 + k) for k in range(F.N_EDGES)])
    assert [p[1:] for p in planted[:4]] == [(1, 65536, 65536), (0, 65536, 65536), (0, 32768, 0), (1, 49152, 32768)]
    assert planted[4][2] == 32768 and planted[4][3] == 1   # 0.5000001 against 0.49999997: one step of 2^-16 apart after truncation
    assert [p[2] for p in planted[5:]] == [k * 4096 for k in range(1, 16)]
    got = confidence.cells_host(prob, pred, (X, Y, Z, T))
    assert np.array_equal(got, F.loop_cells(prob, pred, (X, Y, Z, T), (X, Y, 0, 0)))
    rest = X * Y - len(planted)                            # untouched background voxels of frame 0
    lab1 = [p for p in planted if p[1] == 1]
    assert list(got[0, 1, :3]) == [len(lab1), sum(p[2] for p in lab1), sum(p[3] for p in lab1)]
    hist1 = [0] * 16
    for p in lab1:
        hist1[min(p[2] >> 12, 15)] += 1
    assert list(got[0, 1, 3:19]) == hist1 and hist1[15] == 1 and hist1[12] == 1 and hist1[8] == 1
    lab0 = [p for p in planted if p[1] == 0]
    hist0 = [0] * 16
    for p in lab0:
        hist0[min(p[2] >> 12, 15)] += 1
    hist0[15] += rest
    assert list(got[0, 0, 3:19]) == hist0 and hist0[1:15] == [1] * 7 + [2] + [1] * 6      # k/16 opens bin k; 0.5 twice
    assert got[0, 0, 0] == len(lab0) + rest and got[0, 0, 2] == 65536 * (rest + 1) + sum(k * 4096 for k in range(1, 16))
    # a class absent in a frame: an empty cell but for the soft count; frame 1 holds background only
    assert not got[:, 2, :19].any() and got[0, 2, 19] == 0 and list(got[1, 1]) == [0] * 20
    assert list(got[1, 0]) == [X * Y, 65536 * X * Y, 65536 * X * Y] + [0] * 15 + [X * Y, 65536 * X * Y]
    # a NaN probability (a cine frame no window reaches: 0 / 0) counts as 0, its argmax is 0
    prob[1] = np.nan
    got = confidence.cells_host(prob, pred, (X, Y, Z, T))
    assert list(got[1, 0]) == [X * Y, 0, 0, X * Y] + [0] * 16 and not got[1, 1:].any()
    assert np.array_equal(got, F.loop_cells(prob, pred, (X, Y, Z, T), (X, Y, 0, 0)))


def test_sums_beyond_32_bits():
    X, Y, Z, T = 200, 208, 2, 1
    prob = np.zeros((Z, X, Y, 2), np.float32)
    prob[..., 1] = 1.0
    got = confidence.cells_host(prob, np.ones((Z, X, Y), np.int32), (X, Y, Z, T))
    n = X * Y * Z
    assert 65536 * n > 1 << 32
    assert list(got[0, 1]) == [n, 65536 * n, 65536 * n] + [0] * 15 + [n, 65536 * n] and not got[0, 0].any()


def test_refused_inputs():
    prob, pred = F.softmax_batch(6, 8, 9, 3, seed=1)
    with pytest.raises(TypeError, match='float32'):
        confidence.cells_host(prob.astype(np.float64), pred, SHAPE, PAD)
    with pytest.raises(ValueError, match='lie outside the batch'):
        confidence.cells_host(prob, pred, SHAPE, PAD, first_slice=1)
    with pytest.raises(ValueError, match='expected prob'):
        confidence.cells_host(prob, pred[:, :7], SHAPE, PAD)
    with pytest.raises(ValueError, match='image region'):
        confidence.cells_host(prob, pred, SHAPE, (8, 9, 4, 1))
    with pytest.raises(ValueError, match='uint64'):
        confidence.frame_rows(np.zeros((2, 3, 20), np.int64))


def _cells_for_table():
    prob, pred = F.softmax_batch(6, 8, 9, 4, seed=11, sharp=1.5)
    pred[pred == 3] = 0                                    # label 3 absent everywhere, label 2 absent in frame 1
    pred[2:4][pred[2:4] == 2] = 0
    return confidence.cells_host(prob, pred, SHAPE, PAD)


def test_rows_and_csv_text_against_pandas(tmp_path):
    pd = pytest.importorskip('pandas')
    cells = _cells_for_table()
    rows = confidence.frame_rows(cells)
    T, C = cells.shape[:2]
    assert len(rows) == (T + 1) * (C - 1) and [r[0] for r in rows[-3:]] == ['all'] * 3 and [r[:2] for r in rows[:4]] == [[0, 1], [0, 2], [0, 3], [1, 1]]
    # every number from the integers, in float64
    t, c = 2, 1
    cell = [int(v) for v in cells[t, c]]
    assert cell[0] > 0 and rows[t * 3][2:] == [cell[0], cell[1] / (65536 * cell[0]), cell[2] / (65536 * cell[0]), sum(cell[3:11]) / cell[0],
                                              sum(cell[3:15]) / cell[0], cell[19] / 65536]
    assert 0 < rows[t * 3][4] <= rows[t * 3][3] <= 1 and 0 <= rows[t * 3][5] <= rows[t * 3][6] <= 1
    total = cells.sum(axis=0)
    assert rows[-3][2] == int(total[1, 0]) and rows[-3][3] == int(total[1, 1]) / (65536 * int(total[1, 0]))
    absent = rows[1 * 3 + 1]                               # frame 1, label 2: empty cells but the count and the soft volume
    assert absent[:3] == [1, 2, 0] and all(v != v for v in absent[3:7]) and absent[7] == int(cells[1, 2, 19]) / 65536 > 0
    path = str(tmp_path / 'conf.csv')
    confidence.write_csv(path, [('s1', r) for r in rows] + [('s2', r) for r in rows[:2]])
    df = pd.DataFrame(rows + rows[:2], index=['s1'] * len(rows) + ['s2'] * 2, columns=confidence.CONF_COLUMNS)
    assert df['n'].dtype == np.int64 and df['mean_conf'].dtype == np.float64 and df['frame'].dtype == object
    df.to_csv(str(tmp_path / 'pandas.csv'))
    text = open(path, newline='').read()
    assert text == open(str(tmp_path / 'pandas.csv'), newline='').read()
    assert text.splitlines()[0] == ',frame,label,n,mean_conf,mean_margin,frac_below_0.5,frac_below_0.75,soft_n'
    assert ',1,2,0,,,,,' in text and 's1,all,1,' in text


def flags(**kw):
    base = dict(seq_name='sa', seg4=False, process_seq=True, data_dir='.', shard_index=0, num_shards=1, batch_slices=7)
    base.update(kw)
    return SimpleNamespace(**base)


def test_flag_validation():
    with pytest.raises(ValueError, match='--confidence_csv .* needs sequence mode'):
        LabelTables(flags(confidence_csv='a.csv', process_seq=False))
    with pytest.raises(ValueError, match='--confidence_csv .* needs sequence mode'):
        AorticTable(flags(confidence_csv='a.csv', process_seq=False))
    assert LabelTables(flags(confidence_csv='a.csv')).confidence == {} and AorticTable(flags(confidence_csv='a.csv')).confidence == {}
    assert LabelTables(flags()).confidence is None and AorticTable(flags()).confidence is None
    for script in (deploy_network, deploy_network_ao):
        with pytest.raises(script.FlagError):
            script.define_flags().parse(['--confidence_cvs', 'x'])
        assert script.define_flags().parse([])[0].confidence_csv == ''
        assert script.define_flags().parse(['--confidence_csv', 'c.csv'])[0].confidence_csv == 'c.csv'
    # ED / ES mode is refused by the run itself, before it looks at a subject
    FLAGS, _ = deploy_network.define_flags().parse(['--noprocess_seq', '--confidence_csv', 'c.csv', '--data_dir', '.'])
    with pytest.raises(ValueError, match='needs sequence mode'):
        deploy_network.run(FLAGS, lambda b: None)
    FLAGS, _ = deploy_network_ao.define_flags().parse(['--noprocess_seq', '--model', 'UNet', '--confidence_csv', 'c.csv', '--data_dir', '.'])
    with pytest.raises(ValueError, match='needs sequence mode'):
        deploy_network_ao.run(FLAGS, lambda b: None)


def test_statistics_hold_the_confidence_only_with_the_flag():
    from ukbb_cardiac_amd import device_pipeline
    assert LabelTables(flags()).statistics() == []
    assert not any(isinstance(s, device_pipeline.ConfidenceStats) for s in LabelTables(flags(qc_csv='q.csv')).statistics())
    engine = SimpleNamespace(arch=SimpleNamespace(n_class=4), device=0)
    stats = LabelTables(flags(confidence_csv='a.csv', qc_csv='q.csv'), engine).statistics()
    assert [s.key for s in stats] == ['qc', 'confidence'] and [s.per_chunk for s in stats] == [False, True]
    conf = stats[1]
    # one chunk of probabilities, never the subject's: 7 slices of 208 x 208 x 4 floats; 160 bytes per (frame, class)
    assert conf.sizes((200, 208, 10, 50), 16) == (7 * 208 * 208 * 4, 50 * 4 * 40)
    assert conf.sizes((200, 208, 1, 3), 16) == (3 * 208 * 208 * 4, 3 * 4 * 40)
    with pytest.raises(RuntimeError, match='launch_chunk'):
        conf.launch(0, (8, 8, 1, 1), 4, 0, 0, 0)


# ---- the host path of deploy_network.py: a stand-in forward that returns probabilities ------------------------------------------------
PIXDIM = np.array([1, 1.8, 1.8, 10, 0.03, 0, 0, 0], np.float32)


def _stand_in(C, calls):
    """forward(batch) -> prob and pred that depend on the batch's voxels only, so that any chunking gives the same maps."""
    def forward(batch):
        x = np.asarray(batch, np.float32)[..., 0]
        lg = np.stack([np.sin(x * (3.0 + c) + c) * 2.0 for c in range(C)], axis=-1).astype(np.float32)
        e = np.exp(lg - lg.max(axis=-1, keepdims=True))
        prob = (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)
        calls.append(len(x))
        return {'prob': prob, 'pred': np.argmax(prob, axis=-1).astype(np.int32)}
    return forward


def _write_subjects(root, names, shape, seed=5):
    rng = np.random.default_rng(seed)
    for nm in names:
        os.makedirs(os.path.join(root, nm))
        nifti.save(rng.uniform(10, 200, size=shape).astype(np.float32), os.path.join(root, nm, 'sa.nii.gz'), np.eye(4), PIXDIM)


def test_host_deploy_run_writes_the_table(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    shape, C = (13, 18, 2, 3), 4
    _write_subjects('data', ['s1', 's2'], shape)
    outputs = ('seg_sa.nii.gz', 'seg_sa_ED.nii.gz', 'seg_sa_ES.nii.gz', 'sa_ED.nii.gz', 'sa_ES.nii.gz')

    def files(remove):
        got = {}
        for nm in ('s1', 's2'):
            for f in outputs:
                got[nm, f] = open(os.path.join('data', nm, f), 'rb').read()
                if remove:
                    os.remove(os.path.join('data', nm, f))
        return got
    base = ['--seq_name', 'sa', '--data_dir', 'data', '--model_path', 'x', '--io_threads', '0', '--batch_slices', '4', '--output_csv', 'vol.csv']
    calls = []
    # without the flag nothing of the feature is built: a forward that returns no probabilities serves
    import ukbb_cardiac_amd.confidence as conf_mod
    monkeypatch.setattr(conf_mod, 'HostCells', None)
    FLAGS, _ = deploy_network.define_flags().parse(base)
    plain_forward = _stand_in(C, calls)
    assert deploy_network.run(FLAGS, lambda b: {'pred': plain_forward(b)['pred']}, log=lambda *a: None) == ['s1', 's2']
    monkeypatch.undo()
    monkeypatch.chdir(tmp_path)
    plain, plain_csv = files(remove=True), open('vol.csv', newline='').read()
    lines = []
    FLAGS, _ = deploy_network.define_flags().parse(base + ['--confidence_csv', 'conf.csv'])
    calls.clear()
    assert deploy_network.run(FLAGS, _stand_in(C, calls), log=lambda *a: lines.append(' '.join(str(x) for x in a))) == ['s1', 's2']
    assert calls == [4, 2, 4, 2]                           # chunk edges inside frames (Z = 2, 4 slices per call)
    assert files(remove=False) == plain and open('vol.csv', newline='').read() == plain_csv
    # the table is frame_rows(cells_host) of what the forward returns for the subject's packed batch
    want = []
    for nm in ('s1', 's2'):
        image = nifti.load(os.path.join('data', nm, 'sa.nii.gz')).get_data()
        seen = {}

        def forward(batch):
            seen['out'] = _stand_in(C, [])(batch)
            return seen['out']
        pipeline.segment_sequence(image.copy(), forward, 1000)
        X2, Y2, x_pre, _, y_pre, _ = pipeline.pad_amounts(*shape[:2])
        cells = confidence.cells_host(seen['out']['prob'], seen['out']['pred'], shape, (X2, Y2, x_pre, y_pre))
        assert np.array_equal(cells, F.loop_cells(seen['out']['prob'], seen['out']['pred'], shape, (X2, Y2, x_pre, y_pre)))
        want += [(nm, r) for r in confidence.frame_rows(cells)]
    confidence.write_csv('want.csv', want)
    text = open('conf.csv', newline='').read()
    assert text == open('want.csv', newline='').read() and len(text.splitlines()) == 1 + 2 * (3 + 1) * (C - 1)
    assert any('Confidence of 24 frames and labels written to conf.csv' in l for l in lines)
    # a forward without probabilities cannot serve the flag
    os.remove('data/s1/seg_sa.nii.gz')
    with pytest.raises(ValueError, match='has to return prob'):
        deploy_network.run(FLAGS, lambda b: {'pred': plain_forward(b)['pred']}, log=lambda *a: None)
    # a second run segments nothing: the probabilities of the earlier run are gone, said once per subject, no rows
    nifti.save(nifti.load('data/s2/seg_sa.nii.gz').get_data(), 'data/s1/seg_sa.nii.gz', np.eye(4), PIXDIM, as_dtype=np.float64)
    lines.clear()
    FLAGS.confidence_csv = 'again.csv'
    assert deploy_network.run(FLAGS, _stand_in(C, calls), log=lambda *a: lines.append(' '.join(str(x) for x in a))) == []
    assert sum('probabilities are gone' in l for l in lines) == 2
    assert open('again.csv', newline='').read() == ',' + ','.join(confidence.CONF_COLUMNS) + '\n'


def test_host_aortic_run_writes_the_table(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    shape, C = (20, 17, 1, 5), 3
    rng = np.random.default_rng(9)
    os.makedirs('data/a1')
    nifti.save(rng.uniform(10, 200, size=shape).astype(np.float32), 'data/a1/ao.nii.gz', np.eye(4), PIXDIM)
    base = ['--data_dir', 'data', '--model_path', 'x', '--model', 'UNet', '--io_threads', '0', '--batch_slices', '2', '--nodevice_preproc']
    FLAGS, _ = deploy_network_ao.define_flags().parse(base)
    assert deploy_network_ao.run(FLAGS, _stand_in(C, []), log=lambda *a: None) == ['a1']
    plain = open('data/a1/seg_ao.nii.gz', 'rb').read()
    FLAGS, _ = deploy_network_ao.define_flags().parse(base + ['--confidence_csv', 'conf.csv'])
    assert deploy_network_ao.run(FLAGS, _stand_in(C, []), log=lambda *a: None) == ['a1']
    assert open('data/a1/seg_ao.nii.gz', 'rb').read() == plain
    prob = pipeline.aortic_prob_sequence(nifti.load('data/a1/ao.nii.gz').get_data(), _stand_in(C, []), True, 1000)
    pred = np.argmax(prob, axis=-1).astype(np.int32)
    cells = confidence.cells_from_volume(prob, pred)
    X, Y, Z, T = shape
    flat_p = np.ascontiguousarray(prob.transpose(3, 2, 0, 1, 4)).reshape(T * Z, X, Y, C)
    assert np.array_equal(cells, F.loop_cells(flat_p, pred.transpose(3, 2, 0, 1).reshape(T * Z, X, Y), shape, (X, Y, 0, 0)))
    confidence.write_csv('want.csv', [('a1', r) for r in confidence.frame_rows(cells)])
    assert open('conf.csv', newline='').read() == open('want.csv', newline='').read()
