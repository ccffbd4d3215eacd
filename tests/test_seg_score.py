"""seg_score (Dice, mean contour distance, Hausdorff distance against a second segmentation): the host twin against the reference's
own formulation fed by an independent border follower, against scipy's Euclidean transform and np_categorical_dice; the table, the
flags and the host path of deploy_network against the stand-alone script."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

from ukbb_cardiac_amd import deploy_network, eval_segmentation, image_utils, nifti, seg_score
from ukbb_cardiac_amd.label_tables import LabelTables

import seg_score_fixtures as F

FIX = F.fixtures()
OTHER = F.disc(cx=14, cy=22, r2=60)                       # what every fixture is scored against: a disc, no repeated contour pixel
PIXDIM = np.array([1, 1.8, 1.8, 10, 0.03, 0, 0, 0], np.float32)


def point_set(mask):
    return set(map(tuple, np.argwhere(mask)))


def test_contour_set_is_what_the_border_follower_visits():
    masks = dict(FIX)
    for p, plane in enumerate(F.phantom_labels(2, 48, 40)):
        for k in (1, 2, 3):
            masks['phantom%d_%d' % (p, k)] = plane == k
    masks['noise'] = F.noise_labels((21, 19), 2, 5) == 1
    for name, m in masks.items():
        assert m.any(), name
        assert set(F.followed_points(m)) == point_set(seg_score.contour_mask(m)), name
    # what the rule says about the named cases: the hole and the island are not visited, the pocket is not outer
    c = seg_score.contour_mask(FIX['ring'])
    assert not (c & F.disc(r2=64)).any() and point_set(c) == point_set(seg_score.contour_mask(F.disc(r2=144)))
    assert point_set(seg_score.contour_mask(FIX['ring_island'])) == point_set(c)
    assert not seg_score.outer_background(FIX['diagonal_pocket'])[6, 6] and seg_score.outer_background(FIX['diagonal_pocket'])[5, 5]
    assert len(F.external_contours(FIX['two_components'])) == 2 and len(F.external_contours(FIX['corner_squares'])) == 1
    c = seg_score.contour_mask(FIX['all_edges'])
    assert c[0, 10] and c[-1, 10] and c[10, 0] and c[10, -1] and not c[10, 10]
    assert seg_score.outer_background(FIX['serpentine'])[F.X0 - 2, F.Y0 // 2]        # the far end of the corridor is outer background


def test_contour_set_against_opencv():
    """Skips until OpenCV is installed: the de-duplicated points of cv2.findContours, as distance_metric calls it, against C(M)."""
    cv2 = pytest.importorskip('cv2')
    for name, m in FIX.items():
        contours = cv2.findContours(cv2.inRange(m.astype(np.uint8), 1, 1), cv2.RETR_EXTERNAL, cv2.CHAIN_APPROX_NONE)[-2]
        pts = {(int(p[0][1]), int(p[0][0])) for c in contours for p in c}          # OpenCV points are (column, row) = (y, x)
        assert pts == point_set(seg_score.contour_mask(m)), name


def test_which_fixtures_the_follower_passes_without_a_repeat():
    clean = {name for name, m in FIX.items() if len(F.followed_points(m)) == len(set(F.followed_points(m)))}
    assert clean == set(F.NO_REPEAT)
    assert len(F.followed_points(OTHER)) == len(set(F.followed_points(OTHER)))


@pytest.mark.parametrize('name', sorted(FIX))
def test_twin_equals_the_literal_distance_metric(name):
    dx = float(PIXDIM[1])
    pred, truth = F.volume_from_planes([FIX[name]]).astype(np.uint8), F.volume_from_planes([OTHER]).astype(np.uint8)
    st = seg_score.stats_host(pred, truth, 2)
    assert st['cells'][0, 1, 0] == 1 and not st['cells'][0, 0].any()
    md, hd = seg_score.slice_distances(st['cells'][0, 1], st['sums'][0, 1], dx)
    pts_a, pts_b = F.followed_points(FIX[name]), F.followed_points(OTHER)
    if name in F.NO_REPEAT:
        # the same points in the twin's order: the two means are then the same float64 additions
        want_md, want_hd = F.distance_metric_literal(sorted(pts_a), sorted(pts_b), dx)
        assert (md, hd) == (want_md, want_hd)
    else:
        want_md, want_hd = F.distance_metric_literal(pts_a, pts_b, dx)
        print('%s: md %r, with the follower\'s repeated pixels %r' % (name, md, want_md))
        assert hd == want_hd
    row = seg_score.frame_rows(st, PIXDIM)
    assert row == [[0, 1, row[0][2], float(md), float(hd), 1]]


def test_minima_equal_the_squared_euclidean_transform():
    ndi = pytest.importorskip('scipy.ndimage')
    for name, m in FIX.items():
        ca, cb = seg_score.contour_mask(m), seg_score.contour_mask(OTHER)
        for this, other in ((ca, cb), (cb, ca)):
            edt = ndi.distance_transform_edt(~other)
            want = np.rint(edt[this] ** 2).astype(np.int64)
            got = seg_score.min_sq_distances(np.argwhere(this), np.argwhere(other))
            assert got.dtype == np.int32 and np.array_equal(got, want), name


def scored_volumes():
    """(pred, truth) uint8 (40, 36, 3, 4), 4 classes: frame 1 has no truth labels, class 3 is absent from frame 2 on both sides, class 2
    is absent from the truth of frame 3's slice 0."""
    lab = F.phantom_labels(12, 40, 36, seed=11)
    pred = np.asfortranarray(np.moveaxis(lab, 0, 2).reshape(40, 36, 3, 4, order='F'))
    truth = np.asfortranarray(np.roll(pred, (2, -1), axis=(0, 1)))
    truth[:, :, :, 1] = 0
    pred[:, :, :, 2][pred[:, :, :, 2] == 3] = 0
    truth[:, :, :, 2][truth[:, :, :, 2] == 3] = 0
    truth[:, :, 0, 3][truth[:, :, 0, 3] == 2] = 0
    return pred, truth


def test_rows_dice_and_empty_cells():
    pred, truth = scored_volumes()
    st = seg_score.stats_host(pred, truth, 4)
    rows = seg_score.frame_rows(st, PIXDIM)
    assert [(r[0], r[1]) for r in rows] == [(t, k) for t in (0, 2, 3) for k in (1, 2, 3)]          # frame 1: no truth label, no rows
    for t, k, dice, md, hd, n in rows:
        with np.errstate(invalid='ignore'):
            want = image_utils.np_categorical_dice(pred[..., t], truth[..., t], k)
        if (t, k) == (2, 3):
            assert dice != dice and md != md and hd != hd and n == 0                             # 0 / 0 in the reference; None, None
        else:
            assert want.dtype == np.float32 and np.float32(dice) == want and float(np.float32(dice)) == dice
            cells = st['cells'].reshape(4, 3, 4, 8)[t, :, k]
            assert n == int(cells[:, 0].sum()) == (2 if (t, k) == (3, 2) else 3)
            per = [seg_score.slice_distances(cells[z], st['sums'].reshape(4, 3, 4, 2)[t, z, k], PIXDIM[1]) for z in range(3) if cells[z, 0]]
            assert md == np.mean([v[0] for v in per]) and hd == np.mean([v[1] for v in per])
    # labels beyond n_class are ignored; an undefined cell keeps its counts and zeroes the rest
    st3 = seg_score.stats_host(pred, truth, 3)
    assert np.array_equal(st3['cells'], st['cells'][:, :3]) and np.array_equal(st3['sums'], st['sums'][:, :3])
    one_sided = st['cells'].reshape(4, 3, 4, 8)[3, 0, 2]
    assert one_sided[0] == 0 and one_sided[1] > 0 and one_sided[2] == 0 and not one_sided[3:].any()


def test_table_text_is_what_pandas_writes(tmp_path):
    pd = pytest.importorskip('pandas')
    pred, truth = scored_volumes()
    rows = seg_score.frame_rows(seg_score.stats_host(pred, truth, 4), PIXDIM)
    path = str(tmp_path / 'score.csv')
    seg_score.write_csv(path, [('s1', r) for r in rows] + [('s2', r) for r in rows[:2]])
    df = pd.DataFrame(rows + rows[:2], index=['s1'] * len(rows) + ['s2'] * 2, columns=seg_score.SCORE_COLUMNS)
    assert df['frame'].dtype == np.int64 and df['Dice'].dtype == np.float64
    df.to_csv(str(tmp_path / 'pandas.csv'))
    assert open(path, newline='').read() == open(str(tmp_path / 'pandas.csv'), newline='').read()


def flags(**kw):
    base = dict(seq_name='sa', seg4=False, process_seq=True, data_dir='.', shard_index=0, num_shards=1)
    base.update(kw)
    return SimpleNamespace(**base)


def test_flag_validation():
    for bad in (dict(score_csv='a.csv'), dict(score_against='label_sa')):
        with pytest.raises(ValueError, match='need each other'):
            LabelTables(flags(**bad))
    with pytest.raises(ValueError, match='needs sequence mode'):
        LabelTables(flags(score_csv='a.csv', score_against='label_sa', process_seq=False))
    assert LabelTables(flags(score_csv='a.csv', score_against='label_sa')).score == {}
    assert LabelTables(flags()).score is None
    with pytest.raises(deploy_network.FlagError):
        deploy_network.define_flags().parse(['--score_cvs', 'x'])
    FLAGS, _ = deploy_network.define_flags().parse([])
    assert FLAGS.score_csv == '' and FLAGS.score_against == ''


def write_subjects(root):
    """s1: scored; s2: no truth file; s3: a truth label the pair's other file does not reach but beyond 15; s4: truth of another shape;
    s5: segmented by an earlier run, scored from its file."""
    pred, truth = scored_volumes()
    subjects = {'s1': pred, 's2': pred[::-1].copy(), 's3': pred, 's4': pred, 's5': pred[:, ::-1].copy()}
    rng = np.random.default_rng(4)
    for name, lab in subjects.items():
        d = os.path.join(root, name)
        os.makedirs(d)
        nifti.save(rng.uniform(10, 200, size=lab.shape).astype(np.float32), os.path.join(d, 'sa.nii.gz'), np.eye(4), PIXDIM)
        t = truth.copy()
        if name == 's3':
            t[3, 3, 0, 0] = 200
        if name == 's4':
            t = t[:, :, :2]
        if name != 's2':
            nifti.save(t, os.path.join(d, 'label_sa.nii.gz'), np.eye(4), PIXDIM)
        if name == 's5':
            nifti.save(lab, os.path.join(d, 'seg_sa.nii.gz'), np.eye(4), PIXDIM, as_dtype=np.float64)
    return subjects


def test_host_deploy_run_writes_the_table_of_the_stand_alone_script(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    subjects = write_subjects('data')
    state, lines = {}, []

    def log(*a):
        line = ' '.join(str(x) for x in a)
        lines.append(line)
        if line in subjects:
            state['subject'] = line

    def forward(batch):                                   # the engine stand-in: the whole sequence in one call, [T*Z][X2][Y2]
        lab = subjects[state['subject']]
        pred = np.zeros(batch.shape[:3], lab.dtype)
        x0, y0 = (batch.shape[1] - lab.shape[0]) // 2, (batch.shape[2] - lab.shape[1]) // 2
        pred[:, x0:x0 + lab.shape[0], y0:y0 + lab.shape[1]] = lab.transpose(3, 2, 0, 1).reshape((-1,) + lab.shape[:2])
        return {'pred': pred}
    argv = ['--seq_name', 'sa', '--data_dir', 'data', '--model_path', 'x', '--io_threads', '0', '--batch_slices', '1000',
            '--score_against', 'label_sa', '--score_csv', 'deploy.csv']
    FLAGS, _ = deploy_network.define_flags().parse(argv)
    assert deploy_network.run(FLAGS, forward, log=log) == ['s1', 's2', 's3', 's4']
    text = open('deploy.csv', newline='').read()
    assert sum('does not contain label_sa.nii.gz' in l for l in lines) == 1
    assert sum('label 200 outside' in l for l in lines) == 1 and sum('shape (40, 36, 2, 4)' in l for l in lines) == 1
    assert {l.split(',')[0] for l in text.splitlines()[1:]} == {'s1', 's5'}
    assert np.array_equal(nifti.load('data/s1/seg_sa.nii.gz').get_data(), subjects['s1'])
    # the stand-alone script reads s3 too (its label 200 makes 201 classes: refused) and s4 (shapes differ: refused)
    eval_segmentation.main(['--data_dir', 'data', '--seg_name', 'seg_sa', '--truth_name', 'label_sa', '--output_csv', 'alone.csv', '--host'])
    assert text == open('alone.csv', newline='').read()
    rows = [l.split(',') for l in text.splitlines()[1:]]
    assert len(rows) == 18 and rows[0][:3] == ['s1', '0', '1'] and all(len(r) == 7 for r in rows)
    # a second run segments nothing and scores every subject from its files
    lines.clear()
    FLAGS.score_csv = 'again.csv'
    assert deploy_network.run(FLAGS, forward, log=log) == []
    assert open('again.csv', newline='').read() == text
