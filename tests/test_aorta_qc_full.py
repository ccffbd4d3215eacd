"""The full aortic quality control (aorta_qc.py, deploy_network_ao.py --aortic_qc_full) against a restatement of
cardiac_utils.aorta_pass_quality_control (reference common/cardiac_utils.py:1739-1796) written here: numpy's own mean / max /
division for criterion 2, a plain breadth-first labeller with the 18-neighbourhood of skimage's connectivity=2 for criterion 3.
No GPU: the device statistics are compared with stats_host in test_aorta_qc_gpu.py."""
import collections
import itertools
import warnings

import numpy as np
import pytest

from ukbb_cardiac_amd import aorta_qc, measures, nifti
from ukbb_cardiac_amd import deploy_network_ao as DA

# neighbours differ in at most two coordinates (connectivity=2 in 3-D): 18 offsets
N18 = [d for d in itertools.product((-1, 0, 1), repeat=3) if d != (0, 0, 0) and sum(map(abs, d)) <= 2]


def bfs_label(mask):
    """Component sizes of a 3-D boolean mask (18-neighbourhood), breadth-first."""
    seen = np.zeros(mask.shape, bool)
    sizes = []
    for start in zip(*np.nonzero(mask)):
        if seen[start]:
            continue
        seen[start] = True
        queue, n = collections.deque([start]), 0
        while queue:
            p = queue.popleft()
            n += 1
            for d in N18:
                q = (p[0] + d[0], p[1] + d[1], p[2] + d[2])
                if all(0 <= q[i] < mask.shape[i] for i in range(3)) and mask[q] and not seen[q]:
                    seen[q] = True
                    queue.append(q)
        sizes.append(n)
    return sizes


def ref_qc(image, seg):
    """aorta_pass_quality_control restated: (passed, message of the first failing criterion)."""
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        for l_name, l in [('AAo', 1), ('DAo', 2)]:
            T = seg.shape[3]
            for t in range(T):
                if np.sum(seg[:, :, :, t] == l) == 0:
                    return False, 'The area of {0} is 0 at time frame {1}.'.format(l_name, t)
            mean_ed = image[:, :, :, 0][seg[:, :, :, 0] == l].mean()
            for t in range(T):
                if np.max(image[:, :, :, t][seg[:, :, :, t] == l]) / mean_ed >= 3:
                    return False, 'The image becomes very noisy at time frame {0}.'.format(t)
            for t in range(T):
                if sum(s > 10 for s in bfs_label(seg[:, :, :, t] == l)) >= 2:
                    return False, ('The segmentation has at least two connected components with more than 10 pixels '
                                   'at time frame {0}.'.format(t))
            A = np.sum(seg == l, axis=(0, 1, 2))
            for t in range(T):
                ratio = A[t] / float(A[t - 1])
                if ratio >= 2 or ratio <= 0.5:
                    return False, 'There is abrupt change of area at time frame {0}.'.format(t)
            if np.max(A) / np.min(A) >= 2:
                return False, 'There is large change of area between maximum and minimum areas.'
    return True, ''


def full_qc(image, seg):
    return aorta_qc.aorta_qc_full(measures.counts_from_labels(seg, 3), aorta_qc.stats_host(image, seg))


def test_bfs_labeller_equals_scipy():
    ndimage = pytest.importorskip('scipy.ndimage')
    st = ndimage.generate_binary_structure(3, 2)
    rng = np.random.default_rng(1)
    for _ in range(60):
        m = rng.random(tuple(rng.integers(1, 9, size=3))) < rng.uniform(0.2, 0.7)
        lab, n = ndimage.label(m, st)
        assert sorted(bfs_label(m)) == sorted(np.bincount(lab.ravel())[1:].tolist())


def test_host_labeller_equals_bfs():
    rng = np.random.default_rng(2)
    for _ in range(150):
        X, Y, Z, T = rng.integers(1, 12), rng.integers(1, 12), rng.integers(1, 4), rng.integers(1, 4)
        seg = rng.choice(3, size=(X, Y, Z, T), p=[0.4, 0.3, 0.3])
        m = int(rng.integers(0, 4))
        got = aorta_qc.count_large_components(seg, 3, min_size=m)
        want = [[0] + [sum(s > m for s in bfs_label(seg[..., t] == k)) for k in (1, 2)] for t in range(T)]
        assert got.tolist() == want


# ---- constructed cines: one failure per criterion, the order of the criteria, the thresholds ---------------------------
def base(T=6, Z=1, dtype=np.float32):
    """A cine that passes: steady AAo and DAo blocks of 30 voxels, intensities 100..120."""
    rng = np.random.default_rng(5)
    image = rng.uniform(100, 120, size=(24, 20, Z, T)).astype(dtype)
    seg = np.zeros((24, 20, Z, T), np.int32)
    seg[2:8, 2:7, 0] = 1
    seg[14:20, 10:15, 0] = 2
    return image, seg


def check(image, seg, want):
    got = full_qc(image, seg)
    assert got == ref_qc(image, seg)
    assert got == want
    return got


def test_passing_cine():
    check(*base(), (True, ''))


def test_criterion_1():
    image, seg = base()
    seg[..., 0, 3][seg[..., 0, 3] == 2] = 0
    check(image, seg, (False, 'The area of DAo is 0 at time frame 3.'))


def test_criterion_2():
    image, seg = base()
    image[3, 3, 0, 4] = 400.0
    check(image, seg, (False, 'The image becomes very noisy at time frame 4.'))


def test_criterion_3():
    image, seg = base()
    seg[14:20, 10:15, 0, 2] = 0
    seg[14:20, 10:12, 0, 2] = 2
    seg[14:20, 13:15, 0, 2] = 2                          # two 12-voxel pieces
    check(image, seg, (False, 'The segmentation has at least two connected components with more than 10 pixels at time frame 2.'))


def test_criterion_4():
    image, seg = base()
    seg[2:14, 2:7, 0, 3] = 1                             # AAo 30 -> 60 voxels
    check(image, seg, (False, 'There is abrupt change of area at time frame 3.'))


def test_criterion_5():
    image, seg = base()
    seg[..., 0, :][seg[..., 0, :] == 1] = 0
    for t, n in enumerate([40, 50, 64, 80, 64, 50]):    # adjacent ratios < 2 (also frame 0 against the last), max / min = 2
        seg[..., 0, t][(np.arange(24 * 20) < n).reshape(24, 20)] = 1      # the first n voxels of rows 0..3: one block
    check(image, seg, (False, 'There is large change of area between maximum and minimum areas.'))


def test_order_aao_before_dao():
    image, seg = base()
    seg[..., 0, 1][seg[..., 0, 1] == 2] = 0              # DAo: criterion 1
    seg[2:14, 2:7, 0, 3] = 1                             # AAo: criterion 4
    check(image, seg, (False, 'There is abrupt change of area at time frame 3.'))


def test_order_2_before_3_before_4():
    image, seg = base()
    seg[14:20, 10:15, 0, 1] = 0
    seg[14:20, 10:12, 0, 1] = 2
    seg[14:20, 13:15, 0, 1] = 2                          # DAo fragmented in frame 1
    image[15, 11, 0, 5] = 1000.0                         # DAo noisy in frame 5
    check(image, seg, (False, 'The image becomes very noisy at time frame 5.'))
    image[15, 11, 0, 5] = 110.0
    seg[14:24, 10:16, 0, 4] = 2                          # DAo abrupt change in frame 4
    check(image, seg, (False, 'The segmentation has at least two connected components with more than 10 pixels at time frame 1.'))


def test_ratio_exactly_three_and_one_ulp_below():
    image, seg = base()
    image[..., 0, 0][seg[..., 0, 0] == 1] = 1.0          # mean_ED of AAo = 1 exactly
    image[..., 0, 1:][seg[..., 0, 1:] == 1] = 1.0
    image[4, 4, 0, 2] = 3.0
    check(image, seg, (False, 'The image becomes very noisy at time frame 2.'))
    image[4, 4, 0, 2] = np.nextafter(np.float32(3.0), np.float32(0.0))
    check(image, seg, (True, ''))


def test_components_of_ten_and_eleven_voxels():
    image, seg = base()
    seg[9:11, 16:20, 0, :] = 2
    seg[11, 16:18, 0, :] = 2                             # a separate DAo piece of 10 voxels in every frame: not counted
    check(image, seg, (True, ''))
    seg[11, 18, 0, 3] = 2                                # 11 voxels in frame 3: counted
    check(image, seg, (False, 'The segmentation has at least two connected components with more than 10 pixels at time frame 3.'))


def test_diagonal_join_is_one_component():
    image, seg = base()
    seg[14:20, 10:15, 0, :] = 0
    seg[10:14, 10:13, 0, :] = 2                          # 12 voxels ...
    seg[14:18, 13:16, 0, :] = 2                          # ... and 12 more touching only at (13,12)-(14,13)
    check(image, seg, (True, ''))


def test_three_d_corner_does_not_connect():
    image, seg = base(Z=2)
    seg[..., 1, :] = 0
    seg[14:20, 10:15, :, :] = 0
    seg[2:5, 11:15, 0, :] = 2                            # 12 voxels in z = 0 ...
    seg[5:8, 15:19, 1, :] = 2                            # ... 12 in z = 1 touching only at the corner (4,14,0)-(5,15,1)
    check(image, seg, (False, 'The segmentation has at least two connected components with more than 10 pixels at time frame 0.'))
    seg[5, 14, 1, :] = 2                                 # an edge neighbour across z joins them
    check(image, seg, (True, ''))


def test_nan_under_the_mask_does_not_fail_criterion_2():
    image, seg = base()
    image[3, 3, 0, 2] = np.nan
    check(image, seg, (True, ''))
    assert np.isnan(aorta_qc.stats_host(image, seg)['max'][2, 1])
    image[3, 3, 0, 0] = np.nan                           # NaN mean_ED: every ratio NaN
    check(image, seg, (True, ''))


def _random_cine(rng, dtype):
    X, Y, Z, T = int(rng.integers(6, 15)), int(rng.integers(6, 15)), int(rng.choice([1, 1, 2])), int(rng.integers(2, 6))
    seg = np.zeros((X, Y, Z, T), np.int32)
    for t in range(T):
        for k in (1, 2):
            for _ in range(int(rng.integers(1, 3))):
                x0, y0 = rng.integers(0, X - 2), rng.integers(0, Y - 2)
                seg[x0:x0 + rng.integers(2, 6), y0:y0 + rng.integers(2, 6), rng.integers(0, Z), t] = k
        speck = rng.random((X, Y, Z)) < rng.uniform(0, 0.1)
        seg[..., t][speck] = rng.integers(0, 3, size=int(speck.sum()))
    if np.dtype(dtype).kind == 'f':
        image = rng.uniform(50, 100, size=seg.shape).astype(dtype)
    else:
        info = np.iinfo(dtype)
        lo, hi = (20, 80) if dtype == np.uint8 else (info.min // 4 if info.min < 0 else 100, 3000)
        image = rng.integers(lo, hi, size=seg.shape).astype(dtype)
    spikes = rng.random(seg.shape) < 0.01
    image[spikes] = image[spikes] * rng.choice([1, 3, 5]) if np.dtype(dtype).kind == 'f' else np.iinfo(dtype).max
    return image, seg


@pytest.mark.parametrize('dtype', [np.float32, np.uint8, np.int16, np.uint16])
def test_random_cines_equal_the_restatement(dtype):
    rng = np.random.default_rng({np.float32: 11, np.uint8: 12, np.int16: 13, np.uint16: 14}[dtype])
    outcomes = collections.Counter()
    for _ in range(80):
        image, seg = _random_cine(rng, dtype)
        got = full_qc(image, seg)
        assert got == ref_qc(image, seg)
        outcomes[got[1].split(' at ')[0].split(' of ')[0]] += 1
    assert len(outcomes) >= 3, outcomes                  # more than one criterion decides


# ---- the statistics themselves --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float32, np.float64, np.uint8, np.int16, np.uint16])
def test_mean_ed_is_numpys_mean_bit_for_bit(dtype):
    rng = np.random.default_rng(21)
    image = (rng.gamma(2.0, 300.0, size=(150, 130, 1, 2)) % 250).astype(dtype)
    seg = np.zeros(image.shape, np.int32)
    seg[:140, :120, 0, :] = 1                            # 16800 voxels: more than two of numpy's 8192-element buffers
    seg[140:, :50, 0, :] = 2
    st = aorta_qc.stats_host(image, seg)
    for k in (1, 2):
        want = image[..., 0][seg[..., 0] == k].mean()
        assert st['mean_ed'][k].dtype == want.dtype and st['mean_ed'][k].tobytes() == want.tobytes()
        assert np.array_equal(st['max'][:, k], [np.max(image[..., t][seg[..., t] == k]) for t in range(2)])


# ---- deploy_network_ao.py --aortic_qc_full on the host path -----------------------------------------------------------------
def test_deploy_drops_fragmented_and_noisy_subjects(tmp_path):
    names = ['3001', '3002', '3003']
    data = tmp_path / 'd'
    data.mkdir()
    rng = np.random.default_rng(31)
    for n in names:
        (data / n).mkdir()
        cine = rng.uniform(100, 120, size=(40, 36, 1, 6)).astype(np.float32)
        if n == '3003':
            cine[..., 3] *= 10.0                         # a noisy frame
        nifti.save(cine, str(data / n / 'ao.nii.gz'), np.diag([1.8, 1.8, 10.0, 1.0]), np.array([1, 1.8, 1.8, 10, 0.03, 0, 0, 0], np.float32))
    state = {'subject': None, 'frame': 0}
    lines = []

    def log(*a):
        line = ' '.join(str(x) for x in a)
        lines.append(line)
        if line in names:
            state['subject'], state['frame'] = line, 0

    def forward(batch):                                  # steady discs; 3002's DAo gains a separate 16-voxel piece in frame 2
        pred = np.zeros(batch.shape[:3], np.int32)
        cy, cx = batch.shape[1] // 2, batch.shape[2] // 2
        pred[:, cy - 16:cy - 6, cx - 14:cx - 4] = 1
        pred[:, cy + 2:cy + 12, cx + 2:cx + 10] = 2
        for k in range(batch.shape[0]):
            if state['subject'] == '3002' and state['frame'] + k == 2:
                pred[k, cy + 14:cy + 18, cx - 14:cx - 10] = 2
        state['frame'] += batch.shape[0]
        prob = np.zeros(batch.shape[:3] + (3,), np.float32)
        np.put_along_axis(prob, pred[..., None], 1.0, axis=-1)
        return {'prob': prob, 'pred': pred}

    rows = {}
    for flag in ([], ['--aortic_qc_full']):
        out = str(tmp_path / ('ao%d.csv' % len(flag)))
        F, _ = DA.define_flags().parse(['--data_dir', str(data), '--model', 'UNet', '--model_path', 'x', '--io_threads', '0',
                                        '--output_csv', out] + flag)
        assert F.aortic_qc_full == bool(flag)
        del lines[:]
        DA.run(F, forward, log=log)
        rows[bool(flag)] = open(out).read().splitlines()
    assert [r.split(',')[0] for r in rows[False][1:]] == names
    assert rows[True] == rows[False][:2]                 # header and 3001, byte for byte
    assert 'The segmentation has at least two connected components with more than 10 pixels at time frame 2.' in lines
    assert 'The image becomes very noisy at time frame 3.' in lines


def test_flag_defaults_to_off_and_help_names_it():
    F, _ = DA.define_flags().parse(['--data_dir', 'x'])
    assert F.aortic_qc_full is False
    assert '--aortic_qc_full' in DA.define_flags().usage()
