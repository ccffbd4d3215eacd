"""The atrial measures on the host: atrial.frame_stats_host (the specification of ukbb_fcn_atrial_area_length) and what is derived
from it equal the literal restatement of cardiac_utils.evaluate_atrial_area_length exactly on fixtures whose near-ties are asserted
away first; atrial.line_pixels draws the hand-written pixel lists; the table equals pandas' from the reference's formulas; the two
command lines agree.  tests/test_atrial_gpu.py takes its fixtures from here."""
import math
import os

import numpy as np
import pytest

from ukbb_cardiac_amd import atrial, measures, nifti, qc_gates

PIXDIM = np.array([1, 1.8, 1.8, 6.0, 0.03, 0, 0, 0], np.float32)
GAP = 1e-9


def rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def oblique(angles, spacing, origin):
    a = np.eye(4)
    a[:3, :3] = rot(*angles) @ np.diag(spacing)
    a[:3, 3] = origin
    return a


# three oblique long-axis affines (sines and cosines of these angles: no direction cosine is rational), each with the long axis of
# an oblique short-axis stack; and an axis-aligned pair, where d takes few values and the stable rule decides
AFFINES = [(oblique((0.37, 1.1, -0.6), (1.8, 1.8, 6.0), (-70.3, 41.9, 12.7)), oblique((-0.9, 0.3, 0.5), (1.8, 1.8, 10.0), (1.0, 2.0, 3.0))),
           (oblique((-1.3, 0.21, 2.2), (1.826, 1.826, 6.0), (55.1, -80.7, -33.3)), oblique((0.45, -0.8, 1.9), (1.8, 1.8, 10.0), (-9.0, 4.0, 7.0))),
           (oblique((2.9, -0.47, 0.83), (1.4, 1.4, 8.0), (13.2, 17.9, -120.4)), oblique((1.2, 0.66, -2.4), (1.8, 1.8, 10.0), (30.0, -2.0, 11.0)))]
ALIGNED = (np.diag([1.8, 1.8, 6.0, 1.0]), np.array([[0, 0, 1.8, 0], [1.8, 0, 0, 0], [0, 10.0, 0, 0], [0, 0, 0, 1.0]]))


def geometry(i):
    aff, sa = ALIGNED if i < 0 else AFFINES[i]
    return aff, atrial.long_axis_from_sa(sa)


def ellipse(X, Y, cx, cy, rx, ry, angle):
    xx, yy = np.meshgrid(np.arange(X), np.arange(Y), indexing='ij')
    u = (xx - cx) * np.cos(angle) + (yy - cy) * np.sin(angle)
    v = -(xx - cx) * np.sin(angle) + (yy - cy) * np.cos(angle)
    return (u / rx) ** 2 + (v / ry) ** 2 <= 1


def phantom_atrium(X, Y, seed, label=1, where=(0.5, 0.5), scale=1.0):
    """An atrium-like blob: an ellipse with a few lobes (pulmonary veins, appendage) and a handful of stray specks of the label."""
    rng = np.random.default_rng(seed)
    cx, cy = where[0] * X + rng.uniform(-2, 2), where[1] * Y + rng.uniform(-2, 2)
    rx, ry = scale * rng.uniform(0.12, 0.18) * X, scale * rng.uniform(0.10, 0.15) * Y
    m = ellipse(X, Y, cx, cy, rx, ry, rng.uniform(0, np.pi))
    for _ in range(3):
        a = rng.uniform(0, 2 * np.pi)
        m |= ellipse(X, Y, cx + 0.9 * rx * np.cos(a), cy + 0.9 * ry * np.sin(a), 0.35 * rx, 0.3 * ry, rng.uniform(0, np.pi))
    lab = np.where(m, label, 0).astype(np.int32)
    for _ in range(4):                                 # specks: smaller components that get_largest_cc drops
        lab[int(rng.integers(0, X)), int(rng.integers(0, Y))] = label
    return lab


def four_chamber(X, Y, seed):
    lab = phantom_atrium(X, Y, seed, 1, (0.35, 0.4), 0.8)
    ra = phantom_atrium(X, Y, seed + 1000, 2, (0.68, 0.62), 0.7)
    return np.where(lab != 0, lab, ra)


ARC_48x48 = (48, 48, 17.5624039937461, 26.78534654973304, 27.828210129390328, 0.9019783444108452, 3.76991094925643, 400)
ARC_48x40 = (48, 40, 16.898643823222162, 26.9701835665339, 16.94088829068449, 4.052559672951749, 5.131603259136801, 600)


def crescent(arc=ARC_48x48):
    """A one-pixel arc that the rasterised axis line steps across without touching: status 3 -- ARC_48x48 under AFFINES[0],
    ARC_48x40 (108 voxels) under the float32 copy of AFFINES[1].  Found by a search on the CPU."""
    X, Y, R, cx, cy, a0, span, steps = arc
    m = np.zeros((X, Y), np.int32)
    for a in np.linspace(a0, a0 + span, steps):
        m[int(round(cx + R * np.cos(a))), int(round(cy + R * np.sin(a)))] = 1
    return m


def fixtures():
    """[(name, (X, Y) labels, index into AFFINES)]: ellipse and phantom atria and a 4-chamber frame with both labels, under every
    oblique affine."""
    out = []
    for g in range(3):
        out.append(('ellipse_%d' % g, np.where(ellipse(64, 56, 30.3, 25.1, 15.2, 9.7, 0.4 + g), 1, 0).astype(np.int32), g))
        out.append(('phantom_%d' % g, phantom_atrium(72, 80, 10 + g), g))
        out.append(('four_chamber_%d' % g, four_chamber(88, 72, 20 + g), g))
    return out


def _gap_ok(d, i):
    """The sorted keys on both sides of position i | i+1 differ by more than GAP (an edge position has no neighbour)."""
    return not (0 <= i < len(d) - 1) or d[i + 1] - d[i] > GAP


def assert_no_near_ties(label2d, n_class, affine, long_axis):
    """The condition on the inputs under which the literal restatement (BLAS dot products, an unstable sort) and the kernel's
    specification must agree: for every non-zero cell the keys around the two third boundaries and next to the two extreme hits
    are more than 1e-9 apart, and no end-point coordinate lies within 1e-9 of an integer."""
    member, _ = atrial.winning_components(label2d[:, :, None], n_class)
    for k in range(1, n_class):
        row, det = atrial.cell_detail(member[:, :, 0], k, affine, long_axis)
        if row[0] == 0:
            continue
        d = det['d']
        assert _gap_ok(d, det['k1'] - 1) and _gap_ok(d, det['k2'] - 1), ('third boundary', k)
        if 'ends' in det:
            assert all(abs(v - round(v)) > GAP for v in det['ends']), ('end point', k, det['ends'])
        if 'hit_d' in det:
            h = det['hit_d']
            assert _gap_ok(h, 0) and _gap_ok(h, len(h) - 2), ('extreme hits', k)


def _same(ref, got):
    if isinstance(ref[0], int):
        return got == (-1, -1, -1) and ref == (-1, -1, -1)
    return (not isinstance(got[0], int) and ref[0] == got[0] and ref[1] == got[1] and len(ref[2]) == len(got[2])
            and all(np.array_equal(a, b) for a, b in zip(ref[2], got[2])))


@pytest.mark.parametrize('name,lab,g', fixtures(), ids=[f[0] for f in fixtures()])
def test_twin_equals_the_literal_restatement(name, lab, g):
    affine, long_axis = geometry(g)
    n_class = int(lab.max()) + 1
    assert_no_near_ties(lab, n_class, affine, long_axis)
    stats = atrial.frame_stats_host(lab, n_class, affine, long_axis)[0]
    assert stats.dtype == np.int32 and stats.shape == (n_class, 8) and not stats[0].any() and not stats[:, 7].any()
    assert (stats[1:, 1] == atrial.MEASURED).all()
    ref = atrial.area_length_reference(lab, affine, PIXDIM, long_axis)
    got = atrial.frame_measures(stats, affine, PIXDIM)
    assert _same(ref, got), (ref, got)
    # the integers themselves: the component size behind A, the two pixels behind the landmarks
    area_per_pix = PIXDIM[1] * PIXDIM[2] * 1e-2
    for i, k in enumerate(range(1, n_class)):
        assert ref[0][i] == stats[k, 0] * area_per_pix
        assert np.array_equal(ref[2][2 * i], atrial.world_point(affine, stats[k, 2], stats[k, 3]))
        assert np.array_equal(ref[2][2 * i + 1], atrial.world_point(affine, stats[k, 4], stats[k, 5]))
        assert 1 <= stats[k, 6] <= max(lab.shape)


def test_invalid_frames_are_invalid_in_both():
    affine, long_axis = geometry(0)
    for n in (1, 2):                                   # fewer than 3 voxels: the bottom third is empty
        lab = np.zeros((12, 9), np.int32)
        lab[4, 3:3 + n] = 1
        stats = atrial.frame_stats_host(lab, 2, affine, long_axis)[0]
        assert list(stats[1]) == [n, atrial.NO_AXIS, 0, 0, 0, 0, 0, 0]
        assert atrial.area_length_reference(lab, affine, PIXDIM, long_axis) == (-1, -1, -1) == atrial.frame_measures(stats, affine, PIXDIM)
    lab = np.zeros((12, 9), np.int32)
    lab[4, 3:6] = 1                                    # 3 voxels: one in each third, measured
    assert atrial.frame_stats_host(lab, 2, affine, long_axis)[0, 1, 1] == atrial.MEASURED
    assert not isinstance(atrial.area_length_reference(lab, affine, PIXDIM, long_axis)[0], int)
    c = crescent()
    stats = atrial.frame_stats_host(c, 2, affine, long_axis)[0]
    assert list(stats[1]) == [int(c.sum()), atrial.NO_HIT, 0, 0, 0, 0, 0, 0]
    assert atrial.area_length_reference(c, affine, PIXDIM, long_axis) == (-1, -1, -1)
    # one bad label invalidates the whole frame, the good label with it
    both = np.zeros((60, 48), np.int32)
    both[:48, :] = c * 2
    both[50:58, 10:30] = 1
    stats = atrial.frame_stats_host(both, 3, affine, long_axis)[0]
    assert stats[1, 1] == atrial.MEASURED and stats[2, 1] != atrial.MEASURED
    assert atrial.area_length_reference(both, affine, PIXDIM, long_axis) == (-1, -1, -1) == atrial.frame_measures(stats, affine, PIXDIM)
    # an absent label is not a bad one
    stats = atrial.frame_stats_host(np.where(both == 1, 1, 0), 3, affine, long_axis)[0]
    assert stats[2, 1] == atrial.ABSENT and len(atrial.frame_measures(stats, affine, PIXDIM)[0]) == 1


def test_tie_rule_and_stable_order_on_an_aligned_grid():
    affine, long_axis = geometry(-1)
    lab = np.zeros((20, 16), np.int32)
    lab[2:5, 10:14] = 1                                # 12 voxels, first in C order
    lab[12:16, 1:4] = 1                                # 12 voxels, first in the kernels' own NIfTI order
    lab[8, 8] = 1
    member, size = atrial.winning_components(lab[:, :, None], 2)
    assert size[0, 1] == 12 and member[2:5, 10:14, 0].all() and not member[12:16, 1:4, 0].any()
    stats = atrial.frame_stats_host(lab, 2, affine, long_axis)[0]
    assert stats[1, 0] == 12 and stats[1, 1] == atrial.MEASURED
    ref = atrial.area_length_reference(lab, affine, PIXDIM, long_axis)
    assert ref[0] == atrial.frame_measures(stats, affine, PIXDIM)[0]


# ---- line_pixels: 8 columns x 6 rows, expected lists written out by hand ---------------------------------------------------------
LINES = [
    ('horizontal', (1, 2), (5, 2), [(1, 2), (2, 2), (3, 2), (4, 2), (5, 2)]),
    ('vertical', (3, 0), (3, 4), [(3, 0), (3, 1), (3, 2), (3, 3), (3, 4)]),
    ('point', (2, 2), (2, 2), [(2, 2)]),
    ('diagonal', (0, 0), (5, 5), [(0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (5, 5)]),
    ('shallow_down', (0, 0), (7, 2), [(0, 0), (1, 0), (2, 1), (3, 1), (4, 1), (5, 1), (6, 2), (7, 2)]),
    ('shallow_up', (0, 4), (7, 2), [(0, 4), (1, 4), (2, 3), (3, 3), (4, 3), (5, 3), (6, 2), (7, 2)]),
    ('steep_down', (1, 0), (3, 5), [(1, 0), (1, 1), (2, 2), (2, 3), (3, 4), (3, 5)]),
    ('steep_right_to_left', (3, 0), (1, 5), [(1, 5), (1, 4), (2, 3), (2, 2), (3, 1), (3, 0)]),
    # leftToRight: drawn from the second point, which is NOT the mirror of walking from (7, 2)
    ('reversed', (7, 2), (0, 0), [(0, 0), (1, 0), (2, 1), (3, 1), (4, 1), (5, 1), (6, 2), (7, 2)]),
    ('both_outside_horizontal', (-3, 2), (10, 2), [(x, 2) for x in range(8)]),
    ('both_outside_diagonal', (-2, -2), (9, 9), [(0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (5, 5)]),
    ('one_outside', (4, 2), (10, 5), [(4, 2), (5, 3), (6, 3), (7, 4)]),
    ('outside_left', (-5, 1), (-1, 4), []),
    ('outside_above', (0, -3), (7, -1), []),
]


@pytest.mark.parametrize('name,p1,p2,want', LINES, ids=[l[0] for l in LINES])
def test_line_pixels_by_hand(name, p1, p2, want):
    assert atrial.line_pixels(p1, p2, 8, 6) == want


def test_line_pixels_degenerate_images_and_a_corner_miss():
    assert atrial.line_pixels((0, 1), (0, 4), 1, 6) == [(0, 1), (0, 2), (0, 3), (0, 4)]
    assert atrial.line_pixels((-3, 2), (4, 2), 1, 6) == [(0, 2)]
    assert atrial.line_pixels((2, -4), (5, 4), 8, 1) == [(3, 0)]
    assert atrial.line_pixels((1, 0), (6, 0), 8, 1) == [(x, 0) for x in range(1, 7)]
    assert atrial.line_pixels((-5, -1), (1, 100), 10, 10) == []          # passes the corner: rejected after the first clip stage


def test_line_closed_form_and_bounds():
    """What the kernel's lanes evaluate (pixel i from minor_steps) is the stepping rule, and a clipped line stays in the image."""
    rng = np.random.default_rng(5)
    for _ in range(2000):
        W, H = int(rng.integers(1, 12)), int(rng.integers(1, 12))
        p1, p2 = tuple(int(v) for v in rng.integers(-120, 130, 2)), tuple(int(v) for v in rng.integers(-120, 130, 2))
        px = atrial.line_pixels(p1, p2, W, H)
        s = atrial.line_setup(p1, p2, W, H)
        if s is None:
            assert px == []
            continue
        x, y, major, minor, dmaj, dmin, count = s
        cf = [(x + i * major[0] + atrial.minor_steps(i, dmaj, dmin) * minor[0], y + i * major[1] + atrial.minor_steps(i, dmaj, dmin) * minor[1])
              for i in range(count)]
        assert cf == px and all(0 <= a < W and 0 <= b < H for a, b in px), (p1, p2, W, H)


def test_line_pixels_against_opencv():
    cv2 = pytest.importorskip('cv2')
    rng = np.random.default_rng(6)
    for _ in range(3000):
        W, H = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        p1, p2 = tuple(int(v) for v in rng.integers(-130, 170, 2)), tuple(int(v) for v in rng.integers(-130, 170, 2))
        img = np.zeros((H, W))
        cv2.line(img, p1, p2, (1, 0, 0))
        want = np.zeros((H, W))
        for x, y in atrial.line_pixels(p1, p2, W, H):
            want[y, x] = 1
        assert np.array_equal(img, want), (p1, p2, W, H)


# ---- the table and the command lines ---------------------------------------------------------------------------------------------
X4, Y4, T4 = 48, 40, 4


def _sequence(seq, seed, T=T4, bad=None):
    """(X4, Y4, 1, T) labels of a beating atrium (both atria for la_4ch).  bad: 'invalid' -- frame 2 of la_2ch is the crescent;
    'empty' -- LA missing in frame 1; 'two' -- a second large LA component in frame 1; 'abrupt' -- frame 2 a third of the area."""
    seg = np.zeros((X4, Y4, 1, T), np.float64)
    for t in range(T):
        s = 1.0 + 0.08 * np.sin(2 * np.pi * t / T)
        f = np.where(ellipse(X4, Y4, 15.3, 14.2, 9.1 * s, 6.2 * s, 0.5), 1, 0)
        if seq == 'la_4ch':
            f = np.where(ellipse(X4, Y4, 33.4, 27.6, 7.3 * s, 5.9 * s, 2.0 + 0.1 * seed), 2, f)
        seg[:, :, 0, t] = f
    if bad == 'invalid':
        seg[:, :, 0, 2] = crescent(ARC_48x40)
    if bad == 'empty':
        seg[:, :, 0, 1][seg[:, :, 0, 1] == 1] = 0
    if bad == 'two':
        seg[40:46, 2:8, 0, 1] = 1
    if bad == 'abrupt':
        seg[:, :, 0, 2] = np.where(ellipse(X4, Y4, 15.3, 14.2, 5.0, 3.4, 0.5), 1, np.where(seg[:, :, 0, 2] == 2, 2, 0))
    return seg


SUBJECTS = {                                           # name -> (bad in la_2ch, bad in la_4ch, has sa, frames of la_4ch)
    's01_good': (None, None, True, T4),
    's02_invalid_frame': ('invalid', None, True, T4),
    's03_area_zero': ('empty', None, True, T4),
    's04_two_components': (None, 'two', True, T4),
    's05_abrupt': ('abrupt', None, True, T4),
    's06_no_sa': (None, None, False, T4),
    's07_short_4ch': (None, None, True, T4 - 1),
    's08_long_4ch': (None, None, True, T4 + 2),
}


def write_cohort(root):
    """The label files, long-axis and short-axis headers of SUBJECTS under ``root``."""
    for i, (name, (bad2, bad4, has_sa, t4)) in enumerate(sorted(SUBJECTS.items())):
        d = os.path.join(root, name)
        os.makedirs(d)
        aff2, sa = AFFINES[i % 3]
        aff4 = AFFINES[(i + 1) % 3][0]
        nifti.save(_sequence('la_2ch', i, T4, bad2), os.path.join(d, 'seg_la_2ch.nii.gz'), aff2, PIXDIM, as_dtype=np.float64)
        nifti.save(_sequence('la_4ch', i, t4, bad4), os.path.join(d, 'seg_la_4ch.nii.gz'), aff4, PIXDIM, as_dtype=np.float64)
        if has_sa:
            nifti.save(np.zeros((4, 4, 2, 1), np.float32), os.path.join(d, 'sa.nii.gz'), sa, np.array([1, 1.8, 1.8, 10, 0.03, 0, 0, 0], np.float32))


def reference_table(root, log):
    """long_axis/eval_atrial_volume.py:32-168 with evaluate_atrial_area_length = atrial.area_length_reference, the gate =
    qc_gates.atrium_gate, nib.load = nifti.load, as a pandas frame."""
    pd = pytest.importorskip('pandas')
    table, processed_list = [], []
    for data in sorted(os.listdir(root)):
        data_dir = os.path.join(root, data)
        names = ['{0}/seg_la_2ch.nii.gz'.format(data_dir), '{0}/seg_la_4ch.nii.gz'.format(data_dir), '{0}/sa.nii.gz'.format(data_dir)]
        if not all(os.path.exists(n) for n in names):
            continue
        long_axis = atrial.long_axis_from_sa(nifti.load(names[2]).affine)
        A, L, V = {}, {}, {}
        nim_2ch = nifti.load(names[0])
        seg_la_2ch = nim_2ch.get_data()
        T = seg_la_2ch.shape[3]
        if not qc_gates.gate_from_stats(qc_gates.stats_host(seg_la_2ch, 'la_2ch'), 'la_2ch', False, '')[0]:
            log.append('{0} seg_la_2ch does not atrium_pass_quality_control.'.format(data))
            continue
        A['LA_2ch'], L['LA_2ch'], V['LA_2ch'] = np.zeros(T), np.zeros(T), np.zeros(T)
        for t in range(T):
            area, length, landmarks = atrial.area_length_reference(seg_la_2ch[:, :, 0, t], nim_2ch.affine, nim_2ch.header['pixdim'], long_axis)
            if type(area) == int:
                if area < 0:
                    continue
            A['LA_2ch'][t] = area[0]
            L['LA_2ch'][t] = length[0]
            V['LA_2ch'][t] = 8 / (3 * math.pi) * area[0] * area[0] / length[0]
        nim_4ch = nifti.load(names[1])
        seg_la_4ch = nim_4ch.get_data()
        if not qc_gates.gate_from_stats(qc_gates.stats_host(seg_la_4ch, 'la_4ch'), 'la_4ch', False, '')[0]:
            log.append('{0} seg_la_4ch does not atrium_pass_quality_control.'.format(data))
            continue
        if seg_la_4ch.shape[3] < T:                    # the reference: IndexError
            continue
        for n in ('LA_4ch', 'RA_4ch'):
            A[n], L[n], V[n] = np.zeros(T), np.zeros(T), np.zeros(T)
        V['LA_bip'] = np.zeros(T)
        for t in range(T):
            area, length, landmarks = atrial.area_length_reference(seg_la_4ch[:, :, 0, t], nim_4ch.affine, nim_4ch.header['pixdim'], long_axis)
            if type(area) == int:
                if area < 0:
                    continue
            A['LA_4ch'][t] = area[0]
            L['LA_4ch'][t] = length[0]
            V['LA_4ch'][t] = 8 / (3 * math.pi) * area[0] * area[0] / length[0]
            V['LA_bip'][t] = 8 / (3 * math.pi) * area[0] * A['LA_2ch'][t] / (0.5 * (length[0] + L['LA_2ch'][t]))
            A['RA_4ch'][t] = area[1]
            L['RA_4ch'][t] = length[1]
            V['RA_4ch'][t] = 8 / (3 * math.pi) * area[1] * area[1] / length[1]
        val = {}
        val['LAV_bip_max'] = np.max(V['LA_bip'])
        val['LAV_bip_min'] = np.min(V['LA_bip'])
        val['LASV_bip'] = val['LAV_bip_max'] - val['LAV_bip_min']
        val['LAEF_bip'] = val['LASV_bip'] / val['LAV_bip_max'] * 100
        val['RAV_4ch_max'] = np.max(V['RA_4ch'])
        val['RAV_4ch_min'] = np.min(V['RA_4ch'])
        val['RASV_4ch'] = val['RAV_4ch_max'] - val['RAV_4ch_min']
        val['RAEF_4ch'] = val['RASV_4ch'] / val['RAV_4ch_max'] * 100
        table += [[val['LAV_bip_max'], val['LAV_bip_min'], val['LASV_bip'], val['LAEF_bip'],
                   val['RAV_4ch_max'], val['RAV_4ch_min'], val['RASV_4ch'], val['RAEF_4ch']]]
        processed_list += [data]
    return pd.DataFrame(table, index=processed_list, columns=['LAV max (mL)', 'LAV min (mL)', 'LASV (mL)', 'LAEF (%)',
                                                              'RAV max (mL)', 'RAV min (mL)', 'RASV (mL)', 'RAEF (%)'])


def test_cohort_fixtures_meet_the_input_condition():
    for i, (name, (bad2, bad4, _, t4)) in enumerate(sorted(SUBJECTS.items())):
        for seq, bad, g, T in (('la_2ch', bad2, i % 3, T4), ('la_4ch', bad4, (i + 1) % 3, t4)):
            seg = _sequence(seq, i, T, bad)
            affine = AFFINES[g][0].astype(np.float32).astype(np.float64)      # as the file stores it
            long_axis = atrial.long_axis_from_sa(AFFINES[i % 3][1].astype(np.float32).astype(np.float64))
            for t in range(T):
                assert_no_near_ties(seg[:, :, 0, t].astype(np.int32), 3, affine, long_axis)


def test_table_and_command_lines(tmp_path, capsys):
    from ukbb_cardiac_amd import deploy_network, eval_atrial_volume
    root = str(tmp_path / 'data')
    os.makedirs(root)
    write_cohort(root)
    ref_log = []
    want = reference_table(root, ref_log)
    want_csv = str(tmp_path / 'want.csv')
    want.to_csv(want_csv)
    assert list(want.index) == ['s01_good', 's02_invalid_frame', 's08_long_4ch']
    assert list(want.columns) == atrial.ATRIAL_COLUMNS
    # the invalid frame stays 0 and the minimum runs over it
    assert want.loc['s02_invalid_frame', 'LAV min (mL)'] == 0 and want.loc['s01_good', 'LAV min (mL)'] > 0
    got_csv = str(tmp_path / 'got.csv')
    capsys.readouterr()
    eval_atrial_volume.main(['--data_dir', root, '--output_csv', got_csv, '--host'])
    out = capsys.readouterr().out.splitlines()
    assert open(got_csv).read() == open(want_csv).read()
    assert [l for l in out if 'does not atrium_pass_quality_control' in l] == ref_log and len(ref_log) == 3
    for message in ('The area of LA is 0 at time frame 1.', 'The segmentation has at least two connected components with more than 10 pixels '
                    'at time frame 1.', 'There is abrupt change of area at time frame 2.'):
        assert message in out
    assert any(l.startswith('s07_short_4ch seg_la_4ch has 3 frames') for l in out) and 's06_no_sa' not in out
    # the per-frame records of the deploy script, from the label files of an 'earlier run' (no engine: nothing is segmented)
    frames = {}
    for seq in ('la_2ch', 'la_4ch'):
        frames[seq] = str(tmp_path / (seq + '_frames.csv'))
        FLAGS, _ = deploy_network.define_flags().parse(['--seq_name', seq, '--data_dir', root, '--atrial_csv', frames[seq]])
        deploy_network.run(FLAGS, None, log=lambda *_: None)
        rows = open(frames[seq]).read().splitlines()
        assert rows[0] == ',' + ','.join(atrial.FRAME_COLUMNS)
        n_lab = 1 if seq == 'la_2ch' else 2
        assert len(rows) - 1 == n_lab * sum(T4 if seq == 'la_2ch' else v[3] for v in SUBJECTS.values() if v[2])
        assert not any(r.startswith('s06_no_sa') for r in rows)
    two = [r.split(',') for r in open(frames['la_2ch']).read().splitlines()[1:]]
    assert [r[4] for r in two if r[0] == 's02_invalid_frame'] == ['1', '1', '3', '1']
    assert {r[0] for r in two if r[-1] == 'False'} == {'s03_area_zero', 's05_abrupt'}
    frames_csv = str(tmp_path / 'frames.csv')
    eval_atrial_volume.main(['--frames_2ch', frames['la_2ch'], '--frames_4ch', frames['la_4ch'], '--output_csv', frames_csv])
    assert open(frames_csv).read() == open(want_csv).read()


def test_frames_csv_merges_by_subject_frame_and_label(tmp_path):
    path = str(tmp_path / 'a.csv')
    row = lambda t, k: [t, k, 5, 1, 1, 2, 3, 4, 2, 0.5, 1.25, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, True]
    atrial.write_frames_csv(measures.shard_csv_name(path, 0, 2), [('b', row(t, k)) for t in range(12) for k in (1, 2)] + [('a', row(0, 1))])
    atrial.write_frames_csv(measures.shard_csv_name(path, 1, 2), [('a', row(0, 1)), ('a', row(1, 1)), ('c', row(0, 1))])
    assert atrial.merge_frames_csv(path, 2)
    rows = [r.split(',')[:3] for r in open(path).read().splitlines()[1:]]
    assert rows == [['a', '0', '1'], ['a', '1', '1']] + [['b', str(t), str(k)] for t in range(12) for k in (1, 2)] + [['c', '0', '1']]
    back = atrial.read_frames_csv(path)
    assert back['b']['gate'] and len(back['b']['frames']) == 12 and back['b']['frames'][3] == [(0.5, 1.25), (0.5, 1.25)]


def test_atrial_csv_flag_validation(tmp_path):
    from ukbb_cardiac_amd import deploy_network
    os.makedirs(str(tmp_path / 'd'))
    base = ['--data_dir', str(tmp_path / 'd'), '--atrial_csv', str(tmp_path / 'x.csv')]
    for bad in (['--seq_name', 'sa'], ['--seq_name', 'la_4ch', '--seg4'], ['--seq_name', 'la_2ch', '--noprocess_seq']):
        FLAGS, _ = deploy_network.define_flags().parse(base + bad)
        with pytest.raises(ValueError, match='--atrial_csv'):
            deploy_network.run(FLAGS, None, log=lambda *_: None)
    FLAGS, _ = deploy_network.define_flags().parse(['--seq_name', 'la_2ch', '--data_dir', str(tmp_path / 'd'), '--output_csv', str(tmp_path / 'y.csv')])
    with pytest.raises(ValueError, match='--output_csv'):                          # unchanged: still sa only
        deploy_network.run(FLAGS, None, log=lambda *_: None)
    FLAGS, _ = deploy_network.define_flags().parse(base + ['--seq_name', 'la_4ch'])
    deploy_network.run(FLAGS, None, log=lambda *_: None)
    assert open(str(tmp_path / 'x.csv')).read() == ',' + ','.join(atrial.FRAME_COLUMNS) + '\n'
