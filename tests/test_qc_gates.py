"""qc_gates.py against restatements of the three reference functions it serves -- cardiac_utils.sa_pass_quality_control
(reference common/cardiac_utils.py:77-136), la_pass_quality_control (:139-169) and atrium_pass_quality_control (:1616-1652), with
get_largest_cc / remove_small_cc of common/image_utils.py:227-249 -- written here on arrays instead of file names, over a plain
breadth-first labeller that numbers components by their first voxel in a C-order scan (what skimage.measure.label does; checked
below against scipy.ndimage.label, label arrays and all).  Then deploy_network.py --qc_csv on the host path."""
import collections
import itertools

import numpy as np
import pytest

from ukbb_cardiac_amd import aorta_qc, nifti, qc_gates
from ukbb_cardiac_amd import deploy_network as D

# ---- the restatement ---------------------------------------------------------------------------------------------------------
N8 = [d for d in itertools.product((-1, 0, 1), repeat=2) if d != (0, 0)]
N18 = [d for d in itertools.product((-1, 0, 1), repeat=3) if 0 < sum(abs(c) for c in d) <= 2]


def bfs_label(binary, offsets=None):
    """(label array, number of labels) of a 2-D (8-neighbourhood) or 3-D (18-neighbourhood: skimage's connectivity=2) mask; label
    i is the i-th component met in a C-order scan of the array's indices, whatever its memory order."""
    binary = np.asarray(binary)
    offsets = offsets or (N8 if binary.ndim == 2 else N18)
    cc = np.zeros(binary.shape, np.int32)
    n = 0
    for start in zip(*np.nonzero(binary)):             # np.nonzero walks in C order
        if cc[start]:
            continue
        n += 1
        cc[start] = n
        queue = collections.deque([start])
        while queue:
            v = queue.popleft()
            for d in offsets:
                w = tuple(a + b for a, b in zip(v, d))
                if all(0 <= c < s for c, s in zip(w, binary.shape)) and binary[w] and not cc[w]:
                    cc[w] = n
                    queue.append(w)
    return cc, n


def components(mask):
    """(label array, sizes) of a mask: sizes[i] voxels carry label i + 1."""
    cc, n = bfs_label(mask)
    return cc, np.bincount(cc.ravel(), minlength=n + 1)[1:]


def largest_component(mask):
    """The component with the most voxels -- of several that many, the one with the lowest label, i.e. met first in the scan (the
    reference keeps a label only for a strictly greater area, image_utils.py:227-238); all False for an empty mask."""
    cc, sizes = components(mask)
    return cc == 1 + int(np.argmax(sizes)) if sizes.size else np.zeros(np.shape(mask), bool)


def without_small(mask, thres=10):
    """The mask less its components of fewer than thres voxels (image_utils.py:241-249)."""
    cc, sizes = components(mask)
    return np.concatenate([[False], sizes >= thres])[cc]


def epi_size(plane, a=1, b=2, thres=10):
    """Voxels of the largest component of (largest cavity component | myocardium without small components): cardiac_utils.py:123-128."""
    return int(largest_component(largest_component(plane == a) | without_small(plane == b, thres)).sum())


def ref_plane_stats(planes, n_class, a=1, b=2, keep_min=10):
    """The statistics of qc_gates' docstring read off the labeller, plane by plane."""
    X, Y, P = planes.shape
    st = {k: np.zeros((P, n_class), np.int32) for k in ('count', 'largest', 'kept')}
    st['union_largest'] = np.zeros(P, np.int32)
    for p in range(P):
        for k in range(1, n_class):
            sizes = components(planes[:, :, p] == k)[1]
            st['count'][p, k] = sizes.sum()
            st['largest'][p, k] = sizes.max(initial=0)
            st['kept'][p, k] = sizes[sizes >= keep_min].sum()
        st['union_largest'][p] = epi_size(planes[:, :, p], a, b, keep_min)
    return st


TOO_SMALL = '{0}: The segmentation for class {1} is smaller than 10 pixels. It does not pass the quality control.'
FEW_SLICES = '{0}: The segmentation has less than 6 slices. It does not pass the quality control.'
GAP = '{0}: There is missing segmentation between the slices. It does not pass the quality control.'
NO_AHA = '{0}: Can not find LV epi or RV to determine the AHA coordinate system.'
NO_CONTOUR = '{0}: Can not find LV endo, myo or epi to extract the long-axis myocardial contour.'
NO_AREA = 'The area of {0} is 0 at time frame {1}.'
FRAGMENTS = 'The segmentation has at least two connected components with more than 10 pixels at time frame {0}.'
ABRUPT = 'There is abrupt change of area at time frame {0}.'


def ref_sa(seg, name):
    """sa_pass_quality_control (cardiac_utils.py:77-136) on an (X,Y,Z) label array: (passed, what it prints)."""
    per_slice = {l: (seg == k).sum(axis=(0, 1)) for l, k in (('LV', 1), ('Myo', 2), ('RV', 3))}
    for l in ('LV', 'Myo', 'RV'):                      # 1: each class has 10 voxels in the volume
        if per_slice[l].sum() < 10:
            return False, TOO_SMALL.format(name, l)
    usable = np.flatnonzero((per_slice['LV'] >= 10) & (per_slice['Myo'] >= 10))
    if usable.size < 6:                                # 2: six slices with cavity and myocardium, without a hole between them
        return False, FEW_SLICES.format(name)
    if usable[-1] - usable[0] + 1 != usable.size:
        return False, GAP.format(name)
    mid = seg[:, :, int(round(np.mean(np.nonzero(seg == 1)[2])))]      # 3: the slice at the rounded mean z of the cavity voxels
    if epi_size(mid) < 10 or largest_component(mid == 3).sum() < 10:
        return False, NO_AHA.format(name)
    return True, ''


def ref_la(seg, name):
    """la_pass_quality_control (cardiac_utils.py:139-169) on an (X,Y,Z) label array: plane 0 only."""
    plane = seg[:, :, 0]
    for l, k in (('LV', 1), ('Myo', 2), ('RV', 3), ('LA', 4), ('RA', 5)):
        if (plane == k).sum() < 10:
            return False, TOO_SMALL.format(name, l)
    if min(largest_component(plane == 1).sum(), without_small(plane == 2).sum(), epi_size(plane)) < 10:
        return False, NO_CONTOUR.format(name)
    return True, ''


def ref_atrium(label, label_dict):
    """atrium_pass_quality_control (cardiac_utils.py:1616-1652) on an (X,Y,Z,T) label array; per label, in dict order: no empty
    frame, no frame with two components of more than 10 voxels (18-neighbourhood), no area ratio to the previous frame (frame 0: to
    the last) of 2 or more or of a half or less."""
    T = label.shape[3]
    for l, k in label_dict.items():
        area = (label == k).sum(axis=(0, 1, 2))
        if (area == 0).any():
            return False, NO_AREA.format(l, int(np.argmax(area == 0)))
        for t in range(T):
            if (components(label[:, :, :, t] == k)[1] > 10).sum() >= 2:
                return False, FRAGMENTS.format(t)
        ratio = area / np.roll(area, 1).astype(float)
        jumps = (ratio >= 2) | (ratio <= 0.5)
        if jumps.any():
            return False, ABRUPT.format(int(np.argmax(jumps)))
    return True, ''


def ref_gate(seg, seq_name, seg4, name):
    kind = qc_gates.gate_kind(seq_name, seg4)
    if kind == 'sa':
        return ref_sa(seg[..., 0], name)
    if kind == 'la':
        return ref_la(seg[..., 0], name)
    return ref_atrium(seg, qc_gates.ATRIUM_LABELS[seq_name])


def host_gate(seg, seq_name, seg4, name):
    return qc_gates.gate_from_stats(qc_gates.stats_host(seg, seq_name, seg4), seq_name, seg4, name)


# ---- 1. the labeller is scipy's (and so skimage's) ----------------------------------------------------------------------------
@pytest.mark.parametrize('order', ['C', 'F'])
def test_labeller_numbers_components_like_scipy(order):
    ndi = pytest.importorskip('scipy.ndimage')
    rng = np.random.default_rng(5)
    for shape in [(9, 13), (13, 9), (1, 20), (20, 1), (16, 16)] * 4:
        m = np.asarray(rng.random(shape) < rng.uniform(0.2, 0.6), order=order)
        want, n = ndi.label(m, structure=np.ones((3, 3)))
        got, k = bfs_label(m)
        assert k == n and np.array_equal(got, want)
    for shape in [(6, 7, 3), (5, 5, 1), (4, 9, 2)] * 3:
        m = np.asarray(rng.random(shape) < 0.3, order=order)
        want, n = ndi.label(m, structure=ndi.generate_binary_structure(3, 2))
        got, k = bfs_label(m)
        assert k == n and np.array_equal(got, want)


# ---- 2. plane_stats_host on random planes ------------------------------------------------------------------------------------
def test_plane_stats_host_equals_the_labeller_on_random_planes():
    rng = np.random.default_rng(6)
    shapes = [(1, 17), (17, 1), (1, 1), (12, 9), (9, 12), (16, 16), (7, 20)]
    ties = 0
    for i in range(150):
        X, Y = shapes[i % len(shapes)]
        n_class = 2 + i % 5
        P = 1 + i % 3
        planes = rng.integers(0, n_class + (i % 4 == 0), size=(X, Y, P))          # sometimes a label beyond n_class: ignored
        planes[rng.random((X, Y, P)) < rng.uniform(0, 0.7)] = 0
        planes = np.asarray(planes.astype([np.uint8, np.int32, np.float64][i % 3]), order='CF'[i % 2])
        a, b = (1, 2) if n_class < 4 or i % 2 else (3, 1)
        if n_class < 3:
            a, b = 1, 2                                                          # class b is then absent: the union is the largest of a
        keep_min = int(rng.integers(1, 6))
        got = qc_gates.plane_stats_host(planes, max(n_class, 3), a, b, keep_min)
        want = ref_plane_stats(planes, max(n_class, 3), a, b, keep_min)
        for k in want:
            assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), (i, k, planes[:, :, 0])
        for p in range(P):                                                      # how often the tie rule had to decide
            cc, n = bfs_label(planes[:, :, p] == a)
            sizes = np.bincount(cc.ravel())[1:]
            ties += int(n > 1 and (sizes == sizes.max()).sum() > 1)
    assert ties > 20


# ---- 3. constructed volumes: every criterion, every boundary ----------------------------------------------------------------
NAME = 'subject/seg_sa_ED.nii.gz'
SA_MSG = {
    'LV': NAME + ': The segmentation for class LV is smaller than 10 pixels. It does not pass the quality control.',
    'Myo': NAME + ': The segmentation for class Myo is smaller than 10 pixels. It does not pass the quality control.',
    'RV': NAME + ': The segmentation for class RV is smaller than 10 pixels. It does not pass the quality control.',
    'slices': NAME + ': The segmentation has less than 6 slices. It does not pass the quality control.',
    'gap': NAME + ': There is missing segmentation between the slices. It does not pass the quality control.',
    'aha': NAME + ': Can not find LV epi or RV to determine the AHA coordinate system.',
}
LA_MSG = {l: NAME + ': The segmentation for class %s is smaller than 10 pixels. It does not pass the quality control.' % l
          for l in ('LV', 'Myo', 'RV', 'LA', 'RA')}
LA_MSG['contour'] = NAME + ': Can not find LV endo, myo or epi to extract the long-axis myocardial contour.'


def sa_slice(seg, z):
    """A healthy slice: a 4x4 cavity inside a 6x6 ring (16 + 20 voxels) and a 4x5 RV."""
    seg[4:10, 4:10, z] = 2
    seg[5:9, 5:9, z] = 1
    seg[12:16, 4:9, z] = 3


def sa_volume(slices=range(8), Z=8):
    seg = np.zeros((24, 20, Z), np.int32)
    for z in slices:
        sa_slice(seg, z)
    return seg


def _wipe(seg, z):
    seg[:, :, z] = 0


def sa_cases():
    """name -> ((X,Y,Z) labels, expected (passed, message))."""
    ok = (True, '')
    cases = {'healthy': (sa_volume(), ok)}
    for l_name, l in (('LV', 1), ('Myo', 2), ('RV', 3)):                        # criterion 1: 3-D totals of 9 and 10
        for n in (9, 10):
            seg = sa_volume()
            seg[seg == l] = 0
            seg[20, 0:5, 0] = l                                                 # 5 voxels on slice 0, 4 or 5 on slice 1
            seg[20, 0:n - 5, 1] = l
            assert (seg == l).sum() == n
            # with 10 the class exists; LV / Myo then leave no usable slice, a 10-voxel RV in two pieces fails on the mid slice
            cases['%s_total_%d' % (l_name, n)] = (seg, (False, SA_MSG[l_name] if n == 9 else SA_MSG['slices' if l < 3 else 'aha']))
    cases['five_slices'] = (sa_volume(range(5)), (False, SA_MSG['slices']))
    cases['six_slices'] = (sa_volume(range(6)), ok)
    for l, n, want in ((1, 9, 'slices'), (1, 10, None), (2, 9, 'slices'), (2, 10, None)):     # a slice counts with 10 + 10 voxels
        seg = sa_volume(range(6))
        seg[:, :, 5] = 0
        seg[2, 0:10, 5] = 1
        seg[4, 0:10, 5] = 2
        seg[2 if l == 1 else 4, n:10, 5] = 0
        cases['slice_with_%d_of_class_%d' % (n, l)] = (seg, ok if want is None else (False, SA_MSG[want]))
    seg = sa_volume()
    _wipe(seg, 3)
    cases['one_slice_gap'] = (seg, (False, SA_MSG['gap']))
    seg = sa_volume()
    seg[seg[:, :, 3] == 1, 3] = 2                                               # no cavity on slice 3: a gap as well
    cases['gap_without_cavity'] = (seg, (False, SA_MSG['gap']))
    # criterion 3 looks at int(round(cz)): 2.5 -> 2 and 3.5 -> 4 (half to even).  Removing the RV there fails, elsewhere not.
    for cz, sl, z_used in ((2.5, range(0, 6), 2), (3.5, range(1, 7), 4)):
        for z in (2, 3, 4):
            seg = sa_volume(sl)
            seg[12:16, 4:9, z] = 0
            cases['cz_%.1f_no_rv_on_%d' % (cz, z)] = (seg, (False, SA_MSG['aha']) if z == z_used else ok)
    for n in (9, 10):                                                          # the mid slice of nine: cz = 4 whatever slice 4 holds
        seg = sa_volume(range(9), 9)
        seg[12:16, 4:9, 4] = 0
        seg[12, 0:n, 4] = 3                                                     # RV: largest component of n voxels ...
        seg[14, 0:9, 4] = 3                                                     # ... beside one of 9
        cases['rv_largest_%d' % n] = (seg, ok if n == 10 else (False, SA_MSG['aha']))
        seg = sa_volume(range(9), 9)
        seg[4:10, 4:10, 4] = 0
        seg[0, 0:5, 4] = 1
        seg[2, 0:5, 4] = 1                                                      # cavity: two pieces of 5 (the slice still counts)
        seg[4, 0:n, 4] = 2                                                      # myocardium: a piece of n beside one of 9
        seg[6, 0:9, 4] = 2
        cases['myo_component_%d' % n] = (seg, ok if n == 10 else (False, SA_MSG['aha']))
    for which in ('later', 'earlier'):                                         # two equal-largest cavities, one touches the myocardium
        seg = sa_volume(range(9), 9)
        seg[4:10, 4:10, 4] = 0
        seg[1:3, 14:17, 4] = 1                                                  # first in C order (x = 1), last in NIfTI order (y = 14)
        seg[18:20, 1:4, 4] = 1
        x0, y0 = (20, 1) if which == 'later' else (3, 14)
        seg[x0:x0 + 2, y0:y0 + 6, 4] = 2                                        # 12 voxels against that cavity
        cases['tie_%s_touches_myo' % which] = (seg, ok)
    return cases


def la_plane():
    seg = np.zeros((24, 20, 1), np.int32)
    seg[2:8, 2:8, 0] = 2
    seg[3:7, 3:7, 0] = 1
    for i, l in enumerate((3, 4, 5)):
        seg[10 + 4 * i:13 + 4 * i, 2:6, 0] = l                                  # 12 voxels each
    return seg


def la_cases():
    ok = (True, '')
    cases = {'healthy': (la_plane(), ok)}
    for l_name, l in qc_gates.LA_LABELS:
        for n in (9, 10):
            seg = la_plane()
            seg[seg == l] = 0
            seg[22, 0:n, 0] = l
            want = ok if n == 10 else (False, LA_MSG[l_name])
            cases['%s_%d' % (l_name, n)] = (seg, want)
    seg = la_plane()
    seg[2:8, 2:8, 0] = 0
    seg[0, 0:9, 0] = 1
    seg[2, 0:9, 0] = 1                                                          # 18 cavity voxels, largest component 9
    seg[4, 0:12, 0] = 2
    cases['endo_largest_9'] = (seg, (False, LA_MSG['contour']))
    seg = seg.copy()
    seg[0, 9, 0] = 1
    cases['endo_largest_10'] = (seg, ok)
    for n in (9, 10):
        seg = la_plane()
        seg[2:8, 2:8, 0] = 0
        seg[0, 0:12, 0] = 1
        seg[2, 0:9, 0] = 2
        seg[4, 0:n, 0] = 2                                                      # myocardium: pieces of 9 and n
        cases['myo_component_%d' % n] = (seg, ok if n == 10 else (False, LA_MSG['contour']))
    seg = la_plane()
    seg = np.concatenate([seg, np.zeros_like(seg)], axis=2)                     # only plane 0 is read
    cases['second_plane_empty'] = (seg, ok)
    return cases


def atrium_volume(areas_la, areas_ra=None, Z=1):
    """(28, 20, Z, T) labels: per frame a single bar of areas_la[t] LA voxels (and one of RA), 2 voxels wide."""
    T = len(areas_la)
    seg = np.zeros((28, 20, Z, T), np.int32)
    for l, areas, x0 in ((1, areas_la, 0), (2, areas_ra, 14)):
        for t, n in enumerate(areas or []):
            bar = np.zeros(13 * 20, np.int32)
            bar[:n] = l
            seg[x0:x0 + 13, :, 0, t] = np.maximum(seg[x0:x0 + 13, :, 0, t], bar.reshape(13, 20))
    return seg


def atrium_cases():
    """name -> ((X,Y,Z,T) labels, seq_name, expected)."""
    ok = (True, '')
    abrupt = 'There is abrupt change of area at time frame {0}.'
    two = 'The segmentation has at least two connected components with more than 10 pixels at time frame {0}.'
    steady = [40, 42, 44, 43, 41]
    cases = {'healthy_2ch': (atrium_volume(steady), 'la_2ch', ok),
             'healthy_4ch': (atrium_volume(steady, steady[::-1]), 'la_4ch', ok),
             'la_vanishes': (atrium_volume([40, 42, 0, 43, 41]), 'la_2ch', (False, 'The area of LA is 0 at time frame 2.')),
             'ra_vanishes': (atrium_volume(steady, [40, 42, 44, 43, 0]), 'la_4ch', (False, 'The area of RA is 0 at time frame 4.')),
             'ra_ignored_in_2ch': (atrium_volume(steady, [40, 42, 44, 43, 0]), 'la_2ch', ok),
             'la_first': (atrium_volume([40, 80, 60, 50, 41], [0, 1, 1, 1, 1]), 'la_4ch', (False, abrupt.format(1))),
             'ratio_2': (atrium_volume([40, 42, 84, 60, 41]), 'la_2ch', (False, abrupt.format(2))),
             'ratio_below_2': (atrium_volume([40, 42, 83, 60, 41]), 'la_2ch', ok),
             'ratio_half': (atrium_volume([40, 60, 84, 42, 41]), 'la_2ch', (False, abrupt.format(3))),
             'ratio_above_half': (atrium_volume([40, 60, 84, 43, 41]), 'la_2ch', ok),
             'wrap_ratio_2': (atrium_volume([80, 70, 60, 50, 40]), 'la_2ch', (False, abrupt.format(0))),
             'wrap_ratio_half': (atrium_volume([40, 50, 60, 70, 80]), 'la_2ch', (False, abrupt.format(0))),
             'wrap_ok': (atrium_volume([79, 70, 60, 50, 40]), 'la_2ch', ok),
             'ra_abrupt': (atrium_volume(steady, [40, 42, 44, 88, 60]), 'la_4ch', (False, abrupt.format(3)))}
    for n in (10, 11):                                                         # two more pieces of n voxels: counted above 10 only
        seg = atrium_volume(steady)
        seg[20, 0:n, 0, 3] = 1
        seg[22, 0:n, 0, 3] = 1
        seg[0:2, 0:n, 0, 3] = 0                                                 # the bar gives 2n voxels back: no abrupt change
        cases['two_pieces_of_%d' % n] = (seg, 'la_2ch', ok if n == 10 else (False, two.format(3)))
    seg = atrium_volume(steady, steady, Z=2)
    seg[20:22, 0:6, 1, 2] = 2                                                   # 12 RA voxels on z = 1, away from the bar on z = 0
    cases['second_piece_on_other_plane'] = (seg, 'la_4ch', (False, two.format(2)))
    return cases


@pytest.mark.parametrize('case', sorted(sa_cases()))
def test_sa_gate_constructed(case):
    seg, want = sa_cases()[case]
    assert ref_sa(seg, NAME) == want
    assert qc_gates.sa_gate(qc_gates.plane_stats_host(seg, 4), NAME) == want
    assert host_gate(seg[..., None], 'sa', False, NAME) == want


def test_sa_tie_rule_changes_the_union():
    got = {}
    for which in ('later', 'earlier'):
        seg, _ = sa_cases()['tie_%s_touches_myo' % which]
        st = qc_gates.plane_stats_host(seg, 4)
        ref = ref_plane_stats(seg, 4)
        for k in ref:
            assert np.array_equal(st[k], ref[k]), (which, k)
        assert st['largest'][4, 1] == 6 and st['kept'][4, 2] == 12
        got[which] = int(st['union_largest'][4])
    assert got == {'later': 12, 'earlier': 18}          # the cavity first in C order joins the union, touching or not


@pytest.mark.parametrize('case', sorted(la_cases()))
def test_la_gate_constructed(case):
    seg, want = la_cases()[case]
    assert ref_la(seg, NAME) == want
    assert qc_gates.la_gate(qc_gates.plane_stats_host(seg[:, :, :1], 6), NAME) == want
    assert host_gate(seg[..., None], 'la_4ch', True, NAME) == want


@pytest.mark.parametrize('case', sorted(atrium_cases()))
def test_atrium_gate_constructed(case):
    seg, seq, want = atrium_cases()[case]
    assert ref_atrium(seg, qc_gates.ATRIUM_LABELS[seq]) == want
    assert host_gate(seg, seq, False, NAME) == want


# ---- 4. a random sweep ---------------------------------------------------------------------------------------------------------
def _blobs(rng, shape, classes, p_drop, speckle):
    """Blob-plus-speckle labels: per plane and class a box (sometimes missing, sometimes in two parts), then speckle."""
    X, Y, P = shape
    seg = np.zeros(shape, np.int32)
    for p in range(P):
        for k in classes:
            if rng.random() < p_drop:
                continue
            for _ in range(1 if rng.random() < 0.8 else 2):
                x0, y0 = rng.integers(0, X - 3), rng.integers(0, Y - 3)
                seg[x0:x0 + rng.integers(1, 7), y0:y0 + rng.integers(1, 7), p] = k
    sp = rng.random(shape) < speckle
    seg[sp] = rng.integers(0, max(classes) + 1, size=int(sp.sum()))
    return seg


def _key(msg):
    for k in ('smaller than', 'less than', 'missing', 'AHA', 'long-axis', 'area of', 'two connected', 'abrupt'):
        if k in msg:
            return k
    return 'pass' if msg == '' else msg


def test_random_sweep_equals_the_restatement():
    rng = np.random.default_rng(7)
    seen = {g: collections.Counter() for g in ('sa', 'la', 'atrium')}
    for i in range(150):
        Z = int(rng.integers(6, 11))
        seg = np.zeros((16, 14, Z), np.int32)
        mode = i % 6                                                            # healthy, a gap, few slices, no RV, crumbs, anything
        used = list(range(Z)) if mode != 2 else list(range(int(rng.integers(0, 3)), int(rng.integers(4, 8))))
        if mode == 1:
            used.remove(int(rng.integers(1, Z - 1)))
        for z in used:
            x0, y0, w = int(rng.integers(1, 4)), int(rng.integers(1, 4)), int(rng.integers(3, 6))
            seg[x0 - 1:x0 + w + 1, y0 - 1:y0 + w + 1, z] = 2
            seg[x0:x0 + w, y0:y0 + w, z] = 1
            if mode != 3 or rng.random() < 0.5:
                seg[11:11 + int(rng.integers(2, 5)), 2:2 + int(rng.integers(3, 7)), z] = 3
        if mode == 4:
            seg[rng.random(seg.shape) < 0.9] = 0
            if i % 12 == 4:
                seg[seg == rng.integers(1, 4)] = 0
        sp = rng.random(seg.shape) < rng.choice([0.0, 0.02, 0.1]) * (mode == 5 or i % 2)
        seg[sp] = rng.integers(0, 4, size=int(sp.sum()))
        got = host_gate(seg[..., None], 'sa', False, NAME)
        assert got == ref_sa(seg, NAME), i
        seen['sa'][_key(got[1])] += 1
    for i in range(120):
        seg = _blobs(rng, (16, 14, 1), (1, 2, 3, 4, 5), rng.choice([0.0, 0.0, 0.1]), rng.choice([0.0, 0.03, 0.15]))
        if i % 3 == 0:                                                          # cavity and myocardium in crumbs only
            crumbs = rng.random(seg.shape) < 0.25
            seg[(seg == 1) | (seg == 2)] = 0
            seg[crumbs & (seg == 0)] = rng.integers(1, 3, size=int((crumbs & (seg == 0)).sum()))
        got = host_gate(seg[..., None], 'la_4ch', True, NAME)
        assert got == ref_la(seg, NAME), i
        seen['la'][_key(got[1])] += 1
    for i in range(120):
        T, Z = int(rng.integers(2, 6)), int(rng.choice([1, 1, 2]))
        seq = ('la_2ch', 'la_4ch')[i % 2]
        seg = np.zeros((14, 12, Z, T), np.int32)
        x0, y0, w = rng.integers(0, 4), rng.integers(0, 4), rng.integers(4, 7)
        for t in range(T):
            grow = int(rng.integers(0, 2)) if i % 4 else int(rng.integers(0, 5))
            seg[x0:x0 + w + grow, y0:y0 + 4, 0, t] = 1
            seg[x0:x0 + 5, y0 + 6:y0 + 10 + grow // 2, Z - 1, t] = 2
        sp = rng.random(seg.shape) < rng.choice([0.0, 0.0, 0.01, 0.1])
        seg[sp] = rng.integers(0, 3, size=int(sp.sum()))
        if i % 5 == 0:
            seg[..., rng.integers(0, T)][seg[..., 0] == 1 + i % 2] = 0           # an empty frame (if the blob did not move)
        if i % 7 == 0:
            seg[10:13, 8:12, 0, rng.integers(0, T)] = 1 + i % 2                  # a second large piece
        got = host_gate(seg, seq, False, NAME)
        assert got == ref_atrium(seg, qc_gates.ATRIUM_LABELS[seq]), i
        seen['atrium'][_key(got[1])] += 1
    assert set(seen['sa']) == {'pass', 'smaller than', 'less than', 'missing', 'AHA'}, seen['sa']
    assert set(seen['la']) == {'pass', 'smaller than', 'long-axis'}, seen['la']
    assert set(seen['atrium']) == {'pass', 'area of', 'two connected', 'abrupt'}, seen['atrium']


# ---- 5. deploy_network.py --qc_csv on the host path -------------------------------------------------------------------------------
def cli_subjects(seq, seg4):
    """name -> (32, 48, Z, T) labels: subjects that pass and that fail the gate of this sequence."""
    kind = qc_gates.gate_kind(seq, seg4)

    def embed(v):                                                               # into the 32 x 48 frames the stub network sees
        out = np.zeros((32, 48) + v.shape[2:], np.int32)
        out[:v.shape[0], :v.shape[1]] = v
        return out
    if kind == 'sa':
        c = sa_cases()
        vols = {'1001': c['healthy'][0], '1002': c['one_slice_gap'][0], '1003': c['rv_largest_9'][0], '1004': c['five_slices'][0]}
        out = {}
        for n, v in vols.items():
            seq4 = np.repeat(embed(v)[..., None], 3, axis=3)
            seq4[..., 1:][seq4[..., 1:] == 1] = 0                               # only the ED frame decides
            out[n] = seq4
        return out
    if kind == 'la':
        c = la_cases()
        return {n: np.repeat(embed(c[k][0][:, :, :1])[..., None], 2, axis=3)
                for n, k in (('1001', 'healthy'), ('1002', 'RA_9'), ('1003', 'myo_component_9'), ('1004', 'RV_9'))}
    c = atrium_cases()
    names = ('healthy_4ch', 'ra_vanishes', 'two_pieces_of_11', 'wrap_ratio_2') if seq == 'la_4ch' else \
        ('healthy_2ch', 'la_vanishes', 'two_pieces_of_11', 'ratio_half')
    out = {}
    for i, k in enumerate(names):
        v = embed(c[k][0])
        if seq == 'la_2ch':
            v[v == 2] = 0                                                        # a two-class model
        out[str(1001 + i)] = v
    return out


def run_cli(tmp_path, seq, seg4, subjects, extra=(), csv_name='qc.csv', data=None):
    if data is None:
        data = tmp_path / 'data'
        data.mkdir()
        rng = np.random.default_rng(8)
        for n, lab in subjects.items():
            (data / n).mkdir()
            nifti.save(rng.uniform(10, 200, size=lab.shape).astype(np.float32), str(data / n / (seq + '.nii.gz')),
                       np.diag([1.8, 1.8, 10.0, 1.0]), np.array([1, 1.8, 1.8, 10, 0.03, 0, 0, 0], np.float32))
    state = {'subject': None}
    lines = []

    def log(*a):
        line = ' '.join(str(x) for x in a)
        lines.append(line)
        if line in subjects:
            state['subject'] = line

    def forward(batch):                                                        # the whole sequence in one call: [T*Z][32][48]
        lab = subjects[state['subject']]
        pred = np.ascontiguousarray(lab.transpose(3, 2, 0, 1).reshape((-1,) + lab.shape[:2]))
        assert pred.shape == batch.shape[:3]
        return {'pred': pred}
    out = str(tmp_path / csv_name)
    F, _ = D.define_flags().parse(['--seq_name', seq, '--data_dir', str(data), '--model_path', 'x', '--io_threads', '0', '--batch_slices', '1000',
                                   '--qc_csv', out] + (['--seg4'] if seg4 else []) + list(extra))
    D.run(F, forward, log=log)
    return data, out, lines


@pytest.mark.parametrize('seq,seg4', [('sa', False), ('la_4ch', True), ('la_2ch', False), ('la_4ch', False)])
def test_cli_writes_the_verdicts(tmp_path, seq, seg4):
    subjects = cli_subjects(seq, seg4)
    data, out, lines = run_cli(tmp_path, seq, seg4, subjects)
    gate = qc_gates.gate_name(seq, seg4)
    want_rows, want_msgs = [], []
    for n in sorted(subjects):
        name = '{0}/{1}'.format(data / n, qc_gates.seg_file_name(seq, seg4))
        ok, msg = ref_gate(subjects[n], seq, seg4, name)
        want_rows.append([n, gate, str(ok), msg])
        if not ok:
            want_msgs.append(msg)
    import csv
    text = open(out).read()
    assert list(csv.reader(text.splitlines())) == [['', 'gate', 'passed', 'message']] + want_rows
    assert [r[2] for r in want_rows].count('False') == 3 and want_rows[0][2] == 'True'
    assert len(set(want_msgs)) == 3 and [l for l in lines if l in want_msgs] == want_msgs      # each logged once, in subject order
    assert 'Quality-control verdicts of 4 subjects written to ' + out in lines
    # a second run finds every subject segmented and gates the files: the same table
    _, out2, lines2 = run_cli(tmp_path, seq, seg4, subjects, csv_name='again.csv', data=data)
    assert open(out2).read() == text and not any('Segmenting' in l for l in lines2)
    assert [l for l in lines2 if l in want_msgs] == want_msgs


def test_cli_shards_and_nosave(tmp_path):
    from ukbb_cardiac_amd import measures
    subjects = cli_subjects('sa', False)
    data, out, _ = run_cli(tmp_path, 'sa', False, subjects, extra=['--nosave_seg'])
    text = open(out).read()                                                    # written without any segmentation file
    assert text.count('\n') == 5 and not any(f.startswith('seg') for n in subjects for f in __import__('os').listdir(str(data / n)))
    for i in range(2):
        run_cli(tmp_path, 'sa', False, subjects, extra=['--nosave_seg', '--num_shards', '2', '--shard_index', str(i), '--nowork_stealing'],
                csv_name='sharded.csv', data=data)
    parts = [open(measures.shard_csv_name(str(tmp_path / 'sharded.csv'), i, 2)).read().splitlines() for i in range(2)]
    assert len(parts[0]) == len(parts[1]) == 3
    assert measures.merge_shard_csv(str(tmp_path / 'sharded.csv'), 2)
    assert open(str(tmp_path / 'sharded.csv')).read() == text


def test_flag_needs_sequence_mode_and_defaults_to_off(tmp_path):
    F, _ = D.define_flags().parse(['--data_dir', str(tmp_path)])
    assert F.qc_csv == '' and '--qc_csv' in D.define_flags().usage()
    F, _ = D.define_flags().parse(['--data_dir', str(tmp_path), '--qc_csv', str(tmp_path / 'q.csv'), '--noprocess_seq'])
    with pytest.raises(ValueError, match='sequence mode'):
        D.run(F, lambda b: None, log=lambda *a: None)


def test_atrium_gate_reads_what_label_components_counts():
    """n_large of the atrial gate is aorta_qc.count_large_components with min_size 10 -- the host twin of
    ukbb_fcn_label_components -- on any class count."""
    seg, _, _ = atrium_cases()['two_pieces_of_11']
    st = qc_gates.stats_host(seg, 'la_2ch')
    assert st['n_large'].shape == (5, 2) and st['n_large'][:, 1].tolist() == [1, 1, 1, 3, 1]
    assert np.array_equal(st['n_large'], aorta_qc.count_large_components(seg, 2, 10))
