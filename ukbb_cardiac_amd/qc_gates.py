"""The three quality-control gates of the reference that read nothing but a label map, from statistics the deploy run has
at hand (deploy_network.py --qc_csv):

  ``sa_gate``      cardiac_utils.sa_pass_quality_control (reference common/cardiac_utils.py:77-136), applied to seg_sa_ED
                   before eval_wall_thickness.py and eval_strain_sax.py
  ``la_gate``      cardiac_utils.la_pass_quality_control (:139-169), applied to seg4_la_4ch_ED before eval_strain_lax.py
  ``atrium_gate``  cardiac_utils.atrium_pass_quality_control (:1616-1652), applied to seg_la_2ch ({'LA': 1}) and seg_la_4ch
                   ({'LA': 1, 'RA': 2}) by eval_atrial_volume.py

The first two work on the plane statistics of ``plane_stats_host`` / ``device_pipeline.device_plane_stats``
(ukbb_fcn_plane_components), int32 and exact:

  ``count [P, n_class]``    voxels of class k on plane p
  ``largest [P, n_class]``  size of the largest 8-connected component of plane == k (get_largest_cc, image_utils.py:227-238)
  ``kept [P, n_class]``     voxels in components of plane == k with at least keep_min voxels (remove_small_cc, :241-249)
  ``union_largest [P]``     size of the largest component of (largest component of class a) | (kept components of class b):
                            ``epi`` of cardiac_utils.py:123-128 and :158-163

get_largest_cc takes the first label of the strictly greatest area, and skimage numbers labels by each component's first voxel
in a C-order scan of the [x][y] array (y fastest): of two equal-largest class-a components the one with the smaller least
x*Y + y joins the union.  The third gate needs the per-frame class counts and the count of components with more than 10 voxels
that ukbb_fcn_label_components / aorta_qc.count_large_components already give."""
import csv
import io
import os

import numpy as np

from . import aorta_qc, measures

PIXEL_THRES = 10                                       # every pixel threshold of the three functions
SLICE_THRES = 6                                        # cardiac_utils.py:107
SA_LABELS = (('LV', 1), ('Myo', 2), ('RV', 3))         # :84
LA_LABELS = SA_LABELS + (('LA', 4), ('RA', 5))         # :147
ATRIUM_LABELS = {'la_2ch': {'LA': 1}, 'la_4ch': {'LA': 1, 'RA': 2}}   # eval_atrial_volume.py
COLUMNS = ['gate', 'passed', 'message']


def plane_stats_host(planes, n_class, a=1, b=2, keep_min=PIXEL_THRES):
    """The four statistics of the module docstring for an (X, Y, P) array of label planes, in numpy: the union-find of
    aorta_qc._components with every plane a frame of one slice (8-connectivity, nothing across planes)."""
    planes = np.asarray(planes)
    if planes.ndim == 2:
        planes = planes[:, :, None]
    X, Y, P = planes.shape
    n = X * Y * P
    lab, root = aorta_qc._components(planes.reshape(X, Y, 1, P))
    first_of = (np.arange(X, dtype=np.int64)[:, None, None] * Y + np.arange(Y, dtype=np.int64)[None, :, None]
                + np.zeros((1, 1, P), np.int64)).reshape(-1, order='F')          # x*Y + y of every voxel, NIfTI order
    fg = np.flatnonzero((lab != 0) & (lab < n_class))
    size = np.bincount(root[fg], minlength=n)
    first = np.full(n, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(first, root[fg], first_of[fg])
    roots = fg[root[fg] == fg]
    cell = (roots // (X * Y), lab[roots].astype(np.int64))
    count = np.zeros((P, n_class), np.int64)
    kept = np.zeros((P, n_class), np.int64)
    best = np.zeros((P, n_class), np.int64)
    np.add.at(count, cell, size[roots])
    big = size[roots] >= keep_min
    np.add.at(kept, (cell[0][big], cell[1][big]), size[roots][big])
    np.maximum.at(best, cell, (size[roots] << 32) | (0xFFFFFFFF - first[roots]))      # largest, then earliest in scan order
    plane_of = np.arange(n, dtype=np.int64) // (X * Y)
    win_first = 0xFFFFFFFF - (best[:, a] & 0xFFFFFFFF)
    mask = ((lab == a) & (best[plane_of, a] != 0) & (first[root] == win_first[plane_of])) | ((lab == b) & (size[root] >= keep_min))
    mlab, mroot = aorta_qc._components(mask.reshape((X, Y, 1, P), order='F').astype(np.uint8))
    mfg = np.flatnonzero(mlab)
    msize = np.bincount(mroot[mfg], minlength=n)
    union_largest = np.zeros(P, np.int64)
    np.maximum.at(union_largest, mfg // (X * Y), msize[mfg])
    return {'count': count.astype(np.int32), 'largest': (best >> 32).astype(np.int32), 'kept': kept.astype(np.int32),
            'union_largest': union_largest.astype(np.int32)}


def sa_gate(stats, name):
    """(passed, message) of sa_pass_quality_control from the plane statistics of the Z planes of the ED frame; ``name`` stands
    where the function prints the file name."""
    count = np.asarray(stats['count']).astype(np.int64)
    Z = count.shape[0]
    for l_name, l in SA_LABELS:                        # criterion 1: the 3-D totals, in dict order
        if count[:, l].sum() < PIXEL_THRES:
            return False, ('{0}: The segmentation for class {1} is smaller than {2} pixels. '
                           'It does not pass the quality control.'.format(name, l_name, PIXEL_THRES))
    z_pos = [z for z in range(Z) if count[z, 1] >= PIXEL_THRES and count[z, 2] >= PIXEL_THRES]      # criterion 2
    if len(z_pos) < SLICE_THRES:
        return False, ('{0}: The segmentation has less than {1} slices. '
                       'It does not pass the quality control.'.format(name, SLICE_THRES))
    if len(z_pos) != z_pos[-1] - z_pos[0] + 1:
        return False, ('{0}: There is missing segmentation between the slices. '
                       'It does not pass the quality control.'.format(name))
    # criterion 3: np.mean of the z indices of the LV voxels (float64: an exact integer sum over an exact count), then round
    # half to even as round() of a numpy float64 does
    cz = np.float64((np.arange(Z, dtype=np.int64) * count[:, 1]).sum()) / np.float64(count[:, 1].sum())
    z = int(round(cz))
    if stats['union_largest'][z] < PIXEL_THRES or stats['largest'][z, 3] < PIXEL_THRES:
        return False, ('{0}: Can not find LV epi or RV to determine the AHA '
                       'coordinate system.'.format(name))
    return True, ''


def la_gate(stats, name):
    """(passed, message) of la_pass_quality_control from the plane statistics (n_class 6) of plane 0 of the ED frame."""
    count = np.asarray(stats['count'])
    for l_name, l in LA_LABELS:
        if count[0, l] < PIXEL_THRES:
            return False, ('{0}: The segmentation for class {1} is smaller than {2} pixels. '
                           'It does not pass the quality control.'.format(name, l_name, PIXEL_THRES))
    if stats['largest'][0, 1] < PIXEL_THRES or stats['kept'][0, 2] < PIXEL_THRES or stats['union_largest'][0] < PIXEL_THRES:
        return False, ('{0}: Can not find LV endo, myo or epi to extract the long-axis '
                       'myocardial contour.'.format(name))
    return True, ''


def atrium_gate(counts, n_large, label_dict):
    """(passed, message) of atrium_pass_quality_control.  counts [T, n_class]: voxels per class and frame; n_large [T, n_class]:
    components of frame t == k with MORE than 10 voxels (connectivity 2 in 3-D: ukbb_fcn_label_components with min_size 10, or
    aorta_qc.count_large_components)."""
    counts, n_large = np.asarray(counts), np.asarray(n_large)
    T = counts.shape[0]
    for l_name, l in label_dict.items():
        A = counts[:, l]
        for t in range(T):
            if A[t] == 0:
                return False, 'The area of {0} is 0 at time frame {1}.'.format(l_name, t)
        for t in range(T):
            if n_large[t, l] >= 2:
                return False, ('The segmentation has at least two connected components with more than {0} pixels '
                               'at time frame {1}.'.format(PIXEL_THRES, t))
        for t in range(T):
            ratio = A[t] / float(A[t - 1])             # t = 0 against the LAST frame, as the script's A[t - 1]
            if ratio >= 2 or ratio <= 0.5:
                return False, 'There is abrupt change of area at time frame {0}.'.format(t)
    return True, ''


# ---- which gate a sequence gets, and the statistics it needs ----------------------------------------------------------------
def gate_kind(seq_name, seg4=False):
    """'sa' | 'la' | 'atrium': the gate the reference applies to the segmentation of this sequence."""
    if seq_name == 'sa':
        return 'sa'
    if seq_name == 'la_4ch' and seg4:
        return 'la'
    return 'atrium'


def gate_name(seq_name, seg4=False):
    """The gate column of the table: the reference function's name."""
    return {'sa': 'sa_pass_quality_control', 'la': 'la_pass_quality_control',
            'atrium': 'atrium_pass_quality_control'}[gate_kind(seq_name, seg4)]


def min_classes(seq_name, seg4=False):
    """Classes the gate reads (the n_class of the model that segments the sequence)."""
    return {'sa': 4, 'la': 6}.get(gate_kind(seq_name, seg4), 1 + max(ATRIUM_LABELS.get(seq_name, {'LA': 1}).values()))


def stats_host(seg, seq_name, seg4=False, n_class=None):
    """What the gate of this sequence reads, from an (X,Y,Z,T) label volume in numpy: the host twin of
    device_pipeline.device_gate_stats."""
    seg = np.asarray(seg)
    kind = gate_kind(seq_name, seg4)
    n_class = max(min_classes(seq_name, seg4), n_class or 0)
    if kind == 'sa':
        return plane_stats_host(seg[:, :, :, 0], n_class)
    if kind == 'la':
        return plane_stats_host(seg[:, :, :1, 0], n_class)
    return {'counts': measures.counts_from_labels(seg, n_class),
            'n_large': aorta_qc.count_large_components(seg, n_class, PIXEL_THRES)}


def gate_from_stats(stats, seq_name, seg4, name):
    """(passed, message) of this sequence's gate from stats_host / device_pipeline.device_gate_stats."""
    kind = gate_kind(seq_name, seg4)
    if kind == 'sa':
        return sa_gate(stats, name)
    if kind == 'la':
        return la_gate(stats, name)
    return atrium_gate(stats['counts'], stats['n_large'], ATRIUM_LABELS[seq_name])


def seg_file_name(seq_name, seg4=False):
    """The file the reference hands to the gate (it is the ED frame of the sequence for the first two)."""
    pre = 'seg4' if (seq_name == 'la_4ch' and seg4) else 'seg'
    return '{0}_{1}.nii.gz'.format(pre, seq_name) if gate_kind(seq_name, seg4) == 'atrium' else '{0}_{1}_ED.nii.gz'.format(pre, seq_name)


def write_csv(path, seq_name, seg4, rows):
    """rows: [(subject, (passed, message))] -> index of subject names, columns gate / passed / message.  Written under a
    temporary name and renamed, as measures.write_csv."""
    buf = io.StringIO()
    wr = csv.writer(buf, lineterminator='\n')
    wr.writerow([''] + COLUMNS)
    gate = gate_name(seq_name, seg4)
    for subject, (passed, message) in rows:
        wr.writerow([subject, gate, 'True' if passed else 'False', message])
    tmp = '%s.tmp.%d' % (path, os.getpid())
    with open(tmp, 'w', newline='') as f:
        f.write(buf.getvalue())
    os.replace(tmp, path)
