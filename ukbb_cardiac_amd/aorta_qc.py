"""All five criteria of cardiac_utils.aorta_pass_quality_control (reference common/cardiac_utils.py:1739-1796, applied by
aortic/eval_aortic_area.py:68-69), from three statistics of the cine and its label map:

  ``n_large [T, n_class]``  components of ``seg_t == k`` with more than 10 voxels (criterion 3: skimage.measure.label with
                            connectivity 2 = 18-neighbourhood in 3-D, no connectivity across frames)
  ``max [T, n_class]``      ``np.max(image_t[seg_t == k])`` as float64 (exact for every voxel type; NaN propagated; -inf for
                            an empty mask)
  ``mean_ed [n_class]``     ``image_ED[seg_ED == k].mean()`` in numpy's result dtype (float32 for a float32 image, float64 for
                            an integer one; NaN for an empty mask; column 0 is not computed and holds NaN)

``device_pipeline.device_qc_stats`` computes them on the GPU from the cine and the labels already there (``qc=True`` of
``device_pipeline.aortic_sequence_device``); ``stats_host`` computes the same numbers in numpy for the host path.
``aorta_qc_full`` turns them and the per-frame class counts into the script's verdict and message."""
import warnings

import numpy as np

from . import measures

PIXEL_THRES = 10                                       # cardiac_utils.py:1767: a component counts with MORE than this many voxels
RATIO_THRES = 3                                        # :1756: the frame is noisy when max_t / mean_ED >= this


def _half_neighbourhood(Z):
    """Offsets (dx, dy, dz) of the half 18-neighbourhood: every unordered neighbour pair appears once."""
    offs = [(-1, 0, 0), (-1, -1, 0), (0, -1, 0), (1, -1, 0)]
    if Z > 1:
        offs += [(0, 0, -1), (-1, 0, -1), (1, 0, -1), (0, -1, -1), (0, 1, -1)]
    return offs


def _components(seg):
    """Root (smallest flat index, NIfTI order) of the 18-connected component of every voxel of the (X,Y,Z,T) label volume,
    a voxel uniting only with neighbours of its own non-zero label and frame.  Union by vectorised min-hooking and pointer
    jumping over the edge list; background voxels are their own roots."""
    X, Y, Z, T = seg.shape
    seg = np.asarray(seg)
    lab = seg.reshape(-1, order='F')
    idx = np.arange(lab.size, dtype=np.int64).reshape((X, Y, Z, T), order='F')
    us, vs = [], []
    for dx, dy, dz in _half_neighbourhood(Z):         # voxel a and its neighbour b = a + (dx, dy, dz), both inside the frame
        sa = (slice(max(0, -dx), X - max(0, dx)), slice(max(0, -dy), Y - max(0, dy)), slice(max(0, -dz), Z - max(0, dz)))
        sb = (slice(max(0, dx), X + min(0, dx)), slice(max(0, dy), Y + min(0, dy)), slice(max(0, dz), Z + min(0, dz)))
        la = seg[sa]
        keep = (la == seg[sb]) & (la != 0)
        us.append(idx[sa][keep])
        vs.append(idx[sb][keep])
    u, v = np.concatenate(us), np.concatenate(vs)
    parent = np.arange(lab.size, dtype=np.int64)
    nodes = np.unique(np.concatenate([u, v]))          # every root a hook touches is one of these: jump over them only
    while u.size:
        pu, pv = parent[u], parent[v]
        lo, hi = np.minimum(pu, pv), np.maximum(pu, pv)
        differ = lo != hi
        if not differ.any():
            break
        u, v = u[differ], v[differ]                    # edges inside one tree stay there
        np.minimum.at(parent, hi[differ], lo[differ])  # hook roots onto smaller roots: parent[i] <= i, no cycles
        while True:                                    # pointer jumping: every voxel onto its root
            pn = parent[nodes]
            pp = parent[pn]
            if np.array_equal(pp, pn):
                break
            parent[nodes] = pp
    return lab, parent


def count_large_components(seg, n_class=3, min_size=PIXEL_THRES):
    """n_large [T, n_class] (int32): components of seg[..., t] == k with more than min_size voxels, k >= 1; column 0 is 0."""
    seg = np.asarray(seg)
    X, Y, Z, T = seg.shape
    lab, root = _components(seg)
    n_large = np.zeros((T, n_class), np.int32)
    fg = np.flatnonzero((lab != 0) & (lab < n_class))
    size = np.bincount(root[fg], minlength=lab.size)
    big = np.flatnonzero(size > min_size)              # only roots have a size
    np.add.at(n_large, (big // (X * Y * Z), lab[big].astype(np.int64)), 1)
    return n_large


def stats_host(image, seg, n_class=3):
    """The three statistics of the module docstring for an (X,Y,Z,T) image and its label map, in numpy (any voxel type)."""
    image, seg = np.asarray(image), np.asarray(seg)
    T = seg.shape[3]
    mx = np.empty((T, n_class), np.float64)
    for k in range(n_class):
        masked = np.where(seg == k, image, -np.inf)    # NaN under the mask stays NaN: np.max propagates it
        mx[:, k] = np.max(masked.reshape(-1, T, order='F'), axis=0)
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)                  # the mean of an empty mask: NaN
        rt = np.mean(image[..., 0][:0]).dtype                            # numpy's result dtype of .mean()
        means = [rt.type(np.nan)]                                        # column 0 (background): not computed
        for k in range(1, n_class):
            means.append(image[..., 0][seg[..., 0] == k].mean())         # cardiac_utils.py:1753-1755, numpy itself
    mean_ed = np.array(means, dtype=rt)
    return {'n_large': count_large_components(seg, n_class), 'max': mx, 'mean_ed': mean_ed}


def aorta_qc_full(counts, stats):
    """(passed, message) of cardiac_utils.aorta_pass_quality_control: per label (AAo = 1, then DAo = 2) criteria 1 (zero area),
    2 (max_t / mean_ED >= 3: 'noisy'), 3 (two or more components of more than 10 voxels), 4 (abrupt change between adjacent
    frames) and 5 (max / min area >= 2), in that order; the message is the script's for the first failing criterion.
    counts [T, >= 3]: voxels per class and frame; stats: what stats_host / device_pipeline.device_qc_stats return."""
    counts = np.asarray(counts)
    T = counts.shape[0]
    mean_ed, mx, n_large = stats['mean_ed'], np.asarray(stats['max']), np.asarray(stats['n_large'])
    for l in (1, 2):
        alone = np.ones_like(counts)                   # the other label constant: it passes 1, 4 and 5
        alone[:, l] = counts[:, l]
        ok, why = measures.aorta_qc_from_counts(alone)  # criteria 1, 4 and 5 of this label, the script's messages
        if not ok and (counts[:, l] == 0).any():
            return False, why                          # criterion 1 comes before 2 and 3
        # criterion 2: max_intensity_t / mean_intensity_ED in numpy's type (float32 / float32 for a float32 image, integer /
        # float64 for an integer one: float64); the maximum converts exactly.  A NaN ratio is not >= 3.
        mean = mean_ed[l]
        with np.errstate(all='ignore'):
            ratio = mx[:, l].astype(mean.dtype) / mean
        for t in range(T):
            if ratio[t] >= RATIO_THRES:
                return False, 'The image becomes very noisy at time frame {0}.'.format(t)
        for t in range(T):                             # criterion 3
            if n_large[t, l] >= 2:
                return False, ('The segmentation has at least two connected components with more than {0} pixels '
                               'at time frame {1}.'.format(PIXEL_THRES, t))
        if not ok:
            return False, why                          # criteria 4, 5
    return True, ''
