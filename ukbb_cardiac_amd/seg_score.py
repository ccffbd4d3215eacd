"""How good is a segmentation: Dice, mean contour distance and Hausdorff distance of a label volume against a second one (manual
annotations, another tool's seg_*.nii.gz), per subject, frame and class -- the three numbers of the paper's accuracy tables, by the
arithmetic of the reference's ``np_categorical_dice`` (common/image_utils.py:171-175) and ``distance_metric`` (:178-224).

``stats_host`` is the specification; ukbb_fcn_score_planes (csrc/kernels_score.hip) computes the same integers and the same two
float64 sums on the device.  For every plane p = z + Z*t of two (X,Y,Z,T) uint8 volumes and every class k >= 1, with
A = pred plane == k and B = truth plane == k:

    nA, nB, nAB   |A|, |B|, |A & B|
    C(M)          the contour set of a mask: the pixels of M with at least one 4-neighbour off the image or in the OUTER background,
                  the non-M pixels 4-connected to the image frame (an imaginary one-pixel ring of background around the plane).
                  Holes are not outer background -- a ring contributes its outer border only, an island inside a hole nothing --
                  and a background pocket that touches the outside only diagonally is not outer: foreground is 8-connected, so
                  background is 4-connected.
    mA(a)         min over b in C(B) of (ax - bx)^2 + (ay - by)^2 for a in C(A), int32; mB(b) likewise
    cA, cB        |C(A)|, |C(B)|;  hA, hB = max mA, max mB
    sA, sB        np.add.reduce(np.sqrt(float64(mA))) with the points in the order x*Y + y (numpy's pairwise tree); sB likewise
    status        1 when nA > 0 and nB > 0 -- the distance is defined only when both contours exist -- else 0 and cA .. sB are zero

``frame_rows`` forms the tables as the reference does: per slice md = 0.5 * (sA/cA + sB/cB) * dx and hd = sqrt(max(hA, hB)) * dx,
dx = pixdim[1]; per frame and class np.mean over the defined slices (empty where there is none: the reference returns None);
Dice = 2*nAB / (nA + nB) over the frame's volume in float32 as np_categorical_dice (empty when nA + nB == 0).  Frames whose truth
volume holds no non-zero label -- the un-annotated frames of a label_sa.nii.gz -- give no rows.

NOT PINNED.  OpenCV is not a dependency and was not at hand: C(M) restates from memory the set of pixels
cv2.findContours(..., RETR_EXTERNAL, CHAIN_APPROX_NONE) visits (like atrial.line_pixels for cv2.line), and
tests/test_seg_score.py checks it against a sequential Suzuki border follower, against OpenCV only where cv2 imports.  OpenCV's
follower emits a pixel once per visit, so the pixels of one-pixel-wide parts appear twice in its point list: the reference's mean
distance weights them twice, this module weights every contour pixel once.  The Hausdorff distance is a maximum over the set and
depends on neither multiplicity nor order.
"""
import numpy as np

from . import measures

MAX_CLASSES = 16
SCORE_COLUMNS = ['frame', 'label', 'Dice', 'MCD (mm)', 'HD (mm)', 'n_slices']
_PAIR_CHUNK = 1 << 22                                   # entries of the distance matrix formed at a time


def _fill_runs(seed, free):
    """``seed`` spread along the runs of ``free`` on the last axis: a free pixel is set when its run holds a seed."""
    start = np.ones(free.shape, bool)
    start[..., 1:] = free[..., 1:] != free[..., :-1]
    ids = np.cumsum(start.ravel()) - 1
    hit = np.bincount(ids, weights=seed.ravel(), minlength=int(ids[-1]) + 1) > 0
    return free & hit[ids].reshape(free.shape)


def outer_background(mask):
    """The non-mask pixels 4-connected to the image frame, of a boolean [..., X, Y] stack of planes: run fills along y and along x
    from the frame pixels until nothing changes (every 4-path is a chain of runs)."""
    mask = np.asarray(mask, bool)
    free = ~mask
    outer = np.zeros(mask.shape, bool)
    outer[..., 0, :] = outer[..., -1, :] = outer[..., :, 0] = outer[..., :, -1] = True
    outer &= free
    free_t = np.ascontiguousarray(np.swapaxes(free, -1, -2))
    while True:
        grown = _fill_runs(outer, free)
        grown = np.swapaxes(_fill_runs(np.ascontiguousarray(np.swapaxes(grown, -1, -2)), free_t), -1, -2)
        if np.array_equal(grown, outer):
            return outer
        outer = np.ascontiguousarray(grown)


def contour_mask(mask):
    """C(M) of a boolean [..., X, Y] stack of planes, as a mask."""
    mask = np.asarray(mask, bool)
    outer = np.pad(outer_background(mask), [(0, 0)] * (mask.ndim - 2) + [(1, 1), (1, 1)], constant_values=True)   # the frame
    near = outer[..., :-2, 1:-1] | outer[..., 2:, 1:-1] | outer[..., 1:-1, :-2] | outer[..., 1:-1, 2:]
    return mask & near


def min_sq_distances(pts_a, pts_b):
    """mA: for every point of pts_a [n, 2] the smallest squared distance to a point of pts_b [m, 2], int32."""
    pts_a, pts_b = np.asarray(pts_a, np.int32), np.asarray(pts_b, np.int32)
    out = np.empty(len(pts_a), np.int32)
    step = max(1, _PAIR_CHUNK // max(1, len(pts_b)))
    for i in range(0, len(pts_a), step):
        d = pts_a[i:i + step, None, :] - pts_b[None, :, :]
        out[i:i + step] = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).min(axis=1)
    return out


def stats_host(pred, truth, n_class):
    """{'shape': (X,Y,Z,T), 'cells': int32 [P, n_class, 8] = status, nA, nB, nAB, cA, cB, hA, hB; 'sums': float64 [P, n_class, 2] =
    sA, sB} of two (X,Y,Z,T) label volumes, P = Z*T planes p = z + Z*t (see the module docstring).  Class 0 cells are zero; labels
    >= n_class are ignored."""
    pred, truth = np.asarray(pred), np.asarray(truth)
    if pred.ndim != 4 or pred.shape != truth.shape:
        raise ValueError('expected two (X,Y,Z,T) label volumes of one shape, got %s and %s' % (pred.shape, truth.shape))
    if not 2 <= n_class <= MAX_CLASSES:
        raise ValueError('n_class %d: label maps of 2 to %d classes are scored' % (n_class, MAX_CLASSES))
    X, Y, Z, T = pred.shape
    P = Z * T
    a_all = np.ascontiguousarray(np.moveaxis(pred.reshape(X, Y, P, order='F'), 2, 0))     # [P, X, Y], p = z + Z*t
    b_all = np.ascontiguousarray(np.moveaxis(truth.reshape(X, Y, P, order='F'), 2, 0))
    cells = np.zeros((P, n_class, 8), np.int32)
    sums = np.zeros((P, n_class, 2), np.float64)
    for k in range(1, n_class):
        A, B = a_all == k, b_all == k
        cells[:, k, 1] = A.sum(axis=(1, 2))
        cells[:, k, 2] = B.sum(axis=(1, 2))
        cells[:, k, 3] = (A & B).sum(axis=(1, 2))
        defined = np.nonzero((cells[:, k, 1] > 0) & (cells[:, k, 2] > 0))[0]
        if not len(defined):
            continue
        CA, CB = contour_mask(A[defined]), contour_mask(B[defined])
        for i, p in enumerate(defined):
            pts_a, pts_b = np.argwhere(CA[i]), np.argwhere(CB[i])          # C order of the [x][y] plane: x*Y + y ascending
            m_a, m_b = min_sq_distances(pts_a, pts_b), min_sq_distances(pts_b, pts_a)
            cells[p, k] = (1, cells[p, k, 1], cells[p, k, 2], cells[p, k, 3], len(pts_a), len(pts_b), m_a.max(), m_b.max())
            sums[p, k] = (np.add.reduce(np.sqrt(m_a.astype(np.float64))), np.add.reduce(np.sqrt(m_b.astype(np.float64))))
    return {'shape': (X, Y, Z, T), 'cells': cells, 'sums': sums}


def slice_distances(cells, sums, dx):
    """(md, hd) of one defined cell, as distance_metric forms them for a slice: np.mean(np.min(M, axis)) = sum / count."""
    s_a, s_b = np.float64(sums[0]), np.float64(sums[1])
    md = 0.5 * (s_a / int(cells[4]) + s_b / int(cells[5])) * dx
    hd = np.sqrt(np.float64(max(int(cells[6]), int(cells[7])))) * dx
    return md, hd


def frame_rows(stats, pixdim):
    """The --score_csv lines of one subject: [frame, label, Dice, MCD (mm), HD (mm), n_slices] per (annotated frame, label >= 1)."""
    X, Y, Z, T = stats['shape']
    cells = np.asarray(stats['cells']).reshape(T, Z, -1, 8)
    sums = np.asarray(stats['sums']).reshape(T, Z, -1, 2)
    n_class = cells.shape[2]
    dx = pixdim[1]
    nan = float('nan')
    rows = []
    for t in range(T):
        # a truth label >= n_class is refused before it gets here, so the frame is annotated iff some class >= 1 has truth pixels
        if not cells[t, :, 1:, 2].any():
            continue
        for k in range(1, n_class):
            n_a, n_b, n_ab = (int(cells[t, :, k, j].sum(dtype=np.int64)) for j in (1, 2, 3))
            assert max(n_a, n_b) < 1 << 24, 'class counts of a frame beyond 2^24: float32 sums are no longer exact'
            dice = nan
            if n_a + n_b:                                  # np_categorical_dice: float32 sums of 0/1 values, exact below 2^24
                dice = float(2 * np.float32(n_ab) / (np.float32(n_a) + np.float32(n_b)))
            table = [slice_distances(cells[t, z, k], sums[t, z, k], dx) for z in range(Z) if cells[t, z, k, 0]]
            md = float(np.mean([v[0] for v in table])) if table else nan
            hd = float(np.mean([v[1] for v in table])) if table else nan
            rows.append([t, k, dice, md, hd, len(table)])
    return rows


def check_truth(truth, shape, n_class):
    """The truth volume of one subject as uint8, or a ValueError saying why it cannot be scored against labels of ``shape``."""
    truth = np.asarray(truth)
    if truth.shape != tuple(shape):
        raise ValueError('shape %s, the image has %s' % (truth.shape, tuple(shape)))
    if truth.dtype.kind == 'f':
        if not np.all(np.isfinite(truth)) or np.any(truth != np.floor(truth)):
            raise ValueError('labels are not integers')
    elif truth.dtype.kind not in 'iub':
        raise ValueError('labels of type %s' % truth.dtype)
    lo, hi = (truth.min(), truth.max()) if truth.size else (0, 0)
    if lo < 0 or hi >= n_class:
        raise ValueError('label %d outside 0..%d' % (int(hi if hi >= n_class else lo), n_class - 1))
    return np.asfortranarray(truth.astype(np.uint8))


def write_csv(path, rows):
    """rows: [(subject, [SCORE_COLUMNS values])], one per (subject, frame, label): the text pandas' to_csv writes for them."""
    from .atrial import write_frames_csv
    write_frames_csv(path, rows, SCORE_COLUMNS)


def merge_csv(path, num_shards, remove=True):
    """measures.merge_shard_csv for a --score_csv file: sorted by (subject, frame, label)."""
    return measures.merge_shard_csv(path, num_shards, remove, key_columns=3)
