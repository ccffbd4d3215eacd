"""How sure was the network: per subject, frame and class, reductions of the softmax the forward forms next to the label map -- the mean
winning probability, the mean margin to the runner-up, the share of low-confidence voxels and the soft volume -- for the
``--confidence_csv`` table of deploy_network.py and deploy_network_ao.py.

``cells_host`` is the specification; ukbb_fcn_confidence_cells (csrc/kernels_conf.hip) computes the same integers on the device while
the probabilities of a chunk of slices are in HBM.  No float is ever summed.  For a float32 probability p

    q(p) = (int)(p * 65536.0f)      the multiply by a power of two is exact and the conversion truncates: 0 <= q <= 65536; a denormal p
                                    gives 0 whether or not the multiply flushes it, and so does a NaN (a frame of a cine that no window
                                    reaches: deploy_network_ao.py --time_step)

and for a voxel with label c = pred -- in every forward of the engine the lowest-index argmax of the float32 probabilities --

    q1 = q(p[c]),    q2 = max over c' != c of q(p[c']),    margin = q1 - q2 >= 0

Per (frame t, class c) a cell of 20 unsigned 64-bit integers:

    0       n: the voxels of the frame with pred == c
    1       the sum of q1 over those voxels
    2       the sum of margin over those voxels (added as a signed 64-bit number: labels that are not the argmax, which no forward
            produces, may make it negative)
    3..18   the histogram of min(q1 >> 12, 15) over those voxels: 16 bins of width 1/16, p == 1 in the last
    19      the soft count: the sum of q(p[c]) over ALL voxels of the frame

Only the image region counts, not the padding the network input adds; the frame of slice b of the batch [T*Z][X2][Y2] is b // Z.  A
voxel whose label lies outside 0 .. n_class - 1 counts in field 19 only.  Integer sums do not depend on their order: the cells are the
same whatever chunks of slices they are added from.

``frame_rows`` turns the cells of a subject into table lines; every division is float64, from the integers.
"""
import numpy as np

FIELDS = 20
MAX_CLASSES = 16
CONF_COLUMNS = ['frame', 'label', 'n', 'mean_conf', 'mean_margin', 'frac_below_0.5', 'frac_below_0.75', 'soft_n']
ALL_FRAMES = 'all'


def quantise(prob):
    """q(p) of a float32 array, int64."""
    prob = np.asarray(prob)
    if prob.dtype != np.float32:
        raise TypeError('probabilities are float32 (got %s): q(p) is defined on the float32 value' % prob.dtype)
    with np.errstate(invalid='ignore'):
        x = prob * np.float32(65536.0)                    # float32: exact but for denormals, which give less than 1 either way
        return np.where(x == x, x, np.float32(0)).astype(np.int64)


def new_cells(T, n_class):
    return np.zeros((T, n_class, FIELDS), np.uint64)


def cells_host(prob, pred, shape, pad=None, first_slice=0, cells=None):
    """The cells [T, n_class, 20] uint64 of n slices of the network's batch: prob [n, X2, Y2, C] float32 and pred [n, X2, Y2] integer,
    the first of them slice ``first_slice`` of the subject's [T*Z] slices.  shape = (X, Y, Z, T) of the subject; pad = (X2, Y2, x_pre,
    y_pre) as the batch was padded (None: not at all).  Added into ``cells`` when given (chunk after chunk), else into zeros."""
    X, Y, Z, T = (int(v) for v in shape)
    prob, pred = np.asarray(prob), np.asarray(pred)
    X2, Y2, x_pre, y_pre = (X, Y, 0, 0) if pad is None else (int(v) for v in pad)
    if prob.ndim != 4 or pred.shape != prob.shape[:3] or prob.shape[1:3] != (X2, Y2):
        raise ValueError('expected prob [n, %d, %d, C] and pred [n, %d, %d], got %s and %s' % (X2, Y2, X2, Y2, prob.shape, pred.shape))
    n, C = prob.shape[0], prob.shape[3]
    if not 2 <= C <= MAX_CLASSES:
        raise ValueError('n_class %d: 2 to %d classes' % (C, MAX_CLASSES))
    if x_pre < 0 or y_pre < 0 or x_pre + X > X2 or y_pre + Y > Y2:
        raise ValueError('the image region %d+%d x %d+%d lies outside the %d x %d batch' % (x_pre, X, y_pre, Y, X2, Y2))
    if first_slice < 0 or first_slice + n > Z * T:
        raise ValueError('slices %d .. %d lie outside the batch of Z*T = %d x %d slices' % (first_slice, first_slice + n - 1, Z, T))
    if cells is None:
        cells = new_cells(T, C)
    if cells.shape != (T, C, FIELDS) or cells.dtype != np.uint64:
        raise ValueError('cells: uint64 [%d, %d, %d]' % (T, C, FIELDS))
    if n == 0:
        return cells
    q = quantise(prob[:, x_pre:x_pre + X, y_pre:y_pre + Y, :]).reshape(n, X * Y, C)
    lab = pred[:, x_pre:x_pre + X, y_pre:y_pre + Y].reshape(n, X * Y).astype(np.int64)
    frame = np.broadcast_to(((first_slice + np.arange(n)) // Z)[:, None], lab.shape)
    # every weighted bincount below adds integers in float64: exact while the totals stay below 2^53
    assert 65536 * n * X * Y < 1 << 53
    add = np.zeros((T, C, FIELDS), np.int64)
    for c in range(C):
        add[:, c, 19] = np.bincount(frame.ravel(), weights=q[:, :, c].ravel(), minlength=T).astype(np.int64)
    ok = (lab >= 0) & (lab < C)
    lab_ok, frame_ok, q_ok = lab[ok], frame[ok], q[ok]
    q1 = np.take_along_axis(q_ok, lab_ok[:, None], axis=1)[:, 0]
    others = q_ok.copy()
    np.put_along_axis(others, lab_ok[:, None], -1, axis=1)
    margin = q1 - others.max(axis=1)
    key = frame_ok * C + lab_ok
    add[:, :, 0] = np.bincount(key, minlength=T * C).reshape(T, C)
    add[:, :, 1] = np.bincount(key, weights=q1, minlength=T * C).astype(np.int64).reshape(T, C)
    add[:, :, 2] = np.bincount(key, weights=margin, minlength=T * C).astype(np.int64).reshape(T, C)
    add[:, :, 3:19] = np.bincount(key * 16 + np.minimum(q1 >> 12, 15), minlength=T * C * 16).reshape(T, C, 16)
    cells += add.view(np.uint64)                          # two's complement: a negative margin sum wraps as the device's add does
    return cells


def cells_from_volume(prob, pred):
    """The cells of a subject from its cropped volumes: prob (X,Y,Z,T,C) float32 and pred (X,Y,Z,T), as the host path of
    deploy_network_ao.py holds them."""
    prob, pred = np.asarray(prob), np.asarray(pred)
    X, Y, Z, T = pred.shape
    return cells_host(np.ascontiguousarray(prob.transpose(3, 2, 0, 1, 4)).reshape(T * Z, X, Y, prob.shape[4]),
                      pred.transpose(3, 2, 0, 1).reshape(T * Z, X, Y), (X, Y, Z, T))


class HostCells:
    """The cells of one subject on the host path: ``add`` takes what the forward returned for the next chunk of slices."""

    def __init__(self, shape, pad, n_class):
        self.shape, self.pad, self.first = tuple(int(v) for v in shape), pad, 0
        self.cells = new_cells(self.shape[3], n_class)

    def add(self, prob, pred):
        cells_host(prob, pred, self.shape, self.pad, self.first, self.cells)
        self.first += len(pred)


def _row(frame, label, cell):
    n, s1, soft = int(cell[0]), int(cell[1]), int(cell[19])
    sm = int(np.asarray(cell[2], np.uint64).astype(np.int64))
    hist = [int(v) for v in cell[3:19]]
    nan = float('nan')
    if n == 0:                                            # the class is absent: nothing to average (written empty, as an undefined distance)
        return [frame, label, 0, nan, nan, nan, nan, float(np.float64(soft) / np.float64(65536))]
    den = np.float64(65536 * n)
    return [frame, label, n, float(np.float64(s1) / den), float(np.float64(sm) / den), float(np.float64(sum(hist[:8])) / np.float64(n)),
            float(np.float64(sum(hist[:12])) / np.float64(n)), float(np.float64(soft) / np.float64(65536))]


def frame_rows(cells):
    """The --confidence_csv lines of one subject from its cells [T, n_class, 20]: CONF_COLUMNS per (frame, label >= 1), then one line per
    label with frame = 'all' from the cells summed over the frames.
        mean_conf = cell[1] / (65536 n), mean_margin = cell[2] / (65536 n), frac_below_0.5 = (bins 0..7) / n,
        frac_below_0.75 = (bins 0..11) / n, soft_n = cell[19] / 65536"""
    cells = np.asarray(cells)
    if cells.ndim != 3 or cells.shape[2] != FIELDS or cells.dtype != np.uint64:
        raise ValueError('cells: uint64 [T, n_class, %d], got %s %s' % (FIELDS, cells.dtype, cells.shape))
    T, C = cells.shape[:2]
    rows = [_row(t, c, cells[t, c]) for t in range(T) for c in range(1, C)]
    total = cells.sum(axis=0, dtype=np.uint64)
    return rows + [_row(ALL_FRAMES, c, total[c]) for c in range(1, C)]


def write_csv(path, rows):
    """rows: [(subject, [CONF_COLUMNS values])], one per (subject, frame, label): the text pandas' to_csv writes for them (the frame
    column holds numbers and 'all'; floats by repr, empty for NaN), written under a temporary name and renamed."""
    import csv
    import io
    import os
    from .atrial import _cell
    buf = io.StringIO()
    wr = csv.writer(buf, lineterminator='\n')
    wr.writerow([''] + CONF_COLUMNS)
    for subject, vals in rows:
        wr.writerow([subject] + [v if isinstance(v, str) else _cell(v) for v in vals])
    tmp = '%s.tmp.%d' % (path, os.getpid())
    with open(tmp, 'w', newline='') as f:
        f.write(buf.getvalue())
    os.replace(tmp, path)
