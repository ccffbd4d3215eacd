"""Atrial area, length and volume from long-axis label maps: cardiac_utils.evaluate_atrial_area_length (reference
common/cardiac_utils.py:1655-1736) and the table of long_axis/eval_atrial_volume.py, stated twice.

  ``area_length_reference``  the literal restatement: the Python loops, np.dot, the default argsort, the early
                             ``return -1, -1, -1`` that invalidates the whole frame, ``labs`` from the labels present
  ``frame_stats_host``       the specification of ukbb_fcn_atrial_area_length (csrc/kernels_qc.hip): vectorised, int32
                             [P, n_class, 8] = size, status, x0, y0, x1, y1, n_hits, 0 per (plane, label)

Statuses: 0 label absent from the plane, 1 measured, 2 the major axis is NaN (the bottom third is empty or the two centres
coincide), 3 the axis line misses the component.  The rules of ``frame_stats_host`` for label k on a plane, every
floating-point step a single rounded float64 operation in this order (no BLAS, nothing that can fuse):

  component   C = the largest 8-connected component of plane == k, ties to the component whose first voxel comes first in
              the C-order scan of the [x][y] array (qc_gates.py); size = |C|
  key         d(x, y) = (w0*l0 + w1*l1) + w2*l2 with w_i = (a_i0*x + a_i1*y) + a_i3, l = long_axis (-0.0 counts as 0.0)
  order       by (d, x*Y + y): a stable sort on d
  thirds      k1 = int(size / 3), k2 = int(2 * size / 3); bottom = the first k1 voxels, top = the voxels from k2 on;
              their coordinate sums are exact integers, bx = sum_x / k1 and so on
  axis        m = (cx - bx, cy - by); norm = sqrt(m0*m0 + m1*m1); m /= norm; p = c + 100*m, q = c - 100*m; any NaN:
              status 2; the end points are int() of each (truncated toward zero)
  line        line_pixels((int(qy), int(qx)), (int(py), int(px)), width=Y, height=X): the cv point is (y, x)
  hits        the line pixels inside C; none: status 3; otherwise (x0, y0) = the hit with the smallest (d, x*Y + y),
              (x1, y1) the one with the largest, n_hits their count

The cm and cm2 values come from these integers on the host (``cell_measures``), with the reference's own expressions.
OpenCV is not a dependency: ``line_pixels`` restates its 8-connected line, see there."""
import math
import os

import numpy as np

from . import aorta_qc, measures

ATRIAL_COLUMNS = ['LAV max (mL)', 'LAV min (mL)', 'LASV (mL)', 'LAEF (%)',
                  'RAV max (mL)', 'RAV min (mL)', 'RASV (mL)', 'RAEF (%)']      # eval_atrial_volume.py:166-167
# --atrial_csv: one row per (subject, frame, label); the index column is the subject
FRAME_COLUMNS = ['frame', 'label', 'size', 'status', 'x0', 'y0', 'x1', 'y1', 'n_hits', 'area (cm2)', 'length (cm)',
                 'lm0 x (mm)', 'lm0 y (mm)', 'lm0 z (mm)', 'lm1 x (mm)', 'lm1 y (mm)', 'lm1 z (mm)', 'gate passed']
ABSENT, MEASURED, NO_AXIS, NO_HIT = 0, 1, 2, 3


# ---- cv2.line(img, pt1, pt2, colour): thickness 1, 8-connected, shift 0 ------------------------------------------------------
def _clip_line(W, H, x1, y1, x2, y2):
    """cv::clipLine on the rectangle [0, W-1] x [0, H-1] with Python integers (OpenCV: int64).  Returns the clipped end
    points, or None when the line is rejected."""
    right, bottom = W - 1, H - 1
    c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8
    c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8
    if (c1 & c2) == 0 and (c1 | c2) != 0:
        if c1 & 12:
            a = 0 if c1 < 8 else bottom
            x1 += int(float(a - y1) * float(x2 - x1) / float(y2 - y1))
            y1 = a
            c1 = (x1 < 0) + (x1 > right) * 2
        if c2 & 12:
            a = 0 if c2 < 8 else bottom
            x2 += int(float(a - y2) * float(x2 - x1) / float(y2 - y1))
            y2 = a
            c2 = (x2 < 0) + (x2 > right) * 2
        if (c1 & c2) == 0 and (c1 | c2) != 0:
            if c1:
                a = 0 if c1 == 1 else right
                y1 += int(float(a - x1) * float(y2 - y1) / float(x2 - x1))
                x1 = a
                c1 = 0
            if c2:
                a = 0 if c2 == 1 else right
                y2 += int(float(a - x2) * float(y2 - y1) / float(x2 - x1))
                x2 = a
                c2 = 0
    return (x1, y1, x2, y2) if (c1 | c2) == 0 else None


def line_setup(pt1, pt2, width, height):
    """The start pixel, the steps and the error term of ``line_pixels``: (x, y, major step (dx, dy), minor step (dx, dy),
    dmaj, dmin, count), or None for a line that lies outside the image."""
    c = _clip_line(width, height, int(pt1[0]), int(pt1[1]), int(pt2[0]), int(pt2[1]))
    if c is None:
        return None
    x1, y1, x2, y2 = c
    dx, dy = x2 - x1, y2 - y1
    sx = sy = 1
    if dx < 0:                                         # leftToRight: start from the second point
        dx, dy = -dx, -dy
        x1, y1 = x2, y2
    if dy < 0:
        dy, sy = -dy, -1
    if dy > dx:                                        # steep: y is the major axis
        return x1, y1, (0, sy), (sx, 0), dy, dx, dy + 1
    return x1, y1, (sx, 0), (0, sy), dx, dy, dx + 1


def line_pixels(pt1, pt2, width, height):
    """The pixels (x, y) that ``cv2.line(img, pt1, pt2, colour)`` sets in an image of ``height`` rows and ``width`` columns
    (thickness 1, 8-connected, shift 0), in drawing order, restated from OpenCV's cv::clipLine and cv::LineIterator -- OpenCV
    itself is not installed where this was written, so parity with it is pinned only by tests/test_atrial.py where cv2 exists.

    Clipping: if an end point lies outside [0, W-1] x [0, H-1], outcodes (x<0) + 2(x>right) + 4(y<0) + 8(y>bottom); the line is
    rejected when c1 & c2; each outside point moves to y = 0 / bottom first with x += (int64)((double)(a - y) * (x2 - x1) /
    (y2 - y1)) (truncation toward zero; the second point sees the first one already moved), the x outcode is recomputed, and the
    same is done for x = 0 / right.
    Stepping (LineIterator, leftToRight): dx < 0: start from the second point with both deltas negated; dy < 0: the minor step
    is -1; dy > dx: the axes swap roles.  err = dx - 2dy, count = dx + 1; every step emits the pixel, then -- if err < 0 before
    the update -- advances the minor axis and adds 2dx, and always advances the major axis and subtracts 2dy."""
    s = line_setup(pt1, pt2, width, height)
    if s is None:
        return []
    x, y, major, minor, dmaj, dmin, count = s
    err = dmaj - 2 * dmin
    out = []
    for _ in range(count):
        out.append((x, y))
        if err < 0:
            x, y = x + minor[0], y + minor[1]
            err += 2 * dmaj
        x, y = x + major[0], y + major[1]
        err -= 2 * dmin
    return out


def minor_steps(i, dmaj, dmin):
    """Minor-axis advances before pixel i of ``line_pixels``, in closed form (what the kernel's lanes evaluate): the step j
    advances iff dmaj - 2 dmin (j + 1) + 2 dmaj m_j < 0, so m_i = ceil((2 dmin i - dmaj) / (2 dmaj))."""
    return 0 if dmaj == 0 else (2 * dmin * i + dmaj - 1) // (2 * dmaj)


# ---- the literal restatement -------------------------------------------------------------------------------------------------
def get_largest_cc(binary):
    """image_utils.get_largest_cc (reference common/image_utils.py:227-238) of a 2-D mask: skimage.measure.label (8-connected,
    labels numbered by each component's first voxel in C order), regionprops areas, the first label of the greatest area."""
    binary = np.asarray(binary).astype(bool)
    X, Y = binary.shape
    _, root = aorta_qc._components(binary.astype(np.uint8).reshape(X, Y, 1, 1))
    root = root.reshape((X, Y), order='F')
    roots = []                                         # in C-order scan order of their first voxel
    seen = set()
    for x in range(X):
        for y in range(Y):
            if binary[x, y] and root[x, y] not in seen:
                seen.add(root[x, y])
                roots.append(root[x, y])
    if not roots:
        return np.zeros_like(binary)
    area = [int(np.sum(binary & (root == r))) for r in roots]
    return binary & (root == roots[int(np.argmax(area))])


def world_point(affine, x, y):
    """np.dot(nim.affine, np.array([x, y, 0, 1]))[:3] (cardiac_utils.py:1721)."""
    return np.dot(affine, np.array([x, y, 0, 1]))[:3]


def area_length_reference(label2d, affine, pixdim, long_axis):
    """evaluate_atrial_area_length(label, nim, long_axis) with nim.affine = ``affine`` and nim.header['pixdim'] = ``pixdim``
    (the header's float32 array of 8): (A, L, landmarks) lists over the labels present, or (-1, -1, -1).  cv2.line is
    ``line_pixels``; get_largest_cc is the function above."""
    label = np.asarray(label2d)
    pixdim = np.asarray(pixdim)[1:4]
    area_per_pix = pixdim[0] * pixdim[1] * 1e-2
    L = []
    A = []
    landmarks = []
    labs = np.sort(list(set(np.unique(label)) - set([0])))
    for i in labs:
        label_i = (label == i)
        label_i = get_largest_cc(label_i)
        points_label = np.nonzero(label_i)
        points = []
        for j in range(len(points_label[0])):
            x = points_label[0][j]
            y = points_label[1][j]
            points += [[x, y, np.dot(np.dot(affine, np.array([x, y, 0, 1]))[:3], long_axis)]]
        points = np.array(points)
        points = points[points[:, 2].argsort()]
        n_points = len(points)
        top_points = points[int(2 * n_points / 3):]
        with np.errstate(all='ignore'):
            cx, cy, _ = np.mean(top_points, axis=0)
            bottom_points = points[:int(n_points / 3)]
            if len(bottom_points):
                bx, by, _ = np.mean(bottom_points, axis=0)
            else:                                      # np.mean of an empty slice: NaN (and a RuntimeWarning)
                bx = by = np.float64(np.nan)
            major_axis = np.array([cx - bx, cy - by])
            major_axis = major_axis / np.linalg.norm(major_axis)
        px = cx + major_axis[0] * 100
        py = cy + major_axis[1] * 100
        qx = cx - major_axis[0] * 100
        qy = cy - major_axis[1] * 100
        if np.isnan(px) or np.isnan(py) or np.isnan(qx) or np.isnan(qy):
            return -1, -1, -1
        image_line = np.zeros(label_i.shape)
        for cvx, cvy in line_pixels((int(qy), int(qx)), (int(py), int(px)), label_i.shape[1], label_i.shape[0]):
            image_line[cvy, cvx] = 1
        image_line = label_i & (image_line > 0)
        points_line = np.nonzero(image_line)
        points = []
        for j in range(len(points_line[0])):
            x = points_line[0][j]
            y = points_line[1][j]
            point = np.dot(affine, np.array([x, y, 0, 1]))[:3]
            points += [np.append(point, np.dot(point, long_axis))]
        points = np.array(points)
        if len(points) == 0:
            return -1, -1, -1
        points = points[points[:, 3].argsort(), :3]
        L += [np.linalg.norm(points[-1] - points[0]) * 1e-1]
        A += [np.sum(label_i) * area_per_pix]
        landmarks += [points[0]]
        landmarks += [points[-1]]
    return A, L, landmarks


# ---- the specification of the kernel -------------------------------------------------------------------------------------
def projection(affine, long_axis, x, y):
    """d(x, y) of the module docstring for integer arrays x, y: float64, one rounding per operation."""
    a = np.asarray(affine, np.float64)
    l = np.asarray(long_axis, np.float64)
    fx, fy = np.asarray(x).astype(np.float64), np.asarray(y).astype(np.float64)
    w = [(a[i, 0] * fx + a[i, 1] * fy) + a[i, 3] for i in range(3)]
    return ((w[0] * l[0] + w[1] * l[1]) + w[2] * l[2]) + 0.0


def winning_components(planes, n_class):
    """(member, size): member (X, Y, P) uint8 = k where the voxel belongs to the largest component of plane == k (the tie rule
    of qc_gates.plane_stats_host), else 0; size [P, n_class] int64 of those components."""
    planes = np.asarray(planes)
    X, Y, P = planes.shape
    n = X * Y * P
    lab, root = aorta_qc._components(planes.reshape(X, Y, 1, P))
    first_of = (np.arange(X, dtype=np.int64)[:, None, None] * Y + np.arange(Y, dtype=np.int64)[None, :, None]
                + np.zeros((1, 1, P), np.int64)).reshape(-1, order='F')
    fg = np.flatnonzero((lab != 0) & (lab < n_class))
    size = np.bincount(root[fg], minlength=n)
    first = np.full(n, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(first, root[fg], first_of[fg])
    roots = fg[root[fg] == fg]
    best = np.zeros((P, n_class), np.int64)
    np.maximum.at(best, (roots // (X * Y), lab[roots].astype(np.int64)), (size[roots] << 32) | (0xFFFFFFFF - first[roots]))
    plane_of = np.arange(n, dtype=np.int64) // (X * Y)
    k = np.where(lab < n_class, lab, 0).astype(np.int64)
    win = (k != 0) & (first[root] == 0xFFFFFFFF - (best[plane_of, k] & 0xFFFFFFFF))
    return np.where(win, k, 0).astype(np.uint8).reshape((X, Y, P), order='F'), best >> 32


def cell_detail(member2d, k, affine, long_axis):
    """One (plane, label) cell from the member map of its plane: the 8 integers and, for tests, the sorted keys."""
    X, Y = member2d.shape
    xs, ys = np.nonzero(member2d == k)                 # C order: ascending x*Y + y
    size = len(xs)
    row = np.zeros(8, np.int32)
    if size == 0:
        return row, None
    row[0], row[1] = size, NO_AXIS
    d = projection(affine, long_axis, xs, ys)
    order = np.lexsort((xs * Y + ys, d))               # by (d, x*Y + y)
    xs, ys, d = xs[order], ys[order], d[order]
    k1, k2 = int(size / 3), int(2 * size / 3)
    detail = {'d': d, 'k1': k1, 'k2': k2}
    with np.errstate(all='ignore'):
        bx = np.float64(xs[:k1].sum()) / np.float64(k1)
        by = np.float64(ys[:k1].sum()) / np.float64(k1)
        cx = np.float64(xs[k2:].sum()) / np.float64(size - k2)
        cy = np.float64(ys[k2:].sum()) / np.float64(size - k2)
        m0, m1 = cx - bx, cy - by
        norm = np.sqrt(m0 * m0 + m1 * m1)
        m0, m1 = m0 / norm, m1 / norm
        px, py = cx + 100.0 * m0, cy + 100.0 * m1
        qx, qy = cx - 100.0 * m0, cy - 100.0 * m1
    if np.isnan(px) or np.isnan(py) or np.isnan(qx) or np.isnan(qy):
        return row, detail
    detail['ends'] = (px, py, qx, qy)
    row[1] = NO_HIT
    hits = [(cvy, cvx) for cvx, cvy in line_pixels((int(qy), int(qx)), (int(py), int(px)), Y, X)
            if 0 <= cvy < X and 0 <= cvx < Y and member2d[cvy, cvx] == k]
    if not hits:
        return row, detail
    hx, hy = np.array([h[0] for h in hits], np.int64), np.array([h[1] for h in hits], np.int64)
    hd = projection(affine, long_axis, hx, hy)
    ho = np.lexsort((hx * Y + hy, hd))
    detail['hit_d'] = hd[ho]
    row[1:7] = MEASURED, hx[ho[0]], hy[ho[0]], hx[ho[-1]], hy[ho[-1]], len(hits)
    return row, detail


def frame_stats_host(planes, n_class, affine, long_axis):
    """int32 [P, n_class, 8] (size, status, x0, y0, x1, y1, n_hits, 0) of an (X, Y, P) array of label planes: the module
    docstring's rules, the host twin of device_pipeline.device_atrial_stats.  Labels >= n_class are ignored; row 0 is zero."""
    planes = np.asarray(planes)
    if planes.ndim == 2:
        planes = planes[:, :, None]
    P = planes.shape[2]
    member, _ = winning_components(planes, n_class)
    out = np.zeros((P, n_class, 8), np.int32)
    for p in range(P):
        for k in range(1, n_class):
            out[p, k] = cell_detail(member[:, :, p], k, affine, long_axis)[0]
    return out


# ---- cm and cm2 from the integers, as the reference computes them ----------------------------------------------------------
def cell_measures(row, affine, pixdim):
    """(A, L, lm0, lm1) of a measured cell (status 1): the reference's np.sum(label_i) * area_per_pix (:1731), the norm of the
    difference of its two world points * 1e-1 (:1728) and the points themselves (:1734-1735)."""
    pd = np.asarray(pixdim)[1:4]
    area_per_pix = pd[0] * pd[1] * 1e-2
    lm0, lm1 = world_point(affine, row[2], row[3]), world_point(affine, row[4], row[5])
    return np.int64(row[0]) * area_per_pix, np.linalg.norm(lm1 - lm0) * 1e-1, lm0, lm1


def frame_measures(stats_p, affine, pixdim):
    """What evaluate_atrial_area_length returns for a frame with the statistics ``stats_p`` [n_class, 8]: (A, L, landmarks) over
    the labels present in ascending order, or (-1, -1, -1) as soon as one of them has no axis or no hit."""
    A, L, landmarks = [], [], []
    for row in np.asarray(stats_p)[1:]:
        if row[1] == ABSENT:
            continue
        if row[1] != MEASURED:
            return -1, -1, -1
        a, l, lm0, lm1 = cell_measures(row, affine, pixdim)
        A.append(a)
        L.append(l)
        landmarks += [lm0, lm1]
    return A, L, landmarks


def frame_rows(stats, affine, pixdim, gate_passed):
    """The --atrial_csv lines of one subject: [FRAME_COLUMNS values] per (frame, label >= 1)."""
    nan = float('nan')
    rows = []
    stats = np.asarray(stats)
    for t in range(stats.shape[0]):
        for k in range(1, stats.shape[1]):
            row = stats[t, k]
            vals = [nan] * 8
            if row[1] == MEASURED:
                a, l, lm0, lm1 = cell_measures(row, affine, pixdim)
                vals = [a, l] + list(lm0) + list(lm1)
            rows.append([t, k] + [int(v) for v in row[:7]] + vals + [bool(gate_passed)])
    return rows


def frames_from_stats(stats, affine, pixdim):
    """Per frame what ``atrial_volumes`` reads: None for a frame the reference skips, else [(A, L)] over the labels present."""
    out = []
    for t in range(np.asarray(stats).shape[0]):
        A, L, _ = frame_measures(stats[t], affine, pixdim)
        out.append(None if isinstance(A, int) else list(zip(A, L)))
    return out


def atrial_volumes(frames_2ch, frames_4ch, pixdim4, T):
    """eval_atrial_volume.py:70-161.  frames_2ch / frames_4ch: per frame None (the frame returned -1: it stays 0) or [(area,
    length)] over its labels; pixdim4: pixdim[4] of the 4-chamber header; T: dim[4] of the 2-CHAMBER file, which also bounds
    the 4-chamber loop (the caller skips a subject whose 4-chamber sequence is shorter; the reference raises IndexError).
    Returns {'A', 'L', 'V': dicts of arrays, 'heart_rate', 'val': the eight values}; min / max run over the zero frames too."""
    A, L, V = {}, {}, {}
    A['LA_2ch'], L['LA_2ch'], V['LA_2ch'] = np.zeros(T), np.zeros(T), np.zeros(T)
    with np.errstate(all='ignore'):
        for t in range(T):
            fr = frames_2ch[t]
            if fr is None:
                continue
            area, length = [np.float64(f[0]) for f in fr], [np.float64(f[1]) for f in fr]
            A['LA_2ch'][t] = area[0]
            L['LA_2ch'][t] = length[0]
            V['LA_2ch'][t] = 8 / (3 * math.pi) * area[0] * area[0] / length[0]
        for name in ('LA_4ch', 'RA_4ch'):
            A[name], L[name], V[name] = np.zeros(T), np.zeros(T), np.zeros(T)
        V['LA_bip'] = np.zeros(T)
        for t in range(T):
            fr = frames_4ch[t]
            if fr is None:
                continue
            area, length = [np.float64(f[0]) for f in fr], [np.float64(f[1]) for f in fr]
            A['LA_4ch'][t] = area[0]
            L['LA_4ch'][t] = length[0]
            V['LA_4ch'][t] = 8 / (3 * math.pi) * area[0] * area[0] / length[0]
            V['LA_bip'][t] = 8 / (3 * math.pi) * area[0] * A['LA_2ch'][t] / (0.5 * (length[0] + L['LA_2ch'][t]))
            A['RA_4ch'][t] = area[1]
            L['RA_4ch'][t] = length[1]
            V['RA_4ch'][t] = 8 / (3 * math.pi) * area[1] * area[1] / length[1]
        duration_per_cycle = T * pixdim4
        heart_rate = 60.0 / duration_per_cycle
        val = {}
        val['LAV_bip_max'] = np.max(V['LA_bip'])
        val['LAV_bip_min'] = np.min(V['LA_bip'])
        val['LASV_bip'] = val['LAV_bip_max'] - val['LAV_bip_min']
        val['LAEF_bip'] = val['LASV_bip'] / val['LAV_bip_max'] * 100
        val['RAV_4ch_max'] = np.max(V['RA_4ch'])
        val['RAV_4ch_min'] = np.min(V['RA_4ch'])
        val['RASV_4ch'] = val['RAV_4ch_max'] - val['RAV_4ch_min']
        val['RAEF_4ch'] = val['RASV_4ch'] / val['RAV_4ch_max'] * 100
    return {'A': A, 'L': L, 'V': V, 'heart_rate': heart_rate, 'val': val}


def atrial_row(val):
    """The table line of eval_atrial_volume.py:160-161."""
    return [val['LAV_bip_max'], val['LAV_bip_min'], val['LASV_bip'], val['LAEF_bip'],
            val['RAV_4ch_max'], val['RAV_4ch_min'], val['RASV_4ch'], val['RAEF_4ch']]


def long_axis_from_sa(sa_affine):
    """eval_atrial_volume.py:45-48: the normalised third column of the short-axis affine, pointing to +z."""
    sa_affine = np.asarray(sa_affine, np.float64)
    long_axis = sa_affine[:3, 2] / np.linalg.norm(sa_affine[:3, 2])
    if long_axis[2] < 0:
        long_axis *= -1
    return long_axis


# ---- the per-frame record (--atrial_csv) ---------------------------------------------------------------------------------------
def _cell(v):
    if isinstance(v, (bool, np.bool_)):
        return 'True' if v else 'False'
    if isinstance(v, (int, np.integer)):
        return str(int(v))
    return measures._fmt(v)


def write_frames_csv(path, rows, columns=None):
    """rows: [(subject, [FRAME_COLUMNS values])], one per (subject, frame, label).  Floats as measures.write_csv writes them
    (repr: they read back exactly), written under a temporary name and renamed.  columns: those of another table with several rows
    per subject (seg_score.SCORE_COLUMNS)."""
    import csv
    import io
    buf = io.StringIO()
    wr = csv.writer(buf, lineterminator='\n')
    wr.writerow([''] + list(FRAME_COLUMNS if columns is None else columns))
    for subject, vals in rows:
        wr.writerow([subject] + [_cell(v) for v in vals])
    tmp = '%s.tmp.%d' % (path, os.getpid())
    with open(tmp, 'w', newline='') as f:
        f.write(buf.getvalue())
    os.replace(tmp, path)


def merge_frames_csv(path, num_shards, remove=True):
    """measures.merge_shard_csv for an --atrial_csv file: sorted by (subject, frame, label), one row per such key."""
    return measures.merge_shard_csv(path, num_shards, remove, key_columns=3)


def read_frames_csv(path):
    """{subject: {'frames': [None | [(A, L)] per frame], 'gate': bool}} from an --atrial_csv file, for ``atrial_volumes``: a
    frame is None as soon as one of its labels present (status != 0) is not measured."""
    import csv
    with open(path, newline='') as f:
        rd = list(csv.reader(f))
    col = {name: i + 1 for i, name in enumerate(FRAME_COLUMNS)}
    by = {}
    for r in rd[1:]:
        s = by.setdefault(r[0], {'cells': {}, 'gate': r[col['gate passed']] == 'True'})
        status = int(r[col['status']])
        al = (np.float64(r[col['area (cm2)']]), np.float64(r[col['length (cm)']])) if status == MEASURED else None
        s['cells'].setdefault(int(r[col['frame']]), []).append((int(r[col['label']]), status, al))
    out = {}
    for subject, s in by.items():
        frames = []
        for t in range(max(s['cells']) + 1):
            cells = sorted(c for c in s['cells'].get(t, []) if c[1] != ABSENT)
            frames.append(None if any(c[1] != MEASURED for c in cells) else [c[2] for c in cells])
        out[subject] = {'frames': frames, 'gate': s['gate']}
    return out
