"""Label planes for the seg_score tests (CPU and GPU), an independent contour source -- Suzuki and Abe's sequential border following
(1985, algorithm 1), pure Python, outer borders of the outermost components only, which is what cv2.findContours(RETR_EXTERNAL,
CHAIN_APPROX_NONE) returns -- and the reference's distance_metric restated literally on point lists."""
import numpy as np

from ukbb_cardiac_amd.phantom import cine_phantom

X0, Y0 = 33, 41                                          # odd, no multiple of a word: the hand-made planes


def _grid(X, Y):
    return np.meshgrid(np.arange(X), np.arange(Y), indexing='ij')


def disc(X=X0, Y=Y0, cx=16, cy=20, r2=81):
    x, y = _grid(X, Y)
    return (x - cx) ** 2 + (y - cy) ** 2 <= r2


def ring(X=X0, Y=Y0):
    return disc(X, Y, r2=144) & ~disc(X, Y, r2=49)


def serpentine(X, Y):
    """A block whose background corridor snakes through every second line of x from an opening at (0, 1): the outer background
    reaches its far end only after on the order of X*Y/2 one-pixel steps."""
    m = np.ones((X, Y), bool)
    m[0, 1] = False
    for x in range(1, X - 1, 2):
        m[x, 1:Y - 1] = False
        if x + 2 < X - 1:
            m[x + 1, Y - 2 if (x // 2) % 2 == 0 else 1] = False
    return m


def checkerboard(X, Y):
    x, y = _grid(X, Y)
    return (x + y) % 2 == 0


def stripes(X, Y):
    """Every second line of x: each of its X*Y/2 pixels borders the outer background -- the longest contour a plane can have.  (A
    checkerboard or dense noise has fewer: their background does not connect, so only the rim is outer.)"""
    m = np.zeros((X, Y), bool)
    m[::2] = True
    return m


def fixtures():
    """name -> boolean [X0, Y0] mask."""
    f = {'disc': disc(), 'ring': ring()}
    f['ring_island'] = ring() | disc(r2=9)
    f['two_components'] = disc(cx=8, cy=9, r2=30) | disc(cx=24, cy=30, r2=40)
    m = np.zeros((X0, Y0), bool)
    m[5:10, 5:10] = m[10:15, 10:15] = True
    f['corner_squares'] = m
    m = np.zeros((X0, Y0), bool)
    m[5:13, 5:13] = True
    m[5, 5] = m[6, 6] = False                           # (6, 6) touches the outside through the missing corner (5, 5) only diagonally
    f['diagonal_pocket'] = m
    m = np.ones((X0, Y0), bool)
    m[:4, :4] = m[-4:, :4] = m[:4, -4:] = m[-4:, -4:] = False
    f['all_edges'] = m
    m = np.zeros((X0, Y0), bool)
    m[16, 5:30] = True
    f['line'] = m
    m = np.zeros((X0, Y0), bool)
    m[7, 11] = True
    f['pixel'] = m
    f['serpentine'] = serpentine(X0, Y0)
    f['serpentine_t'] = np.ascontiguousarray(serpentine(Y0, X0).T)
    f['checkerboard'] = checkerboard(X0, Y0)
    return f


# the fixtures whose followed contour passes no pixel twice (asserted in test_seg_score.py): everything without a one-pixel-wide part
NO_REPEAT = ('disc', 'ring', 'ring_island', 'two_components', 'diagonal_pocket', 'all_edges', 'pixel')


def phantom_labels(n, X, Y, seed=3, n_class=4):
    """[n, X, Y] uint8 label planes with blobs, rings and speckle: the synthetic cine thresholded into n_class levels."""
    img = cine_phantom(n, X, Y, seed=seed)[..., 0]
    return np.digitize(img, np.linspace(0.25, 0.75, n_class - 1)).astype(np.uint8)


def noise_labels(shape, n_class, seed):
    return np.random.default_rng(seed).integers(0, n_class, size=shape, dtype=np.uint8)


def volume_from_planes(planes):
    """[P, X, Y] planes -> the (X, Y, P, 1) volume whose plane p they are."""
    return np.asfortranarray(np.moveaxis(np.asarray(planes), 0, 2)[..., None])


# ---- Suzuki & Abe border following ---------------------------------------------------------------------------------------------
_CW = [(0, -1), (-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1)]      # clockwise from west, i down, j right


def _follow(f, i, j, i2, j2, nbd):
    """Steps 3.1-3.5 from the start (i, j) with the first neighbour to look at (i2, j2): marks f, returns the pixels as visited."""
    start = _CW.index((i2 - i, j2 - j))
    found = None
    for s in range(8):
        di, dj = _CW[(start + s) % 8]
        if f[i + di, j + dj] != 0:
            found = (i + di, j + dj)
            break
    if found is None:
        f[i, j] = -nbd
        return [(i, j)]
    i1, j1 = found
    i2, j2, i3, j3 = i1, j1, i, j
    pts = []
    while True:
        pts.append((i3, j3))
        start = _CW.index((i2 - i3, j2 - j3))
        east_zero_seen = False
        for s in range(1, 9):                           # counterclockwise from the element after (i2, j2)
            di, dj = _CW[(start - s) % 8]
            if f[i3 + di, j3 + dj] != 0:
                i4, j4 = i3 + di, j3 + dj
                break
            if (di, dj) == (0, 1):
                east_zero_seen = True
        if east_zero_seen:
            f[i3, j3] = -nbd
        elif f[i3, j3] == 1:
            f[i3, j3] = nbd
        if (i4, j4) == (i, j) and (i3, j3) == (i1, j1):
            return pts
        i2, j2, i3, j3 = i3, j3, i4, j4


def external_contours(mask):
    """The point lists (in visiting order, a pixel once per visit) of the outer borders whose parent is the frame."""
    mask = np.asarray(mask, bool)
    f = np.zeros((mask.shape[0] + 2, mask.shape[1] + 2), np.int64)
    f[1:-1, 1:-1] = mask
    nbd = 1
    parent, is_hole = {1: 1}, {1: True}
    out = []
    for i in range(1, f.shape[0] - 1):
        lnbd = 1
        for j in range(1, f.shape[1] - 1):
            if f[i, j] == 0:
                continue
            hole = None
            if f[i, j] == 1 and f[i, j - 1] == 0:
                hole, i2, j2 = False, i, j - 1
            elif f[i, j] >= 1 and f[i, j + 1] == 0:
                hole, i2, j2 = True, i, j + 1
                if f[i, j] > 1:
                    lnbd = int(f[i, j])
            if hole is not None:
                nbd += 1
                is_hole[nbd] = hole
                parent[nbd] = lnbd if is_hole[lnbd] != hole else parent[lnbd]
                pts = _follow(f, i, j, i2, j2, nbd)
                if not hole and parent[nbd] == 1:
                    out.append([(a - 1, b - 1) for a, b in pts])
            if f[i, j] != 1:
                lnbd = abs(int(f[i, j]))
    return out


def followed_points(mask):
    """All points of the external contours, stacked as the reference stacks them (np.vstack over the contours)."""
    return [p for c in external_contours(mask) for p in c]


def distance_metric_literal(pts_a, pts_b, dx):
    """(md, hd) of one slice as common/image_utils.py:209-217 computes them from two point lists."""
    pts_a, pts_b = np.asarray(pts_a), np.asarray(pts_b)
    M = np.linalg.norm((pts_a[:, None, :] - pts_b[None, :, :]).astype(np.float64), axis=2)     # M[i, j] = np.linalg.norm(pts_A[i] - pts_B[j])
    md = 0.5 * (np.mean(np.min(M, axis=0)) + np.mean(np.min(M, axis=1))) * dx
    hd = np.max([np.max(np.min(M, axis=0)), np.max(np.min(M, axis=1))]) * dx
    return md, hd
