"""What tests/test_confidence.py and tests/test_confidence_gpu.py share: the per-voxel restatement of the cell definition, random softmax
batches inside a padded frame, and the planted edge values."""
import numpy as np

FIELDS = 20


def q_of(p):
    """q(p) of one float32 probability, as the definition says it: one float32 multiply, truncation; NaN gives 0."""
    x = np.float32(p) * np.float32(65536.0)
    return 0 if x != x else int(x)


def loop_cells(prob, pred, shape, pad, first_slice=0):
    """The cells [T, C, 20] by a plain loop over the voxels of the image region: Python integers, no numpy reduction."""
    X, Y, Z, T = shape
    X2, Y2, x_pre, y_pre = pad
    n, C = prob.shape[0], prob.shape[3]
    cells = [[[0] * FIELDS for _ in range(C)] for _ in range(T)]
    for b in range(n):
        t = (first_slice + b) // Z
        for x in range(x_pre, x_pre + X):
            for y in range(y_pre, y_pre + Y):
                q = [q_of(prob[b, x, y, c]) for c in range(C)]
                for c in range(C):
                    cells[t][c][19] += q[c]
                c = int(pred[b, x, y])
                if not 0 <= c < C:
                    continue
                q1 = q[c]
                margin = q1 - max(q[k] for k in range(C) if k != c)
                cell = cells[t][c]
                cell[0] += 1
                cell[1] += q1
                cell[2] += margin
                cell[3 + min(q1 >> 12, 15)] += 1
    return np.array([[[v % (1 << 64) for v in cell] for cell in frame] for frame in cells], dtype=np.uint64)


def softmax_batch(n, X2, Y2, C, seed, sharp=3.0):
    """prob [n, X2, Y2, C] float32 (rows sum to about 1) and pred = its lowest-index argmax, int32."""
    rng = np.random.default_rng(seed)
    lg = (rng.standard_normal((n, X2, Y2, C)) * sharp).astype(np.float32)
    e = np.exp(lg - lg.max(axis=-1, keepdims=True))
    prob = (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)
    return prob, np.argmax(prob, axis=-1).astype(np.int32)


def spoil_padding(prob, pred, shape, pad):
    """Fill everything outside the image region with values that would change every field of every cell if they were counted: label 1
    (and others) with probability 1, runner-up 0.25."""
    X, Y = shape[:2]
    X2, Y2, x_pre, y_pre = pad
    C = prob.shape[3]
    outside = np.ones((X2, Y2), bool)
    outside[x_pre:x_pre + X, y_pre:y_pre + Y] = False
    idx = np.argwhere(outside)
    for k, (x, y) in enumerate(idx):
        c = k % C
        prob[:, x, y, :] = 0.25 if C > 2 else 0.0
        prob[:, x, y, c] = (1.0, 0.4375, 0.8125)[k % 3]
        pred[:, x, y] = c
    return prob, pred


N_EDGES = 20


def plant_edges(prob, pred, b, voxels):
    """The edge values at the N_EDGES given (x2, y2) voxels of slice b; returns [(voxel, label, q1, margin)] as the definition gives them."""
    assert len(voxels) == N_EDGES
    C = prob.shape[3]
    tiny = np.float32(1e-40)                              # a denormal
    assert 0 < tiny < np.finfo(np.float32).tiny
    planted = []

    def put(i, values, label):
        x, y = voxels[i]
        p = np.zeros(C, np.float32)
        p[:len(values)] = values
        prob[b, x, y] = p
        pred[b, x, y] = label
        q = [q_of(v) for v in p]
        planted.append(((b, x, y), label, q[label], q[label] - max(q[k] for k in range(C) if k != label)))

    put(0, [0.0, 1.0], 1)                                # p exactly 1: q = 65536, the last bin
    put(1, [1.0, tiny], 0)                           # a denormal runner-up: q2 = 0 whether or not the multiply flushes
    put(2, [0.5, 0.5], 0)                            # equal top two: margin 0, the lower index labelled
    put(3, [0.25, 0.75], 1)
    put(4, [np.float32(0.49999997), np.float32(0.5000001)], 1)
    for k in range(1, 16):                                # p exactly k/16: the first value of bin k (rows need not sum to 1 here)
        put(4 + k, [k / 16.0, 0.0], 0)
    return planted
