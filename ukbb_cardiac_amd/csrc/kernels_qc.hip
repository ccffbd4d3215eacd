// The label-map and image statistics of the aortic quality control (cardiac_utils.aorta_pass_quality_control, reference
// common/cardiac_utils.py:1739-1796, as eval_aortic_area.py:68-69 calls it), on the volumes the aortic device path already
// holds in HBM:
//
//   ukbb_fcn_label_components  per (frame, class): components of seg_t == k with more than min_size voxels
//                              -- skimage.measure.label(seg_t == l, connectivity=2) + the size filter of :1766-1780
//   ukbb_fcn_label_max         per (frame, class): np.max(image_t[seg_t == k]) as float64, NaN propagated -- :1757-1764
//
//   ukbb_fcn_plane_components per (plane, class) of P label planes: voxels, the largest 8-connected component, the voxels in
//                              components of at least keep_min voxels; per plane: the largest component of (largest of class a |
//                              kept of class b) -- get_largest_cc / remove_small_cc of sa_pass_quality_control (:77-136) and
//                              la_pass_quality_control (:139-169)
//
// (the third statistic, the float32 / float64 mean of image_ED[seg_ED == l] of :1753-1755, is ukbb_fcn_label_compact in
// kernels_prep.hip followed by the pairwise sums there.)
//
// Connected components: a union-find on an int32 parent array over the whole (X,Y,Z,T) label volume, every non-zero class at
// once (a voxel unites only with neighbours of its own label, which gives exactly the components of each seg_t == k mask).
// Neighbourhood: connectivity 2 of skimage in 3-D = 18: the 8 in-plane neighbours and, across z, the voxel itself and its 4
// edge neighbours (3-D corners do not connect); never across frames.  Four launches:
//   1. ccl_local_kernel   a 32x32 tile of one (z, t) plane per workgroup: union-find in LDS, then every voxel's global parent
//                         = its tile-local root (the smallest index of its tile component) and that root's voxel count
//   2. ccl_border_kernel  the neighbour pairs that cross a tile edge or a z plane: union in the global array (agent-scope atomics)
//   3. ccl_size_kernel    every tile-local root adds its count to its global root (one integer atomic per tile component)
//   4. ccl_count_kernel   every global root with more than min_size voxels adds 1 to n_large[t][k]
// Roots are the smallest voxel index of their component: parent[i] <= i always, so every find terminates and the result does
// not depend on the order in which unions arrive; the counts are integer sums, order-independent too.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/ukbb_fcn.h"
#include "kernels.h"

namespace ukbb {

namespace {

constexpr int TILE = 32;                                // tile edge of ccl_local_kernel (1024 voxels, 4 per thread)
constexpr int MAXC = 16;                                // classes per call (as ukbb_fcn_unpack_labels)

// ---- union-find in LDS (one workgroup, workgroup-scope atomics) ---------------------------------------------------------
__device__ __forceinline__ int lds_find(int *p, int i) {
    for (;;) {
        const int q = __hip_atomic_load(&p[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (q == i) return i;
        i = q;
    }
}
__device__ __forceinline__ void lds_union(int *p, int a, int b) {
    for (;;) {                                          // hang the larger root under the smaller one
        a = lds_find(p, a);
        b = lds_find(p, b);
        if (a == b) return;
        if (a > b) { const int s = a; a = b; b = s; }
        const int old = __hip_atomic_fetch_min(&p[b], a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (old == b) return;                           // b was still a root: linked
        b = old;                                        // b was linked meanwhile: its (smaller) parent now takes a
    }
}

// ---- union-find in HBM (all workgroups, agent-scope atomics) -----------------------------------------------------------
// Workgroups on other XCDs rewrite parents while this one reads them.  The links are agent-scope atomic minima: they execute
// at the memory side and return the parent as it is.  The loads are agent-scope atomic loads (sc1: past this CU's L1), but
// this XCD's L2 may still hold an older copy of the line.  Stale loads are harmless: parents only ever decrease and always
// stay inside the component, so a stale value is an older, larger ancestor; find then stops at a former root, the atomic
// minimum on it returns its newer parent, and union carries on from there.  Every failed link replaces the larger of the two
// roots by a smaller index, so union terminates.
__device__ __forceinline__ int hbm_find(int *p, int i) {
    for (;;) {
        const int q = __hip_atomic_load(&p[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (q == i) return i;
        i = q;
    }
}
__device__ __forceinline__ void hbm_union(int *p, int a, int b) {
    for (;;) {
        a = hbm_find(p, a);
        b = hbm_find(p, b);
        if (a == b) return;
        if (a > b) { const int s = a; a = b; b = s; }
        const int old = __hip_atomic_fetch_min(&p[b], a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == b) return;
        b = old;
    }
}

// grid (tiles_x * tiles_y, Z * T), 256 threads; voxel gi = x + X*(y + Y*(z + Z*t)) (NIfTI order)
__global__ __launch_bounds__(256) void ccl_local_kernel(const unsigned char *__restrict__ lab, int X, int Y, int *__restrict__ parent,
                                                        int *__restrict__ size) {
    __shared__ int lp[TILE * TILE];
    __shared__ int cnt[TILE * TILE];
    __shared__ unsigned char ll[TILE * TILE];
    const int tiles_x = (X + TILE - 1) / TILE;
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const long long base = (long long)X * Y * blockIdx.y;
    unsigned char v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int li = threadIdx.x + 256 * j, x = tx * TILE + (li & (TILE - 1)), y = ty * TILE + li / TILE;
        v[j] = (x < X && y < Y) ? lab[base + x + (long long)X * y] : 0;
        ll[li] = v[j];
        lp[li] = li;
        cnt[li] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {                       // the in-plane half neighbourhood inside the tile: (-1,0) (-1,-1) (0,-1) (+1,-1)
        if (!v[j]) continue;
        const int li = threadIdx.x + 256 * j, lx = li & (TILE - 1), ly = li / TILE;
        if (lx > 0 && ll[li - 1] == v[j]) lds_union(lp, li, li - 1);
        if (ly > 0) {
            if (lx > 0 && ll[li - TILE - 1] == v[j]) lds_union(lp, li, li - TILE - 1);
            if (ll[li - TILE] == v[j]) lds_union(lp, li, li - TILE);
            if (lx < TILE - 1 && ll[li - TILE + 1] == v[j]) lds_union(lp, li, li - TILE + 1);
        }
    }
    __syncthreads();
    int root[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        root[j] = -1;
        if (!v[j]) continue;
        root[j] = lds_find(lp, threadIdx.x + 256 * j);
        atomicAdd(&cnt[root[j]], 1);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int li = threadIdx.x + 256 * j, x = tx * TILE + (li & (TILE - 1)), y = ty * TILE + li / TILE;
        if (x >= X || y >= Y) continue;
        const long long gi = base + x + (long long)X * y;
        const int r = root[j];
        // background: its own root of size 0 (never counted, never a neighbour: the labels differ)
        parent[gi] = r < 0 ? (int)gi : (int)(base + tx * TILE + (r & (TILE - 1)) + (long long)X * (ty * TILE + r / TILE));
        size[gi] = r == li ? cnt[li] : 0;
    }
}

// one thread per voxel; only voxels with a half-neighbourhood neighbour outside their tile or in the plane below do any work
__global__ __launch_bounds__(256) void ccl_border_kernel(const unsigned char *__restrict__ lab, int X, int Y, int Z, long long n,
                                                         int *parent) {
    const long long gi = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gi >= n) return;
    const int x = (int)(gi % X);
    long long r = gi / X;
    const int y = (int)(r % Y);
    r /= Y;
    const int z = (int)(r % Z);
    const int ex = x & (TILE - 1);
    if (!(ex == 0 || ex == TILE - 1 || (y & (TILE - 1)) == 0 || z > 0)) return;
    const unsigned char v = lab[gi];
    if (!v) return;
    const int txo = x / TILE, tyo = y / TILE;
    auto link = [&](int dx, int dy, long long off) {    // neighbour (x+dx, y+dy) of this plane, if it lies in another tile
        const int xn = x + dx, yn = y + dy;
        if (xn < 0 || xn >= X || yn < 0) return;
        if (xn / TILE == txo && yn / TILE == tyo) return;   // inside the tile: done by ccl_local_kernel
        if (lab[gi + off] == v) hbm_union(parent, (int)gi, (int)(gi + off));
    };
    link(-1, 0, -1);
    link(-1, -1, -1LL - X);
    link(0, -1, -(long long)X);
    link(1, -1, 1LL - X);
    if (z > 0) {                                        // the plane below: the voxel itself and its 4 edge neighbours (18-connectivity)
        const long long dz = -(long long)X * Y;
        auto down = [&](int dx, int dy) {
            const int xn = x + dx, yn = y + dy;
            if (xn < 0 || xn >= X || yn < 0 || yn >= Y) return;
            const long long o = gi + dz + dx + (long long)X * dy;
            if (lab[o] == v) hbm_union(parent, (int)gi, (int)o);
        };
        down(0, 0);
        down(-1, 0);
        down(1, 0);
        down(0, -1);
        down(0, 1);
    }
}

// every tile-local root (size > 0 after ccl_local_kernel) that is no longer a global root hands its count to its global root.
// parent is read-only in this launch; size[i] of a tile-local root i changes only if i is a global root, which adds nothing.
__global__ __launch_bounds__(256) void ccl_size_kernel(const unsigned char *__restrict__ lab, long long n, const int *__restrict__ parent,
                                                       int *size) {
    const long long gi = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gi >= n || !lab[gi]) return;
    const int s = __hip_atomic_load(&size[gi], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (s == 0) return;
    int i = (int)gi;
    for (int q = parent[i]; q != i; q = parent[i]) i = q;
    if (i != (int)gi) __hip_atomic_fetch_add(&size[i], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void ccl_count_kernel(const unsigned char *__restrict__ lab, long long n, long long frame, int n_class,
                                                        int min_size, const int *__restrict__ parent, const int *__restrict__ size,
                                                        int *n_large) {
    const long long gi = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gi >= n) return;
    const int k = lab[gi];
    if (k == 0 || k >= n_class || parent[gi] != (int)gi || size[gi] <= min_size) return;
    atomicAdd(&n_large[(gi / frame) * n_class + k], 1);
}

// ---- plane-wise component statistics (ukbb_fcn_plane_components) -------------------------------------------------------
// The planes are labelled by the three ccl_* kernels above with Z = 1 (a plane is a frame: 8-connectivity, nothing across
// planes).  What the short- and long-axis gates need on top is each component's size and, for the tie rule of get_largest_cc
// (the first label of the strictly greatest area, labels numbered by the first voxel of a C-order scan of the [x][y] array),
// the smallest x*Y + y of each component.  A voxel whose (x-1, y-1), (x-1, y), (x-1, y+1) or (x, y-1) neighbour carries its
// label cannot be that minimum -- the neighbour is in its component and comes earlier in the scan -- so only the few voxels
// without such a neighbour offer their index to their root (integer atomic minimum).  Every root then offers the key
// (size << 32) | (0xFFFFFFFF - first) to an integer atomic maximum per (plane, class): the largest component, the earliest
// in scan order among equals, whatever the arrival order.

// first[] = INT_MAX, the keys and the three accumulated outputs = 0
__global__ __launch_bounds__(256) void plane_init_kernel(long long n, int cells, int planes, int *__restrict__ first,
                                                         unsigned long long *__restrict__ keys, int *__restrict__ count,
                                                         int *__restrict__ kept, int *__restrict__ union_largest) {
    const long long gi = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gi < n) first[gi] = 0x7FFFFFFF;
    if (gi < cells) {
        keys[gi] = 0;
        count[gi] = 0;
        kept[gi] = 0;
    }
    if (gi < planes) union_largest[gi] = 0;
}

__device__ __forceinline__ int root_of(const int *__restrict__ parent, int i) {     // parent is read-only in the launches that call this
    for (int q = parent[i]; q != i; q = parent[i]) i = q;
    return i;
}

__global__ __launch_bounds__(256) void plane_first_kernel(const unsigned char *__restrict__ lab, int X, int Y, long long n,
                                                          const int *__restrict__ parent, int *first) {
    const long long gi = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gi >= n) return;
    const unsigned char v = lab[gi];
    if (!v) return;
    const int x = (int)(gi % X), y = (int)((gi / X) % Y);
    if (y > 0 && lab[gi - X] == v) return;                                  // (x, y-1)
    if (x > 0 && (lab[gi - 1] == v || (y > 0 && lab[gi - 1 - X] == v) || (y < Y - 1 && lab[gi - 1 + X] == v))) return;
    __hip_atomic_fetch_min(&first[root_of(parent, (int)gi)], x * Y + y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// every root of a class below n_class: its size to count (and to kept, if it has at least keep_min voxels), its key to the maximum
__global__ __launch_bounds__(256) void plane_root_kernel(const unsigned char *__restrict__ lab, long long n, long long plane, int n_class,
                                                         int keep_min, const int *__restrict__ parent, const int *__restrict__ size,
                                                         const int *__restrict__ first, unsigned long long *keys, int *count, int *kept) {
    const long long gi = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gi >= n) return;
    const int k = lab[gi];
    if (k == 0 || k >= n_class || parent[gi] != (int)gi) return;
    const int s = size[gi];
    const size_t cell = (size_t)(gi / plane) * n_class + k;
    atomicAdd(&count[cell], s);
    if (s >= keep_min) atomicAdd(&kept[cell], s);
    atomicMax(&keys[cell], ((unsigned long long)(unsigned)s << 32) | (0xFFFFFFFFu - (unsigned)first[gi]));
}

__global__ __launch_bounds__(256) void plane_largest_kernel(const unsigned long long *__restrict__ keys, int cells, int *__restrict__ largest) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < cells) largest[i] = (int)(keys[i] >> 32);
}

// mask = (the largest component of class a) | (the components of class b with at least keep_min voxels)
__global__ __launch_bounds__(256) void plane_mask_kernel(const unsigned char *__restrict__ lab, long long n, long long plane, int n_class, int a,
                                                         int b, int keep_min, const int *__restrict__ parent, const int *__restrict__ size,
                                                         const int *__restrict__ first, const unsigned long long *__restrict__ keys,
                                                         unsigned char *__restrict__ mask) {
    const long long gi = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gi >= n) return;
    const int k = lab[gi];
    unsigned char m = 0;
    if (k == a) {
        const unsigned long long key = keys[(size_t)(gi / plane) * n_class + a];   // non-zero: the class has a voxel, so a component
        m = (unsigned)first[root_of(parent, (int)gi)] == 0xFFFFFFFFu - (unsigned)key;
    } else if (k == b) {
        m = size[root_of(parent, (int)gi)] >= keep_min;
    }
    mask[gi] = m;
}

__global__ __launch_bounds__(256) void plane_union_kernel(const unsigned char *__restrict__ mask, long long n, long long plane,
                                                          const int *__restrict__ parent, const int *__restrict__ size, int *union_largest) {
    const long long gi = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gi >= n || !mask[gi] || parent[gi] != (int)gi) return;
    atomicMax(&union_largest[gi / plane], size[gi]);
}

// ---- atrial area and length (ukbb_fcn_atrial_area_length) -------------------------------------------------------------------
// cardiac_utils.evaluate_atrial_area_length (reference common/cardiac_utils.py:1655-1736) per (plane, class) cell, by the rules
// of ukbb_cardiac_amd/atrial.py (frame_stats_host is the specification; the numbers below are its).  The planes are labelled
// as for ukbb_fcn_plane_components; atrial_member_kernel then marks the voxels of every class's winning component, and one
// workgroup per cell works on that map alone.  Float64 throughout, every operation rounded once (-ffp-contract=off), in the
// order atrial.projection states; the order of the voxels is the integer order of (key of d, x*Y + y), so the thirds, the sums
// (integers) and the two extreme hits (integer minima / maxima) do not depend on which lane or wave comes first.
struct AtrialGeom {
    double a[12];                                       // rows 0..2 of the affine
    double l[3];                                        // the long axis
};

// member[gi] = k if voxel gi belongs to the largest component of its plane's class k (the earliest in scan order among equals)
__global__ __launch_bounds__(256) void atrial_member_kernel(const unsigned char *__restrict__ lab, long long n, long long plane, int n_class,
                                                            const int *__restrict__ parent, const int *__restrict__ first,
                                                            const unsigned long long *__restrict__ keys, unsigned char *__restrict__ member) {
    const long long gi = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gi >= n) return;
    const int k = lab[gi];
    unsigned char m = 0;
    if (k != 0 && k < n_class) {
        const unsigned long long key = keys[(size_t)(gi / plane) * n_class + k];   // non-zero: the class has a voxel here
        if ((unsigned)first[root_of(parent, (int)gi)] == 0xFFFFFFFFu - (unsigned)key) m = (unsigned char)k;
    }
    member[gi] = m;
}

// the order-preserving key of d(x, y); -0.0 counts as 0.0 (d + 0.0)
__device__ __forceinline__ unsigned long long atrial_key(const AtrialGeom &g, int x, int y) {
    const double fx = (double)x, fy = (double)y;
    const double w0 = (g.a[0] * fx + g.a[1] * fy) + g.a[3];
    const double w1 = (g.a[4] * fx + g.a[5] * fy) + g.a[7];
    const double w2 = (g.a[8] * fx + g.a[9] * fy) + g.a[11];
    const double d = ((w0 * g.l[0] + w1 * g.l[1]) + w2 * g.l[2]) + 0.0;
    const unsigned long long u = (unsigned long long)__double_as_longlong(d);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// cv::clipLine on [0, W-1] x [0, H-1] (atrial._clip_line); false: the line is rejected
__device__ bool atrial_clip(long long W, long long H, long long &x1, long long &y1, long long &x2, long long &y2) {
    const long long right = W - 1, bottom = H - 1;
    int c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8;
    int c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8;
    if ((c1 & c2) == 0 && (c1 | c2) != 0) {
        if (c1 & 12) {
            const long long a = c1 < 8 ? 0 : bottom;
            x1 += (long long)((double)(a - y1) * (double)(x2 - x1) / (double)(y2 - y1));
            y1 = a;
            c1 = (x1 < 0) + (x1 > right) * 2;
        }
        if (c2 & 12) {
            const long long a = c2 < 8 ? 0 : bottom;
            x2 += (long long)((double)(a - y2) * (double)(x2 - x1) / (double)(y2 - y1));
            y2 = a;
            c2 = (x2 < 0) + (x2 > right) * 2;
        }
        if ((c1 & c2) == 0 && (c1 | c2) != 0) {
            if (c1) {
                const long long a = c1 == 1 ? 0 : right;
                y1 += (long long)((double)(a - x1) * (double)(y2 - y1) / (double)(x2 - x1));
                x1 = a;
                c1 = 0;
            }
            if (c2) {
                const long long a = c2 == 1 ? 0 : right;
                y2 += (long long)((double)(a - x2) * (double)(y2 - y1) / (double)(x2 - x1));
                x2 = a;
                c2 = 0;
            }
        }
    }
    return (c1 | c2) == 0;
}

// grid (P * n_class), 256 threads: cell = plane * n_class + class; out[cell][8] = size, status, x0, y0, x1, y1, n_hits, 0
__global__ __launch_bounds__(256) void atrial_cell_kernel(const unsigned char *__restrict__ member, int X, int Y, int n_class,
                                                          const unsigned long long *__restrict__ keys, AtrialGeom g, int *__restrict__ out) {
    __shared__ int hist[2][256];
    __shared__ int scan[2][256];
    __shared__ int box[4];                              // x min, x max, y min, y max of the component
    __shared__ int sel_digit[2], sel_rank[2];
    __shared__ unsigned long long sums[4];              // sum x, sum y of the bottom third; of the top third
    __shared__ long long line[8];                       // status, start x, y (cv), major dx, dy, minor dx, dy, count
    __shared__ long long line_d[2];                     // dmaj, dmin
    __shared__ unsigned long long hit_key[2];           // the smallest and the largest key among the hits
    __shared__ unsigned hit_idx[2];
    __shared__ int n_hits;
    const int tid = threadIdx.x, cell = blockIdx.x, k = cell % n_class;
    int *o = out + (size_t)cell * 8;
    const unsigned long long win = k ? keys[cell] : 0;
    if (win == 0) {                                     // class 0, or no voxel of the class on this plane (uniform: all lanes leave)
        if (tid < 8) o[tid] = 0;
        return;
    }
    const int size = (int)(win >> 32);
    const unsigned char *pl = member + (size_t)(cell / n_class) * X * Y;
    const int plane = X * Y;                            // < 2^29
    if (tid == 0) {
        box[0] = X; box[1] = -1; box[2] = Y; box[3] = -1;
        sums[0] = sums[1] = sums[2] = sums[3] = 0;
        hit_key[0] = ~0ull; hit_key[1] = 0;
        hit_idx[0] = 0xFFFFFFFFu; hit_idx[1] = 0;
        n_hits = 0;
    }
    __syncthreads();
    {
        int x0 = X, x1 = -1, y0 = Y, y1 = -1;
        for (int gi = tid; gi < plane; gi += 256) {
            if (pl[gi] != k) continue;
            const int x = gi % X, y = gi / X;
            x0 = x < x0 ? x : x0; x1 = x > x1 ? x : x1;
            y0 = y < y0 ? y : y0; y1 = y > y1 ? y : y1;
        }
        if (x1 >= 0) {
            atomicMin(&box[0], x0); atomicMax(&box[1], x1);
            atomicMin(&box[2], y0); atomicMax(&box[3], y1);
        }
    }
    __syncthreads();
    const int bx0 = box[0], by0 = box[2], bw = box[1] - box[0] + 1, bh = box[3] - box[2] + 1;
    const long long bn = (long long)bw * bh;            // >= 1: the component has a voxel

    // the elements of ranks k1 and k2 in the order (key, x*Y + y): a most-significant-digit-first radix select over the 12 bytes
    unsigned long long sel_k[2] = {0, 0};
    unsigned sel_i[2] = {0, 0};
    int rank[2] = {(int)(size / 3), (int)(2 * (long long)size / 3)};
    for (int p = 0; p < 12; ++p) {
        hist[0][tid] = 0;
        hist[1][tid] = 0;
        __syncthreads();
        for (long long i = tid; i < bn; i += 256) {
            const int x = bx0 + (int)(i % bw), y = by0 + (int)(i / bw);
            if (pl[x + (size_t)X * y] != k) continue;
            const unsigned long long key = atrial_key(g, x, y);
            const unsigned idx = (unsigned)(x * Y + y);
            const int digit = p < 8 ? (int)((key >> (56 - 8 * p)) & 255) : (int)((idx >> (24 - 8 * (p - 8))) & 255);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                bool match;
                if (p == 0) match = true;
                else if (p <= 8) match = (key >> (64 - 8 * p)) == (sel_k[j] >> (64 - 8 * p));
                else match = key == sel_k[j] && (idx >> (32 - 8 * (p - 8))) == (sel_i[j] >> (32 - 8 * (p - 8)));
                if (match) atomicAdd(&hist[j][digit], 1);
            }
        }
        __syncthreads();
        const int h0 = hist[0][tid], h1 = hist[1][tid];
        scan[0][tid] = h0;
        scan[1][tid] = h1;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {       // inclusive prefix sums of the two histograms
            const int v0 = tid >= off ? scan[0][tid - off] : 0, v1 = tid >= off ? scan[1][tid - off] : 0;
            __syncthreads();
            scan[0][tid] += v0;
            scan[1][tid] += v1;
            __syncthreads();
        }
        const int e0 = scan[0][tid] - h0, e1 = scan[1][tid] - h1;
        if (e0 <= rank[0] && rank[0] < e0 + h0) { sel_digit[0] = tid; sel_rank[0] = rank[0] - e0; }     // one bin holds the rank
        if (e1 <= rank[1] && rank[1] < e1 + h1) { sel_digit[1] = tid; sel_rank[1] = rank[1] - e1; }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (p < 8) sel_k[j] |= (unsigned long long)sel_digit[j] << (56 - 8 * p);
            else sel_i[j] |= (unsigned)sel_digit[j] << (24 - 8 * (p - 8));
            rank[j] = sel_rank[j];
        }
        __syncthreads();                                // sel_digit is rewritten in the next pass
    }

    // coordinate sums of the bottom third (below the element of rank k1) and of the top third (from the element of rank k2 on)
    {
        unsigned long long s[4] = {0, 0, 0, 0};
        for (long long i = tid; i < bn; i += 256) {
            const int x = bx0 + (int)(i % bw), y = by0 + (int)(i / bw);
            if (pl[x + (size_t)X * y] != k) continue;
            const unsigned long long key = atrial_key(g, x, y);
            const unsigned idx = (unsigned)(x * Y + y);
            if (key < sel_k[0] || (key == sel_k[0] && idx < sel_i[0])) { s[0] += x; s[1] += y; }
            if (key > sel_k[1] || (key == sel_k[1] && idx >= sel_i[1])) { s[2] += x; s[3] += y; }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            for (int off = 32; off > 0; off >>= 1) s[j] += __shfl_xor(s[j], off);
            if ((tid & 63) == 0 && s[j]) atomicAdd(&sums[j], s[j]);
        }
    }
    __syncthreads();
    if (tid == 0) {                                     // the major axis, its end points, the clipped line
        const int k1 = size / 3, k2 = (int)(2 * (long long)size / 3);
        const double bx = (double)sums[0] / (double)k1, by = (double)sums[1] / (double)k1;       // k1 = 0: 0 / 0 = NaN
        const double cx = (double)sums[2] / (double)(size - k2), cy = (double)sums[3] / (double)(size - k2);
        double m0 = cx - bx, m1 = cy - by;
        const double norm = sqrt(m0 * m0 + m1 * m1);
        m0 = m0 / norm;
        m1 = m1 / norm;
        const double px = cx + 100.0 * m0, py = cy + 100.0 * m1, qx = cx - 100.0 * m0, qy = cy - 100.0 * m1;
        long long st = 2;
        if (px == px && py == py && qx == qx && qy == qy) {
            // cv points are (y, x): width Y, height X
            long long x1 = (long long)qy, y1 = (long long)qx, x2 = (long long)py, y2 = (long long)px;
            st = 3;
            if (atrial_clip(Y, X, x1, y1, x2, y2)) {
                long long dx = x2 - x1, dy = y2 - y1, sy = 1;
                if (dx < 0) { dx = -dx; dy = -dy; x1 = x2; y1 = y2; }
                if (dy < 0) { dy = -dy; sy = -1; }
                st = 1;
                line[1] = x1; line[2] = y1;
                if (dy > dx) {
                    line[3] = 0; line[4] = sy; line[5] = 1; line[6] = 0; line[7] = dy + 1;
                    line_d[0] = dy; line_d[1] = dx;
                } else {
                    line[3] = 1; line[4] = 0; line[5] = 0; line[6] = sy; line[7] = dx + 1;
                    line_d[0] = dx; line_d[1] = dy;
                }
            }
        }
        line[0] = st;
    }
    __syncthreads();
    int status = (int)line[0];
    if (status == 1) {
        // pixel i of the line in closed form: i major steps and ceil((2 dmin i - dmaj) / (2 dmaj)) minor steps (atrial.minor_steps)
        const long long count = line[7], dmaj = line_d[0], dmin = line_d[1];
        for (int pass = 0; pass < 2; ++pass) {
            for (long long i = tid; i < count; i += 256) {
                const long long mi = dmaj == 0 ? 0 : (2 * dmin * i + dmaj - 1) / (2 * dmaj);
                const long long cvx = line[1] + i * line[3] + mi * line[5], cvy = line[2] + i * line[4] + mi * line[6];
                if (cvx < 0 || cvx >= Y || cvy < 0 || cvy >= X) continue;           // never after the clip; a guard all the same
                const int x = (int)cvy, y = (int)cvx;
                if (pl[x + (size_t)X * y] != k) continue;
                const unsigned long long key = atrial_key(g, x, y);
                const unsigned idx = (unsigned)(x * Y + y);
                if (pass == 0) {
                    atomicMin(&hit_key[0], key);
                    atomicMax(&hit_key[1], key);
                    atomicAdd(&n_hits, 1);
                } else {
                    if (key == hit_key[0]) atomicMin(&hit_idx[0], idx);
                    if (key == hit_key[1]) atomicMax(&hit_idx[1], idx);
                }
            }
            __syncthreads();
        }
        if (n_hits == 0) status = 3;
    }
    if (tid == 0) {
        const bool ok = status == 1;
        o[0] = size;
        o[1] = status;
        o[2] = ok ? (int)(hit_idx[0] / (unsigned)Y) : 0;
        o[3] = ok ? (int)(hit_idx[0] % (unsigned)Y) : 0;
        o[4] = ok ? (int)(hit_idx[1] / (unsigned)Y) : 0;
        o[5] = ok ? (int)(hit_idx[1] % (unsigned)Y) : 0;
        o[6] = ok ? n_hits : 0;
        o[7] = 0;
    }
}

// ---- masked maximum ----------------------------------------------------------------------------------------------------
// The maximum as an unsigned key whose integer order is numpy's: NaN above everything (np.max propagates it), then the value
// order; 0 = no voxel (the key of every value is >= 1).  Integer maxima are order-independent, so the result does not depend
// on which workgroup comes first; the keys live in the 8-byte output cells until label_max_final_kernel decodes them in place.
__device__ __forceinline__ unsigned long long max_key(float v) {
    if (v != v) return 0x100000000ull;
    const unsigned u = __float_as_uint(v);
    return (unsigned long long)((u & 0x80000000u) ? ~u : (u | 0x80000000u)) + 1;   // -0 < +0; every key >= 0x7FFFFF + 1
}
__device__ __forceinline__ unsigned long long max_key(uint8_t v) { return (unsigned long long)v + 1; }
__device__ __forceinline__ unsigned long long max_key(uint16_t v) { return (unsigned long long)v + 1; }
__device__ __forceinline__ unsigned long long max_key(int16_t v) { return (unsigned long long)(v + 32768) + 1; }

template <typename T> __device__ double key_value(unsigned long long k);
template <> __device__ double key_value<float>(unsigned long long k) {
    if (k == 0x100000000ull) return __longlong_as_double(0x7FF8000000000000ll);
    const unsigned u = (unsigned)(k - 1);
    return (double)__uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}
template <> __device__ double key_value<uint8_t>(unsigned long long k) { return (double)(k - 1); }
template <> __device__ double key_value<uint16_t>(unsigned long long k) { return (double)(k - 1); }
template <> __device__ double key_value<int16_t>(unsigned long long k) { return (double)((long long)k - 1 - 32768); }

constexpr int MAX_CHUNK = 4096;                         // voxels of one frame per workgroup (16 per thread)

// grid (chunks of a frame, T), 256 threads; keys [T][n_class] as uint64 in the output cells (zeroed by the caller)
template <typename T>
__global__ __launch_bounds__(256) void label_max_kernel(const T *__restrict__ vol, const unsigned char *__restrict__ lab, int X, int Y,
                                                        long long frame, long long sx, long long sy, long long sz, long long st, int n_class,
                                                        unsigned long long *keys) {
    const int t = blockIdx.y;
    unsigned long long best[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) best[c] = 0;
    const long long i0 = (long long)blockIdx.x * MAX_CHUNK;
    const long long i1 = i0 + MAX_CHUNK < frame ? i0 + MAX_CHUNK : frame;
    for (long long i = i0 + threadIdx.x; i < i1; i += 256) {    // x fastest across the lanes: coalesced for F-ordered volumes
        const int k = lab[frame * t + i];
        if (k >= n_class) continue;
        const int x = (int)(i % X);
        const long long r = i / X;
        const int y = (int)(r % Y), z = (int)(r / Y);
        const unsigned long long key = max_key(vol[x * sx + y * sy + z * sz + t * st]);
#pragma unroll
        for (int c = 0; c < MAXC; ++c)                  // unrolled selects keep best[] in registers
            if (c == k && key > best[c]) best[c] = key;
    }
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        if (c >= n_class) continue;                     // uniform: no divergence, and the loop stays unrolled
        unsigned long long b = best[c];
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long u = __shfl_xor(b, o);
            b = u > b ? u : b;
        }
        if ((threadIdx.x & 63) == 0 && b) atomicMax(&keys[(size_t)t * n_class + c], b);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void label_max_final_kernel(unsigned long long *keys, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = keys[i];
    reinterpret_cast<double *>(keys)[i] = k ? key_value<T>(k) : -INFINITY;      // an empty mask: the identity of max
}

template <typename T>
int label_max_impl(const T *d_vol, int X, int Y, int Z, int T_, int64_t sx, int64_t sy, int64_t sz, int64_t st, const uint8_t *d_lab,
                   int n_class, double *d_max, hipStream_t s) {
    const long long frame = (long long)X * Y * Z;
    const int n = T_ * n_class;
    if (hipMemsetAsync(d_max, 0, sizeof(double) * (size_t)n, s) != hipSuccess) { set_error("label_max: memset failed"); return UKBB_EDEVICE; }
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(d_max);
    hipLaunchKernelGGL((label_max_kernel<T>), dim3((unsigned)((frame + MAX_CHUNK - 1) / MAX_CHUNK), (unsigned)T_), dim3(256), 0, s,
                       d_vol, d_lab, X, Y, frame, (long long)sx, (long long)sy, (long long)sz, (long long)st, n_class, keys);
    hipLaunchKernelGGL((label_max_final_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, keys, n);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("label_max: launch failed: %s", hipGetErrorString(e)); return UKBB_EDEVICE; }
    return UKBB_OK;
}

}  // namespace
}  // namespace ukbb

using namespace ukbb;

extern "C" {

int ukbb_fcn_label_components(const uint8_t *d_lab, int X, int Y, int Z, int T, int n_class, int min_size, int32_t *d_work,
                              int32_t *d_n_large, void *stream) {
    const long long n = (long long)X * Y * Z * T;
    if (!d_lab || !d_work || !d_n_large || X < 1 || Y < 1 || Z < 1 || T < 1 || n_class < 1 || n_class > MAXC ||
        (long long)Z * T > 65535 || 2 * n > 0x7FFFFFFFll) {
        set_error("label_components: bad argument (n_class 1..16, Z*T <= 65535, 2*X*Y*Z*T < 2^31)");
        return UKBB_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    int *parent = d_work, *size = d_work + n;
    if (hipMemsetAsync(d_n_large, 0, sizeof(int32_t) * (size_t)T * n_class, s) != hipSuccess) {
        set_error("label_components: memset failed");
        return UKBB_EDEVICE;
    }
    const unsigned tiles = (unsigned)(((X + TILE - 1) / TILE) * ((Y + TILE - 1) / TILE));
    const unsigned nb = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(ccl_local_kernel, dim3(tiles, (unsigned)(Z * T)), dim3(256), 0, s, d_lab, X, Y, parent, size);
    hipLaunchKernelGGL(ccl_border_kernel, dim3(nb), dim3(256), 0, s, d_lab, X, Y, Z, n, parent);
    hipLaunchKernelGGL(ccl_size_kernel, dim3(nb), dim3(256), 0, s, d_lab, n, (const int *)parent, size);
    hipLaunchKernelGGL(ccl_count_kernel, dim3(nb), dim3(256), 0, s, d_lab, n, (long long)X * Y * Z, n_class, min_size,
                       (const int *)parent, (const int *)size, d_n_large);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("label_components: launch failed: %s", hipGetErrorString(e)); return UKBB_EDEVICE; }
    return UKBB_OK;
}

int ukbb_fcn_plane_components(const uint8_t *d_planes, int X, int Y, int P, int n_class, int a, int b, int keep_min, int32_t *d_work,
                              int32_t *d_count, int32_t *d_largest, int32_t *d_kept, int32_t *d_union_largest, void *stream) {
    // X*Y < 2^62 for any two ints, and once it is known to be below 2^29 the product with P <= 65535 cannot overflow either
    const long long plane = X >= 1 && Y >= 1 ? (long long)X * Y : 0;
    const long long n = plane >= 1 && plane <= 0x1FFFFFFFll && P >= 1 && P <= 65535 ? plane * P : 0;
    if (!d_planes || !d_work || !d_count || !d_largest || !d_kept || !d_union_largest || n < 1 || 4 * n > 0x7FFFFFFFll ||
        n_class < 1 || n_class > MAXC || a < 1 || a >= n_class || b < 1 || b >= n_class || a == b || ((uintptr_t)d_work & 7)) {
        set_error("plane_components: bad argument (n_class 1..16, 1 <= a != b < n_class, P <= 65535, 4*X*Y*P < 2^31, d_work 8-byte aligned)");
        return UKBB_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    const int cells = P * n_class;
    // d_work: keys [P*n_class] uint64 | parent [n] | size [n] | first [n] int32 | mask [n] uint8
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(d_work);
    int *parent = d_work + 2 * (size_t)cells, *size = parent + n, *first = size + n;
    unsigned char *mask = reinterpret_cast<unsigned char *>(first + n);
    const unsigned tiles = (unsigned)(((X + TILE - 1) / TILE) * ((Y + TILE - 1) / TILE));
    const unsigned nb = (unsigned)((n + 255) / 256);
    const unsigned nb_init = (unsigned)(((n > cells ? n : (long long)cells) + 255) / 256);
    hipLaunchKernelGGL(plane_init_kernel, dim3(nb_init), dim3(256), 0, s, n, cells, P, first, keys, d_count, d_kept, d_union_largest);
    hipLaunchKernelGGL(ccl_local_kernel, dim3(tiles, (unsigned)P), dim3(256), 0, s, d_planes, X, Y, parent, size);
    hipLaunchKernelGGL(ccl_border_kernel, dim3(nb), dim3(256), 0, s, d_planes, X, Y, 1, n, parent);
    hipLaunchKernelGGL(ccl_size_kernel, dim3(nb), dim3(256), 0, s, d_planes, n, (const int *)parent, size);
    hipLaunchKernelGGL(plane_first_kernel, dim3(nb), dim3(256), 0, s, d_planes, X, Y, n, (const int *)parent, first);
    hipLaunchKernelGGL(plane_root_kernel, dim3(nb), dim3(256), 0, s, d_planes, n, plane, n_class, keep_min, (const int *)parent,
                       (const int *)size, (const int *)first, keys, d_count, d_kept);
    hipLaunchKernelGGL(plane_largest_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, (const unsigned long long *)keys, cells,
                       d_largest);
    hipLaunchKernelGGL(plane_mask_kernel, dim3(nb), dim3(256), 0, s, d_planes, n, plane, n_class, a, b, keep_min, (const int *)parent,
                       (const int *)size, (const int *)first, (const unsigned long long *)keys, mask);
    // the same labeller on the derived mask; only the largest size is asked for, so the key is the size itself
    hipLaunchKernelGGL(ccl_local_kernel, dim3(tiles, (unsigned)P), dim3(256), 0, s, (const unsigned char *)mask, X, Y, parent, size);
    hipLaunchKernelGGL(ccl_border_kernel, dim3(nb), dim3(256), 0, s, (const unsigned char *)mask, X, Y, 1, n, parent);
    hipLaunchKernelGGL(ccl_size_kernel, dim3(nb), dim3(256), 0, s, (const unsigned char *)mask, n, (const int *)parent, size);
    hipLaunchKernelGGL(plane_union_kernel, dim3(nb), dim3(256), 0, s, (const unsigned char *)mask, n, plane, (const int *)parent,
                       (const int *)size, d_union_largest);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("plane_components: launch failed: %s", hipGetErrorString(e)); return UKBB_EDEVICE; }
    return UKBB_OK;
}

int ukbb_fcn_atrial_area_length(const uint8_t *d_planes, int X, int Y, int P, int n_class, const double affine[12], const double long_axis[3],
                                int32_t *d_work, int32_t *d_out, void *stream) {
    const long long plane = X >= 1 && Y >= 1 ? (long long)X * Y : 0;
    const long long n = plane >= 1 && plane <= 0x1FFFFFFFll && P >= 1 && P <= 65535 ? plane * P : 0;
    bool finite = affine && long_axis;
    for (int i = 0; finite && i < 12; ++i) finite = std::isfinite(affine[i]);
    for (int i = 0; finite && i < 3; ++i) finite = std::isfinite(long_axis[i]);
    if (!d_planes || !d_work || !d_out || !finite || n < 1 || 4 * n > 0x7FFFFFFFll || n_class < 1 || n_class > MAXC ||
        ((uintptr_t)d_work & 7)) {
        set_error("atrial_area_length: bad argument (n_class 1..16, P <= 65535, 4*X*Y*P < 2^31, finite affine and long axis, d_work 8-byte aligned)");
        return UKBB_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    const int cells = P * n_class;
    // d_work: keys [P*n_class] uint64 | parent [n] | size [n] | first [n] int32 | member [n] uint8
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(d_work);
    int *parent = d_work + 2 * (size_t)cells, *size = parent + n, *first = size + n;
    unsigned char *member = reinterpret_cast<unsigned char *>(first + n);
    // the class totals plane_init_kernel / plane_root_kernel also keep are not asked for here: they go to the first 2*cells + P
    // of the 8*cells output cells, every one of which atrial_cell_kernel writes afterwards
    int *count = d_out, *kept = d_out + cells, *unused = d_out + 2 * (size_t)cells;
    AtrialGeom g;
    for (int i = 0; i < 12; ++i) g.a[i] = affine[i];
    for (int i = 0; i < 3; ++i) g.l[i] = long_axis[i];
    const unsigned tiles = (unsigned)(((X + TILE - 1) / TILE) * ((Y + TILE - 1) / TILE));
    const unsigned nb = (unsigned)((n + 255) / 256);
    const unsigned nb_init = (unsigned)(((n > cells ? n : (long long)cells) + 255) / 256);
    hipLaunchKernelGGL(plane_init_kernel, dim3(nb_init), dim3(256), 0, s, n, cells, P, first, keys, count, kept, unused);
    hipLaunchKernelGGL(ccl_local_kernel, dim3(tiles, (unsigned)P), dim3(256), 0, s, d_planes, X, Y, parent, size);
    hipLaunchKernelGGL(ccl_border_kernel, dim3(nb), dim3(256), 0, s, d_planes, X, Y, 1, n, parent);
    hipLaunchKernelGGL(ccl_size_kernel, dim3(nb), dim3(256), 0, s, d_planes, n, (const int *)parent, size);
    hipLaunchKernelGGL(plane_first_kernel, dim3(nb), dim3(256), 0, s, d_planes, X, Y, n, (const int *)parent, first);
    hipLaunchKernelGGL(plane_root_kernel, dim3(nb), dim3(256), 0, s, d_planes, n, plane, n_class, 1, (const int *)parent, (const int *)size,
                       (const int *)first, keys, count, kept);
    hipLaunchKernelGGL(atrial_member_kernel, dim3(nb), dim3(256), 0, s, d_planes, n, plane, n_class, (const int *)parent, (const int *)first,
                       (const unsigned long long *)keys, member);
    hipLaunchKernelGGL(atrial_cell_kernel, dim3((unsigned)cells), dim3(256), 0, s, (const unsigned char *)member, X, Y, n_class,
                       (const unsigned long long *)keys, g, d_out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("atrial_area_length: launch failed: %s", hipGetErrorString(e)); return UKBB_EDEVICE; }
    return UKBB_OK;
}

int ukbb_fcn_label_max(const void *d_vol, int nifti_datatype, int X, int Y, int Z, int T, int64_t sx, int64_t sy, int64_t sz, int64_t st,
                       const uint8_t *d_lab, int n_class, double *d_max, void *stream) {
    if (!d_vol || !d_lab || !d_max || X < 1 || Y < 1 || Z < 1 || T < 1 || T > 65535 || n_class < 1 || n_class > MAXC) {
        set_error("label_max: bad argument (n_class 1..16, T <= 65535)");
        return UKBB_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    switch (nifti_datatype) {
    case 16: return label_max_impl(static_cast<const float *>(d_vol), X, Y, Z, T, sx, sy, sz, st, d_lab, n_class, d_max, s);
    case 2: return label_max_impl(static_cast<const uint8_t *>(d_vol), X, Y, Z, T, sx, sy, sz, st, d_lab, n_class, d_max, s);
    case 4: return label_max_impl(static_cast<const int16_t *>(d_vol), X, Y, Z, T, sx, sy, sz, st, d_lab, n_class, d_max, s);
    case 512: return label_max_impl(static_cast<const uint16_t *>(d_vol), X, Y, Z, T, sx, sy, sz, st, d_lab, n_class, d_max, s);
    default:
        set_error("label_max: NIfTI datatype %d is not supported (16 float32, 2 uint8, 4 int16, 512 uint16)", nifti_datatype);
        return UKBB_EINVAL;
    }
}

}  // extern "C"
