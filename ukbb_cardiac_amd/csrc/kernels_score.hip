// Overlap and contour distances of two label volumes (reference common/image_utils.py:171-224: np_categorical_dice and
// distance_metric), per (plane, class) cell, on the labels ukbb_fcn_unpack_labels left in HBM and a second label volume of the
// same layout.  ukbb_cardiac_amd/seg_score.py states the semantics (stats_host is the specification):
//
//   nA, nB, nAB          pixels of pred == k, truth == k, both
//   C(M)                 the contour set of a mask: its pixels with a 4-neighbour off the image or in the OUTER background (the
//                        non-M pixels 4-connected to the image frame) -- what cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_NONE)
//                        visits, as a set
//   cA, cB               |C(A)|, |C(B)|
//   hA, hB               max over C(A) of mA(a) = min over b in C(B) of |a - b|^2, and the other way round (int32, exact)
//   sA, sB               sum over C(A) of sqrt(float64(mA)) in the order x*Y + y, added as np.add.reduce adds a contiguous array
//
// One workgroup per cell (a grid-stride loop over the cells).  The two masks are bit planes in LDS (bits along x, one row of
// W = ceil(X/32) words per y); per mask:
//   1. flood    the outer background grows from the frame to a fixed point: every word takes its four neighbours' bits and smears
//               them along its own free bits (Kogge-Stone occluded fill); passes repeat until one changes nothing.  Monotone, so
//               reading a neighbour's old or new word within a pass are both right.
//   2. contour  M & (outer background shifted four ways | frame), in place of the mask; the count from popcounts
// and per direction (A against B, B against A) the exact two-phase squared Euclidean transform:
//   3. columns  g(x, y) = distance along y to the nearest contour pixel of the OTHER mask (two scans per column, uint16 in HBM)
//   4. points   the contour pixels of THIS mask in the order x*Y + y (a column count, its prefix sum, one rank per pixel), then
//               one thread per pixel: min over x' of (x - x')^2 + g(x', y)^2, walking outwards from x until dx^2 reaches the
//               minimum so far.  X*Y + c*X steps at most, whatever the labels are: no capacity, no decline path.
//   5. sums     sqrt of the minima along numpy's pairwise tree: one thread per leaf (pairwise_leaf, device_prims.h), one thread
//               combines the leaves, one tree per 8192-element buffer of numpy's reduction iterator, buffers in sequence.
// Integer minima, maxima and adds only; the float64 additions have a fixed order: nothing depends on arrival order.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/ukbb_fcn.h"
#include "device_prims.h"
#include "kernels.h"

namespace ukbb {

namespace {

constexpr int MAXC = 16;                                // classes per call (as ukbb_fcn_unpack_labels)
constexpr int SCORE_MAX_EDGE = 1024;                    // X, Y <= this (the column counts live in LDS; g is uint16)
constexpr int SCORE_MAX_WORDS = 8192;                   // ceil(X/32) * Y <= this: three bit planes of 32 KB each (512 x 512)
constexpr int SCORE_THREADS = 256;
constexpr int SCORE_MAX_GRID = 1024;                    // workgroups per launch at most; the cells beyond take the grid-stride loop
constexpr uint64_t SCORE_WORK_BUDGET = 64ull << 20;     // bytes of d_work at most (one workgroup's share: always granted)
constexpr unsigned G_INF = 0xFFFFu;                     // no contour pixel of the other mask in this column
constexpr int NPY_BUF = 8192;                           // elements per buffer of numpy's reduction iterator (np.getbufsize())
constexpr int MAX_LEAVES = 256;                         // leaves of one buffer's tree: every leaf of a split node has >= 57 elements

// bytes of d_work one workgroup owns: g [X*Y rounded up to even] uint16 | the minima of the contour pixels, compacted [X*Y] int32
__host__ __device__ inline uint64_t score_wg_bytes(int X, int Y) { return ((uint64_t)X * Y * 6 + 2 + 15) & ~15ull; }

inline int score_grid(int X, int Y, int P, int n_class) {
    const uint64_t cells = (uint64_t)P * (n_class - 1);
    uint64_t g = SCORE_WORK_BUDGET / score_wg_bytes(X, Y);
    if (g > SCORE_MAX_GRID) g = SCORE_MAX_GRID;
    if (g > cells) g = cells;
    return g < 1 ? 1 : (int)g;
}

inline bool score_shape_ok(int X, int Y, int P, int n_class) {
    return X >= 1 && Y >= 1 && X <= SCORE_MAX_EDGE && Y <= SCORE_MAX_EDGE && ((X + 31) / 32) * Y <= SCORE_MAX_WORDS && P >= 1 && P <= 65535 &&
           n_class >= 2 && n_class <= MAXC;
}

// seed & f spread along the runs of set bits of f, both ways (Kogge-Stone occluded fill)
__device__ __forceinline__ unsigned smear(unsigned seed, unsigned f) {
    unsigned o = seed & f, m = f;
    o |= (o << 1) & m; m &= m << 1;
    o |= (o << 2) & m; m &= m << 2;
    o |= (o << 4) & m; m &= m << 4;
    o |= (o << 8) & m; m &= m << 8;
    o |= (o << 16) & m;
    m = f;
    o |= (o >> 1) & m; m &= m >> 1;
    o |= (o >> 2) & m; m &= m >> 2;
    o |= (o >> 4) & m; m &= m >> 4;
    o |= (o >> 8) & m; m &= m >> 8;
    o |= (o >> 16) & m;
    return o;
}

// numpy's pairwise_sum over n <= 8192 elements, by an explicit stack: leaf(off, len) -> the sum of one leaf (<= 128 elements), in order
template <class F>
__device__ double pairwise_walk(int n, F &&leaf) {
    int nn[16], ph[16];
    double left[16];
    int sp = 0, off = 0;
    double ret = 0.0;
    nn[0] = n; ph[0] = 0;
    for (;;) {
        if (ph[sp] == 0) {
            if (nn[sp] > 128 && sp < 15) {              // split: n2 = n / 2 rounded down to a multiple of 8
                int n2 = nn[sp] / 2;
                n2 -= n2 % 8;
                ph[sp] = 1;
                nn[sp + 1] = n2; ph[sp + 1] = 0;
                ++sp;
                continue;
            }
            ret = leaf(off, nn[sp]);
            off += nn[sp];
        } else if (ph[sp] == 1) {                       // the left half is in ret
            int n2 = nn[sp] / 2;
            n2 -= n2 % 8;
            left[sp] = ret;
            ph[sp] = 2;
            nn[sp + 1] = nn[sp] - n2; ph[sp + 1] = 0;
            ++sp;
            continue;
        } else {
            ret = left[sp] + ret;
        }
        if (sp == 0) return ret;
        --sp;
    }
}

struct ScoreShared {
    int cnt[8];                                         // nA, nB, nAB, cA, cB, hA, hB, changed
    int col[SCORE_MAX_EDGE + 1];                        // contour pixels per column, then their exclusive prefix sum
    int leaf_off[MAX_LEAVES], leaf_len[MAX_LEAVES], n_leaf;
    double leaf_sum[MAX_LEAVES], total;
};

// grid: min(cells, cap) workgroups of SCORE_THREADS; dynamic LDS: 3 * W * Y words
__global__ __launch_bounds__(SCORE_THREADS) void score_planes_kernel(const unsigned char *__restrict__ pred, const unsigned char *__restrict__ truth,
                                                                     int X, int Y, int P, int n_class, unsigned char *__restrict__ work,
                                                                     int *__restrict__ cells, double *__restrict__ sums) {
    extern __shared__ unsigned planes[];
    __shared__ ScoreShared sh;
    const int tid = threadIdx.x, W = (X + 31) >> 5, NW = W * Y;
    unsigned *mk[2] = {planes, planes + NW};            // mask, then contour, of pred == k and of truth == k
    unsigned *O = planes + 2 * NW;                      // the outer background of the mask in hand
    const unsigned last_valid = (X & 31) ? (1u << (X & 31)) - 1u : 0xFFFFFFFFu;
    unsigned short *g = reinterpret_cast<unsigned short *>(work + (size_t)blockIdx.x * score_wg_bytes(X, Y));
    int *mins = reinterpret_cast<int *>(g + (((size_t)X * Y + 1) & ~(size_t)1));
    const int n_cell = P * (n_class - 1);

    for (int cell = blockIdx.x; cell < n_cell; cell += gridDim.x) {
        const int p = cell / (n_class - 1), k = 1 + cell % (n_class - 1);
        const unsigned char *pa = pred + (size_t)p * X * Y, *pb = truth + (size_t)p * X * Y;
        if (tid < 8) sh.cnt[tid] = 0;
        __syncthreads();

        // ---- the two masks as bit planes, and the three overlap counts
        int nA = 0, nB = 0, nAB = 0;
        for (int w = tid; w < NW; w += SCORE_THREADS) {
            const int y = w / W, x0 = (w - y * W) << 5, nx = X - x0 < 32 ? X - x0 : 32;
            const size_t at = (size_t)y * X + x0;
            unsigned a = 0, b = 0;
            for (int i = 0; i < nx; ++i) {
                a |= (unsigned)(pa[at + i] == k) << i;
                b |= (unsigned)(pb[at + i] == k) << i;
            }
            mk[0][w] = a; mk[1][w] = b;
            nA += __popc(a); nB += __popc(b); nAB += __popc(a & b);
        }
        if (nA) atomicAdd(&sh.cnt[0], nA);
        if (nB) atomicAdd(&sh.cnt[1], nB);
        if (nAB) atomicAdd(&sh.cnt[2], nAB);
        __syncthreads();
        const bool defined = sh.cnt[0] > 0 && sh.cnt[1] > 0;   // the same for every thread
        double total[2] = {0.0, 0.0};

        if (defined) {
            // ---- flood and contour, mask by mask
            for (int s = 0; s < 2; ++s) {
                unsigned *M = mk[s];
                for (int w = tid; w < NW; w += SCORE_THREADS) {
                    const int y = w / W, xw = w - y * W;
                    const unsigned valid = xw == W - 1 ? last_valid : 0xFFFFFFFFu;
                    unsigned frame = (y == 0 || y == Y - 1) ? valid : 0u;
                    if (xw == 0) frame |= 1u;
                    if (xw == W - 1) frame |= 1u << ((X - 1) & 31);
                    O[w] = frame & ~M[w] & valid;
                }
                __syncthreads();
                for (;;) {
                    int changed = 0;
                    for (int w = tid; w < NW; w += SCORE_THREADS) {
                        const int y = w / W, xw = w - y * W;
                        const unsigned f = ~M[w] & (xw == W - 1 ? last_valid : 0xFFFFFFFFu);
                        const unsigned o = O[w];
                        unsigned seed = o;
                        if (y > 0) seed |= O[w - W];
                        if (y < Y - 1) seed |= O[w + W];
                        if (xw > 0) seed |= O[w - 1] >> 31;
                        if (xw < W - 1) seed |= O[w + 1] << 31;
                        const unsigned grown = smear(seed, f);
                        if (grown != o) { O[w] = grown; changed = 1; }
                    }
                    if (!__syncthreads_or(changed)) break;     // a pass that wrote nothing read a state at rest: the fixed point
                }
                int c = 0;
                for (int w = tid; w < NW; w += SCORE_THREADS) {
                    const int y = w / W, xw = w - y * W;
                    const unsigned valid = xw == W - 1 ? last_valid : 0xFFFFFFFFu;
                    const unsigned o = O[w];
                    unsigned near = (o << 1) | (o >> 1);
                    if (xw > 0) near |= O[w - 1] >> 31;
                    if (xw < W - 1) near |= O[w + 1] << 31;
                    if (y > 0) near |= O[w - W];
                    if (y < Y - 1) near |= O[w + W];
                    if (y == 0 || y == Y - 1) near |= valid;
                    if (xw == 0) near |= 1u;
                    if (xw == W - 1) near |= 1u << ((X - 1) & 31);
                    const unsigned cw = M[w] & near & valid;
                    M[w] = cw;                                 // only this thread reads M[w]
                    c += __popc(cw);
                }
                if (c) atomicAdd(&sh.cnt[3 + s], c);
                __syncthreads();                               // O is rewritten for the next mask; the contours are complete
            }

            // ---- the distances, direction by direction: the contour of mask s against the contour of mask 1 - s
            for (int s = 0; s < 2; ++s) {
                const unsigned *CT = mk[s], *CO = mk[1 - s];
                const int n_pts = sh.cnt[3 + s];
                for (int x = tid; x < X; x += SCORE_THREADS) {
                    const int xw = x >> 5;
                    const unsigned bit = 1u << (x & 31);
                    unsigned d = G_INF;
                    int c = 0;
                    for (int y = 0; y < Y; ++y) {
                        if (CO[y * W + xw] & bit) d = 0; else if (d != G_INF) ++d;
                        g[(size_t)y * X + x] = (unsigned short)d;
                        c += (CT[y * W + xw] & bit) != 0;
                    }
                    d = G_INF;
                    for (int y = Y - 1; y >= 0; --y) {
                        if (CO[y * W + xw] & bit) d = 0; else if (d != G_INF) ++d;
                        if (d < g[(size_t)y * X + x]) g[(size_t)y * X + x] = (unsigned short)d;
                    }
                    sh.col[x] = c;
                }
                __syncthreads();
                if (tid == 0) {                                // exclusive prefix sum over the columns: X <= 1024 steps
                    int run = 0;
                    for (int x = 0; x < X; ++x) { const int c = sh.col[x]; sh.col[x] = run; run += c; }
                    sh.col[X] = run;
                }
                __syncthreads();
                for (int x = tid; x < X; x += SCORE_THREADS) {   // the contour pixels of this mask in the order x*Y + y
                    const int xw = x >> 5;
                    const unsigned bit = 1u << (x & 31);
                    int pos = sh.col[x];
                    for (int y = 0; y < Y; ++y)
                        if ((CT[y * W + xw] & bit) && pos < n_pts) mins[pos++] = (x << 16) | y;
                }
                __syncthreads();
                int h = 0;
                for (int i = tid; i < n_pts; i += SCORE_THREADS) {
                    const int x = mins[i] >> 16, y = mins[i] & 0xFFFF;
                    const unsigned short *row = g + (size_t)y * X;
                    const unsigned g0 = row[x];
                    int best = g0 == G_INF ? 0x7FFFFFFF : (int)(g0 * g0);
                    for (int dx = 1; dx * dx < best && (x - dx >= 0 || x + dx < X); ++dx) {
                        if (x - dx >= 0) {
                            const unsigned v = row[x - dx];
                            if (v != G_INF) { const int d2 = dx * dx + (int)(v * v); best = d2 < best ? d2 : best; }
                        }
                        if (x + dx < X) {
                            const unsigned v = row[x + dx];
                            if (v != G_INF) { const int d2 = dx * dx + (int)(v * v); best = d2 < best ? d2 : best; }
                        }
                    }
                    mins[i] = best;
                    h = best > h ? best : h;
                }
                if (h) atomicMax(&sh.cnt[5 + s], h);
                __syncthreads();

                // ---- sum of the square roots along numpy's tree, one buffer of the reduction iterator after the other
                if (tid == 0) sh.total = 0.0;
                for (int b0 = 0; b0 < n_pts; b0 += NPY_BUF) {
                    const int nb = n_pts - b0 < NPY_BUF ? n_pts - b0 : NPY_BUF;
                    if (tid == 0) {
                        int nl = 0;
                        pairwise_walk(nb, [&](int off, int len) {
                            if (nl < MAX_LEAVES) { sh.leaf_off[nl] = b0 + off; sh.leaf_len[nl] = len; ++nl; }
                            return 0.0;
                        });
                        sh.n_leaf = nl;
                    }
                    __syncthreads();
                    for (int l = tid; l < sh.n_leaf; l += SCORE_THREADS) {
                        const int *m = mins + sh.leaf_off[l];
                        sh.leaf_sum[l] = pairwise_leaf<double>(sh.leaf_len[l], [&](int i) { return __dsqrt_rn((double)m[i]); });
                    }
                    __syncthreads();
                    if (tid == 0) {
                        int l = 0;
                        const double tree = pairwise_walk(nb, [&](int, int) { const double v = sh.leaf_sum[l < MAX_LEAVES ? l : MAX_LEAVES - 1]; ++l; return v; });
                        sh.total = sh.total + tree;            // add.reduce starts from 0 and adds one pairwise sum per buffer
                    }
                    __syncthreads();
                }
                __syncthreads();
                total[s] = sh.total;
                __syncthreads();                               // g, mins and sh.col are rewritten by the other direction
            }
        }

        if (tid == 0) {
            int *out = cells + ((size_t)p * n_class + k) * 8;
            out[0] = defined ? 1 : 0;
            out[1] = sh.cnt[0]; out[2] = sh.cnt[1]; out[3] = sh.cnt[2];
            out[4] = defined ? sh.cnt[3] : 0; out[5] = defined ? sh.cnt[4] : 0;
            out[6] = defined ? sh.cnt[5] : 0; out[7] = defined ? sh.cnt[6] : 0;
            double *so = sums + ((size_t)p * n_class + k) * 2;
            so[0] = total[0]; so[1] = total[1];
        }
        __syncthreads();                                       // sh.cnt is cleared for the next cell
    }
}

}  // namespace
}  // namespace ukbb

using namespace ukbb;

extern "C" {

uint64_t ukbb_fcn_score_planes_work(int X, int Y, int P, int n_class) {
    if (!score_shape_ok(X, Y, P, n_class)) return 0;
    return (uint64_t)score_grid(X, Y, P, n_class) * score_wg_bytes(X, Y);
}

int ukbb_fcn_score_planes(const uint8_t *d_pred, const uint8_t *d_truth, int X, int Y, int P, int n_class, void *d_work, int32_t *d_cells,
                          double *d_sums, void *stream) {
    if (!d_pred || !d_truth || !d_work || !d_cells || !d_sums || ((uintptr_t)d_work & 15) || ((uintptr_t)d_sums & 7) || X < 1 || Y < 1 || P < 1 ||
        P > 65535 || n_class < 2 || n_class > MAXC) {
        set_error("score_planes: bad argument (n_class 2..16, 1 <= P <= 65535, d_work 16-byte and d_sums 8-byte aligned)");
        return UKBB_EINVAL;
    }
    if (!score_shape_ok(X, Y, P, n_class)) {
        set_error("score_planes: a %d x %d plane does not fit the bit planes in LDS (X, Y <= %d and ceil(X/32)*Y <= %d words: 512 x 512)", X, Y,
                  SCORE_MAX_EDGE, SCORE_MAX_WORDS);
        return UKBB_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    const size_t n_cell = (size_t)P * n_class;
    if (hipMemsetAsync(d_cells, 0, n_cell * 8 * sizeof(int32_t), s) != hipSuccess || hipMemsetAsync(d_sums, 0, n_cell * 2 * sizeof(double), s) != hipSuccess) {
        set_error("score_planes: memset failed");
        return UKBB_EDEVICE;
    }
    const int lds = 3 * ((X + 31) / 32) * Y * (int)sizeof(unsigned);
    const hipError_t e = launch_lds<score_planes_kernel, 3 * SCORE_MAX_WORDS * (int)sizeof(unsigned)>(
        dim3((unsigned)score_grid(X, Y, P, n_class)), dim3(SCORE_THREADS), lds, s, d_pred, d_truth, X, Y, P, n_class,
        static_cast<unsigned char *>(d_work), d_cells, d_sums);
    if (e != hipSuccess) { set_error("score_planes: launch failed: %s", hipGetErrorString(e)); return UKBB_EDEVICE; }
    return UKBB_OK;
}

}  // extern "C"
