// How sure was the network: per (frame, class) reductions of the softmax the forward leaves in HBM, over the image region of the padded
// batch.  ukbb_cardiac_amd/confidence.py states the semantics (cells_host is the specification):
//
//   q(p)     = (int)(p * 65536.0f) of a float32 probability: the multiply by a power of two is exact, the conversion truncates, so
//              0 <= q <= 65536; a denormal p gives 0 whether or not the multiply flushes it, and so does a NaN (a cine frame no window
//              reaches)
//   per voxel with label c = pred:  q1 = q(p[c]),  q2 = max over c' != c of q(p[c']),  margin = q1 - q2
//   cell[t][c][20] (uint64):  0 n = voxels of frame t with pred == c | 1 sum q1 | 2 sum margin | 3..18 histogram of min(q1 >> 12, 15) |
//                             19 sum of q(p[c]) over ALL voxels of the frame (the "soft count")
//
// A streaming kernel: 4*n_class + 4 bytes read per voxel, nothing written but the cells.  One workgroup takes CONF_ITER * 256 consecutive
// image voxels (y fastest, as the batch stores them) of ONE slice, so all it counts belongs to one frame.  A voxel's probabilities come in
// with the widest loads their 4*n_class-byte pitch keeps aligned (16 bytes when n_class is a multiple of 4, 8 when it is even, else 4).
// Counters are private three times over before they reach HBM:
//   registers   n, sum q1, sum margin and the soft count of every class (the class loop is unrolled: no indexed registers), uint32 --
//               CONF_ITER * 65536 per thread at most
//   lanes       the histogram goes to LDS voxel by voxel, into one of CONF_COPIES copies chosen by the lane: the voxels of a wave mostly
//               share one (class, bin) -- the background, the inside of a structure -- and LDS atomics on one address take their
//               turns, so a single copy ran the kernel at the LDS's pace, not HBM's; with 32 copies at most two lanes meet
//   wave        one butterfly reduction per register counter at the end
//   workgroup   a [n_class][20] uint32 table in LDS (CONF_ITER * 256 * 65536 = 2^28 at most); its non-zero entries, a handful for a
//               typical workgroup, are the only global atomics
// Integer adds only (the margin sum is carried signed and added in two's complement, as the twin's int64 sum): nothing depends on
// arrival order.  The one float operation is the exact multiply.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/ukbb_fcn.h"
#include "kernels.h"

namespace ukbb {

namespace {

constexpr int CONF_MAXC = 16;                           // classes per call (as ukbb_fcn_unpack_labels)
constexpr int CONF_FIELDS = 20;
constexpr int CONF_THREADS = 256;
constexpr int CONF_ITER = 16;                           // voxels per thread
constexpr int CONF_COPIES = 32;                         // lane-private copies of the histogram (n_class * 16 * 32 uint32: 32 KB at 16 classes)

__device__ __forceinline__ int conf_q(float p) {
    const float x = p * 65536.0f;
    return x == x ? (int)x : 0;
}

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (unsigned)__shfl_xor((int)v, d, 64);
    return v;
}

// the NC probabilities of the voxel at p (4*NC-byte pitch from a 16-byte aligned base)
template <int NC>
__device__ __forceinline__ void load_probs(const float *__restrict__ p, float (&v)[NC]) {
    if constexpr (NC % 4 == 0) {
#pragma unroll
        for (int j = 0; j < NC / 4; ++j) {
            const float4 f = reinterpret_cast<const float4 *>(p)[j];
            v[4 * j] = f.x; v[4 * j + 1] = f.y; v[4 * j + 2] = f.z; v[4 * j + 3] = f.w;
        }
    } else if constexpr (NC % 2 == 0) {
#pragma unroll
        for (int j = 0; j < NC / 2; ++j) {
            const float2 f = reinterpret_cast<const float2 *>(p)[j];
            v[2 * j] = f.x; v[2 * j + 1] = f.y;
        }
    } else {
#pragma unroll
        for (int j = 0; j < NC; ++j) v[j] = p[j];
    }
}

template <int NC>
__global__ __launch_bounds__(CONF_THREADS) void confidence_cells_kernel(const float *__restrict__ prob, const int *__restrict__ pred, int X, int Y,
                                                                        int Z, int X2, int Y2, int x_pre, int y_pre, int first_slice,
                                                                        unsigned long long *cells) {
    __shared__ unsigned table[NC * CONF_FIELDS];
    __shared__ unsigned hist[NC * 16 * CONF_COPIES];        // [class][bin][copy]: a wave's lanes spread over the banks
    const int tid = threadIdx.x, lane = tid & 63, copy = tid & (CONF_COPIES - 1);
    for (int i = tid; i < NC * CONF_FIELDS; i += CONF_THREADS) table[i] = 0;
    for (int i = tid; i < NC * 16 * CONF_COPIES; i += CONF_THREADS) hist[i] = 0;
    __syncthreads();
    const int b = blockIdx.y;                           // slice of this launch's batch
    const int t = (first_slice + b) / Z;                // its frame in the whole T*Z batch
    const int n_vox = X * Y;
    const int base = blockIdx.x * (CONF_ITER * CONF_THREADS);
    const size_t plane = (size_t)b * X2 * Y2;

    unsigned cnt[NC], s1[NC], soft[NC];
    int sm[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) { cnt[c] = 0; s1[c] = 0; soft[c] = 0; sm[c] = 0; }

    // (x, y) of voxel i = x*Y + y, stepped by 256 voxels per round: one division per thread, none per voxel
    const int step_x = CONF_THREADS / Y, step_y = CONF_THREADS - step_x * Y;
    int x = (base + tid) / Y, y = (base + tid) - x * Y;
#pragma unroll 4
    for (int it = 0; it < CONF_ITER; ++it, x += step_x, y += step_y) {
        if (y >= Y) { y -= Y; ++x; }
        const int i = base + it * CONF_THREADS + tid;
        if (i < n_vox) {
            const size_t at = plane + (size_t)(x + x_pre) * Y2 + (y + y_pre);
            const int lab = pred[at];
            float p[NC];
            load_probs<NC>(prob + at * NC, p);
            int q1 = 0, q2 = 0;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const int q = conf_q(p[c]);
                soft[c] += (unsigned)q;
                if (c == lab) q1 = q;
                else q2 = q > q2 ? q : q2;
            }
            const int margin = q1 - q2;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const bool is = c == lab;
                cnt[c] += is ? 1u : 0u;
                s1[c] += is ? (unsigned)q1 : 0u;
                sm[c] += is ? margin : 0;
            }
            if (lab >= 0 && lab < NC) {                 // a label outside the model's classes has no cell
                const int bin = q1 >> 12;
                atomicAdd(&hist[(lab * 16 + (bin < 15 ? bin : 15)) * CONF_COPIES + copy], 1u);
            }
        }
    }

#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const unsigned a = wave_sum(cnt[c]), s = wave_sum(s1[c]), m = wave_sum((unsigned)sm[c]), f = wave_sum(soft[c]);
        if (lane == 0) {
            if (a) atomicAdd(&table[c * CONF_FIELDS + 0], a);
            if (s) atomicAdd(&table[c * CONF_FIELDS + 1], s);
            if (m) atomicAdd(&table[c * CONF_FIELDS + 2], m);
            if (f) atomicAdd(&table[c * CONF_FIELDS + 19], f);
        }
    }
    __syncthreads();
    for (int i = tid; i < NC * 16 * CONF_COPIES; i += CONF_THREADS) {   // the copies of a bin into the table: few are non-zero
        const unsigned v = hist[i];
        if (v) { const int k = i / CONF_COPIES; atomicAdd(&table[(k >> 4) * CONF_FIELDS + 3 + (k & 15)], v); }
    }
    __syncthreads();
    for (int i = tid; i < NC * CONF_FIELDS; i += CONF_THREADS) {
        const unsigned v = table[i];
        if (!v) continue;
        const int c = i / CONF_FIELDS, f = i - c * CONF_FIELDS;
        // the margin sum is signed (pred is the argmax of the engine's probabilities, so it is >= 0 there): sign-extended, it adds as the
        // twin's int64 sum does
        const unsigned long long w = f == 2 ? (unsigned long long)(long long)(int)v : (unsigned long long)v;
        atomicAdd(&cells[((size_t)t * NC + c) * CONF_FIELDS + f], w);
    }
}

template <int NC>
hipError_t launch_confidence(dim3 grid, hipStream_t s, const float *prob, const int *pred, int X, int Y, int Z, int X2, int Y2, int x_pre, int y_pre,
                             int first_slice, unsigned long long *cells) {
    hipLaunchKernelGGL(confidence_cells_kernel<NC>, grid, dim3(CONF_THREADS), 0, s, prob, pred, X, Y, Z, X2, Y2, x_pre, y_pre, first_slice, cells);
    return hipGetLastError();
}

}  // namespace
}  // namespace ukbb

using namespace ukbb;

extern "C" {

int ukbb_fcn_confidence_cells(const float *d_prob, const int32_t *d_pred, int n, int X, int Y, int Z, int T, int X2, int Y2, int x_pre, int y_pre,
                              int n_class, int first_slice, uint64_t *d_cells, void *stream) {
    if (!d_prob || !d_pred || !d_cells || ((uintptr_t)d_prob & 15) || ((uintptr_t)d_pred & 3) || ((uintptr_t)d_cells & 7) || n < 1 || X < 1 || Y < 1 ||
        Z < 1 || T < 1 || x_pre < 0 || y_pre < 0 || X2 < X + x_pre || Y2 < Y + y_pre || n_class < 2 || n_class > CONF_MAXC ||
        (long long)Z * T > 65535 || (long long)X * Y > (1ll << 30)) {
        set_error("confidence_cells: bad argument (n_class 2..16, Z*T <= 65535, X*Y <= 2^30, d_prob 16-byte and d_cells 8-byte aligned)");
        return UKBB_EINVAL;
    }
    if (first_slice < 0 || (long long)first_slice + n > (long long)Z * T) {
        set_error("confidence_cells: slices %d .. %lld lie outside the batch of Z*T = %d x %d slices", first_slice, (long long)first_slice + n - 1, Z, T);
        return UKBB_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    const int per_wg = CONF_ITER * CONF_THREADS;
    const dim3 grid((unsigned)(((long long)X * Y + per_wg - 1) / per_wg), (unsigned)n);
    unsigned long long *cells = reinterpret_cast<unsigned long long *>(d_cells);
    hipError_t e = hipErrorInvalidValue;
    switch (n_class) {
#define UKBB_CONF_CASE(NC) case NC: e = launch_confidence<NC>(grid, s, d_prob, d_pred, X, Y, Z, X2, Y2, x_pre, y_pre, first_slice, cells); break;
        UKBB_CONF_CASE(2) UKBB_CONF_CASE(3) UKBB_CONF_CASE(4) UKBB_CONF_CASE(5) UKBB_CONF_CASE(6) UKBB_CONF_CASE(7) UKBB_CONF_CASE(8)
        UKBB_CONF_CASE(9) UKBB_CONF_CASE(10) UKBB_CONF_CASE(11) UKBB_CONF_CASE(12) UKBB_CONF_CASE(13) UKBB_CONF_CASE(14) UKBB_CONF_CASE(15)
        UKBB_CONF_CASE(16)
#undef UKBB_CONF_CASE
    }
    if (e != hipSuccess) { set_error("confidence_cells: launch failed: %s", hipGetErrorString(e)); return UKBB_EDEVICE; }
    return UKBB_OK;
}

}  // extern "C"
