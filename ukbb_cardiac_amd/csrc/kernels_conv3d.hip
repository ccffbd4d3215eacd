// 3-D convolutions of the aortic Temporal-UNet (reference common/network_ao.py:67-114, common/network.py:37-52
// conv3d_bn_relu / conv3d_transpose_bn_relu) in inference mode, fp32.
//
// A batch holds windows of T consecutive frames: image n = window * T + t.  Time stride is always 1 and the TF 'SAME'
// pad along time is one zero frame at each WINDOW edge, so a 3x3x3 conv is a 3x3 conv whose K loop also runs over the
// three time taps dt = -1, 0, +1 -- and a tap whose frame t + dt falls outside [0, T) is skipped for the whole K chunk
// (no load, no MFMA; it would only multiply zeros).
//
//   conv3d_kernel        3x3x3 conv + folded BN + ReLU, spatial stride 1 or 2, one or two sources (skip concat), and the
//                        3x3x3 transposed conv with spatial stride 2 as its 4 sub-pixel phases (blockIdx.y = phase): output
//                        pixel (2y + py, 2x + px) sums the kernel rows ky = py + 2j over input rows y - j, the same for x,
//                        and along time out[t] = sum_kt in[t + 1 - kt] W[kt] (the packing puts W[2 - (dt + 1)] at dt).
//                        Implicit GEMM on v_mfma_f32_32x32x2_f32: A = weights (32 output channels), B = pixels (32 of one
//                        frame, flattened), K = time taps x spatial taps x channels in chunks of 8.  Lane (col, h) loads ONE
//                        float4 of channels c + 4h .. c + 4h + 3 of its pixel per chunk and supplies element s as k = h of
//                        k-step s, so k-step s covers channels {c + s, c + 4 + s}; the weights are packed in that order as one
//                        float4 per lane (pack_conv3d_weights).  The accumulator holds 4 consecutive output channels of one
//                        pixel per register group: NHWC float4 stores.  Each tap's channel sum runs in an accumulator of its
//                        own and is then added to the total in tap order: 27 chains of C_in terms instead of one of 27 C_in keep
//                        the fp32 rounding of the deep layers (C_in 256-512) near that of the 2-D convs.
//   conv3d_first_kernel  the first layer (C_in = 1, 27 taps) on the vector ALU, its input gathered from the cine through a
//                        window -> frame table (a window's frames are never copied out of the cine).
//   t3d_tile_kernel      the weighted circular tiling of deploy_network_ao.py:176-183 for a chunk of windows, in the
//                        reference's order and arithmetic (float32 accumulator updated through float64), as
//                        kernels_lstm.hip lstm_tile_kernel does; prob /= weight and argmax behind the last chunk.
#include "kernels.h"
#include "device_prims.h"

namespace ukbb {

namespace {

template <int CB>
__global__ __launch_bounds__(256) void conv3d_kernel(const Conv3dArgs a) {
    const int lane = threadIdx.x & 63, col = lane & 31, h = lane >> 5;
    const Conv3dPhase &P = a.ph[blockIdx.y];
    const int npix = a.Hg * a.Wg, ptiles = (npix + 31) / 32, ncob = a.Cout_pad / 32, cgroups = ncob / CB;
    const long long item = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= (long long)a.N * ptiles * cgroups) return;                      // whole wave
    const int cg = (int)(item % cgroups);
    const long long r = item / cgroups;
    const int pt = (int)(r % ptiles), n = (int)(r / ptiles);
    const int t = n % a.T;
    const int p = pt * 32 + col;
    const bool pv = p < npix;
    const int gy = pv ? p / a.Wg : 0, gx = pv ? p - gy * a.Wg : 0;
    const int nch0 = a.C0 / 8, nch = nch0 + a.C1 / 8;
    f32x16 acc[CB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[cb][i] = 0.f;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int dti = 0; dti < 3; ++dti) {
        const int tt = t + dti - 1;
        if (tt < 0 || tt >= a.T) continue;                                       // window edge: TF SAME zero frame, skipped
        const size_t ni = (size_t)(n + dti - 1);
        for (int jy = 0; jy < P.ny; ++jy) {
            const int iy = gy * a.stride + a.oy + jy * a.jstep;
            for (int jx = 0; jx < P.nx; ++jx) {
                const int ix = gx * a.stride + a.ox + jx * a.jstep;
                const bool ok = pv && iy >= 0 && iy < a.Hi && ix >= 0 && ix < a.Wi;
                const size_t pix = (ni * a.Hi + (ok ? iy : 0)) * a.Wi + (ok ? ix : 0);
                const int tap = (dti * P.ny + jy) * P.nx + jx;
                const f32x4 *wp = reinterpret_cast<const f32x4 *>(P.wpk) + ((size_t)tap * nch * ncob + (size_t)cg * CB) * 64 + lane;
                const float *src = a.in0 + pix * a.C0 + 4 * h;
                f32x16 part[CB];                                         // this tap's channel sum, added to the total below
#pragma unroll
                for (int cb = 0; cb < CB; ++cb)
#pragma unroll
                    for (int i = 0; i < 16; ++i) part[cb][i] = 0.f;
                for (int c = 0; c < nch; ++c) {
                    if (c == nch0) src = a.in1 + pix * a.C1 + 4 * h;
                    const int cc = c < nch0 ? c : c - nch0;
                    const f32x4 b = ok ? *reinterpret_cast<const f32x4 *>(src + 8 * cc) : zero;
                    f32x4 w[CB];
#pragma unroll
                    for (int cb = 0; cb < CB; ++cb) w[cb] = wp[((size_t)c * ncob + cb) * 64];
#pragma unroll
                    for (int s = 0; s < 4; ++s)
#pragma unroll
                        for (int cb = 0; cb < CB; ++cb) part[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[cb][s], b[s], part[cb], 0, 0, 0);
                }
#pragma unroll
                for (int cb = 0; cb < CB; ++cb) acc[cb] += part[cb];
            }
        }
    }
    if (!pv) return;
    const int oy = gy * a.up + P.py, ox = gx * a.up + P.px;
    float *o = a.out + (((size_t)n * a.Ho + oy) * a.Wo + ox) * a.Cout;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int co = (cg * CB + cb) * 32 + 8 * j + 4 * h;
            if (co >= a.Cout) continue;
            const f32x4 bi = *reinterpret_cast<const f32x4 *>(a.bias + co);
            f32x4 v;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                v[i] = acc[cb][4 * j + i] + bi[i];
                if (a.relu) v[i] = fmaxf(v[i], 0.f);
            }
            *reinterpret_cast<f32x4 *>(o + co) = v;
        }
    }
}

// one thread = one output pixel of one image, 16 output channels; taps in (dt, ky, kx) order, fp32 fma chain per channel
constexpr int FIRST_COUT = 16;

__global__ __launch_bounds__(256) void conv3d_first_kernel(const Conv3dFirstArgs a) {
    __shared__ float ws[27 * FIRST_COUT + FIRST_COUT];
    for (int i = threadIdx.x; i < 27 * FIRST_COUT; i += 256) ws[i] = a.w[i];
    if (threadIdx.x < FIRST_COUT) ws[27 * FIRST_COUT + threadIdx.x] = a.bias[threadIdx.x];
    __syncthreads();
    const long long HW = (long long)a.H * a.W, total = (long long)a.N * HW;
    for (long long id = (long long)blockIdx.x * 256 + threadIdx.x; id < total; id += (long long)gridDim.x * 256) {
        const int n = (int)(id / HW);
        const int q = (int)(id - (long long)n * HW), y = q / a.W, x = q - y * a.W;
        const int t = n % a.T;
        float acc[FIRST_COUT];
#pragma unroll
        for (int c = 0; c < FIRST_COUT; ++c) acc[c] = 0.f;
        for (int dti = 0; dti < 3; ++dti) {
            const int tt = t + dti - 1;
            if (tt < 0 || tt >= a.T) continue;
            const int ni = n + dti - 1;
            const long long f = a.map ? a.map[ni] : ni;
            const float *img = a.image + f * HW;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int iy = y + ky - 1;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int ix = x + kx - 1;
                    const float v = (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) ? img[(long long)iy * a.W + ix] : 0.f;
                    const float *w = ws + ((dti * 3 + ky) * 3 + kx) * FIRST_COUT;
#pragma unroll
                    for (int c = 0; c < FIRST_COUT; ++c) acc[c] = fmaf(v, w[c], acc[c]);
                }
            }
        }
        float *o = a.out + id * FIRST_COUT;
#pragma unroll
        for (int j = 0; j < FIRST_COUT / 4; ++j) {
            f32x4 v;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = fmaxf(acc[4 * j + i] + ws[27 * FIRST_COUT + 4 * j + i], 0.f);
            *reinterpret_cast<f32x4 *>(o + 4 * j) = v;
        }
    }
}

// a term of the tiling (kernels.h cine_tile_pixel) is the stored softmax of a window frame
template <int NCLS>
__global__ __launch_bounds__(256) void t3d_tile_kernel(const T3dTileArgs a) {
    const long long total = (long long)a.tb.F * a.HW;
    for (long long id = (long long)blockIdx.x * 256 + threadIdx.x; id < total; id += (long long)gridDim.x * 256) {
        const int f = (int)(id / a.HW);
        const long long pix = id - (long long)f * a.HW;
        cine_tile_pixel<NCLS, true>(a.tb, f, a.w0, a.w1, a.first, a.last, a.prob, a.pred, id, [&](int wi, int k, float (&p)[NCLS]) {
            const float *src = a.probw + (((long long)(wi - a.w0) * a.tb.K + k) * a.HW + pix) * NCLS;
#pragma unroll
            for (int c = 0; c < NCLS; ++c) p[c] = src[c];
        });
    }
}

}  // namespace

hipError_t launch_conv3d(const Conv3dArgs &a, hipStream_t s) {
    if (a.C0 % 8 || a.C1 % 8 || a.Cout % 16 || a.Cout_pad % 32 || a.Cout > a.Cout_pad || a.nph < 1 || a.nph > 4 || a.T < 1)
        return hipErrorInvalidValue;
    const int cb = a.Cout_pad % 64 == 0 ? 2 : 1;
    const long long items = (long long)a.N * ((a.Hg * a.Wg + 31) / 32) * (a.Cout_pad / 32 / cb);
    const long long blocks = (items + 3) / 4;
    if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
    const dim3 g((unsigned)blocks, (unsigned)a.nph), t(256);
    if (cb == 2) hipLaunchKernelGGL((conv3d_kernel<2>), g, t, 0, s, a);
    else hipLaunchKernelGGL((conv3d_kernel<1>), g, t, 0, s, a);
    return hipGetLastError();
}

hipError_t launch_conv3d_first(const Conv3dFirstArgs &a, hipStream_t s) {
    const long long total = (long long)a.N * a.H * a.W;
    long long blocks = (total + 255) / 256;
    if (blocks > 256 * 64) blocks = 256 * 64;
    hipLaunchKernelGGL(conv3d_first_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_t3d_tile(const T3dTileArgs &a, hipStream_t s) {
    const long long total = (long long)a.tb.F * a.HW;
    long long blocks = (total + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    const dim3 g((unsigned)blocks), t(256);
    const bool ok = with_classes(a.C, [&](auto nc) { hipLaunchKernelGGL((t3d_tile_kernel<decltype(nc)::value>), g, t, 0, s, a); });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace ukbb
