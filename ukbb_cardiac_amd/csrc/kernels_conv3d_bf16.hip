// 3-D convolutions of the aortic Temporal-UNet under UKBB_PREC_BF16_3D: bf16 maps in HBM, v_mfma_f32_32x32x16_bf16, fp32 accumulation.
// The fp32 kernels of kernels_conv3d.hip are untouched; window semantics are theirs: image n = window * T + t, a time tap whose frame
// t + dt falls outside [0, T) of ITS OWN window is skipped (never read from the neighbouring window), the transposed conv reads
// in[t + 1 - kt] (the packing puts W[2 - (dt + 1)] at dt) and runs as its 4 sub-pixel phases (blockIdx.y).
//
// Every map is bf16, channel-blocked [N][C/16][H*W][16] (kernels.h): lane (pixel, h) fetches channels 16 b + 8 h .. 16 b + 8 h + 7 of
// its pixel as ONE 16-byte load, which is the B fragment of one MFMA (k = 8 h + j); 32 consecutive pixels are one contiguous 1 KB wave
// load.  The stored input is read without any rounding.  The folded kernel is rounded once to bf16 (ties to even) and packed at create
// time into A fragments (pack_conv3d_weights_bf16), 16 bytes per lane and 16-channel K step.
//
//   conv3d_bf16_kernel        the item decomposition of conv3d_kernel: one wave = 32 pixels of one frame x CB 32-row channel blocks.  The
//                             channel sums of the 9 (or 4, 2, 1) spatial taps of ONE time tap run in an accumulator of their own, which
//                             is then added to the total in time-tap order: chains of 9 C_in terms, as in the 2-D bf16 kernels, not of
//                             27 C_in.  The accumulator holds 4 consecutive output channels of one pixel per register group: + bias,
//                             ReLU, ONE rounding to bf16, an 8-byte store into the pixel's 32-byte row of its 16-channel block.  Rows of
//                             the MFMA beyond C_out (C_out = 16: rows 16..31 multiply zeros) are not stored.
//   conv3d_first_bf16_kernel  the first layer (C_in = 1, 27 taps) on the vector ALU from the fp32 cine through the window -> frame
//                             table, with the UNROUNDED fp32 folded weights and conv3d_first_kernel's arithmetic (taps in (dt, ky, kx)
//                             order, one fma chain per channel); its 16 channels rounded once and stored as 32 bytes.  One thread per
//                             pixel, no grid cap: the kernel has no loop to wrap.
//
// Built with -mllvm -amdgpu-mfma-vgpr-form (Makefile, FLAGS_kernels_conv3d_bf16): the accumulators live in VGPRs.  In the AGPR form hipcc
// moved conv3d_bf16_kernel<1>'s per-time-tap accumulator AGPR -> VGPR -> AGPR around every spatial tap and read a15 too soon behind the
// loop's last MFMA: output channels 27 and 31 of every 32-channel block were stale (tests/test_temporal_bf16_launches_gpu.py caught it).
#include "kernels.h"
#include "device_prims.h"

namespace ukbb {

namespace {

typedef unsigned short bf16_t;      // a stored bf16 value

template <int CB>
__global__ __launch_bounds__(256) void conv3d_bf16_kernel(const Conv3dArgs a) {
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
    const int nk0 = a.C0 / 16, nk = nk0 + a.C1 / 16;
    const size_t HWi = (size_t)a.Hi * a.Wi;
    const bf16_t *in0 = reinterpret_cast<const bf16_t *>(a.in0), *in1 = reinterpret_cast<const bf16_t *>(a.in1);
    f32x16 acc[CB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[cb][i] = 0.f;
    const u32x4 zero = {0u, 0u, 0u, 0u};
    for (int dti = 0; dti < 3; ++dti) {
        const int tt = t + dti - 1;
        if (tt < 0 || tt >= a.T) continue;                                       // window edge: TF SAME zero frame, skipped
        const size_t ni = (size_t)(n + dti - 1);
        f32x16 part[CB];                                                         // this time tap's sum, added to the total below
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int i = 0; i < 16; ++i) part[cb][i] = 0.f;
        for (int jy = 0; jy < P.ny; ++jy) {
            const int iy = gy * a.stride + a.oy + jy * a.jstep;
            for (int jx = 0; jx < P.nx; ++jx) {
                const int ix = gx * a.stride + a.ox + jx * a.jstep;
                const bool ok = pv && iy >= 0 && iy < a.Hi && ix >= 0 && ix < a.Wi;
                const size_t pofs = ((size_t)(ok ? iy : 0) * a.Wi + (ok ? ix : 0)) * 16 + 8 * h;
                const int tap = (dti * P.ny + jy) * P.nx + jx;
                const u32x4 *wp = reinterpret_cast<const u32x4 *>(P.wpk) + ((size_t)tap * nk * ncob + (size_t)cg * CB) * 64 + lane;
                const bf16_t *src = in0 + ni * HWi * a.C0 + pofs;
                for (int c = 0; c < nk; ++c) {
                    if (c == nk0) src = in1 + ni * HWi * a.C1 + pofs;
                    const int cc = c < nk0 ? c : c - nk0;
                    const u32x4 b = ok ? *reinterpret_cast<const u32x4 *>(src + (size_t)cc * HWi * 16) : zero;
                    u32x4 w[CB];
#pragma unroll
                    for (int cb = 0; cb < CB; ++cb) w[cb] = wp[((size_t)c * ncob + cb) * 64];
#pragma unroll
                    for (int cb = 0; cb < CB; ++cb) part[cb] = mfma_bf16(w[cb], b, part[cb]);
                }
            }
        }
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) acc[cb] += part[cb];
    }
    if (!pv) return;
    const int oy = gy * a.up + P.py, ox = gx * a.up + P.px;
    const size_t HWo = (size_t)a.Ho * a.Wo;
    bf16_t *o = reinterpret_cast<bf16_t *>(a.out) + (size_t)n * HWo * a.Cout + ((size_t)oy * a.Wo + ox) * 16;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int co = (cg * CB + cb) * 32 + 8 * j + 4 * h;
            if (co >= a.Cout) continue;                                          // padded MFMA rows: nothing stored beyond C_out
            const f32x4 bi = *reinterpret_cast<const f32x4 *>(a.bias + co);
            float v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                v[i] = acc[cb][4 * j + i] + bi[i];
                if (a.relu) v[i] = fmaxf(v[i], 0.f);
            }
            const u32x2 pk = {pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
            *reinterpret_cast<u32x2 *>(o + (size_t)(co >> 4) * HWo * 16 + (co & 15)) = pk;
        }
    }
}

constexpr int FIRST_COUT = 16;

__global__ __launch_bounds__(256) void conv3d_first_bf16_kernel(const Conv3dFirstArgs a) {
    __shared__ float ws[27 * FIRST_COUT + FIRST_COUT];
    for (int i = threadIdx.x; i < 27 * FIRST_COUT; i += 256) ws[i] = a.w[i];
    if (threadIdx.x < FIRST_COUT) ws[27 * FIRST_COUT + threadIdx.x] = a.bias[threadIdx.x];
    __syncthreads();
    const long long HW = (long long)a.H * a.W, total = (long long)a.N * HW;
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= total) return;
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
    bf16_t *o = reinterpret_cast<bf16_t *>(a.out) + id * FIRST_COUT;
#pragma unroll
    for (int j = 0; j < FIRST_COUT / 8; ++j) {
        u32x4 pk;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            pk[i] = pack_bf16x2(fmaxf(acc[8 * j + 2 * i] + ws[27 * FIRST_COUT + 8 * j + 2 * i], 0.f),
                                fmaxf(acc[8 * j + 2 * i + 1] + ws[27 * FIRST_COUT + 8 * j + 2 * i + 1], 0.f));
        *reinterpret_cast<u32x4 *>(o + 8 * j) = pk;
    }
}

}  // namespace

hipError_t launch_conv3d_bf16(const Conv3dArgs &a, hipStream_t s) {
    if (a.C0 < 16 || a.C0 % 16 || a.C1 % 16 || (a.C1 && !a.in1) || a.Cout % 16 || a.Cout_pad % 32 || a.Cout > a.Cout_pad || a.nph < 1 || a.nph > 4 || a.T < 1)
        return hipErrorInvalidValue;
    const int cb = a.Cout_pad % 64 == 0 ? 2 : 1;
    const long long items = (long long)a.N * ((a.Hg * a.Wg + 31) / 32) * (a.Cout_pad / 32 / cb);
    const long long blocks = (items + 3) / 4;
    if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
    const dim3 g((unsigned)blocks, (unsigned)a.nph), t(256);
    if (cb == 2) hipLaunchKernelGGL((conv3d_bf16_kernel<2>), g, t, 0, s, a);
    else hipLaunchKernelGGL((conv3d_bf16_kernel<1>), g, t, 0, s, a);
    return hipGetLastError();
}

hipError_t launch_conv3d_first_bf16(const Conv3dFirstArgs &a, hipStream_t s) {
    const long long total = (long long)a.N * a.H * a.W;
    const long long blocks = (total + 255) / 256;
    if (blocks < 1 || blocks > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(conv3d_first_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace ukbb
