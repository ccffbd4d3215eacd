// Fused FCN head for gfx950.  Two kernels replace the full-resolution part of
// build_FCN (reference common/network.py:201-229) and the prob / pred definition
// (common/train_network.py:198-199):
//
//   same_dim_l   1x1 C_l -> 32, BN, ReLU                       (network.py:203-204)
//   up_l         transpose_upsample2d x2/x4/x8/x16             (network.py:138-167,210-211)
//   concat       -> 160 channels                               (network.py:218)
//   out0         1x1 160 -> 64, BN, ReLU ; out1 1x1 64 -> 64, BN, ReLU ; logits 1x1 64 -> n_class + bias
//   softmax, argmax
//
// Algebra used: out0's pre-activation is  W0 * concat_l(up_l(s_l)) = sum_l up_l(W0_l * s_l),
// because the bilinear "transposed conv" acts per channel and linearly, and a 1x1 conv acts
// per pixel and linearly, so they commute (borders included: both sides apply the same,
// possibly un-normalised, tap weights).  Levels 1..4 are therefore projected to 64
// channels at LOW resolution by sqg_kernel (G_l = W0_l * relu(BN(Ws_l * x_l))), and the
// full-resolution kernel only gathers the <= 2x2 taps of G_l and adds them.  This removes
// 128 of the 160 input channels of out0 at full resolution (-300 M of 603 M MAC per slice)
// and the 160-channel concat / the four upsampled maps are never materialised.
//
// Common mapping: one wave owns 32 pixels; the pixel sits on the MFMA N dimension
// (lane & 31), channels on M, so every 1x1 layer is D[cout][px] = W[cout][k] X[k][px] with
// v_mfma_f32_32x32x2_f32.  The 32x32 result has its column (pixel) on the lane and its rows
// (channels) in the 16 accumulator registers, so after bias + ReLU the registers ARE the next
// layer's B operand: k-step r supplies rows rowmap(r,0) on lanes 0-31 and rowmap(r,1) on
// lanes 32-63, and the weights are packed on the host in that k order.
#include "kernels.h"
#include "device_prims.h"
#include "pack.h"       // rowmap

#include <atomic>
#include <cstdio>

#include <cstdlib>
#include <type_traits>

namespace ukbb {

#define MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

// Accumulator tile pre-loaded with the bias of its 16 rows: acc[4j+i] = bias[8j + 4g + i].
// Used as the C operand of the first MFMA of a chain, so the bias add costs no VALU op.
__device__ __forceinline__ f32x16 bias_tile(const float *bias, int g) {
    f32x16 acc;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const f32x4 b = ld4(bias + 8 * j + 4 * g);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[4 * j + i] = b[i];
    }
    return acc;
}

__device__ __forceinline__ void relu16(f32x16 &acc) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = relu_bits(acc[r]);
}

// D0/D1 (two Cout blocks of 32) += W[64][32 rows of X] * X, X given as an accumulator tile.
// wp: packed [cb][q4][lane][4]
__device__ __forceinline__ void chain_32to64(const float *wp, int lane, const f32x16 &X, f32x16 &D0, f32x16 &D1) {
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
        const f32x4 wa = ld4(wp + ((0 * 4 + q4) * 64 + lane) * 4);
        const f32x4 wb = ld4(wp + ((1 * 4 + q4) * 64 + lane) * 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            D0 = MFMA32(wa[i], X[4 * q4 + i], D0);
            D1 = MFMA32(wb[i], X[4 * q4 + i], D1);
        }
    }
}

// D (one Cout block of 32) += W[32 couts][32 rows of X] * X.  wp: packed [q4][lane][4] of that block.
__device__ __forceinline__ void chain_32to32(const float *wp, int lane, const f32x16 &X, f32x16 &D) {
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
        const f32x4 w = ld4(wp + (q4 * 64 + lane) * 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) D = MFMA32(w[i], X[4 * q4 + i], D);
    }
}

// ---- bf16 channel-blocked inputs (UKBB_PREC_BF16_STORE: SqgArgs::x_bf16, HeadArgs::conv0_bf16) ------------------------------------
// A pixel's 16-channel block is 32 bytes, and the two lanes that hold a pixel (p, g = 0 | 1) fetch it as ONE unit: lane g loads the 16 bytes
// of channels 8 g .. 8 g + 7, so a wave's 32 consecutive pixels are one contiguous 1-KB load.  The fp32 k order (pack_sq) wants channels
// 4 g .. 4 g + 3 (k-group 2 c) and 8 + 4 g .. 8 + 4 g + 3 (k-group 2 c + 1) of chunk c on lane g, so the halves exchange one 8-byte piece
// with v_permlane32_swap a, b (a's upper 32 lanes <-> b's lower 32 lanes) and widen: bf16 -> fp32 is a shift / a mask, exact.  What the
// MFMAs behind it see is, value for value and in the same order, what the fp32 launch sees for a map that holds the same numbers.
// Every lane of the wave must be active (the callers clamp the address of a pixel past the map instead of masking the lane).
__device__ __forceinline__ void bf16_block_to_k(const u32x4 &d, f32x4 &x0, f32x4 &x1) {
    const auto s0 = __builtin_amdgcn_permlane32_swap(d[0], d[2], false, false);
    const auto s1 = __builtin_amdgcn_permlane32_swap(d[1], d[3], false, false);
    x0 = f32x4{__builtin_bit_cast(float, s0[0] << 16), __builtin_bit_cast(float, s0[0] & 0xffff0000u),
               __builtin_bit_cast(float, s1[0] << 16), __builtin_bit_cast(float, s1[0] & 0xffff0000u)};
    x1 = f32x4{__builtin_bit_cast(float, s0[1] << 16), __builtin_bit_cast(float, s0[1] & 0xffff0000u),
               __builtin_bit_cast(float, s1[1] << 16), __builtin_bit_cast(float, s1[1] & 0xffff0000u)};
}
__device__ __forceinline__ u32x4 ld_block_half(const char *p) { return *reinterpret_cast<const u32x4 *>(p); }
// lane (pixel q of the flattened [N * hw] map, half g): address of its half of chunk 0's block; chunk c lies c * hw * 32 bytes further
__device__ __forceinline__ const char *bf16_block_addr(const SqgArgs &a, long long q, int nchunk, int g) {
    const unsigned n = (unsigned)q / (unsigned)a.hw, pix = (unsigned)q - n * (unsigned)a.hw;      // q < 2^31 (engine.cpp check_shape)
    return reinterpret_cast<const char *>(a.x) + ((size_t)n * nchunk * a.hw + pix) * 32 + 16 * g;
}

// ---------------------------------------------------------------------------
// sqg_kernel: G[px][64] = W0_l (64x32) * relu(Ws (32xCIN) * x[px] + bs)   at low resolution.
// One wave per 32 consecutive pixels of the flattened [N*H_l*W_l] map; no LDS.
// BF: x is bf16, channel-blocked (SqgArgs::x_bf16).
// ---------------------------------------------------------------------------
template <int CIN, bool BF = false>
__device__ __forceinline__ void sqg_body(const SqgArgs &a, int vblock, int vgrid) {
    const int lane = threadIdx.x & 63;
    const int p = lane & 31, g = lane >> 5;
    const long long nblk = (a.npix + 31) >> 5;
    for (long long blk = (long long)vblock * 4 + (threadIdx.x >> 6); blk < nblk; blk += (long long)vgrid * 4) {
        const long long q = blk * 32 + p;
        const bool valid = q < a.npix;
        f32x16 S = bias_tile(a.b_s, g);
        // k-step (j,i) pairs channels 8j+i (lanes 0-31) and 8j+4+i (lanes 32-63).
        // Levels 3-4 are small (1-2 blocks per wave): all of the block's feature loads are issued before
        // the first MFMA so their latency is paid once, not once per group of k-steps.
        // (at most 128 channels at a time: inside sqg_multi_kernel this body must not push the register count past the
        // two-waves-per-SIMD limit, or level 1's bandwidth-bound stream loses half of its loads in flight)
        constexpr int XG = CIN / 8 < 16 ? CIN / 8 : 16;
        if constexpr (BF) {                             // the same k-steps in the same order, two k-groups per 32-byte block
            const char *xb = bf16_block_addr(a, valid ? q : a.npix - 1, CIN / 16, g);
            const size_t cstride = (size_t)a.hw * 32;
#pragma unroll
            for (int j0 = 0; j0 < CIN / 8; j0 += XG) {
                u32x4 xr[XG / 2];
#pragma unroll
                for (int c = 0; c < XG / 2; ++c) xr[c] = ld_block_half(xb + (j0 / 2 + c) * cstride);
#pragma unroll
                for (int c = 0; c < XG / 2; ++c) {
                    f32x4 xk[2];
                    bf16_block_to_k(xr[c], xk[0], xk[1]);
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const f32x4 wv = ld4(a.w_s + ((j0 + 2 * c + h) * 64 + lane) * 4);
#pragma unroll
                        for (int i = 0; i < 4; ++i) S = MFMA32(wv[i], xk[h][i], S);
                    }
                }
            }
        } else {
        const float *xp = a.x + (valid ? q : a.npix - 1) * CIN + 4 * g;
#pragma unroll
        for (int j0 = 0; j0 < CIN / 8; j0 += XG) {
            f32x4 xv[XG];
#pragma unroll
            for (int j = 0; j < XG; ++j) xv[j] = ld4(xp + 8 * (j0 + j));
#pragma unroll
            for (int j = 0; j < XG; ++j) {
                const f32x4 wv = ld4(a.w_s + ((j0 + j) * 64 + lane) * 4);
#pragma unroll
                for (int i = 0; i < 4; ++i) S = MFMA32(wv[i], xv[j][i], S);
            }
        }
        }
        relu16(S);
        f32x16 G0, G1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { G0[r] = 0.f; G1[r] = 0.f; }
        chain_32to64(a.w_g, lane, S, G0, G1);
        if (valid) {
            float *o = a.out + q * 64 + 4 * g;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                f32x4 v0, v1;
#pragma unroll
                for (int i = 0; i < 4; ++i) { v0[i] = G0[4 * j + i]; v1[i] = G1[4 * j + i]; }
                *reinterpret_cast<f32x4 *>(o + 8 * j) = v0;
                *reinterpret_cast<f32x4 *>(o + 32 + 8 * j) = v1;
            }
        }
    }
}

// Levels 1 and 2 (C_in = 32, 64) are big enough to be bandwidth-bound (level 1 of the batch-64
// workload: 82 MB in, 164 MB out against 27 us of MFMA time), so this variant keeps both weight
// matrices and the bias tile in registers and requests the features of the wave's next 32-pixel
// block before it starts the MFMA chains of the current one: loads, MFMAs and stores of different
// blocks overlap inside a wave instead of relying on occupancy alone.
template <int CIN, bool BF = false>
__global__ __launch_bounds__(256) void sqg_kernel(const SqgArgs a) { sqg_body<CIN, BF>(a, blockIdx.x, gridDim.x); }

// TR: the last layer is computed transposed (G^T = S^T W0^T: the same registers with the MFMA operands swapped), which puts
// the 32 output channels of a block on the lanes and the pixels on the registers: every store instruction then writes two
// contiguous 128-byte segments (one accumulator register as it stands) instead of 32 segments of 32 bytes.
// LT: the features of a block (32 pixels x CIN floats, one contiguous chunk of the NHWC map) are fetched with fully contiguous
// 1-KB wave loads and turned into the operand layout (pixel on the lane) through a wave-private LDS tile, instead of loads
// that touch 32 rows with 32 bytes each.
// BF: x is bf16, channel-blocked (SqgArgs::x_bf16).  A block's 32 pixels x one 16-channel chunk are 1 KB contiguous and each lane pair loads a
// pixel's 32 bytes, so the loads are whole-line as they stand and LT is not used; a block in flight is NJ / 2 registers of 16 bytes.
constexpr int SQG_LDS_WAVE = 32 * (64 + 4);
template <int CIN, bool TR = false, bool LT = false, bool BF = false>
__device__ __forceinline__ void sqg_stream_body(const SqgArgs &a, int vblock, int vgrid, float *lds_x = nullptr) {
    constexpr int NJ = CIN / 8;
    const int lane = threadIdx.x & 63;
    const int p = lane & 31, g = lane >> 5;
    const long long nblk = (a.npix + 31) >> 5;
    const long long step = (long long)vgrid * 4;
    f32x4 ws[NJ], wa[4], wb[4];
#pragma unroll
    for (int j = 0; j < NJ; ++j) ws[j] = ld4(a.w_s + (j * 64 + lane) * 4);
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
        wa[q4] = ld4(a.w_g + ((0 * 4 + q4) * 64 + lane) * 4);
        wb[q4] = ld4(a.w_g + ((1 * 4 + q4) * 64 + lane) * 4);
    }
    const f32x16 bias = bias_tile(a.b_s, g);
    constexpr int RS = CIN + 4;                         // LDS row stride (floats): b128-aligned, the strided read is conflict-free
    float *const xl = LT ? lds_x + (threadIdx.x >> 6) * SQG_LDS_WAVE : nullptr;
    const long long qlast = a.npix * (CIN / 4) - 1;     // last valid 16-byte quad of the map (rows past the end are never stored)
    static_assert(!(LT && BF), "the LDS transpose serves the fp32 NHWC map only");
    constexpr int NX = BF ? NJ / 2 : NJ;                // 16-byte registers of a block in flight
    auto fetch = [&](long long blk, f32x4 *dst) {
        if constexpr (BF) {
            const long long q = blk * 32 + p;
            const char *xb = bf16_block_addr(a, q < a.npix ? q : a.npix - 1, CIN / 16, g);
            const size_t cstride = (size_t)a.hw * 32;
#pragma unroll
            for (int c = 0; c < NX; ++c) dst[c] = __builtin_bit_cast(f32x4, ld_block_half(xb + c * cstride));
        } else if constexpr (LT) {
#pragma unroll
            for (int t = 0; t < NJ; ++t) {
                const long long f = blk * (32 * (CIN / 4)) + t * 64 + lane;
                dst[t] = ld4(a.x + 4 * (f < qlast ? f : qlast));
            }
        } else {
            const long long q = blk * 32 + p;
            const float *xp = a.x + (q < a.npix ? q : a.npix - 1) * CIN + 4 * g;
#pragma unroll
            for (int j = 0; j < NJ; ++j) dst[j] = ld4(xp + 8 * j);
        }
    };
    long long blk = (long long)vblock * 4 + (threadIdx.x >> 6);
    f32x4 xn[NX];
    if (blk < nblk) fetch(blk, xn);
    for (; blk < nblk; blk += step) {
        f32x4 xv[NJ];
        if constexpr (BF) {
#pragma unroll
            for (int c = 0; c < NX; ++c) bf16_block_to_k(__builtin_bit_cast(u32x4, xn[c]), xv[2 * c], xv[2 * c + 1]);
        } else if constexpr (LT) {
#pragma unroll
            for (int t = 0; t < NJ; ++t) {
                const int f = t * 64 + lane;
                *reinterpret_cast<f32x4 *>(xl + (f / (CIN / 4)) * RS + (f % (CIN / 4)) * 4) = xn[t];
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j) xv[j] = *reinterpret_cast<const f32x4 *>(xl + p * RS + (2 * j + g) * 4);
        } else {
#pragma unroll
            for (int j = 0; j < NJ; ++j) xv[j] = xn[j];
        }
        if (blk + step < nblk) fetch(blk + step, xn);
        f32x16 S = bias;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) S = MFMA32(ws[j][i], xv[j][i], S);
        relu16(S);
        f32x16 G0, G1;
        const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if constexpr (TR) {
            G0 = MFMA32(S[0], wa[0][0], zero);
            G1 = MFMA32(S[0], wb[0][0], zero);
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4)
#pragma unroll
                for (int i = (q4 == 0 ? 1 : 0); i < 4; ++i) {
                    G0 = MFMA32(S[4 * q4 + i], wa[q4][i], G0);
                    G1 = MFMA32(S[4 * q4 + i], wb[q4][i], G1);
                }
            // register r of G0/G1: pixel 8*(r/4) + 4*g + r%4 of the block, channel p (+32)
            const long long q0 = blk * 32 + 4 * g;
            float *o = a.out + q0 * 64 + p;
            if (blk * 32 + 32 <= a.npix) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    o[(8 * (r / 4) + r % 4) * 64] = G0[r];
                    o[(8 * (r / 4) + r % 4) * 64 + 32] = G1[r];
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (q0 + 8 * (r / 4) + r % 4 < a.npix) {
                        o[(8 * (r / 4) + r % 4) * 64] = G0[r];
                        o[(8 * (r / 4) + r % 4) * 64 + 32] = G1[r];
                    }
            }
            continue;
        }
        G0 = MFMA32(wa[0][0], S[0], zero);              // C = 0 as an inline constant: no accumulator clearing
        G1 = MFMA32(wb[0][0], S[0], zero);
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4)
#pragma unroll
            for (int i = (q4 == 0 ? 1 : 0); i < 4; ++i) {
                G0 = MFMA32(wa[q4][i], S[4 * q4 + i], G0);
                G1 = MFMA32(wb[q4][i], S[4 * q4 + i], G1);
            }
        const long long q = blk * 32 + p;
        if (q < a.npix) {
            float *o = a.out + q * 64 + 4 * g;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                f32x4 v0, v1;
#pragma unroll
                for (int i = 0; i < 4; ++i) { v0[i] = G0[4 * j + i]; v1[i] = G1[4 * j + i]; }
                *reinterpret_cast<f32x4 *>(o + 8 * j) = v0;
                *reinterpret_cast<f32x4 *>(o + 32 + 8 * j) = v1;
            }
        }
    }
}

template <int CIN, bool BF = false>
__global__ __launch_bounds__(256) void sqg_stream_kernel(const SqgArgs a) { sqg_stream_body<CIN, false, false, BF>(a, blockIdx.x, gridDim.x); }

// Levels 1-4 in ONE launch (C_in = 32, 64, 128, 256).  Levels 2-4 together are a tenth of level 1's work and as
// launches of their own were dominated by launch ramp and tail (13-25 us each for 2-9 us of work); level 1 is a pure
// HBM stream (82 MB in, 164 MB out at batch 64).  r02: every launch of this network costs ~10 us of fixed time
// (dispatch + first-load latency + tail, measured as 2 t(N=64) - t(N=128) per kernel), so the four go out together after
// level 4: the small levels' blocks come first and finish inside the first microseconds of level 1's stream.
template <bool TR, bool LT, bool BF = false>
__global__ __launch_bounds__(256, 2) void sqg_multi_kernel(const SqgMultiArgs m) {
    __shared__ __attribute__((aligned(16))) float lds_x[LT ? 4 * SQG_LDS_WAVE : 4];
    const int b = blockIdx.x;
    const int e1 = m.nb[1], e2 = e1 + m.nb[2], e3 = e2 + m.nb[3];
    if (b < e1) sqg_stream_body<64, TR, LT, BF>(m.lv[1], b, m.nb[1], lds_x);
    else if (b < e2) sqg_body<128, BF>(m.lv[2], b - e1, m.nb[2]);
    else if (b < e3) sqg_body<256, BF>(m.lv[3], b - e2, m.nb[3]);
    else sqg_stream_body<32, TR, LT, BF>(m.lv[0], b - e3, m.nb[0], lds_x);
}

hipError_t launch_sqg_multi(const SqgArgs lv[4], hipStream_t s) {
    if (lv[0].cin != 32 || lv[1].cin != 64 || lv[2].cin != 128 || lv[3].cin != 256) return hipErrorInvalidValue;
    SqgMultiArgs m;
    int total = 0;
    for (int i = 0; i < 4; ++i) {
        m.lv[i] = lv[i];
        long long wg = ((lv[i].npix + 31) / 32 + 3) / 4;
        if (wg > 2048) wg = 2048;
        m.nb[i] = (int)wg;
        total += m.nb[i];
    }
    const int bf = lv[0].x_bf16;                        // one input format per launch: the four maps belong to one plan
    for (int i = 1; i < 4; ++i) if (lv[i].x_bf16 != bf) return hipErrorInvalidValue;
    for (int i = 0; i < 4; ++i) if (bf && lv[i].npix && (lv[i].hw < 1 || lv[i].npix % lv[i].hw)) return hipErrorInvalidValue;
    if (bf) hipLaunchKernelGGL((sqg_multi_kernel<true, false, true>), dim3((unsigned)total), dim3(256), 0, s, m);
    else hipLaunchKernelGGL((sqg_multi_kernel<true, true>), dim3((unsigned)total), dim3(256), 0, s, m);
    return hipGetLastError();
}

hipError_t launch_sqg(const SqgArgs &a, hipStream_t s) {
    const long long nblk = (a.npix + 31) / 32;
    long long wg = (nblk + 3) / 4;
    if (wg > 256 * 8) wg = 256 * 8;
    dim3 grid((unsigned)wg), block(256);
    if (a.x_bf16) {
        if (a.hw < 1 || a.npix % a.hw) return hipErrorInvalidValue;
        switch (a.cin) {
            case 32: hipLaunchKernelGGL((sqg_stream_kernel<32, true>), grid, block, 0, s, a); break;
            case 64: hipLaunchKernelGGL((sqg_stream_kernel<64, true>), grid, block, 0, s, a); break;
            case 128: hipLaunchKernelGGL((sqg_kernel<128, true>), grid, block, 0, s, a); break;
            case 256: hipLaunchKernelGGL((sqg_kernel<256, true>), grid, block, 0, s, a); break;
            default: return hipErrorInvalidValue;
        }
        return hipGetLastError();
    }
    switch (a.cin) {
        case 32: hipLaunchKernelGGL(sqg_stream_kernel<32>, grid, block, 0, s, a); break;
        case 64: hipLaunchKernelGGL(sqg_stream_kernel<64>, grid, block, 0, s, a); break;
        case 128: hipLaunchKernelGGL(sqg_kernel<128>, grid, block, 0, s, a); break;
        case 256: hipLaunchKernelGGL(sqg_kernel<256>, grid, block, 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// The head works on 16x16 pixel tiles (H, W are multiples of 16) = 8 blocks of 32 pixels (two tile rows each).
//
// LDS holds the low-resolution windows of G_1..G_4 a tile's bilinear taps touch:
// for level l (factor f = 2^l, pb = (f-1)/2) output row y reads source rows
// i1 = (y+pb)>>l and i1-1, so a 16-row tile origin y0 needs rows (y0>>l)-1 .. (y0>>l)+((15+pb)>>l):
// 9, 6, 4, 3 rows (and columns) for l = 1..4, i.e. 81+36+16+9 = 142 source pixels x 64 ch.
// Rows/columns outside the map are stored as zeros, which is exactly the reference's
// un-normalised border (the tap is dropped).  Pixel stride is 68 floats
// so the ds_read_b128 of 16 lanes with different source pixels hit distinct bank quads.
// ---------------------------------------------------------------------------
constexpr int HT = 16;                                 // tile edge
constexpr int GSTRIDE = 68;                            // floats per staged source pixel
__host__ __device__ constexpr int win_n(int l) { return l == 1 ? 9 : l == 2 ? 6 : l == 3 ? 4 : 3; }
__host__ __device__ constexpr int win_base(int l) { return l == 1 ? 0 : l == 2 ? 81 : l == 3 ? 117 : 133; }
constexpr int GPIX = 142;

#ifdef UKBB_DIAG
__device__ unsigned long long g_hstamps[16];
#endif
// ---------------------------------------------------------------------------
// Producer/consumer head (768 threads, persistent over 16x16 tiles, one workgroup per CU):
//   waves 4-11 "producers": stage the G windows of upcoming tiles (global -> registers -> LDS,
//       double buffered per tile) and evaluate, for the 32-pixel block their partner wave will
//       process next, out0's pre-activation  b0 + sum_l up_l(G_l)  (all VALU + LDS work), which
//       they hand over through LDS as a ready accumulator tile (8 float4 per lane, laid out
//       [slot][lane] so both sides touch consecutive 16-byte words);
//   waves 0-3 "consumers": same_dim0 (8 MFMA) -> out0 level-0 slice accumulated ONTO the handed
//       tile (32 MFMA) -> ReLU -> out1 (64 MFMA) -> ReLU -> logits / softmax / argmax.
// A stage = one block per consumer wave (2 stages per tile); one barrier per stage.
// r08: the producers evaluate the bilinear taps separably with channels on the lanes (x once per window row, y per output row with
// compile-time weights), so a stage is eight contiguous tile rows and consumer wave w takes block 4 * (stage & 1) + w; the
// r02-r07 direct 2-D gather (one pixel per lane, blocks 2 w + (stage & 1)) is the DG instance (UKBB_HEAD_DIRECT_GATHER=1).
// r01 measurements behind this split: in the single-role kernel (one workgroup per tile, every wave both roles; since removed,
// its numbers are in profiles/r01_notes.md) the gather (VALU+LDS), the G staging and the MFMA chains simply added up (ablation:
// 76 + 63 + 40%..) because every wave ran them back to back and at most 3 waves fit per SIMD.
// ---------------------------------------------------------------------------
constexpr int PX_WAVE = 8 * 64 * 4;                    // floats of one handed-over tile (64 ch x 32 px)
// LDS map of fcn_head_pc_kernel (floats)
constexpr int L_GW = 0;                                // [2][GPIX][GSTRIDE]  G windows, double buffered per tile
constexpr int L_PX = L_GW + 2 * GPIX * GSTRIDE;        // [4][PX_WAVE]        hand-over tiles (single buffered)
// Weight part of the map: fp32 fragments, or (X3) out0's level-0 slice and out1 as three bf16 pieces per weight, or (BM, UKBB_PREC_BF16_FULL)
// the three matrices as one bf16 piece each (pack_head_bf16)
template <bool X3, bool BM = false> struct HeadLds {
    static constexpr int WS0 = L_PX + 4 * PX_WAVE;             // pack_sq(same_dim0)                                   512 | BM 256 dwords
    static constexpr int WO0 = WS0 + (BM ? 256 : 512);         // pack_rowmap(out0 rows 0..31) 2048 | pack_head_x3(.., 32) 3072 dwords | BM 1024
    static constexpr int WO1 = WO0 + (BM ? 1024 : X3 ? 3072 : 2048);   // pack_rowmap(out1) x2  4096 | pack_head_x3(.., 64) 6144 dwords | BM 2048
    static constexpr int BS0 = WO1 + (BM ? 2048 : X3 ? 6144 : 4096);   // 32
    static constexpr int BO0 = BS0 + 32;                       // 64
    static constexpr int BO1 = BO0 + 64;                       // 64
    static constexpr int WLG = BO1 + 64;                       // [2][NCLS][32] <= 384
    static constexpr int BLG = WLG + 384;                      // <= 8
    static constexpr int FLOATS = BLG + 8;
};
constexpr int HEADPC_LDS_FLOATS = HeadLds<false>::FLOATS;
constexpr int HEADPC_X3_LDS_FLOATS = HeadLds<true>::FLOATS;
constexpr int HEADPC_BM_LDS_FLOATS = HeadLds<false, true>::FLOATS;
static_assert(HEADPC_BM_LDS_FLOATS < HEADPC_LDS_FLOATS, "the bf16 head's weights take less LDS than the fp32 fragments");
static_assert(HEADPC_X3_LDS_FLOATS * 4 <= 160 * 1024, "head kernel LDS");

// An LDS pointer the optimiser cannot see through: reads at compile-time distances from it become one base register plus the
// instruction's immediate offset, instead of one loop-invariant address register per distance (r11: 16 of them in the consumer loop)
typedef const __attribute__((address_space(3))) float lds_cf;
typedef const __attribute__((address_space(3))) f32x4 lds_cf4;
__device__ __forceinline__ lds_cf *lds_opaque(const float *p) { lds_cf *q = (lds_cf *)p; asm volatile("" : "+v"(q)); return q; }
__device__ __forceinline__ f32x4 lds4(lds_cf *p) { return *(lds_cf4 *)p; }

__device__ __forceinline__ f32x16 bias_tile_lds(const float *bias, int g) {
    f32x16 acc;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const f32x4 b = ld4(bias + 8 * j + 4 * g);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[4 * j + i] = b[i];
    }
    return acc;
}

__device__ __forceinline__ void chain_32to64_lds(const float *wp, int lane, const f32x16 &X, f32x16 &D0, f32x16 &D1) {
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
        const f32x4 wa = ld4(wp + ((0 * 4 + q4) * 64 + lane) * 4);
        const f32x4 wb = ld4(wp + ((1 * 4 + q4) * 64 + lane) * 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            D0 = MFMA32(wa[i], X[4 * q4 + i], D0);
            D1 = MFMA32(wb[i], X[4 * q4 + i], D1);
        }
    }
}

// ---- X3 experiment: an fp32-exact product from bf16 pieces on the dense matrix cores ---------------------------------------
// x = h + m + l with h = bf16(x), m = bf16(x - h), l = x - h - m (all exact in fp32); W likewise on the host.  The six partial
// products that matter (hh, hm, mh, mm, hl, lh) run as v_mfma_f32_32x32x16_bf16 with fp32 accumulation; what is dropped is
// below 2^-24 of |x||w| per product (profiles/r02_notes.md section 11).
// split_pair (device_prims.h) forms the pieces of two values at once.

// ---- separable gather (r08): which x-interpolated window rows a run of four output rows reads ---------------------------------
// Tile origins are multiples of 16 >= f, so for tile row r the level-l taps sit in window rows (r + pb) >> l (weight
// (f - 1 - jy) / f, zero when jy = f - 1) and that + 1 (weight (jy + 1) / f), jy = (r + pb) & (f - 1): compile-time per run.
__host__ __device__ constexpr int sep_pb(int l) { return ((1 << l) - 1) >> 1; }
__host__ __device__ constexpr int sep_row0(int r0, int l) { return (r0 + sep_pb(l)) >> l; }   // window row of h[0]
__host__ __device__ constexpr bool sep_row_used(int r0, int l, int k) {   // does output row r0..r0+3 read window row row0 + k?
    const int f = 1 << l, i = sep_row0(r0, l) + k;
    bool used = false;
    for (int t = 0; t < 4; ++t) {
        const int y = r0 + t + sep_pb(l);
        if ((y >> l) + 1 == i || ((y >> l) == i && (y & (f - 1)) != f - 1)) used = true;
    }
    return used;
}

// ---- deferred tail (r11): behind which MFMA of the next block's same_dim0 (slots 0..7) and out0 (8..39) step k = 0..6 of finishing
// a block's logits issues.  One step per three or four MFMAs: a step's LDS reads are used by the next one, two to four MFMAs later,
// and step 2 falls behind same_dim0's last MFMA, whose result the wave has to wait for anyway.
__host__ __device__ constexpr int fin_slot(int k) { return k < 3 ? 1 + 3 * k : 7 + 4 * (k - 2); }
__host__ __device__ constexpr int fin_step_at(int m) {
    for (int k = 0; k < 7; ++k) if (fin_slot(k) == m) return k;
    return -1;
}
static_assert(fin_slot(2) == 7 && fin_slot(6) == 23, "tail steps end well inside out0's 32 MFMAs");

#ifdef UKBB_DIAG
#define UKBB_HS(var, prev) { __builtin_amdgcn_sched_barrier(0); asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); const unsigned long long t_ = __builtin_amdgcn_s_memtime(); var += t_ - prev; prev = t_; __builtin_amdgcn_sched_barrier(0); }
#else
#define UKBB_HS(var, prev)
#endif

// The consumer waves (0-3) of the fp32 separable instance of fcn_head_pc_kernel; same barriers, hand-over tile and block order as the
// in-stage loop in the kernel (barrier X, then A_s and B_s per stage).
// BF: conv0 is bf16 (HeadArgs::conv0_bf16); the prefetched block half rides in xv0 and is widened where the fp32 form first uses x0 / x1.
template <int NCLS, bool BF>
__device__ __forceinline__ void head_consumer_deferred(const HeadArgs &a, float *lds, int nstages, int tiles_x, int tiles_y) {
    using LM = HeadLds<false>;
    constexpr int L_WS0 = LM::WS0, L_WO0 = LM::WO0, L_WO1 = LM::WO1, L_BS0 = LM::BS0, L_BO1 = LM::BO1, L_WLG = LM::WLG, L_BLG = LM::BLG;
    const float *px = lds + L_PX;
    const int lane = threadIdx.x & 63, p = lane & 31, g = lane >> 5, wave = threadIdx.x >> 6;
    auto pixel_of = [&](int s) -> size_t {
        int bid = blockIdx.x + (s >> 1) * gridDim.x;
        const int tx = bid % tiles_x; bid /= tiles_x;
        const int ty = bid % tiles_y;
        const int n = bid / tiles_y;
        const int blk = 4 * (s & 1) + wave;             // stage s & 1 = tile rows 8 (s & 1) .. + 7
        const int y = ty * HT + 2 * blk + (p >> 4), x = tx * HT + (p & 15);
        return ((size_t)n * a.H + y) * a.W + x;
    };
    f32x4 xv0 = {0.f, 0.f, 0.f, 0.f}, xv1 = xv0;          // conv0 features of the NEXT block, prefetched
    size_t qnext = 0;                                   // and its pixel index: pixel_of runs once per stage
    auto fetch_conv0 = [&](size_t q) {
        if constexpr (BF) xv0 = __builtin_bit_cast(f32x4, ld_block_half(reinterpret_cast<const char *>(a.conv0) + q * 32 + 16 * g));
        else { xv0 = ld4(a.conv0 + q * 16 + 4 * g); xv1 = ld4(a.conv0 + q * 16 + 8 + 4 * g); }
    };
    if (nstages > 0) {
        qnext = pixel_of(0);
        fetch_conv0(qnext);
    }
    __syncthreads();                                    // barrier X
#ifdef UKBB_DIAG
    // stamps as in the kernel's in-stage loop; the segments here: same_dim0 with three steps of the previous block's tail | out0 with
    // four steps, the store and relu16(P0) | out1 with relu16(P1) and this block's first logits half | (empty)
    unsigned long long hs_a = 0, hs_r = 0, hs_b = 0, hs_j[4] = {0, 0, 0, 0}, hs_t0 = __builtin_amdgcn_s_memtime();
#endif
    // ---- deferred tail (r11) ---------------------------------------------------------------------------------------------
    // A block's logits need out1's last MFMA, and every step after it (ReLU, a chain of dependent FMAs per class fed from LDS,
    // the exchange between the lane halves, the compare chain, the store) waits on the one before while the SIMD's matrix pipe
    // has nothing to issue.  So out1 runs as two dependent runs, Q0's 32 MFMAs and then Q1's: Q0's ReLU and its half of the
    // logits FMAs issue between Q1's MFMAs, and Q1 (before its ReLU), the NCLS partial sums and the pixel index are carried
    // over the back-edge and finished between the MFMAs of the next block's same_dim0 and out0 (fin_slot); the store fills the
    // wait at the end of out0.  Every accumulator and every class sum adds its terms in the order of the in-stage form, so no bit moves
    // (tests/test_head_tail_gpu.py).  sched_barrier pins each step behind its MFMA for the machine scheduler (left alone it sinks the
    // step to its first use); Q1's MFMAs, whose result nothing reads inside the stage, are tied to their steps by an empty asm as well.
    lds_cf *const wbase = lds_opaque(lds + L_WS0 + lane * 4);          // weight fragments: [fragment][lane] float4
    lds_cf *const bbase = lds_opaque(lds + L_BS0 + 4 * g);             // bias tiles: register 4 j + i = bias[8 j + 4 g + i]
    lds_cf *const lbase = lds_opaque(lds + L_WLG + g * NCLS * 32);     // logits weights of the lane's half
    auto bias_tile_at = [&](int off) {
        f32x16 acc;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f32x4 b = lds4(bbase + off + 8 * j);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[4 * j + i] = b[i];
        }
        return acc;
    };
    f32x16 Qd;                                      // out1 rows 32..63 of the deferred block, before ReLU
#pragma unroll
    for (int r = 0; r < 16; ++r) Qd[r] = 0.f;
    f32x2 accd[NCLS];                               // its class sums over rows 0..31
    f32x4 wl[NCLS];                                 // logits weights in flight
    float hsum[NCLS], hoth[NCLS], hbias[NCLS], lgd[NCLS];
#pragma unroll
    for (int c = 0; c < NCLS; ++c) accd[c] = f32x2{0.f, 0.f};
    size_t qd = 0;
    auto relu_n = [&](f32x16 &Q, auto r0c, auto nc) {
#pragma unroll
        for (int r = 0; r < decltype(nc)::value; ++r) Q[decltype(r0c)::value + r] = relu_bits(Q[decltype(r0c)::value + r]);
    };
    auto lg_load = [&](int j, int half) {           // weights of channels 32 half + rowmap(4 j .. 4 j + 3, g), every class
#pragma unroll
        for (int c = 0; c < NCLS; ++c) wl[c] = lds4(lbase + c * 32 + 16 * half + 4 * j);
    };
    // step k of one half (16 registers Q) of the logits product: 0, 1 ReLU (and the first weights), 2..5 the FMAs of registers
    // 4 (k - 2) .. + 3, classes interleaved (per class the additions keep the order of the in-stage form), weights one step ahead
    auto half_step = [&](auto kc, auto halfc, f32x16 &Q, f32x2 (&acc)[NCLS]) {
        constexpr int k = decltype(kc)::value, half = decltype(halfc)::value;
        if constexpr (k == 0) { lg_load(0, half); relu_n(Q, std::integral_constant<int, 0>{}, std::integral_constant<int, 8>{}); }
        else if constexpr (k == 1) relu_n(Q, std::integral_constant<int, 8>{}, std::integral_constant<int, 8>{});
        else if constexpr (k <= 5) {
            constexpr int j = k - 2;
#pragma unroll
            for (int c = 0; c < NCLS; ++c) acc[c] = pk_fma(f32x2{wl[c][0], wl[c][1]}, f32x2{Q[4 * j], Q[4 * j + 1]}, acc[c]);
#pragma unroll
            for (int c = 0; c < NCLS; ++c) acc[c] = pk_fma(f32x2{wl[c][2], wl[c][3]}, f32x2{Q[4 * j + 2], Q[4 * j + 3]}, acc[c]);
            if constexpr (j < 3) lg_load(j + 1, half);
        }
    };
    auto fin = [&](auto kc) {                       // step k = 0..7 of finishing the deferred block: Qd's half, then the reduction
        constexpr int k = decltype(kc)::value;
        if constexpr (k <= 5) half_step(kc, std::integral_constant<int, 1>{}, Qd, accd);
        else if constexpr (k == 6) {
#pragma unroll
            for (int c = 0; c < NCLS; ++c) { hsum[c] = accd[c][0] + accd[c][1]; hbias[c] = lds[L_BLG + c]; }
#pragma unroll
            for (int c = 0; c < NCLS; ++c) hoth[c] = __shfl_xor(hsum[c], 32);
        } else {
            // both halves form (lower + upper) in the SAME order -> identical bits
#pragma unroll
            for (int c = 0; c < NCLS; ++c) lgd[c] = (g == 0 ? hsum[c] + hoth[c] : hoth[c] + hsum[c]) + hbias[c];
        }
    };
    auto store_tail = [&](size_t qq) {
        if (g == 0) {
            if (a.logits) {
#pragma unroll
                for (int c = 0; c < NCLS; ++c) a.logits[qq * NCLS + c] = lgd[c];
            }
            float pr[NCLS];
            const int best = softmax_argmax_opt<NCLS>(lgd, a.prob != nullptr, pr);
            if (a.pred) a.pred[qq] = best;
            if (a.prob) {
#pragma unroll
                for (int c = 0; c < NCLS; ++c) a.prob[qq * NCLS + c] = pr[c];
            }
        }
    };
#pragma unroll 1
    for (int s = 0; s < nstages; ++s) {
        const size_t q = qnext;
        f32x4 x0 = xv0, x1 = xv1;
#ifdef UKBB_DIAG
        unsigned long long hs_p = __builtin_amdgcn_s_memtime();
#endif
        __syncthreads();                                // barrier A_s: px[wave] ready
        UKBB_HS(hs_a, hs_p)
        f32x16 P0, P1;
        {
            const float *src = px + wave * PX_WAVE + lane * 4;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 v0 = ld4(src + j * 256);
                const f32x4 v1 = ld4(src + (4 + j) * 256);
#pragma unroll
                for (int i = 0; i < 4; ++i) { P0[4 * j + i] = v0[i]; P1[4 * j + i] = v1[i]; }
            }
        }
        UKBB_HS(hs_r, hs_p)
        __syncthreads();                                // barrier B_s: px may be overwritten
        UKBB_HS(hs_b, hs_p)
        if constexpr (BF) bf16_block_to_k(__builtin_bit_cast(u32x4, xv0), x0, x1);
        if (s + 1 < nstages) {                          // features of the next block: a whole stage to arrive
            qnext = pixel_of(s + 1);
            fetch_conv0(qnext);
        }
        // ---- same_dim0 and out0 (slots 0..39), with the seven steps of the tail of block s - 1 spread between their MFMAs
        // (at s = 0 that tail is all zeros and is not stored) ----
        f32x16 S = bias_tile_at(0);
        auto at_slot = [&](auto mc, auto &&mfma) {  // the MFMA of slot m and, pinned behind it, the tail step that belongs there
            constexpr int k = fin_step_at(decltype(mc)::value);
            if constexpr (k >= 0) __builtin_amdgcn_sched_barrier(0);
            mfma();
            if constexpr (k >= 0) { fin(std::integral_constant<int, k>{}); __builtin_amdgcn_sched_barrier(0); }
        };
        constexpr int WO0 = L_WO0 - L_WS0, WO1 = L_WO1 - L_WS0;
        f32x4 oa = lds4(wbase + WO0), ob = lds4(wbase + WO0 + 4 * 256);     // out0's first fragments
        {
            const f32x4 wv0 = lds4(wbase), wv1 = lds4(wbase + 256);
            unroll<8>([&](auto mc) {
                constexpr int m = decltype(mc)::value;
                at_slot(mc, [&] { S = MFMA32(m < 4 ? wv0[m & 3] : wv1[m & 3], m < 4 ? x0[m & 3] : x1[m & 3], S); });
            });
        }
        relu16(S);
        UKBB_HS(hs_j[0], hs_p)
        unroll<4>([&](auto qc) {
            constexpr int q4 = decltype(qc)::value;
            f32x4 na = oa, nb = ob;
            if constexpr (q4 < 3) { na = lds4(wbase + WO0 + (q4 + 1) * 256); nb = lds4(wbase + WO0 + (4 + q4 + 1) * 256); }
            unroll<4>([&](auto ic) {
                constexpr int i = decltype(ic)::value, m = 8 + 8 * q4 + 2 * i;
                at_slot(std::integral_constant<int, m>{}, [&] { P0 = MFMA32(oa[i], S[4 * q4 + i], P0); });
                at_slot(std::integral_constant<int, m + 1>{}, [&] { P1 = MFMA32(ob[i], S[4 * q4 + i], P1); });
            });
            oa = na; ob = nb;
        });
        f32x16 Q0 = bias_tile_at(L_BO1 - L_BS0), Q1;
        auto wf = [&](int G) {                   // out1 fragment G = 8 cb + k: rows 32 cb .. + 31 of the output, k steps 4 k .. 4 k + 3 of P0 (k < 4) / P1
            return lds4(wbase + WO1 + (((G & 4) ? 2 * 4 * 64 : 0) + ((G >> 3) * 4 + (G & 3)) * 64) * 4);
        };
        f32x4 wq = wf(0);
        fin(std::integral_constant<int, 7>{});
        if (s > 0) store_tail(qd);              // the last step and the stores, in the wait for out0's last MFMAs
        relu16(P0);
        UKBB_HS(hs_j[1], hs_p)
        // ---- out1 (slots 0..63): Q0's 32 MFMAs, then Q1's.  relu16(P1) sits behind the first MFMAs on P0; Q0's ReLU and its
        // half of the logits behind every fourth of Q1's ----
        f32x2 acc[NCLS];
#pragma unroll
        for (int c = 0; c < NCLS; ++c) acc[c] = f32x2{0.f, 0.f};
        unroll<16>([&](auto Gc) {
            constexpr int G = decltype(Gc)::value, k = G & 7;
            f32x4 wn = wq;
            if constexpr (G < 15) wn = wf(G + 1);
            if constexpr (G == 6) Q1 = bias_tile_at(L_BO1 - L_BS0 + 32);
            unroll<4>([&](auto ic) {
                constexpr int i = decltype(ic)::value, slot = 4 * G + i;
                constexpr bool relu_p1 = slot >= 1 && slot <= 4, head = slot >= 33 && slot <= 53 && (slot - 33) % 4 == 0;
                const float xb = k < 4 ? P0[4 * (k & 3) + i] : P1[4 * (k & 3) + i];
                if constexpr (relu_p1 || head) __builtin_amdgcn_sched_barrier(0);
                if constexpr (G < 8) Q0 = MFMA32(wq[i], xb, Q0);
                else Q1 = MFMA32(wq[i], xb, Q1);
                // sched_barrier binds the machine scheduler only: before it, an MFMA whose result nothing reads until the loop's end
                // floats below every barrier (all of Q1's run came out behind the last head step).  An empty volatile asm that
                // "rewrites" Q1 keeps this MFMA above the step and the next one below it.
                if constexpr (head) asm volatile("" : "+v"(Q1));
                if constexpr (relu_p1) relu_n(P1, std::integral_constant<int, 4 * (slot - 1)>{}, std::integral_constant<int, 4>{});
                if constexpr (head) half_step(std::integral_constant<int, (slot - 33) / 4>{}, std::integral_constant<int, 0>{}, Q0, acc);
                if constexpr (relu_p1 || head) __builtin_amdgcn_sched_barrier(0);
            });
            wq = wn;
        });
        UKBB_HS(hs_j[2], hs_p)
        Qd = Q1;
#pragma unroll
        for (int c = 0; c < NCLS; ++c) accd[c] = acc[c];
        qd = q;
    }
    if (nstages > 0) {                                  // the last block's tail
        unroll<8>([&](auto kc) { fin(kc); });
        store_tail(qd);
    }
#ifdef UKBB_DIAG
    if (lane == 0 && (a.diag & 64)) {
        atomicAdd(g_hstamps + 0, hs_a); atomicAdd(g_hstamps + 1, hs_r); atomicAdd(g_hstamps + 2, hs_b);
        atomicAdd(g_hstamps + 3, __builtin_amdgcn_s_memtime() - hs_t0); atomicAdd(g_hstamps + 4, (unsigned long long)nstages);
#pragma unroll
        for (int j = 0; j < 4; ++j) atomicAdd(g_hstamps + 5 + j, hs_j[j]);
    }
#endif
}

// DG: the r02-r07 direct 2-D gather (UKBB_HEAD_DIRECT_GATHER=1, A/B); otherwise the separable one
// IT: the consumers finish a block's logits inside its own stage (r01-r08; UKBB_HEAD_INLINE_TAIL=1, A/B).  The fp32 separable instance
// defers them instead (r11, DESIGN.md section 4 "Deferred tail"); the X3 and DG instances exist with IT = true only.
// BF: conv0 is bf16 [N][1][H][W][16] (HeadArgs::conv0_bf16, UKBB_PREC_BF16_STORE), widened to fp32 on the way in; the fp32 instances, and BM (below), which takes it as stored.
// BM: UKBB_PREC_BF16_FULL (HeadArgs::mm_bf16, include/ukbb_fcn.h).  The BF instance with same_dim0, out0's level-0 slice and out1 on
// v_mfma_f32_32x32x16_bf16, one bf16 piece per operand: 1 + 4 + 8 MFMAs per block instead of 8 + 32 + 64.  The stored conv0 half-block a lane
// loads (channels 8 g .. 8 g + 7 of pixel p) IS the B fragment of same_dim0, so nothing is widened or exchanged; S and P are rounded once (RNE)
// in registers as X3 rounds its high piece, and their registers are the next product's B fragments in the k order pack_head_bf16 gives the
// weights.  The handed tile enters out0 as the fp32 accumulator; biases, accumulators and everything behind out1's ReLU are the fp32 code of the
// in-stage form.  Separable gather and in-stage tail only: 13 MFMAs leave nothing to defer a tail under, and the two A/B knobs do not apply.
template <int NCLS, bool X3 = false, bool DG = false, bool IT = true, bool BF = false, bool BM = false>
__global__ __launch_bounds__(768) void fcn_head_pc_kernel(const HeadArgs a) {
    static_assert(!(X3 && BF), "bf16 conv0 is not combined with the f32x3 head");
    static_assert(!BM || (BF && !DG && IT), "the bf16 head reads the bf16 conv0 and exists in the separable, in-stage form only");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    using LM = HeadLds<X3, BM>;
    constexpr int L_WS0 = LM::WS0, L_WO0 = LM::WO0, L_WO1 = LM::WO1, L_BS0 = LM::BS0, L_BO0 = LM::BO0, L_BO1 = LM::BO1, L_WLG = LM::WLG, L_BLG = LM::BLG;
    float *gw = lds + L_GW;
    float *px = lds + L_PX;
    const int tiles_x = a.W / HT, tiles_y = a.H / HT;
    const int ntiles = a.N * tiles_y * tiles_x;
    const int my_tiles = (ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
    const int nstages = 2 * my_tiles;
    const bool producer = __builtin_amdgcn_readfirstlane(threadIdx.x) >= 256;
    const int lane = threadIdx.x & 63, p = lane & 31, g = lane >> 5;

    // ---- every weight / bias of the head lives in LDS for the lifetime of the workgroup ----
    {
        const int t = threadIdx.x;
        auto copy = [&](int dst, const float *src, int nfloat) {
            for (int i = t; i < nfloat; i += 768) lds[dst + i] = src[i];
        };
        if constexpr (BM) { copy(L_WS0, a.w_s0bf, 256); copy(L_WO0, a.w_o0bf, 1024); copy(L_WO1, a.w_o1bf, 2048); }
        else {
        copy(L_WS0, a.w_s0, 512);
        if constexpr (X3) { copy(L_WO0, a.w_o0x3, 3072); copy(L_WO1, a.w_o1x3, 6144); }
        else              { copy(L_WO0, a.w_o0, 2048);   copy(L_WO1, a.w_o1, 4096); }
        }
        copy(L_BS0, a.b_s0, 32);  copy(L_BO0, a.b_o0, 64);   copy(L_BO1, a.b_o1, 64);
        copy(L_WLG, a.w_lg, 2 * NCLS * 32); copy(L_BLG, a.b_lg, NCLS);
    }

    if (producer) {
        // 8 producer waves: waves 4-7 build channels 0..31 of the hand-over tile of consumer wave pw,
        // waves 8-11 channels 32..63 (the gather is the longest per-stage job; halving it per wave keeps
        // the producers ahead of the MFMA waves).  All 512 producer threads share the window staging.
        const int tid = threadIdx.x - 256, pw = (tid >> 6) & 3, half = tid >> 8;
        // Staging index space: every iteration (512 threads = 32 source pixels x 16 float4) belongs to ONE
        // level, so level, window width and the row/column split are compile-time per iteration:
        // l=1: 81 px -> 3 iterations, l=2: 36 -> 2, l=3: 16 -> 1, l=4: 9 -> 1.
        constexpr int NIT = 7;
        u32x4 gv[NIT];
        const int sp32 = tid >> 4, c4 = tid & 15;
        // Every VALU instruction of this role takes issue time from the consumers' MFMA stream (they
        // share the SIMDs), so the staging keeps its per-tile arithmetic on the scalar unit: per-thread
        // window coordinates and byte offsets are computed once, validity is one and/compare against a
        // per-tile row|column mask, and taps outside the map are buffer loads with an out-of-range
        // offset (the hardware returns 0, border taps are dropped).
        // The 14 per-thread window constants, evaluated once and kept in registers across the stage loop (recomputing them per tile freed the
        // 2 spilled VGPRs and cost 10 % of the head: profiles/r05_notes.md).  A lambda with its own sp32: written in line, hipcc orders two
        // instruction pairs of the fp32 instances differently from the code that was measured.
        unsigned tbit[NIT], goff[NIT];
        auto window_consts = [&]() {
        int sp32 = tid >> 4;
        unroll<NIT>([&](auto ic) {
            constexpr int it = decltype(ic)::value;
            constexpr int l = it < 3 ? 1 : it < 5 ? 2 : it < 6 ? 3 : 4;
            constexpr int it0 = l == 1 ? 0 : l == 2 ? 3 : l == 3 ? 5 : 6;
            constexpr int wn_ = win_n(l);
            const int rel = (it - it0) * 32 + sp32;
            const int ry = rel / wn_, rx = rel - ry * wn_;
            tbit[it] = rel < wn_ * wn_ ? (1u << ry) | (1u << (16 + rx)) : 0x80000000u;   // bit 31 never set in a tile mask
            goff[it] = (unsigned)((ry * (a.W >> l) + rx) * 64 + 4 * c4) * 4u;
        });
        };
        window_consts();
        auto g_load = [&](int k) {                      // G windows of this workgroup's k-th tile -> registers
            int bid = blockIdx.x + k * gridDim.x;
            const int tx = bid % tiles_x; bid /= tiles_x;
            const int ty = bid % tiles_y;
            const int n = bid / tiles_y;
            const int y0 = ty * HT, x0 = tx * HT;
            __amdgpu_buffer_rsrc_t rs[4];
            unsigned cm[4];
#pragma unroll
            for (int l = 1; l <= 4; ++l) {
                const int hl = a.H >> l, wl = a.W >> l, wn_ = win_n(l);
                const int sy0 = (y0 >> l) - 1, sx0 = (x0 >> l) - 1;     // window origin in the level-l map
                const int ylo = sy0 < 0 ? -sy0 : 0, yhi = hl - sy0 < wn_ ? hl - sy0 : wn_;
                const int xlo = sx0 < 0 ? -sx0 : 0, xhi = wl - sx0 < wn_ ? wl - sx0 : wn_;
                cm[l - 1] = (((1u << yhi) - 1u) & ~((1u << ylo) - 1u)) | ((((1u << xhi) - 1u) & ~((1u << xlo) - 1u)) << 16);
                const float *base = a.G[l - 1] + ((long long)(n * hl + sy0) * wl + sx0) * 64;   // may precede the map; masked lanes never use it
                rs[l - 1] = __builtin_amdgcn_make_buffer_rsrc((void *)base, 0, 0x7fffffff, 0x00020000);
            }
            unroll<NIT>([&](auto ic) {
                constexpr int it = decltype(ic)::value;
                constexpr int l = it < 3 ? 1 : it < 5 ? 2 : it < 6 ? 3 : 4;
                const unsigned vo = (cm[l - 1] & tbit[it]) == tbit[it] ? goff[it] : 0x80000000u;
                gv[it] = __builtin_amdgcn_raw_buffer_load_b128(rs[l - 1], vo, 0, 0);
            });
        };
        float *const gdst = gw + sp32 * GSTRIDE + 4 * c4;
        auto g_store = [&](int b) {
            float *dst = gdst + b * GPIX * GSTRIDE;
            unroll<NIT>([&](auto ic) {
                constexpr int it = decltype(ic)::value;
                constexpr int l = it < 3 ? 1 : it < 5 ? 2 : it < 6 ? 3 : 4;
                constexpr int it0 = l == 1 ? 0 : l == 2 ? 3 : l == 3 ? 5 : 6;
                const int rel = (it - it0) * 32 + sp32;
                if (rel < win_n(l) * win_n(l))
                    *reinterpret_cast<u32x4 *>(dst + (win_base(l) + (it - it0) * 32) * GSTRIDE) = gv[it];
            });
        };
        // Gather constants of this thread, for both block parities (a wave alternates between the two
        // 32-pixel blocks 2*pw and 2*pw+1 of a tile): LDS offset of the top-left tap and the four tap
        // weights per level.  Computed once; the stage loop is unrolled by four so the block parity and
        // the window buffer are compile-time and every LDS address is base register + immediate.
        int tap0[2][4];
        float tw[2][4][4];
#pragma unroll
        for (int par = 0; par < (DG ? 2 : 0); ++par) {
            const int blk = pw * 2 + par;
            const int yl = 2 * blk + (p >> 4), xl = p & 15;
#pragma unroll
            for (int l = 1; l <= 4; ++l) {
                const int f = 1 << l, pb = (f - 1) >> 1;
                const float inv = 1.0f / (float)f;
                const int tyy = yl + pb, txx = xl + pb;
                const int ry1 = (tyy >> l) + 1, rx1 = (txx >> l) + 1;
                const int jy = tyy & (f - 1), jx = txx & (f - 1);
                const float wy1 = (float)(jy + 1) * inv, wy0 = (float)(f - 1 - jy) * inv;
                const float wx1 = (float)(jx + 1) * inv, wx0 = (float)(f - 1 - jx) * inv;
                tap0[par][l - 1] = (win_base(l) + (ry1 - 1) * win_n(l) + (rx1 - 1)) * GSTRIDE + 4 * g + 32 * half;
                tw[par][l - 1][0] = wy0 * wx0; tw[par][l - 1][1] = wy0 * wx1;
                tw[par][l - 1][2] = wy1 * wx0; tw[par][l - 1][3] = wy1 * wx1;
            }
        }
        // Separable gather constants.  Channels on the lanes: producer wave 4 + 4 rg + cb owns channels 16 cb .. 16 cb + 15 of tile rows
        // 8 PAR + 4 rg .. + 3 (a run of four rows, consumer waves 2 rg and 2 rg + 1); a lane holds the float4 of channels 4 k4 .. 4 k4 + 3
        // (k4 = 4 cb + cg) of column lane & 15.  cg is the lane's ds_read_b128 lane group ({0-3,12-15,20-27}, {4-11,16-19,28-31}, and
        // the same + 32), so the 16 lanes the LDS serves together read one channel group of 16 different columns: at most 9 window
        // pixels, on distinct bank quads (stride 68 floats).  The hand-over stores (8 consecutive lanes per LDS cycle) then write 8
        // different columns.  Per level: the LDS offset of the lane's x0 tap in window row 0, and its two x weights (the y weights are
        // compile-time, sep_row_used).
        const int l5 = lane & 31, col = lane & 15;
        const int cb = (tid >> 6) & 3, k4 = 4 * cb + 2 * (lane >> 5) + ((((l5 + 4) >> 3) ^ (l5 >> 4)) & 1);
        int xoff[4];
        float wx0[4], wx1[4];
#pragma unroll
        for (int l = 1; l <= (DG ? 0 : 4); ++l) {
            const int f = 1 << l, txx = col + sep_pb(l), jx = txx & (f - 1);
            const float inv = 1.0f / (float)f;
            xoff[l - 1] = (win_base(l) + (txx >> l)) * GSTRIDE + 4 * k4;
            wx1[l - 1] = (float)(jx + 1) * inv;
            wx0[l - 1] = (float)(f - 1 - jx) * inv;
        }
        f32x16 P;                                       // DG: 16 channels of one pixel; else register 4 t + i = channel 4 k4 + i of run row t
        auto gather_sep = [&](auto parc, auto bufc, auto rgc) {
            constexpr int BUF = decltype(bufc)::value, R0 = 8 * decltype(parc)::value + 4 * decltype(rgc)::value;
            const f32x4 b = ld4(lds + L_BO0 + 4 * k4);
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int i = 0; i < 4; ++i) P[4 * t + i] = b[i];
#ifdef UKBB_DIAG
            if (a.diag & 1) return;                 // ablation: no gather (hand over the bias tile only)
#endif
            unroll<4>([&](auto lc) {
                constexpr int l = decltype(lc)::value + 1, f = 1 << l, wn_ = win_n(l), I0 = sep_row0(R0, l);
                static_assert(sep_row0(R0 + 3, l) + 1 - I0 < 3, "a run of four rows reads at most three window rows");
                const float *src = gw + BUF * GPIX * GSTRIDE + xoff[l - 1] + I0 * wn_ * GSTRIDE;
                const float u0 = wx0[l - 1], u1 = wx1[l - 1];
                f32x4 h[3];                             // window rows I0 .. I0 + 2, interpolated in x at the lane's column
                unroll<3>([&](auto kc) {
                    constexpr int k = decltype(kc)::value;
                    if constexpr (sep_row_used(R0, l, k)) {
                        const f32x4 a0 = ld4(src + k * wn_ * GSTRIDE), a1 = ld4(src + k * wn_ * GSTRIDE + GSTRIDE);
#pragma unroll
                        for (int i = 0; i < 4; ++i) h[k][i] = fmaf(u0, a0[i], u1 * a1[i]);
                    }
                });
                unroll<4>([&](auto tc) {
                    constexpr int t = decltype(tc)::value, y = R0 + t + sep_pb(l), i1 = (y >> l) - I0, jy = y & (f - 1);
                    constexpr float wy1 = (float)(jy + 1) / (float)f, wy0 = (float)(f - 1 - jy) / (float)f;
#pragma unroll
                    for (int i = 0; i < 4; ++i) P[4 * t + i] = fmaf(wy1, h[i1 + 1][i], P[4 * t + i]);
                    if constexpr (jy != f - 1) {        // a zero y weight: the tap is dropped, not multiplied
#pragma unroll
                        for (int i = 0; i < 4; ++i) P[4 * t + i] = fmaf(wy0, h[i1][i], P[4 * t + i]);
                    }
                });
            });
        };
        auto hand_over_sep = [&](auto rgc) {            // run row t = pixel 16 (t & 1) + col of consumer wave 2 RG + (t >> 1)
            constexpr int RG = decltype(rgc)::value;
            float *dst = px + (4 * (k4 >> 3) + ((k4 >> 1) & 3)) * 256 + (col + 32 * (k4 & 1)) * 4;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                f32x4 v;
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = P[4 * t + i];
                *reinterpret_cast<f32x4 *>(dst + (2 * RG + (t >> 1)) * PX_WAVE + 16 * (t & 1) * 4) = v;
            }
        };
        auto gather = [&](auto parc, auto bufc) {       // block 2*pw + PAR of the tile staged in window buffer BUF -> P (32 channels)
            constexpr int PAR = decltype(parc)::value, BUF = decltype(bufc)::value;
            P = bias_tile_lds(lds + L_BO0 + 32 * half, g);
#ifdef UKBB_DIAG
            if (a.diag & 1) return;                 // ablation: no gather (hand over the bias tile only)
#endif
#pragma unroll
            for (int l = 1; l <= 4; ++l) {
                const int wn_ = win_n(l);
                const float *b00 = gw + BUF * GPIX * GSTRIDE + tap0[PAR][l - 1];
                const float *b01 = b00 + GSTRIDE, *b10 = b00 + wn_ * GSTRIDE, *b11 = b10 + GSTRIDE;
                const float w00 = tw[PAR][l - 1][0], w01 = tw[PAR][l - 1][1], w10 = tw[PAR][l - 1][2], w11 = tw[PAR][l - 1][3];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f32x4 a00 = ld4(b00 + 8 * j), a01 = ld4(b01 + 8 * j), a10 = ld4(b10 + 8 * j), a11 = ld4(b11 + 8 * j);
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        P[4 * j + i] = fmaf(w00, a00[i], fmaf(w01, a01[i], fmaf(w10, a10[i], fmaf(w11, a11[i], P[4 * j + i]))));
                }
            }
        };
        auto hand_over = [&]() {                        // P -> px[pw]  ([slot][lane] float4 image)
            float *dst = px + pw * PX_WAVE + (4 * half) * 256 + lane * 4;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                f32x4 v;
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = P[4 * j + i];
                *reinterpret_cast<f32x4 *>(dst + j * 256) = v;
            }
        };
        // prologue: windows of tiles 0 and 1 into LDS
        if (my_tiles > 0) { g_load(0); g_store(0); }
        if (my_tiles > 1) { g_load(1); g_store(1); }
        __syncthreads();                                // barrier X: weights, GW[0], GW[1] visible
        auto stage = [&](auto parc, auto bufc, auto rgc, int s) {
            constexpr int PAR = decltype(parc)::value, BUF = decltype(bufc)::value;
            if constexpr (DG) {
                gather(parc, bufc);                     // LDS windows -> registers (consumers still busy with s-1)
                hand_over();                            // px was released at barrier B of stage s-1
            } else {
                gather_sep(parc, bufc, rgc);
                hand_over_sep(rgc);
            }
            __syncthreads();                            // barrier A_s: px ready
            __syncthreads();                            // barrier B_s: px consumed
            if constexpr (PAR == 1) {                   // tile k = s>>1 fully gathered: its window buffer is free
                // Fetch the windows of tile k+2 into it now, synchronously: the producers are far ahead of the
                // MFMA waves (they would only wait at barrier A), and a prefetch held in registers across the
                // next two gathers pushed the kernel into scratch spills.
                const int k = s >> 1;
                if (k + 2 < my_tiles) { g_load(k + 2); g_store(BUF); }
            }
        };
        constexpr std::integral_constant<int, 0> I0{};
        constexpr std::integral_constant<int, 1> I1{};
        auto run = [&](auto rgc) {                      // separable gather: one copy of the loop per run of rows (rg is wave-uniform)
#pragma unroll 1
            for (int s = 0; s < nstages; s += 4) {      // nstages is even
                stage(I0, I0, rgc, s);
                stage(I1, I0, rgc, s + 1);
                if (s + 2 < nstages) { stage(I0, I1, rgc, s + 2); stage(I1, I1, rgc, s + 3); }
            }
        };
        if constexpr (DG) run(I0);
        else if (__builtin_amdgcn_readfirstlane(tid) < 256) run(I0);
        else run(I1);
    } else if constexpr (!X3 && !DG && !IT) {
        head_consumer_deferred<NCLS, BF>(a, lds, nstages, tiles_x, tiles_y);
    } else {
        const int wave = threadIdx.x >> 6;
        const float *w_s0 = lds + L_WS0, *w_o0 = lds + L_WO0, *w_o1 = lds + L_WO1, *w_lg = lds + L_WLG;
        auto pixel_of = [&](int s) -> size_t {
            int bid = blockIdx.x + (s >> 1) * gridDim.x;
            const int tx = bid % tiles_x; bid /= tiles_x;
            const int ty = bid % tiles_y;
            const int n = bid / tiles_y;
            const int blk = DG ? wave * 2 + (s & 1) : 4 * (s & 1) + wave;   // separable gather: stage s & 1 = tile rows 8 (s & 1) .. + 7
            const int y = ty * HT + 2 * blk + (p >> 4), x = tx * HT + (p & 15);
            return ((size_t)n * a.H + y) * a.W + x;
        };
        f32x4 xv0 = {0.f, 0.f, 0.f, 0.f}, xv1 = xv0;      // conv0 features of the NEXT block, prefetched
        auto fetch_conv0 = [&](size_t q) {
            if constexpr (BF) xv0 = __builtin_bit_cast(f32x4, ld_block_half(reinterpret_cast<const char *>(a.conv0) + q * 32 + 16 * g));
            else { xv0 = ld4(a.conv0 + q * 16 + 4 * g); xv1 = ld4(a.conv0 + q * 16 + 8 + 4 * g); }
        };
        if (nstages > 0) fetch_conv0(pixel_of(0));
        __syncthreads();                                // barrier X
#ifdef UKBB_DIAG
        // diagnostic build, UKBB_HEAD_STAMPS=1: where an MFMA wave's stage goes -- wait at barrier A (the producers' hand-off), the LDS
        // read of the handed tile, wait at barrier B, and the rest split at the joints of the chain (hs_j): same_dim0 with its ReLU,
        // out0 with its ReLU, out1 with its ReLU, logits up to the store (head_consumer_deferred: what its three segments hold).
        unsigned long long hs_a = 0, hs_r = 0, hs_b = 0, hs_j[4] = {0, 0, 0, 0}, hs_t0 = __builtin_amdgcn_s_memtime();
#endif
#pragma unroll 1
        for (int s = 0; s < nstages; ++s) {
            const size_t q = pixel_of(s);
            f32x4 x0 = xv0, x1 = xv1;
#ifdef UKBB_DIAG
            unsigned long long hs_p = __builtin_amdgcn_s_memtime();
#endif
            __syncthreads();                            // barrier A_s: px[wave] ready
            UKBB_HS(hs_a, hs_p)
            f32x16 P0, P1;
            {
                const float *src = px + wave * PX_WAVE + lane * 4;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f32x4 v0 = ld4(src + j * 256);
                    const f32x4 v1 = ld4(src + (4 + j) * 256);
#pragma unroll
                    for (int i = 0; i < 4; ++i) { P0[4 * j + i] = v0[i]; P1[4 * j + i] = v1[i]; }
                }
            }
            UKBB_HS(hs_r, hs_p)
            __syncthreads();                            // barrier B_s: px may be overwritten
            UKBB_HS(hs_b, hs_p)
            if constexpr (BF && !BM) bf16_block_to_k(__builtin_bit_cast(u32x4, xv0), x0, x1);
            if (s + 1 < nstages) fetch_conv0(pixel_of(s + 1));   // features of the next block: a whole stage to arrive
            // ---- same_dim0 ----
            f32x16 S = bias_tile_lds(lds + L_BS0, g);
            // BM: A fragment f of a block lies at [f][lane] float4; element e of the B fragment built from registers 8 c .. 8 c + 7 of a tile is
            // its row rowmap(8 c + e, g), the k order of pack_head_bf16(.., acc_k = 1)
            [[maybe_unused]] auto frag = [&](const float *w, int f) { return __builtin_bit_cast(u32x4, ld4(w + f * 256 + lane * 4)); };
            [[maybe_unused]] auto tile_b = [&](const f32x16 &X, int c) {
                u32x4 b;
#pragma unroll
                for (int d = 0; d < 4; ++d) b[d] = pack_bf16x2(X[8 * c + 2 * d], X[8 * c + 2 * d + 1]);
                return b;
            };
            if constexpr (BM) {                         // K = 16: the stored half-block as it was loaded is the B fragment
                S = mfma_bf16(frag(w_s0, 0), __builtin_bit_cast(u32x4, x0), S);
            } else {
                const f32x4 wv0 = ld4(w_s0 + lane * 4), wv1 = ld4(w_s0 + (64 + lane) * 4);
#pragma unroll
                for (int i = 0; i < 4; ++i) S = MFMA32(wv0[i], x0[i], S);
#pragma unroll
                for (int i = 0; i < 4; ++i) S = MFMA32(wv1[i], x1[i], S);
            }
            relu16(S);
            UKBB_HS(hs_j[0], hs_p)
#ifdef UKBB_DIAG
            if (a.diag & 2) { relu16(P0); relu16(P1); if (a.pred) a.pred[q] = (int)P0[0]; continue; }   // ablation: no out0/out1/logits
#endif
            // ---- out0: handed tile (bias + upsampled levels 1..4) + W0_0 * S ----
            if constexpr (BM) {                         // bf16(W) . bf16(S) onto the handed fp32 tile: fragment 2 cb + kc
                const u32x4 s0 = tile_b(S, 0), s1 = tile_b(S, 1);
                P0 = mfma_bf16(frag(w_o0, 0), s0, P0); P1 = mfma_bf16(frag(w_o0, 2), s0, P1);
                P0 = mfma_bf16(frag(w_o0, 1), s1, P0); P1 = mfma_bf16(frag(w_o0, 3), s1, P1);
            } else if constexpr (X3) {                  // out0's level-0 slice from bf16 pieces: K = 32 -> two chunks of 16
                u32x4 sh[2], sm[2], sl[2];
#pragma unroll
                for (int kc = 0; kc < 2; ++kc)
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        unsigned th, tm, tl;
                        split_pair(S[8 * kc + 2 * d], S[8 * kc + 2 * d + 1], th, tm, tl);
                        sh[kc][d] = th; sm[kc][d] = tm; sl[kc][d] = tl;
                    }
                const float *wx0 = lds + L_WO0 + lane * 4;
                auto A0 = [&](int t, int cb, int kc) { return __builtin_bit_cast(u32x4, ld4(wx0 + ((t * 2 + cb) * 2 + kc) * 256)); };
#pragma unroll
                for (int kc = 0; kc < 2; ++kc) {
                    const u32x4 ah0 = A0(0, 0, kc), ah1 = A0(0, 1, kc), am0 = A0(1, 0, kc), am1 = A0(1, 1, kc), al0 = A0(2, 0, kc), al1 = A0(2, 1, kc);
                    P0 = mfma_bf16(al0, sh[kc], P0); P1 = mfma_bf16(al1, sh[kc], P1);
                    P0 = mfma_bf16(ah0, sl[kc], P0); P1 = mfma_bf16(ah1, sl[kc], P1);
                    P0 = mfma_bf16(am0, sm[kc], P0); P1 = mfma_bf16(am1, sm[kc], P1);
                    P0 = mfma_bf16(am0, sh[kc], P0); P1 = mfma_bf16(am1, sh[kc], P1);
                    P0 = mfma_bf16(ah0, sm[kc], P0); P1 = mfma_bf16(ah1, sm[kc], P1);
                    P0 = mfma_bf16(ah0, sh[kc], P0); P1 = mfma_bf16(ah1, sh[kc], P1);
                }
            } else {
                chain_32to64_lds(w_o0, lane, S, P0, P1);
            }
            relu16(P0);
            relu16(P1);
            UKBB_HS(hs_j[1], hs_p)
            // ---- out1 ----
            f32x16 Q0 = bias_tile_lds(lds + L_BO1, g), Q1 = bias_tile_lds(lds + L_BO1 + 32, g);
            if constexpr (BM) {                         // K = 64: chunks 0, 1 are P0's registers, 2, 3 are P1's; fragment 4 cb + kc
                const u32x4 b0 = tile_b(P0, 0), b1 = tile_b(P0, 1), b2 = tile_b(P1, 0), b3 = tile_b(P1, 1);
                Q0 = mfma_bf16(frag(w_o1, 0), b0, Q0); Q1 = mfma_bf16(frag(w_o1, 4), b0, Q1);
                Q0 = mfma_bf16(frag(w_o1, 1), b1, Q0); Q1 = mfma_bf16(frag(w_o1, 5), b1, Q1);
                Q0 = mfma_bf16(frag(w_o1, 2), b2, Q0); Q1 = mfma_bf16(frag(w_o1, 6), b2, Q1);
                Q0 = mfma_bf16(frag(w_o1, 3), b3, Q0); Q1 = mfma_bf16(frag(w_o1, 7), b3, Q1);
            } else if constexpr (X3) {
                // B operands: lane (pixel p, half g) supplies k slots e = 0..7 of chunk kc = registers 8 (kc & 1) + e of P0 (kc < 2) / P1.
                // The split of chunk kc+1 (~60 vector instructions) is interleaved with the 12 MFMAs of chunk kc: a bf16 MFMA leaves
                // about six vector-issue slots free inside the issuing wave (tools/mfma_bf16_coissue.hip).
                u32x4 bh[4], bm[4], bl[4];
                auto split = [&](auto kcc) {
                    constexpr int kc = decltype(kcc)::value;
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        constexpr int r0 = 8 * (kc & 1);
                        const float x0 = kc < 2 ? P0[r0 + 2 * d] : P1[r0 + 2 * d], x1 = kc < 2 ? P0[r0 + 2 * d + 1] : P1[r0 + 2 * d + 1];
                        unsigned th, tm, tl;
                        split_pair(x0, x1, th, tm, tl);
                        bh[kc][d] = th; bm[kc][d] = tm; bl[kc][d] = tl;
                    }
                };
                const float *wx = lds + L_WO1 + lane * 4;
                auto A = [&](int t, int cb, int kc) { return __builtin_bit_cast(u32x4, ld4(wx + ((t * 2 + cb) * 4 + kc) * 256)); };
                split(std::integral_constant<int, 0>{});
                unroll<4>([&](auto kcc) {
                    constexpr int kc = decltype(kcc)::value;
                    const u32x4 ah0 = A(0, 0, kc), ah1 = A(0, 1, kc), am0 = A(1, 0, kc), am1 = A(1, 1, kc), al0 = A(2, 0, kc), al1 = A(2, 1, kc);
                    if constexpr (kc < 3) split(std::integral_constant<int, kc + 1>{});
                    Q0 = mfma_bf16(al0, bh[kc], Q0); Q1 = mfma_bf16(al1, bh[kc], Q1);      // small terms first
                    Q0 = mfma_bf16(ah0, bl[kc], Q0); Q1 = mfma_bf16(ah1, bl[kc], Q1);
                    Q0 = mfma_bf16(am0, bm[kc], Q0); Q1 = mfma_bf16(am1, bm[kc], Q1);
                    Q0 = mfma_bf16(am0, bh[kc], Q0); Q1 = mfma_bf16(am1, bh[kc], Q1);
                    Q0 = mfma_bf16(ah0, bm[kc], Q0); Q1 = mfma_bf16(ah1, bm[kc], Q1);
                    Q0 = mfma_bf16(ah0, bh[kc], Q0); Q1 = mfma_bf16(ah1, bh[kc], Q1);
                    if constexpr (kc < 3) {
#pragma unroll
                        for (int i = 0; i < 12; ++i) {
                            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // one MFMA
                            __builtin_amdgcn_sched_group_barrier(0x002, 5, 0);   // five vector instructions of the next chunk's split
                        }
                    }
                });
            } else {
                chain_32to64_lds(w_o1, lane, P0, Q0, Q1);
                chain_32to64_lds(w_o1 + 2 * 4 * 64 * 4, lane, P1, Q0, Q1);
            }
            relu16(Q0);
            relu16(Q1);
            UKBB_HS(hs_j[2], hs_p)
#ifdef UKBB_DIAG
            if (a.diag & 4) { if (a.pred) a.pred[q] = (int)(Q0[0] + Q1[0]); continue; }   // ablation: no logits / softmax VALU
#endif
            // ---- logits / softmax / argmax ----
            // Packed over channel pairs (weights and activations are both consecutive registers), so
            // each class costs 16 v_pk_fma_f32 + 1 add and no operand shuffling.
            float lg[NCLS];
#pragma unroll
            for (int c = 0; c < NCLS; ++c) {
                const float *wp = w_lg + (g * NCLS + c) * 32;
                f32x2 acc2 = {0.f, 0.f};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f32x4 w = ld4(wp + 4 * j);
                    acc2 = pk_fma(f32x2{w[0], w[1]}, f32x2{Q0[4 * j], Q0[4 * j + 1]}, acc2);
                    acc2 = pk_fma(f32x2{w[2], w[3]}, f32x2{Q0[4 * j + 2], Q0[4 * j + 3]}, acc2);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f32x4 w = ld4(wp + 16 + 4 * j);
                    acc2 = pk_fma(f32x2{w[0], w[1]}, f32x2{Q1[4 * j], Q1[4 * j + 1]}, acc2);
                    acc2 = pk_fma(f32x2{w[2], w[3]}, f32x2{Q1[4 * j + 2], Q1[4 * j + 3]}, acc2);
                }
                const float acc = acc2[0] + acc2[1];
                const float other = __shfl_xor(acc, 32);
                lg[c] = (g == 0 ? acc + other : other + acc) + lds[L_BLG + c];
            }
            if (g == 0) {
                if (a.logits) {
#pragma unroll
                    for (int c = 0; c < NCLS; ++c) a.logits[q * NCLS + c] = lg[c];
                }
                float pr[NCLS];
                const int best = softmax_argmax_opt<NCLS>(lg, a.prob != nullptr, pr);
                if (a.pred) a.pred[q] = best;
                if (a.prob) {
#pragma unroll
                    for (int c = 0; c < NCLS; ++c) a.prob[q * NCLS + c] = pr[c];
                }
            }
            UKBB_HS(hs_j[3], hs_p)
        }
#ifdef UKBB_DIAG
        if (lane == 0 && (a.diag & 64)) {
            atomicAdd(g_hstamps + 0, hs_a); atomicAdd(g_hstamps + 1, hs_r); atomicAdd(g_hstamps + 2, hs_b);
            atomicAdd(g_hstamps + 3, __builtin_amdgcn_s_memtime() - hs_t0); atomicAdd(g_hstamps + 4, (unsigned long long)nstages);
#pragma unroll
            for (int j = 0; j < 4; ++j) atomicAdd(g_hstamps + 5 + j, hs_j[j]);
        }
#endif
    }
}

static std::atomic<int> g_head_tail_form{-1};
int head_tail_form() { return g_head_tail_form.load(std::memory_order_relaxed); }

template <int NC>
static hipError_t launch_head_pc_nc(const HeadArgs &a, dim3 grid, hipStream_t s) {
    static const bool dg = [] { const char *e = getenv("UKBB_HEAD_DIRECT_GATHER"); return e && atoi(e) != 0; }();   // A/B knob (r08)
    static const bool inline_tail = [] { const char *e = getenv("UKBB_HEAD_INLINE_TAIL"); return e && atoi(e) != 0; }();   // A/B knob (r11)
#define UKBB_HEAD_GO(X3, DG, IT, BYTES) launch_lds<fcn_head_pc_kernel<NC, X3, DG, IT>>(grid, dim3(768), BYTES, s, a)
#define UKBB_HEAD_GO_BF(DG, IT, BYTES) launch_lds<fcn_head_pc_kernel<NC, false, DG, IT, true>>(grid, dim3(768), BYTES, s, a)
    if (a.x3 && a.conv0_bf16) return hipErrorInvalidValue;      // no such instance (include/ukbb_fcn.h: the modes are not combined)
    if (a.mm_bf16) {                                    // UKBB_PREC_BF16_FULL: one form (separable gather, in-stage tail); the two knobs do not apply
        if (a.x3 || !a.conv0_bf16 || !a.w_s0bf || !a.w_o0bf || !a.w_o1bf) return hipErrorInvalidValue;
        g_head_tail_form.store(1, std::memory_order_relaxed);
        return launch_lds<fcn_head_pc_kernel<NC, false, false, true, true, true>>(grid, dim3(768), HEADPC_BM_LDS_FLOATS * 4, s, a);
    }
    if (a.x3 && a.w_o1x3 && a.w_o0x3) {                 // UKBB_PREC_F32X3; its tail stays in the stage (profiles/r11_notes.md)
        constexpr int ldsx = HEADPC_X3_LDS_FLOATS * 4;
        g_head_tail_form.store(1, std::memory_order_relaxed);
        return dg ? UKBB_HEAD_GO(true, true, true, ldsx) : UKBB_HEAD_GO(true, false, true, ldsx);
    }
    constexpr int lds = HEADPC_LDS_FLOATS * 4;
    bool it = inline_tail;
#ifdef UKBB_DIAG
    if (a.diag & 6) it = true;                          // ablation bits 2 and 4 exist in the in-stage loop only
#endif
    g_head_tail_form.store(dg || it ? 1 : 0, std::memory_order_relaxed);
    if (a.conv0_bf16) {                                 // UKBB_PREC_BF16_STORE: the same three forms behind a bf16 load
        if (dg) return UKBB_HEAD_GO_BF(true, true, lds);
        return it ? UKBB_HEAD_GO_BF(false, true, lds) : UKBB_HEAD_GO_BF(false, false, lds);
    }
    if (dg) return UKBB_HEAD_GO(false, true, true, lds);
    return it ? UKBB_HEAD_GO(false, false, true, lds) : UKBB_HEAD_GO(false, false, false, lds);
#undef UKBB_HEAD_GO
#undef UKBB_HEAD_GO_BF
}

static hipError_t launch_head_pc(const HeadArgs &a, hipStream_t s) {
    const int n_cu = device_cu_count();
    const int ntiles = a.N * (a.H / HT) * (a.W / HT);
    dim3 grid((unsigned)(ntiles < n_cu ? ntiles : n_cu));
    switch (a.n_class) {
        case 2: return launch_head_pc_nc<2>(a, grid, s);
        case 3: return launch_head_pc_nc<3>(a, grid, s);
        case 4: return launch_head_pc_nc<4>(a, grid, s);
        case 5: return launch_head_pc_nc<5>(a, grid, s);
        case 6: return launch_head_pc_nc<6>(a, grid, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_head(const HeadArgs &a_in, hipStream_t s) {
    HeadArgs a = a_in;
#ifdef UKBB_DIAG
    { const char *e = getenv("UKBB_HEAD_DIAG"); a.diag = e ? atoi(e) : 0; }
#endif
    if ((a.H % HT) || (a.W % HT)) return hipErrorInvalidValue;
#ifdef UKBB_DIAG
    if (getenv("UKBB_HEAD_STAMPS")) {        // the 6th stamped launch reports the MFMA waves' stage budget
        static int shots = 0;
        unsigned long long z[16] = {0};
        a.diag |= 64;
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_hstamps), z, sizeof(z));
        const hipError_t e = launch_head_pc(a, s);
        (void)hipStreamSynchronize(s);
        if (++shots == 6) {
            unsigned long long h[16];
            (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_hstamps), sizeof(h));
            const double st = (double)h[4];
            if (st > 0) fprintf(stderr, "[head stamps] per MFMA wave and stage (32-pixel block): wait at barrier A (hand-off) %.0f, read of the handed tile %.0f, wait at barrier B %.0f, "
                                        "MFMA chain + own vector work %.0f; total %.0f cycles\n", h[0] / st, h[1] / st, h[2] / st, (h[3] - h[0] - h[1] - h[2]) / st, h[3] / st);
            // in-stage tail: the four joints of the chain.  Deferred tail (the default of the fp32 separable instance): the first two hold the
            // previous block's logits and store, the third this block's first logits half, the fourth is empty
            if (st > 0) fprintf(stderr, "[head stamps] of it: same_dim0 + ReLU %.0f, out0 + ReLU %.0f, out1 + ReLU %.0f, logits to store %.0f; outside the stamps "
                                        "(prologue, prefetch issue, flush) %.0f\n", h[5] / st, h[6] / st, h[7] / st, h[8] / st,
                                (h[3] - h[0] - h[1] - h[2] - h[5] - h[6] - h[7] - h[8]) / st);
        }
        return e;
    }
#endif
    return launch_head_pc(a, s);
}

// ---------------------------------------------------------------------------
// U-Net logits: 1x1 conv C -> n_class + bias, softmax / argmax
// (reference common/network_ao.py:63,159-160).  C = 16: 48 MAC per pixel,
// bandwidth-bound; one thread per pixel on the vector ALU.
// ---------------------------------------------------------------------------
template <int C, int NCLS, bool IBF = false>
__global__ __launch_bounds__(256) void logits_kernel(const LogitsArgs a) {
    __shared__ float wl[C * NCLS + NCLS];
    for (int i = threadIdx.x; i < C * NCLS; i += 256) wl[i] = a.w[i];
    for (int i = threadIdx.x; i < NCLS; i += 256) wl[C * NCLS + i] = a.bias[i];
    __syncthreads();
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < a.npix; q += (int64_t)gridDim.x * 256) {
        float xin[C];
        if constexpr (IBF) {                                  // bf16 -> f32 is a 16-bit shift
            const unsigned short *ib = reinterpret_cast<const unsigned short *>(a.in) + q * C;
#pragma unroll
            for (int j = 0; j < C / 8; ++j) {
                const uint4 v = *reinterpret_cast<const uint4 *>(ib + 8 * j);
                const unsigned u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    xin[8 * j + 2 * k] = __builtin_bit_cast(float, u[k] << 16);
                    xin[8 * j + 2 * k + 1] = __builtin_bit_cast(float, u[k] & 0xffff0000u);
                }
            }
        } else {
#pragma unroll
        for (int j = 0; j < C / 4; ++j) {
            const float4 v = *reinterpret_cast<const float4 *>(a.in + q * C + 4 * j);
            xin[4 * j] = v.x; xin[4 * j + 1] = v.y; xin[4 * j + 2] = v.z; xin[4 * j + 3] = v.w;
        }
        }
        float lg[NCLS];
#pragma unroll
        for (int c = 0; c < NCLS; ++c) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < C; ++k) s = fmaf(xin[k], wl[k * NCLS + c], s);
            lg[c] = s + wl[C * NCLS + c];
        }
        if (a.logits) {
#pragma unroll
            for (int c = 0; c < NCLS; ++c) a.logits[q * NCLS + c] = lg[c];
        }
        float pr[NCLS];
        const int best = softmax_argmax_opt<NCLS>(lg, a.prob != nullptr, pr);
        if (a.pred) a.pred[q] = best;
        if (a.prob) {
#pragma unroll
            for (int c = 0; c < NCLS; ++c) a.prob[q * NCLS + c] = pr[c];
        }
    }
}

hipError_t launch_logits(const LogitsArgs &a, hipStream_t s) {
    unsigned grid = (unsigned)((a.npix + 255) / 256);
    if (grid > 256u * 16u) grid = 256u * 16u;
    if (a.in_bf16) {
        if (a.C == 16 && a.n_class == 3) hipLaunchKernelGGL((logits_kernel<16, 3, true>), dim3(grid), dim3(256), 0, s, a);
        else if (a.C == 16 && a.n_class == 2) hipLaunchKernelGGL((logits_kernel<16, 2, true>), dim3(grid), dim3(256), 0, s, a);
        else if (a.C == 16 && a.n_class == 4) hipLaunchKernelGGL((logits_kernel<16, 4, true>), dim3(grid), dim3(256), 0, s, a);
        else return hipErrorInvalidValue;
        return hipGetLastError();
    }
    if (a.C == 16 && a.n_class == 3) hipLaunchKernelGGL((logits_kernel<16, 3>), dim3(grid), dim3(256), 0, s, a);
    else if (a.C == 16 && a.n_class == 2) hipLaunchKernelGGL((logits_kernel<16, 2>), dim3(grid), dim3(256), 0, s, a);
    else if (a.C == 16 && a.n_class == 4) hipLaunchKernelGGL((logits_kernel<16, 4>), dim3(grid), dim3(256), 0, s, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace ukbb
