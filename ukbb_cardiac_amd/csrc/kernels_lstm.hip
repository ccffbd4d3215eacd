// BiConvLSTM head of the aortic UNet-LSTM model (reference common/network_ao.py:255-319 with
// tf.contrib.rnn.Conv2DLSTMCell semantics, SURVEY.md App. B.6 [TF-recall]).
//
// r05: the gate convolution AND the cell update run in one kernel (kernels_wino24.hip, ConvArgs::ls_mode): the x half of the gate
// conv (W_x * x_t + b, the same for every window a frame is part of) is evaluated once per frame and direction, each time step
// then convolves the 16 hidden channels only and forms  c' = sigmoid(f + 1) * c + sigmoid(i) * tanh(j);  h' = tanh(c') * sigmoid(o)
// in the epilogue -- the 64-channel gate map never exists in HBM.  What is left for this file:
//   lstm_out_kernel   prob / pred / logits of one time step from the two directions' hidden maps: the 1x1 output conv over
//                     concat([h_fw, h_bw]) + bias, softmax, argmax (network_ao.py:305-312, 396-397);
//   lstm_tile_kernel  the same per (window, step) and, fused behind it, the weighted circular tiling of
//                     deploy_network_ao.py:176-183 in the reference's accumulation order and arithmetic (float32 accumulator
//                     updated through float64) -- the per-window probabilities are never stored.
#include "kernels.h"
#include "device_prims.h"

namespace ukbb {

namespace {

constexpr int NH = 16;                       // hidden channels (train_network_ao.py num_hidden = 16)

// 16 hidden channels of one pixel, fp32 or bf16 in memory
template <bool BF>
__device__ __forceinline__ void load_h16(const float *base, long long elem, float (&v)[NH]) {
    if constexpr (BF) {
        const u32x4 *p = reinterpret_cast<const u32x4 *>(reinterpret_cast<const unsigned short *>(base) + elem);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const u32x4 d = p[q];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const unsigned w = d[i];
                v[8 * q + 2 * i] = __builtin_bit_cast(float, w << 16);
                v[8 * q + 2 * i + 1] = __builtin_bit_cast(float, w & 0xffff0000u);
            }
        }
    } else {
#pragma unroll
        for (int q = 0; q < NH / 4; ++q) {
            const f32x4 d = *reinterpret_cast<const f32x4 *>(base + elem + 4 * q);
#pragma unroll
            for (int i = 0; i < 4; ++i) v[4 * q + i] = d[i];
        }
    }
}

// logits of one pixel: W[0:16] . h_fw + W[16:32] . h_bw + b (each direction's sum formed on its own, ascending hidden channel)
template <int NCLS>
__device__ __forceinline__ void out_conv(const float (&vf)[NH], const float (&vb)[NH], const float (&w)[2 * NH][NCLS], const float (&b)[NCLS], float (&lg)[NCLS]) {
    float pf[NCLS], pb[NCLS];
#pragma unroll
    for (int k = 0; k < NCLS; ++k) { pf[k] = 0.f; pb[k] = 0.f; }
#pragma unroll
    for (int i = 0; i < NH; ++i)
#pragma unroll
        for (int k = 0; k < NCLS; ++k) { pf[k] = fmaf(vf[i], w[i][k], pf[k]); pb[k] = fmaf(vb[i], w[NH + i][k], pb[k]); }
#pragma unroll
    for (int k = 0; k < NCLS; ++k) lg[k] = (pf[k] + pb[k]) + b[k];
}

template <int NCLS>
__device__ __forceinline__ void load_out_weights(const float *w_out, const float *b_out, float (&w)[2 * NH][NCLS], float (&b)[NCLS]) {
#pragma unroll
    for (int i = 0; i < 2 * NH; ++i)
#pragma unroll
        for (int k = 0; k < NCLS; ++k) w[i][k] = w_out[i * NCLS + k];
#pragma unroll
    for (int k = 0; k < NCLS; ++k) b[k] = b_out[k];
}

// one thread = one pixel of one window
template <int NCLS, bool BF>
__global__ __launch_bounds__(256) void lstm_out_kernel(const LstmOutArgs a) {
    float w[2 * NH][NCLS], b[NCLS];
    load_out_weights<NCLS>(a.w_out, a.b_out, w, b);
    const long long total = (long long)a.M * a.HW;
    for (long long id = (long long)blockIdx.x * 256 + threadIdx.x; id < total; id += (long long)gridDim.x * 256) {
        const long long m = id / a.HW, pix = id - m * a.HW;
        const long long mf = a.mapf ? a.mapf[m] : m, mb = a.mapb ? a.mapb[m] : m;
        float lg[NCLS], pr[NCLS], vf[NH], vb[NH];
        load_h16<BF>(a.hf, (mf * a.HW + pix) * NH, vf);
        load_h16<BF>(a.hb, (mb * a.HW + pix) * NH, vb);
        out_conv<NCLS>(vf, vb, w, b, lg);
        const int best = softmax_argmax<NCLS>(lg, pr);
        float *po = a.prob + m * a.m_stride + pix * NCLS;
#pragma unroll
        for (int k = 0; k < NCLS; ++k) po[k] = pr[k];
        if (a.logits) {
            float *lo = a.logits + m * a.m_stride + pix * NCLS;
#pragma unroll
            for (int k = 0; k < NCLS; ++k) lo[k] = lg[k];
        }
        if (a.pred) a.pred[m * (a.m_stride / NCLS) + pix] = best;
    }
}

// prob / pred of a cine (kernels.h cine_tile_pixel): a term is
//   prob(w, k) = softmax(out_conv(h_fw[k][w], h_bw[k][w])) exactly as lstm_out_kernel forms it (forward_seq of that window).
// CHUNKED: the launch of one chunk of windows [w0, w1) of a cine that runs in chunks; every (frame, pixel) belongs to one lane per launch
// (no atomics).  Not CHUNKED: the whole cine in one launch.
template <int NCLS, bool BF, bool CHUNKED>
__global__ __launch_bounds__(256) void lstm_tile_kernel(const LstmTileArgs a) {
    float w[2 * NH][NCLS], b[NCLS];
    load_out_weights<NCLS>(a.w_out, a.b_out, w, b);
    const int K = a.tb.K;
    const long long total = (long long)a.tb.F * a.HW;
    for (long long id = (long long)blockIdx.x * 256 + threadIdx.x; id < total; id += (long long)gridDim.x * 256) {
        const int f = (int)(id / a.HW);
        const long long pix = id - (long long)f * a.HW;
        cine_tile_pixel<NCLS, CHUNKED>(a.tb, f, a.w0, a.w1, a.first, a.last, a.prob, a.pred, id, [&](int wi, int k, float (&p)[NCLS]) {
            const int wl = CHUNKED ? wi - a.w0 : wi;
            // the first step of a direction comes from the per-FRAME maps of the x pass, later steps from that direction's per-window maps
            const long long mf = k == 0 ? a.map_first[wl] : wl, mb = k == K - 1 ? a.map_last[wl] : wl;
            float lg[NCLS], vf[NH], vb[NH];
            load_h16<BF>(k == 0 ? a.h1f : a.hf, (k == 0 ? 0 : (long long)k * a.k_stride) + (mf * a.HW + pix) * NH, vf);
            load_h16<BF>(k == K - 1 ? a.h1b : a.hb, (k == K - 1 ? 0 : (long long)k * a.k_stride) + (mb * a.HW + pix) * NH, vb);
            out_conv<NCLS>(vf, vb, w, b, lg);
            (void)softmax_argmax<NCLS>(lg, p);
        });
    }
}

}  // namespace

hipError_t launch_lstm_out(const LstmOutArgs &a, hipStream_t s) {
    const long long total = (long long)a.M * a.HW;
    long long blocks = (total + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    const dim3 g((unsigned)blocks), t(256);
    const bool ok = with_classes(a.n_class, [&](auto nc) {
        constexpr int C = decltype(nc)::value;
        if (a.h_bf16) hipLaunchKernelGGL((lstm_out_kernel<C, true>), g, t, 0, s, a);
        else hipLaunchKernelGGL((lstm_out_kernel<C, false>), g, t, 0, s, a);
    });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_lstm_tile(const LstmTileArgs &a, hipStream_t s) {
    if (a.w0 < 0 || a.w1 <= a.w0 || a.Wn != a.w1 - a.w0) return hipErrorInvalidValue;
    const long long total = (long long)a.tb.F * a.HW;
    long long blocks = (total + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    const dim3 g((unsigned)blocks), t(256);
    const bool chunked = !(a.first && a.last);
    const bool ok = with_classes(a.C, [&](auto nc) {
        constexpr int C = decltype(nc)::value;
        if (a.h_bf16 && chunked) hipLaunchKernelGGL((lstm_tile_kernel<C, true, true>), g, t, 0, s, a);
        else if (a.h_bf16) hipLaunchKernelGGL((lstm_tile_kernel<C, true, false>), g, t, 0, s, a);
        else if (chunked) hipLaunchKernelGGL((lstm_tile_kernel<C, false, true>), g, t, 0, s, a);
        else hipLaunchKernelGGL((lstm_tile_kernel<C, false, false>), g, t, 0, s, a);
    });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace ukbb
