// Internal interface between the engine (plan.cpp: which kernels and tilings; engine.cpp: packing and launches) and the gfx950 kernels.
// Not part of the public ABI (that is include/ukbb_fcn.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_state.h"

namespace ukbb {

// ---- per-device launch state (device_state.h) on top of the HIP runtime ------------------------------------------------
inline int current_device() { int d = 0; return hipGetDevice(&d) == hipSuccess ? d : -1; }
// compute units of the CURRENT device (sizes the persistent grids); 256 if the query fails
inline int device_cu_count() {
    static PerDeviceInt cu;
    const int d = current_device();
    return cu.get(d, [d] { hipDeviceProp_t p; return d >= 0 && hipGetDeviceProperties(&p, d) == hipSuccess ? p.multiProcessorCount : 0; }, 256);
}
// grant `kernel` `bytes` of dynamic LDS on the CURRENT device, once per device.  The internal step of launch_lds(): nothing else calls it
inline hipError_t allow_dynamic_lds(OncePerDevice &once, const void *kernel, int bytes) {
    return (hipError_t)once.run(current_device(), [&] {
        return (int)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes); });
}
// Launch `Kernel` with `lds_bytes` of dynamic LDS.  A kernel that uses more than 64 KB must be granted it on every device it runs on;
// the static that records the grant lives in this template, so every kernel instantiation owns its own by construction.  Every launch
// with dynamic LDS goes through here, and no launcher declares a OncePerDevice of its own.
// GRANT: the bytes to grant where one kernel is launched with several sizes (its largest, the same at every site); 0 = lds_bytes.
template <auto Kernel, int GRANT = 0, class... Args>
hipError_t launch_lds(dim3 grid, dim3 block, int lds_bytes, hipStream_t s, const Args &...args) {
    static OncePerDevice granted;
    const hipError_t e = allow_dynamic_lds(granted, reinterpret_cast<const void *>(Kernel), GRANT ? GRANT : lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(Kernel, grid, block, lds_bytes, s, args...);
    return hipGetLastError();
}

// prob / pred of train_network.py:198-199 (network_ao.py:159-160): prob = softmax(logits), pred = argmax(prob) -- the argmax
// is taken over the float32 PROBABILITIES, lowest index on ties.  It equals argmax(logits) unless another class's logit lies
// within a few ulps of 1.0 (in exp's argument) of the maximum: exp(l - m) then rounds to 1, or the products with 1/sum
// round to the same float, and the lower index wins although its logit is smaller.  Only in that case (rare: |logits| of the
// top two below ~1 and almost equal) the probabilities are formed to decide; the common path costs a subtract and a compare
// per class.  ``p`` (optional) receives the probabilities, formed the same way, so argmax(p) == return value always.
// (r04: callers pass either a real array or the literal nullptr.  Handed `cond ? array : nullptr`, hipcc kept the array in SCRATCH
// memory -- 15-36 scratch instructions in the epilogues of the head / fused-logits kernels, whose reloads sit in the same vmcnt queue
// as the prefetched tiles.  softmax_argmax_opt() below is the call shape for an optional output.)
template <int NCLS>
__device__ __forceinline__ int softmax_argmax(const float (&lg)[NCLS], float *p) {
    int best = 0; float m = lg[0];
#pragma unroll
    for (int c = 1; c < NCLS; ++c) if (lg[c] > m) { m = lg[c]; best = c; }
    bool near = false;
#pragma unroll
    for (int c = 0; c < NCLS; ++c) near |= (c != best) & (m - lg[c] < 4e-7f);
    if (p || near) {
        float e[NCLS]; float sum = 0.f;
#pragma unroll
        for (int c = 0; c < NCLS; ++c) { e[c] = expf(lg[c] - m); sum += e[c]; }
        const float inv = 1.0f / sum;
        float pm = -1.f;
#pragma unroll
        for (int c = 0; c < NCLS; ++c) {
            const float pc = e[c] * inv;
            if (p) p[c] = pc;
            if (pc > pm) { pm = pc; best = c; }
        }
    }
    return best;
}

// pred (and, only if `want_prob`, the probabilities into p) without an escaping conditional pointer: two straight-line instantiations
template <int NCLS>
__device__ __forceinline__ int softmax_argmax_opt(const float (&lg)[NCLS], bool want_prob, float (&p)[NCLS]) {
    if (want_prob) return softmax_argmax<NCLS>(lg, p);
#pragma unroll
    for (int c = 0; c < NCLS; ++c) p[c] = 0.f;
    return softmax_argmax<NCLS>(lg, nullptr);
}

// ---- the weighted circular tiling of deploy_network_ao.py:176-183, one body for the UNet-LSTM and the Temporal-UNet cines ----
struct CineTable {          // the per-cine tables on the device (engine.cpp cine_aux)
    const int *order;       // [F][K] for frame f: the <= K contributing (window w, position k) pairs packed w*K + k, ascending w (the way the
                            //        reference's loop over t adds them), -1 ends the list
    const double *wk;       // [K] window weights
    const double *wsum;     // [F] accumulated weight per frame
    int F, K;
};
// One (frame f, pixel) of prob / pred, element `id` of the [F][HW] maps:
//   prob = (sum over the frame's terms, in list order, of p(window w, position k) * wk[k]) / wsum[f], pred = its lowest-index argmax.
// term(w, k, p) supplies a term's NCLS probabilities.  Reference arithmetic: prob is float32, `prob[..., idx] += prob_idx * w` runs in
// float64 and is cast back per addition; `prob /= weight` likewise.  A frame no window reaches (time_step > window) has wsum = 0:
// 0/0 = NaN and argmax 0, as numpy gives the reference.
// CHUNKED: this launch adds the terms of the windows [w0, w1) only.  A frame's terms come in ascending window order, chunks run in
// ascending order, and the accumulator is rounded to float32 after every term -- so carrying that float32 in prob between chunks performs
// the same sequence of float64-widened adds.  The first chunk starts from 0, the last divides and takes the argmax; a frame the chunk
// does not reach is not touched otherwise.  Not CHUNKED: the whole list in one pass, prob is written only.
template <int NCLS, bool CHUNKED, class Term>
__device__ __forceinline__ void cine_tile_pixel(const CineTable &tb, int f, int w0, int w1, bool first, bool last,
                                                float *prob, int32_t *pred, long long id, Term &&term) {
    float acc[NCLS];
    float *o = prob + id * NCLS;
    bool open = !CHUNKED || first;                                       // acc holds the running sum (else it still lies in prob)
    auto resume = [&] {
        if (!open) {
#pragma unroll
            for (int c = 0; c < NCLS; ++c) acc[c] = o[c];
            open = true;
        }
    };
#pragma unroll
    for (int c = 0; c < NCLS; ++c) acc[c] = 0.f;
    for (int j = 0; j < tb.K; ++j) {
        const int wk_ = tb.order[f * tb.K + j];
        if (wk_ < 0) break;                                              // fewer than K windows reach this frame (time_step > 1, F < K)
        const int wi = wk_ / tb.K, k = wk_ - wi * tb.K;
        if constexpr (CHUNKED) {
            if (wi < w0) continue;                                       // an earlier chunk's window (already added)
            if (wi >= w1) break;                                         // a later chunk's
            resume();
        }
        float p[NCLS];
        term(wi, k, p);
        const double wt = tb.wk[k];
#pragma unroll
        for (int c = 0; c < NCLS; ++c) acc[c] = (float)((double)acc[c] + (double)p[c] * wt);
    }
    if (!CHUNKED || last) {
        if constexpr (CHUNKED) resume();
        const double ws = tb.wsum[f];
        int best = 0;
#pragma unroll
        for (int c = 0; c < NCLS; ++c) acc[c] = (float)((double)acc[c] / ws);
#pragma unroll
        for (int c = 1; c < NCLS; ++c) if (acc[c] > acc[best]) best = c;
        if (pred) pred[id] = best;
    }
    if (!open) return;
#pragma unroll
    for (int c = 0; c < NCLS; ++c) o[c] = acc[c];
}

// ---------------------------------------------------------------------------
// Generic implicit-GEMM convolution (3x3 or 1x1, stride 1 or 2) + bias + ReLU
// on the f32 MFMA pipes.  NHWC activations, weights pre-packed in MFMA
// A-fragment order by pack_conv_weights().
// ---------------------------------------------------------------------------
struct ConvArgs {
    const float *in0;   // first source  [N,H,W,C0]
    const float *in1;   // optional second source [N,H,W,C1] (U-Net skip concat, network_ao.py:51)
    int C0, C1;
    const float *wpk;   // packed A fragments
    const float *bias;  // [Cout] folded BN shift (or conv bias)
    float *out;         // [N,Ho,Wo,Cout]
    int N, H, W;        // input spatial size
    int Ho, Wo, Cout;
    int pad_y, pad_x;   // TF 'SAME' pad_before (oracle/fcn_oracle.py same_pads)
    int tiles_y, tiles_x;
    int relu;
    const float *first_w;   // fused first layer (conv_pc_kernel<..., FIRST>): folded conv0_0 weights [9][KC]
    const float *first_b;   //   and bias [KC]; in0 is then the 1-channel network input [N,H,W]
    int up2;            // 0: plain conv.  C > 0: the 4*C output channels are the 4 sub-pixel phases of a
                        // stride-2 transposed conv with C real channels; scatter to out[N,2Ho,2Wo,C]
    const int *in0_map; // optional (Winograd kernel only): image n of the batch reads in0 image in0_map[n]
                        // (ConvLSTM windows share cached U-Net feature frames); in1 / out are not remapped
    int diag;           // diagnostic builds only (-DUKBB_DIAG, env UKBB_CONV_DIAG): ablation bits of conv_pc_kernel
    // bf16-storage tilings only (ConvFamily::Bf16Store): the 1x1 logits conv + softmax / argmax of network_ao.py:63,159-160 evaluated in the
    // epilogue of the LAST 16-channel conv (out is then not written at all): lg_w [16][lg_ncls], lg_b [lg_ncls]
    const float *lg_w, *lg_b;
    float *lg_logits, *lg_prob;   // optional [N,Ho,Wo,lg_ncls]
    int32_t *lg_pred;             // optional [N,Ho,Wo]
    int lg_ncls;
    int xcd_local;      // kernels_ws.hip only: tile order (set by launch_conv_ws)
    int cout_store;     // bf16-storage tilings (stores_bf16) only: real channel count of `out` when Cout is the zero-padded
                        // count the weights were packed for (a 16-channel layer on the 32-row MFMA); 0 = Cout
    // ---- ConvLSTM cell in the epilogue of the F(2x4) Winograd kernel (kernels_wino24.hip, launch_wino24_lstm; network_ao.py:255-319) ----
    // ls_mode 1 ("x pass", once per call): in0 = the U-Net feature frames [N][H][W][16], Cout = 64 per direction (groups = directions),
    //   filter = the x rows of the gate kernel, bias = the gate bias.  Per frame and direction the epilogue stores gx = W_x * x + b
    //   (ls_gx), and the cell's first step from the zero state: c1 (ls_c_out), h1 (out, [N][H][W][16]).
    // ls_mode 2 (one time step of one direction): in0 = the previous hidden state [N][H][W][16] (image n reads in0_map[n] if given),
    //   Cout = 64, filter = the h rows of the gate kernel, bias = nullptr; gates = W_h * h + gx[ls_gx_map[n]], cell state read from
    //   ls_c_in (entry in0_map[n] if given, else n) and written to ls_c_out[n], h written to out.
    // gx / c live in the consumer lanes' own order ("lane-native": [image][region][wave][tile block][pixel of the 2x4 tile][lane]), the gate
    // channels are packed so that one lane holds i, j, f, o of ONE hidden channel (pack_lstm_gate_weights).
    int ls_mode;
    float *ls_gx;               // mode 1: written; mode 2: read (const in effect)
    const int *ls_gx_map;       // mode 2: frame whose gx window n adds at this step
    const float *ls_c_in;       // mode 2
    float *ls_c_out;
    long long ls_gx_dir, ls_c_dir, ls_h_dir;   // mode 1: floats between the two directions' halves of ls_gx / ls_c_out / out
    float ls_forget_bias;
    int ls_bf16;                // 1: in0, gx and the hidden maps (out) are bf16 in HBM (UKBB_PREC_BF16 on a UNet-LSTM handle); c stays fp32.
                                //    Strides (ls_*_dir) still count ELEMENTS; ls_gx_dir counts gx values (4 per lane-slot)
};

// The kernel family a tiling belongs to: which kernel runs it, in which number formats, from which packed weights.
enum class ConvFamily {
    Direct,         // single-role kernel
    ProdCons,       // producer/consumer persistent kernel (512 threads)
    ProdConsFirst,  // producer/consumer with the C_in = 1 first layer fused into the producers
    Bf16Operands,   // single-role kernel with bf16 operands / fp32 accumulation (mb = 32, kc = 16)
    Wino22,         // Winograd F(2x2,3x3) producer/consumer kernel (kernels_wino.hip): 8 x 16- or 16 x 8-pixel regions
    Wino24,         // Winograd F(2x4,3x3) (kernels_wino24.hip): 8 x 32- or 8 x 16-pixel regions (id 306: 8 x 16 over image pairs; 307: 32-channel items)
    Bf16Store,      // as Bf16Operands with bf16 activations in HBM on both sides (in0 / in1 / out point at bf16 data), CHANNEL-BLOCKED:
                    // [N][C/16][H][W][16] -- a 16-channel K chunk of a row of pixels is one contiguous run of 32-byte pixels
                    // (r04: in plain NHWC a wave's 16-byte pieces of one chunk lay 2 C bytes apart, every piece pulled a whole
                    // 128-byte line out of L2 for 16-32 useful bytes); for C = 16 the two layouts coincide
    Bf16StoreWs,    // bf16 storage as Bf16Store, weight-stationary persistent kernel of independent waves (kernels_ws.hip)
    FirstWino22,    // as ProdConsFirst (fused first layer, fp32), the 16 -> 16 conv as Winograd F(2x2,3x3) in the consumers (id 134;
                    // weights from pack_wino_first_weights)
    F32x3Operands,  // single-role kernel of kernels_conv_x3.hip (ids 330-345): fp32 maps in HBM on both sides, each operand as three bf16 pieces
                    // (activations split while staging, weights when packed: pack_conv_x3), six bf16 MFMAs per (tap, chunk) into the one
                    // fp32 accumulator, fp32 epilogue.  Planned only with PlanMode::conv_x3 (UKBB_PREC_F32X3 + ukbb_fcn_set_f32x3_convs)
};

// One compiled tiling of the conv kernel.
struct ConvConfig {
    int id;
    int ks, stride;     // kernel size (1|3), stride (1|2)
    int mb;             // MFMA M block: 16 -> v_mfma_f32_16x16x4_f32, 32 -> v_mfma_f32_32x32x2_f32
    int th, tw;         // output tile per workgroup
    int kc;             // input channels staged in LDS per pass
    int wm, wn, cb;     // waves along Cout / along pixels; Cout blocks per wave
    int lds_bytes;
    ConvFamily family;
    const char *name;
    int fuse;           // Bf16Store / Bf16StoreWs only: 1 = the C_in = 1 first layer evaluated in this conv's staging (ConvArgs::first_w /
                        // first_b, in0 = the fp32 image), 2 = the logits conv + softmax / argmax in its epilogue (ConvArgs::lg_*); else 0
};

// What follows from a tiling's family, each fact stated once.
inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
inline bool fuses_first(const ConvConfig &c) { return c.family == ConvFamily::ProdConsFirst || c.family == ConvFamily::FirstWino22; }
inline bool stores_bf16(const ConvConfig &c) { return c.family == ConvFamily::Bf16Store || c.family == ConvFamily::Bf16StoreWs; }   // activations bf16 in HBM
inline bool packs_bf16(const ConvConfig &c) { return c.family == ConvFamily::Bf16Operands || stores_bf16(c); }                      // weights packed as bf16
inline bool is_wino24(const ConvConfig &c) { return c.family == ConvFamily::Wino24; }
inline bool is_wino(const ConvConfig &c) { return c.family == ConvFamily::Wino22 || is_wino24(c); }
inline int cout_per_item(const ConvConfig &c) { return is_wino(c) ? 16 * c.wm : c.mb * c.cb * c.wm; }    // output channels of one work item
inline int packed_cout(const ConvConfig &c, int cout) { return stores_bf16(c) ? round_up(cout, 32) : cout; }   // 16-channel layers run zero-padded on the 32-row MFMA
inline int map_tiles(const ConvConfig &c, int Ho, int Wo) { return ((Ho + c.th - 1) / c.th) * ((Wo + c.tw - 1) / c.tw); }   // tiles (regions) of one Ho x Wo map

int num_conv_configs();
const ConvConfig &conv_config(int id);
// the persistent last-layer tilings of the bf16 U-Net (ids 324-325) live in kernels_bf16.hip; the three functions above cover them
int num_pk16_configs();
const ConvConfig &pk16_config(int i);
hipError_t launch_conv16_pk(int cfg_id, const ConvArgs &a, hipStream_t s);
// weight-stationary persistent 3x3 stride-1 tilings of the bf16 U-Net (ids 400-, ConvFamily::Bf16StoreWs: bf16 storage as Bf16Store; th = rows per
// tile, tw = 32, wn = independent waves per workgroup, cb = 32-channel Cout blocks per workgroup) live in kernels_ws.hip; the three
// functions above cover them.  LDS need depends on the layer's input channels (the whole packed filter of a Cout group is resident).
int num_ws_configs();
const ConvConfig &ws_config(int i);
int ws_lds_bytes_for(const ConvConfig &c, int cin);
hipError_t launch_conv_ws(int cfg_id, const ConvArgs &a, hipStream_t s);
// the three-piece (UKBB_PREC_F32X3) 3x3 tilings of ConvFamily::F32x3Operands (ids 330-345) live in kernels_conv_x3.hip; the three functions above
// cover them.  LDS = three times the bf16-operand tiling's
int num_x3_configs();
const ConvConfig &x3_config(int i);
hipError_t launch_conv_x3(int cfg_id, const ConvArgs &a, hipStream_t s);
// cout handled by one workgroup = mb*cb*wm
hipError_t launch_conv(int cfg_id, const ConvArgs &a, hipStream_t s);

// The host-side weight packers (pack_*, tconv_as_conv2x2, wst_pack_order) live in pack.h / pack.cpp, a host-only unit without HIP.

// Winograd F(2x2,3x3) producer/consumer kernel (kernels_wino.hip): 3x3, stride 1, C_out % 64 == 0,
// C_in % 16 == 0.  ConvFamily::Wino22, ids 300-303.  Same ConvArgs; wpk from pack_wino_weights().
// thread-local error string behind ukbb_fcn_last_error() (engine.cpp)
void set_error(const char *fmt, ...);

hipError_t launch_wino(const ConvArgs &a, int ncb /*16-channel blocks per item: 4 or 2*/, int tile_rows /*4: 8x16-pixel regions, 8: 16x8*/,
                       hipStream_t s);
int wino_lds_bytes();
// Winograd F(2x4,3x3) (kernels_wino24.hip): 64-channel output groups, 8 x 32- or 8 x 16-pixel regions, ConvFamily::Wino24, ids 304 / 305 / 306 / 307 (306: 8 x 16 over image pairs; 307: 32-channel items)
hipError_t launch_wino24(const ConvArgs &a, int tile_cols /*32 | 16*/, int pair /*id 306: image pairs with seam regions, Ho % 8 == 4*/, int ncb /*4 | 2 (id 307)*/,
                         hipStream_t s);
int wino24_lds_bytes(int tbw, int pair);
// ConvLSTM forms of the same kernel (ConvArgs::ls_mode 1 | 2): tile_cols 32 | 16.  Both region shapes give identical bits.
hipError_t launch_wino24_lstm(const ConvArgs &a, int tile_cols, hipStream_t s);
// floats of the lane-native gx / c buffers per image (frame or window) for maps of Ho x Wo
size_t wino24_lstm_gx_floats(int Ho, int Wo, int tile_cols);
size_t wino24_lstm_c_floats(int Ho, int Wo, int tile_cols);
// bf16 form of the same pair of kernels (kernels_ws.hip, ws_main LS): direct 3x3 conv on v_mfma_f32_32x32x16_bf16 (bf16 hidden maps / features / gx, fp32
// accumulation and cell state), weight-stationary independent waves.  ConvArgs as above with ls_bf16 = 1; its own lane-native layouts and packing
// (pack_lstm_gate_weights_bf16; ls_mode 3, a time step with the x half not hoisted: pack_lstm_gate_weights_bf16_xh)
hipError_t launch_lstm_ws(const ConvArgs &a, hipStream_t s);
size_t lstm_ws_gx_elems(int H, int W);      // bf16 values of gx per image (frame)
size_t lstm_ws_c_floats(int H, int W);      // fp32 values of the cell state per image

// ---------------------------------------------------------------------------
// First layer: conv3x3, C_in = 1 (network.py:186 with l = 0), direct stencil.
// ---------------------------------------------------------------------------
struct FirstArgs {
    const float *in;    // [N,H,W,1]
    const float *w;     // [9][Cout] folded
    const float *bias;  // [Cout]
    float *out;         // [N,H,W,Cout]
    int N, H, W, Cout;
    int out_bf16;       // 1: out holds bf16 (UKBB_PREC_BF16 of the U-Net: every activation between layers is bf16)
};
hipError_t launch_first(const FirstArgs &a, hipStream_t s);

// ---------------------------------------------------------------------------
// FCN head (network.py:201-229 + train_network.py:198-199), see kernels_head.hip.
// sqg: G_l[px][64] = W0_l * relu(BN(Ws_l * conv_l[px]))   at the resolution of level l = 1..4
// head: same_dim0 -> out0 (level-0 slice) + sum_l bilinear-gather(G_l) -> out1 -> logits
//       -> softmax / argmax, at full resolution.
// ---------------------------------------------------------------------------
struct SqgArgs {
    const float *x;          // [npix][cin] level-l features
    const float *w_s;        // pack_sq(same_dim_l)            [cin/8][64][4]
    const float *b_s;        // [32]
    const float *w_g;        // pack_rowmap_32x64(out0 rows 32l..32l+31)
    float *out;              // [npix][64]
    long long npix;
    int cin;
    int x_bf16;              // input format.  0: x is fp32 [npix][cin].  1 (UKBB_PREC_BF16_STORE): x is bf16, channel-blocked [N][cin/16][hw][16]
                             // (ConvFamily::Bf16Store), decoded to fp32 on the way in (exact); everything behind the load is the fp32 launch
    int hw;                  // x_bf16 only: pixels per image (npix = N * hw)
};
hipError_t launch_sqg(const SqgArgs &a, hipStream_t s);
struct SqgMultiArgs { SqgArgs lv[4]; int nb[4]; };   // levels 1..4 (C_in 32, 64, 128, 256) and their virtual grid sizes
hipError_t launch_sqg_multi(const SqgArgs lv[4], hipStream_t s);

struct HeadArgs {
    const float *conv0;      // [N,H,W,16] level-0 features
    const float *G[4];       // projected maps of levels 1..4: [N,H>>l,W>>l,64]
    const float *w_s0;       // pack_sq(same_dim0, 16)
    const float *b_s0;       // [32]
    const float *w_o0;       // pack_rowmap_32x64(out0 rows 0..31)
    const float *b_o0;       // [64]
    const float *w_o1;       // pack_rowmap_32x64(out1 rows 0..31) ++ pack_rowmap_32x64(out1 rows 32..63)
    const float *b_o1;       // [64]
    const float *w_o0x3;     // optional (UKBB_PREC_F32X3): pack_head_x3(out0 rows 0..31, 32) -- three bf16 pieces per weight; may be null
    const float *w_o1x3;     // optional: pack_head_x3(out1, 64)
    const float *w_lg;       // pack_head_lg: [2][n_class][32]
    const float *b_lg;       // [n_class]
    float *logits;           // optional [N,H,W,n_class]
    float *prob;             // optional
    int32_t *pred;           // optional [N,H,W]
    int N, H, W, n_class;
    int x3;                  // UKBB_PREC_F32X3: out0's level-0 slice and out1 from bf16 pieces (needs w_o0x3 / w_o1x3)
    int diag;                // diagnostic builds only (-DUKBB_DIAG, env UKBB_HEAD_DIAG): ablation bits of fcn_head_pc_kernel
    int conv0_bf16;          // input format of conv0.  0: fp32 [N,H,W,16].  1 (UKBB_PREC_BF16_STORE): bf16 [N][1][H][W][16], decoded to fp32 on the
                             // way in (exact); not combined with x3
    int mm_bf16;             // UKBB_PREC_BF16_FULL: same_dim0, out0's level-0 slice and out1 on v_mfma_f32_32x32x16_bf16, one bf16 piece per operand
                             // (needs conv0_bf16 and the three blocks below; not combined with x3)
    const float *w_s0bf;     // pack_head_bf16(same_dim0, 16, 32, natural k): 256 dwords
    const float *w_o0bf;     // pack_head_bf16(out0 rows 0..31, 32, 64, accumulator k): 1024 dwords
    const float *w_o1bf;     // pack_head_bf16(out1, 64, 64, accumulator k): 2048 dwords
};
hipError_t launch_head(const HeadArgs &a, hipStream_t s);
int head_tail_form();      // ukbb_fcn_head_tail_form()

// ---------------------------------------------------------------------------
// U-Net pieces (network_ao.py:48-63)
// ---------------------------------------------------------------------------
// conv2d_transpose 3x3 stride 2 'SAME' (network.py:28-34 via network_ao.py:49) is run by
// conv_mfma_kernel as a 2x2-tap stride-1 conv over the INPUT grid with 4*Cout output channels
// (phase-major: (py,px,co)) and ConvArgs::up2 = Cout; tconv_as_conv2x2 (pack.h) builds that dense filter.

// Fused tail of the bf16 U-Net (kernels_tail.hip): up0_0 -> up0_1 -> logits -> softmax / argmax in one launch (network_ao.py:51-63,159-160)
struct TailArgs {
    const float *in0, *in1;     // bf16 [N][H][W][16]: the level-0 skip map (conv0) and the transposed conv's output (up0_t)
    const float *wA0, *wA1;     // pack_tail_weights(): MFMA A fragments of up0_0 (9 taps) and up0_1 (5 tap pairs)
    const float *b0, *b1;       // folded BN shifts [16]
    const float *lg_w, *lg_b;   // logits conv [16][n_class], [n_class]
    float *logits, *prob;       // optional [N,H,W,n_class]
    int32_t *pred;              // optional [N,H,W]
    int N, H, W, ncls;
    unsigned long long *stamps;  // diagnostic builds only (-DUKBB_DIAG, env UKBB_TAIL_STAMPS): per-wave phase cycle sums
    int seg_tiles;               // strip mode (set by the launcher): tile rows per segment of a column strip; 0 = whole strips
};
hipError_t launch_unet_tail(const TailArgs &a, hipStream_t s);

// Fused stem of the bf16 U-Net (kernels_stem.hip): conv0_0 -> conv0_1 in one launch (network_ao.py:31-35 with l = 0)
struct StemArgs {
    const float *image;         // fp32 [N][H][W]
    const float *wA0, *wA1;     // pack_stem_weights() (conv0_0) and the second output of pack_tail_weights() (conv0_1: 5 tap pairs)
    const float *b0, *b1;       // folded BN shifts [16]
    float *out;                 // bf16 [N][H][W][16]
    int N, H, W;
};
hipError_t launch_unet_stem(const StemArgs &a, hipStream_t s);

struct LogitsArgs {         // 1x1 conv C -> n_class + bias, softmax / argmax (network_ao.py:63,159-160)
    const float *in;        // [N,H,W,C]
    const float *w;         // [C][n_class]
    const float *bias;
    float *logits; float *prob; int32_t *pred;
    int64_t npix; int C, n_class;
    int in_bf16;            // 1: `in` holds bf16
};
hipError_t launch_logits(const LogitsArgs &a, hipStream_t s);

// ---- BiConvLSTM head of the aortic UNet-LSTM (network_ao.py:255-319), kernels_lstm.hip ----
struct LstmOutArgs {        // one time step's outputs from the two directions' hidden maps (1x1 output conv + bias, softmax, argmax)
    const float *hf, *hb;   // [.][HW][NH] hidden maps of the forward / backward cell at this step
    const int *mapf, *mapb; // optional: window m reads entry mapf[m] / mapb[m] (the first step of a direction lives per FRAME)
    const float *w_out;     // [2*NH][n_class] (forward rows first, network_ao.py:305-312)
    const float *b_out;     // [n_class]
    float *prob;            // per (window m, pixel): n_class floats at prob + m*m_stride + pix*n_class
    float *logits;          // optional, same addressing
    int32_t *pred;          // optional: argmax at pred + m*(m_stride/n_class) + pix
    long long m_stride;     // floats between consecutive windows in prob / logits
    int M, HW, n_class;
    int h_bf16;             // 1: hf / hb hold bf16
};
hipError_t launch_lstm_out(const LstmOutArgs &a, hipStream_t s);

struct LstmTileArgs {       // per-(window, step) outputs + the weighted tiling of deploy_network_ao.py:176-183 in one pass
    const float *hf, *hb;   // [K][Wn][HW][NH] hidden maps per step k and window (entry k = 0 of hf / k = K-1 of hb unused, see h1f / h1b)
    const float *h1f, *h1b; // [frames][HW][NH]: the first step of each direction, per frame (the x pass of the fused kernel)
    const int *map_first, *map_last;   // [Wn]: frame of window w at step 0 / at step K-1
    long long k_stride;     // floats between steps in hf / hb
    const float *w_out, *b_out;
    CineTable tb;           // of the whole cine
    float *prob;            // [F][HW][C]
    int32_t *pred;          // [F][HW]
    int Wn, HW, C;
    int h_bf16;             // 1: hf / hb / h1f / h1b hold bf16 (k_stride still counts elements)
    // The windows [w0, w1) of the cine, Wn = w1 - w0: all of them (first = last = 1), or one chunk of a cine that runs in chunks (forward_cine under a
    // scratch budget).  hf / hb / map_first / map_last then hold the CHUNK's windows (index w - w0, k_stride = (w1 - w0) * HW * NH), h1f / h1b the chunk's
    // frame run (map_first / map_last give run-local frames); tb / prob / pred: the whole cine
    int w0, w1;
    int first, last;        // first chunk: start from 0; between chunks prob is the float32 accumulator; last chunk: prob /= weight, argmax
};
hipError_t launch_lstm_tile(const LstmTileArgs &a, hipStream_t s);

// ---- 3-D convolutions of the aortic Temporal-UNet (network_ao.py:67-114), kernels_conv3d.hip ----
struct Conv3dPhase {        // one sub-pixel phase of a transposed conv (the whole conv: one phase at (0, 0))
    const float *wpk;       // packed A fragments (pack_conv3d_weights) of the taps this phase reads
    int py, px;             // output pixel = (up * gy + py, up * gx + px)
    int ny, nx;             // spatial taps along y / x
};
struct Conv3dArgs {         // 3x3x3 conv (+ folded BN + ReLU) over windows of T frames: image n = window * T + t
    const float *in0, *in1; // NHWC sources [N][Hi][Wi][C0] and (skip concat second source, or NULL) [N][Hi][Wi][C1]
    int C0, C1;             // multiples of 8
    const float *bias;      // [Cout]
    float *out;             // [N][Ho][Wo][Cout]
    int N, T, Hi, Wi;
    int Hg, Wg;             // output grid the launch iterates (per phase)
    int Ho, Wo, Cout, Cout_pad;   // stored map; Cout_pad = Cout rounded up to the MFMA's 32 rows
    int stride, up;         // input row = gy * stride + oy + j * jstep; output row = gy * up + py
    int oy, ox, jstep;      // conv: -pad_before, -pad_before, +1; transposed conv: 0, 0, -1
    int relu;
    int nph;                // phases (blockIdx.y): 1 or 4
    Conv3dPhase ph[4];
};
hipError_t launch_conv3d(const Conv3dArgs &a, hipStream_t s);

struct Conv3dFirstArgs {    // first layer, C_in = 1 -> 16, 3x3x3, stride 1 (+ folded BN + ReLU)
    const float *image;     // frames [.][H][W]
    const int *map;         // image n of the batch reads frame map[n] (NULL: frame n)
    const float *w;         // [27][16] folded, taps in (kt, ky, kx) order
    const float *bias;      // [16]
    float *out;             // [N][H][W][16]
    int N, T, H, W;
};
hipError_t launch_conv3d_first(const Conv3dFirstArgs &a, hipStream_t s);

// UKBB_PREC_BF16_3D (kernels_conv3d_bf16.hip): the same launches on v_mfma_f32_32x32x16_bf16.  The argument structs are the fp32 ones with
// every map bf16, channel-blocked [N][C/16][H*W][16] (in0 / in1 / out point at bf16; C0, C1 multiples of 16), wpk the A fragments of
// pack_conv3d_weights_bf16 (the folded kernel rounded once to bf16); bias stays fp32.  The first layer reads the fp32 cine and the
// unrounded fp32 folded weights and stores its 16 channels as bf16.
hipError_t launch_conv3d_bf16(const Conv3dArgs &a, hipStream_t s);
hipError_t launch_conv3d_first_bf16(const Conv3dFirstArgs &a, hipStream_t s);

struct T3dTileArgs {        // weighted circular tiling (deploy_network_ao.py:176-183) of the windows [w0, w1) of a cine
    const float *probw;     // [(w1 - w0) * K][HW][C]: softmax of each window frame
    CineTable tb;           // of the whole cine
    float *prob;            // [F][HW][C]: the accumulator between chunks, the result after the last
    int32_t *pred;          // [F][HW] (last chunk)
    int HW, C, w0, w1;
    int first, last;        // first chunk: start from 0; last chunk: prob /= weight, argmax
};
hipError_t launch_t3d_tile(const T3dTileArgs &a, hipStream_t s);

}  // namespace ukbb
