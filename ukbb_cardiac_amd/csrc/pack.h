// Host-side weight packers: every kernel reads its weights in a lane order that one of these functions produces when a plan is bound
// (engine.cpp ensure_packed*, ukbb_fcn_create).  Plain host arithmetic on the standard library alone -- no HIP header, so a plain C++
// compiler builds pack.cpp and tools/pack_digest.cpp pins every layout byte for byte on a CPU (tests/test_pack.py, which also keeps
// packers and private host roundings out of the kernel files).  The layout comments in pack.cpp are the specification of each layout.
// The kernel files include this header only for the layout helpers a packer shares with its kernel (rowmap, WKC, NK).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace ukbb {

// Layout helpers shared with the kernels.
// FCN head (kernels_head.hip): row of a 32x32 f32 MFMA result held in register r by lane half g
constexpr int rowmap(int r, int g) { return (r & 3) + 8 * (r >> 2) + 4 * g; }
// Winograd kernels (kernels_wino.hip, kernels_wino24.hip)
constexpr int WKC = 16;                               // input channels per stage
constexpr int NK = 24;                                // F(2x4) GEMM positions: k = 6 i + j, i = row position 0..3, j = column position 0..5

uint16_t bf16_rne(float f);         // round to nearest, ties to even; a NaN stays a NaN
float bf16_to_f32(uint16_t b);

// Host-side: pack folded weights W[ks][ks][Cin][Cout] into A-fragment order
// for tiling (mb, kc) and workgroups of ncbl = wm*cb Cout blocks.  Returns floats written.
size_t pack_conv_weights(const float *w, int ks, int cin, int cout, int mb, int kc, int ncbl, float *dst);
// bf16 operand variant (packs_bf16): 8 bf16 per lane per tap, returns dwords written.
size_t pack_conv_weights_bf16(const float *w, int ks, int cin, int cout, int ncbl, float *dst);
// three-piece variant (ConvFamily::F32x3Operands, 3x3 only): per chunk the bf16 pieces h, m, l of the bf16 layout above, residuals formed in
// fp32 (as pack_head_x3); returns dwords written (3 x the bf16 packing)
size_t pack_conv_x3(const float *w, int cin, int cout, int ncbl, float *dst);
int wst_pack_order(int cout, int v);    // transposed-conv tilings (ids 410-, ks 2): source column of packed virtual channel v

// Winograd convs (kernels_wino.hip, kernels_wino24.hip, the fused first layer of kernels_conv.hip)
size_t pack_wino_weights(const float *w /*[3][3][cin][cout] folded*/, int cin, int cout, int ncb, float *dst /*16*cin*cout*/);
size_t pack_wino_first_weights(const float *w /*[3][3][16][16] folded*/, float *dst /*16*16*16*/);
size_t pack_wino24_weights(const float *w /*[3][3][cin][cout] folded*/, int cin, int cout, int ncb, float *dst /*24*cin*cout*/);

// gate filter rows [3][3][cin_total][64] (HWIO, channels i | j | f | o x 16 hidden) -> packed F(2x4) A fragments of the input-channel slice
// [c_first, c_first + 16) with the output channels permuted so that MFMA row 4 g + e of 16-channel block w is gate e of hidden channel
// 4 w + g; `bias_perm` (optional, 64) receives the bias in the same order.  Returns floats written to dst (24 * 16 * 64).
size_t pack_lstm_gate_weights(const float *w, int cin_total, int c_first, const float *bias, float *dst, float *bias_perm);
// bf16 form (kernels_ws.hip, ws_main LS): its own lane-native layouts and packing
size_t pack_lstm_gate_weights_bf16(const float *w, int cin_total, int c_first, const float *bias, float *dst /*9 * 16 * 64 / 2 dwords*/, float *bias_perm);
// r06, ls_mode 3 (a time step with the x half NOT hoisted: in0 = feature frames through ls_gx_map, in1 = previous hidden maps through in0_map, bias = the
// permuted gate bias, no gx): the whole [3][3][32][64] gate kernel as one two-chunk filter
size_t pack_lstm_gate_weights_bf16_xh(const float *w /*[3][3][32][64]*/, const float *bias, float *dst /*9 * 32 * 64 / 2 dwords*/, float *bias_perm);

// FCN head (kernels_head.hip)
void pack_sq(const float *w /*[cin][32] folded*/, int cin, float *dst /*cin*32*/);
void pack_rowmap_32x64(const float *w /*32 rows x 64 cols*/, int ld, float *dst /*2*4*64*4*/);
void pack_head_lg(const float *w /*[64][n_class]*/, int n_class, float *dst /*2*n_class*32*/);
void pack_head_x3(const float *w /*[k_in][64 out]*/, int k_in /*32 | 64*/, float *dst /*3*2*(k_in/16)*64*4 dwords*/);
// UKBB_PREC_BF16_FULL: W rounded to bf16 (RNE) once, as A fragments of mfma_bf16.  acc_k 0: k in the order of the stored conv0 block (same_dim0);
// 1: k in the order an accumulator tile's registers supply it (out0, out1)
void pack_head_bf16(const float *w /*[k_in][n_out]*/, int k_in /*16 | 32 | 64*/, int n_out /*32 | 64*/, int acc_k, float *dst /*(n_out/32)*(k_in/16)*64*4 dwords*/);

// conv2d_transpose 3x3 stride 2 'SAME' (network.py:28-34 via network_ao.py:49) is run by
// conv_mfma_kernel as a 2x2-tap stride-1 conv over the INPUT grid with 4*Cout output channels
// (phase-major: (py,px,co)) and ConvArgs::up2 = Cout.  This builds that dense filter
// [2][2][Cin][4*Cout] from the folded transposed filter w[3][3][Cin][Cout] (already re-laid
// out as HWIO by the engine):  out[2m+py] = sum_a x[m+a-1] * w[kh(py,a)],
//   py = 0: a=0 -> kh=2, a=1 -> kh=0 ;  py = 1: a=1 -> kh=1 (a=0: no tap).
void tconv_as_conv2x2(const float *w, int cin, int cout, float *dst);
// fused tail (kernels_tail.hip) and stem (kernels_stem.hip) of the bf16 U-Net
void pack_tail_weights(const float *w0 /*[3][3][32][16] folded*/, const float *w1 /*[3][3][16][16] folded*/, float *dst0 /*9*64*4*/, float *dst1 /*5*64*4*/);
void pack_stem_weights(const float *w0 /*[3][3][1][16] folded*/, float *dst0 /*64*4*/);

// 3-D convolutions of the Temporal-UNet (kernels_conv3d.hip, kernels_conv3d_bf16.hip)
void pack_conv3d_weights(const float *w /*[ntap][cin][cout]*/, int ntap, int cin, int cout, int cout_pad, float *dst);
void pack_conv3d_weights_bf16(const float *w /*[ntap][cin][cout]*/, int ntap, int cin, int cout, int cout_pad, float *dst /*ntap * cin * cout_pad / 2 dwords*/);

}  // namespace ukbb
