// Host-side weight packers (pack.h).  Built without contraction (-ffp-contract=off): the Winograd packers accumulate G g G^T in double and
// round once, the three-piece split relies on exact fp32 subtraction.
#include "pack.h"

#include <cstring>
#include <vector>

namespace ukbb {

uint16_t bf16_rne(float f) {
    unsigned u; memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
float bf16_to_f32(uint16_t b) { const unsigned u = (unsigned)b << 16; float f; memcpy(&f, &u, 4); return f; }

// UKBB_PREC_F32X3: piece t of x.  Piece 0 = bf16(x), piece 1 = bf16(x - piece 0), piece 2 = bf16(x - piece 0 - piece 1), the residuals
// formed in fp32 (exact) -- the host form of split_pair (device_prims.h)
static uint16_t x3_piece(float x, int t) {
    uint16_t b = 0;
    for (int k = 0; k <= t; ++k) { b = bf16_rne(x); x -= bf16_to_f32(b); }
    return b;
}

// F(2x2,3x3): U = G g G^T
static const float G22[4][3] = {{1.f, 0.f, 0.f}, {.5f, .5f, .5f}, {.5f, -.5f, .5f}, {0.f, 0.f, 1.f}};

size_t pack_conv_weights(const float *w, int ks, int cin, int cout, int mb, int kc, int ncbl, float *dst) {
    // dst[group][chunk][cbl][tap][lane][s] = W[tap][ci][co],  cb = group*ncbl + cbl
    //   k-step s of lane group g uses channel ci = chunk*kc + g*ksteps + s  (so the B operands
    //   of a lane for all k-steps of a tap are ksteps CONSECUTIVE channels = one LDS vector read)
    //   mb = 32: lane = (g<<5)|m (g < 2), co = cb*32 + m ;  mb = 16: lane = (g<<4)|m (g < 4), co = cb*16 + m
    // One workgroup (= one group of ncbl Cout blocks) reads, per chunk, one contiguous slab.
    const int kk = (mb == 32) ? 2 : 4, ksteps = kc / kk, ks2 = ks * ks, nchunk = cin / kc;
    size_t o = 0;
    for (int grp = 0; grp < cout / (mb * ncbl); ++grp)
        for (int ch = 0; ch < nchunk; ++ch)
            for (int cbl = 0; cbl < ncbl; ++cbl)
                for (int tap = 0; tap < ks2; ++tap)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int m = lane % mb, g = lane / mb;
                        for (int s = 0; s < ksteps; ++s) {
                            const int ci = ch * kc + g * ksteps + s, co = (grp * ncbl + cbl) * mb + m;
                            dst[o++] = w[((size_t)tap * cin + ci) * cout + co];
                        }
                    }
    return o;
}

size_t pack_wino_first_weights(const float *w, float *dst) {
    // w: folded [3][3][16][16] of a 16 -> 16 3x3 conv.  U = G g G^T per (ci, co), G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]] (the +-1/2
    // factors stay in the weights, as in pack_wino_weights).  dst[h][k = 4*xi + nu][lane][s]: the A fragment of k-step s of half h of the
    // Winograd consumers of conv_pc_kernel<..., WINO>: lane = (g << 4) | m, co = m, ci = 4*g + 2*h + s.
    size_t o = 0;
    for (int h = 0; h < 2; ++h)
        for (int k = 0; k < 16; ++k)
            for (int lane = 0; lane < 64; ++lane)
                for (int s = 0; s < 2; ++s) {
                    const int m = lane & 15, g = lane >> 4, ci = 4 * g + 2 * h + s, co = m;
                    const int xi = k >> 2, nu = k & 3;
                    double u = 0.0;                         // exact products of small dyadic factors; one rounding
                    for (int i = 0; i < 3; ++i)
                        for (int j = 0; j < 3; ++j)
                            u += (double)G22[xi][i] * (double)w[((size_t)(i * 3 + j) * 16 + ci) * 16 + co] * (double)G22[nu][j];
                    dst[o++] = (float)u;
                }
    return o;
}

size_t pack_conv_weights_bf16(const float *w, int ks, int cin, int cout, int ncbl, float *dst) {
    // dst[group][chunk][cbl][tap][lane][4 dwords]; dword d of lane (g<<5)|m holds bf16 pair
    //   W[tap][ci = chunk*16 + 8g + 2d (+1)][co = cb*32 + m]   (low half = even channel)
    const int ks2 = ks * ks, nchunk = cin / 16;
    unsigned *out = reinterpret_cast<unsigned *>(dst);
    size_t o = 0;
    for (int grp = 0; grp < cout / (32 * ncbl); ++grp)
        for (int ch = 0; ch < nchunk; ++ch)
            for (int cbl = 0; cbl < ncbl; ++cbl)
                for (int tap = 0; tap < ks2; ++tap)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int m = lane & 31, g = lane >> 5, co = (grp * ncbl + cbl) * 32 + m;
                        for (int d = 0; d < 4; ++d) {
                            const int ci = ch * 16 + 8 * g + 2 * d;
                            const unsigned lo = bf16_rne(w[((size_t)tap * cin + ci) * cout + co]);
                            const unsigned hi = bf16_rne(w[((size_t)tap * cin + ci + 1) * cout + co]);
                            out[o++] = lo | (hi << 16);
                        }
                    }
    return o;
}

size_t pack_conv_x3(const float *w, int cin, int cout, int ncbl, float *dst) {
    // dst[group][chunk][piece][cbl][tap][lane][4 dwords]: piece t of pack_conv_weights_bf16's layout -- dword d of lane (g << 5) | m holds the
    // bf16 pair of W[tap][ci = chunk * 16 + 8 g + 2 d (+ 1)][co = cb * 32 + m] (low half = even channel).  Piece 0 = bf16(w), piece 1 =
    // bf16(w - piece 0), piece 2 = bf16(w - piece 0 - piece 1), the residuals formed in fp32 (exact), as pack_head_x3 does.
    const int nchunk = cin / 16;
    unsigned *out = reinterpret_cast<unsigned *>(dst);
    size_t o = 0;
    for (int grp = 0; grp < cout / (32 * ncbl); ++grp)
        for (int ch = 0; ch < nchunk; ++ch)
            for (int t = 0; t < 3; ++t)
                for (int cbl = 0; cbl < ncbl; ++cbl)
                    for (int tap = 0; tap < 9; ++tap)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int m = lane & 31, g = lane >> 5, co = (grp * ncbl + cbl) * 32 + m;
                            for (int d = 0; d < 4; ++d) {
                                unsigned short piece[2];
                                for (int hh = 0; hh < 2; ++hh)
                                    piece[hh] = x3_piece(w[((size_t)tap * cin + ch * 16 + 8 * g + 2 * d + hh) * cout + co], t);
                                out[o++] = (unsigned)piece[0] | ((unsigned)piece[1] << 16);
                            }
                        }
    return o;
}

// Order of the 4 x cout phase-major virtual channels (phase = 2 py + px, then channel) in the packed filter / bias of the transposed
// conv tilings: dst column v takes source column wst_pack_order(cout, v).  cout = 16: unchanged (blocks {00 + 01}, {10 + 11}).
// cout % 32 == 0: workgroup (group) 2 i holds {phase 00, phase 11} of channels 32 i .., group 2 i + 1 holds {01, 10} (tconv_ws_kernel).
int wst_pack_order(int cout, int v) {
    if (cout == 16) return v;
    const int nb = v / 32, r = v % 32, grp = nb / 2, k = nb % 2, i = grp / 2;
    const int ph = (grp & 1) ? (k == 0 ? 1 : 2) : (k == 0 ? 0 : 3);
    return ph * cout + i * 32 + r;
}

size_t pack_wino_weights(const float *w, int cin, int cout, int ncb, float *dst) {
    const int WNCBL = ncb;
    // w: folded [3][3][cin][cout].  U = G g G^T per (ci, co), G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]].
    // dst[group][chunk][cbl][k = 4*xi + nu][lane][s]:  lane = (g << 4) | m,
    //   ci = chunk*16 + 4*g + s, co = (group*4 + cbl)*16 + m          (A fragment of v_mfma_f32_16x16x4_f32)
    const int nchunk = cin / WKC;
    size_t o = 0;
    for (int grp = 0; grp < cout / (16 * WNCBL); ++grp)
        for (int ch = 0; ch < nchunk; ++ch)
            for (int cbl = 0; cbl < WNCBL; ++cbl)
                for (int k = 0; k < 16; ++k)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int s = 0; s < 4; ++s) {
                            const int m = lane & 15, g = lane >> 4;
                            const int ci = ch * WKC + 4 * g + s, co = (grp * WNCBL + cbl) * 16 + m;
                            const int xi = k >> 2, nu = k & 3;
                            double u = 0.0;                 // exact products of small dyadic factors; one rounding
                            for (int i = 0; i < 3; ++i)
                                for (int j = 0; j < 3; ++j)
                                    u += (double)G22[xi][i] * (double)w[((size_t)(i * 3 + j) * cin + ci) * cout + co] * (double)G22[nu][j];
                            dst[o++] = (float)u;
                        }
    return o;
}

size_t pack_lstm_gate_weights(const float *w, int cin_total, int c_first, const float *bias, float *dst, float *bias_perm) {
    // packed channel P = 16 w + m (MFMA row m = 4 g + e of block w)  <-  original channel 16 e + (4 w + g): gate e of hidden channel 4 w + g
    float tmp[9 * WKC * 64];
    for (int P = 0; P < 64; ++P) {
        const int wv = P / 16, m = P % 16, orig = (m % 4) * 16 + 4 * wv + m / 4;
        if (bias_perm) bias_perm[P] = bias ? bias[orig] : 0.f;
        for (int t = 0; t < 9; ++t)
            for (int ci = 0; ci < WKC; ++ci) tmp[(t * WKC + ci) * 64 + P] = w[((size_t)t * cin_total + c_first + ci) * 64 + orig];
    }
    return pack_wino24_weights(tmp, WKC, 64, 4, dst);
}

size_t pack_wino24_weights(const float *w, int cin, int cout, int ncb, float *dst) {
    // w: folded [3][3][cin][cout].  U = G_y g G_x^T per (ci, co); G_y = F(2,3) rows, G_x = F(4,3) columns.
    // dst[group of 16 ncb][chunk][cbl 0..ncb-1][k = 6 i + j][lane][s]:  lane = (g << 4) | m, ci = chunk*16 + 4*g + s, co = (group*ncb + cbl)*16 + m
    static const double GY[4][3] = {{1, 0, 0}, {.5, .5, .5}, {.5, -.5, .5}, {0, 0, 1}};
    static const double GX[6][3] = {{1.0 / 4, 0, 0}, {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                                    {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6}, {0, 0, 1}};
    const int nchunk = cin / WKC;
    size_t o = 0;
    for (int grp = 0; grp < cout / (16 * ncb); ++grp)
        for (int ch = 0; ch < nchunk; ++ch)
            for (int cbl = 0; cbl < ncb; ++cbl)
                for (int k = 0; k < NK; ++k)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int s = 0; s < 4; ++s) {
                            const int m = lane & 15, g = lane >> 4;
                            const int ci = ch * WKC + 4 * g + s, co = (grp * ncb + cbl) * 16 + m;
                            const int i = k / 6, j = k % 6;
                            double u = 0.0;
                            for (int p = 0; p < 3; ++p)
                                for (int q = 0; q < 3; ++q)
                                    u += GY[i][p] * (double)w[((size_t)(p * 3 + q) * cin + ci) * cout + co] * GX[j][q];
                            dst[o++] = (float)u;
                        }
    return o;
}

// bf16 ConvLSTM (ws_main, LS): the input-channel slice [c_first, c_first + ncin) of the gate kernel [3][3][cin_total][64] with the output channels permuted:
// packed channel P = 32 cb + 8 j + 4 g + i (MFMA row 8 j + 4 g + i of block cb)  <-  gate e = 2 cb + (j >> 1) of hidden channel 8 g + 4 (j & 1) + i:
// the accumulator registers of lane half g are then (i | j) in block 0 and (f | o) in block 1, eight hidden channels each
static size_t lstm_gate_bf16(const float *w, int cin_total, int c_first, int ncin, const float *bias, float *dst, float *bias_perm) {
    std::vector<float> tmp((size_t)9 * ncin * 64);
    for (int P = 0; P < 64; ++P) {
        const int cb = P / 32, row = P % 32, j = row / 8, g = (row / 4) & 1, i = row % 4;
        const int orig = (2 * cb + (j >> 1)) * 16 + 8 * g + 4 * (j & 1) + i;
        if (bias_perm) bias_perm[P] = bias ? bias[orig] : 0.f;
        for (int t = 0; t < 9; ++t)
            for (int ci = 0; ci < ncin; ++ci) tmp[((size_t)t * ncin + ci) * 64 + P] = w[((size_t)t * cin_total + c_first + ci) * 64 + orig];
    }
    return pack_conv_weights_bf16(tmp.data(), 3, ncin, 64, 2, dst);
}

size_t pack_lstm_gate_weights_bf16_xh(const float *w, const float *bias, float *dst, float *bias_perm) {
    // both 16-channel halves of the gate kernel [3][3][16 + 16][64] as the two chunks of ONE filter (chunk 0 = x rows, chunk 1 = h rows),
    // output channels permuted as in pack_lstm_gate_weights_bf16: the resident filter of ws_main LS 3
    return lstm_gate_bf16(w, 32, 0, 32, bias, dst, bias_perm);
}

size_t pack_lstm_gate_weights_bf16(const float *w, int cin_total, int c_first, const float *bias, float *dst, float *bias_perm) {
    return lstm_gate_bf16(w, cin_total, c_first, 16, bias, dst, bias_perm);
}

// FCN head (k order documented at the top of kernels_head.hip)
void pack_sq(const float *w, int cin, float *dst) {
    // W is [cin][32].  dst[j][lane][i] = W[ci = 8j + 4g + i][co = m],  lane = (g<<5)|m
    for (int j = 0; j < cin / 8; ++j)
        for (int lane = 0; lane < 64; ++lane)
            for (int i = 0; i < 4; ++i)
                dst[(j * 64 + lane) * 4 + i] = w[(8 * j + 4 * (lane >> 5) + i) * 32 + (lane & 31)];
}

void pack_rowmap_32x64(const float *w, int ld, float *dst) {
    // W is 32 rows (k) x 64 cols (cout), row stride ld.  dst[cb][q4][lane][i]:
    //   k = rowmap(4*q4 + i, g), co = 32*cb + m   (B operand = a 32-row accumulator tile)
    for (int cb = 0; cb < 2; ++cb)
        for (int q4 = 0; q4 < 4; ++q4)
            for (int lane = 0; lane < 64; ++lane)
                for (int i = 0; i < 4; ++i) {
                    const int g = lane >> 5, m = lane & 31;
                    dst[(((cb * 4 + q4) * 64 + lane) * 4) + i] = w[rowmap(4 * q4 + i, g) * ld + cb * 32 + m];
                }
}

void pack_head_x3(const float *w, int k_in, float *dst) {
    // W is [k_in rows (32 or 64)][64 out], row stride 64.  dst[t][cb][kc][lane][d] (dwords), kc < k_in / 16: t = piece (bf16 of w, of
    // the remainder, of the rest), lane = (g << 5) | m, cout = 32 cb + m, k slot e = 2 d (+1 in the high half) <-> input row
    // 32 (kc / 2) + rowmap(8 (kc & 1) + e, g): the registers of the 32-row accumulator tile(s) the MFMA wave holds
    unsigned *o = reinterpret_cast<unsigned *>(dst);
    const int nkc = k_in / 16;
    for (int t = 0; t < 3; ++t)
        for (int cb = 0; cb < 2; ++cb)
            for (int kc = 0; kc < nkc; ++kc)
                for (int lane = 0; lane < 64; ++lane)
                    for (int d = 0; d < 4; ++d) {
                        const int g = lane >> 5, m = lane & 31;
                        unsigned short piece[2];
                        for (int hh = 0; hh < 2; ++hh) {
                            const int e = 2 * d + hh, ch = 32 * (kc / 2) + rowmap(8 * (kc & 1) + e, g);
                            piece[hh] = x3_piece(w[ch * 64 + 32 * cb + m], t);
                        }
                        o[((((t * 2 + cb) * nkc + kc) * 64 + lane) * 4) + d] = (unsigned)piece[0] | ((unsigned)piece[1] << 16);
                    }
}

void pack_head_bf16(const float *w, int k_in, int n_out, int acc_k, float *dst) {
    // W is [k_in rows][n_out], row stride n_out.  dst[cb][kc][lane][d] (dwords), cb < n_out / 32, kc < k_in / 16: the A fragments of mfma_bf16,
    // lane = (g << 5) | m, cout = 32 cb + m, k slot e = 2 d (+1 in the high half) of chunk kc <-> input row 16 kc + 8 g + e (acc_k 0: the
    // stored conv0 half-block) or 32 (kc / 2) + rowmap(8 (kc & 1) + e, g) (acc_k 1: the registers of the accumulator tile(s), as pack_head_x3).
    // Each weight is rounded to bf16 (RNE) once, here.
    unsigned *o = reinterpret_cast<unsigned *>(dst);
    const int nkc = k_in / 16;
    for (int cb = 0; cb < n_out / 32; ++cb)
        for (int kc = 0; kc < nkc; ++kc)
            for (int lane = 0; lane < 64; ++lane)
                for (int d = 0; d < 4; ++d) {
                    const int g = lane >> 5, m = lane & 31;
                    unsigned short piece[2];
                    for (int hh = 0; hh < 2; ++hh) {
                        const int e = 2 * d + hh, row = acc_k ? 32 * (kc / 2) + rowmap(8 * (kc & 1) + e, g) : 16 * kc + 8 * g + e;
                        piece[hh] = bf16_rne(w[row * n_out + 32 * cb + m]);
                    }
                    o[(((cb * nkc + kc) * 64 + lane) * 4) + d] = (unsigned)piece[0] | ((unsigned)piece[1] << 16);
                }
}

void pack_head_lg(const float *w, int n_class, float *dst) {
    // W is [64][n_class].  dst[g][c][cb*16 + r] = W[cb*32 + rowmap(r, g)][c]
    for (int g = 0; g < 2; ++g)
        for (int c = 0; c < n_class; ++c)
            for (int cb = 0; cb < 2; ++cb)
                for (int r = 0; r < 16; ++r)
                    dst[(g * n_class + c) * 32 + cb * 16 + r] = w[(cb * 32 + rowmap(r, g)) * n_class + c];
}

// the layout of tconv_as_conv2x2 is documented in pack.h
void tconv_as_conv2x2(const float *w, int cin, int cout, float *dst) {
    const int c4 = 4 * cout;
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b)
            for (int ci = 0; ci < cin; ++ci)
                for (int py = 0; py < 2; ++py)
                    for (int px = 0; px < 2; ++px) {
                        const int kh = py == 0 ? (a == 0 ? 2 : 0) : (a == 1 ? 1 : -1);
                        const int kw = px == 0 ? (b == 0 ? 2 : 0) : (b == 1 ? 1 : -1);
                        for (int co = 0; co < cout; ++co) {
                            const float v = (kh < 0 || kw < 0) ? 0.f : w[((size_t)(kh * 3 + kw) * cin + ci) * cout + co];
                            dst[((size_t)(a * 2 + b) * cin + ci) * c4 + (py * 2 + px) * cout + co] = v;
                        }
                    }
}

// Fused tail: A fragments of v_mfma_f32_16x16x32_bf16 (lane l: row l & 15, k = 8 (l >> 4) + j, j = 0..7; two bf16 per dword).
//   wA0 [9 taps][64 lanes][4 dwords]: up0_0, k = input channel of concat[skip 0..15, up 16..31], row = output channel
//   wA1 [5 pairs][64][4]: up0_1, k < 16: tap 2 p, channel k; k >= 16: tap 2 p + 1, channel k - 16 (zero for the missing tap 9)
void pack_tail_weights(const float *w0 /*[3][3][32][16] folded*/, const float *w1 /*[3][3][16][16] folded*/, float *dst0 /*9*64*4*/, float *dst1 /*5*64*4*/) {
    unsigned *o0 = reinterpret_cast<unsigned *>(dst0), *o1 = reinterpret_cast<unsigned *>(dst1);
    for (int t = 0; t < 9; ++t)
        for (int l = 0; l < 64; ++l)
            for (int d = 0; d < 4; ++d) {
                const int m = l & 15, k = 8 * (l >> 4) + 2 * d;
                o0[(t * 64 + l) * 4 + d] = (unsigned)bf16_rne(w0[((size_t)t * 32 + k) * 16 + m]) | ((unsigned)bf16_rne(w0[((size_t)t * 32 + k + 1) * 16 + m]) << 16);
            }
    for (int p = 0; p < 5; ++p)
        for (int l = 0; l < 64; ++l)
            for (int d = 0; d < 4; ++d) {
                const int m = l & 15, k = 8 * (l >> 4) + 2 * d, t = 2 * p + (k >> 4), c = k & 15;
                const float v0 = t < 9 ? w1[((size_t)t * 16 + c) * 16 + m] : 0.f, v1 = t < 9 ? w1[((size_t)t * 16 + c + 1) * 16 + m] : 0.f;
                o1[(p * 64 + l) * 4 + d] = (unsigned)bf16_rne(v0) | ((unsigned)bf16_rne(v1) << 16);
            }
}

// Fused stem: A fragments (lane l: row l & 15, k = 8 (l >> 4) + j):
//   wA0 [64 lanes][4 dwords]: conv0_0 [3][3][1][16] folded: k = 4 kh + kw for kw < 3, kh < 3; zero elsewhere
void pack_stem_weights(const float *w0 /*[3][3][1][16] folded*/, float *dst0 /*64*4*/) {
    unsigned *o0 = reinterpret_cast<unsigned *>(dst0);
    for (int l = 0; l < 64; ++l)
        for (int d = 0; d < 4; ++d) {
            unsigned short h[2];
            for (int e = 0; e < 2; ++e) {
                const int m = l & 15, k = 8 * (l >> 4) + 2 * d + e, kh = k >> 2, kw = k & 3;
                h[e] = (kh < 3 && kw < 3) ? bf16_rne(w0[(kh * 3 + kw) * 16 + m]) : (unsigned short)0;
            }
            o0[l * 4 + d] = (unsigned)h[0] | ((unsigned)h[1] << 16);
        }
}

// w: folded weights [3 dt][ny][nx][cin][cout] of ONE phase (dt = time tap - 1, taps already in kernel order);
// dst: [tap][chunk of 8 channels][32-channel block][lane][4]: lane (m, h) k-step s -> W[c*8 + 4h + s][blk*32 + m] (0 beyond cout)
void pack_conv3d_weights(const float *w, int ntap, int cin, int cout, int cout_pad, float *dst) {
    const int nch = cin / 8, ncob = cout_pad / 32;
    for (int tap = 0; tap < ntap; ++tap)
        for (int c = 0; c < nch; ++c)
            for (int blk = 0; blk < ncob; ++blk)
                for (int lane = 0; lane < 64; ++lane)
                    for (int s = 0; s < 4; ++s) {
                        const int m = lane & 31, hh = lane >> 5, ci = c * 8 + 4 * hh + s, co = blk * 32 + m;
                        dst[((((size_t)tap * nch + c) * ncob + blk) * 64 + lane) * 4 + s] =
                            co < cout ? w[((size_t)tap * cin + ci) * cout + co] : 0.f;
                    }
}

// w: folded fp32 weights [ntap][cin][cout] of ONE phase (taps already in kernel order), rounded here, once, to bf16;
// dst: [tap][K step of 16 channels][32-channel block][lane][8] bf16: lane (m, h) element j -> W[16 c + 8 h + j][32 blk + m] (0 beyond cout);
// ntap * cin * cout_pad / 2 dwords
void pack_conv3d_weights_bf16(const float *w, int ntap, int cin, int cout, int cout_pad, float *dst) {
    const int nk = cin / 16, ncob = cout_pad / 32;
    uint16_t *d = reinterpret_cast<uint16_t *>(dst);
    for (int tap = 0; tap < ntap; ++tap)
        for (int c = 0; c < nk; ++c)
            for (int blk = 0; blk < ncob; ++blk)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j) {
                        const int m = lane & 31, hh = lane >> 5, ci = c * 16 + 8 * hh + j, co = blk * 32 + m;
                        d[((((size_t)tap * nk + c) * ncob + blk) * 64 + lane) * 8 + j] =
                            co < cout ? bf16_rne(w[((size_t)tap * cin + ci) * cout + co]) : (uint16_t)0;
                    }
}

}  // namespace ukbb
