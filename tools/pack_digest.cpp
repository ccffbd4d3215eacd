// Every host-side weight packer (ukbb_cardiac_amd/csrc/pack.h) on fixed inputs: one line per case with the name, the arguments, the number
// of 32-bit words written and an FNV-1a-64 digest of the output bytes; last, bf16_rne of a fixed list of bit patterns.  Links pack.cpp and
// nothing else (make -C ukbb_cardiac_amd/csrc pack_digest).  tests/test_pack.py compares the digest lines with tests/golden/pack_digests.txt,
// so a packed layout cannot move by a byte unnoticed.
//
// Inputs: an integer LCG (no library RNG: the stream is the same everywhere), re-seeded per case.  Every value is finite, of either sign, with
// an exponent between 2^-15 and 2^4; one in eight lies exactly on a bf16 rounding tie (low 16 bits 0x8000) and one in eight is a bf16 value
// already (low 16 bits 0).
// Shapes: the smallest at which every loop of a packer makes two or more trips wherever the engine ever gives it two or more (engine.cpp
// ensure_packed*, ukbb_fcn_create).  Outputs are pre-filled with 0xffffffff, so a word a packer leaves unwritten shows in the digest.
#include "pack.h"

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace ukbb;

namespace {

uint32_t g_lcg;
uint32_t lcg() { g_lcg = g_lcg * 1664525u + 1013904223u; return g_lcg >> 8; }      // the high 24 bits: the low ones of an LCG have short periods

float next_weight() {
    const uint32_t a = lcg(), b = lcg();
    uint32_t u = ((a & 1u) << 31) | ((112u + (a >> 1) % 20u) << 23) | (b & 0x7fffffu);
    const uint32_t kind = (a >> 8) & 7u;
    if (kind == 0) u = (u & 0xffff0000u) | 0x8000u;      // a tie between two bf16 neighbours
    if (kind == 1) u &= 0xffff0000u;                     // a bf16 value
    float f; memcpy(&f, &u, 4);
    return f;
}

std::vector<float> weights(size_t n, uint32_t seed) {
    g_lcg = seed;
    std::vector<float> v(n);
    for (float &x : v) x = next_weight();
    return v;
}

// an output buffer of n 32-bit words, every bit set
std::vector<float> blank(size_t n) {
    std::vector<float> v(n);
    if (n) memset(v.data(), 0xff, n * 4);
    return v;
}

uint64_t fnv1a64(uint64_t h, const void *p, size_t bytes) {
    const unsigned char *c = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < bytes; ++i) { h ^= c[i]; h *= 0x100000001b3ull; }
    return h;
}
constexpr uint64_t FNV0 = 0xcbf29ce484222325ull;

int g_bad = 0;

// one result line: the outputs, in order, as (pointer, words) pairs
struct Out { const void *p; size_t words; };
void report(std::initializer_list<Out> outs, const char *fmt, ...) {
    char args[256];
    va_list ap; va_start(ap, fmt); vsnprintf(args, sizeof args, fmt, ap); va_end(ap);
    uint64_t h = FNV0; size_t words = 0;
    for (const Out &o : outs) { h = fnv1a64(h, o.p, o.words * 4); words += o.words; }
    printf("%s words=%zu fnv1a64=%016llx\n", args, words, (unsigned long long)h);
}
// a packer that returns its count must have filled the buffer exactly
void expect_count(const char *name, size_t got, size_t want) {
    if (got != want) { fprintf(stderr, "%s returned %zu words, expected %zu\n", name, got, want); g_bad = 1; }
}

void conv(int ks, int cin, int cout, int mb, int kc, int ncbl) {
    const size_t n = (size_t)ks * ks * cin * cout;
    const auto w = weights(n, 101); auto d = blank(n);
    expect_count("pack_conv_weights", pack_conv_weights(w.data(), ks, cin, cout, mb, kc, ncbl, d.data()), n);
    report({{d.data(), n}}, "pack_conv_weights ks=%d cin=%d cout=%d mb=%d kc=%d ncbl=%d", ks, cin, cout, mb, kc, ncbl);
}
void conv_bf16(int ks, int cin, int cout, int ncbl) {
    const size_t n = (size_t)ks * ks * cin * cout;
    const auto w = weights(n, 102); auto d = blank(n / 2);
    expect_count("pack_conv_weights_bf16", pack_conv_weights_bf16(w.data(), ks, cin, cout, ncbl, d.data()), n / 2);
    report({{d.data(), n / 2}}, "pack_conv_weights_bf16 ks=%d cin=%d cout=%d ncbl=%d", ks, cin, cout, ncbl);
}
void conv_x3(int cin, int cout, int ncbl) {
    const size_t n = (size_t)9 * cin * cout;
    const auto w = weights(n, 103); auto d = blank(3 * n / 2);
    expect_count("pack_conv_x3", pack_conv_x3(w.data(), cin, cout, ncbl, d.data()), 3 * n / 2);
    report({{d.data(), 3 * n / 2}}, "pack_conv_x3 cin=%d cout=%d ncbl=%d", cin, cout, ncbl);
}
void wino(bool f24, int cin, int cout, int ncb) {
    const size_t n = (size_t)(f24 ? 24 : 16) * cin * cout;
    const auto w = weights((size_t)9 * cin * cout, 104); auto d = blank(n);
    const char *name = f24 ? "pack_wino24_weights" : "pack_wino_weights";
    expect_count(name, f24 ? pack_wino24_weights(w.data(), cin, cout, ncb, d.data()) : pack_wino_weights(w.data(), cin, cout, ncb, d.data()), n);
    report({{d.data(), n}}, "%s cin=%d cout=%d ncb=%d", name, cin, cout, ncb);
}
void wino_first() {
    const size_t n = 16 * 16 * 16;
    const auto w = weights(9 * 16 * 16, 105); auto d = blank(n);
    expect_count("pack_wino_first_weights", pack_wino_first_weights(w.data(), d.data()), n);
    report({{d.data(), n}}, "pack_wino_first_weights");
}
// form 0: fp32 F(2x4), 1: bf16 -- a 16-channel slice of [3][3][cin_total][64]; 2: bf16, both halves of [3][3][32][64]
void lstm_gate(int form, int cin_total, int c_first, bool with_bias) {
    const auto w = weights((size_t)9 * cin_total * 64, 106), b = weights(64, 107);
    const size_t n = form == 0 ? (size_t)24 * 16 * 64 : form == 1 ? (size_t)9 * 16 * 64 / 2 : (size_t)9 * 32 * 64 / 2;
    auto d = blank(n), bp = blank(64);
    const float *bias = with_bias ? b.data() : nullptr;
    float *perm = with_bias ? bp.data() : nullptr;
    const size_t got = form == 0 ? pack_lstm_gate_weights(w.data(), cin_total, c_first, bias, d.data(), perm)
                     : form == 1 ? pack_lstm_gate_weights_bf16(w.data(), cin_total, c_first, bias, d.data(), perm)
                                 : pack_lstm_gate_weights_bf16_xh(w.data(), bias, d.data(), perm);
    const char *name = form == 0 ? "pack_lstm_gate_weights" : form == 1 ? "pack_lstm_gate_weights_bf16" : "pack_lstm_gate_weights_bf16_xh";
    expect_count(name, got, n);
    const Out o_d{d.data(), n}, o_b{bp.data(), with_bias ? (size_t)64 : 0};      // the permuted bias is part of the digest
    if (form == 2) report({o_d, o_b}, "%s bias=%d", name, (int)with_bias);
    else report({o_d, o_b}, "%s cin_total=%d c_first=%d bias=%d", name, cin_total, c_first, (int)with_bias);
}
void sq(int cin) {
    const auto w = weights((size_t)cin * 32, 108); auto d = blank((size_t)cin * 32);
    pack_sq(w.data(), cin, d.data());
    report({{d.data(), d.size()}}, "pack_sq cin=%d", cin);
}
void rowmap_32x64(int row0) {      // as ukbb_fcn_create calls it: 32 rows of a 64-column matrix, from row row0
    const auto w = weights(64 * 64, 109); auto d = blank(2 * 4 * 64 * 4);
    pack_rowmap_32x64(w.data() + (size_t)row0 * 64, 64, d.data());
    report({{d.data(), d.size()}}, "pack_rowmap_32x64 ld=64 row0=%d", row0);
}
void head_lg(int n_class) {
    const auto w = weights((size_t)64 * n_class, 110); auto d = blank((size_t)2 * n_class * 32);
    pack_head_lg(w.data(), n_class, d.data());
    report({{d.data(), d.size()}}, "pack_head_lg n_class=%d", n_class);
}
void head_x3(int k_in) {
    const auto w = weights((size_t)k_in * 64, 111); auto d = blank((size_t)3 * 2 * (k_in / 16) * 64 * 4);
    pack_head_x3(w.data(), k_in, d.data());
    report({{d.data(), d.size()}}, "pack_head_x3 k_in=%d", k_in);
}
void head_bf16(int k_in, int n_out, int acc_k) {
    const auto w = weights((size_t)k_in * n_out, 112); auto d = blank((size_t)(n_out / 32) * (k_in / 16) * 64 * 4);
    pack_head_bf16(w.data(), k_in, n_out, acc_k, d.data());
    report({{d.data(), d.size()}}, "pack_head_bf16 k_in=%d n_out=%d acc_k=%d", k_in, n_out, acc_k);
}
void tail() {
    const auto w0 = weights(9 * 32 * 16, 113), w1 = weights(9 * 16 * 16, 114);
    auto d0 = blank(9 * 64 * 4), d1 = blank(5 * 64 * 4);
    pack_tail_weights(w0.data(), w1.data(), d0.data(), d1.data());
    report({{d0.data(), d0.size()}, {d1.data(), d1.size()}}, "pack_tail_weights");
}
void stem() {
    const auto w = weights(9 * 16, 115); auto d = blank(64 * 4);
    pack_stem_weights(w.data(), d.data());
    report({{d.data(), d.size()}}, "pack_stem_weights");
}
void conv3d(bool bf16, int ntap, int cin, int cout, int cout_pad) {
    const auto w = weights((size_t)ntap * cin * cout, 116); auto d = blank((size_t)ntap * cin * cout_pad / (bf16 ? 2 : 1));
    if (bf16) pack_conv3d_weights_bf16(w.data(), ntap, cin, cout, cout_pad, d.data());
    else pack_conv3d_weights(w.data(), ntap, cin, cout, cout_pad, d.data());
    report({{d.data(), d.size()}}, "%s ntap=%d cin=%d cout=%d cout_pad=%d", bf16 ? "pack_conv3d_weights_bf16" : "pack_conv3d_weights", ntap, cin, cout, cout_pad);
}
void tconv(int cin, int cout) {
    const auto w = weights((size_t)9 * cin * cout, 117); auto d = blank((size_t)4 * cin * 4 * cout);
    tconv_as_conv2x2(w.data(), cin, cout, d.data());
    report({{d.data(), d.size()}}, "tconv_as_conv2x2 cin=%d cout=%d", cin, cout);
}
void wst_order(int cout) {
    std::vector<int32_t> o((size_t)4 * cout);
    for (int v = 0; v < 4 * cout; ++v) o[v] = wst_pack_order(cout, v);
    report({{o.data(), o.size()}}, "wst_pack_order cout=%d", cout);
}

}  // namespace

int main() {
    conv(3, 16, 64, 32, 8, 1); conv(3, 16, 64, 16, 8, 2); conv(1, 32, 32, 32, 16, 1); conv(2, 16, 128, 32, 16, 2);
    conv_bf16(3, 32, 64, 1); conv_bf16(3, 32, 128, 2); conv_bf16(2, 32, 64, 2);
    conv_x3(32, 64, 1); conv_x3(32, 128, 2);
    wino(false, 32, 128, 4); wino(false, 32, 64, 2);
    wino(true, 32, 128, 4); wino(true, 32, 64, 2);
    wino_first();
    for (int form = 0; form < 2; ++form) { lstm_gate(form, 32, 0, true); lstm_gate(form, 32, 16, false); }
    lstm_gate(2, 32, 0, true); lstm_gate(2, 32, 0, false);
    sq(16); sq(32);
    rowmap_32x64(0); rowmap_32x64(32);
    head_lg(2); head_lg(3); head_lg(4);
    head_x3(32); head_x3(64);
    head_bf16(16, 32, 0); head_bf16(32, 64, 1); head_bf16(64, 64, 1);
    tail(); stem();
    conv3d(false, 27, 8, 16, 32); conv3d(false, 12, 16, 64, 64);
    conv3d(true, 27, 16, 16, 32); conv3d(true, 12, 32, 64, 64);
    tconv(16, 16); tconv(32, 32);
    wst_order(16); wst_order(32); wst_order(64);

    // ties down and up, just above a tie, the largest finite value, the infinities, three NaNs (quiet, the smallest signalling one, a full
    // mantissa), the smallest subnormal, a subnormal tie, minus zero
    static const uint32_t pats[] = {0x3f808000u, 0x3f818000u, 0x3f808001u, 0x7f7fffffu, 0x7f800000u, 0xff800000u,
                                    0x7fc00000u, 0x7f800001u, 0x7fffffffu, 0x00000001u, 0x00008000u, 0x80000000u};
    printf("bf16_rne");
    for (const uint32_t u : pats) { float f; memcpy(&f, &u, 4); printf(" %08x:%04x", u, (unsigned)bf16_rne(f)); }
    printf("\n");
    return g_bad;
}
