// Per-run arithmetic of the label-volume gzip writer, ONE text for the host (label_gzip.cpp: the serial walk and the parallel formulation
// run serially) and for the gfx950 kernels (kernels_labelgz.hip).  The stream both write is a pure function of the run list of the label
// volume: a run of `run` equal labels whose voxel is the E-byte pattern P opens with E literals and continues with matches at distance E
// (split_run), the Huffman codes come from the exact token histogram (run_*_histogram, dynamic_codes), and the CRC-32 of a run has a
// closed form because the CRC register is linear over GF(2) (crc_pattern_run, crc_join).  Everything a kernel needs per run:
//   histogram contribution   run_open_histogram + run_tail_histogram
//   bit count                run_bits
//   emission                 emit_run through a sink with put(value, bits) and fill258(count, token, token bits)
//   CRC                      crc_pattern_run -> CrcPiece, joined in order with crc_join
// No tables in memory: length symbols and the fixed codes are arithmetic (RFC 1951 3.2.5 / 3.2.6).
#pragma once
#include <stdint.h>
#include <string.h>

#ifndef UKBB_HD
#if defined(__HIPCC__)
#define UKBB_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define UKBB_HD inline
#endif
#endif

namespace ukbb_labelgz {

constexpr uint32_t POLY = 0xEDB88320u;                 // CRC-32 (reflected)
constexpr int FIXED = 0, DYNAMIC = 1;                  // UKBB_GZIP_FIXED / UKBB_GZIP_DYNAMIC

// ---- GF(2) ------------------------------------------------------------------------------------------------------------------------------
UKBB_HD uint32_t mult(uint32_t a, uint32_t b) {        // a * b mod P (reflected polynomials, zlib's multmodp)
    if (!a) return 0;
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) { p ^= b; if ((a & (m - 1)) == 0) break; }
        m >>= 1;
        b = b & 1 ? (b >> 1) ^ POLY : b >> 1;
    }
    return p;
}
UKBB_HD void x2n_fill(uint32_t *x2n) {                 // x2n[k] = x^(2^k) mod P, k < 32
    x2n[0] = 1u << 30;
    for (int k = 1; k < 32; ++k) x2n[k] = mult(x2n[k - 1], x2n[k - 1]);
}
UKBB_HD uint32_t xpow8(const uint32_t *x2n, uint64_t nbytes) {          // x^(8 n)
    uint32_t p = 1u << 31;                             // x^0
    unsigned k = 3;
    for (uint64_t n = nbytes; n; n >>= 1, ++k)
        if (n & 1) p = mult(x2n[k & 31], p);
    return p;
}
UKBB_HD uint32_t shift_zero_bytes(const uint32_t *x2n, uint32_t reg, uint64_t nbytes) {   // CRC register after nbytes zero bytes: reg * x^(8 n)
    return mult(xpow8(x2n, nbytes), reg);
}
UKBB_HD uint32_t crc_byte(uint32_t reg, uint8_t b) {  // one byte, no table
    reg ^= b;
    for (int k = 0; k < 8; ++k) reg = reg & 1 ? (reg >> 1) ^ POLY : reg >> 1;
    return reg;
}

// A piece of the inflated stream as the CRC sees it: c = the register after the piece when started from 0 ("pure"), pw = x^(8 * its length).
// The register after the piece from any start value r is r * pw ^ c, hence the associative join of A followed by B.
struct CrcPiece { uint32_t c, pw; };
UKBB_HD CrcPiece crc_identity() { return CrcPiece{0u, 1u << 31}; }
UKBB_HD CrcPiece crc_join(CrcPiece a, CrcPiece b) { return CrcPiece{mult(b.pw, a.c) ^ b.c, mult(a.pw, b.pw)}; }
// k >= 1 copies of the E-byte pattern P.  Doubling: c(2k) = c(k) * x^(8kE) ^ c(k); a zero pattern has c = 0 and only its length counts.
UKBB_HD CrcPiece crc_pattern_run(const uint32_t *x2n, const uint8_t *P, int E, uint64_t k) {
    bool zero = true;
    for (int b = 0; b < E; ++b) zero = zero && P[b] == 0;
    if (zero) return CrcPiece{0u, xpow8(x2n, k * (uint64_t)E)};
    CrcPiece one{0u, x2n[E == 1 ? 3 : E == 2 ? 4 : E == 4 ? 5 : 6]};
    for (int b = 0; b < E; ++b) one.c = crc_byte(one.c, P[b]);
    int top = 0;
    for (uint64_t t = k; t >>= 1;) ++top;
    CrcPiece r = one;
    for (int b = top - 1; b >= 0; --b) {
        r = crc_join(r, r);
        if ((k >> b) & 1) r = crc_join(r, one);
    }
    return r;
}

// ---- voxels and tokens ------------------------------------------------------------------------------------------------------------------
UKBB_HD int element_pattern(int datatype, unsigned label, uint8_t out[8]) {   // little-endian bytes of `label` as NIfTI datatype; returns the size
    switch (datatype) {
        case 2:  out[0] = (uint8_t)label; return 1;                                                   // uint8
        case 4:  { const int16_t v = (int16_t)label; __builtin_memcpy(out, &v, 2); return 2; }         // int16
        case 8:  { const int32_t v = (int32_t)label; __builtin_memcpy(out, &v, 4); return 4; }         // int32
        case 16: { const float v = (float)label; __builtin_memcpy(out, &v, 4); return 4; }             // float32
        case 64: { const double v = (double)label; __builtin_memcpy(out, &v, 8); return 8; }           // float64
        default: return 0;
    }
}

// The matches that follow the E opening literals of a run: R = (run - 1) * E bytes at distance E as n258 matches of
// length 258 plus a tail: 0, a literal tail of 1-2 bytes (tail < 3), one match (3..258) or two (259, 260 -> tail - 3, 3).
UKBB_HD void split_run(uint64_t R, uint64_t &n258, unsigned &tail) {
    n258 = 0;
    if (R >= 261) { n258 = (R - 3) / 258; R -= 258 * n258; }
    if (R == 258) { ++n258; R = 0; }
    tail = (unsigned)R;
}

// length 3..258 -> symbol 257..285, extra bits and their value (RFC 1951 3.2.5)
UKBB_HD void length_code(int l, int &sym, int &xbits, int &xval) {
    const int m = l - 3;
    if (l == 258) { sym = 285; xbits = 0; xval = 0; return; }
    if (m < 8) { sym = 257 + m; xbits = 0; xval = 0; return; }
    int msb = 3;
    while ((m >> (msb + 1)) != 0) ++msb;
    xbits = msb - 2;
    sym = 261 + 4 * xbits + ((m >> xbits) & 3);
    xval = m & ((1 << xbits) - 1);
}
UKBB_HD int dist_code_of(int E) { return E == 1 ? 0 : E == 2 ? 1 : E == 4 ? 3 : 5; }

// ---- code sets --------------------------------------------------------------------------------------------------------------------------
struct CodeSet {
    uint16_t lit_bits[288]; uint8_t lit_len[288];     // literal/length codes, bit-reversed for LSB-first output
    uint32_t dbits; int dlen;                          // the one distance in use (E), extra bit included
};

UKBB_HD uint32_t rev_bits(uint32_t v, int n) { uint32_t r = 0; for (int i = 0; i < n; ++i) { r = (r << 1) | (v & 1); v >>= 1; } return r; }

UKBB_HD void fixed_codes(int E, CodeSet &c) {          // RFC 1951 3.2.6
    for (int s = 0; s < 288; ++s) {
        uint32_t code; int len;
        if (s < 144) { code = 0x30 + s; len = 8; }
        else if (s < 256) { code = 0x190 + (s - 144); len = 9; }
        else if (s < 280) { code = s - 256; len = 7; }
        else { code = 0xC0 + (s - 280); len = 8; }
        c.lit_bits[s] = (uint16_t)rev_bits(code, len); c.lit_len[s] = (uint8_t)len;
    }
    // distance code of E: 1 -> 0, 2 -> 1, 4 -> 3, 8 -> code 5 + extra bit 1 (distances 7-8); 5-bit codes go out MSB first
    c.dbits = rev_bits((uint32_t)dist_code_of(E), 5); c.dlen = 5;
    if (E == 8) { c.dbits |= 1u << 5; c.dlen = 6; }
}

struct HuffWork {
    uint64_t w[2 * 290];
    int32_t parent[2 * 290], sym[288 + 2], L[290];
    uint8_t alive[2 * 290];
};

// Huffman code lengths for freq[0..n) limited to max_len bits; symbols with freq 0 get length 0.  At least two symbols
// get a code (zlib's inflate rejects an incomplete literal/length or code-length code).
UKBB_HD void huffman_lengths(const uint64_t *freq, int n, int max_len, uint8_t *len, HuffWork &k) {
    uint64_t *w = k.w; int32_t *parent = k.parent, *sym = k.sym, *L = k.L; uint8_t *alive = k.alive;
    int m = 0;
    for (int i = 0; i < n; ++i) { len[i] = 0; if (freq[i]) sym[m++] = i; }
    for (int i = 0; m < 2 && i < n; ++i) if (!freq[i]) sym[m++] = i;    // pad with unused symbols (weight 0 -> treated as 1)
    // plain O(m^2) Huffman over <= 288 leaves: parent links, depth = code length
    int nn = m;
    for (int i = 0; i < m; ++i) { w[i] = freq[sym[i]] ? freq[sym[i]] : 1; parent[i] = -1; alive[i] = 1; }
    for (int left = m; left > 1; --left) {
        int a = -1, b = -1;
        for (int i = 0; i < nn; ++i) if (alive[i]) {
            if (a < 0 || w[i] < w[a]) { b = a; a = i; }
            else if (b < 0 || w[i] < w[b]) b = i;
        }
        w[nn] = w[a] + w[b]; parent[nn] = -1; alive[nn] = 1;
        parent[a] = parent[b] = nn; alive[a] = alive[b] = 0;
        ++nn;
    }
    for (int i = 0; i < m; ++i) { int d = 0; for (int j = i; parent[j] >= 0; j = parent[j]) ++d; L[i] = d < 1 ? 1 : d; }
    // limit: clamp, then repair the Kraft sum (unit 2^-max_len) to exactly 1
    int64_t K = 0;
    const int64_t full = (int64_t)1 << max_len;
    for (int i = 0; i < m; ++i) { if (L[i] > max_len) L[i] = max_len; K += full >> L[i]; }
    while (K > full) {                                 // lengthen the cheapest symbol that still can be (longest code < max_len, smallest weight)
        int best = -1;
        for (int i = 0; i < m; ++i) if (L[i] < max_len && (best < 0 || L[i] > L[best] || (L[i] == L[best] && w[i] < w[best]))) best = i;
        K -= full >> (L[best] + 1); ++L[best];
    }
    while (K < full) {                                 // shorten: the heaviest symbol whose step fits the deficit
        int best = -1;
        for (int i = 0; i < m; ++i) if (L[i] > 1 && (full >> L[i]) <= full - K && (best < 0 || w[i] > w[best])) best = i;
        K += full >> L[best]; --L[best];
    }
    for (int i = 0; i < m; ++i) len[sym[i]] = (uint8_t)L[i];
}

UKBB_HD void canonical_codes(const uint8_t *len, int n, int max_len, uint16_t *bits) {   // RFC 1951 3.2.2, bit-reversed
    int count[16], next[16];
    for (int i = 0; i < 16; ++i) { count[i] = 0; next[i] = 0; }
    for (int i = 0; i < n; ++i) ++count[len[i]];
    count[0] = 0;
    int code = 0;
    for (int b = 1; b <= max_len; ++b) { code = (code + count[b - 1]) << 1; next[b] = code; }
    for (int i = 0; i < n; ++i) bits[i] = len[i] ? (uint16_t)rev_bits((uint32_t)next[len[i]]++, len[i]) : 0;
}

struct HeaderWork {
    HuffWork huff;
    uint64_t clfreq[19];
    uint16_t clb[19];
    uint8_t cll[19];
    uint8_t seq[286 + 30], cl_sym[286 + 30], cl_xbits[286 + 30], cl_xval[286 + 30];
};

// The dynamic code set from the exact token histogram lit[0..286) (end of block counted), and the BTYPE 10 block header -- BTYPE, HLIT /
// HDIST / HCLEN, the code-length code, the run-length coded code lengths -- into w (put(value, bits), LSB first).
template <class W>
UKBB_HD void dynamic_codes(const uint64_t *lit, int E, CodeSet &cs, HeaderWork &k, W &w) {
    huffman_lengths(lit, 286, 15, cs.lit_len, k.huff);
    cs.lit_len[286] = cs.lit_len[287] = 0;
    canonical_codes(cs.lit_len, 286, 15, cs.lit_bits);
    cs.lit_bits[286] = cs.lit_bits[287] = 0;
    // one distance code in use: a single 1-bit code (RFC 1951 3.2.7), then the extra bit of distances 7-8 for E = 8
    const int dcode = dist_code_of(E);
    cs.dbits = 0; cs.dlen = 1;
    if (E == 8) { cs.dbits |= 1u << 1; cs.dlen = 2; }
    int nlit = 286;
    while (nlit > 257 && !cs.lit_len[nlit - 1]) --nlit;
    const int ndist = dcode + 1;
    uint8_t *seq = k.seq;
    for (int i = 0; i < nlit; ++i) seq[i] = cs.lit_len[i];
    for (int i = 0; i < ndist; ++i) seq[nlit + i] = (uint8_t)(i == dcode ? 1 : 0);
    const int nseq = nlit + ndist;
    int ncl = 0;
    auto cl = [&](int sym, int xbits, int xval) { k.cl_sym[ncl] = (uint8_t)sym; k.cl_xbits[ncl] = (uint8_t)xbits; k.cl_xval[ncl] = (uint8_t)xval; ++ncl; };
    for (int i = 0; i < 19; ++i) k.clfreq[i] = 0;
    for (int i = 0; i < nseq;) {
        int j = i + 1;
        while (j < nseq && seq[j] == seq[i]) ++j;
        int rep = j - i;
        if (seq[i] == 0) {
            while (rep >= 11) { const int n = rep > 138 ? 138 : rep; cl(18, 7, n - 11); rep -= n; }
            if (rep >= 3) { cl(17, 3, rep - 3); rep = 0; }
            while (rep-- > 0) cl(0, 0, 0);
        } else {
            cl(seq[i], 0, 0); --rep;
            while (rep >= 3) { const int n = rep > 6 ? 6 : rep; cl(16, 2, n - 3); rep -= n; }
            while (rep-- > 0) cl(seq[i], 0, 0);
        }
        i = j;
    }
    for (int i = 0; i < ncl; ++i) ++k.clfreq[k.cl_sym[i]];
    huffman_lengths(k.clfreq, 19, 7, k.cll, k.huff);
    canonical_codes(k.cll, 19, 7, k.clb);
    // the order of RFC 1951 3.2.7 (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15) as arithmetic
    auto order = [](int i) { return i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? 10 - ((i + 1) >> 1) : 6 + (i >> 1); };
    int hclen = 19;
    while (hclen > 4 && !k.cll[order(hclen - 1)]) --hclen;
    w.put(2, 2);                                       // BTYPE = 10, dynamic Huffman
    w.put((uint32_t)(nlit - 257), 5);
    w.put((uint32_t)(ndist - 1), 5);
    w.put((uint32_t)(hclen - 4), 4);
    for (int i = 0; i < hclen; ++i) w.put(k.cll[order(i)], 3);
    for (int i = 0; i < ncl; ++i) {
        w.put(k.clb[k.cl_sym[i]], k.cll[k.cl_sym[i]]);
        if (k.cl_xbits[i]) w.put(k.cl_xval[i], k.cl_xbits[i]);
    }
}

// the (258, E) token under a code set
UKBB_HD void token258(const CodeSet &cs, uint32_t &bits, int &len) {
    len = cs.lit_len[285] + cs.dlen;
    bits = (uint32_t)cs.lit_bits[285] | (cs.dbits << cs.lit_len[285]);
}

// ---- one run: histogram, bit count, emission ---------------------------------------------------------------------------------------------
// add(symbol, count).  The opening literals of `count` runs of one label, and what follows the opening literals of one run.
template <class F>
UKBB_HD void run_open_histogram(const uint8_t *P, int E, uint64_t count, F &&add) { for (int b = 0; b < E; ++b) add((int)P[b], count); }
template <class F>
UKBB_HD void run_tail_histogram(const uint8_t *P, int E, uint64_t run, F &&add) {
    uint64_t n258; unsigned tail;
    split_run((run - 1) * (uint64_t)E, n258, tail);
    int s, xb, xv;
    if (n258) add(285, n258);
    if (tail > 258) { length_code((int)tail - 3, s, xb, xv); add(s, (uint64_t)1); add(257, (uint64_t)1); }
    else if (tail >= 3) { length_code((int)tail, s, xb, xv); add(s, (uint64_t)1); }
    else for (unsigned b = 0; b < tail; ++b) add((int)P[b % E], (uint64_t)1);
}

UKBB_HD int match_bits(const CodeSet &cs, int len) {
    int s, xb, xv;
    length_code(len, s, xb, xv);
    return cs.lit_len[s] + xb + cs.dlen;
}
UKBB_HD uint64_t run_bits(const CodeSet &cs, const uint8_t *P, int E, uint64_t run) {
    uint64_t n258; unsigned tail;
    split_run((run - 1) * (uint64_t)E, n258, tail);
    uint64_t bits = n258 * (uint64_t)(cs.lit_len[285] + cs.dlen);
    for (int b = 0; b < E; ++b) bits += cs.lit_len[P[b]];
    if (tail > 258) bits += match_bits(cs, (int)tail - 3) + match_bits(cs, 3);
    else if (tail >= 3) bits += match_bits(cs, (int)tail);
    else for (unsigned b = 0; b < tail; ++b) bits += cs.lit_len[P[b % E]];
    return bits;
}

template <class S>
UKBB_HD void emit_match(S &s, const CodeSet &cs, int len) {               // (length, distance E)
    int sym, xb, xv;
    length_code(len, sym, xb, xv);
    s.put(cs.lit_bits[sym], cs.lit_len[sym]);
    if (xb) s.put((uint32_t)xv, xb);
    s.put(cs.dbits, cs.dlen);
}
// what follows the opening literals: n258 (258, E) tokens through s.fill258, then the tail
template <class S>
UKBB_HD void emit_run_body(S &s, const CodeSet &cs, const uint8_t *P, int E, uint64_t run) {
    uint64_t n258; unsigned tail;
    split_run((run - 1) * (uint64_t)E, n258, tail);
    if (n258) { uint32_t tok; int len; token258(cs, tok, len); s.fill258(n258, tok, len); }
    if (tail > 258) { emit_match(s, cs, (int)tail - 3); emit_match(s, cs, 3); }
    else if (tail >= 3) emit_match(s, cs, (int)tail);
    else for (unsigned b = 0; b < tail; ++b) s.put(cs.lit_bits[P[b % E]], cs.lit_len[P[b % E]]);
}
template <class S>
UKBB_HD void emit_run(S &s, const CodeSet &cs, const uint8_t *P, int E, uint64_t run) {
    for (int b = 0; b < E; ++b) s.put(cs.lit_bits[P[b]], cs.lit_len[P[b]]);
    emit_run_body(s, cs, P, E, run);
}

// ---- the head of the member: gzip header, BFINAL, block header, the prefix as literals; and the prefix's CRC register ------------------------
// w: put(value, bits).  lit: the finished histogram (DYNAMIC only).  Returns the CRC register behind the prefix (started from 0xFFFFFFFF).
template <class W>
UKBB_HD uint32_t emit_head(W &w, int mode, const uint64_t *lit, int E, const uint8_t *prefix, uint64_t prefix_len, CodeSet &cs, HeaderWork &k) {
    // gzip header as Python's GzipFile(filename='', mtime=0, compresslevel=1) writes it (ukbb_cardiac_amd/nifti.py)
    w.put(0x1f, 8); w.put(0x8b, 8); w.put(8, 8); w.put(0, 8); w.put(0, 32); w.put(4, 8); w.put(0xff, 8);
    w.put(1, 1);                                       // BFINAL
    if (mode == FIXED) { w.put(1, 2); fixed_codes(E, cs); }   // BTYPE = 01, fixed Huffman
    else dynamic_codes(lit, E, cs, k, w);
    uint32_t reg = 0xFFFFFFFFu;
    for (uint64_t i = 0; i < prefix_len; ++i) { const uint8_t b = prefix[i]; w.put(cs.lit_bits[b], cs.lit_len[b]); reg = crc_byte(reg, b); }
    return reg;
}
// upper bound of the head's bits: 80 + 3 + 14 + 19 * 3 + (286 + 30) * (7 + 7) + 15 per prefix byte
UKBB_HD constexpr uint64_t head_bits_bound(uint64_t prefix_len) { return 80 + 3 + 14 + 57 + 316 * 14 + 15 * prefix_len; }

// bits accumulated in 32-bit words (the head on the device and in the parallel host formulation)
struct WordSink {
    uint32_t *words;                                   // zeroed by the caller
    uint64_t pos;
    UKBB_HD void put(uint32_t v, int bits) {
        if (!bits) return;
        const uint64_t x = (uint64_t)v << (pos & 31);
        words[pos >> 5] |= (uint32_t)x;
        if (x >> 32) words[(pos >> 5) + 1] |= (uint32_t)(x >> 32);
        pos += (uint64_t)bits;
    }
};

}  // namespace ukbb_labelgz
