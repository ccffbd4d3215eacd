// Raw-deflate (RFC 1951) decoder core, ONE text for the host and for the gfx950 kernel (kernels_inflate.hip): bit reader, code-length
// parsing, canonical table builder and symbol loop are plain C++ behind UKBB_HD.  gz_inflate.cpp stays the host reader of the deploy
// loops (64-bit unchecked fast loop, 43 KB of tables); this one is built for a wave that decodes one stream next to hundreds of others:
//   * every access to the input and the output goes through an `Io` policy that checks it against src_len / dst_cap -- the host policy
//     (HostIo below) reads and writes memory directly, the device policy (kernels_inflate.hip) stages input through LDS, keeps the last
//     32 KB of output in an LDS ring and copies matches with all lanes;
//   * the tables are small enough for LDS: a 10-bit first level for literal / length codes and an 8-bit one for distances, second-level
//     tables sized by the longest code under their prefix.  A second-level table of 2^k entries holds a complete subtree with a leaf at
//     depth k, hence at least k + 1 symbols; with k <= 15 - root that bounds all second-level entries by 47 * 32 + 8 = 1512 (286
//     symbols, root 10) and 3 * 128 + 32 = 416 (30 symbols, root 8).  The builder checks the bound all the same;
//   * strictness and error classes are those of gz_inflate.cpp: -1 out of input, -2 invalid stream, -3 does not fit the output.
// Work (all tables and scratch arrays) is 15.0 KB: __shared__ in the kernel, on the stack on the host.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define UKBB_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define UKBB_HD inline
#endif

namespace ukbb_inflate {

enum { E_INPUT = -1, E_DATA = -2, E_OUTPUT = -3 };

constexpr int LL_ROOT = 10, D_ROOT = 8, PRE_ROOT = 7;
constexpr int LL_SIZE = (1 << LL_ROOT) + 1512, D_SIZE = (1 << D_ROOT) + 416;

// Table entry: bits 0-4 code bits this lookup drops, bits 5-8 extra-bit count (second-level pointer: index bits of that table), bits 9-12
// kind, bits 16-31 base value (literal, length base, distance base, code-length symbol, or second-level table start).
constexpr uint32_t K_LIT = 1u << 9, K_SUB = 1u << 10, K_EOB = 1u << 11, K_BAD = 1u << 12;
UKBB_HD uint32_t mk(uint32_t base, uint32_t extra, uint32_t len, uint32_t kind) { return (base << 16) | kind | (extra << 5) | len; }

struct Work {
    uint32_t ll[LL_SIZE];
    uint32_t d[D_SIZE];
    uint32_t pre[1 << PRE_ROOT];
    uint16_t codes[320];
    uint16_t count[16], next[16];
    uint8_t lens[320];
    uint8_t sub_bits[1 << LL_ROOT];
    int32_t status;
};

UKBB_HD uint32_t bitrev(uint32_t v, int n) {               // the low n <= 16 bits of v, reversed
    v = ((v & 0x5555u) << 1) | ((v >> 1) & 0x5555u);
    v = ((v & 0x3333u) << 2) | ((v >> 2) & 0x3333u);
    v = ((v & 0x0f0fu) << 4) | ((v >> 4) & 0x0f0fu);
    v = ((v & 0x00ffu) << 8) | ((v >> 8) & 0x00ffu);
    return v >> (16 - n);
}

// base value and extra bits of length symbol 257 + c (c < 29) and of distance symbol d (d < 30): RFC 1951 3.2.5 as arithmetic
UKBB_HD uint32_t len_extra(uint32_t c) { return c < 8 || c == 28 ? 0 : (c - 4) >> 2; }
UKBB_HD uint32_t len_base(uint32_t c) { return c < 8 ? 3 + c : c == 28 ? 258 : 3 + ((4 + (c & 3)) << ((c - 4) >> 2)); }
UKBB_HD uint32_t dist_extra(uint32_t d) { return d < 4 ? 0 : (d - 2) >> 1; }
UKBB_HD uint32_t dist_base(uint32_t d) { return d < 4 ? d + 1 : 1 + ((2 + (d & 1)) << ((d - 2) >> 1)); }

// kind: 0 literal / length alphabet, 1 distance alphabet, 2 code-length alphabet
UKBB_HD uint32_t table_entry(int kind, uint32_t sym, uint32_t drop) {
    if (kind == 2) return mk(sym, 0, drop, 0);
    if (kind == 1) return sym < 30 ? mk(dist_base(sym), dist_extra(sym), drop, 0) : mk(0, 0, drop, K_BAD);
    if (sym < 256) return mk(sym, 0, drop, K_LIT);
    if (sym == 256) return mk(0, 0, drop, K_EOB);
    return sym < 286 ? mk(len_base(sym - 257), len_extra(sym - 257), drop, 0) : mk(0, 0, drop, K_BAD);
}

// Canonical Huffman code of `n` symbols with lengths lens[] (0 = unused, <= 15) -> two-level decode table of `cap` entries.
// Returns 0, or -1 for an over-subscribed or (other than the one length-1 distance code RFC 1951 allows) incomplete code.
// The serial steps run in the leader lane, the fills are spread over the lanes (one lane on the host).
template <class Io>
UKBB_HD int build_table(Io &io, Work &w, const uint8_t *lens, int n, int kind, uint32_t *tab, int root, int cap) {
    const int nroot = 1 << root;
    if (io.leader()) {
        int st = 0;                                         // < 0 refused; bit 0: fill the first level with K_BAD first; bit 1: no code at all; bit 2: long codes
        for (int l = 0; l < 16; ++l) w.count[l] = 0;
        for (int i = 0; i < n; ++i) ++w.count[lens[i]];
        const int used = n - w.count[0];
        int left = 1;                                       // Kraft sum bookkeeping, as a count of unassigned codes
        for (int l = 1; l <= 15; ++l) { left = (left << 1) - w.count[l]; if (left < 0) { st = -1; break; } }
        if (st == 0 && left > 0) {
            // only "at most one distance code" may be incomplete, and that one code has length 1 (as zlib's inflate_table demands)
            if (kind == 1 && (used == 0 || (used == 1 && w.count[1] == 1))) st = used ? 1 : 3;
            else st = -1;
        }
        if (st >= 0 && used) {
            uint32_t nx = 0;
            w.next[0] = 0; w.next[1] = 0;
            for (int l = 1; l < 15; ++l) { nx = (nx + w.count[l]) << 1; w.next[l + 1] = (uint16_t)nx; }
            for (int s = 0; s < n; ++s) {
                const int l = lens[s];
                w.codes[s] = l ? (uint16_t)bitrev(w.next[l]++, l) : 0;
                if (l > root) st |= 4;
            }
        }
        w.status = st;
    }
    io.sync();
    int st = io.uni(w.status);
    if (st < 0) return -1;
    if (st & 1) for (int i = io.lane(); i < nroot; i += io.lanes()) tab[i] = mk(0, 0, 1, K_BAD);
    if (st & 4) for (int i = io.lane(); i < nroot; i += io.lanes()) w.sub_bits[i] = 0;
    io.sync();
    if (st & 2) return 0;                                   // literals only: any distance code is an error when met
    if (st & 4) {
        // second-level tables: one per root-bit prefix that long codes share, sized by the longest code under that prefix.  An incomplete
        // code cannot reach here (the one allowed has length 1 <= root), so every second-level slot gets filled below.
        if (io.leader()) {
            for (int s = 0; s < n; ++s) {
                const int l = lens[s];
                if (l > root) { const uint32_t p = w.codes[s] & (nroot - 1); if (l - root > w.sub_bits[p]) w.sub_bits[p] = (uint8_t)(l - root); }
            }
            int base = nroot, ok = 0;
            for (int s = 0; s < n; ++s) {
                if (lens[s] <= root) continue;
                const uint32_t p = w.codes[s] & (nroot - 1);
                if (w.sub_bits[p] & 0x80) continue;         // this prefix has its table
                const int sb = w.sub_bits[p];
                if (base + (1 << sb) > cap) { ok = -1; break; }   // cannot happen (bound in the header comment); never write past the table
                tab[p] = mk((uint32_t)base, (uint32_t)sb, (uint32_t)root, K_SUB);
                w.sub_bits[p] = (uint8_t)(sb | 0x80);
                base += 1 << sb;
            }
            w.status = ok;
        }
        io.sync();
        if (io.uni(w.status) < 0) return -1;
    }
    for (int s = io.lane(); s < n; s += io.lanes()) {
        const int l = lens[s];
        if (!l) continue;
        const uint32_t code = w.codes[s];
        if (l <= root) {
            const uint32_t e = table_entry(kind, (uint32_t)s, (uint32_t)l);
            for (uint32_t i = code; i < (uint32_t)nroot; i += 1u << l) tab[i] = e;
        } else {
            const uint32_t p = code & (nroot - 1);
            const uint32_t b = tab[p] >> 16, sb = w.sub_bits[p] & 0x7f;
            const uint32_t e = table_entry(kind, (uint32_t)s, (uint32_t)(l - root));
            for (uint32_t i = code >> root; i < (1u << sb); i += 1u << (l - root)) tab[b + i] = e;
        }
    }
    io.sync();
    return 0;
}

// Bit reader over Io: a 64-bit buffer refilled 32 bits at a time from 4-byte aligned input words (io.in_word), bytes at the unaligned
// start (io.in_byte), zeros beyond the end.  `in` is the index of the next byte to load; consumed bits = 8 * in - cnt, and a caller that
// has consumed more than 8 * src_len bits has read padding: overrun().
template <class Io>
struct Bits {
    Io &io;
    const uint64_t src_len;
    uint64_t buf = 0, in = 0;
    uint32_t cnt = 0;
    UKBB_HD Bits(Io &io_, uint64_t n) : io(io_), src_len(n) {}
    UKBB_HD void start(uint64_t at) {                      // (re)start at byte `at`: single bytes up to the next aligned word
        buf = 0; cnt = 0; in = at;
        while ((io.in_align() + in) & 3) {
            if (in < src_len) buf |= (uint64_t)io.in_byte(in) << cnt;
            ++in; cnt += 8;
        }
    }
    UKBB_HD void refill() {                                // afterwards cnt >= 33: one literal / length code + extra (20), or one distance code + extra (28)
        if (cnt <= 32) {
            uint32_t v = 0;
            if (in + 4 <= src_len) v = io.in_word(in);
            else for (int k = 0; k < 4; ++k) if (in + k < src_len) v |= io.in_byte(in + k) << (8 * k);
            buf |= (uint64_t)v << cnt;
            cnt += 32; in += 4;
        }
    }
    UKBB_HD uint32_t peek(uint32_t n) const { return (uint32_t)buf & ((1u << n) - 1); }
    UKBB_HD uint32_t take(uint32_t n) { const uint32_t v = peek(n); buf >>= n; cnt -= n; return v; }
    UKBB_HD bool overrun() const { return in * 8 - cnt > src_len * 8; }
};

// One raw deflate stream of exactly src_len bytes through `io` into an output of dst_cap bytes.  Returns the bytes written or E_*
// (E_DATA also when the last block ends before byte src_len - 1).
// Io: in_align(), in_byte(i), in_word(i) (i + 4 <= src_len, 4-byte aligned address), put_byte(b), copy_match(dist, len),
// copy_stored(in, len), finish(), leader(), lane(), lanes(), sync(), uni(v) (v is the same in every lane: lets the device keep it scalar).
// The caller has checked nothing: every length and distance is checked here before Io is asked to move a byte.
template <class Io>
UKBB_HD int64_t inflate_core(Io &io, Work &w, const uint64_t src_len, const uint64_t dst_cap) {
    Bits<Io> b(io, src_len);
    b.start(0);
    uint64_t pos = 0;
    bool last;
    // Every iteration of every loop below consumes at least one input bit (3 per block header, >= 1 per code: table entries, K_BAD ones
    // included, drop >= 1 bit) or ends the stream, and a stream that has consumed more than 8 * src_len bits ends with E_INPUT; stored
    // blocks copy bytes they have checked to be there.  So the iteration count is bounded by 8 * src_len + 8 plus the output size: no
    // spins, no waiting on another workgroup.
    do {
        b.refill();
        last = b.take(1);
        const uint32_t type = b.take(2);
        if (b.overrun()) return E_INPUT;
        if (type == 0) {                                    // stored: drop to a byte boundary, LEN / NLEN, raw bytes
            b.take(b.cnt & 7);
            uint64_t in = b.in - (b.cnt >> 3);              // whole bytes still in the bit buffer go back (<= src_len: no overrun above)
            if (src_len - in < 4) return E_INPUT;
            const uint32_t len = io.in_byte(in) | (io.in_byte(in + 1) << 8), nlen = io.in_byte(in + 2) | (io.in_byte(in + 3) << 8);
            if ((len ^ nlen) != 0xffff) return E_DATA;
            in += 4;
            if (src_len - in < len) return E_INPUT;
            if (dst_cap - pos < len) return E_OUTPUT;
            io.copy_stored(in, len);
            pos += len;
            b.start(in + len);
            continue;
        }
        if (type == 3) return E_DATA;
        if (type == 1) {
            if (io.leader()) {
                for (int i = 0; i < 144; ++i) w.lens[i] = 8;
                for (int i = 144; i < 256; ++i) w.lens[i] = 9;
                for (int i = 256; i < 280; ++i) w.lens[i] = 7;
                for (int i = 280; i < 288; ++i) w.lens[i] = 8;
                for (int i = 288; i < 320; ++i) w.lens[i] = 5;
            }
            io.sync();
            build_table(io, w, w.lens, 288, 0, w.ll, LL_ROOT, LL_SIZE);
            build_table(io, w, w.lens + 288, 32, 1, w.d, D_ROOT, D_SIZE);
        } else {
            const int hlit = (int)b.take(5) + 257, hdist = (int)b.take(5) + 1, hclen = (int)b.take(4) + 4;
            if (hlit > 286 || hdist > 30) return E_DATA;
            if (io.leader()) for (int i = 0; i < 19; ++i) w.lens[i] = 0;
            for (int i = 0; i < hclen; ++i) {
                b.refill();
                const uint32_t v = b.take(3);
                // the order of RFC 1951 3.2.7 (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15) as arithmetic
                const int o = i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? 10 - ((i + 1) >> 1) : 6 + (i >> 1);
                if (io.leader()) w.lens[o] = (uint8_t)v;
            }
            if (b.overrun()) return E_INPUT;
            io.sync();
            // zlib rejects an incomplete code-length code too (unless a single code: rare, and the callers fall back to zlib)
            if (build_table(io, w, w.lens, 19, 2, w.pre, PRE_ROOT, 1 << PRE_ROOT)) return E_DATA;
            const int total = hlit + hdist;
            int i = 0;
            uint32_t prev = 0;
            while (i < total) {
                b.refill();
                const uint32_t e = io.uni(w.pre[b.peek(PRE_ROOT)]);
                b.take(e & 31);
                const uint32_t sym = e >> 16;
                if (b.overrun()) return E_INPUT;
                if (sym < 16) { if (io.leader()) w.lens[i] = (uint8_t)sym; prev = sym; ++i; continue; }
                int rep; uint32_t v = 0;
                if (sym == 16) { if (i == 0) return E_DATA; v = prev; rep = 3 + (int)b.take(2); }
                else if (sym == 17) rep = 3 + (int)b.take(3);
                else rep = 11 + (int)b.take(7);
                if (i + rep > total) return E_DATA;
                if (io.leader()) for (int k = 0; k < rep; ++k) w.lens[i + k] = (uint8_t)v;
                prev = v; i += rep;
            }
            if (b.overrun()) return E_INPUT;
            io.sync();
            if (io.uni(w.lens[256]) == 0) return E_DATA;   // no end-of-block code
            if (build_table(io, w, w.lens, hlit, 0, w.ll, LL_ROOT, LL_SIZE) || build_table(io, w, w.lens + hlit, hdist, 1, w.d, D_ROOT, D_SIZE))
                return E_DATA;
        }
        for (;;) {
            b.refill();
            uint32_t e = io.uni(w.ll[b.peek(LL_ROOT)]);
            if (e & K_SUB) { b.take(LL_ROOT); e = io.uni(w.ll[(e >> 16) + b.peek((e >> 5) & 15)]); }
            b.take(e & 31);
            if (e & K_LIT) {
                if (b.overrun()) return E_INPUT;
                if (pos >= dst_cap) return E_OUTPUT;
                io.put_byte(e >> 16);
                ++pos;
                continue;
            }
            if (e & K_BAD) return E_DATA;
            if (b.overrun()) return E_INPUT;
            if (e & K_EOB) break;
            const uint32_t len = (e >> 16) + b.take((e >> 5) & 15);
            b.refill();
            uint32_t d = io.uni(w.d[b.peek(D_ROOT)]);
            if (d & K_SUB) { b.take(D_ROOT); d = io.uni(w.d[(d >> 16) + b.peek((d >> 5) & 15)]); }
            if (d & K_BAD) return E_DATA;
            b.take(d & 31);
            const uint32_t dist = (d >> 16) + b.take((d >> 5) & 15);
            if (b.overrun()) return E_INPUT;
            if (dist > pos) return E_DATA;                  // reaches before the first byte this stream wrote
            if (dst_cap - pos < len) return E_OUTPUT;
            io.copy_match(dist, len);
            pos += len;
        }
    } while (!last);
    // src_len is the stream, no more: what follows the last block's final byte is not this decoder's to skip (in a gzip member the
    // trailer follows at once, and gz_inflate.cpp looks for it there)
    if (((b.in * 8 - b.cnt + 7) >> 3) != src_len) return E_DATA;
    io.finish();
    return (int64_t)pos;
}

// Host policy: the input and output in memory.  The core has checked every index it passes.
struct HostIo {
    const uint8_t *src;
    uint8_t *dst;
    uint64_t pos = 0;
    HostIo(const uint8_t *s, uint8_t *d) : src(s), dst(d) {}
    uint32_t in_align() const { return (uint32_t)((uintptr_t)src & 3); }
    uint32_t in_byte(uint64_t i) const { return src[i]; }
    uint32_t in_word(uint64_t i) const { uint32_t v; memcpy(&v, src + i, 4); return v; }      // little-endian hosts only
    void put_byte(uint32_t v) { dst[pos++] = (uint8_t)v; }
    void copy_match(uint32_t dist, uint32_t len) { for (uint32_t i = 0; i < len; ++i, ++pos) dst[pos] = dst[pos - dist]; }
    void copy_stored(uint64_t in, uint32_t len) { if (len) memcpy(dst + pos, src + in, len); pos += len; }
    void finish() {}
    bool leader() const { return true; }
    int lane() const { return 0; }
    int lanes() const { return 1; }
    void sync() {}
    template <class T> T uni(T v) const { return v; }
};

// ---- CRC-32 (IEEE 802.3, reflected) as polynomial arithmetic: combining the values of two pieces ---------------------------------------
// Polynomials over GF(2) modulo P, reflected: bit 31 is x^0.  crc(A || B) = crc(A) * x^(8 |B|) mod P  xor  crc(B), for the finished
// values zlib returns as well as for the raw registers of pieces started from 0.
constexpr uint32_t CRC_POLY = 0xEDB88320u;
UKBB_HD uint32_t crc_mul(uint32_t a, uint32_t b) {         // a * b mod P
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m && a; m >>= 1) {          // <= 32 steps
        if (a & m) { p ^= b; a &= ~m; }
        b = (b >> 1) ^ (CRC_POLY & (0u - (b & 1)));
    }
    return p;
}
UKBB_HD uint32_t crc_x2n(int n) {                          // x^(2^n) mod P
    uint32_t p = 1u << 30;
    for (int i = 0; i < n; ++i) p = crc_mul(p, p);
    return p;
}
// x^(8 * bytes) mod P from x2n[k] = x^(2^k) mod P, k < 32 (the order of x divides 2^32 - 1, so x^(2^(k + 32)) = x^(2^k))
UKBB_HD uint32_t crc_xpow8(const uint32_t *x2n, uint64_t bytes) {
    uint32_t p = 1u << 31;
    for (int k = 3; bytes; bytes >>= 1, ++k) if (bytes & 1) p = crc_mul(x2n[k & 31], p);     // <= 64 steps
    return p;
}

}  // namespace ukbb_inflate
