// gzip writer for label volumes (host only, no HIP).
//
// The sequence loop of the reference ends with nib.save of np.zeros(image.shape) filled with the predicted labels
// (common/deploy_network.py:92,116,136-138): 160 MB of float64 per short-axis subject whose voxels take one of <= 4 values,
// pushed through zlib.  With the network at 11 ms per subject that deflate (0.5 s of a core at nibabel's level 1) is what a
// deployment waits for.  This encoder writes the SAME uncompressed stream -- header bytes followed by the labels converted
// to the file's voxel type -- as one gzip member without ever forming it: a run of equal labels is a run of equal E-byte
// patterns, i.e. E literals followed by deflate matches of distance E (RFC 1951), and the CRC-32 of a run of zero bytes is a
// multiplication by x^(8n) in GF(2)[x]/P.  Any inflater (nibabel, zlib's gzread, MIRTK) reads the result as the file the
// reference writes.
//
// Two code sets for the same token stream: UKBB_GZIP_FIXED (BTYPE 01: 14 bits per 258 bytes of float64, ~80 bits per
// short run) and UKBB_GZIP_DYNAMIC (BTYPE 10, the default): one counting pass over the runs gives the exact token
// histogram, from which a length-limited Huffman code is built -- the handful of byte values a label pattern consists of
// and the one distance in use then cost 1-3 bits each, which brings the file to the size zlib level 1 reaches on the
// same volume (r03: smaller on every volume tried) for one extra 20 MB read.
// The per-run arithmetic -- element patterns, the split of a run into tokens, length symbols, the Huffman builder and block header, the
// GF(2) helpers and the closed-form CRC of a run -- is label_gzip_core.h, one text with the device encoder (kernels_labelgz.hip).  This
// file keeps the serial walk (table-driven CRC, packed tokens) and runs the parallel formulation serially for tests.
#include "../../include/ukbb_fcn.h"
#include "label_gzip_core.h"

#include <cstdint>
#include <cstring>
#include <vector>

namespace {

using ukbb_labelgz::POLY;

struct Tables {
    uint32_t crc[8][256];                              // slicing-by-8
    uint32_t x2n[32];                                  // x^(2^k) mod P, reflected
    uint16_t len_sym[259]; uint8_t len_xbits[259]; uint16_t len_xval[259];
    Tables() {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = c & 1 ? (c >> 1) ^ POLY : c >> 1;
            crc[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; ++i)
            for (int t = 1; t < 8; ++t) crc[t][i] = (crc[t - 1][i] >> 8) ^ crc[0][crc[t - 1][i] & 0xff];
        ukbb_labelgz::x2n_fill(x2n);
        for (int l = 3; l <= 258; ++l) {
            int s, xb, xv;
            ukbb_labelgz::length_code(l, s, xb, xv);
            len_sym[l] = (uint16_t)s; len_xbits[l] = (uint8_t)xb; len_xval[l] = (uint16_t)xv;
        }
    }
    uint32_t shift_zero_bytes(uint32_t reg, uint64_t nbytes) const { return ukbb_labelgz::shift_zero_bytes(x2n, reg, nbytes); }
};
const Tables &tables() { static const Tables t; return t; }

struct BitWriter {
    uint8_t *p, *end;
    uint64_t acc = 0;
    int n = 0;
    bool overflow = false;
    inline void put(uint32_t v, int bits) {
        acc |= (uint64_t)v << n;
        n += bits;
        if (n >= 32) {
            if (end - p >= 4) { memcpy(p, &acc, 4); p += 4; } else { overflow = true; }
            acc >>= 32; n -= 32;
        }
    }
    void finish() {
        while (n > 0) { if (p < end) *p++ = (uint8_t)acc; else overflow = true; acc >>= 8; n -= 8; }
        n = 0;
    }
};

inline uint32_t crc_bytes(const Tables &t, uint32_t reg, const uint8_t *b, size_t n) {
    while (n >= 8) {
        uint32_t lo, hi;
        memcpy(&lo, b, 4); memcpy(&hi, b + 4, 4);
        lo ^= reg;
        reg = t.crc[7][lo & 0xff] ^ t.crc[6][(lo >> 8) & 0xff] ^ t.crc[5][(lo >> 16) & 0xff] ^ t.crc[4][lo >> 24] ^
              t.crc[3][hi & 0xff] ^ t.crc[2][(hi >> 8) & 0xff] ^ t.crc[1][(hi >> 16) & 0xff] ^ t.crc[0][hi >> 24];
        b += 8; n -= 8;
    }
    while (n--) reg = (reg >> 8) ^ t.crc[0][(reg ^ *b++) & 0xff];
    return reg;
}

using ukbb_labelgz::CodeSet;
using ukbb_labelgz::element_pattern;

// Walks the runs of equal labels: f(v, run_length) per run, in order.
template <class F>
inline void for_each_run(const uint8_t *labels, uint64_t n_voxels, F &&f) {
    uint64_t i = 0;
    while (i < n_voxels) {
        const uint8_t v = labels[i];
        uint64_t j = i + 1;
        const uint64_t splat = 0x0101010101010101ull * v;   // end of the run: bytes, then 8 at a time, then bytes
        while (j < n_voxels && (j & 7) && labels[j] == v) ++j;
        if (j < n_voxels && !(j & 7)) {
            uint64_t wv;
            while (j + 8 <= n_voxels && (memcpy(&wv, labels + j, 8), wv == splat)) j += 8;
            while (j < n_voxels && labels[j] == v) ++j;
        }
        f(v, j - i);
        i = j;
    }
}

}  // namespace

extern "C" {

uint64_t ukbb_fcn_gzip_labels_bound(uint64_t n_voxels, int nifti_datatype, uint64_t prefix_len) {
    uint8_t tmp[8];
    const int e = element_pattern(nifti_datatype, 0, tmp);
    const uint64_t raw = prefix_len + n_voxels * (uint64_t)(e ? e : 8);
    return raw * 2 + 1024;                             // <= 15 bits per literal byte, block header, trailer, bit-buffer slack
}

int64_t ukbb_fcn_gzip_labels_mode(const uint8_t *labels, uint64_t n_voxels, int nifti_datatype, const uint8_t *prefix, uint64_t prefix_len,
                                  uint8_t *out, uint64_t out_cap, int mode) {
    if ((!labels && n_voxels) || (!prefix && prefix_len) || !out) return UKBB_EINVAL;
    if (mode != UKBB_GZIP_FIXED && mode != UKBB_GZIP_DYNAMIC) return UKBB_EINVAL;
    uint8_t pat[256][8];
    uint8_t probe[8];
    const int E = element_pattern(nifti_datatype, 0, probe);
    if (!E) return UKBB_EINVAL;
    if (out_cap < 512) return UKBB_ENOMEM;
    for (unsigned v = 0; v < 256; ++v) element_pattern(nifti_datatype, v, pat[v]);
    const Tables &t = tables();
    CodeSet cs;
    // gzip header as Python's GzipFile(filename='', mtime=0, compresslevel=1) writes it (ukbb_cardiac_amd/nifti.py)
    static const uint8_t head[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 4, 0xff};
    memcpy(out, head, 10);
    BitWriter w{out + 10, out + out_cap - 8};
    w.put(1, 1);                                       // BFINAL
    if (mode == UKBB_GZIP_FIXED) {
        w.put(1, 2);                                   // BTYPE = 01, fixed Huffman
        ukbb_labelgz::fixed_codes(E, cs);
    } else {
        // ---- pass 1: the exact histogram of the tokens pass 2 will write, then the codes and the block header ----
        uint64_t runs[256] = {0}, lit[288] = {0};
        auto add = [&](int s, uint64_t c) { lit[s] += c; };
        for (uint64_t i = 0; i < prefix_len; ++i) ++lit[prefix[i]];
        for_each_run(labels, n_voxels, [&](uint8_t v, uint64_t run) {
            ++runs[v];
            ukbb_labelgz::run_tail_histogram(pat[v], E, run, add);
        });
        for (unsigned v = 0; v < 256; ++v)
            if (runs[v]) ukbb_labelgz::run_open_histogram(pat[v], E, runs[v], add);
        lit[256] = 1;                                  // end of block
        ukbb_labelgz::HeaderWork hw;
        ukbb_labelgz::dynamic_codes(lit, E, cs, hw, w);
    }
    auto literal = [&](uint8_t b) { w.put(cs.lit_bits[b], cs.lit_len[b]); };
    // (258, E) tokens, several to a 32-bit piece
    const int tok258_len = cs.lit_len[285] + cs.dlen;
    const uint32_t tok258 = (uint32_t)cs.lit_bits[285] | (cs.dbits << cs.lit_len[285]);
    int pack_n = 32 / (tok258_len ? tok258_len : 1);
    if (pack_n < 1) pack_n = 1;
    uint32_t pack258 = 0;
    for (int k = 0; k < pack_n && pack_n * tok258_len <= 32; ++k) pack258 |= tok258 << (k * tok258_len);
    struct Chunk { uint32_t bits; int len; };
    struct Sink {                                      // the core's emission into the bit writer; (258, E) tokens go out packed
        BitWriter &w; int pack_n, tok258_len; uint32_t pack258;
        void put(uint32_t v, int bits) { w.put(v, bits); }
        void fill258(uint64_t n258, uint32_t tok258, int) {
            for (; n258 >= (uint64_t)pack_n; n258 -= pack_n) w.put(pack258, pack_n * tok258_len);
            for (; n258; --n258) w.put(tok258, tok258_len);
        }
    } sink{w, pack_n, tok258_len, pack258};
    Chunk first_tok[256][5];                           // the E literals that open a run of label v, packed into <= 32-bit pieces
    int first_n[256];
    bool have[256] = {false};
    uint32_t reg = 0xFFFFFFFFu;
    for (uint64_t i = 0; i < prefix_len; ++i) literal(prefix[i]);
    reg = crc_bytes(t, reg, prefix, (size_t)prefix_len);
    bool overflow = false;
    for_each_run(labels, n_voxels, [&](uint8_t v, uint64_t run) {
        if (overflow) return;
        if (!have[v]) {
            have[v] = true;
            int nchunk = 0;
            Chunk c{0, 0};
            for (int b = 0; b < E; ++b) {
                const uint32_t lb = cs.lit_bits[pat[v][b]];
                const int ll = cs.lit_len[pat[v][b]];
                if (c.len + ll > 32) { first_tok[v][nchunk++] = c; c = Chunk{0, 0}; }
                c.bits |= lb << c.len; c.len += ll;
            }
            first_tok[v][nchunk++] = c;
            first_n[v] = nchunk;
        }
        const uint8_t *P = pat[v];
        // ---- deflate tokens ----
        for (int c = 0; c < first_n[v]; ++c) w.put(first_tok[v][c].bits, first_tok[v][c].len);
        ukbb_labelgz::emit_run_body(sink, cs, P, E, run);
        if (w.overflow) { overflow = true; return; }
        // ---- CRC-32 of the run ----
        bool zero = true;
        for (int b = 0; b < E; ++b) zero = zero && P[b] == 0;
        const uint64_t nbytes = run * (uint64_t)E;
        if (zero && nbytes >= 512) reg = t.shift_zero_bytes(reg, nbytes);
        else if (E == 8) {
            uint32_t lo0, hi;
            memcpy(&lo0, P, 4); memcpy(&hi, P + 4, 4);
            const uint32_t h = t.crc[3][hi & 0xff] ^ t.crc[2][(hi >> 8) & 0xff] ^ t.crc[1][(hi >> 16) & 0xff] ^ t.crc[0][hi >> 24];
            for (uint64_t k = 0; k < run; ++k) {
                const uint32_t lo = lo0 ^ reg;
                reg = t.crc[7][lo & 0xff] ^ t.crc[6][(lo >> 8) & 0xff] ^ t.crc[5][(lo >> 16) & 0xff] ^ t.crc[4][lo >> 24] ^ h;
            }
        } else {
            for (uint64_t k = 0; k < run; ++k) reg = crc_bytes(t, reg, P, (size_t)E);
        }
    });
    if (overflow) return UKBB_ENOMEM;
    w.put(cs.lit_bits[256], cs.lit_len[256]);          // end of block
    w.finish();
    if (w.overflow) return UKBB_ENOMEM;
    uint8_t *p = w.p;
    const uint32_t crc = reg ^ 0xFFFFFFFFu;
    const uint32_t isize = (uint32_t)((prefix_len + n_voxels * (uint64_t)E) & 0xFFFFFFFFull);
    memcpy(p, &crc, 4); memcpy(p + 4, &isize, 4);
    return (int64_t)(p + 8 - out);
}

int64_t ukbb_fcn_gzip_labels(const uint8_t *labels, uint64_t n_voxels, int nifti_datatype, const uint8_t *prefix, uint64_t prefix_len,
                             uint8_t *out, uint64_t out_cap) {
    return ukbb_fcn_gzip_labels_mode(labels, n_voxels, nifti_datatype, prefix, prefix_len, out, out_cap, UKBB_GZIP_DYNAMIC);
}

// The formulation the device encoder runs (kernels_labelgz.hip), step by step and serially: run table, histogram, codes and head,
// per-run bit counts and their exclusive scan, capacity check, every run written at its own bit offset (in no particular order: OR
// onto zeroed bytes), closed-form CRC pieces joined in order.  Nothing is written unless the whole member fits out_cap.
int64_t ukbb_fcn_gzip_labels_parallel_host(const uint8_t *labels, uint64_t n_voxels, int nifti_datatype, const uint8_t *prefix,
                                           uint64_t prefix_len, int mode, uint8_t *out, uint64_t out_cap, uint64_t max_runs) {
    using namespace ukbb_labelgz;
    uint8_t P[8];
    const int E = element_pattern(nifti_datatype, 0, P);
    if (!labels || !out || (!prefix && prefix_len) || !E || (mode != UKBB_GZIP_FIXED && mode != UKBB_GZIP_DYNAMIC) || n_voxels < 1 ||
        n_voxels > UKBB_LABELGZ_MAX_VOXELS || prefix_len > UKBB_LABELGZ_MAX_PREFIX || max_runs < 1)
        return UKBB_EINVAL;
    // 1. runs: a voxel starts one when it differs from its predecessor
    uint64_t n_runs = 0;
    for (uint64_t i = 0; i < n_voxels; ++i) n_runs += i == 0 || labels[i] != labels[i - 1];
    if (n_runs > max_runs) return UKBB_LABELGZ_TOO_MANY_RUNS;
    std::vector<uint32_t> start((size_t)n_runs);
    for (uint64_t i = 0, r = 0; i < n_voxels; ++i) if (i == 0 || labels[i] != labels[i - 1]) start[(size_t)r++] = (uint32_t)i;
    auto run_len = [&](uint64_t r) { return (r + 1 < n_runs ? start[(size_t)r + 1] : n_voxels) - start[(size_t)r]; };
    // 2. histogram
    uint64_t lit[288] = {0};
    auto add = [&](int s, uint64_t c) { lit[s] += c; };
    if (mode == UKBB_GZIP_DYNAMIC) {
        for (uint64_t r = 0; r < n_runs; ++r) {
            element_pattern(nifti_datatype, labels[start[(size_t)r]], P);
            run_open_histogram(P, E, 1, add);
            run_tail_histogram(P, E, run_len(r), add);
        }
        for (uint64_t i = 0; i < prefix_len; ++i) ++lit[prefix[i]];
        lit[256] = 1;
    }
    // 3. codes and head
    std::vector<uint32_t> head_words((size_t)(head_bits_bound(prefix_len) / 32 + 2), 0u);
    WordSink head{head_words.data(), 0};
    CodeSet cs;
    HeaderWork hw;
    uint32_t x2n[32];
    x2n_fill(x2n);
    const uint32_t reg0 = emit_head(head, mode, lit, E, prefix, prefix_len, cs, hw);
    // 4. bit offsets
    std::vector<uint64_t> off((size_t)n_runs + 1);
    off[0] = head.pos;
    for (uint64_t r = 0; r < n_runs; ++r) {
        element_pattern(nifti_datatype, labels[start[(size_t)r]], P);
        off[(size_t)r + 1] = off[(size_t)r] + run_bits(cs, P, E, run_len(r));
    }
    // 5. capacity, then emission
    const uint64_t total_bits = off[(size_t)n_runs] + cs.lit_len[256];
    const uint64_t len = (total_bits + 7) / 8 + 8;
    if (len > out_cap) return UKBB_LABELGZ_NO_ROOM;
    memset(out, 0, (size_t)len);
    memcpy(out, head_words.data(), (size_t)((head.pos + 7) / 8));
    struct ByteSink {
        uint8_t *out; uint64_t pos;
        void put(uint32_t v, int bits) {
            uint64_t x = (uint64_t)v << (pos & 7);
            for (uint64_t i = pos >> 3; x; ++i, x >>= 8) out[i] |= (uint8_t)x;
            pos += (uint64_t)bits;
        }
        void fill258(uint64_t n, uint32_t tok, int len) { for (; n; --n) put(tok, len); }
    };
    CrcPiece all = crc_identity();
    for (uint64_t k = n_runs; k-- > 0;) {              // back to front: the order does not matter
        element_pattern(nifti_datatype, labels[start[(size_t)k]], P);
        ByteSink s{out, off[(size_t)k]};
        emit_run(s, cs, P, E, run_len(k));
        if (s.pos != off[(size_t)k + 1]) return UKBB_EINVAL;   // run_bits and emit_run disagree: cannot happen
    }
    for (uint64_t r = 0; r < n_runs; ++r) {
        element_pattern(nifti_datatype, labels[start[(size_t)r]], P);
        all = crc_join(all, crc_pattern_run(x2n, P, E, run_len(r)));
    }
    // 6. end of block, CRC-32 and ISIZE
    ByteSink s{out, off[(size_t)n_runs]};
    s.put(cs.lit_bits[256], cs.lit_len[256]);
    const uint32_t crc = (mult(all.pw, reg0) ^ all.c) ^ 0xFFFFFFFFu;
    const uint32_t isize = (uint32_t)((prefix_len + n_voxels * (uint64_t)E) & 0xFFFFFFFFull);
    memcpy(out + len - 8, &crc, 4); memcpy(out + len - 4, &isize, 4);
    return (int64_t)len;
}

}  // extern "C"
