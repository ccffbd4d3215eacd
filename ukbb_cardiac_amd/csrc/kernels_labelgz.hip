// Deflate of a label volume on the device (include/ukbb_fcn.h: ukbb_fcn_gzip_labels_device): the gzip member label_gzip.cpp writes, byte
// for byte, from labels that never leave the GPU.  The per-run arithmetic is label_gzip_core.h, the text the host writer runs; this file
// holds the launches and their helper.  No reference counterpart: the reference hands a float64 volume to nibabel / zlib
// (common/deploy_network.py:92,136-138).
//
// The chain, all on the caller's stream, nothing synchronises (a later launch sees an earlier one's stores: kernel boundaries):
//   runs_count / runs_scan / runs_compact   a voxel starts a run when it differs from its predecessor.  Two-level scan: per-workgroup
//                                           counts (VOX_BLOCK voxels each), one workgroup scans the counts, the third launch compacts
//                                           the start positions into the run table.  Runs are global, never cut at a border.  More
//                                           runs than the table holds: status = TOO_MANY_RUNS, and no index >= max_runs is written.
//   histogram (DYNAMIC)                     one run per thread, 286 bins in LDS, one integer atomic per non-empty bin and workgroup.
//   codes                                   ONE wave: lane 0 runs the shared Huffman / header text on the few dozen live symbols, the
//                                           lanes store the CodeSet, the head (gzip header, block header, prefix literals) and x^(2^k).
//   run_bits                                per-run bit count, exclusive scan inside the workgroup (64-bit), per-workgroup sums; the
//                                           per-run CRC pieces (closed form) joined in order inside the workgroup.
//   finish                                  one workgroup: scan of the sums from the head's end, ordered join of the CRC pieces, the
//                                           capacity check, end-of-block code, CRC-32, ISIZE, *d_len.
//   emit                                    a workgroup owns RUN_BLOCK consecutive runs = one bit span.  It walks the span in LDS
//                                           windows of WIN_WORDS words: every run ORs its own tokens into the window at its offset
//                                           (clipped to the window), runs of >= COOP_TOKENS (258, E) tokens are filled by all threads
//                                           as a periodic bit pattern, then whole 32-bit words go out with plain stores.  Only the
//                                           first and last word of the span, shared with the neighbours, go out with atomicOr onto
//                                           the zeroed output: OR commutes, the bytes do not depend on the order.
// Every output word an emit workgroup touches lies below the member's length, which `finish` has checked against out_cap before.
#include "../../include/ukbb_fcn.h"
#include "kernels.h"
#include "label_gzip_core.h"

using namespace ukbb;
using namespace ukbb_labelgz;

namespace {

constexpr int THREADS = 256, WAVE = 64;
constexpr int VOX_PER_THREAD = 16, VOX_BLOCK = THREADS * VOX_PER_THREAD;
constexpr int RUN_BLOCK = THREADS;
constexpr int WIN_WORDS = 4096;                         // 16 KB of LDS
constexpr int COOP_TOKENS = 32;
constexpr int MAX_GRID = 1024;                          // workgroups of the launches that loop over run blocks
constexpr int HEAD_WORDS = (int)(head_bits_bound(UKBB_LABELGZ_MAX_PREFIX) / 32 + 2);
static_assert(sizeof(CodeSet) % 4 == 0, "CodeSet is copied word by word");
static_assert((THREADS & (THREADS - 1)) == 0, "emit_kernel assigns window words to threads by their low bits");

struct Ctl {                                            // zeroed in front of every chain
    unsigned long long hist[288];
    uint32_t n_runs;
    int32_t status;                                     // 0, or the decline code
    unsigned long long base_bits;                       // where run 0 starts: behind gzip header, block header and prefix literals
    uint32_t reg0;                                      // CRC register behind the prefix
    uint32_t x2n[32];
    CodeSet cs;
};

struct Layout {                                         // the caller's scratch; the run table lies last
    uint64_t nvb, nrb, vcount, rbits, rcrc, local_off, run_start, total;
    Layout(uint64_t n, uint64_t max_runs) {
        auto up = [](uint64_t v) { return (v + 15) & ~15ull; };
        nvb = (n + VOX_BLOCK - 1) / VOX_BLOCK;
        nrb = (max_runs + RUN_BLOCK - 1) / RUN_BLOCK;
        vcount = up(sizeof(Ctl));
        rbits = vcount + up((nvb + 1) * 4);
        rcrc = rbits + up((nrb + 1) * 8);
        local_off = rcrc + up(nrb * sizeof(CrcPiece));
        run_start = local_off + up(max_runs * 8);
        total = run_start + max_runs * 4;
    }
};

template <class T>
__device__ __forceinline__ T block_exclusive_scan(T v, T *lds /* [THREADS / WAVE] */, T &total) {
    const int lane = (int)threadIdx.x & (WAVE - 1), wv = (int)threadIdx.x / WAVE;
    T inc = v;
    for (int o = 1; o < WAVE; o <<= 1) { const T t = __shfl_up(inc, o, WAVE); if (lane >= o) inc += t; }
    if (lane == WAVE - 1) lds[wv] = inc;
    __syncthreads();
    T base = 0, sum = 0;
    for (int k = 0; k < THREADS / WAVE; ++k) { if (k < wv) base += lds[k]; sum += lds[k]; }
    __syncthreads();
    total = sum;
    return base + inc - v;
}

// bit k: voxel i0 + k starts a run (k < 16, i0 + k < n)
__device__ __forceinline__ uint32_t start_flags(const uint8_t *labels, uint64_t n, uint64_t i0) {
    if (i0 >= n) return 0;
    const int cnt = n - i0 < (uint64_t)VOX_PER_THREAD ? (int)(n - i0) : VOX_PER_THREAD;
    uint32_t w[4] = {0, 0, 0, 0};
    if (cnt == VOX_PER_THREAD && (((uintptr_t)(labels + i0)) & 15) == 0) {
        const uint4 q = *reinterpret_cast<const uint4 *>(labels + i0);
        w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
    } else {
        for (int k = 0; k < cnt; ++k) w[k >> 2] |= (uint32_t)labels[i0 + k] << (8 * (k & 3));
    }
    uint32_t prev = i0 ? (uint32_t)labels[i0 - 1] : ((w[0] & 0xff) ^ 1u);       // voxel 0 always starts a run
    uint32_t flags = 0;
#pragma unroll
    for (int k = 0; k < VOX_PER_THREAD; ++k) {
        const uint32_t v = (w[k >> 2] >> (8 * (k & 3))) & 0xff;
        if (k < cnt && v != prev) flags |= 1u << k;
        prev = v;
    }
    return flags;
}

__global__ __launch_bounds__(THREADS) void runs_count_kernel(const uint8_t *labels, uint64_t n, uint32_t *vcount) {
    __shared__ uint32_t part[THREADS / WAVE];
    const uint64_t i0 = (uint64_t)blockIdx.x * VOX_BLOCK + (uint64_t)threadIdx.x * VOX_PER_THREAD;
    uint32_t total;
    (void)block_exclusive_scan<uint32_t>(__popc(start_flags(labels, n, i0)), part, total);
    if (threadIdx.x == 0) vcount[blockIdx.x] = total;
}

__global__ __launch_bounds__(THREADS) void runs_scan_kernel(uint32_t *vcount, uint64_t nvb, uint64_t max_runs, Ctl *ctl) {
    __shared__ unsigned long long part[THREADS / WAVE];
    unsigned long long running = 0;
    for (uint64_t c = 0; c < nvb; c += THREADS) {
        const uint64_t i = c + threadIdx.x;
        const unsigned long long v = i < nvb ? vcount[i] : 0;
        unsigned long long total;
        const unsigned long long ex = block_exclusive_scan<unsigned long long>(v, part, total);
        if (i < nvb) vcount[i] = (uint32_t)(running + ex);          // < n_voxels < 2^31
        running += total;
    }
    if (threadIdx.x == 0) {
        vcount[nvb] = (uint32_t)running;
        ctl->n_runs = (uint32_t)running;
        if (running > max_runs) ctl->status = UKBB_LABELGZ_TOO_MANY_RUNS;
    }
}

__global__ __launch_bounds__(THREADS) void runs_compact_kernel(const uint8_t *labels, uint64_t n, const uint32_t *vcount, const Ctl *ctl,
                                                               uint32_t *run_start, uint64_t max_runs) {
    __shared__ uint32_t part[THREADS / WAVE];
    if (ctl->status < 0) return;
    const uint64_t i0 = (uint64_t)blockIdx.x * VOX_BLOCK + (uint64_t)threadIdx.x * VOX_PER_THREAD;
    uint32_t flags = start_flags(labels, n, i0), total;
    uint64_t idx = (uint64_t)vcount[blockIdx.x] + block_exclusive_scan<uint32_t>(__popc(flags), part, total);
    while (flags) {
        const int k = __ffs(flags) - 1;
        flags &= flags - 1;
        if (idx < max_runs) run_start[idx] = (uint32_t)(i0 + k);    // status == 0 says every index is below max_runs; never write past the table all the same
        ++idx;
    }
}

struct Run { uint64_t len; uint8_t P[8]; };
__device__ __forceinline__ Run load_run(const uint8_t *labels, uint64_t n, const uint32_t *run_start, uint32_t n_runs, uint64_t r, int datatype) {
    Run q;
    const uint32_t s = run_start[r];
    q.len = (r + 1 < n_runs ? (uint64_t)run_start[r + 1] : n) - s;
    element_pattern(datatype, labels[s], q.P);
    return q;
}

__global__ __launch_bounds__(THREADS) void histogram_kernel(const uint8_t *labels, uint64_t n, const uint32_t *run_start, Ctl *ctl, int datatype, int E,
                                                            const uint8_t *prefix, uint32_t prefix_len) {
    __shared__ uint32_t h[288];
    if (ctl->status < 0) return;
    const uint32_t n_runs = ctl->n_runs;
    const uint64_t nrb = ((uint64_t)n_runs + RUN_BLOCK - 1) / RUN_BLOCK;
    for (int s = (int)threadIdx.x; s < 288; s += THREADS) h[s] = 0;
    __syncthreads();
    // a workgroup sees at most max(RUN_BLOCK, n_runs / MAX_GRID + RUN_BLOCK) runs of <= 10 literals each and <= 2^31 * 8 / 258 tokens: 32 bits do
    auto add = [&](int s, uint64_t c) { atomicAdd(&h[s], (uint32_t)c); };
    for (uint64_t blk = blockIdx.x; blk < nrb; blk += gridDim.x) {
        const uint64_t r = blk * RUN_BLOCK + threadIdx.x;
        if (r < n_runs) {
            const Run q = load_run(labels, n, run_start, n_runs, r, datatype);
            run_open_histogram(q.P, E, 1, add);
            run_tail_histogram(q.P, E, q.len, add);
        }
    }
    if (blockIdx.x == 0) {
        for (uint32_t i = threadIdx.x; i < prefix_len; i += THREADS) atomicAdd(&h[prefix[i]], 1u);
        if (threadIdx.x == 0) atomicAdd(&h[256], 1u);               // end of block
    }
    __syncthreads();
    for (int s = (int)threadIdx.x; s < 288; s += THREADS)
        if (h[s]) atomicAdd(&ctl->hist[s], (unsigned long long)h[s]);
}

__global__ __launch_bounds__(WAVE) void codes_kernel(Ctl *ctl, int mode, int E, const uint8_t *prefix, uint32_t prefix_len, uint32_t *out_words,
                                                     uint64_t out_cap) {
    __shared__ HeaderWork hw;
    __shared__ CodeSet cs;
    __shared__ uint32_t head[HEAD_WORDS];
    __shared__ uint8_t pre[UKBB_LABELGZ_MAX_PREFIX];
    __shared__ uint64_t lit[288];
    __shared__ uint32_t x2n[32];
    __shared__ uint64_t head_bits_s;
    __shared__ uint32_t reg0_s;
    if (ctl->status < 0) return;
    const int t = (int)threadIdx.x;
    for (int i = t; i < HEAD_WORDS; i += WAVE) head[i] = 0;
    for (uint32_t i = t; i < prefix_len; i += WAVE) pre[i] = prefix[i];
    for (int i = t; i < 288; i += WAVE) lit[i] = ctl->hist[i];
    __syncthreads();
    if (t == 0) {
        x2n_fill(x2n);
        WordSink sink{head, 0};
        reg0_s = emit_head(sink, mode, lit, E, pre, prefix_len, cs, hw);
        head_bits_s = sink.pos;
    }
    __syncthreads();
    const uint64_t head_bits = head_bits_s;
    if ((head_bits + 7) / 8 + 8 > out_cap) {                        // the head alone does not fit
        if (t == 0) ctl->status = UKBB_LABELGZ_NO_ROOM;
        return;
    }
    const uint32_t *src = reinterpret_cast<const uint32_t *>(&cs);
    uint32_t *dst = reinterpret_cast<uint32_t *>(&ctl->cs);
    for (int i = t; i < (int)(sizeof(CodeSet) / 4); i += WAVE) dst[i] = src[i];
    if (t < 32) ctl->x2n[t] = x2n[t];
    if (t == 0) { ctl->base_bits = head_bits; ctl->reg0 = reg0_s; }
    // whole words plainly; the last, partial one is shared with run 0: OR onto the zeroed output.  Its 4 bytes end below head bytes + 3 < out_cap
    const uint32_t full = (uint32_t)(head_bits >> 5);
    for (uint32_t i = t; i < full; i += WAVE) out_words[i] = head[i];
    if (t == 0 && (head_bits & 31) && head[full]) atomicOr(&out_words[full], head[full]);
}

__device__ __forceinline__ void load_codes(const Ctl *ctl, CodeSet &cs, uint32_t *x2n) {
    const uint32_t *src = reinterpret_cast<const uint32_t *>(&ctl->cs);
    uint32_t *dst = reinterpret_cast<uint32_t *>(&cs);
    for (int i = (int)threadIdx.x; i < (int)(sizeof(CodeSet) / 4); i += THREADS) dst[i] = src[i];
    if (x2n && threadIdx.x < 32) x2n[threadIdx.x] = ctl->x2n[threadIdx.x];
    __syncthreads();
}

// ordered join of one piece per thread; the result is in p[0]
__device__ __forceinline__ void join_pieces(CrcPiece *p) {
    __syncthreads();
    for (int s = 1; s < THREADS; s <<= 1) {
        if (((int)threadIdx.x & (2 * s - 1)) == 0) p[threadIdx.x] = crc_join(p[threadIdx.x], p[threadIdx.x + s]);
        __syncthreads();
    }
}

__global__ __launch_bounds__(THREADS) void run_bits_kernel(const uint8_t *labels, uint64_t n, const uint32_t *run_start, const Ctl *ctl, int datatype,
                                                           int E, unsigned long long *local_off, unsigned long long *rbits, CrcPiece *rcrc) {
    __shared__ CodeSet cs;
    __shared__ uint32_t x2n[32];
    __shared__ unsigned long long part[THREADS / WAVE];
    __shared__ CrcPiece pieces[THREADS];
    if (ctl->status < 0) return;
    load_codes(ctl, cs, x2n);
    const uint32_t n_runs = ctl->n_runs;
    const uint64_t nrb = ((uint64_t)n_runs + RUN_BLOCK - 1) / RUN_BLOCK;
    for (uint64_t blk = blockIdx.x; blk < nrb; blk += gridDim.x) {
        const uint64_t r = blk * RUN_BLOCK + threadIdx.x;
        unsigned long long bits = 0, total;
        CrcPiece piece = crc_identity();
        if (r < n_runs) {
            const Run q = load_run(labels, n, run_start, n_runs, r, datatype);
            bits = run_bits(cs, q.P, E, q.len);
            piece = crc_pattern_run(x2n, q.P, E, q.len);
        }
        const unsigned long long ex = block_exclusive_scan<unsigned long long>(bits, part, total);
        if (r < n_runs) local_off[r] = ex;
        pieces[threadIdx.x] = piece;
        join_pieces(pieces);
        if (threadIdx.x == 0) { rbits[blk] = total; rcrc[blk] = pieces[0]; }
        __syncthreads();
    }
}

// OR of `bits` bits of v at bit position p of the zeroed output (global memory)
__device__ __forceinline__ void or_global(uint32_t *out_words, uint64_t p, uint32_t v, int bits) {
    if (!bits) return;
    const uint64_t x = (uint64_t)v << (p & 31);
    if ((uint32_t)x) atomicOr(&out_words[p >> 5], (uint32_t)x);
    if (x >> 32) atomicOr(&out_words[(p >> 5) + 1], (uint32_t)(x >> 32));
}

__global__ __launch_bounds__(THREADS) void finish_kernel(Ctl *ctl, unsigned long long *rbits, const CrcPiece *rcrc, uint8_t *out, uint64_t out_cap,
                                                         uint64_t n, uint64_t prefix_len, int E, long long *d_len) {
    __shared__ unsigned long long part[THREADS / WAVE];
    __shared__ CrcPiece pieces[THREADS];
    if (ctl->status < 0) { if (threadIdx.x == 0) *d_len = ctl->status; return; }
    const uint64_t nrb = ((uint64_t)ctl->n_runs + RUN_BLOCK - 1) / RUN_BLOCK;
    unsigned long long running = ctl->base_bits;
    for (uint64_t c = 0; c < nrb; c += THREADS) {                   // sums -> absolute bit offsets of the run blocks, in place
        const uint64_t i = c + threadIdx.x;
        const unsigned long long v = i < nrb ? rbits[i] : 0;
        unsigned long long total;
        const unsigned long long ex = block_exclusive_scan<unsigned long long>(v, part, total);
        if (i < nrb) rbits[i] = running + ex;
        running += total;
    }
    const uint64_t per = (nrb + THREADS - 1) / THREADS;
    CrcPiece piece = crc_identity();
    for (uint64_t k = threadIdx.x * per; k < (threadIdx.x + 1) * per && k < nrb; ++k) piece = crc_join(piece, rcrc[k]);
    pieces[threadIdx.x] = piece;
    join_pieces(pieces);
    if (threadIdx.x != 0) return;
    rbits[nrb] = running;
    const CodeSet &cs = ctl->cs;
    const uint64_t total_bits = running + cs.lit_len[256];
    const uint64_t len = (total_bits + 7) / 8 + 8;
    if (len > out_cap) { ctl->status = UKBB_LABELGZ_NO_ROOM; *d_len = UKBB_LABELGZ_NO_ROOM; return; }
    or_global(reinterpret_cast<uint32_t *>(out), running, cs.lit_bits[256], cs.lit_len[256]);    // end of block; its words end below len
    const CrcPiece all = pieces[0];
    const uint32_t crc = (mult(all.pw, ctl->reg0) ^ all.c) ^ 0xFFFFFFFFu;
    const uint32_t isize = (uint32_t)((prefix_len + n * (uint64_t)E) & 0xFFFFFFFFull);
    for (int k = 0; k < 4; ++k) { out[len - 8 + k] = (uint8_t)(crc >> (8 * k)); out[len - 4 + k] = (uint8_t)(isize >> (8 * k)); }
    *d_len = (long long)len;
}

// The emission sink of one thread: tokens ORed into the workgroup's LDS window, clipped to it; long (258, E) fills are queued for the workgroup
struct WindowSink {
    uint32_t *win;
    uint64_t lo_word, pos;
    uint32_t *n_long;
    unsigned long long *long_at, *long_n;
    __device__ __forceinline__ void put(uint32_t v, int bits) {
        if (!bits) return;
        const uint64_t x = (uint64_t)v << (pos & 31), w = pos >> 5;
        if ((uint32_t)x && w >= lo_word && w < lo_word + WIN_WORDS) atomicOr(&win[w - lo_word], (uint32_t)x);
        if ((x >> 32) && w + 1 >= lo_word && w + 1 < lo_word + WIN_WORDS) atomicOr(&win[w + 1 - lo_word], (uint32_t)(x >> 32));
        pos += (uint64_t)bits;
    }
    __device__ __forceinline__ void fill258(uint64_t count, uint32_t tok, int len) {
        if (count < (uint64_t)COOP_TOKENS) { for (; count; --count) put(tok, len); return; }
        const uint64_t end = pos + count * (uint64_t)len;
        if (end > lo_word * 32 && pos < (lo_word + WIN_WORDS) * 32) {           // at most one per thread: the lists hold THREADS entries
            const uint32_t i = atomicAdd(n_long, 1u);
            long_at[i] = pos; long_n[i] = count;
        }
        pos = end;
    }
};

__global__ __launch_bounds__(THREADS) void emit_kernel(const uint8_t *labels, uint64_t n, const uint32_t *run_start, const Ctl *ctl, int datatype, int E,
                                                       const unsigned long long *local_off, const unsigned long long *rbits, uint32_t *out_words) {
    __shared__ CodeSet cs;
    __shared__ uint32_t win[WIN_WORDS];
    __shared__ unsigned long long long_at[THREADS], long_n[THREADS];
    __shared__ uint32_t n_long;
    if (ctl->status < 0) return;
    load_codes(ctl, cs, nullptr);
    const uint32_t n_runs = ctl->n_runs;
    const uint64_t nrb = ((uint64_t)n_runs + RUN_BLOCK - 1) / RUN_BLOCK;
    uint32_t tok; int tok_len;
    token258(cs, tok, tok_len);
    for (uint64_t blk = blockIdx.x; blk < nrb; blk += gridDim.x) {
        const uint64_t r = blk * RUN_BLOCK + threadIdx.x;
        const uint64_t B0 = rbits[blk], B1 = rbits[blk + 1];       // this workgroup's span of bits
        const uint64_t W1 = (B1 + 31) >> 5;
        Run q; q.len = 0;
        uint64_t at = 0;
        if (r < n_runs) { q = load_run(labels, n, run_start, n_runs, r, datatype); at = B0 + local_off[r]; }
        for (uint64_t lo_word = B0 >> 5; lo_word < W1; lo_word += WIN_WORDS) {
            for (int j = (int)threadIdx.x; j < WIN_WORDS; j += THREADS) win[j] = 0;
            if (threadIdx.x == 0) n_long = 0;
            __syncthreads();
            if (r < n_runs) {
                WindowSink sink{win, lo_word, at, &n_long, long_at, long_n};
                emit_run(sink, cs, q.P, E, q.len);
            }
            __syncthreads();
            const uint32_t nl = n_long;
            // periodic fills.  Thread t owns the window words j with j % THREADS == t, whichever fill they belong to: two fills that lie
            // next to each other may end and begin in one word, and then one thread ORs both into it, one after the other.  (The tokens
            // the threads put above are complete: a barrier lies between.)
            for (uint32_t e = 0; e < nl; ++e) {
                const uint64_t a = long_at[e], b = a + long_n[e] * (uint64_t)tok_len;
                const uint64_t j0 = (a >> 5) > lo_word ? (a >> 5) - lo_word : 0;
                for (uint64_t j = j0 + ((threadIdx.x - (uint32_t)j0) & (THREADS - 1)); j < WIN_WORDS; j += THREADS) {
                    const uint64_t wlo = (lo_word + j) * 32, whi = wlo + 32;
                    if (wlo >= b) break;
                    const uint64_t s = a > wlo ? a : wlo, e1 = b < whi ? b : whi;
                    uint32_t ph = (uint32_t)((s - a) % (uint64_t)tok_len), val = 0;
                    for (uint64_t p = s; p < e1; p += tok_len - ph, ph = 0) val |= (uint32_t)((uint64_t)(tok >> ph) << (p - wlo));
                    if (e1 < whi) val &= (1u << (e1 - wlo)) - 1;
                    win[j] |= val;
                }
            }
            __syncthreads();
            for (int j = (int)threadIdx.x; j < WIN_WORDS; j += THREADS) {
                const uint64_t gw = lo_word + j;
                if (gw >= W1) break;
                const uint32_t val = win[j];
                if (gw * 32 >= B0 && gw * 32 + 32 <= B1) out_words[gw] = val;
                else if (val) atomicOr(&out_words[gw], val);
            }
            __syncthreads();
        }
    }
}

int datatype_size(int datatype) { uint8_t tmp[8]; return element_pattern(datatype, 0, tmp); }

}  // namespace

extern "C" {

uint64_t ukbb_fcn_gzip_labels_device_scratch(uint64_t n_voxels, uint64_t max_runs) {
    if (n_voxels < 1 || n_voxels > UKBB_LABELGZ_MAX_VOXELS || max_runs < 1 || max_runs > UKBB_LABELGZ_MAX_VOXELS) return 0;
    return Layout(n_voxels, max_runs).total;
}

void ukbb_fcn_gzip_labels_device_geometry(uint32_t geometry[4]) {
    geometry[0] = VOX_BLOCK; geometry[1] = RUN_BLOCK; geometry[2] = WIN_WORDS * 32; geometry[3] = COOP_TOKENS;
}

int ukbb_fcn_gzip_labels_device(const uint8_t *d_labels, uint64_t n_voxels, int nifti_datatype, const uint8_t *d_prefix, uint64_t prefix_len,
                                int mode, uint8_t *d_out, uint64_t out_cap, void *d_scratch, uint64_t max_runs, int64_t *d_len, void *stream) {
    const int E = datatype_size(nifti_datatype);
    if (!d_labels || !d_out || !d_scratch || !d_len || (!d_prefix && prefix_len) || !E || (mode != UKBB_GZIP_FIXED && mode != UKBB_GZIP_DYNAMIC) ||
        n_voxels < 1 || n_voxels > UKBB_LABELGZ_MAX_VOXELS || prefix_len > UKBB_LABELGZ_MAX_PREFIX || max_runs < 1 ||
        max_runs > UKBB_LABELGZ_MAX_VOXELS || ((uintptr_t)d_out & 3) || ((uintptr_t)d_scratch & 15)) {
        set_error("gzip_labels_device: bad argument (datatype 2/4/8/16/64, 1 <= n_voxels <= %llu, prefix_len <= %d, d_out 4-byte and d_scratch "
                  "16-byte aligned, no NULL)", (unsigned long long)UKBB_LABELGZ_MAX_VOXELS, UKBB_LABELGZ_MAX_PREFIX);
        return UKBB_EINVAL;
    }
    if (current_device() < 0) { set_error("gzip_labels_device: no HIP device (there is no CPU fallback)"); return UKBB_EDEVICE; }
    hipStream_t s = (hipStream_t)stream;
    const Layout L(n_voxels, max_runs);
    uint8_t *base = static_cast<uint8_t *>(d_scratch);
    Ctl *ctl = reinterpret_cast<Ctl *>(base);
    uint32_t *vcount = reinterpret_cast<uint32_t *>(base + L.vcount);
    unsigned long long *rbits = reinterpret_cast<unsigned long long *>(base + L.rbits);
    CrcPiece *rcrc = reinterpret_cast<CrcPiece *>(base + L.rcrc);
    unsigned long long *local_off = reinterpret_cast<unsigned long long *>(base + L.local_off);
    uint32_t *run_start = reinterpret_cast<uint32_t *>(base + L.run_start);
    uint32_t *out_words = reinterpret_cast<uint32_t *>(d_out);
    const dim3 vgrid((unsigned)L.nvb), rgrid((unsigned)(L.nrb < (uint64_t)MAX_GRID ? L.nrb : MAX_GRID)), block(THREADS);
    hipError_t e = hipMemsetAsync(ctl, 0, L.vcount, s);
    if (e == hipSuccess && out_cap) e = hipMemsetAsync(d_out, 0, out_cap, s);
    auto launched = [&] { if (e == hipSuccess) e = hipGetLastError(); return e == hipSuccess; };
    if (launched()) hipLaunchKernelGGL(runs_count_kernel, vgrid, block, 0, s, d_labels, n_voxels, vcount);
    if (launched()) hipLaunchKernelGGL(runs_scan_kernel, dim3(1), block, 0, s, vcount, L.nvb, max_runs, ctl);
    if (launched()) hipLaunchKernelGGL(runs_compact_kernel, vgrid, block, 0, s, d_labels, n_voxels, vcount, ctl, run_start, max_runs);
    if (mode == UKBB_GZIP_DYNAMIC && launched())
        hipLaunchKernelGGL(histogram_kernel, rgrid, block, 0, s, d_labels, n_voxels, run_start, ctl, nifti_datatype, E, d_prefix, (uint32_t)prefix_len);
    if (launched()) hipLaunchKernelGGL(codes_kernel, dim3(1), dim3(WAVE), 0, s, ctl, mode, E, d_prefix, (uint32_t)prefix_len, out_words, out_cap);
    if (launched()) hipLaunchKernelGGL(run_bits_kernel, rgrid, block, 0, s, d_labels, n_voxels, run_start, ctl, nifti_datatype, E, local_off, rbits, rcrc);
    if (launched())
        hipLaunchKernelGGL(finish_kernel, dim3(1), block, 0, s, ctl, rbits, rcrc, d_out, out_cap, n_voxels, prefix_len, E, reinterpret_cast<long long *>(d_len));
    if (launched()) hipLaunchKernelGGL(emit_kernel, rgrid, block, 0, s, d_labels, n_voxels, run_start, ctl, nifti_datatype, E, local_off, rbits, out_words);
    if (!launched()) { set_error("gzip_labels_device: launch failed: %s (there is no CPU fallback)", hipGetErrorString(e)); return UKBB_EDEVICE; }
    return UKBB_OK;
}

}  // extern "C"
