// Inflate of gzip NIfTI cines on the device, many streams per launch (include/ukbb_fcn.h: ukbb_fcn_inflate_device).  The decoder is
// inflate_core.h, the same text ukbb_fcn_inflate_core_host runs on the host; this file holds its device policy (DevIo), the two kernels
// and the host entry points.  No reference counterpart: the reference leaves gzip to nibabel (common/deploy_network.py:80-83).
//
// inflate_kernel: one workgroup of ONE wave per stream (a deflate stream is serial; the launch pays through the number of streams in
// flight), grid = min(n_streams, 2 x CUs) with a loop over the streams beyond.  The symbol loop of the core runs wave-uniformly -- every
// lane holds the same bit buffer and positions, table entries come back through readfirstlane so that the state stays scalar -- and the
// lanes share the work that has width:
//   * input: the next 1 KB of the stream (64 lanes x 16 bytes, aligned; the two ragged ends byte by byte, never outside the stream) is
//     asked for one refill before the bit reader needs it and written to a 4 KB LDS window when the reader gets within 2 KB of its end;
//   * tables of a dynamic block: the lanes fill the entries, one symbol each (inflate_core.h build_table);
//   * output: literals and matches go to an LDS ring of the last 36 KB written (32 KB of history + what is not flushed yet), so that a
//     match never reads global memory back; a match is copied by all lanes at once, byte i from i mod distance where distance < length;
//     the ring is flushed to global memory in aligned 16-byte pieces, one per lane, whenever 2 KB are pending.
// LDS per workgroup: Work 15 408 B + ring 36 864 B + window 4 096 B = 56 368 B static -> 2 workgroups per CU by LDS (110.1 of 160 KB;
// 49 KB stay free for whatever else is resident), 512 streams in flight on 256 CUs.
// No lane reads outside [src, src + src_len) or writes outside [dst, dst + bytes written): inflate_core.h checks every length and
// distance before it asks DevIo to move a byte, and the flush writes [0, pos) only.
//
// crc32_chunks_kernel: exact CRC-32 of each stream's inflated bytes.  A workgroup takes a 64 KB chunk, a thread a 256-byte slice from a
// zero register (slicing-by-4, tables in LDS); slices and chunks are combined by multiplication with x^(8 * bytes behind) mod P and
// xor-ed into the stream's word -- integer arithmetic, the same value in whatever order the chunks arrive.
#include <mutex>

#include "../../include/ukbb_fcn.h"
#include "inflate_core.h"
#include "kernels.h"

using namespace ukbb;
using namespace ukbb_inflate;

namespace {

constexpr int RING = 36864, STAGE = 4096, IN_CHUNK = 1024, FLUSH_AT = 2048, OUT_STEP = 1024, WAVE = 64;
static_assert(RING % 16 == 0 && RING >= 32768 + FLUSH_AT + OUT_STEP + 258 + 16, "ring: 32 KB of history + the most that can be pending");
constexpr int CRC_THREADS = 256, CRC_SLICE = UKBB_INFLATE_CRC_CHUNK / CRC_THREADS;

struct DevIo {
    const uint8_t *src16;       // src rounded down to 16 bytes: "s" coordinates below count from here, the stream is [sal, s_end)
    uint8_t *dst16;             // dst rounded down to 16 bytes: "g" coordinates, the output is [a0, a0 + dst_cap)
    uint8_t *ring, *stage;
    uint32_t sal, a0;
    uint64_t s_end;
    int ln;
    // output: ring index = g mod RING.  [g_lo, g_lo + npend) is in the ring only, everything before is in global memory
    uint64_t g_lo;
    uint32_t widx, fidx, npend;  // ring index of the next byte / of g_lo rounded down to 16
    // input window: [st_lo, st_hi) is in LDS at s mod STAGE; pend = this lane's 16 bytes of [st_hi, st_hi + IN_CHUNK), asked for, not yet written
    uint64_t st_lo, st_hi;
    bool has_pend;
    uint4 pend;

    __device__ __forceinline__ DevIo(const uint8_t *src, uint64_t src_len, uint8_t *dst, uint8_t *ring_, uint8_t *stage_) {
        sal = (uint32_t)((uintptr_t)src & 15); src16 = src - sal; s_end = sal + src_len;
        a0 = (uint32_t)((uintptr_t)dst & 15); dst16 = dst - a0;
        ring = ring_; stage = stage_; ln = (int)threadIdx.x;
        g_lo = a0; widx = a0; fidx = 0; npend = 0;
        st_lo = st_hi = ~0ull; has_pend = false; pend = make_uint4(0, 0, 0, 0);
    }
    __device__ __forceinline__ bool leader() const { return ln == 0; }
    __device__ __forceinline__ int lane() const { return ln; }
    __device__ __forceinline__ int lanes() const { return WAVE; }
    // the workgroup is one wave: its LDS and memory instructions execute in order, so a fence of wavefront scope (no instruction) is all
    // that is needed between a lane's write and another lane's read
    __device__ __forceinline__ void sync() const { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }
    template <class T> __device__ __forceinline__ T uni(T v) const { return (T)__builtin_amdgcn_readfirstlane((int)v); }

    // ---- input ----
    __device__ __forceinline__ uint4 load_piece(uint64_t s) const {        // 16 aligned bytes at s; zeros outside the stream, which is never read
        if (s >= sal && s + 16 <= s_end) return *reinterpret_cast<const uint4 *>(src16 + s);
        uint32_t v[4] = {0, 0, 0, 0};
        if (s + 16 > sal && s < s_end)
            for (int k = 0; k < 16; ++k) { const uint64_t t = s + k; if (t >= sal && t < s_end) v[k >> 2] |= (uint32_t)src16[t] << (8 * (k & 3)); }
        return make_uint4(v[0], v[1], v[2], v[3]);
    }
    __device__ __forceinline__ void issue() { pend = load_piece(st_hi + 16u * ln); has_pend = true; }
    __device__ __forceinline__ void commit() {
        *reinterpret_cast<uint4 *>(stage + ((st_hi + 16u * ln) & (STAGE - 1))) = pend;
        st_hi += IN_CHUNK; has_pend = false;
        if (st_hi - st_lo > STAGE) st_lo = st_hi - STAGE;
        sync();
    }
    __device__ __forceinline__ void ensure(uint64_t s) {                   // bytes [s, s + 4) readable from the window
        if (s < st_lo || s > st_hi) { has_pend = false; st_lo = st_hi = s & ~15ull; }       // first use, or the far side of a stored block
        if (st_hi < s + 2 * IN_CHUNK) {
            // the commit overwrites the window's oldest KB, [st_hi - 4 KB, st_hi - 3 KB): 1 KB and more behind s (the reader steps back by at
            // most 8 bytes, after a stored block's header; a step behind st_lo would restart the window, not read stale bytes)
            if (has_pend) commit();
            while (st_hi < s + 4) { if (!has_pend) issue(); commit(); }                      // cold start only: one round
            if (st_hi < s_end) issue();
        }
    }
    __device__ __forceinline__ uint32_t in_align() const { return sal & 3; }
    __device__ __forceinline__ uint32_t in_byte(uint64_t i) { const uint64_t s = i + sal; ensure(s); return uni((uint32_t)stage[s & (STAGE - 1)]); }
    __device__ __forceinline__ uint32_t in_word(uint64_t i) { const uint64_t s = i + sal; ensure(s); return uni(*reinterpret_cast<const uint32_t *>(stage + (s & (STAGE - 1)))); }

    // ---- output ----
    __device__ __forceinline__ static uint32_t wrap(uint32_t i) { return i >= RING ? i - RING : i; }
    __device__ __forceinline__ void flush(bool final) {
        sync();                                              // the leader's literals in the ring before the other lanes read them
        const uint64_t g_hi = g_lo + npend, gA = g_lo & ~15ull, end = final ? g_hi : (g_hi & ~15ull);
        const uint32_t npieces = (uint32_t)((end - gA + 15) >> 4);
        for (uint32_t j = ln; j < npieces; j += WAVE) {
            const uint64_t g = gA + 16ull * j;
            const uint32_t idx = wrap(fidx + 16u * j);       // RING % 16 == 0: a piece never wraps
            if (g >= g_lo && g + 16 <= g_hi) *reinterpret_cast<uint4 *>(dst16 + g) = *reinterpret_cast<const uint4 *>(ring + idx);
            else for (int k = 0; k < 16; ++k) { const uint64_t t = g + k; if (t >= g_lo && t < g_hi) dst16[t] = ring[idx + k]; }
        }
        fidx = wrap(fidx + (uint32_t)((end & ~15ull) - gA));
        g_lo = end; npend = (uint32_t)(g_hi - end);
    }
    __device__ __forceinline__ void advance(uint32_t n) {                   // n <= OUT_STEP bytes were written at widx
        widx = wrap(widx + n); npend += n;
        if (npend >= FLUSH_AT) flush(false);
    }
    __device__ __forceinline__ void put_byte(uint32_t v) { if (ln == 0) ring[widx] = (uint8_t)v; advance(1); }
    __device__ __forceinline__ void copy_match(uint32_t dist, uint32_t len) {   // dist <= 32768 bytes back, all of them in the ring; len <= 258
        const uint32_t sidx = widx >= dist ? widx - dist : widx + RING - dist;
        sync();
        for (uint32_t i = ln; i < len; i += WAVE) {
            const uint32_t off = dist >= len ? i : i % dist;     // run semantics: every source byte was there before this match
            ring[wrap(widx + i)] = ring[wrap(sidx + off)];
        }
        sync();
        advance(len);
    }
    __device__ __forceinline__ void copy_stored(uint64_t in, uint32_t len) {    // [in, in + len) checked against src_len, the room against dst_cap
        for (uint32_t done = 0; done < len; done += OUT_STEP) {
            const uint32_t n = len - done < OUT_STEP ? len - done : OUT_STEP;
            for (uint32_t i = ln; i < n; i += WAVE) ring[wrap(widx + i)] = src16[sal + in + done + i];
            sync();
            advance(n);
        }
    }
    __device__ __forceinline__ void finish() { flush(true); }
};

__global__ __launch_bounds__(WAVE) void inflate_kernel(const uint8_t *src, uint8_t *dst, const ukbb_fcn_gz_stream *streams, int n_streams,
                                                       int64_t *written) {
    __shared__ Work work;
    __shared__ __attribute__((aligned(16))) uint8_t ring[RING];
    __shared__ __attribute__((aligned(16))) uint8_t stage[STAGE];
    for (int s = (int)blockIdx.x; s < n_streams; s += (int)gridDim.x) {
        const ukbb_fcn_gz_stream st = streams[s];
        DevIo io(src + st.src_off, st.src_len, dst + st.dst_off, ring, stage);
        const int64_t r = inflate_core(io, work, st.src_len, st.dst_cap);
        if (threadIdx.x == 0) written[s] = r;
        io.sync();
    }
}

__global__ __launch_bounds__(CRC_THREADS) void crc32_chunks_kernel(const uint8_t *dst, const ukbb_fcn_gz_stream *streams, const int64_t *written,
                                                                   uint32_t *crc /* 0xFFFFFFFF on entry */) {
    __shared__ uint32_t T[4][256];
    __shared__ uint32_t x2n[32];
    __shared__ uint32_t red[CRC_THREADS / WAVE];
    const int s = (int)blockIdx.y, t = (int)threadIdx.x;
    const int64_t wr = written[s];
    const uint64_t chunk0 = (uint64_t)blockIdx.x * UKBB_INFLATE_CRC_CHUNK;
    if (wr < 0) { if (blockIdx.x == 0 && t == 0) atomicXor(&crc[s], 0xFFFFFFFFu); return; }     // a refused stream: 0
    const uint64_t N = (uint64_t)wr;
    if (blockIdx.x != 0 && chunk0 >= N) return;
    {
        uint32_t c = (uint32_t)t;
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (CRC_POLY & (0u - (c & 1)));
        T[0][t] = c;
        if (t < 32) x2n[t] = crc_x2n(t);
    }
    __syncthreads();
    for (int k = 1; k < 4; ++k) T[k][t] = (T[k - 1][t] >> 8) ^ T[0][T[k - 1][t] & 0xff];      // own column only
    __syncthreads();
    const uint64_t chunk_end = N < chunk0 + UKBB_INFLATE_CRC_CHUNK ? N : chunk0 + UKBB_INFLATE_CRC_CHUNK;
    const uint64_t lo = chunk0 + (uint64_t)t * CRC_SLICE, hi = lo + CRC_SLICE < chunk_end ? lo + CRC_SLICE : chunk_end;
    uint32_t c = 0;
    if (lo < hi) {
        const uint8_t *p = dst + streams[s].dst_off + lo, *const e = p + (hi - lo);
        while (p < e && ((uintptr_t)p & 15)) c = (c >> 8) ^ T[0][(c ^ *p++) & 0xff];
        for (; e - p >= 16; p += 16) {
            const uint4 v = *reinterpret_cast<const uint4 *>(p);
            const uint32_t wv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                c ^= wv[k];
                c = T[3][c & 0xff] ^ T[2][(c >> 8) & 0xff] ^ T[1][(c >> 16) & 0xff] ^ T[0][c >> 24];
            }
        }
        while (p < e) c = (c >> 8) ^ T[0][(c ^ *p++) & 0xff];
        c = crc_mul(c, crc_xpow8(x2n, chunk_end - hi));
    }
    for (int o = 32; o; o >>= 1) c ^= __shfl_xor(c, o, WAVE);
    if ((t & (WAVE - 1)) == 0) red[t / WAVE] = c;
    __syncthreads();
    if (t == 0) {
        c = red[0] ^ red[1] ^ red[2] ^ red[3];
        c = crc_mul(c, crc_xpow8(x2n, N - chunk_end));
        if (blockIdx.x == 0) c ^= crc_mul(0xFFFFFFFFu, crc_xpow8(x2n, N));      // the register's start value, carried over all N bytes
        atomicXor(&crc[s], c);                                                   // crc[s] started as 0xFFFFFFFF: the final inversion
    }
}

// The stream table of a launch: pinned host copy + device copy, TWO pairs per device taken in turn and reused from call to call, so
// that a call issued while the previous launch still runs (the next round's inflate under this round's network) does not wait.  A
// call waits for the event of the launch before the previous one -- the last that read the pair it is about to overwrite.  The
// pairs live as long as the process (a few KB per device; the runtime releases them at exit).
struct StreamTable {
    ukbb_fcn_gz_stream *host = nullptr, *dev = nullptr;
    size_t cap = 0;
    hipEvent_t last = nullptr;
};
struct DeviceTables {
    std::mutex mu;
    StreamTable pair[2];
    unsigned turn = 0;
};
DeviceTables g_tables[64];

}  // namespace

extern "C" {

int ukbb_fcn_inflate_device(const uint8_t *d_src, uint8_t *d_dst, const ukbb_fcn_gz_stream *streams, int n_streams, int64_t *d_written,
                            uint32_t *d_crc, void *stream) {
    if (!d_src || !d_dst || !streams || !d_written || n_streams < 1 || n_streams > UKBB_INFLATE_MAX_STREAMS) {
        set_error("inflate_device: bad argument (1 <= n_streams <= %d, no NULL but d_crc)", UKBB_INFLATE_MAX_STREAMS);
        return UKBB_EINVAL;
    }
    uint64_t max_cap = 0;
    for (int i = 0; i < n_streams; ++i) {
        if (streams[i].src_len > UKBB_INFLATE_MAX_BYTES || streams[i].dst_cap > UKBB_INFLATE_MAX_BYTES) {
            set_error("inflate_device: stream %d: src_len / dst_cap above 2^40", i);
            return UKBB_EINVAL;
        }
        if (streams[i].dst_cap > max_cap) max_cap = streams[i].dst_cap;
    }
    const int dev = current_device();
    if (dev < 0 || dev >= 64) { set_error("inflate_device: no HIP device (there is no CPU fallback)"); return UKBB_EDEVICE; }
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(g_tables[dev].mu);
    StreamTable &tb = g_tables[dev].pair[g_tables[dev].turn++ & 1];
    if (!tb.last && hipEventCreateWithFlags(&tb.last, hipEventDisableTiming) != hipSuccess) { tb.last = nullptr; set_error("inflate_device: no event"); return UKBB_EDEVICE; }
    if (tb.cap && hipEventSynchronize(tb.last) != hipSuccess) { set_error("inflate_device: the previous launch failed"); return UKBB_EDEVICE; }
    if (tb.cap < (size_t)n_streams) {
        if (tb.host) (void)hipHostFree(tb.host);
        if (tb.dev) (void)hipFree(tb.dev);
        tb.host = tb.dev = nullptr; tb.cap = 0;
        size_t cap = 256;
        while (cap < (size_t)n_streams) cap *= 2;
        if (hipHostMalloc(reinterpret_cast<void **>(&tb.host), cap * sizeof(ukbb_fcn_gz_stream), hipHostMallocDefault) != hipSuccess ||
            hipMalloc(reinterpret_cast<void **>(&tb.dev), cap * sizeof(ukbb_fcn_gz_stream)) != hipSuccess) {
            if (tb.host) (void)hipHostFree(tb.host);
            tb.host = tb.dev = nullptr;
            set_error("inflate_device: no memory for the stream table");
            return UKBB_ENOMEM;
        }
        tb.cap = cap;
    }
    memcpy(tb.host, streams, sizeof(ukbb_fcn_gz_stream) * (size_t)n_streams);
    if (hipMemcpyAsync(tb.dev, tb.host, sizeof(ukbb_fcn_gz_stream) * (size_t)n_streams, hipMemcpyHostToDevice, s) != hipSuccess) {
        set_error("inflate_device: upload of the stream table failed");
        return UKBB_EDEVICE;
    }
    const int cap_grid = 2 * device_cu_count();
    hipLaunchKernelGGL(inflate_kernel, dim3((unsigned)(n_streams < cap_grid ? n_streams : cap_grid)), dim3(WAVE), 0, s, d_src, d_dst, tb.dev,
                       n_streams, d_written);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && d_crc) {
        e = hipMemsetAsync(d_crc, 0xff, sizeof(uint32_t) * (size_t)n_streams, s);
        if (e == hipSuccess) {
            const uint64_t chunks = (max_cap + UKBB_INFLATE_CRC_CHUNK - 1) / UKBB_INFLATE_CRC_CHUNK;
            hipLaunchKernelGGL(crc32_chunks_kernel, dim3((unsigned)(chunks ? chunks : 1), (unsigned)n_streams), dim3(CRC_THREADS), 0, s, d_dst, tb.dev,
                               d_written, d_crc);
            e = hipGetLastError();
        }
    }
    (void)hipEventRecord(tb.last, s);
    if (e != hipSuccess) { set_error("inflate_device: launch failed: %s (there is no CPU fallback)", hipGetErrorString(e)); return UKBB_EDEVICE; }
    return UKBB_OK;
}

int64_t ukbb_fcn_inflate_core_host(const uint8_t *src, uint64_t src_len, uint8_t *dst, uint64_t dst_cap) {
    if ((!src && src_len) || (!dst && dst_cap)) return E_DATA;
    Work w;
    HostIo io(src, dst);
    return inflate_core(io, w, src_len, dst_cap);
}

uint32_t ukbb_fcn_gzip_crc_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
    uint32_t x2n[32];
    x2n[0] = 1u << 30;
    for (int k = 1; k < 32; ++k) x2n[k] = crc_mul(x2n[k - 1], x2n[k - 1]);
    return crc_mul(crc_xpow8(x2n, len_b), crc_a) ^ crc_b;
}

}  // extern "C"
