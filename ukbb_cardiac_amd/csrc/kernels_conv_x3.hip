// conv3x3 (+ folded BN bias, ReLU), stride 1 or 2, with fp32-grade results from three bf16 pieces per operand on the dense matrix cores:
// the X3 form of the bf16-operand branch of conv_mfma_kernel (kernels_conv.hip, BF && !BFIO).  ConvFamily::F32x3Operands, tilings 330-345,
// planned only under UKBB_PREC_F32X3 with ukbb_fcn_set_f32x3_convs on (plan.cpp).
//
// Arithmetic.  x = h + m + l with h = bf16(x), m = bf16(x - h), l = bf16(x - h - m) (split_pair, device_prims.h; round to nearest even, the
// residuals exact in fp32); the folded weights likewise, on the host when they are packed (pack_conv_x3).  Per (tap, 16-channel chunk, pixel
// block, Cout block) six v_mfma_f32_32x32x16_bf16 add into the ONE fp32 accumulator, weight piece x activation piece, small terms first:
//     l.h   h.l   m.m   m.h   h.m   h.h
// Dropped: m.l, l.m and l.l, each below 2^-24 |w||x| per product, and whatever the third piece does not hold (below 2^-24 |x|).
// fp32 throughout: the maps in HBM on both sides, the accumulator, bias, ReLU and the NHWC store -- the epilogue is the fp32 kernels'.
//
// Data movement per workgroup (256 threads = 4 waves), as in the bf16-operand kernel: the fp32 halo tile of a 16-channel chunk is fetched one
// chunk ahead into registers, split ONCE per staged element (not once per tap) and written as three bf16 planes xs[piece][halo pixel][8 + 4 pad
// dwords]; the packed weight pieces ws[piece][Cout block][tap][lane][4 dwords] come as straight 16-byte copies.  Padding pixels are zero in all
// three planes.  LDS = 3 x the bf16-operand tiling's.
#include "kernels.h"
#include "device_prims.h"

namespace ukbb {

namespace {

__host__ __device__ constexpr int x3_halo(int t, int s) { return (t - 1) * s + 3; }
__host__ __device__ constexpr int conv_x3_lds_bytes(int s, int th, int tw, int wm, int cb) {
    return 3 * ((16 / 2 + 4) * x3_halo(th, s) * x3_halo(tw, s) + wm * cb * 9 * 64 * 4) * 4;      // 3 x conv_bf_lds_bytes (kernels_conv.hip)
}

template <int STRIDE, int TH, int TW, int WM, int WN, int CB>
__global__ __launch_bounds__(256) void conv_x3_kernel(const ConvArgs a) {
    constexpr int KS2 = 9, KC = 16, PB = 32;
    constexpr int NPIX = TH * TW, NPB = (NPIX + PB - 1) / PB, PBW = (NPB + WN - 1) / WN;
    constexpr int IH = x3_halo(TH, STRIDE), IW = x3_halo(TW, STRIDE), HP = IH * IW, XS = KC / 2 + 4, C4 = KC / 4;
    constexpr int NCBL = WM * CB;                       // Cout blocks per workgroup
    constexpr int SLAB = KS2 * 64 * 4;                  // packed dwords of one piece of one Cout block, one chunk
    constexpr int XPL = HP * XS, WPL = NCBL * SLAB;     // dwords of one activation / weight plane
    constexpr int NIT = (HP * C4 + 255) / 256;          // activation float4 per thread per chunk
    constexpr int WF4 = 3 * WPL / 4;                    // weight float4 per workgroup per chunk (the three pieces are contiguous)
    constexpr int NWT = (WF4 + 255) / 256;
    constexpr int PSTEP = 256 / C4;                     // halo pixels advanced per staging iteration
    static_assert(WM * WN == 4, "4 waves per workgroup");
    static_assert(3 * (XPL + WPL) * 4 == conv_x3_lds_bytes(STRIDE, TH, TW, WM, CB), "LDS layout");

    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *xs = lds;                                     // [3][HP][XS]
    float *ws = lds + 3 * XPL;                           // [3][NCBL][KS2][64][4]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int g = lane / PB, pl = lane % PB;

    int bid = blockIdx.x;
    const int tx = bid % a.tiles_x; bid /= a.tiles_x;
    const int ty = bid % a.tiles_y;
    const int n = bid / a.tiles_y;
    const int oy0 = ty * TH, ox0 = tx * TW;
    const int cbg = blockIdx.y * NCBL + wm * CB;         // first Cout block of this wave

    int lbase[PBW];
#pragma unroll
    for (int pb = 0; pb < PBW; ++pb) {
        int q = (wn + pb * WN) * PB + pl;
        if (q >= NPIX) q = 0;                            // a slot beyond the tile multiplies pixel 0 again; never stored
        const int oy = q / TW, ox = q % TW;
        lbase[pb] = ((oy * STRIDE) * IW + ox * STRIDE) * XS + 4 * g;    // lane half g owns channels 8g .. 8g + 7 of the chunk
    }

    f32x16 acc[CB][PBW];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int pb = 0; pb < PBW; ++pb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[cb][pb][r] = 0.f;

    const int nchunk = a.C0 / KC;
    const int iy0 = oy0 * STRIDE - a.pad_y, ix0 = ox0 * STRIDE - a.pad_x;
    const int c4 = tid % C4, pix0 = tid / C4;           // this thread's channel quad / first halo pixel
    const float *wsrc = a.wpk + (size_t)blockIdx.y * nchunk * (3 * WPL);

    // Per-iteration global offsets of this thread's halo pixels (chunk independent), -1 = zero padding / beyond the halo tile.
    int goff[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int pix = pix0 + it * PSTEP;
        const int iy = pix / IW, ix = pix % IW;
        const int gy = iy0 + iy, gx = ix0 + ix;
        const bool ok = pix < HP && (unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W;
        goff[it] = ok ? (n * a.H + gy) * a.W + gx : -1;
    }

    f32x4 xr[NIT], wr[NWT];
    auto prefetch = [&](int ch) {
        const float *src = a.in0 + ch * KC + 4 * c4;
#pragma unroll
        for (int it = 0; it < NIT; ++it)                 // unconditional load from a clamped address (as conv_mfma_kernel): zeroed at the LDS write
            xr[it] = ld4(src + (size_t)(goff[it] < 0 ? 0 : goff[it]) * a.C0);
        const float *wp = wsrc + (size_t)ch * (3 * WPL);
#pragma unroll
        for (int it = 0; it < NWT; ++it)
            wr[it] = ld4((it * 256 + tid < WF4) ? wp + 4 * (it * 256 + tid) : a.wpk);
    };
    prefetch(0);

    for (int ch = 0; ch < nchunk; ++ch) {
        if (ch > 0) __syncthreads();                    // all waves done reading the previous chunk
        // ---- registers -> LDS: the split, once per staged element ----
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int pix = pix0 + it * PSTEP;
            const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
            const f32x4 v = goff[it] < 0 ? zero4 : xr[it];
            unsigned h0, m0, l0, h1, m1, l1;
            split_pair(v[0], v[1], h0, m0, l0);
            split_pair(v[2], v[3], h1, m1, l1);
            if (pix < HP) {
                float *d = xs + pix * XS + 2 * c4;
                *reinterpret_cast<u32x2 *>(d) = u32x2{h0, h1};
                *reinterpret_cast<u32x2 *>(d + XPL) = u32x2{m0, m1};
                *reinterpret_cast<u32x2 *>(d + 2 * XPL) = u32x2{l0, l1};
            }
        }
#pragma unroll
        for (int it = 0; it < NWT; ++it)
            if (it * 256 + tid < WF4) st4(ws + it * 1024 + 4 * tid, wr[it]);
        __syncthreads();
        if (ch + 1 < nchunk) prefetch(ch + 1);          // in flight during the MFMA phase below
        // ---- MFMA over the taps, software-pipelined by one tap (two register sets, statically indexed) ----
        {
            const float *wbase = ws + (wm * CB) * SLAB + lane * 4;
            f32x4 av[2][3][CB], bv[2][3][PBW];
#define UKBB_X3_LOAD_TAP(T, SET)                                                                    \
            {                                                                                      \
                constexpr int kh_ = (T) / 3, kw_ = (T) % 3;                                        \
                _Pragma("unroll") for (int p = 0; p < 3; ++p) {                                    \
                    _Pragma("unroll") for (int cb = 0; cb < CB; ++cb)                              \
                        av[SET][p][cb] = ld4(wbase + p * WPL + (cb * KS2 + (T)) * 256);            \
                    _Pragma("unroll") for (int pb = 0; pb < PBW; ++pb)                             \
                        bv[SET][p][pb] = ld4(xs + p * XPL + lbase[pb] + (kh_ * IW + kw_) * XS);    \
                }                                                                                  \
            }
            UKBB_X3_LOAD_TAP(0, 0)
            unroll<KS2>([&](auto tc) {
                constexpr int t = decltype(tc)::value;
                if constexpr (t + 1 < KS2) UKBB_X3_LOAD_TAP(t + 1, (t + 1) & 1)
                __builtin_amdgcn_sched_barrier(0);      // keep the reads of tap t + 1 ahead of the MFMAs of tap t
                // pieces 0 = h, 1 = m, 2 = l; (weight piece, activation piece) in the head's order: l.h h.l m.m m.h h.m h.h.  Pair outer,
                // accumulator inner: consecutive MFMAs write different accumulators, each accumulator sees the six in this order.
                constexpr int WP[6] = {2, 0, 1, 1, 0, 0}, XP[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
                for (int k = 0; k < 6; ++k)
#pragma unroll
                    for (int pb = 0; pb < PBW; ++pb)
#pragma unroll
                        for (int cb = 0; cb < CB; ++cb)
                            acc[cb][pb] = mfma_bf16(av[t & 1][WP[k]][cb], bv[t & 1][XP[k]][pb], acc[cb][pb]);
                __builtin_amdgcn_sched_barrier(0);
            });
#undef UKBB_X3_LOAD_TAP
        }
    }

    // ---- epilogue: + bias, ReLU, NHWC float4 stores (the fp32 kernels' epilogue) ----
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
        const int co0 = (cbg + cb) * 32 + 4 * g;
        float4 bi[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bi[j] = *reinterpret_cast<const float4 *>(a.bias + co0 + 8 * j);
#pragma unroll
        for (int pb = 0; pb < PBW; ++pb) {
            const int q = (wn + pb * WN) * PB + pl;
            const int oy = oy0 + q / TW, ox = ox0 + q % TW;
            if (q < NPIX && oy < a.Ho && ox < a.Wo) {
                float *o = a.out + ((size_t)(n * a.Ho + oy) * a.Wo + ox) * a.Cout + co0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float4 v;
                    v.x = acc[cb][pb][4 * j + 0] + bi[j].x;
                    v.y = acc[cb][pb][4 * j + 1] + bi[j].y;
                    v.z = acc[cb][pb][4 * j + 2] + bi[j].z;
                    v.w = acc[cb][pb][4 * j + 3] + bi[j].w;
                    if (a.relu) {
                        v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f);
                        v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
                    }
                    *reinterpret_cast<float4 *>(o + 8 * j) = v;
                }
            }
        }
    }
}

// X(id, STRIDE, TH, TW, WM, WN, CB).  12 x 13 tiles divide the 192 x 208 pyramid, 11 x 13 the long-axis models' 176 x 208, 8 x 16 the
// power-of-two maps; w2x2: 64 output channels per workgroup, w1x4: 32 (the 32-channel level 1, whose maps are never smaller than 8 x 8:
// four pixel waves leave three of a 12 x 13 tile's eight block slots idle, so level 1 has the 8 x 16 form only -- plan.cpp choose_x3_cfg)
#define UKBB_X3_CONFIGS(X)             \
    X(330, 1, 12, 13, 2, 2, 1)         \
    X(332, 1, 11, 13, 2, 2, 1)         \
    X(334, 1, 8, 16, 2, 2, 1)          \
    X(335, 1, 8, 16, 1, 4, 1)          \
    X(340, 2, 12, 13, 2, 2, 1)         \
    X(342, 2, 11, 13, 2, 2, 1)         \
    X(344, 2, 8, 16, 2, 2, 1)          \
    X(345, 2, 8, 16, 1, 4, 1)

#define UKBB_X3_ENTRY(ID, S, TH, TW, WM, WN, CB)                                                 \
    {ID, 3, S, 32, TH, TW, 16, WM, WN, CB, conv_x3_lds_bytes(S, TH, TW, WM, CB), ConvFamily::F32x3Operands, \
     "convF32x3_3x3s" #S "_t" #TH "x" #TW "_w" #WM "x" #WN "_cb" #CB},
const ConvConfig g_x3_cfgs[] = {UKBB_X3_CONFIGS(UKBB_X3_ENTRY)};

}  // namespace

int num_x3_configs() { return (int)(sizeof(g_x3_cfgs) / sizeof(g_x3_cfgs[0])); }
const ConvConfig &x3_config(int i) { return g_x3_cfgs[i]; }

hipError_t launch_conv_x3(int cfg_id, const ConvArgs &a, hipStream_t s) {
    const ConvConfig *c = nullptr;
    for (const auto &e : g_x3_cfgs) if (e.id == cfg_id) c = &e;
    if (!c) return hipErrorInvalidValue;
    const int group = cout_per_item(*c);
    // one fp32 source, whole 16-channel chunks and Cout groups, a plain conv; the tile grid must cover the output map and no more
    if (a.in1 || a.C1 || a.in0_map || a.up2 || a.C0 < 16 || a.C0 % 16 || a.Cout % group) return hipErrorInvalidValue;
    if (a.tiles_y != (a.Ho + c->th - 1) / c->th || a.tiles_x != (a.Wo + c->tw - 1) / c->tw) return hipErrorInvalidValue;
    if ((long long)a.N * a.H * a.W > 0x7fffffffll) return hipErrorInvalidValue;      // 32-bit pixel offsets
    dim3 grid((unsigned)(a.N * a.tiles_y * a.tiles_x), (unsigned)(a.Cout / group), 1);
    switch (cfg_id) {
#define UKBB_X3_CASE(ID, S, TH, TW, WM, WN, CB)                                                  \
    case ID: return launch_lds<conv_x3_kernel<S, TH, TW, WM, WN, CB>>(grid, dim3(256), c->lds_bytes, s, a);
        UKBB_X3_CONFIGS(UKBB_X3_CASE)
        default: return hipErrorInvalidValue;
    }
}

}  // namespace ukbb
