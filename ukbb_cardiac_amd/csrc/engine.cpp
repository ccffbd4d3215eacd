// Engine behind include/ukbb_fcn.h: owns device weights (BN folded, packed in
// MFMA fragment order) and the activation workspace in HBM; materialises the launch
// plan the host-only planner lays out (plan.h: layout_plan) and runs it.
//
// Reference counterpart: the TensorFlow session + restored graph of
// common/deploy_network.py:44-49 and the sess.run call at :110-111.
#include "../../include/ukbb_fcn.h"
#include "kernels.h"
#include "pack.h"
#include "plan.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

using namespace ukbb;

extern "C" int ukbb_fcn_debug_poison_lds(uint32_t pattern, void *stream);     // kernels_prep.hip (debugging aid, not in the public header)
extern "C" int ukbb_fcn_debug_fence_kernel(void *stream);                       // kernels_prep.hip (debugging aid)

namespace {

thread_local std::string g_err;

}  // namespace

void ukbb::set_error(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
}

namespace {

#define HIP_TRY(expr, code)                                                            \
    do {                                                                               \
        hipError_t e_ = (expr);                                                        \
        if (e_ != hipSuccess) {                                                        \
            set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return code;                                                               \
        }                                                                              \
    } while (0)

constexpr float BN_EPS = 1e-3f;   // tf.layers.batch_normalization default

struct HostLayer {            // one conv(+BN) unit with BN folded (fp32, same op order as
    std::string name;         // ukbb_cardiac_amd/weights.py fold_bn)
    int ks = 0, cin = 0, cout = 0;
    int kd = 1;               // time taps (3: a conv3d / conv3d_transpose of the Temporal-UNet)
    bool transposed = false, relu = true;
    std::vector<float> w;     // [kd][ks][ks][cin][cout], scale folded in
    std::vector<float> b;     // [cout]
};

// Debugging aid (UKBB_DEBUG_GUARD=<hex pattern> at ukbb_fcn_create, kept per handle): every DevBuf of the handle is allocated as
// guard | payload | guard.  The guards hold GUARD_BYTE; a payload is filled with the pattern when it is allocated, before anything is
// uploaded into it or cleared.  ukbb_fcn_debug_check_guards reads the guards back, ukbb_fcn_debug_poison refills the payloads the
// engine rewrites on every call.  GUARD_BYTES is a power of two, so the payload keeps the alignment hipMalloc gave.
constexpr size_t GUARD_BYTES = (size_t)1 << 20;
constexpr unsigned char GUARD_BYTE = 0xA5;

struct GuardMode {
    bool on = false;
    uint32_t pattern = 0;
};

struct DevBuf {
    float *p = nullptr;
    size_t n = 0;
    const GuardMode *guard = nullptr;       // the owning handle's mode (NULL / off: plain allocations)
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete; DevBuf &operator=(const DevBuf &) = delete;   // owns p
    ~DevBuf() { release(); }
    static size_t units(size_t bytes) { return (bytes + 3) / 4; }   // n counts floats: the 4-byte units that hold `bytes` (bf16 maps, int / double tables)
    hipError_t ensure_bytes(size_t bytes) { return ensure(units(bytes)); }
    bool guarded() const { return guard && guard->on; }
    void release() {
        if (p) (void)hipFree(guarded() ? reinterpret_cast<char *>(p) - GUARD_BYTES : reinterpret_cast<char *>(p));
        p = nullptr; n = 0;
    }
    hipError_t ensure(size_t want) {
        if (want <= n) return hipSuccess;
        release();
        if (guarded()) return ensure_guarded(want);
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&p), want * sizeof(float));
        if (e == hipSuccess) n = want;
        return e;
    }
    hipError_t ensure_guarded(size_t want) {
        char *base = nullptr;
        const size_t bytes = want * sizeof(float);
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&base), bytes + 2 * GUARD_BYTES);
        if (e != hipSuccess) return e;
        // the fills are ordered against every stream of the process: a debugging mode pays for two device-wide waits per allocation
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipMemset(base, GUARD_BYTE, GUARD_BYTES);
        if (e == hipSuccess) e = hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(base + GUARD_BYTES), (int)guard->pattern, want);
        if (e == hipSuccess) e = hipMemset(base + GUARD_BYTES + bytes, GUARD_BYTE, GUARD_BYTES);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) { (void)hipFree(base); return e; }
        p = reinterpret_cast<float *>(base + GUARD_BYTES);
        n = want;
        return hipSuccess;
    }
    hipError_t upload(const std::vector<float> &v) {
        hipError_t e = ensure(v.size());
        if (e != hipSuccess) return e;
        return hipMemcpy(p, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice);
    }
};

// element k of a buffer whose stored elements take esz bytes (2: bf16; the pointers travel as float * either way)
float *at(float *p, size_t k, size_t esz) { return reinterpret_cast<float *>(reinterpret_cast<char *>(p) + k * esz); }

struct ActMap {               // one activation map of the plan's workspace
    DevBuf buf;
    size_t per_image = 0;     // elements per image at the planned H,W
    int esz = 4, alloc_esz = 4;   // bytes of a stored element (2: bf16) / bytes the workspace holds per element (plan.h act_alloc_esz)
    int ch = 0;               // channels of the map (0: not a channel map); bf16 plans store maps with C > 16 channel-blocked
    std::string name;
    float *image(int n0) const { return at(buf.p, (size_t)n0 * per_image, esz); }
    size_t units(int n) const { return DevBuf::units(per_image * (size_t)n * alloc_esz); }   // what buf.ensure takes for n images
};

struct BoundOp : Op {         // the planner's op and the device pointers its launch takes, resolved by materialize_plan
    explicit BoundOp(Op op) : Op(std::move(op)) {}
    const float *wpk = nullptr, *bias = nullptr;                  // packed weights / bias of the op's own layer
    const float *wph[4] = {nullptr, nullptr, nullptr, nullptr};   // OP_TCONV3D: packed weights of the 4 sub-pixel phases
    const float *sq_w_s[4] = {}, *sq_b_s[4] = {}, *sq_w_g[4] = {};   // OP_SQG ([0]) / OP_SQG_MULTI (levels 1..4): squeeze matrix, its bias, out0's slice
};

// The parameters ops share or the ConvLSTM stages read: bound by bind_op / bind_lstm for what the current plan launches, null otherwise.
struct Params {
    const float *conv0_w, *conv0_b, *conv0_1_b, *up0_0_b, *up0_1_b, *logits_w, *logits_b;
    const float *stem_wA0, *stem_wA1, *tail_wA0, *tail_wA1;
    const float *head_w_s0, *head_b_s0, *head_w_o0, *head_b_o0, *head_w_o1, *head_b_o1, *head_w_o1x3, *head_w_o0x3, *head_w_lg;
    const float *head_w_s0bf, *head_w_o0bf, *head_w_o1bf;         // UKBB_PREC_BF16_FULL: pack_head_bf16 of same_dim0, out0's level-0 slice, out1
    struct { const float *wx, *bx, *wh[2]; } lstm[2];             // ConvLSTM filters per form ([0] fp32 Winograd, [1] bf16 direct) and direction
    const float *lstm_wxh[2];                                     // ... un-hoisted bf16 time steps, per direction
    const float *lstm_out_w, *lstm_out_b;
};

// A row of HANDLE_BUFS (behind the handle).  name: in the guard reports; rewritten: a call rewrites it before it reads it, so ukbb_fcn_debug_poison may refill
// it (not: the staged input, tables uploaded once per shape); raw: the name under which ukbb_fcn_get_activation hands it out raw (NULL: it does not)
struct HandleBuf { const char *name; DevBuf ukbb_fcn_handle::*buf; bool rewritten; const char *raw; };

}  // namespace

struct ukbb_fcn_handle {
    ukbb_fcn_arch arch{};
    int device = 0;
    GuardMode guard;                          // UKBB_DEBUG_GUARD at create (debugging aid): every DevBuf below points at it
    std::vector<HostLayer> layers;
    std::map<std::string, int> layer_index;

    // device-side parameters
    std::map<std::string, std::unique_ptr<DevBuf>> dev;   // keyed by "<layer>/<what>": the owner; launches read the pointers below
    Params par{};                             // bound when a plan is materialised

    // activation workspace
    std::vector<ActMap> acts;
    DevBuf io_image, io_logits, io_prob, io_pred;   // staging for forward_host

    // plan
    int precision = UKBB_PREC_FP32;           // the code the next plan is built for (ukbb_fcn_set_precision)
    bool f32x3_convs = false;                 // ukbb_fcn_set_f32x3_convs: plans made under UKBB_PREC_F32X3 run the 3x3 layers on three bf16 pieces too
    PlanLayout plan;                          // the CURRENT plan as layout_plan decided it (plan.h); its ops are bound in `ops`, its acts materialised in `acts`
    int plan_h = 0, plan_w = 0, cap_n = 0;
    bool plan_small = false;                  // plan built with the small-batch tilings
    int plan_n = 0;                           // ... for this largest batch
    int max_n = 0;                            // largest batch this handle was asked for (reserve / forward): the small-batch plan is
                                              // used only while that stays <= SMALL_BATCH, so a large-batch caller's tail batches do
                                              // not flip the plan (a rebuild re-allocates the workspace) back and forth
    std::vector<BoundOp> ops;
    CineUnits cine;                           // what forward_cine holds per frame / window of this plan (plan.h)
    int last_n = 0;

    // UNet-LSTM (kind 2)
    bool lstm_bw_zero = false;                // the backward cell's kernel and bias are all zero (the single-direction head Conv_LSTM of network_ao.py:214-252 embedded by
                                              // weights.embed_unidirectional_lstm): its hidden maps are exactly zero, run_bilstm clears them instead of running its time steps
    // lstm_gx / lstm_c1 / lstm_h1: per direction and FRAME (the x pass); lstm_c: per window; lstm_hall: per direction, step and window
    DevBuf lstm_gx, lstm_c1, lstm_h1, lstm_c, lstm_hall, lstm_probw, lstm_aux;   // lstm_aux: int maps / orders / double weights (raw bytes)
    long long lstm_aux_key = -1;              // which tables lstm_aux holds (shape-keyed, uploaded once per shape)
    DevBuf lstm_img;                          // forward_cine in chunks: the chunk's frame run, contiguous (a run may wrap from frame F-1 to 0)

    // forward_cine scratch budget (ukbb_fcn_set_scratch_budget; 0 = none)
    uint64_t scratch_budget = 0;
    long long budget_key = -1;                // the (shape, chunk plan) the buffers were allocated for under the budget

    // Temporal-UNet (kind 3)
    const int *t3d_map = nullptr;             // first layer: batch image n reads frame t3d_map[n] (NULL: frame n); set around run_plan
    DevBuf t3d_aux, t3d_probw;                // forward_cine tables (window -> frame map, per-frame order, weights); softmax of a chunk's window frames
    long long t3d_aux_key = -1;

    // image-slice streams (experiment UKBB_SPLIT, run_plan): consecutive conv ops run as S independent image ranges on S streams
    // side stream for kernels that only feed the head (sqg_l): fork after level l, join before the head
    hipStream_t side = nullptr, side2 = nullptr;
    hipEvent_t ev_split_fork = nullptr, ev_split_join = nullptr;
    std::vector<hipEvent_t> ev_fork, ev_join;

    // UKBB_DEBUG_POISON_LDS (debugging aid): read once per API call (lds_poison_begin), consulted in front of every launch (announce_launch)
    bool lds_poison_on = false;
    uint32_t lds_poison_pat = 0;
    uint64_t n_launches = 0, n_lds_poisons = 0;   // since the handle was created (ukbb_fcn_debug_launch_counts)

    // timing
    bool timing = false;
    int timing_only = -1;                     // -1: every kernel; else only this op index
    std::vector<hipEvent_t> ev;               // 2 per op
    std::vector<double> t_sum;
    std::vector<int64_t> t_cnt;
    bool ev_pending = false;

    ukbb_fcn_handle();                        // wires the guard mode into the buffers of HANDLE_BUFS
    ~ukbb_fcn_handle() {
        for (auto e : ev) (void)hipEventDestroy(e);
        if (ev_split_fork) (void)hipEventDestroy(ev_split_fork);
        if (ev_split_join) (void)hipEventDestroy(ev_split_join);
        if (side2) (void)hipStreamDestroy(side2);
        for (auto e : ev_fork) (void)hipEventDestroy(e);
        for (auto e : ev_join) (void)hipEventDestroy(e);
        if (side) (void)hipStreamDestroy(side);
    }
};

// THE list of the DevBufs a handle owns besides its parameters (dev) and its activation maps (acts): each is guarded, named and counted as scratch.
static const HandleBuf HANDLE_BUFS[] = {
    {"io_image", &ukbb_fcn_handle::io_image, false, nullptr},  {"io_logits", &ukbb_fcn_handle::io_logits, true, nullptr},
    {"io_prob", &ukbb_fcn_handle::io_prob, true, nullptr},     {"io_pred", &ukbb_fcn_handle::io_pred, true, nullptr},
    {"lstm_gx", &ukbb_fcn_handle::lstm_gx, true, "lstm:gx"},   {"lstm_c1", &ukbb_fcn_handle::lstm_c1, true, "lstm:c1"},
    {"lstm_h1", &ukbb_fcn_handle::lstm_h1, true, "lstm:h1"},   {"lstm_c", &ukbb_fcn_handle::lstm_c, true, "lstm:c"},
    {"lstm_hall", &ukbb_fcn_handle::lstm_hall, true, "lstm:hall"}, {"lstm_probw", &ukbb_fcn_handle::lstm_probw, true, nullptr},
    {"lstm_aux", &ukbb_fcn_handle::lstm_aux, false, nullptr},  {"lstm_img", &ukbb_fcn_handle::lstm_img, true, nullptr},
    {"t3d_aux", &ukbb_fcn_handle::t3d_aux, false, nullptr},    {"t3d_probw", &ukbb_fcn_handle::t3d_probw, true, nullptr},
};
ukbb_fcn_handle::ukbb_fcn_handle() { for (const HandleBuf &b : HANDLE_BUFS) (this->*b.buf).guard = &guard; }

namespace {

// THE search of h->dev, for the packers ("is it on the device yet": NULL) and find_param.  Nothing a forward runs through calls it.
const float *dev_ptr(ukbb_fcn_handle *h, const std::string &key) {
    auto it = h->dev.find(key);
    return it == h->dev.end() ? nullptr : it->second->p;
}

// The device parameter `key` for `who` (an op, a layer or a stage of the plan being materialised): a missing one is an error here, never a null kernel argument.
int find_param(ukbb_fcn_handle *h, const std::string &key, const std::string &who, const float **out) {
    *out = dev_ptr(h, key);
    if (*out) return UKBB_OK;
    set_error("plan: %s needs the device parameter '%s', which the handle does not hold", who.c_str(), key.c_str());
    return UKBB_EARCH;
}

int upload(ukbb_fcn_handle *h, const std::string &key, const std::vector<float> &v) {
    auto &slot = h->dev[key];
    if (!slot) { slot.reset(new DevBuf); slot->guard = &h->guard; }
    HIP_TRY(slot->upload(v), UKBB_EDEVICE);
    return UKBB_OK;
}

// ---- plan: materialise a PlanLayout (plan.h) on the device -------------------------------------------------------------
int ensure_packed(ukbb_fcn_handle *h, int layer, const ConvConfig &c, const float **wpk, const float **bias) {
    const HostLayer &L = h->layers[layer];
    char key[128];
    const int coutp = packed_cout(c, L.cout);
    const size_t rows = (size_t)L.ks * L.ks * L.cin;
    std::vector<float> pk;
    auto fresh = [&](const char *suffix, size_t floats) {     // names the buffer of this packing; true, with pk sized, if it is not on the device yet
        snprintf(key, sizeof key, "%s/pk%s_mb%d_kc%d_g%d", L.name.c_str(), suffix, c.mb, c.kc, c.wm * c.cb);
        if (!dev_ptr(h, key)) pk.resize(floats);
        return !pk.empty();
    };
    switch (c.family) {
        case ConvFamily::Direct: case ConvFamily::ProdCons: case ConvFamily::ProdConsFirst:
            if (fresh("", rows * coutp)) pack_conv_weights(L.w.data(), L.ks, L.cin, L.cout, c.mb, c.kc, c.wm * c.cb, pk.data());
            break;
        case ConvFamily::Bf16Operands: case ConvFamily::Bf16Store: case ConvFamily::Bf16StoreWs:
            if (fresh("bf16", rows * coutp)) {
                std::vector<float> wp(rows * coutp, 0.f);         // zero rows up to the MFMA's 32 where coutp > cout
                for (size_t r = 0; r < rows; ++r) std::copy(L.w.begin() + r * L.cout, L.w.begin() + (r + 1) * L.cout, wp.begin() + r * coutp);
                pack_conv_weights_bf16(wp.data(), L.ks, L.cin, coutp, c.wm * c.cb, pk.data());
            }
            break;
        case ConvFamily::F32x3Operands:
            if (fresh("x3", 3 * rows * coutp / 2)) pack_conv_x3(L.w.data(), L.cin, L.cout, c.wm * c.cb, pk.data());
            break;
        case ConvFamily::Wino22: if (fresh("wino", (size_t)16 * L.cin * L.cout)) pack_wino_weights(L.w.data(), L.cin, L.cout, c.wm, pk.data()); break;
        case ConvFamily::Wino24: if (fresh("wino24", (size_t)24 * L.cin * L.cout)) pack_wino24_weights(L.w.data(), L.cin, L.cout, c.wm, pk.data()); break;
        case ConvFamily::FirstWino22:
            if (L.ks != 3 || L.cin != 16 || L.cout != 16) { set_error("layer %s: the Winograd first-layer tiling needs a 16 -> 16 3x3 conv", L.name.c_str()); return UKBB_EARCH; }
            if (fresh("winofirst", (size_t)16 * L.cin * L.cout)) pack_wino_first_weights(L.w.data(), pk.data());
            break;
    }
    if (!pk.empty()) {
        int rc = upload(h, key, pk);
        if (rc) return rc;
    }
    if (coutp != L.cout && !dev_ptr(h, L.name + "/bias_pad")) {
        std::vector<float> bp((size_t)coutp, 0.f);
        std::copy(L.b.begin(), L.b.end(), bp.begin());
        int rc = upload(h, L.name + "/bias_pad", bp);
        if (rc) return rc;
    }
    const int rc = find_param(h, key, L.name, wpk);
    return rc ? rc : find_param(h, L.name + (coutp != L.cout ? "/bias_pad" : "/bias"), L.name, bias);
}

// conv2d_transpose 3x3 s2 + BN + ReLU as a 2x2 sub-pixel conv (pack.h, tconv_as_conv2x2): packed weights and the bias of the 4 phases
int ensure_packed_tconv(ukbb_fcn_handle *h, int layer, const ConvConfig &c, const float **wpk, const float **bias) {
    const HostLayer &L = h->layers[layer];
    char key[128];
    const bool bfpk = packs_bf16(c);
    const bool paired = c.family == ConvFamily::Bf16StoreWs;   // weight-stationary tilings: virtual channels in the paired block order (wst_pack_order)
    snprintf(key, sizeof key, "%s/pk2x2%s%s_mb%d_kc%d_g%d", L.name.c_str(), bfpk ? "bf16" : "", paired ? "ws" : "", c.mb, c.kc, c.wm * c.cb);
    const std::string bkey = L.name + (paired ? "/bias4ws" : "/bias4");
    if (!dev_ptr(h, key)) {
        const int vc = 4 * L.cout;
        std::vector<float> w2((size_t)4 * L.cin * vc), pk(w2.size());
        tconv_as_conv2x2(L.w.data(), L.cin, L.cout, w2.data());
        std::vector<float> b4((size_t)vc);
        for (int ph = 0; ph < 4; ++ph) std::copy(L.b.begin(), L.b.end(), b4.begin() + (size_t)ph * L.cout);
        if (paired) {
            std::vector<float> w2p(w2.size()), b4p(b4.size());
            for (int v = 0; v < vc; ++v) {
                const int src = wst_pack_order(L.cout, v);
                b4p[v] = b4[src];
                for (size_t r = 0; r < (size_t)4 * L.cin; ++r) w2p[r * vc + v] = w2[r * vc + src];
            }
            w2.swap(w2p); b4.swap(b4p);
        }
        if (bfpk) pack_conv_weights_bf16(w2.data(), 2, L.cin, vc, c.wm * c.cb, pk.data());
        else pack_conv_weights(w2.data(), 2, L.cin, vc, c.mb, c.kc, c.wm * c.cb, pk.data());
        int rc = upload(h, key, pk);
        if (rc) return rc;
        rc = upload(h, bkey, b4);
        if (rc) return rc;
    }
    const int rc = find_param(h, key, L.name, wpk);
    return rc ? rc : find_param(h, bkey, L.name, bias);
}

// Temporal-UNet (kind 3), kernels_conv3d.hip:
// Weights of conv3d (kernel order (kt, ky, kx)) or of one sub-pixel phase (py, px) of conv3d_transpose (kt reversed: the
// transposed conv reads in[t + 1 - kt], kernels_conv3d.hip), packed for conv3d_kernel; key "<layer>/pk3d<phase>".  bf16 (UKBB_PREC_BF16_3D): the
// same fold rounded once to bf16, packed for conv3d_bf16_kernel (kernels_conv3d_bf16.hip); key "<layer>/pk3d<phase>bf16".  A handle that
// switches precision holds both.
const float *ensure_packed3d(ukbb_fcn_handle *h, const HostLayer &L, int py, int px, int ny, int nx, bool bf16) {
    char key[128];
    snprintf(key, sizeof key, "%s/pk3d%d%d%s", L.name.c_str(), py, px, bf16 ? "bf16" : "");
    if (const float *p = dev_ptr(h, key)) return p;
    const int ntap = 3 * ny * nx, cpad = round_up(L.cout, 32);
    std::vector<float> w((size_t)ntap * L.cin * L.cout), pk((size_t)ntap * L.cin * cpad / (bf16 ? 2 : 1));
    for (int dti = 0; dti < 3; ++dti)
        for (int jy = 0; jy < ny; ++jy)
            for (int jx = 0; jx < nx; ++jx) {
                const int kt = L.transposed ? 2 - dti : dti;
                const int ky = L.transposed ? py + 2 * jy : jy, kx = L.transposed ? px + 2 * jx : jx;
                const size_t src = (((size_t)kt * 3 + ky) * 3 + kx) * L.cin * L.cout, dst = (((size_t)dti * ny + jy) * nx + jx) * L.cin * L.cout;
                std::copy(L.w.begin() + src, L.w.begin() + src + (size_t)L.cin * L.cout, w.begin() + dst);
            }
    if (bf16) pack_conv3d_weights_bf16(w.data(), ntap, L.cin, L.cout, cpad, pk.data());
    else pack_conv3d_weights(w.data(), ntap, L.cin, L.cout, cpad, pk.data());
    if (upload(h, key, pk)) return nullptr;
    return dev_ptr(h, key);
}

// bf16 storage: the 1 -> 16 -> 16 stem as one launch (kernels_stem.hip)
int ensure_packed_stem(ukbb_fcn_handle *h) {
    if (dev_ptr(h, "stem/wA0")) return UKBB_OK;
    const HostLayer &L0 = h->layers[h->layer_index.at("conv0_0")], &L1 = h->layers[h->layer_index.at("conv0_1")];
    std::vector<float> p0((size_t)64 * 4), dummy((size_t)9 * 64 * 4), p1((size_t)5 * 64 * 4), w0z((size_t)9 * 32 * 16, 0.f);
    pack_stem_weights(L0.w.data(), p0.data());
    pack_tail_weights(w0z.data(), L1.w.data(), dummy.data(), p1.data());
    const int rc = upload(h, "stem/wA1", p1);
    return rc ? rc : upload(h, "stem/wA0", p0);            // last: its key stands for the pair (above)
}

// bf16 storage: up0_0, up0_1 and the logits as one launch (kernels_tail.hip)
int ensure_packed_tail(ukbb_fcn_handle *h) {
    if (dev_ptr(h, "tail/wA0")) return UKBB_OK;
    const HostLayer &L0 = h->layers[h->layer_index.at("up0_0")], &L1 = h->layers[h->layer_index.at("up0_1")];
    std::vector<float> p0((size_t)9 * 64 * 4), p1((size_t)5 * 64 * 4);
    pack_tail_weights(L0.w.data(), L1.w.data(), p0.data(), p1.data());
    const int rc = upload(h, "tail/wA1", p1);
    return rc ? rc : upload(h, "tail/wA0", p0);            // last: its key stands for the pair (above)
}

// ConvLSTM packed filters: the x rows of both directions as ONE 128-channel conv (groups = directions), the h rows per direction; in the
// fp32 Winograd form and the bf16 form (kernels_ws.hip, ws_main LS: direct 3x3 conv on the bf16 matrix instruction, its own channel order)
int ensure_packed_lstm(ukbb_fcn_handle *h) {
    if (dev_ptr(h, "lstm/wx")) return UKBB_OK;
    const int nf0 = h->arch.n_filter[0];
    const size_t per = (size_t)24 * 16 * 64, perb = (size_t)9 * 16 * 64 / 2;          // perb: dwords
    std::vector<float> wx(2 * per), bx(2 * 64), wh(per), wxb(2 * perb), bxb(2 * 64), whb(perb);
    int rc = UKBB_OK, d = 0;
    for (const std::string nm2 : {"lstm_fw", "lstm_bw"}) {
        const HostLayer &L = h->layers[h->layer_index.at(nm2)];
        if (L.cin != 32 || L.cout != 64 || L.ks != 3) { set_error("ConvLSTM gate kernel must be 3x3x(16+16)x64"); return UKBB_EARCH; }
        pack_lstm_gate_weights(L.w.data(), L.cin, 0, L.b.data(), wx.data() + d * per, bx.data() + d * 64);
        pack_lstm_gate_weights(L.w.data(), L.cin, nf0, nullptr, wh.data(), nullptr);
        pack_lstm_gate_weights_bf16(L.w.data(), L.cin, 0, L.b.data(), wxb.data() + d * perb, bxb.data() + d * 64);
        pack_lstm_gate_weights_bf16(L.w.data(), L.cin, nf0, nullptr, whb.data(), nullptr);
        std::vector<float> wxhb(2 * perb);               // r06: both halves as one two-chunk filter (un-hoisted time steps, ls_mode 3)
        pack_lstm_gate_weights_bf16_xh(L.w.data(), nullptr, wxhb.data(), nullptr);
        if (!rc) rc = upload(h, nm2 + "/wh", wh);
        if (!rc) rc = upload(h, nm2 + "/wh_bf16", whb);
        if (!rc) rc = upload(h, nm2 + "/wxh_bf16", wxhb);
        ++d;
    }
    if (!rc) rc = upload(h, "lstm/bx", bx);
    if (!rc) rc = upload(h, "lstm/wx_bf16", wxb);
    if (!rc) rc = upload(h, "lstm/bx_bf16", bxb);
    return rc ? rc : upload(h, "lstm/wx", wx);            // last: its key stands for the whole set (above)
}

// Packs and uploads what `op`'s kind and tiling need and fills every device pointer its launch takes: the op's own and the shared ones
// of h->par.  The launches search nothing afterwards; a key the handle lacks ends the plan here, with UKBB_EARCH.  mode: of the plan being bound.
int bind_op(ukbb_fcn_handle *h, BoundOp &op, const PlanMode &mode) {
    Params &P = h->par;
    const std::string who = "op " + op.name, lname = op.layer >= 0 ? h->layers[op.layer].name : std::string();
    int rc = UKBB_OK;
    auto need = [&](const float *&dst, const std::string &key) { if (!rc) rc = find_param(h, key, who, &dst); };
    auto sqg = [&](int j, int level, int layer) {
        const std::string ls = std::to_string(level);
        need(op.sq_w_s[j], "sqg" + ls + "/w_s"); need(op.sq_b_s[j], h->layers[layer].name + "/bias"); need(op.sq_w_g[j], "sqg" + ls + "/w_g");
    };
    auto conv0 = [&] { need(P.conv0_w, "conv0_0/w"); need(P.conv0_b, "conv0_0/bias"); };
    auto logits = [&] { need(P.logits_w, "logits/w"); need(P.logits_b, "logits/bias"); };
    ConvConfig c;
    switch (op.kind) {
        case OP_FIRST: need(op.wpk, lname + "/w"); need(op.bias, lname + "/bias"); break;
        case OP_CONV:
        case OP_TCONV:
            find_cfg(op.cfg, c);
            rc = (op.kind == OP_CONV ? ensure_packed : ensure_packed_tconv)(h, op.layer, c, &op.wpk, &op.bias);
            if (op.fused_first) conv0();
            if (op.fused_logits) logits();
            break;
        case OP_SQG: sqg(0, op.stride, op.layer); break;
        case OP_SQG_MULTI:
            for (int j = 0; j < 4; ++j) if (op.mlayer[j] >= 0) sqg(j, j + 1, op.mlayer[j]);
            break;
        case OP_HEAD:
            need(P.head_w_s0, "head/w_s0"); need(P.head_b_s0, "same_dim0/bias"); need(P.head_w_o0, "head/w_o0"); need(P.head_b_o0, "out0/bias");
            need(P.head_w_o1, "head/w_o1"); need(P.head_b_o1, "out1/bias"); need(P.head_w_o1x3, "head/w_o1x3"); need(P.head_w_o0x3, "head/w_o0x3");
            need(P.head_w_lg, "head/w_lg"); need(P.logits_b, "logits/bias");
            if (mode.head_bf16) { need(P.head_w_s0bf, "head/w_s0bf"); need(P.head_w_o0bf, "head/w_o0bf"); need(P.head_w_o1bf, "head/w_o1bf"); }
            break;
        case OP_STEM:
            rc = ensure_packed_stem(h);
            need(P.stem_wA0, "stem/wA0"); need(P.stem_wA1, "stem/wA1"); need(P.conv0_1_b, "conv0_1/bias"); conv0();
            break;
        case OP_TAIL:
            rc = ensure_packed_tail(h);
            need(P.tail_wA0, "tail/wA0"); need(P.tail_wA1, "tail/wA1"); need(P.up0_0_b, "up0_0/bias"); need(P.up0_1_b, "up0_1/bias"); logits();
            break;
        case OP_LOGITS: logits(); break;
        case OP_FIRST3D: conv0(); need(op.bias, lname + "/bias"); break;
        case OP_CONV3D:
            if (!(op.wpk = ensure_packed3d(h, h->layers[op.layer], 0, 0, 3, 3, mode.bfio()))) rc = UKBB_EDEVICE;
            need(op.bias, lname + "/bias");
            break;
        case OP_TCONV3D:
            for (int ph = 0; ph < 4 && !rc; ++ph) {
                const int py = ph >> 1, px = ph & 1;
                if (!(op.wph[ph] = ensure_packed3d(h, h->layers[op.layer], py, px, py ? 1 : 2, px ? 1 : 2, mode.bfio()))) rc = UKBB_EDEVICE;
            }
            need(op.bias, lname + "/bias");
            break;
    }
    return rc;
}

// ... and what the ConvLSTM stages behind the plan take: run_bilstm and the two output kernels
int bind_lstm(ukbb_fcn_handle *h) {
    const HostLayer &B = h->layers[h->layer_index.at("lstm_bw")];
    bool z = getenv("UKBB_LSTM_RUN_ZERO_CELL") == nullptr;      // knob: run the zero cell anyway (tests compare both ways)
    for (size_t i = 0; z && i < B.w.size(); ++i) z = B.w[i] == 0.f;
    for (size_t i = 0; z && i < B.b.size(); ++i) z = B.b[i] == 0.f;
    h->lstm_bw_zero = z;
    int rc = ensure_packed_lstm(h);
    Params &P = h->par;
    auto need = [&](const float *&dst, const std::string &key) { if (!rc) rc = find_param(h, key, "the ConvLSTM", &dst); };
    const std::string dirs[2] = {"lstm_fw", "lstm_bw"};
    for (int f = 0; f < 2; ++f) {
        const char *form = f ? "_bf16" : "";
        need(P.lstm[f].wx, std::string("lstm/wx") + form); need(P.lstm[f].bx, std::string("lstm/bx") + form);
        for (int d = 0; d < 2; ++d) need(P.lstm[f].wh[d], dirs[d] + "/wh" + form);
    }
    for (int d = 0; d < 2; ++d) need(P.lstm_wxh[d], dirs[d] + "/wxh_bf16");
    need(P.lstm_out_w, "lstm_out/w"); need(P.lstm_out_b, "lstm_out/bias");
    return rc;
}

// Takes the layout into the handle: its maps, its ops bound to the device parameters (bind_op, bind_lstm); resets the previous plan's events and timing sums.
int materialize_plan(ukbb_fcn_handle *h, PlanLayout &L) {
    h->ops.clear();
    h->acts = std::vector<ActMap>(L.acts.size());
    h->cap_n = 0;
    h->par = Params{};
    for (size_t i = 0; i < L.acts.size(); ++i) {
        const ActSpec &s = L.acts[i];
        ActMap &m = h->acts[i];
        m.buf.guard = &h->guard; m.name = s.name;
        m.per_image = s.per_image; m.esz = s.esz; m.alloc_esz = (int)act_alloc_esz(h->arch, s); m.ch = s.channels;
    }
    std::vector<BoundOp> ops;
    for (const Op &op : L.ops) {
        ops.emplace_back(op);
        const int rc = bind_op(h, ops.back(), L.mode);
        if (rc) return rc;
    }
    if (L.needs_lstm) {
        const int rc = bind_lstm(h);
        if (rc) return rc;
    }
    h->ops = std::move(ops);
    h->plan = std::move(L);
    for (auto e : h->ev) (void)hipEventDestroy(e);
    h->ev.clear();
    h->t_sum.assign(h->ops.size(), 0.0);
    h->t_cnt.assign(h->ops.size(), 0);
    h->ev_pending = false;
    return UKBB_OK;
}

int build_plan(ukbb_fcn_handle *h, int H, int W, int n_hint) {
    PlanLayout L;
    int rc = layout_plan(h->arch, h->precision, H, W, n_hint, device_cu_count(), L, h->f32x3_convs);
    if (rc) return rc;
    h->cine = cine_units_from(L, h->arch, H, W);
    rc = materialize_plan(h, L);
    if (rc) return rc;
    h->plan_h = H; h->plan_w = W; h->plan_small = n_hint <= SMALL_BATCH; h->plan_n = n_hint;
    return UKBB_OK;
}

int ensure_capacity(ukbb_fcn_handle *h, int n) {
    if (n <= h->cap_n) return UKBB_OK;
    for (ActMap &m : h->acts) HIP_TRY(m.buf.ensure(m.units(n)), UKBB_ENOMEM);
    h->cap_n = n;
    return UKBB_OK;
}

int check_shape(int n, int H, int W) {
    if (n < 1 || H < 16 || W < 16 || (H % 16) || (W % 16)) {
        set_error("invalid batch shape n=%d h=%d w=%d: h and w must be positive multiples of 16 "
                "(the reference pads to that, common/deploy_network.py:97)", n, H, W);
        return UKBB_EINVAL;
    }
    if ((long long)n * H * W > (1ll << 31) - 1) { set_error("batch too large for 32-bit pixel indexing"); return UKBB_EINVAL; }
    return UKBB_OK;
}

// n: the batch the plan is chosen for; cap (>= 0): the batch the workspace is sized for when that is smaller (forward_cine in chunks; 0: plan only)
int prepare(ukbb_fcn_handle *h, int n, int H, int W, int cap = -1) {
    int rc = check_shape(n, H, W);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device), UKBB_EDEVICE);
    if (n > h->max_n) h->max_n = n;
    // the finer siblings of the small-batch plan are chosen from the work items at the largest batch seen (finer_sibling): while the
    // handle stays in the small regime a larger batch re-plans (a handle first used at N = 1 must not keep halved items at N = 16)
    if (H != h->plan_h || W != h->plan_w || (h->max_n <= SMALL_BATCH) != h->plan_small || (h->plan_small && h->max_n > h->plan_n)) {
        HIP_TRY(hipDeviceSynchronize(), UKBB_EDEVICE);
        rc = build_plan(h, H, W, h->max_n);
        if (rc) { h->plan_h = h->plan_w = 0; return rc; }
    }
    if (cap >= 0 && cap < n) n = cap;
    if (n > h->cap_n) {
        HIP_TRY(hipDeviceSynchronize(), UKBB_EDEVICE);
        rc = ensure_capacity(h, n);
        if (rc) return rc;
    }
    return UKBB_OK;
}

// ukbb_fcn_forward / ukbb_fcn_forward_host (`what`) take batches of single images
int refuse_sequence_kinds(const ukbb_fcn_handle *h, const char *what) {
    if (h->arch.kind != UKBB_KIND_UNET_LSTM && h->arch.kind != UKBB_KIND_TEMPORAL_UNET) return UKBB_OK;
    set_error("%s: %s models take sequences: use ukbb_fcn_forward_seq / ukbb_fcn_forward_cine", what, h->arch.kind == UKBB_KIND_UNET_LSTM ? "UNet-LSTM" : "Temporal-UNet");
    return UKBB_EINVAL;
}

int collect_events(ukbb_fcn_handle *h) {
    if (!h->ev_pending) return UKBB_OK;
    HIP_TRY(hipEventSynchronize(h->ev[h->timing_only >= 0 ? 2 * h->timing_only + 1 : h->ev.size() - 1]), UKBB_EDEVICE);
    for (size_t i = 0; i < h->ops.size(); ++i) {
        if (h->timing_only >= 0 && (int)i != h->timing_only) continue;
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, h->ev[2 * i], h->ev[2 * i + 1]), UKBB_EDEVICE);
        h->t_sum[i] += ms;
        h->t_cnt[i] += 1;
    }
    h->ev_pending = false;
    return UKBB_OK;
}

// what a forward reads and writes besides the workspace: the caller's device pointers (an output may be NULL)
struct PlanIo { const float *image; float *logits, *prob; int32_t *pred; };

// UKBB_DEBUG_POISON_LDS=<hex pattern>: every CU's LDS is filled with the pattern in front of EVERY launch the handle makes -- a kernel that
// reads LDS it never wrote now reads this pattern.  The API entries read the variable (once per call); every launch site of the handle
// (launch_op, the ConvLSTM x pass and time steps, lstm_out, lstm_tile, t3d_tile) announces its launch and the stream it goes to here.
void lds_poison_begin(ukbb_fcn_handle *h) {
    const char *env = getenv("UKBB_DEBUG_POISON_LDS");
    h->lds_poison_on = env != nullptr;
    h->lds_poison_pat = env ? (uint32_t)strtoul(env, nullptr, 16) : 0u;
}

void announce_launch(ukbb_fcn_handle *h, hipStream_t s) {
    ++h->n_launches;
    if (h->lds_poison_on && ukbb_fcn_debug_poison_lds(h->lds_poison_pat, s) == UKBB_OK) ++h->n_lds_poisons;
}

// One launch of `op` over images [n0, n0 + n) of the batch on stream s (the whole batch everywhere except inside a split range of run_plan).
int launch_op(ukbb_fcn_handle *h, const BoundOp &op, const PlanIo &io, int n0, int n, hipStream_t s, hipError_t &e) {
    const ukbb_fcn_arch &a = h->arch;
    const Params &P = h->par;
    static const HostLayer no_layer;
    const HostLayer &L = op.layer >= 0 ? h->layers[op.layer] : no_layer;
    const int bfio = h->plan.mode.bfio() ? 1 : 0;
    ConvConfig c;
    if (op.kind == OP_CONV || op.kind == OP_TCONV) find_cfg(op.cfg, c);
    auto actp = [&](int id) { return h->acts[id].image(n0); };
    auto sqg_args = [&](int j, int layer, int in, int out, int H, int W) {      // level j + 1 of the squeeze kernels; OP_SQG binds its one level at [0]
        SqgArgs sa{};
        sa.x = actp(in); sa.out = actp(out); sa.w_s = op.sq_w_s[j]; sa.b_s = op.sq_b_s[j]; sa.w_g = op.sq_w_g[j];
        sa.npix = (long long)n * H * W; sa.cin = h->layers[layer].cin; sa.x_bf16 = bfio; sa.hw = H * W;
        return sa;
    };
    e = hipSuccess;
    announce_launch(h, s);
    switch (op.kind) {
        case OP_FIRST: e = launch_first(FirstArgs{io.image, op.wpk, op.bias, actp(op.out), n, op.H, op.W, L.cout, bfio}, s); break;
        case OP_CONV:
        case OP_TCONV: {                                     // conv2d_transpose: a 2x2 conv onto the 4 * cout virtual channels of its sub-pixel phases, ReLU always
            const bool up = op.kind == OP_TCONV;
            ConvArgs ca{};
            ca.in0 = op.fused_first ? io.image : actp(op.in0);
            if (op.fused_first) { ca.first_w = P.conv0_w; ca.first_b = P.conv0_b; }
            ca.in1 = op.in1 >= 0 ? actp(op.in1) : nullptr;
            ca.C1 = op.in1 >= 0 ? (int)(h->acts[op.in1].per_image / ((size_t)op.H * op.W)) : 0;
            ca.C0 = L.cin - ca.C1;
            ca.wpk = op.wpk; ca.bias = op.bias; ca.out = actp(op.out);
            ca.N = n; ca.H = op.H; ca.W = op.W; ca.Ho = op.Ho; ca.Wo = op.Wo; ca.Cout = up ? 4 * L.cout : L.cout;
            if (!up && stores_bf16(c)) { ca.Cout = packed_cout(c, L.cout); ca.cout_store = L.cout; }
            if (op.fused_logits) {
                ca.lg_w = P.logits_w; ca.lg_b = P.logits_b;
                ca.lg_logits = io.logits; ca.lg_prob = io.prob; ca.lg_pred = io.pred; ca.lg_ncls = a.n_class;
            }
            ca.pad_y = op.pad_y; ca.pad_x = op.pad_x;
            ca.tiles_y = (op.Ho + c.th - 1) / c.th; ca.tiles_x = (op.Wo + c.tw - 1) / c.tw;
            ca.relu = up || L.relu ? 1 : 0; ca.up2 = up ? L.cout : 0;
            e = launch_conv(op.cfg, ca, s);
            break;
        }
        case OP_SQG: e = launch_sqg(sqg_args(0, op.layer, op.in0, op.out, op.H, op.W), s); break;
        case OP_SQG_MULTI: {
            SqgArgs sa[4];
            for (int j = 0; j < 4; ++j) {
                sa[j] = SqgArgs{};
                sa[j].cin = 32 << j;
                sa[j].x_bf16 = bfio;                         // one input format per launch
                if (op.mlayer[j] >= 0) sa[j] = sqg_args(j, op.mlayer[j], op.min_[j], op.mout[j], op.mh[j], op.mw[j]);   // else a launch of its own: npix = 0 -> no blocks
            }
            e = launch_sqg_multi(sa, s);
            break;
        }
        case OP_HEAD: {
            HeadArgs ha{};
            ha.conv0 = actp(op.in0);
            for (int l = 0; l < 4; ++l) ha.G[l] = actp(op.sq[l]);
            ha.w_s0 = P.head_w_s0; ha.b_s0 = P.head_b_s0; ha.w_o0 = P.head_w_o0; ha.b_o0 = P.head_b_o0; ha.w_o1 = P.head_w_o1; ha.b_o1 = P.head_b_o1;
            ha.w_o1x3 = P.head_w_o1x3; ha.w_o0x3 = P.head_w_o0x3; ha.w_lg = P.head_w_lg; ha.b_lg = P.logits_b;
            ha.logits = io.logits; ha.prob = io.prob; ha.pred = io.pred;
            ha.N = n; ha.H = op.H; ha.W = op.W; ha.n_class = a.n_class;
            ha.x3 = h->plan.mode.head_x3; ha.conv0_bf16 = bfio;
            ha.mm_bf16 = h->plan.mode.head_bf16; ha.w_s0bf = P.head_w_s0bf; ha.w_o0bf = P.head_w_o0bf; ha.w_o1bf = P.head_w_o1bf;
            e = launch_head(ha, s);
            break;
        }
        case OP_STEM: {
            StemArgs sa{};
            sa.image = io.image; sa.wA0 = P.stem_wA0; sa.wA1 = P.stem_wA1; sa.b0 = P.conv0_b; sa.b1 = P.conv0_1_b;
            sa.out = actp(op.out); sa.N = n; sa.H = op.H; sa.W = op.W;
            e = launch_unet_stem(sa, s);
            break;
        }
        case OP_TAIL: {
            TailArgs ta{};
            ta.in0 = actp(op.in0); ta.in1 = actp(op.in1);
            ta.wA0 = P.tail_wA0; ta.wA1 = P.tail_wA1; ta.b0 = P.up0_0_b; ta.b1 = P.up0_1_b; ta.lg_w = P.logits_w; ta.lg_b = P.logits_b;
            ta.logits = io.logits; ta.prob = io.prob; ta.pred = io.pred;
            ta.N = n; ta.H = op.H; ta.W = op.W; ta.ncls = a.n_class;
            e = launch_unet_tail(ta, s);
            break;
        }
        case OP_LOGITS: {
            LogitsArgs la{};
            la.in = actp(op.in0); la.w = P.logits_w; la.bias = P.logits_b;
            la.logits = io.logits; la.prob = io.prob; la.pred = io.pred;
            la.npix = (int64_t)n * op.H * op.W; la.C = L.cin; la.n_class = a.n_class; la.in_bf16 = bfio;
            e = launch_logits(la, s);
            break;
        }
        case OP_FIRST3D: {
            const Conv3dFirstArgs fa{io.image, h->t3d_map, P.conv0_w, op.bias, actp(op.out), n, a.fc, op.H, op.W};
            e = bfio ? launch_conv3d_first_bf16(fa, s) : launch_conv3d_first(fa, s);         // UKBB_PREC_BF16_3D: the same arithmetic, 16 bf16 channels stored
            break;
        }
        case OP_CONV3D:
        case OP_TCONV3D: {
            Conv3dArgs ca{};
            ca.in0 = actp(op.in0);
            ca.in1 = op.in1 >= 0 ? actp(op.in1) : nullptr;
            ca.C1 = op.in1 >= 0 ? h->acts[op.in1].ch : 0;
            ca.C0 = L.cin - ca.C1;
            ca.bias = op.bias; ca.out = actp(op.out);
            ca.N = n; ca.T = a.fc; ca.Hi = op.H; ca.Wi = op.W;
            ca.Ho = op.Ho; ca.Wo = op.Wo; ca.Cout = L.cout; ca.Cout_pad = round_up(L.cout, 32);
            ca.relu = L.relu ? 1 : 0;
            if (op.kind == OP_CONV3D) {
                ca.Hg = op.Ho; ca.Wg = op.Wo; ca.stride = op.stride; ca.up = 1;
                ca.oy = -op.pad_y; ca.ox = -op.pad_x; ca.jstep = 1;
                ca.nph = 1; ca.ph[0] = Conv3dPhase{op.wpk, 0, 0, 3, 3};
            } else {
                ca.Hg = op.H; ca.Wg = op.W; ca.stride = 1; ca.up = 2;
                ca.oy = 0; ca.ox = 0; ca.jstep = -1;
                ca.nph = 4;
                for (int ph = 0; ph < 4; ++ph) ca.ph[ph] = Conv3dPhase{op.wph[ph], ph >> 1, ph & 1, (ph >> 1) ? 1 : 2, (ph & 1) ? 1 : 2};
            }
            e = bfio ? launch_conv3d_bf16(ca, s) : launch_conv3d(ca, s);                     // UKBB_PREC_BF16_3D: bf16 maps and A fragments, same tiling
            break;
        }
        default:
            set_error("op kind %d not implemented", (int)op.kind);
            return UKBB_EARCH;
    }
    return UKBB_OK;
}

int run_plan(ukbb_fcn_handle *h, const float *image, int n, float *logits, float *prob, int32_t *pred,
             hipStream_t s) {
    if (h->timing) {
        int rc = collect_events(h);
        if (rc) return rc;
        if (h->ev.size() != 2 * h->ops.size()) {
            for (auto e : h->ev) (void)hipEventDestroy(e);
            h->ev.assign(2 * h->ops.size(), nullptr);
            for (auto &e : h->ev) HIP_TRY(hipEventCreate(&e), UKBB_EDEVICE);
        }
    }
    hipStream_t s_main = s;
    bool forked = false;
    const PlanIo io{image, logits, prob, pred};
    // UKBB_SPLIT_FROM (plan build): the ops of levels >= k -- conv{k}_0 .. up{k}_1, the launches whose fill / drain and serial chains
    // are the largest part of their time -- run as TWO half-batch chains on two streams, enqueued interleaved, joined before the next op
    const int sp0 = h->plan.split_first, sp1 = h->plan.split_last;
    // debugging aids (r06, tools/two_stream_bisect.py): run only the ops [first, last] of the plan (whatever they read was left by an earlier full forward)
    const int dbg_first = h->plan.debug_first_op, dbg_last = h->plan.debug_last_op;
    const bool fence_on = getenv("UKBB_DEBUG_FENCE_KERNEL") != nullptr;
    const bool sync_on = getenv("UKBB_DEBUG_SYNC_EVERY_OP") != nullptr;
    for (size_t i = 0; i < h->ops.size(); ++i) {
        const BoundOp &op = h->ops[i];
        s = s_main;
        if ((int)i < dbg_first || (int)i > dbg_last) continue;
        if ((int)i == sp0 && sp1 >= sp0 && n >= 8 && !h->timing) {      // per-kernel timing (set_timing) measures whole-batch launches
            if (!h->side2) {
                HIP_TRY(hipStreamCreateWithFlags(&h->side2, hipStreamNonBlocking), UKBB_EDEVICE);
                HIP_TRY(hipEventCreateWithFlags(&h->ev_split_fork, hipEventDisableTiming), UKBB_EDEVICE);
                HIP_TRY(hipEventCreateWithFlags(&h->ev_split_join, hipEventDisableTiming), UKBB_EDEVICE);
            }
            HIP_TRY(hipEventRecord(h->ev_split_fork, s_main), UKBB_EDEVICE);
            HIP_TRY(hipStreamWaitEvent(h->side2, h->ev_split_fork, 0), UKBB_EDEVICE);
            const int nA = (n + 1) / 2;
            for (int j = sp0; j <= sp1; ++j) {
                hipError_t e;
                int rc = launch_op(h, h->ops[j], io, 0, nA, s_main, e);
                if (rc) return rc;
                if (e == hipSuccess) rc = launch_op(h, h->ops[j], io, nA, n - nA, h->side2, e);
                if (rc) return rc;
                if (e != hipSuccess) { set_error("launch of %s (split) failed: %s", h->ops[j].name.c_str(), hipGetErrorString(e)); return UKBB_EDEVICE; }
            }
            HIP_TRY(hipEventRecord(h->ev_split_join, h->side2), UKBB_EDEVICE);
            HIP_TRY(hipStreamWaitEvent(s_main, h->ev_split_join, 0), UKBB_EDEVICE);
            i = (size_t)sp1;
            continue;
        }
        if (op.on_side) {                              // fork: side stream waits for everything issued so far
            if (!h->side) {
                HIP_TRY(hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking), UKBB_EDEVICE);
                h->ev_fork.assign(UKBB_FCN_MAX_LEVEL, nullptr);
                h->ev_join.assign(UKBB_FCN_MAX_LEVEL, nullptr);
                for (auto &e : h->ev_fork) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming), UKBB_EDEVICE);
                for (auto &e : h->ev_join) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming), UKBB_EDEVICE);
            }
            HIP_TRY(hipEventRecord(h->ev_fork[op.stride], s_main), UKBB_EDEVICE);
            HIP_TRY(hipStreamWaitEvent(h->side, h->ev_fork[op.stride], 0), UKBB_EDEVICE);
            s = h->side;
            forked = true;
        }
        if (op.kind == OP_HEAD && forked) {            // join: the head needs every side-stream result
            for (const Op &o2 : h->ops)
                if (o2.on_side) HIP_TRY(hipStreamWaitEvent(s_main, h->ev_join[o2.stride], 0), UKBB_EDEVICE);
        }
        const bool timed = h->timing && (h->timing_only < 0 || h->timing_only == (int)i);
        if (timed) HIP_TRY(hipEventRecord(h->ev[2 * i], s), UKBB_EDEVICE);
        hipError_t e = hipSuccess;
        {
            const int rc = launch_op(h, op, io, 0, n, s, e);
            if (rc) return rc;
        }
        if (e != hipSuccess) { set_error("launch of %s failed: %s", op.name.c_str(), hipGetErrorString(e)); return UKBB_EDEVICE; }
        if (fence_on) (void)ukbb_fcn_debug_fence_kernel(s);                  // debugging aid: an explicit system-scope fence launch behind every op
        if (sync_on) (void)hipStreamSynchronize(s);                           // debugging aid: the host waits for every op before it enqueues the next
        if (timed) HIP_TRY(hipEventRecord(h->ev[2 * i + 1], s), UKBB_EDEVICE);
        if (op.on_side) HIP_TRY(hipEventRecord(h->ev_join[op.stride], h->side), UKBB_EDEVICE);
    }
    if (h->timing) h->ev_pending = true;
    h->last_n = n;
    return UKBB_OK;
}

// every DevBuf of the handle by name: the handle's own ("io_prob", "lstm_hall", ...), the activation maps ("act<index>:<name>") and the
// device-side parameters ("dev:<layer>/<what>")
std::vector<std::pair<std::string, DevBuf *>> guard_bufs(ukbb_fcn_handle *h) {
    std::vector<std::pair<std::string, DevBuf *>> v;
    for (const HandleBuf &b : HANDLE_BUFS) v.emplace_back(b.name, &(h->*b.buf));
    for (size_t i = 0; i < h->acts.size(); ++i)
        v.emplace_back("act" + std::to_string(i) + (h->acts[i].name.empty() ? std::string() : ":" + h->acts[i].name), &h->acts[i].buf);
    for (auto &kv : h->dev) v.emplace_back("dev:" + kv.first, kv.second.get());
    return v;
}

// The scratch of the handle: its own buffers (rewritten_only: those of them a call rewrites before it reads them) and the activation maps.
std::vector<DevBuf *> scratch_bufs(ukbb_fcn_handle *h, bool rewritten_only = false) {
    std::vector<DevBuf *> v;
    for (const HandleBuf &b : HANDLE_BUFS) if (b.rewritten || !rewritten_only) v.push_back(&(h->*b.buf));
    for (ActMap &m : h->acts) v.push_back(&m.buf);
    return v;
}

int guard_checks(ukbb_fcn_handle *h, const char *what) {
    if (!h) { set_error("%s: NULL handle", what); return UKBB_EINVAL; }
    if (!h->guard.on) { set_error("%s: the handle was not created under UKBB_DEBUG_GUARD", what); return UKBB_EINVAL; }
    HIP_TRY(hipSetDevice(h->device), UKBB_EDEVICE);
    HIP_TRY(hipDeviceSynchronize(), UKBB_EDEVICE);
    return UKBB_OK;
}

}  // namespace

// =============================== C ABI ===========================================
extern "C" {

int ukbb_fcn_abi_version(void) { return UKBB_FCN_ABI_VERSION; }

// debugging aid, not in the public header (tools/two_stream_bisect.py): forwards launch only the ops [first, last] of the plan from now on
int ukbb_fcn_debug_set_ops(ukbb_fcn_handle *h, int first, int last) {
    if (!h) return UKBB_EINVAL;
    h->plan.debug_first_op = first; h->plan.debug_last_op = last;
    return UKBB_OK;
}

// ---- guarded, poisonable buffers (debugging aids, not in the public header; handles created under UKBB_DEBUG_GUARD only) ----------
// Waits for the device, then reads every guard back.  Returns the number of buffers with a damaged guard (or a negative code); one line
// per damaged guard goes to report (truncated at cap) and to ukbb_fcn_last_error: "<buffer> <front|back> <first> <last>", the first and
// last damaged byte as offsets from the payload's start (front guard: negative; back guard: >= the payload's bytes).
int ukbb_fcn_debug_check_guards(ukbb_fcn_handle *h, char *report, size_t cap) {
    int rc = guard_checks(h, "debug_check_guards");
    if (rc) return rc;
    const auto bufs = guard_bufs(h);
    std::vector<unsigned char> host(GUARD_BYTES);
    std::string out;
    int bad = 0;
    for (auto &kv : bufs) {
        const DevBuf *b = kv.second;
        if (!b->p) continue;
        const long long bytes = (long long)(b->n * sizeof(float));
        bool hit = false;
        for (int side = 0; side < 2; ++side) {
            const long long off = side ? bytes : -(long long)GUARD_BYTES;
            HIP_TRY(hipMemcpy(host.data(), reinterpret_cast<const char *>(b->p) + off, GUARD_BYTES, hipMemcpyDeviceToHost), UKBB_EDEVICE);
            long long first = -1, last = -1;
            for (size_t i = 0; i < GUARD_BYTES; ++i)
                if (host[i] != GUARD_BYTE) { if (first < 0) first = (long long)i; last = (long long)i; }
            if (first < 0) continue;
            char line[256];
            snprintf(line, sizeof line, "%s %s %lld %lld\n", kv.first.c_str(), side ? "back" : "front", off + first, off + last);
            out += line;
            hit = true;
        }
        bad += hit;
    }
    if (report && cap) { const size_t m = std::min(out.size(), cap - 1); memcpy(report, out.data(), m); report[m] = 0; }
    set_error("%s", out.c_str());
    return bad;
}

// The number of guarded buffers the handle holds right now; their payload bytes and the bytes of their guards.
int ukbb_fcn_debug_guard_info(ukbb_fcn_handle *h, uint64_t *payload_bytes, uint64_t *guard_bytes) {
    if (!h) { set_error("debug_guard_info: NULL handle"); return UKBB_EINVAL; }
    const auto bufs = guard_bufs(h);
    int nb = 0;
    uint64_t pay = 0;
    for (auto &kv : bufs)
        if (kv.second->p && kv.second->guarded()) { ++nb; pay += kv.second->n * sizeof(float); }
    if (payload_bytes) *payload_bytes = pay;
    if (guard_bytes) *guard_bytes = (uint64_t)nb * 2 * GUARD_BYTES;
    return nb;
}

// Refills the payloads of the buffers a call rewrites before it reads them -- the activation maps, the ConvLSTM and cine working buffers
// and the host-call staging of the outputs -- with `pattern`.  Weights, the staged input (io_image) and the tables uploaded once per
// shape (lstm_aux, t3d_aux) keep their contents.  Returns the number of buffers refilled.
int ukbb_fcn_debug_poison(ukbb_fcn_handle *h, uint32_t pattern) {
    int rc = guard_checks(h, "debug_poison");
    if (rc) return rc;
    int nb = 0;
    for (DevBuf *b : scratch_bufs(h, true)) {
        if (!b->p) continue;
        HIP_TRY(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(b->p), (int)pattern, b->n), UKBB_EDEVICE);
        ++nb;
    }
    HIP_TRY(hipDeviceSynchronize(), UKBB_EDEVICE);
    return nb;
}

// Launches the handle has made since it was created (out[0]: the plan's ops, a split op counting twice; the ConvLSTM x pass and time steps;
// lstm_out, lstm_tile, t3d_tile) and the LDS poison launches issued in front of them under UKBB_DEBUG_POISON_LDS (out[1]): a call that
// ran with the variable set advances both by the same number.
int ukbb_fcn_debug_launch_counts(ukbb_fcn_handle *h, uint64_t out[2]) {
    if (!h || !out) { set_error("debug_launch_counts: NULL argument"); return UKBB_EINVAL; }
    out[0] = h->n_launches; out[1] = h->n_lds_poisons;
    return UKBB_OK;
}

// Writes one byte that differs from the guard's into a guard of `buffer` (a name as debug_check_guards reports it), `offset` bytes from the
// payload's start: inside the front guard (-GUARD_BYTES .. -1) or the back guard (payload bytes .. + GUARD_BYTES - 1), i.e. inside the
// buffer's own allocation.  So that a test can show the checker sees damage.
int ukbb_fcn_debug_damage_guard(ukbb_fcn_handle *h, const char *buffer, long long offset) {
    int rc = guard_checks(h, "debug_damage_guard");
    if (rc) return rc;
    if (!buffer) { set_error("debug_damage_guard: NULL buffer name"); return UKBB_EINVAL; }
    const auto bufs = guard_bufs(h);
    for (auto &kv : bufs) {
        if (kv.first != buffer) continue;
        const DevBuf *b = kv.second;
        const long long bytes = (long long)(b->n * sizeof(float)), G = (long long)GUARD_BYTES;
        if (!b->p) { set_error("debug_damage_guard: buffer '%s' is not allocated", buffer); return UKBB_EINVAL; }
        if (!((offset >= -G && offset < 0) || (offset >= bytes && offset < bytes + G))) {
            set_error("debug_damage_guard: offset %lld is in no guard of '%s' (payload %lld bytes, guards %lld)", offset, buffer, bytes, G);
            return UKBB_EINVAL;
        }
        const unsigned char v = (unsigned char)~GUARD_BYTE;
        HIP_TRY(hipMemcpy(reinterpret_cast<char *>(b->p) + offset, &v, 1, hipMemcpyHostToDevice), UKBB_EDEVICE);
        return UKBB_OK;
    }
    set_error("debug_damage_guard: no buffer named '%s'", buffer);
    return UKBB_EINVAL;
}

// ukbb_fcn_set_f32x3_convs on any kind but the FCN: the error text set, true
static bool refuse_f32x3_convs(int kind) {
    if (kind == UKBB_KIND_FCN) return false;
    set_error("set_f32x3_convs: the three-piece convolutions are built for the FCN models only (the U-Net kinds have no f32x3 conv kernels)");
    return true;
}

// debugging / testing aid, not in the public header: the plan layout_plan makes for batches of n images of H x W on a device of `cus`
// compute units, as text -- host arithmetic only, no device needed.  One line per op, one per activation map, then the plan's fields.
// Returns the text's length (it is truncated when cap is smaller), or the negative code create / set_precision / reserve would give.
static int debug_plan_text(const ukbb_fcn_arch *arch, int precision, bool f32x3_convs, int n, int H, int W, int cus, char *buf, size_t cap) {
    static const char *const kinds[] = {"first", "conv", "head", "tconv", "logits", "sqg", "sqg_multi", "tail", "stem", "first3d", "conv3d", "tconv3d"};
    if (!arch || (!buf && cap) || cus < 1) { set_error("debug_plan_layout: bad argument"); return UKBB_EINVAL; }
    PlanLayout L;
    const char *why;
    if (plan_mode(*arch, precision, L.mode, &why) == UKBB_EINVAL) { set_error("debug_plan_layout: bad precision"); return UKBB_EINVAL; }
    int rc = check_shape(n, H, W);
    if (rc) return rc;
    rc = layout_plan(*arch, precision, H, W, n, cus, L, f32x3_convs);      // refuses the (kind, precision) pairs plan_mode refuses
    if (rc) return rc;
    std::string out;
    char line[512];
    for (size_t i = 0; i < L.ops.size(); ++i) {
        const Op &op = L.ops[i];
        snprintf(line, sizeof line, "op %zu %s %s %d %d %d %d %d %d %d %d %d %.17g %.17g %.17g\n", i, op.name.c_str(), kinds[op.kind], op.cfg, op.H, op.W, op.Ho, op.Wo,
                 op.stride, op.in0, op.in1, op.out, op.macs_per_image, op.mfma_macs_per_image, op.padded_macs_per_image);
        out += line;
    }
    for (const ActSpec &s : L.acts) {
        snprintf(line, sizeof line, "act %s %zu %d %zu\n", s.name.empty() ? "-" : s.name.c_str(), s.per_image, s.channels, act_alloc_esz(*arch, s));
        out += line;
    }
    snprintf(line, sizeof line, "plan split %d %d bfio %d feat_buf %d lstm %d %d %d %d head_bf16 %d\n", L.split_first, L.split_last, (int)L.mode.bfio(), L.feat_buf,
             (int)L.needs_lstm, L.lstm_tile_cols, (int)L.lstm_bf_wino, (int)L.lstm_bf_hoist, (int)L.mode.head_bf16);
    out += line;
    if (L.mode.conv_x3) out.replace(out.size() - 1, 1, " conv_x3 1\n");      // only a plan that has it says so: every other text is unchanged
    if (cap) { const size_t m = std::min(out.size(), cap - 1); memcpy(buf, out.data(), m); buf[m] = 0; }
    return (int)out.size();
}
int ukbb_fcn_debug_plan_layout(const ukbb_fcn_arch *arch, int precision, int n, int H, int W, int cus, char *buf, size_t cap) {
    return debug_plan_text(arch, precision, false, n, H, W, cus, buf, cap);
}
// ... with the handle's ukbb_fcn_set_f32x3_convs setting as an argument (it takes effect under UKBB_PREC_F32X3 on an FCN architecture only)
int ukbb_fcn_debug_plan_layout_x3(const ukbb_fcn_arch *arch, int precision, int f32x3_convs, int n, int H, int W, int cus, char *buf, size_t cap) {
    if (arch && f32x3_convs && refuse_f32x3_convs(arch->kind)) return UKBB_EARCH;      // as ukbb_fcn_set_f32x3_convs on a handle of that kind
    return debug_plan_text(arch, precision, f32x3_convs != 0, n, H, W, cus, buf, cap);
}

// debugging / testing aid, not in the public header: pack_head_bf16 (pack.cpp) on a host matrix, host arithmetic only.  dst takes
// (n_out / 32) * (k_in / 16) * 256 dwords.
int ukbb_fcn_debug_pack_head_bf16(const float *w, int k_in, int n_out, int acc_k, uint32_t *dst) {
    if (!w || !dst || (k_in != 16 && k_in != 32 && k_in != 64) || (n_out != 32 && n_out != 64) || (acc_k && k_in < 32)) { set_error("debug_pack_head_bf16: bad argument"); return UKBB_EINVAL; }
    pack_head_bf16(w, k_in, n_out, acc_k, reinterpret_cast<float *>(dst));
    return UKBB_OK;
}

const char *ukbb_fcn_last_error(void) { return g_err.c_str(); }

size_t ukbb_fcn_weight_count(const ukbb_fcn_arch *arch) {
    if (!arch) return 0;
    std::vector<Spec> specs;
    if (!arch_specs(*arch, specs)) return 0;
    size_t n = 0;
    for (auto &s : specs) n += spec_floats(s);
    return n;
}

ukbb_fcn_handle *ukbb_fcn_create(const ukbb_fcn_arch *arch, const float *weights, size_t n_floats, int device) {
    if (!arch || !weights) { set_error("create: NULL argument"); return nullptr; }
    std::vector<Spec> specs;
    if (!arch_specs(*arch, specs)) { set_error("create: malformed architecture descriptor"); return nullptr; }
    std::string why;
    if (!supported(*arch, why)) { set_error("create: unsupported architecture: %s", why.c_str()); return nullptr; }
    size_t want = 0;
    for (auto &s : specs) want += spec_floats(s);
    if (want != n_floats) { set_error("create: expected %zu weight floats, got %zu", want, n_floats); return nullptr; }

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        set_error("create: no HIP device visible (this library has no CPU fallback)");
        return nullptr;
    }
    if (device < 0 || device >= ndev) { set_error("create: device %d out of range (0..%d)", device, ndev - 1); return nullptr; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) { set_error("create: hipGetDeviceProperties failed"); return nullptr; }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("create: device %d is %s; kernels are built for gfx950 (MI355X) only", device, prop.gcnArchName);
        return nullptr;
    }
    if (hipSetDevice(device) != hipSuccess) { set_error("create: hipSetDevice failed"); return nullptr; }

    std::unique_ptr<ukbb_fcn_handle> h(new ukbb_fcn_handle);
    h->arch = *arch;
    h->device = device;
    if (const char *g = getenv("UKBB_DEBUG_GUARD")) {   // debugging aid, read here only: guarded, poisoned buffers for this handle
        h->guard.on = true;
        h->guard.pattern = (uint32_t)strtoul(g, nullptr, 16);
    }

    // ---- fold BN (fp32; same op order as weights.py fold_bn) --------------------------
    const float *p = weights;
    for (auto &s : specs) {
        HostLayer L;
        L.name = s.name; L.ks = s.ks; L.kd = s.kd; L.cin = s.cin; L.cout = s.cout; L.transposed = s.transposed;
        L.relu = s.bn;
        const size_t nk = (size_t)s.kd * s.ks * s.ks * s.cin * s.cout;
        const float *k = p; p += nk;
        std::vector<float> scale(s.cout, 1.f);
        L.b.assign(s.cout, 0.f);
        if (s.bn) {
            const float *gamma = p, *beta = p + s.cout, *mean = p + 2 * s.cout, *var = p + 3 * s.cout;
            p += 4 * (size_t)s.cout;
            for (int c = 0; c < s.cout; ++c) {
                const volatile float sc = gamma[c] / sqrtf(var[c] + BN_EPS);
                const volatile float ms = mean[c] * sc;            // volatile: no fma contraction
                scale[c] = sc;
                L.b[c] = beta[c] - ms;
            }
        }
        if (s.bias) { for (int c = 0; c < s.cout; ++c) L.b[c] = p[c]; p += s.cout; }
        L.w.resize(nk);
        if (!s.transposed) {
            for (size_t i = 0; i < nk; ++i) L.w[i] = k[i] * scale[i % s.cout];
        } else {
            // TF transposed filter [kd][kh][kw][Cout][Cin] -> [kd][kh][kw][Cin][Cout]
            for (int t = 0; t < s.kd * s.ks * s.ks; ++t)
                for (int co = 0; co < s.cout; ++co)
                    for (int ci = 0; ci < s.cin; ++ci)
                        L.w[((size_t)t * s.cin + ci) * s.cout + co] = k[((size_t)t * s.cout + co) * s.cin + ci] * scale[co];
        }
        h->layer_index[L.name] = (int)h->layers.size();
        h->layers.push_back(std::move(L));
    }

    // ---- upload biases and the non-MFMA weights ------------------------------------------
    for (auto &L : h->layers)
        if (upload(h.get(), L.name + "/bias", L.b)) return nullptr;
    {
        const HostLayer &L0 = h->layers[h->layer_index.at("conv0_0")];
        if (upload(h.get(), "conv0_0/w", L0.w)) return nullptr;      // [9][16]
    }
    if (arch->kind == UKBB_KIND_UNET_LSTM) {
        const HostLayer &lo = h->layers[h->layer_index.at("lstm_out")];   // [2*NH][n_class]
        if (upload(h.get(), "lstm_out/w", lo.w)) return nullptr;
    }
    if (arch->kind == UKBB_KIND_FCN) {
        const HostLayer &s0 = h->layers[h->layer_index.at("same_dim0")];
        const HostLayer &o0 = h->layers[h->layer_index.at("out0")];
        const HostLayer &o1 = h->layers[h->layer_index.at("out1")];
        const HostLayer &lg = h->layers[h->layer_index.at("logits")];
        std::vector<float> v;
        v.assign(16 * 32, 0.f);                 pack_sq(s0.w.data(), 16, v.data());
        if (upload(h.get(), "head/w_s0", v)) return nullptr;
        v.assign(2 * 4 * 64 * 4, 0.f);          pack_rowmap_32x64(o0.w.data(), 64, v.data());
        if (upload(h.get(), "head/w_o0", v)) return nullptr;
        v.assign(2 * 2 * 4 * 64 * 4, 0.f);
        pack_rowmap_32x64(o1.w.data(), 64, v.data());
        pack_rowmap_32x64(o1.w.data() + 32 * 64, 64, v.data() + 2 * 4 * 64 * 4);
        if (upload(h.get(), "head/w_o1", v)) return nullptr;
        v.assign(3 * 2 * 4 * 64 * 4, 0.f);      pack_head_x3(o1.w.data(), 64, v.data());
        if (upload(h.get(), "head/w_o1x3", v)) return nullptr;
        v.assign(3 * 2 * 2 * 64 * 4, 0.f);      pack_head_x3(o0.w.data(), 32, v.data());
        if (upload(h.get(), "head/w_o0x3", v)) return nullptr;
        v.assign(2 * arch->n_class * 32, 0.f);  pack_head_lg(lg.w.data(), arch->n_class, v.data());
        if (upload(h.get(), "head/w_lg", v)) return nullptr;
        for (int l = 1; l < arch->n_level; ++l) {
            const HostLayer &sl = h->layers[h->layer_index.at("same_dim" + std::to_string(l))];
            v.assign((size_t)sl.cin * 32, 0.f);  pack_sq(sl.w.data(), sl.cin, v.data());
            if (upload(h.get(), "sqg" + std::to_string(l) + "/w_s", v)) return nullptr;
            v.assign(2 * 4 * 64 * 4, 0.f);       pack_rowmap_32x64(o0.w.data() + (size_t)32 * l * 64, 64, v.data());
            if (upload(h.get(), "sqg" + std::to_string(l) + "/w_g", v)) return nullptr;
        }
        // UKBB_PREC_BF16_FULL: the head's three matrices as one bf16 piece each (behind every record that existed before the mode)
        v.assign(1 * 1 * 64 * 4, 0.f);          pack_head_bf16(s0.w.data(), 16, 32, 0, v.data());
        if (upload(h.get(), "head/w_s0bf", v)) return nullptr;
        v.assign(2 * 2 * 64 * 4, 0.f);          pack_head_bf16(o0.w.data(), 32, 64, 1, v.data());
        if (upload(h.get(), "head/w_o0bf", v)) return nullptr;
        v.assign(2 * 4 * 64 * 4, 0.f);          pack_head_bf16(o1.w.data(), 64, 64, 1, v.data());
        if (upload(h.get(), "head/w_o1bf", v)) return nullptr;
    } else if (arch->kind == UKBB_KIND_UNET || arch->kind == UKBB_KIND_TEMPORAL_UNET) {
        const HostLayer &lg = h->layers[h->layer_index.at("logits")];
        if (upload(h.get(), "logits/w", lg.w)) return nullptr;
    }
    return h.release();
}

void ukbb_fcn_destroy(ukbb_fcn_handle *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    delete h;
}

int ukbb_fcn_reserve(ukbb_fcn_handle *h, int n, int height, int width) {
    if (!h) { set_error("reserve: NULL handle"); return UKBB_EINVAL; }
    return prepare(h, n, height, width);
}

int ukbb_fcn_forward(ukbb_fcn_handle *h, const float *image, int n, int height, int width,
                     float *logits, float *prob, int32_t *pred, void *stream) {
    if (!h || !image) { set_error("forward: NULL argument"); return UKBB_EINVAL; }
    lds_poison_begin(h);
    int rc = refuse_sequence_kinds(h, "forward");
    if (!rc) rc = prepare(h, n, height, width);
    if (rc) return rc;
    return run_plan(h, image, n, logits, prob, pred, static_cast<hipStream_t>(stream));
}

int ukbb_fcn_forward_host(ukbb_fcn_handle *h, const float *image, int n, int height, int width,
                          float *logits, float *prob, int32_t *pred) {
    if (!h || !image) { set_error("forward_host: NULL argument"); return UKBB_EINVAL; }
    lds_poison_begin(h);
    int rc = refuse_sequence_kinds(h, "forward_host");
    if (!rc) rc = prepare(h, n, height, width);
    if (rc) return rc;
    const size_t npix = (size_t)n * height * width, ncls = h->arch.n_class;
    const struct { void *host; DevBuf &dev; size_t n; } outs[3] = {{logits, h->io_logits, npix * ncls}, {prob, h->io_prob, npix * ncls}, {pred, h->io_pred, npix}};
    HIP_TRY(h->io_image.ensure(npix), UKBB_ENOMEM);
    for (auto &o : outs) if (o.host) HIP_TRY(o.dev.ensure(o.n), UKBB_ENOMEM);
    HIP_TRY(hipMemcpyAsync(h->io_image.p, image, npix * sizeof(float), hipMemcpyHostToDevice, nullptr), UKBB_EDEVICE);
    rc = run_plan(h, h->io_image.p, n, logits ? h->io_logits.p : nullptr, prob ? h->io_prob.p : nullptr,
                  pred ? reinterpret_cast<int32_t *>(h->io_pred.p) : nullptr, nullptr);
    if (rc) return rc;
    for (auto &o : outs) if (o.host) HIP_TRY(hipMemcpyAsync(o.host, o.dev.p, o.n * sizeof(float), hipMemcpyDeviceToHost, nullptr), UKBB_EDEVICE);
    HIP_TRY(hipStreamSynchronize(nullptr), UKBB_EDEVICE);
    return UKBB_OK;
}

// ---- forward_cine scratch planner: the host-only queries (the arithmetic is plan.cpp's) ---------------------------------------
namespace {

// The units of a FRESH handle's plan for cines of F frames on an MI355X (256 compute units), without a device: the layout the engine
// itself would build, so the A/B knobs that add or drop a map count here as they do there.  false: a request forward_cine would refuse.
bool cine_query_units(const ukbb_fcn_arch *arch, int precision, int F, int H, int W, int time_step, CineUnits &u) {
    if (!arch || !ukbb_fcn_weight_count(arch)) return false;
    if (arch->kind != UKBB_KIND_UNET_LSTM && arch->kind != UKBB_KIND_TEMPORAL_UNET) return false;
    if (precision != UKBB_PREC_FP32 && precision != UKBB_PREC_BF16 && precision != UKBB_PREC_BF16_3D) return false;
    PlanLayout L;
    const char *why;
    if (plan_mode(*arch, precision, L.mode, &why) || !cine_request_ok(arch->fc, F, H, W, time_step)) return false;
    if (layout_plan(*arch, precision, H, W, F, 256, L)) return false;
    u = cine_units_from(L, *arch, H, W);
    return true;
}

// frees every activation and cine buffer (the plan stays); nothing of the handle may be in flight afterwards
int release_scratch(ukbb_fcn_handle *h) {
    HIP_TRY(hipSetDevice(h->device), UKBB_EDEVICE);
    HIP_TRY(hipDeviceSynchronize(), UKBB_EDEVICE);
    for (DevBuf *b : scratch_bufs(h)) b->release();
    h->cap_n = 0;
    h->lstm_aux_key = h->t3d_aux_key = h->budget_key = -1;
    return UKBB_OK;
}

// Under a budget the buffers hold exactly what the chunk plan of the LAST call needs: a call with another shape or plan releases them
// first (buffers only grow otherwise, and two shapes' maxima together could exceed the budget).
int budget_enter(ukbb_fcn_handle *h, int F, int H, int W, int time_step, const CinePlan &pl) {
    if (!h->scratch_budget) return UKBB_OK;
    const long long key = ((((((long long)F * 4099 + H) * 4099 + W) * 4099 + time_step) * 4099 + pl.Wc) * 8 + h->precision) ^ (long long)(h->scratch_budget * 0x9E3779B97F4A7C15ull >> 1);
    if (h->budget_key == key) return UKBB_OK;
    int rc = release_scratch(h);
    if (rc) return rc;
    h->budget_key = key;
    return UKBB_OK;
}

}  // namespace

uint64_t ukbb_fcn_cine_scratch_bytes(const ukbb_fcn_arch *arch, int precision, int n_frames, int height, int width, int time_step, uint64_t budget) {
    CineUnits u;
    CinePlan pl;
    if (!cine_query_units(arch, precision, n_frames, height, width, time_step, u)) return 0;
    return plan_cine(u, n_frames, time_step, budget, pl) ? pl.bytes : 0;
}

uint64_t ukbb_fcn_cine_min_scratch_bytes(const ukbb_fcn_arch *arch, int precision, int n_frames, int height, int width, int time_step) {
    CineUnits u;
    CinePlan pl;
    if (!cine_query_units(arch, precision, n_frames, height, width, time_step, u)) return 0;
    plan_cine(u, n_frames, time_step, 0, pl);
    return pl.min_bytes;
}

int ukbb_fcn_cine_chunk_windows(const ukbb_fcn_arch *arch, int precision, int n_frames, int height, int width, int time_step, uint64_t budget) {
    CineUnits u;
    CinePlan pl;
    if (!cine_query_units(arch, precision, n_frames, height, width, time_step, u)) return 0;
    return plan_cine(u, n_frames, time_step, budget, pl) ? pl.Wc : 0;
}

int ukbb_fcn_set_scratch_budget(ukbb_fcn_handle *h, uint64_t bytes) {
    if (!h) { set_error("set_scratch_budget: NULL handle"); return UKBB_EINVAL; }
    if (h->arch.kind != UKBB_KIND_UNET_LSTM && h->arch.kind != UKBB_KIND_TEMPORAL_UNET) return UKBB_OK;      // no cine scratch: accepted, ignored
    if (bytes == h->scratch_budget) return UKBB_OK;
    h->scratch_budget = bytes;
    return bytes ? release_scratch(h) : UKBB_OK;      // a new budget starts from empty buffers, so that what the handle holds is what the plan predicts
}

uint64_t ukbb_fcn_scratch_bytes(const ukbb_fcn_handle *h) {
    if (!h) return 0;
    uint64_t n = 0;
    for (DevBuf *b : scratch_bufs(const_cast<ukbb_fcn_handle *>(h))) n += b->n;
    return n * sizeof(float);
}

// ---- UNet-LSTM --------------------------------------------------------------------------------------
namespace {

// BiConvLSTM over Wn windows of T steps on NF cached feature frames.  d_map[k*Wn + w] = feature frame of step k of window w.
//   x pass (one launch, both directions): per frame gx = W_x * x + b, and the cell's first step from the zero state (:278,:290) c1, h1;
//   then per direction T - 1 launches of the fused gate-conv (hidden channels only) + cell kernel, every step's hidden map kept
//   ([dir][k][Wn][HW][16]) for the output conv over concat([h_fw, h_bw]) (:305-312), which the caller runs (lstm_out / lstm_tile).
int run_bilstm(ukbb_fcn_handle *h, const float *feat, int NF, const int *d_map, int Wn, int H, int W, hipStream_t s) {
    const ukbb_fcn_arch &a = h->arch;
    const int T = a.fc, NHID = a.same_dim, tc = h->plan.lstm_tile_cols;
    const size_t HW = (size_t)H * W;
    // bf16 plan: the direct-conv bf16 form (kernels_ws.hip) unless UKBB_LSTM_BF16_WINOGRAD=1 asks for the fp32 Winograd arithmetic on bf16 storage (A/B)
    const bool wsf = h->plan.mode.bfio() && !h->plan.lstm_bf_wino;
    // r06 experiment (UKBB_LSTM_BF16_UNHOIST=1): the direct-conv bf16 steps read the feature frame (32 bytes per pixel) and multiply it again
    // instead of reading gx (128 bytes per pixel); no gx buffer exists in that form.  Slower by 5 % per step (plan.cpp, read_knobs), so not the default.
    const bool unhoist = wsf && !h->plan.lstm_bf_hoist;
    const size_t gxf = wsf ? lstm_ws_gx_elems(H, W) : wino24_lstm_gx_floats(H, W, tc), cf = wsf ? lstm_ws_c_floats(H, W) : wino24_lstm_c_floats(H, W, tc);
    const bool bf = h->plan.mode.bfio();                        // bf16 plan: features, gx and hidden maps are bf16 in HBM
    const size_t esz = bf ? 2 : 4;
    // Scratch of one cine (include/ukbb_fcn.h, forward_cine): gx 2 NF gxf + h1 2 NF HW NHID + hall 2 T Wn HW NHID elements of esz bytes,
    // cell state (2 NF + Wn) cf floats.  DevBuf counts 4-byte units: the bf16 maps take half as many.
    if (!unhoist) HIP_TRY(h->lstm_gx.ensure_bytes(2 * (size_t)NF * gxf * esz), UKBB_ENOMEM);
    HIP_TRY(h->lstm_c1.ensure(2 * (size_t)NF * cf), UKBB_ENOMEM);
    HIP_TRY(h->lstm_h1.ensure_bytes(2 * (size_t)NF * HW * NHID * esz), UKBB_ENOMEM);
    HIP_TRY(h->lstm_c.ensure((size_t)Wn * cf), UKBB_ENOMEM);
    HIP_TRY(h->lstm_hall.ensure_bytes(2 * (size_t)T * Wn * HW * NHID * esz), UKBB_ENOMEM);
    const Params &P = h->par;
    ConvArgs base{};
    base.ls_bf16 = bf ? 1 : 0;
    base.C0 = a.n_filter[0]; base.C1 = 0;
    base.H = H; base.W = W; base.Ho = H; base.Wo = W;
    base.pad_y = 1; base.pad_x = 1; base.relu = 0;
    base.tiles_y = (H + 7) / 8; base.tiles_x = (W + tc - 1) / tc;
    base.ls_forget_bias = 1.0f;
    { const char *dg = getenv("UKBB_LSTM_DIAG"); base.diag = dg ? atoi(dg) : 0; }      // honoured by diagnostic builds (-DUKBB_DIAG) only
    {   // x pass
        ConvArgs ca = base;
        ca.in0 = feat; ca.N = NF; ca.Cout = 2 * 4 * NHID;
        ca.wpk = P.lstm[wsf].wx; ca.bias = P.lstm[wsf].bx;
        ca.ls_mode = 1; ca.ls_gx = unhoist ? nullptr : h->lstm_gx.p; ca.ls_c_out = h->lstm_c1.p; ca.out = h->lstm_h1.p;
        ca.ls_gx_dir = (long long)NF * gxf; ca.ls_c_dir = (long long)NF * cf; ca.ls_h_dir = (long long)NF * HW * NHID;
        announce_launch(h, s);
        hipError_t e = wsf ? launch_lstm_ws(ca, s) : launch_wino24_lstm(ca, tc, s);
        if (e != hipSuccess) { set_error("ConvLSTM x-pass launch failed: %s", hipGetErrorString(e)); return UKBB_EDEVICE; }
    }
    const size_t kst = (size_t)Wn * HW * NHID;           // one step's hidden maps
    // A zero backward cell (the single-direction head served through the bidirectional layer set): from the zero state i = o = 1/2, j = tanh(0) = 0,
    // so c and h stay exactly 0 at every step -- the x pass above already produced zeros for its first step; the other T - 1 maps are cleared, not computed.
    const int ndir = h->lstm_bw_zero ? 1 : 2;
    if (h->lstm_bw_zero) HIP_TRY(hipMemsetAsync(at(h->lstm_hall.p, (size_t)T * kst, esz), 0, (size_t)T * kst * esz, s), UKBB_EDEVICE);
    for (int dir = 0; dir < ndir; ++dir) {
        float *const hall = at(h->lstm_hall.p, (size_t)dir * T * kst, esz);
        for (int step = 1; step < T; ++step) {
            const int k = dir ? T - 1 - step : step, kprev = dir ? k + 1 : k - 1;
            ConvArgs ca = base;
            ca.N = Wn; ca.Cout = 4 * NHID;
            ca.wpk = P.lstm[wsf].wh[dir]; ca.bias = nullptr;
            ca.ls_mode = 2;
            ca.ls_gx = unhoist ? nullptr : at(h->lstm_gx.p, (size_t)dir * NF * gxf, esz); ca.ls_gx_map = d_map + (size_t)k * Wn;
            const float *hprev; const int *hmap;
            if (step == 1) {                                // previous state = the x pass's per-frame first step
                hprev = at(h->lstm_h1.p, (size_t)dir * NF * HW * NHID, esz); hmap = d_map + (size_t)kprev * Wn;
                ca.ls_c_in = h->lstm_c1.p + (size_t)dir * NF * cf;
            } else {
                hprev = at(hall, (size_t)kprev * kst, esz); hmap = nullptr;
                ca.ls_c_in = h->lstm_c.p;
            }
            ca.in0 = hprev; ca.in0_map = hmap;
            if (unhoist) {                                  // ls_mode 3: source 0 = the step's feature frames (through ls_gx_map), source 1 = the previous hidden maps (through in0_map)
                ca.ls_mode = 3;
                ca.in0 = feat; ca.in1 = hprev; ca.C1 = NHID;
                ca.wpk = P.lstm_wxh[dir];
                ca.bias = P.lstm[1].bx + dir * 64;
            }
            ca.ls_c_out = h->lstm_c.p;
            ca.out = at(hall, (size_t)k * kst, esz);
            announce_launch(h, s);
            hipError_t e = wsf ? launch_lstm_ws(ca, s) : launch_wino24_lstm(ca, tc, s);
            if (e != hipSuccess) { set_error("ConvLSTM step launch failed: %s", hipGetErrorString(e)); return UKBB_EDEVICE; }
        }
    }
    return UKBB_OK;
}

// host-side tables of the windowed deploy loop (deploy_network_ao.py:129-183) for F frames, windows of T = 2 * weight_R - 1 frames
// centred on range(0, F, time_step): map[k * Wn + w] = frame of position k of window w (circular, :147-158), wk = the window
// weights (:134-144), order[f * T ..] = the (w * T + k) terms frame f receives in the reference's order (-1 ends), wsum[f] their weights
void cine_tables(int F, int T, int time_step, int weight_R, double weight_r, std::vector<int> &map, std::vector<int> &order,
                 std::vector<double> &wk, std::vector<double> &wsum) {
    const int rad = (T - 1) / 2, Wn = (F + time_step - 1) / time_step;
    map.assign((size_t)T * Wn, 0); order.assign((size_t)F * T, -1);
    wk.assign(T, 0.0); wsum.assign(F, 0.0);
    for (int k = 0; k < T; ++k) {
        const int d = k > rad ? k - rad : rad - k;
        wk[k] = d <= weight_R ? pow(1.0 - (double)d / weight_R, weight_r) : 0.0;
        for (int w = 0; w < Wn; ++w) {
            int i = w * time_step - rad + k;
            if (i < 0) i += F; else if (i >= F) i -= F;
            map[(size_t)k * Wn + w] = i;
        }
    }
    // `prob[..., idx] += p * w` with fancy indexing (:179-180) is prob[idx] = prob[idx] + p*w: when a frame occurs
    // more than once in a window's idx (only if F < T) the LAST occurrence wins instead of accumulating
    // (SURVEY.md App. C.7); same for `weight[..., idx] += w`.  So per window a frame receives at most one term.
    std::vector<int> cnt(F, 0), last(F);
    for (int w = 0; w < Wn; ++w) {                                          // the reference's loop over window centres
        std::fill(last.begin(), last.end(), -1);
        for (int k = 0; k < T; ++k) last[map[(size_t)k * Wn + w]] = k;
        for (int k = 0; k < T; ++k) {                                       // frames in idx order; the order across frames is irrelevant
            const int f = map[(size_t)k * Wn + w];
            if (last[f] != k) continue;
            order[(size_t)f * T + cnt[f]++] = w * T + k;
            wsum[f] += wk[k];
        }
    }
}

// The device copy of those tables: map | order | wk | wsum laid into ONE aux buffer of the handle (8-byte aligned pieces), keyed by what
// they were built from and uploaded, blocking, on the first call for that key.  `map` is the window -> frame table in the caller's layout.
struct CineAux { const int *map; CineTable tb; };
int cine_aux(DevBuf &buf, long long &have, long long key, const std::vector<int> &map, const std::vector<int> &order,
             const std::vector<double> &wk, const std::vector<double> &wsum, hipStream_t s, CineAux &out) {
    const size_t T = wk.size(), F = wsum.size();
    const size_t b_map = map.size() * sizeof(int), b_ord = order.size() * sizeof(int);
    const size_t off_ord = (b_map + 7) / 8 * 8, off_wk = (off_ord + b_ord + 7) / 8 * 8, off_ws = off_wk + T * sizeof(double);
    const size_t total = off_ws + F * sizeof(double);
    if (have != key) {
        HIP_TRY(hipStreamSynchronize(s), UKBB_EDEVICE);                      // nothing in flight may still read the old tables
        have = -1;                                                           // until every table is up
        HIP_TRY(buf.ensure_bytes(total), UKBB_ENOMEM);
        char *aux0 = reinterpret_cast<char *>(buf.p);
        HIP_TRY(hipMemcpy(aux0, map.data(), b_map, hipMemcpyHostToDevice), UKBB_EDEVICE);
        HIP_TRY(hipMemcpy(aux0 + off_ord, order.data(), b_ord, hipMemcpyHostToDevice), UKBB_EDEVICE);
        HIP_TRY(hipMemcpy(aux0 + off_wk, wk.data(), T * sizeof(double), hipMemcpyHostToDevice), UKBB_EDEVICE);
        HIP_TRY(hipMemcpy(aux0 + off_ws, wsum.data(), F * sizeof(double), hipMemcpyHostToDevice), UKBB_EDEVICE);
        have = key;
    }
    const char *aux = reinterpret_cast<const char *>(buf.p);
    out.map = reinterpret_cast<const int *>(aux);
    out.tb = CineTable{reinterpret_cast<const int *>(aux + off_ord), reinterpret_cast<const double *>(aux + off_wk),
                       reinterpret_cast<const double *>(aux + off_ws), (int)F, (int)T};
    return UKBB_OK;
}

// ---- Temporal-UNet (kind 3) --------------------------------------------------------------------------
// n_seq windows of T frames through the 3-D plan: image n = window * T + t, outputs in the same [N][T] order
int t3d_forward_seq(ukbb_fcn_handle *h, const float *image, int n_seq, int height, int width,
                    float *logits, float *prob, int32_t *pred, hipStream_t s) {
    if (n_seq < 1) { set_error("forward_seq: n_seq must be positive"); return UKBB_EINVAL; }
    int rc = prepare(h, n_seq * h->arch.fc, height, width);
    if (rc) return rc;
    h->t3d_map = nullptr;
    return run_plan(h, image, n_seq * h->arch.fc, logits, prob, pred, s);
}

// The windowed deploy loop (deploy_network_ao.py:129-183) for one slice position: every window runs the whole 3-D network
// on its T frames (gathered from the cine by the first layer through the window -> frame table); windows go in chunks, in
// ascending order, and each chunk's softmax maps are added into prob by t3d_tile_kernel in the reference's order -- the
// result does not depend on the chunk size.
int t3d_forward_cine(ukbb_fcn_handle *h, const float *image, int F, int height, int width,
                     int weight_R, double weight_r, int time_step, float *prob, int32_t *pred, hipStream_t s) {
    const int T = h->arch.fc, C = h->arch.n_class;
    if (!prob) { set_error("forward_cine: prob must not be NULL"); return UKBB_EINVAL; }
    if (2 * weight_R - 1 != T) { set_error("forward_cine: time window 2*weight_R-1 = %d, the model is built for %d frames", 2 * weight_R - 1, T); return UKBB_EINVAL; }
    if (time_step < 1) { set_error("forward_cine: time_step must be >= 1 (got %d)", time_step); return UKBB_EINVAL; }
    const int rad = (T - 1) / 2;
    if (F < rad || F < 1) { set_error("forward_cine: %d frames, the circular window of radius %d needs at least %d (the reference raises IndexError)", F, rad, rad > 1 ? rad : 1); return UKBB_EINVAL; }
    int rc = prepare(h, T, height, width, h->scratch_budget ? 0 : -1);     // the plan (its per-frame workspace sizes the chunks)
    if (rc) return rc;
    const size_t HW = (size_t)height * width;
    const int Wn = (F + time_step - 1) / time_step;
    // Windows per chunk: as many as fit the scratch budget (without one: T3D_CHUNK_BYTES of activations + window probabilities, at least one
    // window); UKBB_TEMPORAL_CHUNK_WINDOWS=n overrides either (tests force small chunks with it)
    const CineUnits &un = h->cine;
    CinePlan pl;
    if (!plan_cine(un, F, time_step, h->scratch_budget, pl)) {
        set_error("forward_cine: the scratch budget of %llu bytes is below the %llu bytes one window of %d frames of %dx%d needs", (unsigned long long)h->scratch_budget,
                (unsigned long long)pl.min_bytes, T, height, width);
        return UKBB_EINVAL;
    }
    if (const char *e = getenv("UKBB_TEMPORAL_CHUNK_WINDOWS")) { const int v = atoi(e); if (v >= 1) pl.Wc = std::min(v, Wn); }
    const int cw = pl.Wc;
    rc = budget_enter(h, F, height, width, time_step, pl);
    if (rc) return rc;
    rc = prepare(h, cw * T, height, width);
    if (rc) return rc;
    std::vector<int> map, order;
    std::vector<double> wk, wsum;
    cine_tables(F, T, time_step, weight_R, weight_r, map, order, wk, wsum);
    std::vector<int> fmap((size_t)Wn * T);                                  // window-major: batch image (w - w0) * T + k reads frame fmap[w * T + k]
    for (int w = 0; w < Wn; ++w)
        for (int k = 0; k < T; ++k) fmap[(size_t)w * T + k] = map[(size_t)k * Wn + w];
    long long wr_bits;
    memcpy(&wr_bits, &weight_r, sizeof wr_bits);
    const long long key = (((((long long)F << 8) | T) * 1000003ll + time_step) * 1000003ll) ^ wr_bits;
    CineAux aux;
    rc = cine_aux(h->t3d_aux, h->t3d_aux_key, key, fmap, order, wk, wsum, s, aux);
    if (rc) return rc;
    if (h->t3d_probw.n < (size_t)cw * T * HW * C) HIP_TRY(hipStreamSynchronize(s), UKBB_EDEVICE);   // the old buffer may still be read
    HIP_TRY(h->t3d_probw.ensure((size_t)cw * T * HW * C), UKBB_ENOMEM);
    for (int w0 = 0; w0 < Wn; w0 += cw) {
        const int nw = std::min(cw, Wn - w0);
        h->t3d_map = aux.map + (size_t)w0 * T;
        rc = run_plan(h, image, nw * T, nullptr, h->t3d_probw.p, nullptr, s);
        h->t3d_map = nullptr;
        if (rc) return rc;
        T3dTileArgs ta{};
        ta.probw = h->t3d_probw.p;
        ta.tb = aux.tb;
        ta.prob = prob; ta.pred = pred;
        ta.HW = (int)HW; ta.C = C; ta.w0 = w0; ta.w1 = w0 + nw;
        ta.first = w0 == 0; ta.last = w0 + nw == Wn;
        announce_launch(h, s);
        hipError_t e = launch_t3d_tile(ta, s);
        if (e != hipSuccess) { set_error("tiling kernel launch failed: %s", hipGetErrorString(e)); return UKBB_EDEVICE; }
    }
    return UKBB_OK;
}

int lstm_common_checks(ukbb_fcn_handle *h, const float *image, const char *what) {
    if (!h || !image) { set_error("%s: NULL argument", what); return UKBB_EINVAL; }
    if (h->arch.kind != UKBB_KIND_UNET_LSTM) { set_error("%s: the model is not a UNet-LSTM", what); return UKBB_EINVAL; }
    return UKBB_OK;
}

}  // namespace

int ukbb_fcn_forward_seq(ukbb_fcn_handle *h, const float *image, int n_seq, int height, int width,
                         float *logits, float *prob, int32_t *pred, void *stream) {
    if (h) lds_poison_begin(h);
    if (h && image && h->arch.kind == UKBB_KIND_TEMPORAL_UNET)
        return t3d_forward_seq(h, image, n_seq, height, width, logits, prob, pred, static_cast<hipStream_t>(stream));
    int rc = lstm_common_checks(h, image, "forward_seq");
    if (rc) return rc;
    const int T = h->arch.fc, C = h->arch.n_class;
    if (n_seq < 1) { set_error("forward_seq: n_seq must be positive"); return UKBB_EINVAL; }
    h->budget_key = -1;                                                      // the scratch budget bounds forward_cine only: its next call starts from empty buffers again
    rc = prepare(h, n_seq * T, height, width);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    rc = run_plan(h, image, n_seq * T, nullptr, nullptr, nullptr, s);       // U-Net features of every frame
    if (rc) return rc;
    const size_t HW = (size_t)height * width;
    // map[k][w] = w*T + k; outputs straight into [N][T] order
    std::vector<int> map((size_t)T * n_seq);
    for (int k = 0; k < T; ++k)
        for (int w = 0; w < n_seq; ++w) map[(size_t)k * n_seq + w] = w * T + k;
    const long long key = ((long long)n_seq << 8) | T;                       // tables depend on (n_seq, T) only
    if (h->lstm_aux_key != key) {                                            // first call for this shape: upload (blocking)
        HIP_TRY(hipStreamSynchronize(s), UKBB_EDEVICE);                      // nothing in flight may still read the old tables
        HIP_TRY(h->lstm_aux.ensure_bytes(map.size() * sizeof(int)), UKBB_ENOMEM);
        HIP_TRY(hipMemcpy(h->lstm_aux.p, map.data(), map.size() * sizeof(int), hipMemcpyHostToDevice), UKBB_EDEVICE);
        h->lstm_aux_key = key;
    }
    float *out = prob;
    if (!out) {                                                              // the output kernel always forms the probabilities
        HIP_TRY(h->lstm_probw.ensure((size_t)n_seq * T * HW * C), UKBB_ENOMEM);
        out = h->lstm_probw.p;
    }
    const int NF = n_seq * T, NHID = h->arch.same_dim;
    const int *d_map = reinterpret_cast<const int *>(h->lstm_aux.p);
    rc = run_bilstm(h, h->acts[h->plan.feat_buf].buf.p, NF, d_map, n_seq, height, width, s);
    if (rc) return rc;
    const size_t kst = (size_t)n_seq * HW * NHID, esz = h->plan.mode.bfio() ? 2 : 4;
    for (int k = 0; k < T; ++k) {                                            // outputs straight into [N][T] order
        LstmOutArgs oa{};
        oa.h_bf16 = h->plan.mode.bfio() ? 1 : 0;
        oa.hf = k == 0 ? h->lstm_h1.p : at(h->lstm_hall.p, (size_t)k * kst, esz);
        oa.mapf = k == 0 ? d_map : nullptr;
        oa.hb = k == T - 1 ? at(h->lstm_h1.p, (size_t)NF * HW * NHID, esz) : at(h->lstm_hall.p, (size_t)T * kst + (size_t)k * kst, esz);
        oa.mapb = k == T - 1 ? d_map + (size_t)(T - 1) * n_seq : nullptr;
        oa.w_out = h->par.lstm_out_w; oa.b_out = h->par.lstm_out_b;
        oa.prob = out + (size_t)k * HW * C;
        oa.logits = logits ? logits + (size_t)k * HW * C : nullptr;
        oa.pred = pred ? pred + (size_t)k * HW : nullptr;
        oa.m_stride = (long long)T * HW * C; oa.M = n_seq; oa.HW = (int)HW; oa.n_class = C;
        announce_launch(h, s);
        hipError_t e = launch_lstm_out(oa, s);
        if (e != hipSuccess) { set_error("ConvLSTM output kernel launch failed: %s", hipGetErrorString(e)); return UKBB_EDEVICE; }
    }
    return UKBB_OK;
}

int ukbb_fcn_forward_cine(ukbb_fcn_handle *h, const float *image, int n_frames, int height, int width,
                          int weight_R, double weight_r, int time_step, float *prob, int32_t *pred, void *stream) {
    if (h) lds_poison_begin(h);
    if (h && image && h->arch.kind == UKBB_KIND_TEMPORAL_UNET)
        return t3d_forward_cine(h, image, n_frames, height, width, weight_R, weight_r, time_step, prob, pred, static_cast<hipStream_t>(stream));
    int rc = lstm_common_checks(h, image, "forward_cine");
    if (rc) return rc;
    const int T = h->arch.fc, C = h->arch.n_class, F = n_frames;
    if (!prob) { set_error("forward_cine: prob must not be NULL"); return UKBB_EINVAL; }
    if (2 * weight_R - 1 != T) { set_error("forward_cine: time window 2*weight_R-1 = %d, the model is unrolled for %d steps", 2 * weight_R - 1, T); return UKBB_EINVAL; }
    if (time_step < 1) { set_error("forward_cine: time_step must be >= 1 (got %d)", time_step); return UKBB_EINVAL; }
    const int rad = (T - 1) / 2;
    // the reference wraps a window index once only (i < 0: i + T; i >= T: i - T, deploy_network_ao.py:151-157):
    // with fewer than rad frames the wrapped index is still out of range and numpy raises IndexError
    if (F < rad || F < 1) { set_error("forward_cine: %d frames, the circular window of radius %d needs at least %d (the reference raises IndexError)", F, rad, rad > 1 ? rad : 1); return UKBB_EINVAL; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t HW = (size_t)height * width;
    const int Wn = (F + time_step - 1) / time_step;                         // window centres range(0, F, time_step) (:147)
    // The plan is chosen for the whole cine (its tilings and the ConvLSTM region shape must not depend on the chunk size); under a scratch
    // budget the workspace is sized for a chunk's frame run only.
    rc = prepare(h, F, height, width, h->scratch_budget ? 0 : -1);
    if (rc) return rc;
    const CineUnits &un = h->cine;
    CinePlan pl;
    if (!plan_cine(un, F, time_step, h->scratch_budget, pl)) {
        set_error("forward_cine: the scratch budget of %llu bytes is below the minimum of %llu bytes for %d frames of %dx%d at time_step %d", (unsigned long long)h->scratch_budget,
                (unsigned long long)pl.min_bytes, F, height, width, time_step);
        return UKBB_EINVAL;
    }
    const int Wc = pl.Wc;
    if (pl.chunks > 1 && h->plan.mode.bfio() && (h->plan.lstm_bf_wino || !h->plan.lstm_bf_hoist)) {
        set_error("forward_cine: the A/B forms UKBB_LSTM_BF16_WINOGRAD / UKBB_LSTM_BF16_UNHOIST run unchunked only (unset them or the scratch budget)");
        return UKBB_EINVAL;
    }
    rc = budget_enter(h, F, height, width, time_step, pl);
    if (rc) return rc;
    rc = prepare(h, F, height, width, pl.run);
    if (rc) return rc;
    std::vector<int> map, order;
    std::vector<double> wk, wsum;
    cine_tables(F, T, time_step, weight_R, weight_r, map, order, wk, wsum);
    // Chunk c = windows [w0, w0 + nw) reads the circular frame run starting at frame r0 = w0 * time_step - rad; its table (at map offset
    // T * w0, step-major [k * nw + (w - w0)]) holds run-local frames.  One chunk: r0 = 0, the run is the cine and the table is `map` itself.
    auto run_start = [&](int w0) { const int r = (w0 * time_step - rad) % F; return r < 0 ? r + F : r; };
    if (pl.chunks > 1) {
        std::vector<int> cmap(map.size());
        for (int w0 = 0; w0 < Wn; w0 += Wc) {
            const int nw = std::min(Wc, Wn - w0), r0 = run_start(w0);
            for (int k = 0; k < T; ++k)
                for (int w = w0; w < w0 + nw; ++w) {
                    const int loc = map[(size_t)k * Wn + w] - r0;
                    cmap[(size_t)T * w0 + (size_t)k * nw + (w - w0)] = loc < 0 ? loc + F : loc;
                }
        }
        map.swap(cmap);
    }
    long long wr_bits;
    memcpy(&wr_bits, &weight_r, sizeof wr_bits);
    // cine tables: (F, T, time_step, weight_r) and the chunk plan
    const long long key = (((((long long)F << 8) | T) * 1000003ll + time_step) * 1000003ll) ^ wr_bits ^ (1ll << 62) ^ (pl.chunks > 1 ? (long long)Wc << 40 : 0);
    CineAux aux;
    rc = cine_aux(h->lstm_aux, h->lstm_aux_key, key, map, order, wk, wsum, s, aux);
    if (rc) return rc;
    const int NHID = h->arch.same_dim;
    const size_t esz = h->plan.mode.bfio() ? 2 : 4;
    if (pl.chunks > 1) HIP_TRY(h->lstm_img.ensure((size_t)pl.run * HW), UKBB_ENOMEM);
    for (int w0 = 0; w0 < Wn; w0 += Wc) {
        const int nw = std::min(Wc, Wn - w0);
        const int R = pl.chunks > 1 ? (int)std::min<long long>(F, (long long)(nw - 1) * time_step + T) : F;   // frames of this chunk's run
        const float *frames = image;
        if (pl.chunks > 1) {                                                 // the run, contiguous: frames [r0, F) then [0, ...) when it wraps
            const int r0 = run_start(w0), n0 = std::min(R, F - r0);
            HIP_TRY(hipMemcpyAsync(h->lstm_img.p, image + (size_t)r0 * HW, (size_t)n0 * HW * sizeof(float), hipMemcpyDeviceToDevice, s), UKBB_EDEVICE);
            if (R > n0) HIP_TRY(hipMemcpyAsync(h->lstm_img.p + (size_t)n0 * HW, image, (size_t)(R - n0) * HW * sizeof(float), hipMemcpyDeviceToDevice, s), UKBB_EDEVICE);
            frames = h->lstm_img.p;
        }
        rc = run_plan(h, frames, R, nullptr, nullptr, nullptr, s);          // each frame's U-Net features, once per chunk that reads it
        if (rc) return rc;
        const int *d_map = aux.map + (size_t)T * w0;
        rc = run_bilstm(h, h->acts[h->plan.feat_buf].buf.p, R, d_map, nw, height, width, s);
        if (rc) return rc;
        LstmTileArgs ta{};
        ta.k_stride = (long long)nw * HW * NHID;
        ta.h_bf16 = h->plan.mode.bfio() ? 1 : 0;
        ta.hf = h->lstm_hall.p; ta.hb = at(h->lstm_hall.p, (size_t)T * ta.k_stride, esz);
        ta.h1f = h->lstm_h1.p; ta.h1b = at(h->lstm_h1.p, (size_t)R * HW * NHID, esz);
        ta.map_first = d_map; ta.map_last = d_map + (size_t)(T - 1) * nw;
        ta.w_out = h->par.lstm_out_w; ta.b_out = h->par.lstm_out_b;
        ta.tb = aux.tb;
        ta.prob = prob; ta.pred = pred; ta.Wn = nw; ta.HW = (int)HW; ta.C = C;
        ta.w0 = w0; ta.w1 = w0 + nw; ta.first = w0 == 0; ta.last = w0 + nw == Wn;
        announce_launch(h, s);
        hipError_t e = launch_lstm_tile(ta, s);
        if (e != hipSuccess) { set_error("tiling kernel launch failed: %s", hipGetErrorString(e)); return UKBB_EDEVICE; }
    }
    return UKBB_OK;
}

int ukbb_fcn_num_kernels(const ukbb_fcn_handle *h) { return h ? (int)h->ops.size() : 0; }

static const BoundOp *op_at(const ukbb_fcn_handle *h, int i) { return h && i >= 0 && i < (int)h->ops.size() ? &h->ops[i] : nullptr; }

const char *ukbb_fcn_kernel_name(const ukbb_fcn_handle *h, int i) { return op_at(h, i) ? op_at(h, i)->name.c_str() : ""; }

double ukbb_fcn_kernel_macs(const ukbb_fcn_handle *h, int i) { return op_at(h, i) ? op_at(h, i)->macs_per_image * h->last_n : 0.0; }

double ukbb_fcn_kernel_mfma_macs(const ukbb_fcn_handle *h, int i) {
    const BoundOp *op = op_at(h, i);
    return op ? (op->mfma_macs_per_image >= 0 ? op->mfma_macs_per_image : op->macs_per_image) * h->last_n : 0.0;
}

double ukbb_fcn_kernel_mfma_macs_issued(const ukbb_fcn_handle *h, int i) {
    const BoundOp *op = op_at(h, i);
    return op && op->padded_macs_per_image >= 0 ? op->padded_macs_per_image * h->last_n : ukbb_fcn_kernel_mfma_macs(h, i);
}

int ukbb_fcn_set_precision(ukbb_fcn_handle *h, int precision) {
    PlanMode m;
    const char *why;
    const int rc = h ? plan_mode(h->arch, precision, m, &why) : UKBB_EINVAL;
    if (rc == UKBB_EINVAL) { set_error("set_precision: bad argument"); return rc; }
    if (rc) { set_error("set_precision: %s", why); return rc; }
    if (precision != h->precision) {
        if (hipSetDevice(h->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { set_error("set_precision: device sync failed"); return UKBB_EDEVICE; }
        h->precision = precision;
        h->plan_h = h->plan_w = 0;               // re-plan (tilings and packed weights differ)
    }
    return UKBB_OK;
}

int ukbb_fcn_set_f32x3_convs(ukbb_fcn_handle *h, int on) {
    if (!h) { set_error("set_f32x3_convs: NULL handle"); return UKBB_EINVAL; }
    if (refuse_f32x3_convs(h->arch.kind)) return UKBB_EARCH;
    const bool want = on != 0;
    if (want != h->f32x3_convs) {
        if (hipSetDevice(h->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { set_error("set_f32x3_convs: device sync failed"); return UKBB_EDEVICE; }
        h->f32x3_convs = want;
        h->plan_h = h->plan_w = 0;               // re-plan, as set_precision does (under any precision but UKBB_PREC_F32X3 the same plan comes back)
    }
    return UKBB_OK;
}

int ukbb_fcn_kernel_config(const ukbb_fcn_handle *h, int i) {
    const BoundOp *op = op_at(h, i);
    return op && (op->kind == OP_CONV || op->kind == OP_TCONV) ? op->cfg : -1;
}

int ukbb_fcn_head_tail_form(void) { return head_tail_form(); }

const char *ukbb_fcn_conv_config_name(int id) {
    for (int i = 0; i < num_conv_configs(); ++i)
        if (conv_config(i).id == id) return conv_config(i).name;
    return "";
}

int ukbb_fcn_set_timing(ukbb_fcn_handle *h, int enable) {
    if (!h) { set_error("set_timing: NULL handle"); return UKBB_EINVAL; }
    int rc = collect_events(h);
    if (rc) return rc;
    h->timing = enable != 0;
    h->timing_only = -1;
    return UKBB_OK;
}

int ukbb_fcn_set_timing_kernel(ukbb_fcn_handle *h, int kernel) {
    if (!h) { set_error("set_timing_kernel: NULL handle"); return UKBB_EINVAL; }
    int rc = collect_events(h);
    if (rc) return rc;
    if (kernel >= (int)h->ops.size()) { set_error("set_timing_kernel: index out of range"); return UKBB_EINVAL; }
    h->timing = true;
    h->timing_only = kernel < 0 ? -1 : kernel;
    return UKBB_OK;
}

int ukbb_fcn_kernel_times(ukbb_fcn_handle *h, double *sum_ms, int64_t *count, int n, int reset) {
    if (!h) { set_error("kernel_times: NULL handle"); return UKBB_EINVAL; }
    int rc = collect_events(h);
    if (rc) return rc;
    const int m = std::min<int>(n, (int)h->ops.size());
    for (int i = 0; i < m; ++i) {
        if (sum_ms) sum_ms[i] = h->t_sum[i];
        if (count) count[i] = h->t_cnt[i];
    }
    if (reset) { std::fill(h->t_sum.begin(), h->t_sum.end(), 0.0); std::fill(h->t_cnt.begin(), h->t_cnt.end(), 0); }
    return m;
}

int64_t ukbb_fcn_get_activation(ukbb_fcn_handle *h, const char *name, float *dst, int64_t cap) {
    if (!h || !name) { set_error("get_activation: NULL argument"); return UKBB_EINVAL; }
    // an activation map of the plan by its name, or a ConvLSTM working buffer raw (tools/debug_lstm.py decodes the lane-native ones):
    // whatever the last sequence call left in it
    const ActMap *map = nullptr;
    const DevBuf *src = nullptr;
    int64_t n = 0;
    for (const ActMap &m : h->acts)
        if (!src && m.name == name) { map = &m; src = &m.buf; n = (int64_t)m.per_image * h->last_n; }
    for (const HandleBuf &b : HANDLE_BUFS)
        if (!src && b.raw && !strcmp(b.raw, name)) { src = &(h->*b.buf); n = (int64_t)src->n; }
    if (!src) { set_error("get_activation: no activation named '%s'", name); return UKBB_EINVAL; }
    if (!dst) return n;
    if (cap < n) { set_error("get_activation: buffer too small (%lld < %lld)", (long long)cap, (long long)n); return UKBB_EINVAL; }
    const bool bf = map && map->esz == 2;              // stored as bf16: widen on the host
    std::vector<uint16_t> tmp(bf ? (size_t)n : 0);
    if (hipSetDevice(h->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(bf ? (void *)tmp.data() : (void *)dst, src->p, (size_t)n * (bf ? 2 : 4), hipMemcpyDeviceToHost) != hipSuccess) {
        set_error("get_activation: device copy failed");
        return UKBB_EDEVICE;
    }
    if (bf) {
        // channel-blocked on the device ([N][C/16][H][W][16], kernels.h); handed out as NHWC like the fp32 plans' maps
        const int64_t C = map->ch, per = (int64_t)map->per_image, hw = C > 0 ? per / C : 0;
        for (int64_t k = 0; k < n; ++k) {
            int64_t at_k = k;
            if (C > 16 && C % 16 == 0) {
                const int64_t img = k / per, r = k - img * per, px = r / C, c = r - px * C;
                at_k = img * per + ((c >> 4) * hw + px) * 16 + (c & 15);
            }
            const uint32_t u = (uint32_t)tmp[(size_t)at_k] << 16; memcpy(dst + k, &u, 4);
        }
    }
    return n;
}

}  // extern "C"
