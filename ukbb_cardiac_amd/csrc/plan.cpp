// Host-only planner (plan.h): architecture walk, conv tiling choice, the launch plan's layout and the chunk plan of forward_cine.
// No HIP call and no handle in this file: everything here runs, and is tested, without a GPU.  The device's compute-unit count is an
// argument wherever a choice depends on it.
#include "plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace ukbb {

// ---- architecture walk ---------------------------------------------------------
bool arch_specs(const ukbb_fcn_arch &a, std::vector<Spec> &out) {
    out.clear();
    if (a.n_level < 1 || a.n_level > UKBB_FCN_MAX_LEVEL || a.n_class < 1) return false;
    int cin = 1;
    char nm[64];
    for (int l = 0; l < a.n_level; ++l) {
        if (a.n_block[l] < 1 || a.n_filter[l] < 1) return false;
        for (int i = 0; i < a.n_block[l]; ++i) {
            snprintf(nm, sizeof nm, "conv%d_%d", l, i);
            out.push_back({nm, 3, cin, a.n_filter[l], true, false, false});
            cin = a.n_filter[l];
        }
    }
    if (a.kind == UKBB_KIND_FCN) {
        for (int l = 0; l < a.n_level; ++l) {
            snprintf(nm, sizeof nm, "same_dim%d", l);
            out.push_back({nm, 1, a.n_filter[l], a.same_dim, true, false, false});
        }
        out.push_back({"out0", 1, a.same_dim * a.n_level, a.fc, true, false, false});
        out.push_back({"out1", 1, a.fc, a.fc, true, false, false});
        out.push_back({"logits", 1, a.fc, a.n_class, false, true, false});
    } else if (a.kind == UKBB_KIND_TEMPORAL_UNET) {
        // network_ao.py:67-114: every 3x3 unit of the U-Net as a 3x3x3 conv3d (DHWIO) / conv3d_transpose ([3,3,3,Cout,Cin])
        // [TF-recall]; conv_out a 1x1x1 conv3d with bias
        for (auto &s : out) s.kd = 3;
        for (int l = a.n_level - 2; l >= 0; --l) {
            snprintf(nm, sizeof nm, "up%d_t", l);
            out.push_back({nm, 3, a.n_filter[l + 1], a.n_filter[l], true, false, true, 3});
            int c = 2 * a.n_filter[l];
            for (int i = 0; i < a.n_block[l]; ++i) {
                snprintf(nm, sizeof nm, "up%d_%d", l, i);
                out.push_back({nm, 3, c, a.n_filter[l], true, false, false, 3});
                c = a.n_filter[l];
            }
        }
        out.push_back({"logits", 1, a.n_filter[0], a.n_class, false, true, false, 1});
    } else if (a.kind == UKBB_KIND_UNET || a.kind == UKBB_KIND_UNET_LSTM) {
        for (int l = a.n_level - 2; l >= 0; --l) {
            snprintf(nm, sizeof nm, "up%d_t", l);
            out.push_back({nm, 3, a.n_filter[l + 1], a.n_filter[l], true, false, true});
            int c = 2 * a.n_filter[l];
            for (int i = 0; i < a.n_block[l]; ++i) {
                snprintf(nm, sizeof nm, "up%d_%d", l, i);
                out.push_back({nm, 3, c, a.n_filter[l], true, false, false});
                c = a.n_filter[l];
            }
        }
        if (a.kind == UKBB_KIND_UNET) {
            out.push_back({"logits", 1, a.n_filter[0], a.n_class, false, true, false});
        } else {                                  // BiConv_LSTM, network_ao.py:255-319 (same_dim = hidden channels)
            if (a.same_dim < 1 || a.fc < 1) return false;
            out.push_back({"lstm_fw", 3, a.n_filter[0] + a.same_dim, 4 * a.same_dim, false, true, false});
            out.push_back({"lstm_bw", 3, a.n_filter[0] + a.same_dim, 4 * a.same_dim, false, true, false});
            out.push_back({"lstm_out", 1, 2 * a.same_dim, a.n_class, false, true, false});
        }
    } else {
        return false;
    }
    return true;
}

size_t spec_floats(const Spec &s) {
    size_t n = (size_t)s.kd * s.ks * s.ks * s.cin * s.cout;
    if (s.bn) n += 4 * (size_t)s.cout;
    if (s.bias) n += s.cout;
    return n;
}

bool supported(const ukbb_fcn_arch &a, std::string &why) {
    if (a.n_level != 5) { why = "n_level must be 5"; return false; }
    if (a.n_filter[0] != 16) { why = "n_filter[0] must be 16"; return false; }
    for (int l = 1; l < a.n_level; ++l)
        if (a.n_filter[l] < 32 || a.n_filter[l] % 32) { why = "n_filter[l>0] must be multiples of 32"; return false; }
    if (a.kind == UKBB_KIND_FCN) {
        if (a.same_dim != 32 || a.fc != 64) { why = "FCN head kernel is built for same_dim=32, fc=64"; return false; }
        if (a.n_class < 2 || a.n_class > 6) { why = "n_class must be in 2..6"; return false; }
        for (int l = 1; l < a.n_level; ++l)                  // launch_sqg's instances (kernels_head.hip); sqg_body's load loop covers no other width
            if (a.n_filter[l] != 32 && a.n_filter[l] != 64 && a.n_filter[l] != 128 && a.n_filter[l] != 256) {
                why = "FCN squeeze kernels are built for n_filter[l>0] in {32, 64, 128, 256}"; return false;
            }
    } else {
        if (a.n_class < 2 || a.n_class > 4) { why = "UNet n_class must be in 2..4"; return false; }
        if (a.kind == UKBB_KIND_TEMPORAL_UNET) {
            if (a.fc < 1 || a.fc > 31 || !(a.fc & 1)) { why = "the time window must be odd and < 32 frames"; return false; }
        }
        if (a.kind == UKBB_KIND_UNET_LSTM) {
            if (a.same_dim != 16) { why = "ConvLSTM kernels are built for 16 hidden channels"; return false; }
            if (a.fc < 1 || a.fc > 31 || !(a.fc & 1)) { why = "the time window must be odd and < 32 steps"; return false; }
        }
    }
    return true;
}

int find_cfg(int id, ConvConfig &out) {
    for (int i = 0; i < num_conv_configs(); ++i)
        if (conv_config(i).id == id) { out = conv_config(i); return 0; }
    return -1;
}

namespace {

// ---- conv tiling choice --------------------------------------------------------
int override_cfg(const std::string &layer) {
    const char *env = getenv("UKBB_CONV_CFG");     // e.g. "conv0_1:7,conv4_1:6"
    if (!env) return -1;
    std::string s(env);
    size_t pos = 0;
    while (pos < s.size()) {
        size_t e = s.find(',', pos);
        if (e == std::string::npos) e = s.size();
        std::string item = s.substr(pos, e - pos);
        size_t c = item.find(':');
        if (c != std::string::npos && item.substr(0, c) == layer) return atoi(item.c_str() + c + 1);
        pos = e + 1;
    }
    return -1;
}

// Tilings measured best on MI355X (tools/tune_convs.py, profiles/r01_tune_convs*.txt): {ks, stride, cin, cout, cfg}
// per layer type, for large batches (tuned at N = 64, 192x208) and for small ones (tuned at N = 10, the
// reference's own per-frame call, deploy_network.py:103-111: there the persistent kernels have fewer work
// items than CUs, and tilings with smaller channel groups / tiles win).  Other image sizes of the same layer
// type reuse the entry (e.g. the long-axis models at 176x208).
struct Tuned { int ks, stride, cin, cout, cfg, alt, alt2, alt3 = -1; };   // alt.. (or -1): the first of the four whose tiles divide the map wins
const Tuned g_tuned_large[] = {
    {3, 1, 16, 16, 11, -1, -1}, {3, 2, 16, 32, 120, 123, -1},  {3, 1, 32, 32, 307, 301, -1},
    {3, 2, 32, 64, 124, 123, 142, 145},  {3, 1, 64, 64, 304, 300, -1},  {3, 2, 64, 128, 124, 123, 142, 145},
    {3, 1, 128, 128, 304, 300, -1},  {3, 2, 128, 256, 124, 123, 142, 145}, {3, 1, 256, 256, 304, 305, 300},
};      // r03: 13x16 tiles (145) divide the 208x256 pyramid (52x64, 26x32, 13x16: conv2_0 112 -> 86 us, conv3_0 / conv4_0 -6 / -7 at N = 64);
        // r02: the stride-2 layers moved to the producer/consumer kernel once its loads ran two stages ahead (profiles/r02_notes.md);
        // its straight-line producer needs tiles that divide the map: 12x13 tiles for the 192x208 pyramid, 8x16 (123) for the
        // power-of-two maps of the aortic U-Net (256x256: 148 / 143 / 133 / 136 us instead of 184 / 208 / 159 / 156 at N = 100),
        // 11x13 (142) for the long-axis models' 176x208 pyramid (88x104, 44x52, 22x26, 11x13)
const Tuned g_tuned_small[] = {
    {3, 1, 16, 16, 11, -1, -1}, {3, 2, 16, 32, 29, -1, -1},  {3, 1, 32, 32, 301, -1, -1},
    {3, 2, 32, 64, 20, -1, -1},  {3, 1, 64, 64, 300, -1, -1},  {3, 2, 64, 128, 123, -1, -1},
    {3, 1, 128, 128, 301, -1, -1},  {3, 2, 128, 256, 26, -1, -1}, {3, 1, 256, 256, 301, -1, -1},
};
// The small-batch table is opt-in (UKBB_SMALL_BATCH_TILINGS=1; +30 % at N = 10): with it the tiling, and so
// the fp32 summation order, would depend on the batch size, and by default the engine guarantees bit-identical
// results for a slice whatever batch it is part of (tests: batch independence).
bool small_batch_tilings() { static const bool on = getenv("UKBB_SMALL_BATCH_TILINGS") != nullptr; return on; }

// A tuned tiling is reused for another image size only if its tiles still fit that size well.
bool tile_fit_ok(const ConvConfig &c, int Ho, int Wo) {
    const double covered = (double)round_up(Ho, c.th) * round_up(Wo, c.tw);
    // Winograd kept its lead over the direct tilings down to 61 % region fill (12x13 maps, r01 sweep)
    // F(2x4) regions: at 61 % fill (12 x 13 maps) the F(2x2) kernel with its half regions (81 %) is as fast, at 74 % (44 x 52, 22 x 26) F(2x4) still wins by 2 %
    return (double)Ho * Wo >= (is_wino24(c) ? 0.7 : is_wino(c) ? 0.5 : 0.8) * covered;
}
// Fallback preference (small tiles / high occupancy won everywhere in the sweep).
const int g_pref[] = {4, 5, 18, 3, 11, 7, 31, 23, 22, 29, 27, 26};

// a bf16-operand tiling only in a bf16-operand plan, a bf16-storage tiling only in a bf16-storage plan, an fp32 tiling in either of the others;
// x3: the layer is one a conv_x3 plan runs on three bf16 pieces (x3_layer) -- it then takes a ConvFamily::F32x3Operands tiling and no other,
// and no other layer of any plan takes one
bool cfg_valid(const ConvConfig &c, int ks, int stride, int c0, int c1, int cout, bool fused_first = false,
               Bf16Mode bf16 = Bf16Mode::None, int fuse = 0, bool x3 = false) {
    if (c.ks != ks || c.stride != stride) return false;
    if ((c.family == ConvFamily::F32x3Operands) != x3) return false;
    if (x3) return !fused_first && !fuse && bf16 == Bf16Mode::None && ks == 3 && c1 == 0 && c0 >= c.kc && c0 % c.kc == 0 &&
                   cout % cout_per_item(c) == 0 && c.lds_bytes <= 160 * 1024;
    if (c.fuse != fuse) return false;
    if (fuses_first(c) != fused_first) return false;
    if (c.family == ConvFamily::FirstWino22) {        // fused first layer + Winograd conv0_1: the 16 -> 16 stem of the fp32 FCN plans only
        static const bool off = getenv("UKBB_NO_WINOGRAD_FIRST") != nullptr;    // A/B knob: the direct fused kernel (130-133)
        if (off || ks != 3 || stride != 1 || c0 != 16 || c1 != 0 || cout != 16) return false;
    }
    if ((c.family == ConvFamily::Bf16Operands) != (bf16 == Bf16Mode::Operands) || stores_bf16(c) != (bf16 == Bf16Mode::Storage)) return false;
    cout = packed_cout(c, cout);
    if (c.family == ConvFamily::Bf16StoreWs) {        // weight-stationary: the Cout group's whole packed filter + the waves' rings in LDS
        const int nch = (c0 + c1) / 16;
        if (stride != 1 || (c0 + c1) % 16) return false;
        if (ks == 2) {                                // transposed conv as 2x2 sub-pixel conv: cout = 4 x real channels (16, or multiples of 32)
            const int real = cout / 4;
            if (c1 || cout % 64 || (real != 16 && real % 32) || (real == 16 ? nch != 2 : (nch != 4 && nch != 8))) return false;
        } else if (c.kc == 32) {                      // weights through a ring: any even number of chunks, source switch at an even chunk
            if (ks != 3 || nch < 2 || (nch & 1) || (c1 && (c0 / 16) % 2)) return false;
        } else if (ks != 3 || (c1 && c1 != c0) || (nch != 1 && nch != 2 && nch != 4 && nch != 8) || (c1 && nch < 2)) return false;
        if (cout % (32 * c.cb)) return false;
        return ws_lds_bytes_for(c, c0 + c1) <= 160 * 1024;
    }
    if (is_wino(c)) {                                 // Winograd: 3x3 s1, 64-channel output groups, single source ok
        static const bool off = getenv("UKBB_NO_WINOGRAD") != nullptr;
        if (c.id == 306) {                            // image pairs with seam regions (maps with Ho % 8 == 4): only where UKBB_CONV_CFG names it -- at N = 64 its 384
            const char *e = getenv("UKBB_CONV_CFG");   // items leave half the CUs idle in the second round, and the plan must not depend on the batch (r04_notes.md)
            if (!e || !strstr(e, ":306")) return false;
        }
        if (is_wino24(c)) {                           // F(2x4,3x3), kernels_wino24.hip: 64-channel groups, K >= 64 (the MFMA-bound layers; no frame map)
            static const bool off24 = getenv("UKBB_NO_WINOGRAD24") != nullptr;
            if (off24) return false;
            if (c.wm == 2) { if (cout != 32) return false; }   // 32-channel items (307): the layers with exactly 32 output channels
            else if (cout % 64 || c0 + c1 < 32) return false;   // K = 32: the ConvLSTM gate convs (16 + 16 -> 64)
        }
        return !off && !fused_first && ks == 3 && stride == 1 && cout % cout_per_item(c) == 0 && c0 % 16 == 0 && c1 % 16 == 0;
    }
    if (fuses_first(c) && cout != cout_per_item(c)) return false;  // fused kernel stages its weights once: one Cout group
    if (c.lds_bytes > 160 * 1024) return false;      // LDS per CU on gfx950
    return !(cout % cout_per_item(c) || c0 % c.kc || c1 % c.kc);
}

// Winograd regions are 8x16 (ids 300/301) or 16x8 pixels (302/303): take the orientation with fewer regions.
int wino_orient(int id, int Ho, int Wo) {
    if (id < 300 || id > 303) return id;
    const int base = 300 + (id & 1);
    const long long r_8x16 = (long long)((Ho + 7) / 8) * ((Wo + 15) / 16), r_16x8 = (long long)((Ho + 15) / 16) * ((Wo + 7) / 8);
    return r_16x8 < r_8x16 ? base + 2 : base;
}

int choose_cfg_raw(const std::string &layer, int ks, int stride, int c0, int c1, int cout, int Ho, int Wo, int N,
                   bool fused_first, Bf16Mode want_bf16, bool wino_first);

// Small batches (N <= SMALL_BATCH, e.g. the reference's own sess.run of one frame's 10 slices, deploy_network.py:103-111): the
// deep levels have fewer work items than the chip has CUs, and a CU streaming an item's weights alone pulls only ~25-50 GB/s
// from L2, so those layers are bound by the number of CUs at work.  Swap the tiling for a FINER SIBLING THAT COMPUTES EVERY
// OUTPUT WITH THE SAME ARITHMETIC -- same algorithm, MFMA shape, channels per stage and tile, only fewer output channels per
// work item -- so results stay bit-identical whatever batch a slice is part of (tests: batch independence, slices of the
// bench batch against single-slice runs).  The r01 small-batch table (other tiles / KC) stays opt-in for that reason.
int finer_sibling(int id, int ks, int stride, int c0, int c1, int cout, int Ho, int Wo, int N, int cus) {
    static const bool off = getenv("UKBB_NO_SMALL_BATCH_SIBLINGS") != nullptr;    // A/B knob
    if (off || N > SMALL_BATCH) return id;
    static const int sib[][2] = {{300, 301}, {302, 303},     // Winograd: 64 -> 32 output channels per item
                                 {124, 141}};                // stride-2 producer/consumer, mb16 12x13 kc8: Cout blocks per wave 2 -> 1
    ConvConfig c, f;
    if (find_cfg(id, c)) return id;
    for (const auto &p : sib) {
        if (p[0] != id || find_cfg(p[1], f) || !cfg_valid(f, ks, stride, c0, c1, cout)) continue;
        const long long items = (long long)map_tiles(c, Ho, Wo) * N * (cout / cout_per_item(c));
        if (items <= cus / 2) return p[1];      // at most half the CUs (of the planned device) at work: halve the item (r03 on 256 CUs: 160-210 items were faster left alone)
    }
    return id;
}

// Winograd F(2x4,3x3) comes with 8 x 32-pixel regions (304) and 8 x 16 (305); both compute every tile with the same arithmetic (same tile
// grid, same transforms, same K order), so the choice is a matter of filling the CUs: the region shape whose item count wastes less of
// the last round wins, 304 on a tie (fewer, longer items: FCN level 2 60 us against 65); small batches take the finer one.
int pick_wino24(int id, int ks, int stride, int c0, int c1, int cout, int Ho, int Wo, int N, int cus) {
    if (id != 304 && id != 305) return id;
    int best = id; double best_eff = -1.0;
    for (int cand : {304, 305}) {
        ConvConfig c;
        if (find_cfg(cand, c) || !cfg_valid(c, ks, stride, c0, c1, cout) || !tile_fit_ok(c, Ho, Wo)) continue;
        const long long items = (long long)N * map_tiles(c, Ho, Wo) * (cout / 64);
        const long long rounds = (items + cus - 1) / cus;
        // makespan in units of an 8 x 16 region's work (an 8 x 32 item is two): the shorter wins -- that counts the padding columns of the
        // wider regions as well as the idle CUs of the last round
        double eff = 1.0 / (double)(rounds * (c.tw / 16));
        if (N <= SMALL_BATCH) eff = cand == 305 ? 2.0 : 1.0;          // fewer items than CUs either way: more of them
        if (eff > best_eff + 1e-12) { best_eff = eff; best = cand; }
    }
    return best;
}

// wino_first: the plan may run a fused first layer's conv0_1 as Winograd (tiling 134; plan_conv: fp32 FCN plans only)
int choose_cfg(const std::string &layer, int ks, int stride, int c0, int c1, int cout, int Ho, int Wo, int N, int cus,
               bool fused_first = false, Bf16Mode want_bf16 = Bf16Mode::None, bool wino_first = false) {
    const int id = choose_cfg_raw(layer, ks, stride, c0, c1, cout, Ho, Wo, N, fused_first, want_bf16, wino_first);
    if (override_cfg(layer) >= 0) return id;
    return finer_sibling(wino_orient(pick_wino24(id, ks, stride, c0, c1, cout, Ho, Wo, N, cus), Ho, Wo), ks, stride, c0, c1, cout, Ho, Wo, N, cus);
}

// bf16-storage tilings measured best per layer type of the aortic U-Net at N = 100 x 256 x 256 (tools/sweep_convs.py with
// PREC=bf16, profiles/r03_sweep_bf16.txt): {ks, stride, cin (both sources), cout (4 x cout for the 2x2 form of a transposed conv), cfg}.
// Levels 2-4 sit on a 35-50 us floor per launch whatever the tiling (launch + first-load latency + tail at 100-400 tiles);
// the table mostly avoids the bad cases (conv3_0 108 -> 47 us, up2_0 104 -> 80, conv2_0 61 -> 45).
// r04: the weight-stationary persistent tilings (400-403, kernels_ws.hip) where a Cout group's whole filter fits LDS (K <= 1152); up3_0
// (K = 2304) on the ring-streamed form 422 (72 vs 78 us; one barrier per chunk keeps it from the ws rate, r04_notes.md)
const Tuned g_tuned_bfio[] = {
    {3, 1, 16, 16, 236, 232, -1},   {3, 1, 32, 32, 401, 232, -1},   {3, 1, 64, 64, 402, 235, 232},    {3, 1, 128, 128, 400, 235, 232},
    {3, 1, 256, 256, 239, 232, -1}, {3, 1, 256, 128, 422, 239, 232}, {3, 1, 128, 64, 400, 239, 232},  {3, 1, 64, 32, 401, 232, -1},
    {3, 1, 32, 16, 401, 236, 232},
    {3, 2, 16, 32, 241, -1, -1},    {3, 2, 32, 64, 242, 241, -1},   {3, 2, 64, 128, 244, 241, -1},  {3, 2, 128, 256, 244, 241, -1},
    {2, 1, 256, 512, 253, 251, -1}, {2, 1, 128, 256, 411, 253, 251}, {2, 1, 64, 128, 411, 253, 251},  {2, 1, 32, 64, 410, 258, 253},
};

int choose_cfg_raw(const std::string &layer, int ks, int stride, int c0, int c1, int cout, int Ho, int Wo, int N,
                   bool fused_first, Bf16Mode want_bf16, bool wino_first) {
    if (want_bf16 == Bf16Mode::Storage && !fused_first && override_cfg(layer) < 0) {
        for (const Tuned &t : g_tuned_bfio) {
            if (t.ks != ks || t.stride != stride || t.cin != c0 + c1 || t.cout != cout) continue;
            for (int cand : {t.cfg, t.alt, t.alt2}) {
                ConvConfig cc;
                if (cand >= 0 && find_cfg(cand, cc) == 0 && cfg_valid(cc, ks, stride, c0, c1, cout, false, want_bf16) && tile_fit_ok(cc, Ho, Wo)) return cand;
            }
        }
    }
    if (want_bf16 != Bf16Mode::None && !fused_first) {   // bf16 tilings first; fall back to fp32 where none fits (e.g. Cout = 16 with fp32 storage)
        const int forced_bf = override_cfg(layer);
        double best = 1e300; int best_id = -1;
        for (int i = 0; i < num_conv_configs(); ++i) {
            const ConvConfig &c = conv_config(i);
            if (!cfg_valid(c, ks, stride, c0, c1, cout, false, want_bf16)) continue;
            if (c.id == forced_bf) return c.id;
            const int npb = (c.th * c.tw + c.mb - 1) / c.mb, pbw = (npb + c.wn - 1) / c.wn;
            const double cost = (double)map_tiles(c, Ho, Wo) * (packed_cout(c, cout) / cout_per_item(c)) * pbw * c.cb;
            if (cost < best) { best = cost; best_id = c.id; }
        }
        if (best_id >= 0) return best_id;
        if (want_bf16 == Bf16Mode::Storage) return -1;   // bf16 storage has no fp32 fallback
    }
    const int forced = override_cfg(layer);
    if (forced >= 0) {
        for (int i = 0; i < num_conv_configs(); ++i)
            if (conv_config(i).id == forced && cfg_valid(conv_config(i), ks, stride, c0, c1, cout, fused_first)) return forced;
    }
    if (fused_first && wino_first && want_bf16 == Bf16Mode::None) {
        // conv0_1 as Winograd F(2x2) behind the fused first layer (kernels_conv.hip, conv_pc_kernel WINO): 64 MFMAs per consumer wave and
        // 16 x 16 tile instead of the direct form's 144, so even at 60-70 % tile fill it issues less than any direct tiling at 100 %
        ConvConfig cw;
        if (find_cfg(134, cw) == 0 && cfg_valid(cw, ks, stride, c0, c1, cout, true)) return 134;
    }
    if (!fused_first && c1 == 0) {
        const bool small = small_batch_tilings() && N <= SMALL_BATCH;
        const Tuned *tab = small ? g_tuned_small : g_tuned_large;
        const size_t ntab = small ? sizeof(g_tuned_small) / sizeof(Tuned) : sizeof(g_tuned_large) / sizeof(Tuned);
        for (size_t j = 0; j < ntab; ++j) {
            const Tuned &t = tab[j];
            if (t.ks == ks && t.stride == stride && t.cin == c0 && t.cout == cout) {
                const int cand[4] = {t.cfg, t.alt, t.alt2, t.alt3};
                int first_ok = -1;
                for (int k = 0; k < 4; ++k) {
                    ConvConfig cc;
                    if (cand[k] < 0 || find_cfg(cand[k], cc) || !cfg_valid(cc, ks, stride, c0, c1, cout) || !tile_fit_ok(cc, Ho, Wo)) continue;
                    // F(2x4) on 32-channel layers pays only where its 8 x 32 regions fill the map (U-Net 128 x 128: 177 -> 150 us; FCN 96 x 104: 81 %
                    // fill against 100 % of the 16 x 8 F(2x2) regions, no gain)
                    if (cand[k] == 307 && (Ho % 8 || Wo % 32)) continue;
                    if (Ho % cc.th == 0 && Wo % cc.tw == 0) return cand[k];      // tiles divide the map: straight-line producer applies
                    if (first_ok < 0) first_ok = cand[k];
                }
                if (first_ok >= 0) return first_ok;
            }
        }
    }
    if (!fused_first && c1 > 0 && ks == 3 && stride == 1 && cout == 32) {
        // skip-concat conv of the U-Net's level 1 (network_ao.py:51-53, 32 + 32 -> 32): the two-source Winograd kernel in its
        // 32-channel form (r02 sweep at 256x256, N = 100: 345 us against 544 for the best direct tiling)
        ConvConfig cw;
        if (Ho % 8 == 0 && Wo % 32 == 0 && find_cfg(307, cw) == 0 && cfg_valid(cw, ks, stride, c0, c1, cout)) return 307;   // F(2x4): 321 -> 252 us (r04)
        if (find_cfg(301, cw) == 0 && cfg_valid(cw, ks, stride, c0, c1, cout) && tile_fit_ok(cw, Ho, Wo)) return 301;
    }
    double best = 1e300;
    int best_id = -1;
    for (int i = 0; i < num_conv_configs(); ++i) {
        const ConvConfig &c = conv_config(i);
        if (c.id == 306 || c.family == ConvFamily::FirstWino22 || !cfg_valid(c, ks, stride, c0, c1, cout, fused_first)) continue;
        const int npb = (c.th * c.tw + c.mb - 1) / c.mb;
        const int pbw = (npb + c.wn - 1) / c.wn;
        // matrix-pipe cycles per wave x workgroups = padded work (tile overhang + block rounding)
        double cyc = (double)pbw * c.cb * (ks * ks * (c0 + c1) / (c.mb == 32 ? 2 : 4)) * (c.mb == 32 ? 64 : 32);
        // Winograd: one stage (16 input channels of one 8x16 region, 64 output channels) costs ~5.2k cycles
        // per CU measured; 5800 puts it on the scale of the direct estimate above (which ignores the direct
        // kernels' ~70 % matrix-pipe efficiency), calibrated on the three tuned shapes.
        if (is_wino(c)) cyc = ((c0 + c1) / 16) * (is_wino24(c) ? (c.tw == 32 ? 9300.0 : 4700.0) : c.wm == 4 ? 5800.0 : 3500.0);   // F(2x4): 256 / 128 pixels per stage
        double cost = (double)map_tiles(c, Ho, Wo) * (cout / cout_per_item(c)) * cyc;
        int rank = 12;
        for (int r = 0; r < (int)(sizeof(g_pref) / sizeof(g_pref[0])); ++r)
            if (g_pref[r] == c.id) { rank = r % 6; break; }
        cost *= 1.0 + 0.04 * rank;
        if (cost < best) { best = cost; best_id = c.id; }
    }
    return best_id;
}

// ---- conv_x3 plans (UKBB_PREC_F32X3 + ukbb_fcn_set_f32x3_convs) ----
// The layers such a plan runs on ConvFamily::F32x3Operands: every single-source 3x3 conv behind the stem with whole 16-channel chunks in
// and whole 32-row blocks out -- conv1_0 .. conv4_2 of the FCN graph.
bool x3_layer(const PlanMode &m, int ks, int c0, int c1, int cout, bool fused_first) {
    return m.conv_x3 && ks == 3 && !fused_first && c1 == 0 && c0 >= 16 && c0 % 16 == 0 && cout % 32 == 0;
}
// ONE table for every batch size (the plan must not depend on the batch): per layer type the tilings in order of preference among equals.
// 12 x 13 tiles divide the 192 x 208 pyramid, 11 x 13 the long-axis models' 176 x 208, 8 x 16 power-of-two maps.  Measured per kernel at
// N = 64 x 192 x 208 (profiles/f32x3_convs.txt): what a launch costs follows the 32-pixel MFMA blocks it issues, idle wave slots included -- a
// 12 x 13 tile is 5 blocks in 6 slots (8 with four pixel waves), an 8 x 16 tile 4 in 4 -- so 8 x 16 wins level 1 outright (conv1_1 73 against
// 92 us, conv1_0 97 against 104) and 12 x 13 level 4 (75 against 89); where the counts tie (levels 2 and 3) the stride-1 layers were faster on
// 8 x 16 (75 / 72 against 85 / 80 us) and the stride-2 layers, whose halo is four times the tile, on 12 x 13 (68 / 61 against 72 / 62).
// 64 output channels per workgroup wherever the layer has them: with 32 a second workgroup fits the CU, and every layer was slower
// (conv2_1 87 against 85 us, conv2_0 93 against 68).
// Only those two pyramids were timed.  choose_x3_cfg decides by the block count alone, so on other shapes 12 x 13 and 11 x 13 are also taken
// on maps of several tiles with ragged edges (a 12 x 20 map: 12 slots against 16 for 8 x 16) and as single partial tiles: there the order
// among equals is an extrapolation of the measurement, not a measurement.
const Tuned g_tuned_x3[] = {
    {3, 2, 16, 32, 345, -1, -1},    {3, 1, 32, 32, 335, -1, -1},
    {3, 2, 32, 64, 342, 340, 344},  {3, 1, 64, 64, 334, 332, 330},
    {3, 2, 64, 128, 342, 340, 344}, {3, 1, 128, 128, 334, 332, 330},
    {3, 2, 128, 256, 342, 340, 344}, {3, 1, 256, 256, 334, 332, 330},
};
// Of the layer type's tilings the one that issues the fewest 32-pixel MFMA blocks over the map (tiles x block slots of a tile, the slots of
// waves a tile leaves idle included); the table's order among equals.  A layer type the table lacks: the same rule over every valid tiling
// of the family.
int choose_x3_cfg(const std::string &layer, int stride, int c0, int cout, int Ho, int Wo) {
    auto pick = [&](const std::vector<int> &cand) {
        int best = -1; long long best_slots = 0;
        for (int id : cand) {
            ConvConfig c;
            if (id < 0 || find_cfg(id, c) || !cfg_valid(c, 3, stride, c0, 0, cout, false, Bf16Mode::None, 0, true)) continue;
            const int npb = (c.th * c.tw + c.mb - 1) / c.mb, pbw = (npb + c.wn - 1) / c.wn;
            const long long slots = (long long)map_tiles(c, Ho, Wo) * pbw * c.wn;
            if (best < 0 || slots < best_slots) { best = id; best_slots = slots; }
        }
        return best;
    };
    const int forced = pick({override_cfg(layer)});     // UKBB_CONV_CFG, where it names a tiling of the family that is valid for the layer
    if (forced >= 0) return forced;
    for (const Tuned &t : g_tuned_x3)
        if (t.stride == stride && t.cin == c0 && t.cout == cout) return pick({t.cfg, t.alt, t.alt2});
    std::vector<int> all;
    for (int i = 0; i < num_conv_configs(); ++i) all.push_back(conv_config(i).id);
    return pick(all);
}

// bf16 storage: the fused variants of the level-0 tilings (ConvConfig::fuse: 1 = first layer in the staging, 2 = logits in the
// epilogue), first fit in measured order; -1 if none fits (the plan then keeps that layer as a launch of its own).
int pick_fused_bf_cfg(const std::string &lname, int ks, int stride, int c0, int c1, int cout, int Ho, int Wo, int fuse_bf) {
    const int forced = override_cfg(lname);
    // fused logits: the persistent kernel first (kernels_bf16.hip: 104-110 vs 124 us), then the tile-per-workgroup tilings in
    // measured order; fused first layer: tile-per-workgroup only (its persistent form was no faster, r03_notes.md)
    for (int cand : {forced, fuse_bf == 1 ? 296 : 404, fuse_bf == 1 ? 294 : 325, fuse_bf == 1 ? 295 : 324, fuse_bf == 1 ? -1 : 298, fuse_bf == 1 ? -1 : 297, fuse_bf == 1 ? -1 : 299}) {
        ConvConfig cc;
        if (cand >= 0 && find_cfg(cand, cc) == 0 && cfg_valid(cc, ks, stride, c0, c1, cout, false, Bf16Mode::Storage, fuse_bf) &&
            (cand == forced || tile_fit_ok(cc, Ho, Wo))) return cand;
    }
    return -1;
}

// Region width (32 | 16 columns) of the fused ConvLSTM gate-conv / cell kernel (kernels_wino24.hip) for a plan built for batches of N
// on a device of `cus` compute units; 0 when the F(2x4) kernel does not apply.  Both shapes give identical bits; the choice sizes the
// tile-padded gx / cell-state buffers, so it is part of the plan (PlanLayout::lstm_tile_cols).
int lstm_region_cols(const ukbb_fcn_arch &a, int H, int W, int N, int cus) {
    int cfg = choose_cfg_raw("lstm_fw", 3, 1, a.n_filter[0], a.same_dim, 4 * a.same_dim, H, W, N, false, Bf16Mode::None, false);
    if (override_cfg("lstm_fw") < 0) cfg = pick_wino24(cfg, 3, 1, a.n_filter[0], a.same_dim, 4 * a.same_dim, H, W, N, cus);
    ConvConfig c;
    const bool have24 = cfg >= 0 && !find_cfg(cfg, c) && is_wino24(c) && c.wm == 4 && (c.tw == 32 || c.tw == 16);
    return have24 ? c.tw : 0;
}

// ---- plan ------------------------------------------------------------------------
// The A/B knobs of the plan, gathered.  Those read at every plan build can be toggled inside one process by re-planning
// (tools/check_tail.py and the like do); the `static const` ones are read once per process.
struct Knobs {
    bool no_fuse_first, no_fuse_logits, sqg1_separate;                   // once per process
    bool side_stream, no_fuse_stem, no_fuse_tail, lstm_bf_wino, lstm_bf_unhoist;
    const char *lstm_tile_cols, *split_from, *split_op, *debug_ops;
};

Knobs read_knobs() {
    static const bool no_fuse_first = getenv("UKBB_NO_FUSE_FIRST") != nullptr;
    static const bool no_fuse_logits = getenv("UKBB_NO_FUSE_LOGITS") != nullptr;
    static const bool sqg1_separate = getenv("UKBB_SQG1_SEPARATE") != nullptr;     // level-1 squeeze as a launch of its own
    Knobs k;
    k.no_fuse_first = no_fuse_first; k.no_fuse_logits = no_fuse_logits; k.sqg1_separate = sqg1_separate;
    // r01 measurement: running sqg_l concurrently with the deeper convs made the step 9 % SLOWER (1.88 vs 1.72 ms: the sqg waves take
    // SIMD slots and L2 bandwidth from the MFMA-bound persistent conv kernels), so the fork/join path is off unless UKBB_SIDE_STREAM is set.
    k.side_stream = getenv("UKBB_SIDE_STREAM") != nullptr;
    k.no_fuse_stem = getenv("UKBB_NO_FUSE_STEM") != nullptr;             // the r03 form: conv0_0 evaluated in conv0_1's staging
    k.no_fuse_tail = getenv("UKBB_NO_FUSE_TAIL") != nullptr;             // up0_0, up0_1 and the logits as separate launches
    k.lstm_bf_wino = getenv("UKBB_LSTM_BF16_WINOGRAD") != nullptr;
    // r06 experiment, measured and NOT the default: UKBB_LSTM_BF16_UNHOIST=1 makes the bf16 time steps re-multiply x instead of reading the hoisted gx
    // (320 -> 224 bytes per pixel and step).  100-frame 256x256 cine, three alternating rounds + rocprofv3 (profiles/r06_ab_lstm_unhoist.txt): step
    // 354.8 -> 372.1 us, x pass 754 -> 636 us, cine 8.17 -> 8.31 ms: the step is not bound by its bytes alone -- the second chunk's staging and MFMAs
    // cost more issue time than the gx loads they replace.  The hoisted form (r05) stays.
    k.lstm_bf_unhoist = getenv("UKBB_LSTM_BF16_UNHOIST") != nullptr;
    k.lstm_tile_cols = getenv("UKBB_LSTM_TILE_COLS");                    // 16 | 32 (identical bits)
    k.split_from = getenv("UKBB_SPLIT_FROM");
    k.split_op = getenv("UKBB_SPLIT_OP");
    k.debug_ops = getenv("UKBB_DEBUG_OPS");
    return k;
}

struct Planner {               // what the plan_* helpers below share
    const ukbb_fcn_arch &a;
    const int n_hint, cus;
    PlanLayout &L;                   // L.mode is set before any helper runs
    std::vector<Spec> specs;

    int layer(const std::string &name) const {
        for (size_t i = 0; i < specs.size(); ++i)
            if (specs[i].name == name) return (int)i;
        return -1;
    }
    int new_act(const std::string &name, size_t per_image, int channels = 0) {
        L.acts.push_back({name, per_image, channels, L.mode.bfio() && channels > 0 ? 2 : 4});      // bf16 storage: the channel maps
        return (int)L.acts.size() - 1;
    }
};

int plan_conv(Planner &p, const std::string &lname, int in0, int in1, int c1, int H, int W, int stride, int *out_buf,
              bool fused_first = false, bool fused_logits = false) {
    const int li = p.layer(lname);
    const Spec &L = p.specs[li];
    Op op;
    op.kind = OP_CONV; op.name = lname; op.layer = li; op.in0 = in0; op.in1 = in1;
    op.H = H; op.W = W; op.stride = stride;
    op.Ho = (H + stride - 1) / stride; op.Wo = (W + stride - 1) / stride;
    // TF 'SAME' pad_before
    op.pad_y = std::max((op.Ho - 1) * stride + L.ks - H, 0) / 2;
    op.pad_x = std::max((op.Wo - 1) * stride + L.ks - W, 0) / 2;
    const int c0 = L.cin - c1;
    op.fused_first = fused_first;
    const int fuse_bf = !p.L.mode.bfio() ? 0 : fused_first ? 1 : fused_logits ? 2 : 0;
    // the Winograd form of the fused first layer (134) was measured on, and is taken by, the fp32 FCN plans only (UKBB_PREC_F32X3 included:
    // its convs are fp32); the U-Net / UNet-LSTM plans and the bf16-operand FCN plans keep the direct fused kernel (130-133)
    const bool wino_first = fused_first && p.a.kind == UKBB_KIND_FCN && p.L.mode.bf16 == Bf16Mode::None;
    const bool x3 = x3_layer(p.L.mode, L.ks, c0, c1, L.cout, fused_first);
    if (fuse_bf) op.cfg = pick_fused_bf_cfg(lname, L.ks, stride, c0, c1, L.cout, op.Ho, op.Wo, fuse_bf);
    else if (x3) op.cfg = choose_x3_cfg(lname, stride, c0, L.cout, op.Ho, op.Wo);
    else op.cfg = choose_cfg(lname, L.ks, stride, c0, c1, L.cout, op.Ho, op.Wo, p.n_hint, p.cus, fused_first, p.L.mode.bf16, wino_first);
    op.fused_logits = fuse_bf == 2;
    if (op.cfg < 0) { set_error("no conv tiling for layer %s (ks %d stride %d cin %d+%d cout %d)", lname.c_str(), L.ks, stride, c0, c1, L.cout); return UKBB_EARCH; }
    ConvConfig c;
    find_cfg(op.cfg, c);
    op.out = p.new_act(lname, (size_t)op.Ho * op.Wo * L.cout, L.cout);
    op.macs_per_image = (double)op.Ho * op.Wo * L.ks * L.ks * L.cin * L.cout;
    const double tiles = map_tiles(c, op.Ho, op.Wo);
    if (is_wino24(c)) {
        op.mfma_macs_per_image = op.macs_per_image * (24.0 / 72.0);   // F(2x4,3x3): 24 products per 8 outputs
        op.padded_macs_per_image = tiles * c.tw * 24.0 * L.cin * L.cout;      // every 8-row region issues all its tile slots (c.tw / 4 x 4)
    } else if (is_wino(c)) {
        op.mfma_macs_per_image = op.macs_per_image * (16.0 / 36.0);   // F(2x2,3x3): 16 products per 4 outputs
        // what the kernel ISSUES: every region runs two MFMA column blocks of 16 tile slots (one for a region whose lower half lies below
        // the map in the 64-channel form, kernels_wino.hip `half`), whatever part of its 4 x 8 (8 x 4) tiles the map fills
        const int trY = c.th / 2, trX = 32 / trY;        // tiles per region along y / x
        const int regs_y = (op.Ho + 2 * trY - 1) / (2 * trY), regs_x = (op.Wo + 2 * trX - 1) / (2 * trX);
        double slots = 0;
        for (int ry = 0; ry < regs_y; ++ry) slots += (double)regs_x * ((c.wm == 4 && ry * 2 * trY + trY >= op.Ho) ? 16 : 32);
        op.padded_macs_per_image = slots * 16.0 * L.cin * L.cout;
    } else if (c.family == ConvFamily::FirstWino22) {
        // what the kernel issues: conv0_1 as F(2x2) (16 products per 4 outputs) + conv0_0 on the producers' MFMAs (K = 9 taps of 12
        // issued: three 16x16x4 per 16 halo pixels of every 18 x 18 halo tile)
        const double halo_blocks = (double)(((c.th + 2) * (c.tw + 2) + 15) / 16);
        const double first_macs = (double)op.Ho * op.Wo * 9 * L.cin;   // conv0_0: 1 -> L.cin channels
        op.mfma_macs_per_image = op.macs_per_image * (16.0 / 36.0) + first_macs;
        op.padded_macs_per_image = tiles * ((c.th / 2) * (c.tw / 2) * 16.0 * L.cin * L.cout + halo_blocks * 16 * 12 * L.cin);
    } else if (c.family == ConvFamily::F32x3Operands) {  // six bf16 products per fp32 one, over tiles x 32-pixel blocks
        const int npb = (c.th * c.tw + c.mb - 1) / c.mb;
        op.mfma_macs_per_image = 6.0 * op.macs_per_image;
        op.padded_macs_per_image = 6.0 * tiles * npb * c.mb * L.ks * L.ks * (double)L.cin * L.cout;
    } else if (!packs_bf16(c)) {                       // direct fp32 tilings: tiles x pixel blocks of the MFMA's N width
        const int npb = (c.th * c.tw + c.mb - 1) / c.mb;
        op.padded_macs_per_image = tiles * npb * c.mb * L.ks * L.ks * (double)L.cin * L.cout;
    } else if (fused_first) {
        op.mfma_macs_per_image = op.macs_per_image;              // conv0_0 itself runs on the vector ALU
    }
    p.L.ops.push_back(op);
    *out_buf = op.out;
    return UKBB_OK;
}

// conv2d_transpose 3x3 s2 + BN + ReLU as a 2x2 sub-pixel conv (pack.h, tconv_as_conv2x2)
int plan_tconv(Planner &p, const std::string &lname, int in0, int H, int W, int *out_buf) {
    const int li = p.layer(lname);
    const Spec &L = p.specs[li];
    Op op;
    op.kind = OP_TCONV; op.name = lname; op.layer = li; op.in0 = in0;
    op.H = H; op.W = W; op.Ho = H; op.Wo = W; op.stride = 1; op.pad_y = 1; op.pad_x = 1;
    op.cfg = choose_cfg(lname, 2, 1, L.cin, 0, 4 * L.cout, H, W, p.n_hint, p.cus, false, p.L.mode.bf16);
    if (op.cfg < 0) { set_error("no tiling for transposed conv %s", lname.c_str()); return UKBB_EARCH; }
    op.out = p.new_act(lname, (size_t)4 * H * W * L.cout, L.cout);
    op.macs_per_image = (double)H * W * 9 * L.cin * L.cout;
    p.L.ops.push_back(op);
    *out_buf = op.out;
    return UKBB_OK;
}

// ---- Temporal-UNet (kind 3): network_ao.py:67-114 on kernels_conv3d.hip (fp32) / kernels_conv3d_bf16.hip (UKBB_PREC_BF16_3D: the same ops and tiling) -------------------------------------------
int plan_conv3d(Planner &p, const std::string &lname, int in0, int in1, int H, int W, int stride, int *out_buf) {
    const int li = p.layer(lname);
    const Spec &L = p.specs[li];
    Op op;
    op.kind = L.cin == 1 ? OP_FIRST3D : OP_CONV3D; op.name = lname; op.layer = li; op.in0 = in0; op.in1 = in1;
    op.H = H; op.W = W; op.stride = stride;
    op.Ho = (H + stride - 1) / stride; op.Wo = (W + stride - 1) / stride;
    op.pad_y = std::max((op.Ho - 1) * stride + 3 - H, 0) / 2;          // TF 'SAME' pad_before
    op.pad_x = std::max((op.Wo - 1) * stride + 3 - W, 0) / 2;
    if (op.kind == OP_FIRST3D && (stride != 1 || L.cout != 16)) { set_error("%s: the first 3-D layer must be 1 -> 16 channels, stride 1", lname.c_str()); return UKBB_EARCH; }
    op.out = p.new_act(lname, (size_t)op.Ho * op.Wo * L.cout, L.cout);
    op.macs_per_image = (double)op.Ho * op.Wo * 27 * L.cin * L.cout;
    // issued: the window's first and last frame skip one time tap (3T - 2 of 3T); the first layer runs on the vector ALU
    const double tfrac = (3.0 * p.a.fc - 2) / (3.0 * p.a.fc);
    op.mfma_macs_per_image = op.kind == OP_FIRST3D ? 0.0 : op.macs_per_image * tfrac;
    if (op.kind == OP_CONV3D)                                          // ... in 32-pixel tiles x 32-row channel blocks
        op.padded_macs_per_image = (double)((op.Ho * op.Wo + 31) / 32) * 32 * 27 * L.cin * round_up(L.cout, 32) * tfrac;
    p.L.ops.push_back(op);
    *out_buf = op.out;
    return UKBB_OK;
}

int plan_tconv3d(Planner &p, const std::string &lname, int in0, int H, int W, int *out_buf) {
    const int li = p.layer(lname);
    const Spec &L = p.specs[li];
    Op op;
    op.kind = OP_TCONV3D; op.name = lname; op.layer = li; op.in0 = in0;
    op.H = H; op.W = W; op.Ho = 2 * H; op.Wo = 2 * W; op.stride = 1;
    op.out = p.new_act(lname, (size_t)op.Ho * op.Wo * L.cout, L.cout);
    op.macs_per_image = (double)H * W * 27 * L.cin * L.cout;           // 27 taps per INPUT pixel
    const double tfrac = (3.0 * p.a.fc - 2) / (3.0 * p.a.fc);          // window-edge frames skip one time tap
    op.mfma_macs_per_image = op.macs_per_image * tfrac;
    op.padded_macs_per_image = (double)((H * W + 31) / 32) * 32 * 27 * L.cin * round_up(L.cout, 32) * tfrac;
    p.L.ops.push_back(op);
    *out_buf = op.out;
    return UKBB_OK;
}

// the Temporal-UNet plan: encoder, decoder (transposed conv, concat([skip, up]), convs), conv_out + softmax / argmax (network_ao.py:67-114)
int layout_t3d(Planner &p, int H, int W) {
    const ukbb_fcn_arch &a = p.a;
    char nm[64];
    int cur = -1, hh = H, ww = W;
    std::vector<int> level_out(a.n_level), lh(a.n_level), lw(a.n_level);
    for (int l = 0; l < a.n_level; ++l) {
        for (int i = 0; i < a.n_block[l]; ++i) {
            snprintf(nm, sizeof nm, "conv%d_%d", l, i);
            const int stride = (l > 0 && i == 0) ? 2 : 1;
            int rc = plan_conv3d(p, nm, cur, -1, hh, ww, stride, &cur);
            if (rc) return rc;
            hh = (hh + stride - 1) / stride; ww = (ww + stride - 1) / stride;
        }
        level_out[l] = cur; lh[l] = hh; lw[l] = ww;
    }
    for (int l = a.n_level - 2; l >= 0; --l) {
        snprintf(nm, sizeof nm, "up%d_t", l);
        int up = -1;
        int rc = plan_tconv3d(p, nm, cur, lh[l + 1], lw[l + 1], &up);
        if (rc) return rc;
        cur = up;
        for (int i = 0; i < a.n_block[l]; ++i) {
            snprintf(nm, sizeof nm, "up%d_%d", l, i);
            rc = i == 0 ? plan_conv3d(p, nm, level_out[l], up, lh[l], lw[l], 1, &cur)    // concat([skip, up]) (network_ao.py:51 order)
                        : plan_conv3d(p, nm, cur, -1, lh[l], lw[l], 1, &cur);
            if (rc) return rc;
        }
    }
    Op lg;
    lg.kind = OP_LOGITS; lg.name = "logits"; lg.layer = p.layer("logits"); lg.in0 = cur; lg.H = H; lg.W = W;
    lg.macs_per_image = (double)H * W * a.n_filter[0] * a.n_class;
    lg.mfma_macs_per_image = 0.0;
    p.L.ops.push_back(lg);
    return UKBB_OK;
}

// encoder (network.py:179-189 / network_ao.py:31-41) with the FCN's squeeze launches; fills the level outputs and sizes
int layout_encoder(Planner &p, const Knobs &k, int H, int W, std::vector<int> &level_out, std::vector<int> &lh, std::vector<int> &lw,
                   std::vector<int> &sqg_out) {
    const ukbb_fcn_arch &a = p.a;
    PlanLayout &L = p.L;
    char nm[64];
    const bool std0 = a.n_block[0] >= 2 && a.n_filter[0] == 16;
    // conv0_0 evaluated inside conv0_1's producers; bf16 storage: only if a fused tiling fits conv0_1 at this size (otherwise conv0_0
    // runs as its own launch, bf16 out)
    const bool can_fuse = !k.no_fuse_first && std0 && (!p.L.mode.bfio() || pick_fused_bf_cfg("conv0_1", 3, 1, 16, 0, 16, H, W, 1) >= 0);
    // bf16 storage with the standard 1 -> 16 -> 16 stem: conv0_0 and conv0_1 as ONE launch of kernels_stem.hip
    const bool stem = p.L.mode.bfio() && !k.no_fuse_stem && std0 && override_cfg("conv0_1") < 0;
    // levels 1-4 of the standard filter pyramid go out as ONE launch after level 4 (sqg_multi_kernel)
    const bool merge = !k.side_stream && a.n_level == 5 && a.n_filter[1] == 32 && a.n_filter[2] == 64 && a.n_filter[3] == 128 && a.n_filter[4] == 256;
    int cur = -1, hh = H, ww = W;
    Op multi;
    multi.kind = OP_FIRST;                         // becomes OP_SQG_MULTI when the first merged level arrives
    for (int l = 0; l < a.n_level; ++l) {
        for (int i = 0; i < a.n_block[l]; ++i) {
            snprintf(nm, sizeof nm, "conv%d_%d", l, i);
            const int stride = (l > 0 && i == 0) ? 2 : 1;
            if (l == 0 && i == 0 && (stem || can_fuse)) continue;
            if (l == 0 && i == 1 && stem) {
                const int l0 = p.layer("conv0_0"), l1 = p.layer("conv0_1");
                const Spec &L0 = p.specs[l0], &L1 = p.specs[l1];
                Op op; op.kind = OP_STEM; op.name = "conv0_0+conv0_1"; op.layer = l1;
                op.H = op.Ho = H; op.W = op.Wo = W;
                op.out = p.new_act("conv0_1", (size_t)H * W * L1.cout, L1.cout);
                op.macs_per_image = (double)H * W * 9 * (L0.cin * L0.cout + L1.cin * L1.cout);
                L.ops.push_back(op);
                cur = op.out;
            } else if (l == 0 && i == 0) {
                Op op; op.kind = OP_FIRST; op.name = nm; op.layer = p.layer(nm);
                op.H = op.Ho = H; op.W = op.Wo = W;
                op.out = p.new_act(nm, (size_t)H * W * a.n_filter[0], a.n_filter[0]);
                op.macs_per_image = (double)H * W * 9 * a.n_filter[0];
                op.mfma_macs_per_image = 0;          // vector ALU kernel
                L.ops.push_back(op);
                cur = op.out;
            } else {
                const bool fused = (l == 0 && i == 1 && can_fuse);
                int rc = plan_conv(p, nm, cur, -1, 0, hh, ww, stride, &cur, fused);
                if (rc) return rc;
                if (fused) {
                    L.ops.back().name = "conv0_0+conv0_1";
                    L.ops.back().macs_per_image += (double)H * W * 9 * a.n_filter[0];
                }
                if (stride == 2) { hh = (hh + 1) / 2; ww = (ww + 1) / 2; }
            }
        }
        level_out[l] = cur; lh[l] = hh; lw[l] = ww;
        L.acts[cur].name = std::string("conv") + std::to_string(l);
        if (a.kind == UKBB_KIND_FCN && l >= 1) {
            // same_dim_l + out0's level-l slice at low resolution (same_dim0 lives inside the head kernel).
            // Emitted right after its level and run on the side stream: it only feeds the head, is
            // memory-bound, and overlaps with the MFMA-bound convs of the deeper levels.
            snprintf(nm, sizeof nm, "same_dim%d", l);
            Op op; op.kind = OP_SQG; op.name = std::string("sqg") + std::to_string(l);
            op.layer = p.layer(nm); op.in0 = level_out[l];
            op.H = op.Ho = lh[l]; op.W = op.Wo = lw[l]; op.stride = l;
            op.on_side = k.side_stream;
            op.out = p.new_act(std::string("g") + std::to_string(l), (size_t)lh[l] * lw[l] * a.fc);
            // algorithmic MACs: the squeeze; the 32->64 projection is out0's work moved to low
            // resolution and is accounted to the head (so the per-layer sums equal Appendix A)
            op.macs_per_image = (double)lh[l] * lw[l] * a.n_filter[l] * a.same_dim;
            op.mfma_macs_per_image = (double)lh[l] * lw[l] * (a.n_filter[l] * a.same_dim + a.same_dim * a.fc);
            sqg_out[l] = op.out;
            if (merge && !(k.sqg1_separate && l == 1)) {
                if (multi.kind != OP_SQG_MULTI) { multi = Op(); multi.kind = OP_SQG_MULTI; multi.name = k.sqg1_separate ? "sqg2-4" : "sqg1-4"; multi.macs_per_image = 0; multi.mfma_macs_per_image = 0; }
                multi.mlayer[l - 1] = op.layer; multi.min_[l - 1] = op.in0; multi.mout[l - 1] = op.out;
                multi.mh[l - 1] = lh[l]; multi.mw[l - 1] = lw[l];
                multi.macs_per_image += op.macs_per_image; multi.mfma_macs_per_image += op.mfma_macs_per_image;
                if (l == 4) L.ops.push_back(multi);
            } else {
                L.ops.push_back(op);
            }
        }
    }
    return UKBB_OK;
}

// decoder (network_ao.py:44-55): transposed conv, concat [skip, up] (two-source conv), convs; then the logits in whichever form the plan has
int layout_decoder(Planner &p, const Knobs &k, int H, int W, const std::vector<int> &level_out, const std::vector<int> &lh, const std::vector<int> &lw) {
    const ukbb_fcn_arch &a = p.a;
    PlanLayout &L = p.L;
    char nm[64];
    // bf16 storage, level 0 with the standard two 16-channel convs: up0_0, up0_1, logits and softmax / argmax as ONE launch (kernels_tail.hip)
    const bool tail = a.kind == UKBB_KIND_UNET && p.L.mode.bfio() && !k.no_fuse_tail && a.n_block[0] == 2 && a.n_filter[0] == 16 &&
                      a.n_class >= 2 && a.n_class <= 4 && override_cfg("up0_0") < 0 && override_cfg("up0_1") < 0;
    int up = level_out[a.n_level - 1];
    for (int l = a.n_level - 2; l >= 0; --l) {
        snprintf(nm, sizeof nm, "up%d_t", l);
        int t;
        int rc = plan_tconv(p, nm, up, lh[l + 1], lw[l + 1], &t);
        if (rc) return rc;
        if (l == 0 && tail) {
            const int l0 = p.layer("up0_0");
            const Spec &L0 = p.specs[l0], &L1 = p.specs[p.layer("up0_1")];
            Op op; op.kind = OP_TAIL; op.name = "up0_0+up0_1+logits"; op.layer = l0; op.in0 = level_out[0]; op.in1 = t;
            op.H = op.Ho = lh[0]; op.W = op.Wo = lw[0];
            op.macs_per_image = (double)lh[0] * lw[0] * (9.0 * L0.cin * L0.cout + 9.0 * L1.cin * L1.cout + (double)a.n_filter[0] * a.n_class);
            L.ops.push_back(op);
            return UKBB_OK;                            // logits, softmax / argmax are part of the fused tail launch
        }
        int x = -1;
        for (int i = 0; i < a.n_block[l]; ++i) {
            snprintf(nm, sizeof nm, "up%d_%d", l, i);
            // bf16 storage: logits + softmax / argmax ride in the epilogue of the very last conv (its output is never stored)
            const bool flg = a.kind == UKBB_KIND_UNET && p.L.mode.bfio() && !k.no_fuse_logits && l == 0 && i == a.n_block[0] - 1 &&
                             i > 0 && a.n_filter[0] == 16 && pick_fused_bf_cfg(nm, 3, 1, 16, 0, 16, lh[0], lw[0], 2) >= 0;
            rc = (i == 0) ? plan_conv(p, nm, level_out[l], t, a.n_filter[l], lh[l], lw[l], 1, &x)
                          : plan_conv(p, nm, x, -1, 0, lh[l], lw[l], 1, &x, false, flg);
            if (rc) return rc;
        }
        up = x;
        L.acts[up].name = std::string("up") + std::to_string(l);
    }
    L.feat_buf = up;                              // net['conv0_up']: what UNet_LSTM_Model feeds the LSTM (:343-347)
    if (a.kind == UKBB_KIND_UNET && L.ops.back().fused_logits) {
        Op &last = L.ops.back();
        last.name += "+logits";
        last.macs_per_image += (double)H * W * a.n_filter[0] * a.n_class;
        L.acts[up].name = "";                     // net['conv0_up'] does not exist in HBM in this plan
    } else if (a.kind == UKBB_KIND_UNET) {
        Op op; op.kind = OP_LOGITS; op.name = "logits"; op.layer = p.layer("logits"); op.in0 = up;
        op.H = op.Ho = H; op.W = op.Wo = W;
        op.macs_per_image = (double)H * W * a.n_filter[0] * a.n_class;
        L.ops.push_back(op);
    } else {
        // ConvLSTM: region shape of the fused gate-conv / cell kernel, chosen once per plan (both shapes give identical bits)
        L.needs_lstm = true;
        L.lstm_bf_wino = k.lstm_bf_wino;
        L.lstm_bf_hoist = !k.lstm_bf_unhoist;
        const int cols24 = lstm_region_cols(a, H, W, p.n_hint, p.cus);
        // the bf16 plan's time steps run on launch_lstm_ws (kernels_ws.hip) and never touch the F(2x4) kernel: only the fp32 plan and the
        // bf16-storage Winograd A/B form need that tiling
        if (!cols24 && (!L.mode.bfio() || L.lstm_bf_wino)) {
            set_error("the ConvLSTM needs the Winograd F(2x4) kernel (unset UKBB_NO_WINOGRAD / UKBB_NO_WINOGRAD24 / UKBB_CONV_CFG overrides)");
            return UKBB_EARCH;
        }
        L.lstm_tile_cols = cols24 ? cols24 : 32;
        if (k.lstm_tile_cols) { const int v = atoi(k.lstm_tile_cols); if (v == 16 || v == 32) L.lstm_tile_cols = v; }
    }
    return UKBB_OK;
}

// r06: the levels >= k of a plan (U-Net: conv{k}_0 .. up{k}_1) run as two half-batch chains on two streams (run_plan), so that one half's
// fill / drain / serial chains hide under the other half's body.  Measured at N = 100 x 256x256 (profiles/r06_split_levels.txt and
// r06_split_after_fix.txt), labels bit-identical to the unsplit plan in every run: fp32 U-Net 4.02 -> 3.86 ms per forward with k = 1
// (+4 %; k = 2: 3.88, k = 3: 3.92, k = 4: no change), bf16-storage U-Net 1.042 -> 1.042 (nothing to hide once the walkers fill the chip),
// FCN 0.5-1 % slower.  So: ON from level 1 for a UKBB_KIND_UNET plan in fp32, off everywhere else; UKBB_SPLIT_FROM=k overrides (0 = off).
// (While this was first tried the 300-case bf16 sweep met sporadic wrong tiles with it; that was the wide-store hazard of kernels_ws.hip,
// store_b128_sofs there and profiles/r06_notes.md section 10 -- fixed, and the sweep is clean with the split forced on.)
void layout_split_range(const Planner &p, const Knobs &kn) {
    const ukbb_fcn_arch &a = p.a;
    PlanLayout &L = p.L;
    const int k = kn.split_from ? atoi(kn.split_from) : (a.kind == UKBB_KIND_UNET && p.L.mode.bf16 == Bf16Mode::None) ? 1 : 0;
    if (k >= 1 && k < a.n_level) {
        // U-Net: conv{k}_0 .. up{k}_1; FCN (no decoder): conv{k}_0 .. the last encoder conv (the squeeze launches and the head follow unsplit)
        const std::string c0 = "conv" + std::to_string(k) + "_0";
        const std::string u0 = a.kind == UKBB_KIND_FCN ? "conv" + std::to_string(a.n_level - 1) + "_" : "up" + std::to_string(k) + "_";
        for (size_t i = 0; i < L.ops.size(); ++i) {
            if (L.split_first < 0 && L.ops[i].name.compare(0, c0.size(), c0) == 0) L.split_first = (int)i;
            if (L.ops[i].name.compare(0, u0.size(), u0) == 0 && L.ops[i].kind != OP_TAIL) L.split_last = (int)i;
        }
        if (L.split_first < 0 || L.split_last < L.split_first) { L.split_first = -1; L.split_last = -2; }
    }
    if (kn.debug_ops) { int f = 0, l = 1 << 30; if (sscanf(kn.debug_ops, "%d,%d", &f, &l) >= 1) { L.debug_first_op = f; L.debug_last_op = l; } }
    if (kn.split_op) {                                 // debugging: ONLY op i runs as two half-batch launches on two streams
        const int i = atoi(kn.split_op);
        if (i >= 0 && i < (int)L.ops.size()) { L.split_first = i; L.split_last = i; }
    }
}

}  // namespace

int plan_mode(const ukbb_fcn_arch &a, int precision, PlanMode &m, const char **why) {
    m = PlanMode();
    *why = "";
    if (precision != UKBB_PREC_FP32 && precision != UKBB_PREC_BF16 && precision != UKBB_PREC_F32X3 && precision != UKBB_PREC_BF16_STORE && precision != UKBB_PREC_BF16_3D && precision != UKBB_PREC_BF16_FULL) { *why = "bad precision"; return UKBB_EINVAL; }
    if (a.kind == UKBB_KIND_TEMPORAL_UNET && precision == UKBB_PREC_BF16) { *why = "the Temporal-UNet's 3-D convolutions are built for fp32 only (no bf16 plan) under this code; their bf16 mode is UKBB_PREC_BF16_3D ('bf16_3d')"; return UKBB_EARCH; }
    if (a.kind == UKBB_KIND_TEMPORAL_UNET && precision == UKBB_PREC_BF16_STORE) { *why = "UKBB_PREC_BF16_STORE is the FCN's bf16-storage mode; the U-Net kinds already store bf16 under UKBB_PREC_BF16 (the Temporal-UNet: fp32 only under that code, bf16 under UKBB_PREC_BF16_3D, 'bf16_3d')"; return UKBB_EARCH; }
    if (a.kind != UKBB_KIND_FCN && precision == UKBB_PREC_BF16_STORE) { *why = "UKBB_PREC_BF16_STORE is the FCN's bf16-storage mode; the U-Net kinds already store bf16 under UKBB_PREC_BF16"; return UKBB_EARCH; }
    if (a.kind == UKBB_KIND_TEMPORAL_UNET && precision == UKBB_PREC_BF16_FULL) { *why = "UKBB_PREC_BF16_FULL is the FCN's bf16-storage mode with its head on the bf16 matrix instruction; the Temporal-UNet's bf16 mode is UKBB_PREC_BF16_3D ('bf16_3d')"; return UKBB_EARCH; }
    if (a.kind != UKBB_KIND_FCN && precision == UKBB_PREC_BF16_FULL) { *why = "UKBB_PREC_BF16_FULL is the FCN's bf16-storage mode with its head on the bf16 matrix instruction; the U-Net kinds have no such head and already store bf16 under UKBB_PREC_BF16"; return UKBB_EARCH; }
    if (a.kind != UKBB_KIND_TEMPORAL_UNET && precision == UKBB_PREC_BF16_3D) { *why = "UKBB_PREC_BF16_3D is the bf16 mode of the Temporal-UNet's 3-D convolutions; the 2-D kinds take UKBB_PREC_BF16 (the FCN also UKBB_PREC_BF16_STORE)"; return UKBB_EARCH; }
    // UKBB_PREC_BF16 means operands only on an FCN handle (pinned by recorded plans and graders) and storage on the U-Net kinds; with
    // UKBB_PREC_BF16_STORE the FCN encoder takes the same bf16-storage kernels (squeeze and head read the bf16 maps and stay fp32)
    if (precision == UKBB_PREC_BF16) m.bf16 = a.kind == UKBB_KIND_FCN ? Bf16Mode::Operands : Bf16Mode::Storage;
    if (precision == UKBB_PREC_BF16_STORE) m.bf16 = Bf16Mode::Storage;
    if (precision == UKBB_PREC_BF16_FULL) { m.bf16 = Bf16Mode::Storage; m.head_bf16 = true; }      // bf16_store's plan, the head launch on bf16 MFMA
    if (precision == UKBB_PREC_BF16_3D) m.bf16 = Bf16Mode::Storage;       // every 3-D map bf16, channel-blocked (kernels_conv3d_bf16.hip)
    m.head_x3 = precision == UKBB_PREC_F32X3;
    return UKBB_OK;
}

int layout_plan(const ukbb_fcn_arch &a, int precision, int H, int W, int n_hint, int cus, PlanLayout &L, bool f32x3_convs) {
    L = PlanLayout();
    const char *refused;
    if (const int rc = plan_mode(a, precision, L.mode, &refused)) { set_error("%s", refused); return rc; }
    L.mode.conv_x3 = f32x3_convs && L.mode.head_x3 && a.kind == UKBB_KIND_FCN;      // kept and ignored under any other precision
    Planner p{a, n_hint, cus, L, {}};
    std::string why;
    if (!arch_specs(a, p.specs)) { set_error("malformed architecture descriptor"); return UKBB_EARCH; }
    if (!supported(a, why)) { set_error("unsupported architecture: %s", why.c_str()); return UKBB_EARCH; }
    if (a.kind == UKBB_KIND_TEMPORAL_UNET) return layout_t3d(p, H, W);      // fp32 or UKBB_PREC_BF16_3D (the same ops on 2-byte maps), no split range, no knobs
    const Knobs k = read_knobs();
    std::vector<int> level_out(a.n_level), lh(a.n_level), lw(a.n_level), sqg_out(a.n_level, -1);
    int rc = layout_encoder(p, k, H, W, level_out, lh, lw, sqg_out);
    if (rc) return rc;
    if (a.kind == UKBB_KIND_FCN) {
        Op op; op.kind = OP_HEAD; op.name = "head"; op.in0 = level_out[0];
        op.H = op.Ho = H; op.W = op.Wo = W;
        op.macs_per_image = (double)H * W * (a.n_filter[0] * a.same_dim + a.same_dim * a.n_level * a.fc +
                                             a.fc * a.fc + a.fc * a.n_class);
        // matrix pipe: same_dim0, the level-0 slice of out0, out1 (the logits run on the vector ALU)
        op.mfma_macs_per_image = (double)H * W * (a.n_filter[0] * a.same_dim + a.same_dim * a.fc + a.fc * a.fc);
        for (int l = 1; l < 5; ++l) op.sq[l - 1] = sqg_out[l];
        L.ops.push_back(op);
    } else {
        rc = layout_decoder(p, k, H, W, level_out, lh, lw);
        if (rc) return rc;
    }
    layout_split_range(p, k);
    return UKBB_OK;
}

// ---- forward_cine scratch planner ---------------------------------------------------------------------
namespace {

size_t bytes_of(size_t elems, size_t esz) { return (elems * esz + 3) / 4 * 4; }      // a DevBuf of `elems` elements of esz bytes

uint64_t cine_table_bytes(int F, int T, int Wn) {        // lstm_aux / t3d_aux: window -> frame map, per-frame order, window weights, per-frame weight sums
    const size_t b_map = (size_t)T * Wn * sizeof(int), b_ord = (size_t)F * T * sizeof(int);
    const size_t off_ord = (b_map + 7) / 8 * 8, off_wk = (off_ord + b_ord + 7) / 8 * 8, off_ws = off_wk + T * sizeof(double);
    return (off_ws + F * sizeof(double) + 3) / 4 * 4;
}

// UNet-LSTM: bytes held with chunks of Wc windows whose longest run has R frames; stage = the contiguous copy of the run's input frames
uint64_t lstm_cine_bytes(const CineUnits &u, int F, int Wn, int R, int Wc, bool stage) {
    uint64_t b = (uint64_t)u.act_frame * R * 4;                                      // U-Net activations of R frames
    if (stage) b += (uint64_t)u.HW * R * 4;                                          // lstm_img
    b += bytes_of(2 * (size_t)R * u.gx_frame, u.esz);                                // lstm_gx
    b += (uint64_t)2 * R * u.c_item * 4;                                             // lstm_c1
    b += bytes_of(2 * (size_t)R * u.h_item, u.esz);                                  // lstm_h1
    b += (uint64_t)Wc * u.c_item * 4;                                                // lstm_c
    b += bytes_of(2 * (size_t)u.T * Wc * u.h_item, u.esz);                           // lstm_hall
    return b + cine_table_bytes(F, u.T, Wn);
}

constexpr double T3D_CHUNK_BYTES = 4.0e9;      // Temporal-UNet without a budget: the chunk's activations + window probabilities stay within this

}  // namespace

bool plan_cine(const CineUnits &u, int F, int time_step, uint64_t budget, CinePlan &pl) {
    const int T = u.T, Wn = (F + time_step - 1) / time_step;
    pl = CinePlan();
    pl.Wn = Wn;
    if (u.kind == UKBB_KIND_TEMPORAL_UNET) {
        const uint64_t per_window = (uint64_t)(u.act_frame * u.esz + u.HW * u.n_class * 4) * T, tables = cine_table_bytes(F, T, Wn);
        pl.min_bytes = per_window + tables;
        int Wc;
        if (!budget) Wc = std::max(1, (int)std::min<double>(Wn, T3D_CHUNK_BYTES / (double)per_window));
        else if (budget < pl.min_bytes) return false;
        else Wc = (int)std::min<uint64_t>(Wn, (budget - tables) / per_window);
        pl.Wc = Wc; pl.chunks = (Wn + Wc - 1) / Wc; pl.run = Wc * T;
        pl.bytes = (uint64_t)Wc * per_window + tables;
        return true;
    }
    // a chunk of n windows touches one circular run of (n - 1) * time_step + T frames (all F when that exceeds F)
    auto run_of = [&](int n) { return (int)std::min<long long>(F, (long long)(n - 1) * time_step + T); };
    const uint64_t whole = lstm_cine_bytes(u, F, Wn, F, Wn, false);
    pl.min_bytes = Wn > 1 ? std::min(whole, lstm_cine_bytes(u, F, Wn, run_of(1), 1, true)) : whole;
    if (!budget || budget >= whole) { pl.Wc = Wn; pl.chunks = 1; pl.run = F; pl.bytes = whole; return true; }
    if (budget < pl.min_bytes) return false;
    int lo = 1, hi = Wn - 1;                     // lstm_cine_bytes grows with Wc: the largest Wc < Wn that fits (Wc = 1 does, and Wn > 1 here)
    while (lo < hi) {
        const int mid = (lo + hi + 1) / 2;
        if (lstm_cine_bytes(u, F, Wn, run_of(mid), mid, true) <= budget) lo = mid; else hi = mid - 1;
    }
    pl.Wc = lo; pl.chunks = (Wn + lo - 1) / lo; pl.run = run_of(lo);
    pl.bytes = lstm_cine_bytes(u, F, Wn, pl.run, lo, true);
    return true;
}

CineUnits cine_units_from(const PlanLayout &L, const ukbb_fcn_arch &a, int H, int W) {
    CineUnits u;
    u.kind = a.kind; u.T = a.fc; u.n_class = a.n_class; u.HW = (size_t)H * W;
    for (const ActSpec &s : L.acts) u.act_frame += s.per_image;
    if (a.kind == UKBB_KIND_TEMPORAL_UNET) u.esz = L.mode.bfio() ? 2 : 4;       // UKBB_PREC_BF16_3D: the workspace holds what it stores (plan.h act_alloc_esz)
    if (a.kind != UKBB_KIND_UNET_LSTM) return u;
    const bool wsf = L.mode.bfio() && !L.lstm_bf_wino;       // the direct-conv bf16 ConvLSTM (kernels_ws.hip); else the F(2x4) kernel's regions
    u.esz = L.mode.bfio() ? 2 : 4;
    u.h_item = u.HW * a.same_dim;
    u.gx_frame = wsf ? lstm_ws_gx_elems(H, W) : wino24_lstm_gx_floats(H, W, L.lstm_tile_cols);
    u.c_item = wsf ? lstm_ws_c_floats(H, W) : wino24_lstm_c_floats(H, W, L.lstm_tile_cols);
    return u;
}

bool cine_request_ok(int T, int F, int H, int W, int time_step) {
    if (F < 1 || H < 16 || W < 16 || (H % 16) || (W % 16) || time_step < 1 || T < 1 || !(T & 1)) return false;
    if ((long long)F * H * W > (1ll << 31) - 1) return false;
    return F >= (T - 1) / 2;
}

}  // namespace ukbb
