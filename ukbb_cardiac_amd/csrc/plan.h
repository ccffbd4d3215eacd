// Host-only planner of the engine: which launches a forward consists of, the tiling each conv gets, the activation maps and their
// sizes, the MAC accounting and the chunk plan of forward_cine.  Pure arithmetic over (architecture, precision, H, W, batch, CU count,
// environment knobs): no HIP call, no handle, no weights.  engine.cpp materialises a PlanLayout on the device and runs it.
#pragma once
#include "../../include/ukbb_fcn.h"
#include "kernels.h"

#include <string>
#include <vector>

namespace ukbb {

// ---- architecture walk ---------------------------------------------------------
struct Spec { std::string name; int ks, cin, cout; bool bn, bias, transposed; int kd = 1; };

bool arch_specs(const ukbb_fcn_arch &a, std::vector<Spec> &out);     // the layers in the order of the flat weight array
size_t spec_floats(const Spec &s);
bool supported(const ukbb_fcn_arch &a, std::string &why);

// ---- the plan --------------------------------------------------------------------
enum OpKind { OP_FIRST, OP_CONV, OP_HEAD, OP_TCONV, OP_LOGITS, OP_SQG, OP_SQG_MULTI, OP_TAIL, OP_STEM,
              OP_FIRST3D, OP_CONV3D, OP_TCONV3D };   // ..._3D: the Temporal-UNet's 3-D convolutions (kernels_conv3d.hip)

struct Op {                    // one kernel launch of the plan
    OpKind kind;
    std::string name;
    int layer = -1;            // index into arch_specs / the handle's host layers (OP_FIRST/OP_CONV/OP_TCONV/OP_LOGITS)
    int cfg = -1;              // conv config id
    int in0 = -1, in1 = -1;    // activation buffer ids (-1: network input / none)
    int out = -1;
    int sq[4] = {-1, -1, -1, -1};   // OP_HEAD: squeezed maps of levels 1..4
    int mlayer[4] = {-1, -1, -1, -1}, min_[4] = {-1, -1, -1, -1}, mout[4] = {-1, -1, -1, -1}, mh[4] = {0, 0, 0, 0}, mw[4] = {0, 0, 0, 0};   // OP_SQG_MULTI: levels 1..4
    bool fused_first = false;       // OP_CONV: conv0_0 (C_in = 1) evaluated by this kernel's producers
    bool fused_logits = false;      // OP_CONV (bf16 storage): the 1x1 logits conv + softmax / argmax evaluated in this kernel's epilogue
    bool on_side = false;           // launched on the handle's side stream (fork/join by events)
    int H = 0, W = 0, Ho = 0, Wo = 0, stride = 1, pad_y = 0, pad_x = 0;
    double macs_per_image = 0; // algorithmic
    double mfma_macs_per_image = -1; // issued to the matrix pipe; -1 = same as algorithmic
    double padded_macs_per_image = -1;   // ... including the slots of partly filled tiles / Winograd regions; -1 = same as mfma_macs_per_image
};                             // plan data only: engine.cpp's BoundOp adds the device pointers a launch of it takes

struct ActSpec { std::string name; size_t per_image; int channels; int esz = 4; };   // per_image: elements per image; channels 0: not a channel map;
                                                                                       // esz: bytes of a stored element (2: bf16)
// Bytes the workspace holds per element of a map.  The U-Net kinds allocate every map as floats in either precision (CineUnits::act_frame
// and the recorded footprints count that); an FCN plan and a Temporal-UNet plan (fp32: 4, UKBB_PREC_BF16_3D: 2) allocate what they store.
inline size_t act_alloc_esz(const ukbb_fcn_arch &a, const ActSpec &s) { return a.kind == UKBB_KIND_FCN || a.kind == UKBB_KIND_TEMPORAL_UNET ? (size_t)s.esz : 4; }

// What a precision code means for a plan of one architecture.  Storage: bf16 operands AND every activation between layers bf16 in HBM
// (stores_bf16 tilings; an FCN plan: the encoder maps, G_l stays fp32; a UNet-LSTM keeps gx and the hidden maps in bf16 as well)
enum class Bf16Mode { None, Operands /* fp32 maps in HBM, ConvFamily::Bf16Operands */, Storage };
struct PlanMode {
    Bf16Mode bf16 = Bf16Mode::None;
    bool head_x3 = false;                     // UKBB_PREC_F32X3: the FCN head's out0 / out1 from three bf16 pieces per operand (its convs are fp32)
    bool head_bf16 = false;                   // UKBB_PREC_BF16_FULL: the FCN head's same_dim0 / out0 / out1 on the bf16 matrix instruction, one piece per operand
                                              // (the encoder and the squeeze launches are those of UKBB_PREC_BF16_STORE: bf16 == Storage)
    bool conv_x3 = false;                     // UKBB_PREC_F32X3 with ukbb_fcn_set_f32x3_convs on (FCN only): the 3x3 layers behind the stem on
                                              // ConvFamily::F32x3Operands as well; maps, squeeze launches, stem and head as in the f32x3 plan
    bool bfio() const { return bf16 == Bf16Mode::Storage; }
};
// THE list of precision codes and of the (kind, code) pairs the engine refuses.  UKBB_OK; UKBB_EINVAL for an unknown code; UKBB_EARCH
// for a refused pair, *why then the reason (callers put their own prefix in front of it).
int plan_mode(const ukbb_fcn_arch &a, int precision, PlanMode &m, const char **why);

struct PlanLayout {
    std::vector<Op> ops;
    std::vector<ActSpec> acts;
    int feat_buf = -1;                        // UNet-LSTM: activation index of net['conv0_up']
    PlanMode mode;
    int lstm_tile_cols = 0;                   // region shape of the fused gate-conv / cell kernel (kernels_wino24.hip): 32 | 16
    bool lstm_bf_wino = false;                // UKBB_LSTM_BF16_WINOGRAD: fp32 Winograd arithmetic on bf16 storage (A/B form)
    bool lstm_bf_hoist = true;                // false (UKBB_LSTM_BF16_UNHOIST): the bf16 time steps re-multiply x (r06 experiment)
    bool needs_lstm = false;                  // the plan is followed by the ConvLSTM (its packed gate filters must exist)
    int split_first = -1, split_last = -2;    // op range run as two half-batch chains
    int debug_first_op = 0, debug_last_op = 1 << 30;   // UKBB_DEBUG_OPS
};

constexpr int SMALL_BATCH = 16;
int find_cfg(int id, ConvConfig &out);        // 0: found

// The plan for batches of up to n_hint images of H x W on a device of `cus` compute units.  UKBB_OK, or plan_mode's code / UKBB_EARCH with the error text set.
// f32x3_convs: the handle's ukbb_fcn_set_f32x3_convs setting; it becomes PlanMode::conv_x3 on an FCN plan under UKBB_PREC_F32X3 and is ignored otherwise.
int layout_plan(const ukbb_fcn_arch &a, int precision, int H, int W, int n_hint, int cus, PlanLayout &L, bool f32x3_convs = false);

// ---- forward_cine scratch planner ---------------------------------------------------
// Device bytes forward_cine holds per frame / per window of a cine at one (arch, precision, H, W).  DevBufs count floats; bf16 maps take half.
struct CineUnits {
    int kind = 0, T = 0, n_class = 0;
    size_t HW = 0;
    size_t act_frame = 0;        // the plan's activation workspace, elements per frame (U-Net: allocated as floats in either precision)
    size_t esz = 4;              // UNet-LSTM: bytes per stored gx / hidden element; Temporal-UNet: bytes per activation element (2: UKBB_PREC_BF16_3D)
    size_t gx_frame = 0;         // UNet-LSTM: gx elements per frame and direction (tile-padded: wino24_lstm_gx_floats / lstm_ws_gx_elems)
    size_t c_item = 0;           // UNet-LSTM: cell-state floats per frame (c1, per direction) or window (c) (tile-padded likewise)
    size_t h_item = 0;           // UNet-LSTM: hidden elements per frame or window, direction and step (HW * 16)
};

struct CinePlan {
    int Wn = 0, Wc = 0, chunks = 0;
    int run = 0;                 // frames of the longest chunk's run (F when unchunked)
    uint64_t bytes = 0;          // what forward_cine holds for this call
    uint64_t min_bytes = 0;      // the smallest budget that runs this call
};

// THE units of a plan: what the engine allocates for it and what ukbb_fcn_cine_scratch_bytes predicts (from a layout for 256 compute units)
CineUnits cine_units_from(const PlanLayout &L, const ukbb_fcn_arch &a, int H, int W);
// THE chunk plan of forward_cine.  budget 0: UNet-LSTM one chunk, Temporal-UNet the 4e9-byte rule.  false: the budget is below pl.min_bytes.
bool plan_cine(const CineUnits &u, int F, int time_step, uint64_t budget, CinePlan &pl);
bool cine_request_ok(int T, int F, int H, int W, int time_step);

}  // namespace ukbb
