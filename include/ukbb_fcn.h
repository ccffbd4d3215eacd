/*
 * ukbb_fcn.h -- C ABI of the MI355X (gfx950) FCN / U-Net segmentation engine.
 *
 * This boundary replaces the TensorFlow session of the reference deployment
 * scripts.  Each entry point cites the reference interface it stands for
 * (paths relative to the reference repository root):
 *
 *   ukbb_fcn_create        tf.Session() + tf.train.import_meta_graph(...) +
 *                          saver.restore(sess, model_path)
 *                          (common/deploy_network.py:44-49,
 *                           common/deploy_network_ao.py:53-58)
 *   ukbb_fcn_forward_host  sess.run(['prob:0','pred:0'],
 *                                   feed_dict={'image:0': x, 'training:0': False})
 *                          (common/deploy_network.py:110-111,195-196;
 *                           common/deploy_network_ao.py:121-122,252-253)
 *   ukbb_fcn_forward       same call with inputs/outputs already resident in
 *                          HBM (no reference counterpart: TF always copies)
 *   ukbb_fcn_destroy       leaving the `with tf.Session() as sess:` block
 *
 * The graph evaluated is the one common/train_network.py:142-199 builds with
 * common/network.py:170-230 (build_FCN) or common/network_ao.py:18-64 (UNet),
 * in inference mode ('training:0' = False): conv -> BN(moving stats) -> ReLU.
 *
 * Conventions: plain C types only; tensors are dense NHWC float32 / int32;
 * no exceptions cross the ABI: functions return 0 on success or a negative
 * UKBB_E* code and leave a message retrievable with ukbb_fcn_last_error()
 * (thread-local).  A handle belongs to one device and must not be used from
 * two threads at once (the reference is single-threaded too).
 * There is NO CPU fallback: create() fails when no gfx950 device is usable.
 */
#ifndef UKBB_FCN_H
#define UKBB_FCN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UKBB_FCN_ABI_VERSION 11
#define UKBB_FCN_MAX_LEVEL 8

#define UKBB_OK 0
#define UKBB_EINVAL (-1)   /* bad argument (shape not a multiple of 16, NULL, ...) */
#define UKBB_EARCH (-2)    /* architecture not supported by the kernels */
#define UKBB_EDEVICE (-3)  /* HIP runtime error / no device */
#define UKBB_ENOMEM (-4)

#define UKBB_KIND_FCN 0    /* common/network.py:170 build_FCN */
#define UKBB_KIND_UNET 1   /* common/network_ao.py:18 UNet    */
#define UKBB_KIND_UNET_LSTM 2 /* common/network_ao.py:322 UNet_LSTM_Model, bidirectional (BiConv_LSTM :255);
                               same_dim = ConvLSTM hidden channels (16), fc = unrolled time steps (9);
                               weights: the UNet layers without its conv_out, then per direction the gate
                               kernel [3,3,16+16,64] + bias[64] (forward, backward), then the output conv
                               kernel [1,1,32,n_class] + bias.  Use forward_seq / forward_cine.
                               The single-direction head Conv_LSTM (:214-252, bidirectional=False :349-352) is this
                               kind with an all-zero backward gate kernel + bias and the output kernel [W; 0]: exact
                               (that cell's hidden maps are 0 at every step), detected at create, its time steps are
                               skipped (round 6; weights.embed_unidirectional_lstm does the embedding). */
#define UKBB_KIND_TEMPORAL_UNET 3 /* common/network_ao.py:67-114 Temporal_UNet: the UNet with every 3x3 unit a 3x3x3 conv3d
                               (time stride 1, spatial strides (1,2,2) where the UNet has 2; TF 'SAME' zero padding at the
                               WINDOW edges along time); fc = window length T (9); same_dim unused.
                               weights [TF-recall]: per layer of the UNet order (encoder convs; per decoder level the transposed
                               conv then its convs; conv_out) the kernel -- conv3d DHWIO [3,3,3,Cin,Cout], conv3d_transpose
                               [3,3,3,Cout,Cin], conv_out [1,1,1,16,n_class] -- then gamma, beta, moving_mean, moving_variance
                               (BN epsilon 1e-3), or the bias for conv_out.  fp32, or UKBB_PREC_BF16_3D (set_precision(BF16) -> UKBB_EARCH).
                               Use forward_seq / forward_cine. */

/* Hyper-parameters of build_FCN / UNet as bound in common/train_network.py:174-195
 * and common/train_network_ao.py:268,275-284. */
typedef struct ukbb_fcn_arch {
    int32_t kind;
    int32_t n_class;
    int32_t n_level;
    int32_t n_filter[UKBB_FCN_MAX_LEVEL];
    int32_t n_block[UKBB_FCN_MAX_LEVEL];
    int32_t same_dim;   /* FCN only (32) */
    int32_t fc;         /* FCN only (64) */
} ukbb_fcn_arch;

typedef struct ukbb_fcn_handle ukbb_fcn_handle;

int ukbb_fcn_abi_version(void);
const char *ukbb_fcn_last_error(void);

/* Number of floats ukbb_fcn_create expects for this architecture, or 0 if the
 * architecture is malformed.  Layout: for every layer in graph order
 * (encoder convs; FCN: same_dim0..4, out0, out1, logits; UNet: per decoder
 * level the transposed conv then its convs, logits): kernel in TF layout
 * (HWIO; [kh,kw,Cout,Cin] for the transposed conv), then gamma, beta,
 * moving_mean, moving_variance -- or bias for the logits layer. */
size_t ukbb_fcn_weight_count(const ukbb_fcn_arch *arch);

/* Bind a model to `device` (HIP ordinal).  Folds BN into the kernels, packs
 * MFMA operand fragments and uploads them.  `weights` is host memory and is
 * not referenced after return.  NULL on failure.
 * Accepted architectures (anything else: NULL, ukbb_fcn_last_error() gives the reason): n_level 5, n_filter[0] 16, n_filter[l>0]
 * positive multiples of 32, n_block[l] >= 1.  FCN: same_dim 32,
 * fc 64, n_class 2..6, and n_filter[l>0] one of 32, 64, 128, 256 (the widths the squeeze kernels are built for).  UNet kinds:
 * n_class 2..4; UNet-LSTM: 16 hidden channels; UNet-LSTM and Temporal-UNet: an odd window below 32 frames.  Every launch of the
 * named models and of the descriptors of tests/custom_archs.py (widths 32..256, blocks 1..4 per level) is graded against float64;
 * wider U-Net pyramids are accepted as before and have not been run. */
ukbb_fcn_handle *ukbb_fcn_create(const ukbb_fcn_arch *arch, const float *weights,
                                 size_t n_floats, int device);
void ukbb_fcn_destroy(ukbb_fcn_handle *h);

/* Arithmetic of the MFMA convolutions (BASELINE config 5).  UKBB_PREC_FP32 (default): f32 inputs,
 * exact f32 MFMA.  UKBB_PREC_BF16: bf16 (RNE) MFMA operands, fp32 accumulation.  On a UKBB_KIND_UNET
 * handle (round 3) every activation between layers is ALSO stored as bf16 in HBM (rounded once, after
 * bias + ReLU), every layer runs on the bf16 matrix instructions (16-channel layers zero-padded to the
 * 32-row shape), the first layer (fp32 arithmetic) is evaluated inside the second one's staging and
 * the logits conv + softmax / argmax inside the fused tail: 20 launches, 3.6-3.8x the fp32 rate
 * at N = 100 x 256x256 (round 4-5 builds).  On a UKBB_KIND_UNET_LSTM handle (round 5) the U-Net runs the same bf16-storage
 * plan and the ConvLSTM runs as direct 3x3 convs on the bf16 matrix instruction with its features, the
 * hoisted x half of the gate pre-activations and the hidden maps as bf16 in HBM (accumulation and cell
 * state fp32; gate kernels rounded to bf16, fp32 bias; the x pass rounds the x half of the gates to bf16 as it stores it and takes each
 * frame's FIRST step from those rounded values too, the ones every later step adds; each hidden map is rounded once, as stored): 8-9 ms instead of 19 per 100-frame cine, per-class Dice >= 0.98 against the fp32 cine.  On FCN handles only the operands are bf16 (fp32 activations in
 * HBM; layers without such a tiling stay fp32).  Not bit-compatible with the reference; meant to be
 * judged by Dice against the fp32 result (common/image_utils.py:171-175): 0.993 / 0.992 measured.
 * Each bf16-operand FCN launch is graded against float64 on the rounded operands in tests/test_bf16_operand_launches_gpu.py.
 * Concurrency (round 6): a handle of any kind and precision may run beside kernels of other streams of the process (one handle per stream,
 * one thread per handle; tests/test_concurrency_gpu.py runs two engines on two streams with batches in flight on both).  Until round 6 a
 * UKBB_KIND_UNET handle in UKBB_PREC_BF16 could not: 16-byte buffer stores of its weight-stationary kernels lacked a wait state that hipcc
 * does not emit when the store's soffset is an SGPR, and lost their data under another queue's memory traffic (kernels_ws.hip
 * store_b128_sofs, profiles/r06_notes.md section 10; tests/test_store_hazard.py guards the ISA of the whole library). */
#define UKBB_PREC_FP32 0
#define UKBB_PREC_BF16 1
/* UKBB_PREC_F32X3 (round 2: the FCN head; the FCN's 3x3 conv stack behind ukbb_fcn_set_f32x3_convs
 * below): fp32 results from bf16 matrix instructions.  Every fp32 operand x is
 * split exactly into three bf16 pieces (h = bf16(x), m = bf16(x - h), l = x - h - m); the six partial products whose
 * magnitude can reach 2^-24 of |x||w| (hh, hm, mh, mm, hl, lh) run on the dense matrix cores with fp32 accumulation,
 * the other three (< 2^-24 |x||w|) are dropped -- less than what fp32 accumulation itself rounds away.  Measured
 * against the fp64 oracle the logits error is the same as UKBB_PREC_FP32's (4e-6 relative) and the label maps are
 * identical; it is a different instruction sequence from an fp32 MFMA, so it is offered as its own mode and reported
 * under its own name, never as the default.  Without ukbb_fcn_set_f32x3_convs only the head is converted: every other launch runs exactly
 * as in UKBB_PREC_FP32. */
#define UKBB_PREC_F32X3 2
/* UKBB_PREC_BF16_STORE (UKBB_KIND_FCN only; additive to ABI 11): the FCN encoder on the bf16-storage kernels of the aortic U-Net.  Where it
 * rounds: the folded 3x3 kernels are rounded to bf16 (RNE) once, when they are packed; the image is rounded to bf16 as the fused 1 -> 16 -> 16
 * stem reads it and conv0_0's output as the stem hands it to conv0_1; every encoder map (conv0 .. conv4 and the maps between them) is rounded
 * once, after bias + ReLU, as it is stored -- bf16, channel-blocked [N][C/16][H][W][16].  Accumulation is fp32 everywhere.  The squeeze launches
 * and the head decode the stored bf16 values to fp32 on the way in (exact) and then run the very instruction sequence of UKBB_PREC_FP32 on
 * them: the G_l maps, logits, prob and pred stay fp32 / int32.  UKBB_PREC_BF16 keeps its meaning on an FCN handle (operands only).  On every
 * other kind set_precision returns UKBB_EARCH for this code: those kinds already store bf16 under UKBB_PREC_BF16.  Opt-in; each launch is graded
 * in tests/test_fcn_bf16_store_launches_gpu.py. */
#define UKBB_PREC_BF16_STORE 3
/* UKBB_PREC_BF16_3D (UKBB_KIND_TEMPORAL_UNET only; additive to ABI 11, as UKBB_PREC_BF16_STORE is): the 3-D convolutions on v_mfma_f32_32x32x16_bf16 with fp32 accumulation
 * (kernels_conv3d_bf16.hip).  Where it rounds: the folded 3x3x3 kernels are rounded to bf16 (RNE) once, when they are packed; every map a 3-D
 * launch stores (conv*, up*_t, up*) is rounded once, after bias + ReLU, as it is stored -- bf16, channel-blocked [N][C/16][H*W][16]; a stored
 * map is read back without any further rounding.  The first layer (C_in = 1) runs in fp32 on the fp32 frames with the unrounded folded
 * weights and rounds only what it stores.  conv_out widens the stored up0_1 exactly and runs the fp32 logits launch: logits, prob, the window
 * probabilities of forward_cine and pred stay fp32 / int32, and the window tiling is the fp32 one.  The activation workspace and the cine
 * scratch take 2 bytes per activation element.  UKBB_PREC_BF16 and UKBB_PREC_BF16_STORE stay refused on this kind, and every other kind
 * returns UKBB_EARCH for this code.  Opt-in; each launch is graded in tests/test_temporal_bf16_launches_gpu.py. */
#define UKBB_PREC_BF16_3D 4
/* UKBB_PREC_BF16_FULL (UKBB_KIND_FCN only; additive to ABI 11, as codes 3 and 4 are): UKBB_PREC_BF16_STORE with the head's three matrix products
 * on v_mfma_f32_32x32x16_bf16 as well (kernels_head.hip, the BM instance of fcn_head_pc_kernel: 1 + 4 + 8 matrix instructions per 32-pixel
 * block instead of 8 + 32 + 64 fp32 ones).  The encoder and the squeeze launches are those of UKBB_PREC_BF16_STORE, launch for launch and bit
 * for bit.  The head, per pixel, from the stored bf16 conv0 (16 channels, used as stored) and the handed tile T = b_o0 + sum_l up_l(G_l), which
 * the producer waves compute in fp32 from the fp32 G_1..G_4 exactly as in every other mode:
 *     S = relu(b_s0 + bf16(W_s0) . conv0)              K = 16, fp32 accumulation
 *     P = relu(T + bf16(W_o0[:, 0:32]) . bf16(S))      T enters as the fp32 accumulator
 *     Q = relu(b_o1 + bf16(W_o1) . bf16(P))
 *     logits = W_lg . Q + b_lg, softmax, argmax        the fp32 vector code of every other mode
 * Where it rounds: the three folded weight matrices to bf16 (RNE) once, on the host, when they are packed (pack_head_bf16); S and P once (RNE)
 * in registers, after bias + ReLU.  What stays fp32 / int32: the biases, T, every accumulator, the G_l maps, W_lg, logits, prob and pred -- so
 * every table and file path works unchanged.  UKBB_HEAD_DIRECT_GATHER and UKBB_HEAD_INLINE_TAIL do not apply to this mode (one form: separable
 * gather, in-stage tail).  On every other kind set_precision returns UKBB_EARCH for this code.  Not bit-compatible with the other modes; judged by
 * Dice against the fp32 labels (>= 0.98 per class, tests/test_fcn_bf16_full_gpu.py) and graded as a unit against a float64 model of the lines
 * above in tests/test_fcn_bf16_full_launches_gpu.py.  Opt-in; the default and the benchmark's headline stay UKBB_PREC_FP32. */
#define UKBB_PREC_BF16_FULL 5
int ukbb_fcn_set_precision(ukbb_fcn_handle *h, int precision);

/* The FCN's 3x3 conv stack on three bf16 pieces per operand as well (UKBB_KIND_FCN only; additive to ABI 11; off by default).  The setting
 * is stored on the handle and takes effect on plans made while the precision is UKBB_PREC_F32X3; under any other precision it is kept and
 * ignored.  Toggling it re-plans, as ukbb_fcn_set_precision does.  With it on the plan is the UKBB_PREC_F32X3 plan -- the fp32 fused stem
 * conv0_0 + conv0_1, the fp32 squeeze launches, the three-piece head, the same fp32 maps and workspace -- with the eleven layers
 * conv1_0 .. conv4_2 on the kernel of kernels_conv_x3.hip (tilings 330-345).
 * Where the arithmetic splits: every fp32 activation is split once as its 16-channel chunk of a halo tile is staged into LDS
 * (h = bf16(x), m = bf16(x - h), l = bf16(x - h - m), round to nearest even, residuals exact in fp32); the folded weights likewise on the
 * host when they are packed.  Per filter tap and 16-channel chunk six v_mfma_f32_32x32x16_bf16 add into the one fp32 accumulator, weight
 * piece x activation piece, small terms first: l.h, h.l, m.m, m.h, h.m, h.h.
 * What is dropped: the products m.l, l.m and l.l (each below 2^-24 |w||x|) and what the third piece does not hold (below 2^-24 of the
 * operand) -- less than what the fp32 accumulation rounds away.
 * What stays fp32: every map in HBM (the layers read and store fp32 NHWC), the accumulators, bias, ReLU, the stem, the squeeze launches,
 * logits, prob and pred -- so every table and file path works unchanged.  Not bit-compatible with UKBB_PREC_FP32 or with the plain
 * UKBB_PREC_F32X3; each launch is graded against float64 in tests/test_f32x3_convs_launches_gpu.py.
 * Returns UKBB_EARCH (with a message) on any other kind. */
int ukbb_fcn_set_f32x3_convs(ukbb_fcn_handle *h, int on);

/* Pre-size the activation workspace for batches up to n x h x w (optional;
 * forward() grows it on demand, which synchronises the device). */
int ukbb_fcn_reserve(ukbb_fcn_handle *h, int n, int height, int width);

/* One forward pass, everything in device memory, asynchronous on `stream`
 * (a hipStream_t; NULL = the null stream).  image: [n,h,w,1] float32 with
 * h % 16 == 0 and w % 16 == 0 (the reference pads to that,
 * common/deploy_network.py:97).  Any of logits / prob ([n,h,w,n_class]
 * float32) and pred ([n,h,w] int32 = argmax over the float32 probabilities,
 * lowest index on ties, as common/train_network.py:199 defines it -- equal to
 * the argmax of the logits except where two classes' probabilities round to
 * the same float) may be NULL to skip producing it. */
int ukbb_fcn_forward(ukbb_fcn_handle *h, const float *image, int n, int height, int width,
                     float *logits, float *prob, int32_t *pred, void *stream);

/* Same with host buffers: H2D copy, forward, D2H copy, synchronous --
 * the exact shape of the reference's sess.run call. */
int ukbb_fcn_forward_host(ukbb_fcn_handle *h, const float *image, int n, int height, int width,
                          float *logits, float *prob, int32_t *pred);

/* ---- UNet-LSTM (kind 2) and Temporal-UNet (kind 3): the windowed aortic models of demo_pipeline.py:116-117 ---------
 * Both kinds take forward_seq / forward_cine below; forward / forward_host refuse them with UKBB_EINVAL. */
/* ---- UNet-LSTM (kind 2): the default aortic model of demo_pipeline.py:116-117 -------------------
 * Reference call (common/deploy_network_ao.py:171-172):
 *   prob_idx = sess.run('prob:0', {'image:0': image_idx [N,T,X,Y,1], 'training:0': False})  -> [N,T,X,Y,C]
 * forward_seq is that call: n_seq sequences of T = arch.fc frames each, frame (s, t) at image + (s*T + t)*H*W;
 * outputs in the same [N][T] order (any of logits / prob / pred may be NULL).  Device pointers; asynchronous on
 * `stream` except for the first call with a new n_seq (one blocking upload of the window index table). */
int ukbb_fcn_forward_seq(ukbb_fcn_handle *h, const float *image, int n_seq, int height, int width,
                         float *logits, float *prob, int32_t *pred, void *stream);

/* The whole 'UNet-LSTM' branch of the reference's per-subject loop (common/deploy_network_ao.py:129-183,189)
 * for one slice position: n_frames cine frames at image[f]; frames range(0, n_frames, time_step) are each the
 * centre of one circular window of T frames (--time_step, :26,147), window probabilities are tiled with the
 * weights (1 - |k - rad|/weight_R)^weight_r exactly as the reference accumulates them (float32 accumulator
 * updated through float64, same order), then prob /= weight and pred = argmax.  The U-Net features of a frame
 * are computed once instead of once per window (T times in the reference); results are identical because the
 * U-Net acts per frame.  Reference corner cases reproduced: a frame no window reaches (time_step > window)
 * gets prob = NaN (0/0) and pred 0; with n_frames < T a frame that occurs twice in one window receives only
 * its LAST occurrence (numpy's `a[idx] += b` does not accumulate duplicates).
 * Requires 2*weight_R - 1 == arch.fc, time_step >= 1 and n_frames >= (T-1)/2 (below that the reference itself
 * raises IndexError).  prob [n_frames][H][W][C], pred [n_frames][H][W].
 * Device scratch the handle keeps for this call, besides the U-Net's activations (freed by destroy): with F = n_frames, Wn = windows
 * (= ceil(F / time_step)), HW = H*W, T = arch.fc, e = 4 bytes (fp32) or 2 (UKBB_PREC_BF16):
 *   every step's hidden maps 2*T*Wn*HW*16*e  +  hoisted gate pre-activations 2*F*HW*64*e  +  first-step hidden maps 2*F*HW*16*e
 *   +  cell state (2*F + Wn)*HW*16*4.
 * F = Wn = 100 frames of 256x256: 7.5 + 3.4 + 0.8 + 1.3 = 13.0 GB in fp32, 7.2 GB in bf16 -- several handles per GPU, or cines of
 * hundreds of frames, reach UKBB_ENOMEM on that unless a scratch budget is set (below).  Exactly (what ukbb_fcn_cine_scratch_bytes
 * returns): the gate pre-activations and the cell state live in the kernels' tile layouts, so HW in those two terms is the map padded to
 * whole tiles (fp32: 8 rows x 32 or 16 columns, the region shape of the plan; bf16: 2 rows x 32 columns); the U-Net workspace is
 * F * (every activation map of the plan) * 4 bytes in either precision; the tables take (T*Wn + F*T)*4 + (T + F)*8 bytes.
 * With a scratch budget (ABI 11, ukbb_fcn_set_scratch_budget) the windows run in ascending chunks of Wc, each on the circular run of
 * R = min(F, (Wc - 1)*time_step + T) frames it touches: the formula above with Wn -> Wc in the first and last term and F -> R everywhere
 * else (U-Net workspace included), plus R*HW*4 bytes for the contiguous copy of the run's input frames and the same tables -- no term
 * grows with F but the tables.  Frames shared by neighbouring chunks (T - time_step of them) are recomputed: U-Net features, gate
 * pre-activations and first steps are per-frame quantities, so every chunk size gives the bits of the unchunked call.  Wc = the largest that
 * fits; a budget at or above the unchunked size runs unchunked.
 * Temporal-UNet (kind 3): the same call, bit for bit the same tiling arithmetic and corner cases, but each window runs the whole 3-D
 * network on its T frames (its first layer reads them from `image` through a window -> frame table).  Windows run in chunks of Wc,
 * in ascending order (results do not depend on Wc); device scratch the handle keeps, with HW = H*W, C = n_class and the standard
 * filters 16..256 (the activations of every layer, 152*HW elements per frame of e = 4 bytes, or 2 under UKBB_PREC_BF16_3D):
 *   Wc*T*(152*e + C*4)*HW bytes  +  tables (Wn*T + F*T)*4 + (T + F)*8 bytes,
 * Wc = the largest number of windows that keeps the first term within 4e9 bytes (at least 1), or, with a scratch budget, the whole sum
 * within the budget; UKBB_TEMPORAL_CHUNK_WINDOWS=n overrides both (a test knob):
 * 256x256, T = 9, C = 3: Wc = 10, 3.66 GB in fp32 (Wc = 21 under UKBB_PREC_BF16_3D), whatever the number of frames. */
int ukbb_fcn_forward_cine(ukbb_fcn_handle *h, const float *image, int n_frames, int height, int width,
                          int weight_R, double weight_r, int time_step, float *prob, int32_t *pred, void *stream);

/* -- scratch budget of forward_cine (ABI 11) ------------------------------------------------------------------------
 * bytes = 0 (the default): no budget -- forward_cine runs as described above (UNet-LSTM: one chunk; Temporal-UNet: the 4e9-byte rule).
 * bytes > 0: the device memory forward_cine may hold for its per-cine scratch (everything in the formulas above, the U-Net / 3-D network
 * activation workspace included; weights excluded).  A budget below what one window needs makes forward_cine return UKBB_EINVAL with the
 * minimum for that shape in the message; the handle stays usable.  Setting a new non-zero budget releases the handle's activation and
 * cine buffers (after a device synchronise), and under a budget a forward_cine with another shape or chunk plan than the previous one
 * releases them before it allocates -- so after every budgeted call ukbb_fcn_scratch_bytes() equals ukbb_fcn_cine_scratch_bytes() of that
 * call and is <= the budget.  (Without a budget buffers only grow.)  The UNet-LSTM A/B forms UKBB_LSTM_BF16_WINOGRAD /
 * UKBB_LSTM_BF16_UNHOIST run unchunked only.  FCN / UNet handles accept the call and ignore it. */
int ukbb_fcn_set_scratch_budget(ukbb_fcn_handle *h, uint64_t bytes);
/* Bytes of device memory the handle holds right now in its activation, staging and cine buffers (weights and packed filters excluded). */
uint64_t ukbb_fcn_scratch_bytes(const ukbb_fcn_handle *h);
/* What forward_cine allocates for this call under `budget` (0 = none) on a fresh handle: host arithmetic only, no device needed (like
 * ukbb_fcn_weight_count).  precision: UKBB_PREC_FP32 | UKBB_PREC_BF16 | UKBB_PREC_BF16_3D.  0 for a malformed request (kinds 0 / 1, shape not a
 * multiple of 16, fewer frames than the window radius, time_step < 1, a precision the kind refuses: UKBB_PREC_BF16 on a Temporal-UNet,
 * UKBB_PREC_BF16_3D on a UNet-LSTM) and for a budget below the minimum.  The engine plans its chunks
 * with the same function.  The fp32 region shape is chosen for the MI355X's 256 compute units and cines of n_frames frames. */
uint64_t ukbb_fcn_cine_scratch_bytes(const ukbb_fcn_arch *arch, int precision, int n_frames, int height, int width, int time_step,
                                     uint64_t budget);
/* The smallest non-zero budget forward_cine accepts for this call (0: malformed request), and the windows per chunk Wc it runs with
 * under `budget` (0: malformed or below the minimum; the number of windows ceil(n_frames / time_step) when unchunked). */
uint64_t ukbb_fcn_cine_min_scratch_bytes(const ukbb_fcn_arch *arch, int precision, int n_frames, int height, int width, int time_step);
int ukbb_fcn_cine_chunk_windows(const ukbb_fcn_arch *arch, int precision, int n_frames, int height, int width, int time_step, uint64_t budget);

/* ---- device-side pre/post-processing of the deploy loop ----------------
 * Stateless; device pointers; asynchronous on `stream` unless stated.  They take the host numpy work
 * (a full sort of ~20 M voxels per subject, pad, transposes) off the critical path of the reference's
 * common/deploy_network.py:86-131. */

/* Exact order statistics: out_host[i] = the ranks[i]-th smallest (0-based) of the n float32 values at
 * d_data (16-byte aligned, any order; NaNs are not expected in MR magnitudes and sort as their bit
 * pattern).  4-pass radix select on device; synchronous (the few results are copied back).
 * Replaces the sort inside np.percentile(image, thres), common/image_utils.py:72 -- the caller does
 * numpy's linear interpolation between neighbouring ranks on the host.  1 <= nranks <= 8. */
int ukbb_fcn_select_kth(const float *d_data, size_t n, const uint64_t *ranks, int nranks, float *out_host, void *stream);

/* (X,Y,Z,T) float32 volume with element strides (sx,sy,sz,st) -> network input d_batch[T*Z][X2][Y2]:
 * the in-place clip to [lo, hi] as stored in float32, (v - lo) / (hi - lo) in float64 rounded to
 * float32, centred zero padding (x_pre, y_pre before; X2, Y2 multiples of 16), batch index b = t*Z + z.
 * Replaces common/image_utils.py:73-76 and common/deploy_network.py:97-107. */
int ukbb_fcn_rescale_pack(const float *d_vol, int X, int Y, int Z, int T, int64_t sx, int64_t sy, int64_t sz, int64_t st,
                          double lo, double hi, int X2, int Y2, int x_pre, int y_pre, float *d_batch, void *stream);

/* int32 labels d_pred[T*Z][X2][Y2] -> cropped uint8 volume d_vol in NIfTI order (x fastest, then y, z, t)
 * and d_counts[T][n_class] = voxels of each class per frame (what the ES pick of
 * common/deploy_network.py:125-130 sums).  Replaces :114-116.  n_class <= 16. */
int ukbb_fcn_unpack_labels(const int32_t *d_pred, int X, int Y, int Z, int T, int X2, int Y2, int x_pre, int y_pre, int n_class,
                           uint8_t *d_vol, uint64_t *d_counts, void *stream);

/* -- the aortic z-score, common/image_utils.py:60-67 (normalise_intensity), bit-identical to numpy ----------------
 * np.mean / np.std over image[roi] are float32 PAIRWISE sums over the compressed array; the three calls below
 * reproduce numpy's summation tree rather than just its value (ukbb_cardiac_amd/device_pipeline.py
 * device_zscore_stats shows the sequence, including the percentile threshold from ukbb_fcn_select_kth). */

/* d_out[i] = the i-th element >= thr of the (X,Y,Z,T) float32 volume with element strides (sx,sy,sz,st), in
 * row-major INDEX order (last index fastest: the order of numpy's image[image >= thr]).  d_out holds up to
 * X*Y*Z*T floats; *n_host receives the count.  Synchronous. */
int ukbb_fcn_roi_compact(const float *d_vol, int X, int Y, int Z, int T, int64_t sx, int64_t sy, int64_t sz, int64_t st, float thr,
                         float *d_out, uint64_t *n_host, void *stream);

/* *sum_host = np.add.reduce over the n contiguous float32 values at d_a (squared_dev = 0) or over
 * (d_a[i] - mean)^2 evaluated in float32 (squared_dev = 1, the inner sum of np.var), with numpy's pairwise
 * summation order (blocks of <= 128 elements on 8 interleaved accumulators, halves split at a multiple of 8, one
 * such tree per 8192-element buffer of numpy's reduction iterator [np.getbufsize() default], buffers added in
 * sequence): every leaf block is summed by one device thread, the host adds the leaves up.  Synchronous. */
int ukbb_fcn_pairwise_sum(const float *d_a, uint64_t n, int squared_dev, float mean, float *sum_host, void *stream);

/* ukbb_fcn_rescale_pack with the z-score arithmetic: d_batch[t*Z+z][X2][Y2] = (v - mu) / den in float32 (IEEE
 * division), zero padding around it.  Replaces image_utils.py:67 + deploy_network_ao.py:105-108,147-150. */
int ukbb_fcn_zscore_pack(const float *d_vol, int X, int Y, int Z, int T, int64_t sx, int64_t sy, int64_t sz, int64_t st,
                         float mu, float den, int X2, int Y2, int x_pre, int y_pre, float *d_batch, void *stream);

/* -- integer volumes (ABI 9): the same pre-processing for the uint8 / int16 / uint16 files MR converters write ---------
 * What nib.load(...).get_data() returns for them (common/deploy_network.py:80-81, deploy_network_ao.py:82-85) goes through
 * image_utils.py with numpy's integer arithmetic, which the calls below reproduce bit for bit:
 *   - np.percentile takes float64 quantiles (scalar or tuple q alike) and interpolates in float64 between two integer order
 *     statistics (numpy's lerp subtracts them in the integer type first; the caller does that interpolation);
 *   - the in-place clip stores the float64 bound TRUNCATED toward zero into the integer array, the comparisons and the
 *     rescale use the untruncated float64 bounds;
 *   - np.mean / np.std of image[roi] reduce in float64 (the plain sum of 8/16-bit values is exact in any order, the sum of
 *     squared deviations is not: numpy's pairwise tree again), and the z-score is float64 rounded once to float32.
 * nifti_datatype: the NIfTI codes ukbb_fcn_gzip_labels uses -- 2 (uint8), 4 (int16), 512 (uint16); any other code, float32
 * (16) included, returns UKBB_EINVAL (float32 volumes take the untyped calls above).  Device pointers; asynchronous on
 * `stream` unless stated. */

/* ukbb_fcn_select_kth for integer voxels: out_host[i] = the ranks[i]-th smallest value (exact, as a double).  d_data 16-byte
 * aligned.  1 radix pass for uint8, 2 for the 16-bit types (int16 with its sign bit flipped).  Synchronous.
 * Replaces the sort inside np.percentile(image, ...), common/image_utils.py:62,72. */
int ukbb_fcn_select_kth_t(const void *d_data, int nifti_datatype, size_t n, const uint64_t *ranks, int nranks, double *out_host,
                          void *stream);

/* ukbb_fcn_rescale_pack for an integer volume: clip_lo / clip_hi = the float64 percentiles lo / hi truncated toward zero (what
 * image[image < lo] = lo stores; they must fit the voxel type), v compared with lo / hi in float64, then (v - lo) / (hi - lo)
 * in float64 rounded to float32, centred zero padding, batch index b = t*Z + z.  Replaces common/image_utils.py:73-76 and
 * common/deploy_network.py:97-107 for integer data. */
int ukbb_fcn_rescale_pack_t(const void *d_vol, int nifti_datatype, int X, int Y, int Z, int T, int64_t sx, int64_t sy, int64_t sz,
                            int64_t st, int64_t clip_lo, int64_t clip_hi, double lo, double hi, int X2, int Y2, int x_pre, int y_pre,
                            float *d_batch, void *stream);

/* ukbb_fcn_roi_compact for an integer volume: d_out (voxel type, up to X*Y*Z*T elements) = the elements with
 * float64(v) >= thr in numpy's row-major index order -- image[image >= val_l], image_utils.py:63-64.  Synchronous. */
int ukbb_fcn_roi_compact_t(const void *d_vol, int nifti_datatype, int X, int Y, int Z, int T, int64_t sx, int64_t sy, int64_t sz,
                           int64_t st, double thr, void *d_out, uint64_t *n_host, void *stream);

/* ukbb_fcn_pairwise_sum over n contiguous integer values converted to float64: the sum (squared_dev = 0; exact, what np.mean of
 * integer data divides) or the sum of (v - mean)^2 evaluated in float64 (squared_dev = 1, the inner sum of np.var) along
 * numpy's pairwise tree, float64 leaves and float64 additions up the tree.  Synchronous.  Replaces the reductions of
 * image_utils.py:65. */
int ukbb_fcn_pairwise_sum_t(const void *d_a, int nifti_datatype, uint64_t n, int squared_dev, double mean, double *sum_host,
                            void *stream);

/* ukbb_fcn_zscore_pack for an integer volume: d_batch[t*Z+z][X2][Y2] = (float64(v) - mu) / den in float64 (IEEE division),
 * rounded once to float32, zero padding around it.  Replaces image_utils.py:67 + deploy_network_ao.py:105-108,147-150. */
int ukbb_fcn_zscore_pack_t(const void *d_vol, int nifti_datatype, int X, int Y, int Z, int T, int64_t sx, int64_t sy, int64_t sz,
                           int64_t st, double mu, double den, int X2, int Y2, int x_pre, int y_pre, float *d_batch, void *stream);

/* -- the aortic quality control (ABI 10): the label-map and image statistics of cardiac_utils.aorta_pass_quality_control ---
 * (reference common/cardiac_utils.py:1739-1796, applied by aortic/eval_aortic_area.py:68-69) on the cine and the uint8 label
 * volume (NIfTI order, what ukbb_fcn_unpack_labels writes) the aortic device path already holds.  nifti_datatype of the voxels:
 * 16 (float32), 2 (uint8), 4 (int16), 512 (uint16).  ukbb_cardiac_amd/aorta_qc.py shows the sequence and the host arithmetic. */

/* d_n_large[t][k] (int32, T x n_class) = the number of connected components of the mask lab[:, :, :, t] == k with MORE than
 * min_size voxels, k = 1 .. n_class - 1 (column 0 stays 0); connectivity 2 of skimage in 3-D (18-neighbourhood: neighbours
 * differ in at most two coordinates), no connectivity across frames.  Replaces skimage.measure.label(seg_t == l,
 * connectivity=2) and the size filter of cardiac_utils.py:1766-1780.  d_work: 2*X*Y*Z*T int32 the caller allocates (the
 * union-find's parents and component sizes).  Union-find with integer atomics: the counts do not depend on arrival order.
 * Asynchronous.  n_class <= 16, Z*T <= 65535, 2*X*Y*Z*T < 2^31. */
int ukbb_fcn_label_components(const uint8_t *d_lab, int X, int Y, int Z, int T, int n_class, int min_size, int32_t *d_work,
                              int32_t *d_n_large, void *stream);

/* d_max[t][k] (float64, T x n_class) = np.max(image[:, :, :, t][lab[:, :, :, t] == k]) of the (X,Y,Z,T) volume with element
 * strides (sx,sy,sz,st): exact for every voxel type, NaN when a NaN lies under the mask (as np.max), -inf for an empty mask.
 * Integer maxima of order-preserving keys: no float atomics, no dependence on arrival order.  Replaces the np.max of
 * cardiac_utils.py:1757-1761.  Asynchronous.  n_class <= 16, T <= 65535. */
int ukbb_fcn_label_max(const void *d_vol, int nifti_datatype, int X, int Y, int Z, int T, int64_t sx, int64_t sy, int64_t sz, int64_t st,
                       const uint8_t *d_lab, int n_class, double *d_max, void *stream);

/* d_out[i] = the i-th element of frame 0 of the volume (element strides sx,sy,sz) whose label lab[x + X*(y + Y*z)] is `label`,
 * in row-major INDEX order of the (X,Y,Z) frame (z fastest): numpy's image_ED[seg_ED == l], cardiac_utils.py:1753-1755.  d_out
 * (voxel type) holds up to X*Y*Z elements; *n_host receives the count.  ukbb_fcn_pairwise_sum (float32) or
 * ukbb_fcn_pairwise_sum_t (integer types) over it then give numpy's .mean() sum bit for bit.  Synchronous. */
int ukbb_fcn_label_compact(const void *d_vol, int nifti_datatype, int X, int Y, int Z, int64_t sx, int64_t sy, int64_t sz, const uint8_t *d_lab,
                           int label, void *d_out, uint64_t *n_host, void *stream);

/* -- the short- and long-axis quality-control gates (additive to ABI 11): component statistics of P label planes of X*Y uint8
 * voxels (x fastest: the planes ukbb_fcn_unpack_labels leaves behind).  Planes never connect; inside a plane connectivity is 8,
 * skimage.measure.label's default for a 2-D array.  All outputs int32 and exact:
 *   d_count[p][k], d_largest[p][k], d_kept[p][k] (P x n_class, column 0 stays 0): the voxels of class k on plane p, the size
 *     of the largest component of plane == k (0 if absent), the sum of the sizes of its components with AT LEAST keep_min voxels
 *     (remove_small_cc deletes area < thres);
 *   d_union_largest[p]: the size of the largest component of (largest component of class a) | (components of class b with at
 *     least keep_min voxels) -- `epi`.  Of two class-a components of equal largest size the one whose smallest x*Y + y is
 *     smaller joins the union: get_largest_cc takes the first label of the strictly greatest area, and labels are numbered in
 *     a C-order scan of the [x][y] array.
 * Replaces get_largest_cc / remove_small_cc (reference common/image_utils.py:227-249) as sa_pass_quality_control
 * (common/cardiac_utils.py:119-135, a = 1, b = 2, keep_min = 10) and la_pass_quality_control (:157-168) apply them, and the
 * np.sum(seg == l) of :86-105 and :149-155.  Labels >= n_class are ignored.  d_work: 8-byte aligned,
 * 2*P*n_class + 3*X*Y*P + (X*Y*P + 3)/4 int32 the caller allocates (keys, parents, sizes, first indices, the derived mask).
 * Integer atomic add / min / max only: nothing depends on arrival order.  Asynchronous.
 * n_class <= 16, 1 <= a != b < n_class, P <= 65535, 4*X*Y*P < 2^31. */
int ukbb_fcn_plane_components(const uint8_t *d_planes, int X, int Y, int P, int n_class, int a, int b, int keep_min, int32_t *d_work,
                              int32_t *d_count, int32_t *d_largest, int32_t *d_kept, int32_t *d_union_largest, void *stream);

/* -- atrial area and length (additive to ABI 11): cardiac_utils.evaluate_atrial_area_length (reference
 * common/cardiac_utils.py:1655-1736) for every (plane, class) cell of P label planes of X*Y uint8 voxels (x fastest), by the
 * rules ukbb_cardiac_amd/atrial.py states (frame_stats_host is the specification).  d_out[p][k][8] (int32, all P*n_class*8
 * written; the cells of class 0 are zero) = size, status, x0, y0, x1, y1, n_hits, 0:
 *   size    voxels of the largest 8-connected component C of plane == k (ties as ukbb_fcn_plane_components)
 *   status  0 the class is absent, 1 measured, 2 the major axis is NaN (fewer than 3 voxels, or the centres of the bottom and the
 *           top third coincide), 3 the axis line misses C
 *   (x0, y0), (x1, y1)  the pixels of the rasterised axis line inside C that come first and last in the order (d, x*Y + y),
 *           n_hits their number; d(x, y) = (w0*l0 + w1*l1) + w2*l2, w_i = (a_i0*x + a_i1*y) + a_i3 in float64, one rounding per
 *           operation.  affine: rows 0..2 of the voxel-to-world matrix, row-major; long_axis: l.  Both finite.
 * The thirds come from an exact radix select on (order-preserving key of d, x*Y + y), their centres from integer sums, the two
 * hits from integer minima and maxima: no float atomics, nothing depends on arrival order.  The line is the 8-connected line of
 * OpenCV (clipLine + LineIterator, left to right) as atrial.line_pixels restates it.  Labels >= n_class are ignored.
 * d_work: 8-byte aligned, 2*P*n_class + 3*X*Y*P + (X*Y*P + 3)/4 int32 the caller allocates (keys, parents, sizes, first
 * indices, the map of the winning components).  Asynchronous.  n_class <= 16, P <= 65535, 4*X*Y*P < 2^31. */
int ukbb_fcn_atrial_area_length(const uint8_t *d_planes, int X, int Y, int P, int n_class, const double affine[12], const double long_axis[3],
                                int32_t *d_work, int32_t *d_out, void *stream);

/* -- overlap and contour distances of two label volumes (additive to ABI 11): np_categorical_dice and distance_metric (reference
 * common/image_utils.py:171-224) for every (plane, class) cell of P label planes of X*Y uint8 voxels (x fastest: d_pred as
 * ukbb_fcn_unpack_labels leaves it, d_truth a second volume of the same layout), by the rules ukbb_cardiac_amd/seg_score.py states
 * (stats_host is the specification).  With A = pred plane == k, B = truth plane == k:
 *   d_cells[p][k][8] (int32, all P*n_class*8 written; the cells of class 0 are zero) = status, nA, nB, nAB, cA, cB, hA, hB
 *     nA, nB, nAB   |A|, |B|, |A & B|
 *     status        1 when nA > 0 and nB > 0 (the distances are defined), else 0 and the five fields below are zero
 *     cA, cB        the contour pixels of A and of B: the pixels of the mask with a 4-neighbour off the image or in the outer
 *                   background (the non-mask pixels 4-connected to the image frame) -- the set cv2.findContours(RETR_EXTERNAL,
 *                   CHAIN_APPROX_NONE) visits
 *     hA, hB        max over the contour of A of the smallest squared pixel distance to the contour of B, and the other way round
 *   d_sums[p][k][2] (float64) = sA, sB: the sum over the contour of A (of B) of the square root of that smallest squared distance,
 *                   the pixels taken in the order x*Y + y and added as np.add.reduce adds a contiguous float64 array (numpy's
 *                   pairwise tree, one per 8192-element buffer).
 * The outer background is flooded to a fixed point; the distances come from the exact two-phase squared Euclidean transform, at
 * most X*Y + c*X steps per direction whatever the labels are: no capacity, no decline.  Integer minima, maxima and adds only, the
 * float64 additions in a fixed order: nothing depends on arrival order.  Labels >= n_class are ignored.  d_work: 16-byte aligned,
 * ukbb_fcn_score_planes_work(X, Y, P, n_class) bytes (0 for a shape the call refuses), at most 64 MB.  d_sums 8-byte aligned.
 * Asynchronous.  n_class 2..16, P <= 65535; X, Y <= 1024 and ceil(X/32)*Y <= 8192 (the bit planes of one cell live in LDS:
 * 512 x 512 fits): a larger plane returns UKBB_EINVAL with a message and the caller scores it on the host. */
uint64_t ukbb_fcn_score_planes_work(int X, int Y, int P, int n_class);
int ukbb_fcn_score_planes(const uint8_t *d_pred, const uint8_t *d_truth, int X, int Y, int P, int n_class, void *d_work, int32_t *d_cells,
                          double *d_sums, void *stream);

/* -- how sure the network was (additive to ABI 11): per (frame, class) integer reductions of the softmax, by the rules
 * ukbb_cardiac_amd/confidence.py states (cells_host is the specification).  d_prob [n][X2][Y2][n_class] float32 and d_pred [n][X2][Y2]
 * int32 as ukbb_fcn_forward leaves them for n slices of the padded batch [T*Z][X2][Y2], the first of which is slice first_slice of
 * that batch (slice b belongs to frame b / Z, as in ukbb_fcn_unpack_labels).  Only the image region counts: x2 in [x_pre, x_pre + X),
 * y2 in [y_pre, y_pre + Y).  With q(p) = (int)(p * 65536.0f) (exact multiply, truncation; 0 for a denormal or a NaN) and, for a voxel
 * labelled c = pred, q1 = q(p[c]), margin = q1 - max over c' != c of q(p[c']), the call ADDS into d_cells[t][c][20] (uint64):
 *   0       the voxels of frame t with pred == c
 *   1, 2    the sums of q1 and of margin over those voxels
 *   3..18   the histogram of min(q1 >> 12, 15) over those voxels (16 bins of width 1/16; p == 1 lands in the last)
 *   19      the sum of q(p[c]) over ALL voxels of the frame (the soft count)
 * A voxel whose label lies outside 0 .. n_class - 1 counts in field 19 only.  The caller zeroes d_cells [T][n_class][20] once per
 * subject and calls once per chunk of slices.  Integer adds only: nothing depends on arrival order or on the chunking.  Reads
 * 4 * n_class + 4 bytes per image voxel and writes nothing else.  Asynchronous.  n_class 2..16, first_slice + n <= Z*T <= 65535,
 * X*Y <= 2^30, d_prob 16-byte and d_cells 8-byte aligned. */
int ukbb_fcn_confidence_cells(const float *d_prob, const int32_t *d_pred, int n, int X, int Y, int Z, int T, int X2, int Y2, int x_pre, int y_pre,
                              int n_class, int first_slice, uint64_t *d_cells, void *stream);

/* ---- label-volume files (host only: no device, no stream) ---------------------------------------
 * What the reference does with the result: nib.save of np.zeros(image.shape) filled with the labels
 * (common/deploy_network.py:92,116,136-138; deploy_network_ao.py:189-196) -- for a short-axis subject
 * 160 MB of float64 through zlib, 0.5 s of a core against 11 ms of network time.
 *
 * ukbb_fcn_gzip_labels writes ONE gzip member (RFC 1952 / 1951, one deflate block) whose inflated
 * content is  prefix || labels converted to the NIfTI voxel type `nifti_datatype`
 * (2 uint8, 4 int16, 8 int32, 16 float32, 64 float64; little-endian),  i.e. the .nii.gz nibabel writes
 * when prefix is the 352-byte NIfTI-1 header, without forming the converted volume: a run of equal
 * labels becomes E literals + matches of distance E, its CRC-32 is computed per run.  labels[n] uint8
 * in file order (x fastest).  Returns the number of bytes written to out, or UKBB_ENOMEM when out_cap
 * is too small (ukbb_fcn_gzip_labels_bound is always sufficient; a label map of a real segmentation
 * needs ~2 % of it), or UKBB_EINVAL. */
uint64_t ukbb_fcn_gzip_labels_bound(uint64_t n_voxels, int nifti_datatype, uint64_t prefix_len);
int64_t ukbb_fcn_gzip_labels(const uint8_t *labels, uint64_t n_voxels, int nifti_datatype, const uint8_t *prefix, uint64_t prefix_len,
                             uint8_t *out, uint64_t out_cap);
/* Same, with the Huffman code set chosen: UKBB_GZIP_DYNAMIC (what ukbb_fcn_gzip_labels uses: a counting pass over the
 * runs, then codes built from the exact token histogram -- files no larger than zlib level 1 writes for the same volume)
 * or UKBB_GZIP_FIXED (the fixed codes of RFC 1951 3.2.6: no counting pass, files 2-4x larger).  Same inflated bytes. */
#define UKBB_GZIP_FIXED 0
#define UKBB_GZIP_DYNAMIC 1
int64_t ukbb_fcn_gzip_labels_mode(const uint8_t *labels, uint64_t n_voxels, int nifti_datatype, const uint8_t *prefix, uint64_t prefix_len,
                                  uint8_t *out, uint64_t out_cap, int mode);

/* ---- label-volume files, deflated on the device ---------------------------------------------------------------
 * The member ukbb_fcn_gzip_labels_mode writes, byte for byte, from a label volume that lies in device memory: the token stream is a pure
 * function of the run list, so run detection, the token histogram, per-run bit counts, a prefix sum of bit offsets, emission and the
 * CRC-32 (closed form per run, GF(2) combine) are data-parallel (csrc/kernels_labelgz.hip; the per-run arithmetic is
 * csrc/label_gzip_core.h, one text with the host writer).  The inflated stream is never formed.  No reference counterpart.
 *
 * ukbb_fcn_gzip_labels_device: everything is enqueued on `stream`; nothing synchronises.  d_labels[n_voxels] uint8 in file order,
 * d_prefix[prefix_len] the bytes in front of the voxels (the 352-byte NIfTI-1 header), both device memory; mode UKBB_GZIP_FIXED or
 * UKBB_GZIP_DYNAMIC; datatypes 2, 4, 8, 16, 64 as on the host.  d_out[out_cap] (4-byte aligned) receives the member; no byte at or
 * beyond out_cap is written.  d_scratch: ukbb_fcn_gzip_labels_device_scratch(n_voxels, max_runs) bytes (16-byte aligned) holding, among
 * others, a run table of max_runs entries; nothing outside it is written.  *d_len (device int64) = the member's length, or
 * UKBB_LABELGZ_NO_ROOM when it does not fit out_cap, or UKBB_LABELGZ_TOO_MANY_RUNS when the volume has more than max_runs runs; after
 * a decline d_out holds nothing of use.  The return value carries argument and launch errors only.
 * Limits: 1 <= n_voxels <= UKBB_LABELGZ_MAX_VOXELS, prefix_len <= UKBB_LABELGZ_MAX_PREFIX, 1 <= max_runs <= n_voxels is enough.
 * ukbb_fcn_gzip_labels_device_geometry: geometry[0] = voxels per workgroup of the run scan, [1] = runs per workgroup of the
 * histogram / bit-offset / emission launches, [2] = bits per LDS window of the emission, [3] = (258, E) tokens from which a run is
 * filled by the whole workgroup (tests place run starts around these borders). */
#define UKBB_LABELGZ_NO_ROOM (-4)
#define UKBB_LABELGZ_TOO_MANY_RUNS (-5)
#define UKBB_LABELGZ_MAX_VOXELS 0x7fff0000ull
#define UKBB_LABELGZ_MAX_PREFIX 4096
uint64_t ukbb_fcn_gzip_labels_device_scratch(uint64_t n_voxels, uint64_t max_runs);
void ukbb_fcn_gzip_labels_device_geometry(uint32_t geometry[4]);
int ukbb_fcn_gzip_labels_device(const uint8_t *d_labels, uint64_t n_voxels, int nifti_datatype, const uint8_t *d_prefix, uint64_t prefix_len,
                                int mode, uint8_t *d_out, uint64_t out_cap, void *d_scratch, uint64_t max_runs, int64_t *d_len, void *stream);
/* The same parallel formulation, run serially on the host over host pointers (tests, sanitizer program): returns the length,
 * UKBB_LABELGZ_NO_ROOM / UKBB_LABELGZ_TOO_MANY_RUNS (nothing written), or UKBB_EINVAL. */
int64_t ukbb_fcn_gzip_labels_parallel_host(const uint8_t *labels, uint64_t n_voxels, int nifti_datatype, const uint8_t *prefix,
                                           uint64_t prefix_len, int mode, uint8_t *out, uint64_t out_cap, uint64_t max_runs);

/* ---- image files in (host only) -------------------------------------------------------------------
 * What the reference does first with every subject: nib.load(image_name).get_data()
 * (common/deploy_network.py:80-83, deploy_network_ao.py:88-92) -- for a short-axis cine 40 MB of int16
 * through zlib, 0.26 s of a core against 11 ms of network time; it bounds a cohort run.
 *
 * ukbb_fcn_gunzip inflates a whole .gz file image (every member, zero padding between / after members
 * skipped) from src into dst and returns the number of bytes written; each member's ISIZE and -- unless
 * verify_crc is 0 -- CRC-32 are checked.  Whole-buffer decoder (64-bit bit buffer, two-level tables, wide
 * match copies, carry-less-multiply CRC), 1.75-2.3x zlib 1.2.11 on MR image data.  Strict by design: returns
 * UKBB_ENOMEM when the content does not fit dst_cap and UKBB_EINVAL for anything else it does not accept
 * (truncated or invalid stream, header CRC flag, trailing bytes that are not a member, CRC / length
 * mismatch); the caller falls back to zlib, which raises -- or accepts -- as before.
 * ukbb_fcn_gzip_crc: zlib's crc32(crc, data, n). */
int64_t ukbb_fcn_gunzip(const uint8_t *src, uint64_t src_len, uint8_t *dst, uint64_t dst_cap, int verify_crc);
uint32_t ukbb_fcn_gzip_crc(uint32_t crc, const uint8_t *data, uint64_t n);

/* ---- image files in, on the device ------------------------------------------------------------------
 * The same inflate for many files at once: the compressed bytes go up (fewer than the raw volume), ONE wave decodes one stream,
 * hundreds decode side by side in one launch (csrc/kernels_inflate.hip; the decoder is csrc/inflate_core.h, one text for the kernel
 * and for ukbb_fcn_inflate_core_host).  No reference counterpart (it leaves gzip to nibabel).
 *
 * ukbb_fcn_inflate_device: stream i is the RAW deflate stream (after the gzip member header, before the 8-byte trailer)
 * d_src[src_off, src_off + src_len); its output goes to d_dst[dst_off, dst_off + dst_cap) and nothing outside that region is written.
 * d_written[i] = bytes written, or -1 out of input / -2 invalid stream / -3 does not fit dst_cap; an error ends that stream only (its
 * region then holds a prefix of unspecified length).  d_crc (optional) [i] = CRC-32 of the d_written[i] bytes (zlib's crc32; 0 for a
 * refused stream).  Output regions must not overlap; any alignment is accepted, a 16-byte aligned dst_off stores fastest.
 * `streams` is HOST memory and is copied before the call returns (one upload); everything else is asynchronous on `stream`.
 * The library keeps two copies of the table per device and takes them in turn: a call returns at once while the PREVIOUS call's
 * launches still run, and waits on the host for the call before that one if it has not finished.
 * Limits: 1 <= n_streams <= UKBB_INFLATE_MAX_STREAMS, src_len and dst_cap <= UKBB_INFLATE_MAX_BYTES each.  Strictness is that of
 * ukbb_fcn_gunzip's decoder: over-subscribed or incomplete codes (but the single length-1 distance code), symbols 286 / 287 and
 * distance symbols 30 / 31, a repeat with nothing to repeat, HLIT > 286, block type 3 and LEN != ~NLEN are refused, and so is a
 * stream whose last block ends before byte src_len - 1 (in a gzip member the trailer follows the stream at once).
 * LDS: 56 368 bytes static per workgroup of one wave (tables 15.0 KB, 36 KB ring of the last output, 4 KB input window): 2 workgroups
 * per CU, 512 streams in flight on 256 CUs; more streams than that are taken in turn by the same grid.  The CRC kernel takes
 * UKBB_INFLATE_CRC_CHUNK bytes per workgroup. */
typedef struct { uint64_t src_off, src_len, dst_off, dst_cap; } ukbb_fcn_gz_stream;
#define UKBB_INFLATE_MAX_STREAMS 65535
#define UKBB_INFLATE_MAX_BYTES (1ull << 40)
#define UKBB_INFLATE_CRC_CHUNK 65536
int ukbb_fcn_inflate_device(const uint8_t *d_src, uint8_t *d_dst, const ukbb_fcn_gz_stream *streams, int n_streams, int64_t *d_written,
                            uint32_t *d_crc, void *stream);
/* The same decoder core compiled for the host (tests, sanitizer runs): returns the bytes written or -1 / -2 / -3 as above. */
int64_t ukbb_fcn_inflate_core_host(const uint8_t *src, uint64_t src_len, uint8_t *dst, uint64_t dst_cap);
/* CRC-32 of A || B from crc_a = crc32(A), crc_b = crc32(B) and len_b = |B| (zlib's crc32_combine).  Host. */
uint32_t ukbb_fcn_gzip_crc_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);

/* ---- measurement / introspection (bench.py, tests) ---------------------- */

/* Kernel launches of one forward, in launch order. */
int ukbb_fcn_num_kernels(const ukbb_fcn_handle *h);
const char *ukbb_fcn_kernel_name(const ukbb_fcn_handle *h, int i);
/* Algorithmic MACs kernel i performs for the LAST forward's shape. */
double ukbb_fcn_kernel_macs(const ukbb_fcn_handle *h, int i);
/* Multiplies kernel i actually issues to the matrix pipe for that shape (tile padding excluded).
 * Differs from the algorithmic count where the kernel runs a cheaper algorithm: Winograd F(2x2,3x3)
 * layers (16/36 of the direct count), the head (level-0 slice of the 160->64 conv only; the other
 * slices run at low resolution inside the sqg kernels), the first layer (vector ALU, reported as 0). */
double ukbb_fcn_kernel_mfma_macs(const ukbb_fcn_handle *h, int i);
/* The same INCLUDING what the kernel issues for partly filled tiles / Winograd regions (every Winograd region runs its 32 tile slots
 * whatever part of them the map fills): = SQ_INSTS_MFMA x MACs per instruction of a rocprofv3 counter pass. */
double ukbb_fcn_kernel_mfma_macs_issued(const ukbb_fcn_handle *h, int i);

/* Tiling id the plan chose for kernel i (conv kernels; -1 for the others) and
 * its descriptive name; used by tools/tune_convs.py.  The environment variable
 * UKBB_CONV_CFG="layer:id,layer:id" overrides the choice at plan time. */
int ukbb_fcn_kernel_config(const ukbb_fcn_handle *h, int i);
const char *ukbb_fcn_conv_config_name(int id);

/* Which form of the logits tail the most recent producer/consumer head launch of this process ran: 0 deferred into the next
 * block's MFMA stream (the fp32 separable instance's default), 1 inside the block's own stage (UKBB_HEAD_INLINE_TAIL=1, and always
 * the f32x3 and direct-gather instances), -1 before the first such launch.  For A/B tests of the knob, which is latched per
 * process (tests/test_head_tail_gpu.py).  Added without an ABI bump: nothing that existed changed. */
int ukbb_fcn_head_tail_form(void);

/* When enabled, every launch of forward() is bracketed by hipEvents recorded
 * on the forward's own stream; ukbb_fcn_kernel_times() then synchronises and
 * returns, per kernel, the summed duration in ms and the number of timed
 * launches since the last reset. */
int ukbb_fcn_set_timing(ukbb_fcn_handle *h, int enable);
/* Time only kernel `kernel` (index in launch order; < 0 = all): two event records per
 * forward instead of two per launch, so the timed region is not perturbed. */
int ukbb_fcn_set_timing_kernel(ukbb_fcn_handle *h, int kernel);
int ukbb_fcn_kernel_times(ukbb_fcn_handle *h, double *sum_ms, int64_t *count, int n, int reset);

/* Copy an intermediate activation of the LAST forward to host (tests only).
 * Names: the layer names of the plan ("conv0_0".."conv4_1", "up3_t".."up0_1": every conv's output map, NHWC;
 * a Temporal-UNet's are per frame of the batch, [N*T][H][W][C]), "conv0".."conv4" (level outputs), "g1".."g4" (FCN: out0's level-l slice applied to
 * the squeezed map at low resolution, 64 channels),
 * "up3".."up0" (UNet decoder outputs).  Returns the number of floats, or a
 * negative error; with dst == NULL only the size is returned. */
int64_t ukbb_fcn_get_activation(ukbb_fcn_handle *h, const char *name, float *dst, int64_t cap);

/* Shader clock the chip holds RIGHT NOW (bench.py, next to its roofline: the MFMA peak scales with it).  Launches one wave on
 * `stream` that spins for about spin_us microseconds and compares the shader-cycle counter (s_memtime) with the constant 100 MHz
 * counter (s_memrealtime); waits for that wave only.  Run it on a stream of its own while the measured work is queued on another:
 * a single extra wave does not disturb it.  *mhz = the shader clock in MHz.  No reference counterpart (measurement only). */
int ukbb_fcn_clock_probe(int device, void *stream, int spin_us, double *mhz);

/* Synthetic subject for BASELINE.json configs[3] ("1000 synthetic subjects x 500 slices, generated on
 * device from seed = subject id"): d_out[i] = a * b / 2048 with (a, b) = the two low 12-bit fields of splitmix64's finaliser of
 * seed * 0x9E3779B97F4A7C15 + i -- exact in float32, so ukbb_cardiac_amd/synthetic_cohort.py reproduces it bit for bit in numpy
 * for the oracle.  Asynchronous on `stream`.  No reference counterpart (the reference reads sa.nii.gz, common/deploy_network.py:80-83);
 * measurement and tests only. */
int ukbb_fcn_synth_volume(uint64_t seed, size_t n, float *d_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* UKBB_FCN_H */
