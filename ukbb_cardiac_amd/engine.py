"""Python face of the HIP engine: ``Engine`` (one model bound to one GPU) and
``Session``, which mirrors the slice of ``tf.Session`` the reference deploy
scripts use (``common/deploy_network.py:44-49,110-111``)."""
import ctypes as C
import os
from typing import Dict, Optional, Sequence

import numpy as np

from . import _lib
from .arch import KIND_TEMPORAL_UNET, ModelArch, MODELS
from .weights import Params, load_blob, pack_flat, synthetic_params

MODEL_EXT = '.ukbbw'


class Engine:
    """One network on one device.  Host-array entry point ``run`` is the
    ``sess.run`` equivalent; ``run_device`` takes raw device pointers
    (e.g. ``torch.Tensor.data_ptr()``) and a HIP stream handle."""

    def __init__(self, arch: ModelArch, params: Params, device: int = 0):
        self.arch = arch
        flat = np.ascontiguousarray(pack_flat(arch, params), dtype=np.float32)
        a = _lib.arch_struct(arch)
        want = _lib.lib.ukbb_fcn_weight_count(C.byref(a))
        if want != flat.size:
            raise _lib.UkbbFcnError('weight count mismatch: library expects %d floats, got %d' % (want, flat.size))
        self._h = _lib.lib.ukbb_fcn_create(C.byref(a), _lib.f32ptr(flat), flat.size, int(device))
        if not self._h:
            raise _lib.UkbbFcnError('ukbb_fcn_create failed: ' + _lib.last_error())
        self.device = int(device)

    def close(self):
        if getattr(self, '_h', None):
            _lib.lib.ukbb_fcn_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- host arrays -----------------------------------------------------------
    def run(self, image: np.ndarray, want_logits=False, want_prob=True, want_pred=True):
        """image: float32 [N,H,W,1] (or [N,H,W]).  Returns dict with the
        requested 'logits' [N,H,W,C] f32, 'prob' [N,H,W,C] f32, 'pred' [N,H,W] int32."""
        x = np.ascontiguousarray(image, dtype=np.float32)
        if x.ndim == 4:
            if x.shape[3] != 1:
                raise ValueError('image must have a single channel, got shape %s' % (x.shape,))
            x = x[..., 0]
        if x.ndim != 3:
            raise ValueError('image must be [N,H,W,1], got shape %s' % (image.shape,))
        n, h, w = x.shape
        c = self.arch.n_class
        out: Dict[str, np.ndarray] = {}
        lg = np.empty((n, h, w, c), np.float32) if want_logits else None
        pr = np.empty((n, h, w, c), np.float32) if want_prob else None
        pd = np.empty((n, h, w), np.int32) if want_pred else None
        rc = _lib.lib.ukbb_fcn_forward_host(
            self._h, _lib.f32ptr(x), n, h, w,
            _lib.f32ptr(lg) if lg is not None else None,
            _lib.f32ptr(pr) if pr is not None else None,
            _lib.i32ptr(pd) if pd is not None else None)
        _lib.check(rc, 'ukbb_fcn_forward_host')
        if lg is not None:
            out['logits'] = lg
        if pr is not None:
            out['prob'] = pr
        if pd is not None:
            out['pred'] = pd
        return out

    # -- device pointers -------------------------------------------------------
    def reserve(self, n, h, w):
        _lib.check(_lib.lib.ukbb_fcn_reserve(self._h, n, h, w), 'ukbb_fcn_reserve')

    def run_device(self, image_ptr: int, n: int, h: int, w: int, logits_ptr: int = 0, prob_ptr: int = 0,
                   pred_ptr: int = 0, stream: int = 0):
        rc = _lib.lib.ukbb_fcn_forward(self._h, C.c_void_p(image_ptr), n, h, w,
                                       C.c_void_p(logits_ptr or None), C.c_void_p(prob_ptr or None),
                                       C.c_void_p(pred_ptr or None), C.c_void_p(stream or None))
        _lib.check(rc, 'ukbb_fcn_forward')

    # -- UNet-LSTM (aortic default model) and Temporal-UNet -------------------------------
    def run_seq(self, image: np.ndarray, want_logits=False, want_prob=True, want_pred=True):
        """The reference's ``sess.run('prob:0', {'image:0': image_idx})`` for the UNet-LSTM or Temporal-UNet graph
        (common/deploy_network_ao.py:171-172): image float32 [N,T,H,W,1] (or [N,T,H,W]) with T = arch.n_step
        -> 'prob' [N,T,H,W,C], 'pred' [N,T,H,W], optionally 'logits'.  Host arrays; staged through torch tensors."""
        import torch
        x = np.ascontiguousarray(image, dtype=np.float32)
        if x.ndim == 5:
            x = x[..., 0]
        if x.ndim != 4 or x.shape[1] != self.arch.n_step:
            raise ValueError('image must be [N,%d,H,W,1], got shape %s' % (self.arch.n_step, image.shape))
        n, t, h, w = x.shape
        c = self.arch.n_class
        dev = torch.device('cuda', self.device)
        stream = torch.cuda.current_stream(dev).cuda_stream
        xd = torch.from_numpy(x).to(dev)
        lg = torch.empty((n, t, h, w, c), dtype=torch.float32, device=dev) if want_logits else None
        pr = torch.empty((n, t, h, w, c), dtype=torch.float32, device=dev) if (want_prob or True) else None
        pd = torch.empty((n, t, h, w), dtype=torch.int32, device=dev) if want_pred else None
        rc = _lib.lib.ukbb_fcn_forward_seq(self._h, C.c_void_p(xd.data_ptr()), n, h, w,
                                           C.c_void_p(lg.data_ptr() if lg is not None else None),
                                           C.c_void_p(pr.data_ptr()), C.c_void_p(pd.data_ptr() if pd is not None else None),
                                           C.c_void_p(stream or None))
        _lib.check(rc, 'ukbb_fcn_forward_seq')
        out: Dict[str, np.ndarray] = {}
        if want_logits:
            out['logits'] = lg.cpu().numpy()
        if want_prob:
            out['prob'] = pr.cpu().numpy()
        if want_pred:
            out['pred'] = pd.cpu().numpy()
        return out

    def run_seq_device(self, image_ptr: int, n: int, h: int, w: int, logits_ptr: int = 0, prob_ptr: int = 0, pred_ptr: int = 0, stream: int = 0):
        """``run_seq`` on device pointers (image [N,T,H,W] float32; logits / prob [N,T,H,W,C] float32, pred [N,T,H,W] int32, each
        optional), asynchronous on ``stream``."""
        rc = _lib.lib.ukbb_fcn_forward_seq(self._h, C.c_void_p(image_ptr), int(n), int(h), int(w), C.c_void_p(logits_ptr or None),
                                           C.c_void_p(prob_ptr or None), C.c_void_p(pred_ptr or None), C.c_void_p(stream or None))
        _lib.check(rc, 'ukbb_fcn_forward_seq')

    def run_cine(self, frames: np.ndarray, weight_R: int = 5, weight_r: float = 0.1, time_step: int = 1):
        """One slice position of the 'UNet-LSTM' / 'Temporal-UNet' branch of common/deploy_network_ao.py:129-183,189: frames
        float32 [F,H,W] (normalised, padded) -> (prob [F,H,W,C] float32, pred [F,H,W] int32), circular windows centred
        on frames range(0, F, time_step) tiled on the device (UNet-LSTM: the U-Net features of each frame are computed once;
        Temporal-UNet: every window runs the 3-D network, in chunks of windows)."""
        import torch
        x = np.ascontiguousarray(frames, dtype=np.float32)
        if x.ndim != 3:
            raise ValueError('frames must be [F,H,W], got shape %s' % (frames.shape,))
        f, h, w = x.shape
        dev = torch.device('cuda', self.device)
        stream = torch.cuda.current_stream(dev).cuda_stream
        xd = torch.from_numpy(x).to(dev)
        pr = torch.empty((f, h, w, self.arch.n_class), dtype=torch.float32, device=dev)
        pd = torch.empty((f, h, w), dtype=torch.int32, device=dev)
        rc = _lib.lib.ukbb_fcn_forward_cine(self._h, C.c_void_p(xd.data_ptr()), f, h, w, int(weight_R), float(weight_r), int(time_step),
                                            C.c_void_p(pr.data_ptr()), C.c_void_p(pd.data_ptr()), C.c_void_p(stream or None))
        _lib.check(rc, 'ukbb_fcn_forward_cine')
        return pr.cpu().numpy(), pd.cpu().numpy()

    def run_cine_device(self, frames_ptr, f, h, w, prob_ptr, pred_ptr, weight_R=5, weight_r=0.1, time_step=1, stream=0):
        """``run_cine`` on device pointers (frames [F,H,W] float32, prob [F,H,W,C] float32, pred [F,H,W] int32), asynchronous on
        ``stream``: the form device_pipeline.aortic_sequence_device uses."""
        rc = _lib.lib.ukbb_fcn_forward_cine(self._h, C.c_void_p(frames_ptr), int(f), int(h), int(w), int(weight_R), float(weight_r),
                                            int(time_step), C.c_void_p(prob_ptr), C.c_void_p(pred_ptr or None), C.c_void_p(stream or None))
        _lib.check(rc, 'ukbb_fcn_forward_cine')

    def set_precision(self, precision: str):
        """'fp32' (default), 'bf16' (bf16 MFMA inputs, fp32 accumulate; BASELINE config 5), 'f32x3' (fp32 results from three
        bf16 pieces per operand on the dense matrix cores: the FCN head, and with ``set_f32x3_convs(True)`` the FCN's 3x3 conv stack; include/ukbb_fcn.h UKBB_PREC_F32X3), 'bf16_store'
        (FCN models only: bf16 operands and bf16 encoder maps in HBM, squeeze and head in fp32; UKBB_PREC_BF16_STORE), 'bf16_full'
        (FCN models only: 'bf16_store' with the head's three matrix products on the bf16 matrix instruction as well -- weights rounded
        once when packed, the two hidden activations once in registers; biases, the G_l maps, accumulators, logits, prob and pred
        fp32; UKBB_PREC_BF16_FULL) or 'bf16_3d'
        (Temporal-UNet only: its 3-D convolutions on the bf16 matrix instruction, every 3-D map bf16 in HBM, the first layer's
        arithmetic, logits, prob and pred fp32; UKBB_PREC_BF16_3D.  'bf16' and 'bf16_store' stay refused on that model)."""
        _lib.check(_lib.lib.ukbb_fcn_set_precision(self._h, _PLAN_PREC[precision]), 'ukbb_fcn_set_precision')

    def set_f32x3_convs(self, on: bool):
        """FCN models only, off by default: under 'f32x3' run the eleven 3x3 layers conv1_0 .. conv4_2 on three bf16 pieces per operand as
        well (include/ukbb_fcn.h ukbb_fcn_set_f32x3_convs): fp32 maps in HBM, six bf16 matrix instructions per tap and 16-channel chunk into
        one fp32 accumulator, fp32 bias / ReLU / store.  Stored on the handle; kept and ignored under any other precision."""
        _lib.check(_lib.lib.ukbb_fcn_set_f32x3_convs(self._h, int(bool(on))), 'ukbb_fcn_set_f32x3_convs')

    def set_scratch_budget(self, nbytes: int):
        """Bound the device memory ``run_cine`` / ``run_cine_device`` may hold for their per-cine scratch (0 = no budget, the default):
        the windows then run in chunks, bit-identical to the unchunked call (include/ukbb_fcn.h, ukbb_fcn_set_scratch_budget)."""
        if nbytes < 0:
            raise ValueError('scratch budget must be >= 0 bytes, got %r' % (nbytes,))
        _lib.check(_lib.lib.ukbb_fcn_set_scratch_budget(self._h, int(nbytes)), 'ukbb_fcn_set_scratch_budget')

    def scratch_bytes(self) -> int:
        """Bytes of device memory the handle holds right now in its activation and cine buffers (weights excluded)."""
        return int(_lib.lib.ukbb_fcn_scratch_bytes(self._h))

    # -- guarded, poisonable buffers (debugging aid: engines created with UKBB_DEBUG_GUARD=<hex pattern> in the environment) ----------
    def check_guards(self):
        """Waits for the device and reads the guards on either side of every device buffer of the handle.  Returns
        ``(damaged, report)``: the number of buffers with a damaged guard and one line ``<buffer> <front|back> <first> <last>`` per
        damaged guard (byte offsets from the payload's start)."""
        buf = C.create_string_buffer(1 << 14)
        bad = _lib.check(_lib.lib.ukbb_fcn_debug_check_guards(self._h, buf, len(buf)), 'ukbb_fcn_debug_check_guards')
        return bad, buf.value.decode()

    def guard_info(self):
        """``(buffers, payload_bytes, guard_bytes)`` of the guarded buffers the handle holds right now."""
        pay, gb = C.c_uint64(0), C.c_uint64(0)
        nb = _lib.check(_lib.lib.ukbb_fcn_debug_guard_info(self._h, C.byref(pay), C.byref(gb)), 'ukbb_fcn_debug_guard_info')
        return nb, int(pay.value), int(gb.value)

    def poison(self, pattern) -> int:
        """Fill every buffer the engine rewrites on each call (activation maps, ConvLSTM / cine working buffers, output staging) with
        the 32-bit ``pattern`` (int or hex string); returns how many were filled."""
        pat = int(pattern, 16) if isinstance(pattern, str) else int(pattern)
        return _lib.check(_lib.lib.ukbb_fcn_debug_poison(self._h, pat & 0xFFFFFFFF), 'ukbb_fcn_debug_poison')

    def damage_guard(self, buffer: str, offset: int):
        """Write one byte into a guard of ``buffer`` (a name as ``check_guards`` reports it) at ``offset`` bytes from its payload's
        start -- inside the buffer's own allocation; shows that ``check_guards`` sees damage."""
        _lib.check(_lib.lib.ukbb_fcn_debug_damage_guard(self._h, buffer.encode(), int(offset)), 'ukbb_fcn_debug_damage_guard')

    def launch_counts(self):
        """``(launches, lds_poisons)`` since the handle was created: every kernel launch a forward of this handle made (a plan op
        that ran as two half-batch launches counts twice; the ConvLSTM, output and tiling launches count too) and the LDS poison
        launches issued in front of them under ``UKBB_DEBUG_POISON_LDS`` -- a call with the variable set advances both alike."""
        out = (C.c_uint64 * 2)()
        _lib.check(_lib.lib.ukbb_fcn_debug_launch_counts(self._h, C.byref(out)), 'ukbb_fcn_debug_launch_counts')
        return int(out[0]), int(out[1])

    # -- measurement -----------------------------------------------------------
    def kernel_names(self):
        n = _lib.lib.ukbb_fcn_num_kernels(self._h)
        return [_lib.lib.ukbb_fcn_kernel_name(self._h, i).decode() for i in range(n)]

    def kernel_macs(self):
        n = _lib.lib.ukbb_fcn_num_kernels(self._h)
        return [_lib.lib.ukbb_fcn_kernel_macs(self._h, i) for i in range(n)]

    def kernel_mfma_macs(self):
        """Multiplies each kernel issues to the matrix pipe (Winograd / head algebra run fewer than the
        reference graph's algorithmic count returned by kernel_macs)."""
        n = _lib.lib.ukbb_fcn_num_kernels(self._h)
        return [_lib.lib.ukbb_fcn_kernel_mfma_macs(self._h, i) for i in range(n)]

    def kernel_mfma_macs_issued(self):
        """MACs each launch issues to the matrix pipe INCLUDING tile / Winograd-region padding (= SQ_INSTS_MFMA x MACs per instruction)."""
        n = _lib.lib.ukbb_fcn_num_kernels(self._h)
        return [_lib.lib.ukbb_fcn_kernel_mfma_macs_issued(self._h, i) for i in range(n)]

    def kernel_configs(self):
        n = _lib.lib.ukbb_fcn_num_kernels(self._h)
        return [_lib.lib.ukbb_fcn_kernel_config(self._h, i) for i in range(n)]

    def set_timing(self, enable: bool):
        _lib.check(_lib.lib.ukbb_fcn_set_timing(self._h, int(enable)), 'ukbb_fcn_set_timing')

    def set_timing_kernel(self, index: int):
        _lib.check(_lib.lib.ukbb_fcn_set_timing_kernel(self._h, int(index)), 'ukbb_fcn_set_timing_kernel')

    def kernel_times(self, reset=True):
        n = _lib.lib.ukbb_fcn_num_kernels(self._h)
        ms = (C.c_double * n)()
        cnt = (C.c_int64 * n)()
        _lib.check(_lib.lib.ukbb_fcn_kernel_times(self._h, ms, cnt, n, int(reset)), 'ukbb_fcn_kernel_times')
        return list(ms), list(cnt)

    def activation(self, name: str) -> np.ndarray:
        n = _lib.lib.ukbb_fcn_get_activation(self._h, name.encode(), None, 0)
        _lib.check(int(n), 'ukbb_fcn_get_activation')
        buf = np.empty(int(n), np.float32)
        _lib.check(int(_lib.lib.ukbb_fcn_get_activation(self._h, name.encode(), _lib.f32ptr(buf), n)),
                   'ukbb_fcn_get_activation')
        return buf


_PREC = {'fp32': 0, 'bf16': 1, 'bf16_3d': 4}   # what the cine queries take: any other name is a KeyError


def cine_scratch_bytes(arch: ModelArch, precision: str, n_frames: int, height: int, width: int, time_step: int = 1, budget: int = 0) -> int:
    """Device bytes ``Engine.run_cine`` allocates for this call under ``budget`` (0 = none) on a fresh engine; 0 for a malformed
    request or a budget below the minimum.  Host arithmetic only (ukbb_fcn_cine_scratch_bytes): the engine plans with the same function."""
    a = _lib.arch_struct(arch)
    return int(_lib.lib.ukbb_fcn_cine_scratch_bytes(C.byref(a), _PREC[precision], int(n_frames), int(height), int(width), int(time_step), int(budget)))


def cine_min_scratch_bytes(arch: ModelArch, precision: str, n_frames: int, height: int, width: int, time_step: int = 1) -> int:
    """The smallest non-zero scratch budget ``run_cine`` accepts for this call (0: malformed request)."""
    a = _lib.arch_struct(arch)
    return int(_lib.lib.ukbb_fcn_cine_min_scratch_bytes(C.byref(a), _PREC[precision], int(n_frames), int(height), int(width), int(time_step)))


def cine_chunk_windows(arch: ModelArch, precision: str, n_frames: int, height: int, width: int, time_step: int = 1, budget: int = 0) -> int:
    """Windows per chunk ``run_cine`` uses under ``budget`` (all of them when unchunked; 0: malformed or below the minimum)."""
    a = _lib.arch_struct(arch)
    return int(_lib.lib.ukbb_fcn_cine_chunk_windows(C.byref(a), _PREC[precision], int(n_frames), int(height), int(width), int(time_step), int(budget)))


_PLAN_PREC = {'fp32': 0, 'bf16': 1, 'f32x3': 2, 'bf16_store': 3, 'bf16_3d': 4, 'bf16_full': 5}       # the UKBB_PREC_* codes of include/ukbb_fcn.h (set_precision, plan_layout)
_OP_FIELDS = ('cfg', 'H', 'W', 'Ho', 'Wo', 'stride', 'in0', 'in1', 'out')


def plan_layout(arch: ModelArch, precision: str, n: int, h: int, w: int, cus: int = 256, f32x3_convs: bool = False) -> dict:
    """The launch plan the engine builds for batches of ``n`` images of ``h`` x ``w`` on a device of ``cus`` compute units, from
    the host-only planner (no GPU needed): ``{'ops': [dict], 'acts': [dict], 'split': (first, last), 'bfio', 'feat_buf', 'lstm', 'head_bf16'}``.
    An op's ``macs`` / ``mfma_macs`` / ``issued_macs`` are per image, as ``Engine.kernel_macs()`` etc. report them per batch.
    A map of the workspace takes ``per_image * bytes_per_element`` bytes per image.
    ``f32x3_convs``: the plan of an engine with ``set_f32x3_convs(True)``; where it takes effect (an FCN model under 'f32x3') the dict
    also holds ``'conv_x3': True``.
    Raises UkbbFcnError where ``Engine`` would refuse the combination."""
    a = _lib.arch_struct(arch)
    if f32x3_convs:
        fn = _lib.lib.ukbb_fcn_debug_plan_layout_x3              # the same text for a handle with the switch on
        fn.argtypes = [C.POINTER(_lib.ArchStruct)] + [C.c_int] * 6 + [C.c_char_p, C.c_size_t]
        args = (C.byref(a), _PLAN_PREC[precision], 1, int(n), int(h), int(w), int(cus))
    else:
        fn = _lib.lib.ukbb_fcn_debug_plan_layout                 # debugging aid: not part of the public header
        fn.argtypes = [C.POINTER(_lib.ArchStruct)] + [C.c_int] * 5 + [C.c_char_p, C.c_size_t]
        args = (C.byref(a), _PLAN_PREC[precision], int(n), int(h), int(w), int(cus))
    buf = C.create_string_buffer(1 << 16)
    got = _lib.check(fn(*args, buf, len(buf)), 'ukbb_fcn_debug_plan_layout')
    if got >= len(buf):
        buf = C.create_string_buffer(got + 1)
        _lib.check(fn(*args, buf, len(buf)), 'ukbb_fcn_debug_plan_layout')
    out = {'ops': [], 'acts': []}
    for line in buf.value.decode().splitlines():
        f = line.split(' ')
        if f[0] == 'op':
            op = {'name': f[2], 'kind': f[3]}
            op.update(zip(_OP_FIELDS, map(int, f[4:13])))
            macs, mfma, issued = map(float, f[13:16])
            mfma = macs if mfma < 0 else mfma                    # -1: same as the figure before it
            op.update(macs=macs, mfma_macs=mfma, issued_macs=mfma if issued < 0 else issued)
            out['ops'].append(op)
        elif f[0] == 'act':
            out['acts'].append({'name': '' if f[1] == '-' else f[1], 'per_image': int(f[2]), 'channels': int(f[3]),
                                'bytes_per_element': int(f[4]) if len(f) > 4 else 4})       # (a library built before the field existed: floats)
        elif f[0] == 'plan':
            v = list(map(int, f[2:4] + f[5:6] + f[7:8] + f[9:13]))
            out.update(split=(v[0], v[1]), bfio=bool(v[2]), feat_buf=v[3],
                       lstm={'needed': bool(v[4]), 'tile_cols': v[5], 'bf_wino': bool(v[6]), 'bf_hoist': bool(v[7])})
            out['head_bf16'] = len(f) > 14 and f[13] == 'head_bf16' and bool(int(f[14]))      # UKBB_PREC_BF16_FULL: the head on bf16 MFMA
            if len(f) > 16 and f[15] == 'conv_x3' and int(f[16]):                             # only a plan that has it
                out['conv_x3'] = True
    return out


def load_model(model_path: str):
    """Resolve the reference's ``--model_path`` (a TF checkpoint prefix,
    ``demo_pipeline.py:63``): this repo's weight blob ``<model_path>.ukbbw`` if present, else the
    checkpoint-V2 files themselves (``tf_checkpoint.py``)."""
    for cand in (model_path, model_path + MODEL_EXT):
        if os.path.isfile(cand):
            try:
                return load_blob(cand)
            except ValueError:
                continue
    # the reference's own format: a TF checkpoint-V2 prefix (deploy_network.py:48-49)
    from . import tf_checkpoint
    if tf_checkpoint.is_checkpoint(model_path):
        return tf_checkpoint.checkpoint_to_params(model_path)
    raise FileNotFoundError(
        'no weight blob at %s%s and no TF checkpoint at %s.index (convert with '
        '`python -m ukbb_cardiac_amd.tf_checkpoint %s`)' % (model_path, MODEL_EXT, model_path, model_path))


class Session:
    """The slice of ``tf.Session`` the deploy scripts touch.

    Reference usage (``common/deploy_network.py:44-49,110-111``)::

        with tf.Session() as sess:
            saver = tf.train.import_meta_graph(model_path + '.meta'); saver.restore(sess, model_path)
            prob, pred = sess.run(['prob:0', 'pred:0'], feed_dict={'image:0': x, 'training:0': False})

    Here ``Session(model_path)`` binds the model and ``run`` accepts exactly those
    tensor names (``common/train_network.py:142,151,198,199``); anything else
    raises, as TF would for an unknown tensor.
    """

    FETCHABLE = ('prob:0', 'pred:0', 'logits:0')

    def __init__(self, model_path: Optional[str] = None, arch: Optional[ModelArch] = None,
                 params: Optional[Params] = None, device: int = 0):
        if model_path is not None:
            arch, params = load_model(model_path)
        if arch is None or params is None:
            raise ValueError('Session needs model_path or (arch, params)')
        self.engine = Engine(arch, params, device)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        self.engine.close()

    def run(self, fetches, feed_dict):
        single = isinstance(fetches, str)
        names: Sequence[str] = [fetches] if single else list(fetches)
        for f in names:
            if f not in self.FETCHABLE:
                raise KeyError('unknown tensor %r (fetchable: %s)' % (f, ', '.join(self.FETCHABLE)))
        for k in feed_dict:
            if k not in ('image:0', 'training:0'):
                raise KeyError('unknown placeholder %r' % (k,))
        if 'image:0' not in feed_dict:
            raise KeyError("feed_dict lacks 'image:0'")
        if feed_dict.get('training:0', False):
            raise ValueError("'training:0' must be False: only the inference graph (BN moving statistics) exists")
        run = self.engine.run
        if self.engine.arch.kind == KIND_TEMPORAL_UNET:   # image:0 is NTXYC: softmax / argmax of every frame of every window (network_ao.py:159-160)
            run = self.engine.run_seq
        out = run(feed_dict['image:0'], want_logits='logits:0' in names,
                  want_prob='prob:0' in names, want_pred='pred:0' in names)
        res = [out[f.split(':')[0]] for f in names]
        return res[0] if single else res
