"""What the engine may be run beside (r06; profiles/r06_notes.md section 10).

* No kernel depends on LDS it did not write: with every CU's LDS filled with NaN patterns in front of EVERY launch (UKBB_DEBUG_POISON_LDS) all models
  and precisions return identical bits.  "Every launch" is counted: the handle reports the launches it made and the poisons it issued
  (Engine.launch_counts), the two advance alike on every poisoned call, and the launches equal what the test expects of the path -- the plan's
  ops, the half-batch chains of the fp32 U-Net twice, the ConvLSTM x pass and time steps, the output and tiling launches, per chunk of a cine.
* Every plan is right beside another stream's work: two engines on two streams, batches in flight on both, every label map equal to the single-stream
  result -- the use INTEGRATION.md section 4 describes (one handle per stream, one thread per handle).  The bf16-storage U-Net is the case that FAILED
  (85-98 % of forwards) until round 6 padded the 16-byte buffer stores of kernels_ws.hip: hipcc leaves a VALU write of the store's data registers in
  the next issue slot when the store's soffset is an SGPR (tests/test_store_hazard.py checks the ISA for that on the CPU side).
* The half-batch chains (UKBB_SPLIT_FROM; the default for the fp32 U-Net) change no bit of a forward, fp32 or bf16.
"""
import os
import re
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _engine(model, seed=1234):
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.engine import Engine
    from ukbb_cardiac_amd.weights import synthetic_params
    arch = MODELS[model]
    return arch, Engine(arch, synthetic_params(arch, seed))


PATTERNS = ('7FC07FC0', 'FFFFFFFF', '7F800000')                      # bf16 NaN pairs, all ones, fp32 +inf


def _set_precision(eng, prec):
    """'f32x3+convs': 'f32x3' with the conv stack on three bf16 pieces as well (Engine.set_f32x3_convs)."""
    eng.set_precision(prec.split('+')[0])
    if prec.endswith('+convs'):
        eng.set_f32x3_convs(True)


def _poisoned(eng, monkeypatch, pattern, call, launches, what):
    """``call()`` under UKBB_DEBUG_POISON_LDS=pattern: one poison per launch, and ``launches`` launches (a callable: the plan exists
    after the call).  The variable is read at the start of every API call."""
    monkeypatch.setenv('UKBB_DEBUG_POISON_LDS', pattern)
    l0, p0 = eng.launch_counts()
    try:
        out = call()
    finally:
        monkeypatch.delenv('UKBB_DEBUG_POISON_LDS', raising=False)
    l1, p1 = eng.launch_counts()
    print('%s: %d launches, %d LDS poisons' % (what, l1 - l0, p1 - p0))
    assert p1 - p0 == l1 - l0 > 0, what
    assert l1 - l0 == launches(), (what, l1 - l0, launches())
    return out


def _split_ops(names):
    """The ops the half-batch chains launch twice (UKBB_SPLIT_FROM=1, the default of the fp32 U-Net at n >= 8): levels >= 1 of the
    encoder and the decoder down to up1_*, i.e. every conv<l>_* and up<l>_* op with l >= 1."""
    return sum(re.match(r'(conv|up)[1-9]\d*_', name) is not None for name in names)


def _frame_forward_under_lds_poison(model, prec, shape, split_env, monkeypatch):
    """A fresh engine, a reference forward with the variable unset, then each pattern: identical bits, one poison per launch.  Returns
    the reference.  ``split_env``: UKBB_SPLIT_FROM for the plan (None: the default)."""
    from ukbb_cardiac_amd import engine
    from ukbb_cardiac_amd.phantom import uniform_slices
    n, h, w = shape
    # the half-batch chains: the default of the fp32 U-Net (plan.cpp, layout_split_range) for batches of 8 images and more (run_plan)
    split = model == 'UNet_ao' and prec == 'fp32' and n >= 8 and split_env is None
    img = ((uniform_slices(n, h, w, seed=3)[..., 0] - 0.3) / 0.25).astype(np.float32)
    monkeypatch.delenv('UKBB_DEBUG_POISON_LDS', raising=False)
    monkeypatch.delenv('UKBB_SPLIT_FROM', raising=False)
    if split_env is not None:
        monkeypatch.setenv('UKBB_SPLIT_FROM', split_env)                     # read when the plan is built
    arch, eng = _engine(model)
    with eng:
        if prec != 'fp32':
            _set_precision(eng, prec)
        if prec == 'f32x3+convs':
            assert engine.plan_layout(arch, 'f32x3', n, h, w, f32x3_convs=True).get('conv_x3')       # the kernels_conv_x3.hip plan
        ref = eng.run(img, want_logits=True)
        names = eng.kernel_names()
        if split:
            assert _split_ops(names) == 17 and len(names) == 22, names      # conv1_0 .. conv4_1 (8), up3_t .. up1_1 (9)
        for pat in PATTERNS:
            out = _poisoned(eng, monkeypatch, pat, lambda: eng.run(img, want_logits=True),
                            lambda: len(names) + (_split_ops(names) if split else 0), (model, prec, shape, split_env, pat))
            for k in ('logits', 'prob', 'pred'):
                assert np.array_equal(out[k], ref[k]), (model, prec, pat, k)
        assert eng.kernel_names() == names
    return ref


# (9, 64, 96): n >= 8 and odd -- the fp32 U-Net's default split path with halves of 5 and 4 images
@pytest.mark.parametrize('model,prec,shape', [('FCN_sa', 'fp32', (6, 96, 112)), ('FCN_la_4ch_seg4', 'fp32', (3, 176, 208)), ('UNet_ao', 'fp32', (4, 128, 144)),
                                              ('UNet_ao', 'bf16', (10, 304, 272)), ('UNet_ao', 'bf16', (3, 64, 96)), ('FCN_sa', 'f32x3', (4, 192, 208)),
                                              ('FCN_sa', 'bf16_store', (4, 96, 112)), ('FCN_sa', 'bf16_full', (4, 96, 112)), ('FCN_la_4ch_seg4', 'bf16_full', (3, 80, 112)),
                                              ('FCN_sa', 'f32x3+convs', (4, 96, 112)), ('UNet_ao', 'fp32', (9, 64, 96))])
def test_no_kernel_reads_lds_it_did_not_write(model, prec, shape, monkeypatch):
    ref = _frame_forward_under_lds_poison(model, prec, shape, None, monkeypatch)
    if (model, prec, shape) == ('UNet_ao', 'fp32', (9, 64, 96)):
        _SPLIT_REF['split'] = ref


_SPLIT_REF = {}


def test_unsplit_fp32_unet_under_lds_poison_has_the_bits_of_the_split_plan(monkeypatch):
    """UKBB_SPLIT_FROM=0 at (9, 64, 96): whole-batch launches only, the same bits as the default plan's half-batch chains."""
    ref = _frame_forward_under_lds_poison('UNet_ao', 'fp32', (9, 64, 96), '0', monkeypatch)
    if 'split' not in _SPLIT_REF:                                            # (run on its own)
        _SPLIT_REF['split'] = _frame_forward_under_lds_poison('UNet_ao', 'fp32', (9, 64, 96), None, monkeypatch)
    for k in ('logits', 'prob', 'pred'):
        assert np.array_equal(_SPLIT_REF['split'][k], ref[k]), k


# Launches of one BiConvLSTM pass (run_bilstm, csrc/engine.cpp) over windows of T steps: ONE x pass for both directions (gx and the
# cell's first step of every frame), then per direction T - 1 launches of the fused gate conv + cell, one per further step: 1 + ndir * (T - 1)
# with ndir = 2 (the synthetic backward cell is not zero).  ukbb_fcn_forward_seq runs the plan's ops once over all n_seq * T frames, one
# pass, and one output launch (lstm_out) per step k of the windows: ops + 1 + 2 (T - 1) + T.  ukbb_fcn_forward_cine runs per CHUNK of
# windows the plan's ops over the chunk's frame run, one pass and ONE tiling launch (lstm_tile): chunks * (ops + 1 + 2 (T - 1) + 1),
# chunks = ceil(Wn / Wc) with Wn = ceil(F / time_step) window centres and Wc windows per chunk (all of them without a scratch budget).
def _bilstm_launches(T):
    return 1 + 2 * (T - 1)


def _cine_frames(F, H, W):
    from ukbb_cardiac_amd.phantom import cine_phantom
    return ((cine_phantom(F, H, W, seed=2)[..., 0] - 0.3) / 0.25).astype(np.float32)


def test_unet_lstm_cine_does_not_read_foreign_lds(monkeypatch):
    """The 13-frame cine, whole: the U-Net launches of the cine, the ConvLSTM x pass and time steps, the tiling launch."""
    monkeypatch.delenv('UKBB_DEBUG_POISON_LDS', raising=False)
    frames = _cine_frames(13, 48, 64)
    arch, eng = _engine('UNet-LSTM_ao')
    with eng:
        for prec in ('fp32', 'bf16'):
            eng.set_precision(prec)
            p0, l0 = eng.run_cine(frames)
            for pat in PATTERNS:
                p1, l1 = _poisoned(eng, monkeypatch, pat, lambda: eng.run_cine(frames),
                                   lambda: len(eng.kernel_names()) + _bilstm_launches(arch.fc) + 1, (prec, pat))
                assert np.array_equal(p0, p1, equal_nan=True) and np.array_equal(l0, l1), (prec, pat)


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('call', ['seq', 'cine_chunked'])
def test_unet_lstm_sequences_and_chunked_cines_do_not_read_foreign_lds(call, prec, monkeypatch):
    """run_seq (2, 9, 32, 48): lstm_out, one launch per step; the 13-frame cine under the minimum scratch budget: the chunked
    lstm_tile / lstm_img path, every chunk's launches poisoned."""
    from ukbb_cardiac_amd import engine
    monkeypatch.delenv('UKBB_DEBUG_POISON_LDS', raising=False)
    arch, eng = _engine('UNet-LSTM_ao')
    T = arch.fc
    with eng:
        eng.set_precision(prec)
        if call == 'seq':
            x = _cine_frames(2 * T, 32, 48).reshape(2, T, 32, 48)
            run = lambda: eng.run_seq(x, want_logits=True)
            launches = lambda: len(eng.kernel_names()) + _bilstm_launches(T) + T
        else:
            F = 13
            x = _cine_frames(F, 48, 64)
            low = engine.cine_min_scratch_bytes(arch, prec, F, 48, 64, 1)
            wc = engine.cine_chunk_windows(arch, prec, F, 48, 64, 1, low)
            assert low > 0 and 0 < wc < F                                     # really chunked
            eng.set_scratch_budget(low)
            run = lambda: dict(zip(('prob', 'pred'), eng.run_cine(x)))
            launches = lambda: -(-F // wc) * (len(eng.kernel_names()) + _bilstm_launches(T) + 1)
        ref = run()
        assert np.isfinite(ref['prob']).all() and ref['prob'].std() > 0
        for pat in PATTERNS:
            out = _poisoned(eng, monkeypatch, pat, run, launches, (call, prec, pat))
            for k in ref:
                assert np.array_equal(out[k], ref[k], equal_nan=k == 'prob'), (call, prec, pat, k)


# Temporal-UNet (t3d_forward_seq / t3d_forward_cine, csrc/engine.cpp): a sequence call is one pass of the 3-D plan over n_seq * T
# frames: ops launches.  A cine runs its Wn = ceil(F / time_step) windows in chunks of cw (all of them at these sizes, or
# UKBB_TEMPORAL_CHUNK_WINDOWS): per chunk the plan's ops and one tiling launch (t3d_tile): ceil(Wn / cw) * (ops + 1).
@pytest.mark.parametrize('prec', ['fp32', 'bf16_3d'])
@pytest.mark.parametrize('call,chunk', [('seq', None), ('cine', None), ('cine', 4)])
def test_temporal_unet_does_not_read_foreign_lds(call, chunk, prec, monkeypatch):
    from ukbb_cardiac_amd import engine
    monkeypatch.delenv('UKBB_DEBUG_POISON_LDS', raising=False)
    monkeypatch.delenv('UKBB_TEMPORAL_CHUNK_WINDOWS', raising=False)
    if chunk:
        monkeypatch.setenv('UKBB_TEMPORAL_CHUNK_WINDOWS', str(chunk))       # read by every cine call
    arch, eng = _engine('Temporal-UNet_ao')
    T = arch.fc
    with eng:
        eng.set_precision(prec)
        if call == 'seq':
            x = _cine_frames(2 * T, 32, 48).reshape(2, T, 32, 48)
            run = lambda: eng.run_seq(x, want_logits=True)
            launches = lambda: len(eng.kernel_names())
        else:
            F = 13
            x = _cine_frames(F, 32, 48)
            assert engine.cine_chunk_windows(arch, prec, F, 32, 48, 1, 0) == F      # without the variable: every window in one chunk
            run = lambda: dict(zip(('prob', 'pred'), eng.run_cine(x)))
            launches = lambda: -(-F // (chunk or F)) * (len(eng.kernel_names()) + 1)
        ref = run()
        assert np.isfinite(ref['prob']).all() and ref['prob'].std() > 0
        for pat in PATTERNS:
            out = _poisoned(eng, monkeypatch, pat, run, launches, (call, chunk, prec, pat))
            for k in ref:
                assert np.array_equal(out[k], ref[k], equal_nan=k == 'prob'), (call, chunk, prec, pat, k)


def test_unpoisoned_calls_count_launches_and_no_poison(monkeypatch):
    """With the variable unset nothing is enqueued in front of a launch: the poison count stays where it was."""
    monkeypatch.delenv('UKBB_DEBUG_POISON_LDS', raising=False)
    arch, eng = _engine('FCN_sa')
    with eng:
        assert eng.launch_counts() == (0, 0)
        img = _cine_frames(2, 32, 48)
        eng.run(img)
        assert eng.launch_counts() == (len(eng.kernel_names()), 0)
        _poisoned(eng, monkeypatch, PATTERNS[0], lambda: eng.run(img), lambda: len(eng.kernel_names()), 'FCN_sa')
        eng.run(img)
        assert eng.launch_counts() == (3 * len(eng.kernel_names()), len(eng.kernel_names()))


@pytest.mark.parametrize('model,prec,shape,split', [('FCN_sa', 'fp32', (32, 192, 208), None), ('UNet_ao', 'fp32', (10, 304, 272), None), ('UNet_ao', 'fp32', (10, 304, 272), '0'),
                                                    ('UNet_ao', 'bf16', (10, 304, 272), None), ('UNet_ao', 'bf16', (24, 256, 256), '1'), ('FCN_sa', 'bf16', (32, 192, 208), None),
                                                    ('UNet-LSTM_ao', 'fp32', (12, 96, 128), None), ('UNet-LSTM_ao', 'bf16', (20, 128, 160), None)])
def test_plans_are_right_beside_another_streams_work(model, prec, shape, split):
    import subprocess
    n, h, w = shape
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''), PREC=prec)
    env.pop('UKBB_SPLIT_FROM', None)
    if split is not None:
        env['UKBB_SPLIT_FROM'] = split
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'two_stream_check.py'), model, str(n), str(h), str(w), '40' if model.startswith('UNet-LSTM') else '120'], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == 'OK', r.stdout[-2000:]


def test_half_batch_chains_change_no_bit_of_a_forward(monkeypatch):
    """UKBB_SPLIT_FROM=k (default 1 for the fp32 U-Net, 0 otherwise): U-Net levels >= k as two half-batch launches per op on two streams -- odd and
    even batches, a batch below the split threshold; fp32 and bf16 storage."""
    from ukbb_cardiac_amd.phantom import cine_phantom
    for prec in ('fp32', 'bf16'):
        for n, H, W in ((9, 64, 96), (16, 128, 128), (3, 48, 80)):
            img = ((cine_phantom(n, H, W, seed=n)[..., 0] - 0.3) / 0.25).astype(np.float32)
            outs = {}
            for tag in ('0', '1', '2', None):
                if tag is None:
                    monkeypatch.delenv('UKBB_SPLIT_FROM', raising=False)
                else:
                    monkeypatch.setenv('UKBB_SPLIT_FROM', tag)
                arch, eng = _engine('UNet_ao', 77)
                with eng:
                    eng.set_precision(prec)
                    outs[tag] = eng.run(img, want_logits=True)
            for tag in ('1', '2', None):
                for k in ('logits', 'prob', 'pred'):
                    assert np.array_equal(outs['0'][k], outs[tag][k]), (prec, n, H, W, tag, k)


def test_fp32_temporal_unet_on_two_streams_one_engine_per_thread():
    """tools/two_stream_check.py sends a Temporal-UNet through the frame forward, which that model refuses: here two engines run whole
    cines (F = 12, 64 x 64, six in flight per stream, one thread per handle) and every label map equals the single-stream result."""
    import torch
    arch = None
    F, H, W, rounds = 12, 64, 64, 6
    dev = torch.device('cuda', 0)
    xs = [torch.from_numpy(np.random.default_rng(30 + i).standard_normal((F, H, W)).astype(np.float32)).to(dev) for i in range(2)]
    engs = []
    try:
        for _ in range(2):
            arch, eng = _engine('Temporal-UNet_ao')
            engs.append(eng)
        probs = [torch.empty((F, H, W, arch.n_class), dtype=torch.float32, device=dev) for _ in range(2)]
        refs = []
        for i in range(2):                                               # single-stream references
            p = torch.empty((F, H, W), dtype=torch.int32, device=dev)
            engs[i].run_cine_device(xs[i].data_ptr(), F, H, W, probs[i].data_ptr(), p.data_ptr())
            torch.cuda.synchronize()
            refs.append(p.clone())
        streams = [torch.cuda.Stream(dev) for _ in range(2)]
        preds = [[torch.empty((F, H, W), dtype=torch.int32, device=dev) for _ in range(rounds)] for _ in range(2)]
        errors = []

        def work(i):
            try:
                for k in range(rounds):                                  # `rounds` cines in flight on this thread's stream
                    engs[i].run_cine_device(xs[i].data_ptr(), F, H, W, probs[i].data_ptr(), preds[i][k].data_ptr(), stream=streams[i].cuda_stream)
            except Exception as exc:                                     # noqa: BLE001 -- reported by the main thread
                errors.append(exc)
        threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        torch.cuda.synchronize()
        assert not errors, errors
        for i in range(2):
            assert len(torch.unique(refs[i])) > 1
            for k in range(rounds):
                assert int((preds[i][k] != refs[i]).sum()) == 0, (i, k)
    finally:
        for e in engs:
            e.close()
