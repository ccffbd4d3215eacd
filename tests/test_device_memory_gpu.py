"""Does every launch touch only the device memory it owns, and does it write all of what it owns?

The engine's buffers only grow (DevBuf::ensure, csrc/engine.cpp): a handle runs a small shape inside buffers a larger shape filled, a tail
batch inside a batch-64 buffer, and what lies behind and beside the current map is finite data of the previous run.  A kernel that loads it
and masks it gives the bits of a correct kernel; a kernel that leaves part of a map unwritten passes whenever the previous call left the
right values there; a ragged tile that stores a row too far lands in hipMalloc slack or in a neighbouring allocation.  No parity test sees
any of that.  Here handles created under UKBB_DEBUG_GUARD=<hex pattern> allocate every buffer as guard | payload | guard (1 MiB guards),
fill a payload with the pattern when it is allocated, and ``Engine.poison(p)`` refills everything the engine rewrites per call:

  a. first use of fresh memory: a guarded and a plain handle in one process, every model and precision, ragged shapes -> identical bits;
  b. small after large on one handle, a tail batch in a kept plan, each pattern -> the bits of a fresh plain handle that ran only that case
     (frame batches, and sequences through run_seq);
  c. precision switches on one handle, at one shape and with a shape change (bf16 maps take 2 bytes per channel, fp32 maps 4: the stale
     bytes are of the other element size);
  d. cines (UNet-LSTM whole and in chunks under the minimum scratch budget, Temporal-UNet fp32 and bf16_3d in chunks of one window,
     unchunked and under a scratch budget);
  e. the instrument itself: the poison is read back, a damaged guard is reported with buffer and offset;
  f. caller-owned outputs of the device-pointer forwards (frame, sequence, cine) and of the pre- / post-processing entries, carved from
     the middle of larger tensors filled with a sentinel: nothing beside an output changes, everything the entry's contract covers is written.

A precision is a tag: the names Engine.set_precision takes, and 'f32x3+convs' for 'f32x3' with set_f32x3_convs(True).  The switch is stored
on the handle and the module's guarded engines are shared, so every tag sets it (_set_precision).

No tolerance anywhere: bits, and guard bytes."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PATTERNS = ('7FC07FC0', 'FFFFFFFF', '7F800000')                   # bf16 NaN pairs, all ones, fp32 +inf (as tests/test_concurrency_gpu.py)
FRAME_MODELS = ['FCN_sa', 'FCN_la_2ch', 'FCN_la_4ch', 'FCN_la_4ch_seg4', 'UNet_ao']
PRECISIONS = {m: ('fp32', 'bf16', 'f32x3') + (('f32x3+convs', 'bf16_store', 'bf16_full') if m.startswith('FCN') else ()) for m in FRAME_MODELS + ['UNet-LSTM_ao']}
PRECISIONS['Temporal-UNet_ao'] = ('fp32', 'f32x3', 'bf16_3d')
# ascending in pixels, so that the staging buffers of a handle are re-allocated (fresh, poisoned) by every case; 16 and 17 images of
# 64 x 96 lie on either side of the planner's small-batch threshold (plan.h, SMALL_BATCH = 16), and 16 comes first: a handle leaves the
# small-batch plans for good with the first larger batch it sees
FRAME_SHAPES = [(1, 16, 16), (3, 80, 112), (2, 48, 400), (16, 64, 96), (17, 64, 96), (2, 272, 304)]
SEQ_SHAPES = [(1, 9, 32, 48), (2, 9, 48, 80)]
LARGE = (17, 272, 304)


@functools.lru_cache(maxsize=None)
def _params(model):
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.weights import synthetic_params
    return synthetic_params(MODELS[model], 1234)


def _engine(model, guard=None):
    """A fresh engine: guarded and poisoned with the hex pattern ``guard``, or plain (None).  The variable is read in ukbb_fcn_create only."""
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.engine import Engine
    old = os.environ.pop('UKBB_DEBUG_GUARD', None)
    try:
        if guard is not None:
            os.environ['UKBB_DEBUG_GUARD'] = guard
        return Engine(MODELS[model], _params(model))
    finally:
        os.environ.pop('UKBB_DEBUG_GUARD', None)
        if old is not None:
            os.environ['UKBB_DEBUG_GUARD'] = old


@pytest.fixture(scope='module')
def guarded():
    """One guarded engine per model for the whole module (created on first use)."""
    made = {}

    def get(model):
        if model not in made:
            made[model] = _engine(model, PATTERNS[0])
        return made[model]
    yield get
    for eng in made.values():
        eng.close()


@functools.lru_cache(maxsize=None)
def _image(shape):
    rng = np.random.default_rng(sum(shape) + 7 * len(shape))
    return rng.standard_normal(shape).astype(np.float32)


def _set_precision(eng, tag):
    from ukbb_cardiac_amd.arch import KIND_FCN
    eng.set_precision(tag.split('+')[0])
    if eng.arch.kind == KIND_FCN:                                  # (the other kinds refuse the switch)
        eng.set_f32x3_convs(tag.endswith('+convs'))


def _run(eng, shape):
    img = _image(shape)
    return eng.run_seq(img, want_logits=True) if len(shape) == 4 else eng.run(img, want_logits=True)


def _same_bits(got, want, what):
    for k in ('logits', 'prob', 'pred'):
        assert got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), what + (k,)


def _guards_intact(eng, what):
    bad, report = eng.check_guards()
    assert bad == 0, (what, report)


_REF = {}


def _fresh_plain(model, prec, shape):
    """What a fresh plain handle that ran only this case returns (computed once, shared, never modified)."""
    key = (model, prec, shape)
    if key not in _REF:
        with _engine(model) as eng:
            _set_precision(eng, prec)
            out = _run(eng, shape)
        for v in out.values():
            v.setflags(write=False)
        _REF[key] = out
    return _REF[key]


# ---- a. first use of fresh memory ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('model,prec', [(m, p) for m in FRAME_MODELS + ['UNet-LSTM_ao', 'Temporal-UNet_ao'] for p in PRECISIONS[m]])
def test_first_use_of_fresh_memory(model, prec):
    """Every payload of the guarded handle holds NaN pairs when a launch first sees it; the plain handle beside it runs the same calls.
    Fresh handles (not the module's): the small-batch plans exist only on a handle that never saw more than 16 images."""
    shapes = FRAME_SHAPES if model in FRAME_MODELS else SEQ_SHAPES
    with _engine(model, PATTERNS[0]) as g, _engine(model) as p:
        with pytest.raises(Exception, match='UKBB_DEBUG_GUARD'):
            p.check_guards()                                       # the plain handle really is plain
        for eng in (g, p):
            _set_precision(eng, prec)
        for shape in shapes:
            got, want = _run(g, shape), _run(p, shape)
            _same_bits(got, want, (model, prec, shape))
            _guards_intact(g, (model, prec, shape))
            assert g.kernel_configs() == p.kernel_configs()
            assert g.scratch_bytes() == p.scratch_bytes()          # the guards are not part of the documented footprint
            assert np.isfinite(got['logits']).all() and got['logits'].std() > 0
        nb, payload, guards = g.guard_info()
        print('%s %s: %d guarded buffers, %d payload bytes, %d guard bytes' % (model, prec, nb, payload, guards))
        assert nb > 20 and guards == nb * 2 * (1 << 20) and payload > g.scratch_bytes() > 0     # weights are guarded too
        assert p.guard_info()[0] == 0


# ---- b. small after large, on one handle -----------------------------------------------------------------------------------------

@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('model', FRAME_MODELS)
def test_small_after_large_on_one_handle(guarded, model, prec, pattern):
    """17 images of 272 x 304, then -- a poison in front of each -- a tail batch in the kept plan, a small ragged shape, a smaller batch of
    it (plan kept: the tail of every map is stale), the smallest shape.  Each equals a fresh plain handle that ran only that case."""
    _small_after_large(guarded(model), model, prec, pattern, [LARGE, (5,) + LARGE[1:], (3, 80, 112), (2, 80, 112), (1, 16, 16)])


def _small_after_large(eng, model, prec, pattern, shapes):
    _set_precision(eng, prec)
    for i, shape in enumerate(shapes):
        if i:
            assert eng.poison(pattern) > 10
        got = _run(eng, shape)
        _same_bits(got, _fresh_plain(model, prec, shape), (model, prec, pattern, shape))
        _guards_intact(eng, (model, prec, pattern, shape))


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('prec', ['f32x3+convs', 'bf16_store', 'bf16_full'])
@pytest.mark.parametrize('model', ['FCN_sa', 'FCN_la_4ch_seg4'])
def test_small_after_large_on_one_handle_newer_precisions(guarded, model, prec, pattern):
    """The same sequence under the conv stack on three bf16 pieces and under bf16 maps in HBM (half the bytes per channel)."""
    _small_after_large(guarded(model), model, prec, pattern, [LARGE, (5,) + LARGE[1:], (3, 80, 112), (2, 80, 112), (1, 16, 16)])


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('model,prec', [('UNet-LSTM_ao', 'fp32'), ('UNet-LSTM_ao', 'bf16'), ('Temporal-UNet_ao', 'fp32'), ('Temporal-UNet_ao', 'bf16_3d')])
def test_small_after_large_sequences_on_one_handle(guarded, model, prec, pattern):
    """run_seq: two windows of 48 x 80, one window in the kept plan (the second window's half of every map, of the ConvLSTM working
    buffers too, is stale), one window of a smaller shape."""
    _small_after_large(guarded(model), model, prec, pattern, [(2, 9, 48, 80), (1, 9, 48, 80), (1, 9, 32, 48)])


# ---- c. precision switches --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('model,other,shape', [('UNet_ao', 'bf16', (3, 80, 112)), ('UNet-LSTM_ao', 'bf16', (2, 9, 48, 80)), ('FCN_sa', 'f32x3', (3, 80, 112))])
def test_precision_switches_on_one_handle(guarded, model, other, shape):
    eng = guarded(model)
    outs = []
    for i, prec in enumerate(('fp32', other, 'fp32')):
        if i:
            eng.poison(PATTERNS[i])
        _set_precision(eng, prec)
        outs.append(_run(eng, shape))
        _guards_intact(eng, (model, prec, i))
    _same_bits(outs[2], outs[0], (model, 'fp32 again'))
    with _engine(model, PATTERNS[0]) as fresh:
        _set_precision(fresh, other)
        want = _run(fresh, shape)
        _guards_intact(fresh, (model, other, 'fresh'))
    _same_bits(outs[1], want, (model, other))
    if other == 'bf16':
        assert outs[1]['logits'].tobytes() != outs[0]['logits'].tobytes()  # the other precision really ran


@pytest.mark.parametrize('model,steps', [
    ('FCN_sa', [('fp32', (6, 128, 144)), ('bf16_store', (3, 80, 112)), ('f32x3+convs', (2, 80, 112)), ('bf16_full', (1, 16, 16)), ('fp32', (3, 80, 112))]),
    ('Temporal-UNet_ao', [('fp32', (2, 9, 48, 80)), ('bf16_3d', (1, 9, 32, 48)), ('fp32', (1, 9, 32, 48))])])
def test_precision_switches_with_a_shape_change(guarded, model, steps):
    """Each step under another precision AND another shape than the one before it, a poison in front of each: what the maps hold from
    the previous step is of the other element size and of another geometry.  Each equals a fresh plain handle that ran only that case."""
    eng = guarded(model)
    for i, (prec, shape) in enumerate(steps):
        eng.poison(PATTERNS[i % len(PATTERNS)])
        _set_precision(eng, prec)
        got = _run(eng, shape)
        _same_bits(got, _fresh_plain(model, prec, shape), (model, i, prec, shape))
        _guards_intact(eng, (model, i, prec, shape))
        assert np.isfinite(got['logits']).all() and got['logits'].std() > 0


# ---- d. cines ------------------------------------------------------------------------------------------------------------------------

def _same_cine(got, want, what):
    assert np.array_equal(got[0], want[0], equal_nan=True), what + ('prob',)     # NaNs of frames no window covers compare equal
    assert np.array_equal(got[1], want[1]), what + ('pred',)


def _lstm_cines(eng, prec, pattern=None):
    """13 frames of 48 x 64 at time_step 1 and 2, and 5 < 9 frames: whole, then under the minimum scratch budget the host query reports
    (chunks: the CHUNKED lstm_tile_kernel and lstm_img), there twice -- the first call allocates the released buffers, the second finds
    them poisoned with ``pattern``."""
    from ukbb_cardiac_amd import engine
    out = []
    _set_precision(eng, prec)
    for F, ts in ((13, 1), (13, 2), (5, 1)):
        frames = _image((F, 48, 64))
        low = engine.cine_min_scratch_bytes(eng.arch, prec, F, 48, 64, ts)
        assert low > 0
        if F == 13:
            assert engine.cine_chunk_windows(eng.arch, prec, F, 48, 64, ts, low) < -(-F // ts)       # really chunked
        for budget, calls in ((0, 1), (low, 2)):
            eng.set_scratch_budget(budget)
            for _ in range(calls):
                if pattern:
                    eng.poison(pattern)
                out.append(eng.run_cine(frames, time_step=ts))
                if pattern:
                    _guards_intact(eng, (prec, F, ts, budget))
        eng.set_scratch_budget(0)
    return out


_CINE_REF = {}


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
def test_unet_lstm_cines(guarded, prec, pattern):
    if prec not in _CINE_REF:
        with _engine('UNet-LSTM_ao') as plain:
            _CINE_REF[prec] = _lstm_cines(plain, prec)
    got = _lstm_cines(guarded('UNet-LSTM_ao'), prec, pattern)
    assert len(got) == len(_CINE_REF[prec]) == 9
    for i, (g, w) in enumerate(zip(got, _CINE_REF[prec])):
        _same_cine(g, w, (prec, pattern, i))
        assert np.isfinite(g[0]).all() and g[0].std() > 0


@pytest.mark.parametrize('pattern', PATTERNS)
def test_temporal_unet_cines(guarded, pattern, monkeypatch):
    frames = _image((13, 32, 48))
    eng = guarded('Temporal-UNet_ao')
    with _engine('Temporal-UNet_ao') as plain:
        for prec in ('fp32', 'bf16_3d'):
            for e in (eng, plain):
                _set_precision(e, prec)
            for chunk in ('1', None):
                if chunk is None:
                    monkeypatch.delenv('UKBB_TEMPORAL_CHUNK_WINDOWS', raising=False)
                else:
                    monkeypatch.setenv('UKBB_TEMPORAL_CHUNK_WINDOWS', chunk)
                want = plain.run_cine(frames)
                eng.poison(pattern)
                got = eng.run_cine(frames)
                _same_cine(got, want, (prec, pattern, chunk))
                _guards_intact(eng, (prec, pattern, chunk))
                assert np.isfinite(got[0]).all() and got[0].std() > 0


def _plain_cine(model, prec, F, H, W, ts):
    """What a fresh plain handle returns for the cine, whole (computed once, shared, never modified)."""
    key = (model, prec, F, H, W, ts)
    if key not in _CINE_REF:
        with _engine(model) as plain:
            _set_precision(plain, prec)
            _CINE_REF[key] = plain.run_cine(_image((F, H, W)), time_step=ts)
        for v in _CINE_REF[key]:
            v.setflags(write=False)
    return _CINE_REF[key]


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('prec', ['fp32', 'bf16_3d'])
def test_temporal_unet_cines_under_a_scratch_budget(guarded, prec, pattern, monkeypatch):
    """A third of what the unchunked cine takes: chunks of several windows sized by the budget.  Twice -- the first call allocates the
    released buffers, the second finds them poisoned."""
    from ukbb_cardiac_amd import engine
    monkeypatch.delenv('UKBB_TEMPORAL_CHUNK_WINDOWS', raising=False)
    F, H, W = 13, 32, 48
    eng = guarded('Temporal-UNet_ao')
    _set_precision(eng, prec)
    budget = engine.cine_scratch_bytes(eng.arch, prec, F, H, W, 1) // 3
    assert 1 <= engine.cine_chunk_windows(eng.arch, prec, F, H, W, 1, budget) < F        # accepted, and really chunked
    want = _plain_cine('Temporal-UNet_ao', prec, F, H, W, 1)
    eng.set_scratch_budget(budget)
    try:
        for call in range(2):
            eng.poison(pattern)
            got = eng.run_cine(_image((F, H, W)))
            _same_cine(got, want, (prec, pattern, call))
            _guards_intact(eng, (prec, pattern, call))
            assert 0 < eng.scratch_bytes() <= budget
    finally:
        eng.set_scratch_budget(0)


# ---- e. the instrument works ----------------------------------------------------------------------------------------------------------

def test_poison_is_read_back_and_a_damaged_guard_is_reported():
    G = 1 << 20
    with _engine('FCN_sa', PATTERNS[0]) as eng:                       # a throw-away handle: its guards end up damaged
        eng.run(_image((2, 32, 48)))
        _guards_intact(eng, 'before')
        for pat in PATTERNS:
            eng.poison(pat)
            conv0 = eng.activation('conv0')                            # before any forward: what the poison left
            assert conv0.size == 2 * 32 * 48 * 16
            assert np.all(conv0.view(np.uint32) == int(pat, 16)), pat
        nbytes = conv0.size * 4
        with pytest.raises(Exception, match='no guard'):
            eng.damage_guard('act0:conv0', 0)                           # the payload is not a guard
        with pytest.raises(Exception, match='no buffer'):
            eng.damage_guard('act0:nonsense', -1)
        eng.damage_guard('act0:conv0', nbytes + 7)
        bad, report = eng.check_guards()
        assert bad == 1 and report.splitlines() == ['act0:conv0 back %d %d' % (nbytes + 7, nbytes + 7)], report
        from ukbb_cardiac_amd import _lib
        assert 'act0:conv0 back' in _lib.last_error()
        eng.damage_guard('act0:conv0', nbytes + G - 1)                 # the guard's last byte
        eng.damage_guard('dev:conv0_0/bias', -G)                       # a weight buffer, the front guard's first byte
        eng.damage_guard('io_prob', -1)
        bad, report = eng.check_guards()
        assert bad == 3, report
        assert sorted(report.splitlines()) == sorted(['act0:conv0 back %d %d' % (nbytes + 7, nbytes + G - 1), 'dev:conv0_0/bias front %d %d' % (-G, -G),
                                                      'io_prob front -1 -1']), report
        out = eng.run(_image((2, 32, 48)))                              # a damaged guard harms nothing: the handle still runs
        assert np.isfinite(out['prob']).all() and out['prob'].std() > 0


# ---- e2. the handle's own buffers, every name -------------------------------------------------------------------------------------

HANDLE_BUFS = ('io_image', 'io_logits', 'io_prob', 'io_pred', 'lstm_gx', 'lstm_c1', 'lstm_h1', 'lstm_c', 'lstm_hall', 'lstm_probw', 'lstm_aux',
               'lstm_img', 't3d_aux', 't3d_probw')
KEPT = ('io_image', 'lstm_aux', 't3d_aux')                          # what a call does not rewrite before it reads it: poison() leaves them
RAW = {'lstm:h1': 'lstm_h1', 'lstm:hall': 'lstm_hall', 'lstm:gx': 'lstm_gx', 'lstm:c1': 'lstm_c1', 'lstm:c': 'lstm_c'}


def _payload_bytes(eng, name):
    """The payload bytes of the buffer ``name``, None if the handle knows the name and has not allocated it: from the refusal to
    damage offset 0, which lies in no guard.  An unknown name fails here."""
    with pytest.raises(Exception) as ei:
        eng.damage_guard(name, 0)
    msg = str(ei.value)
    assert 'no buffer named' not in msg, msg
    if "buffer '%s' is not allocated" % name in msg:
        return None
    m = re.search(r"is in no guard of '%s' \(payload (\d+) bytes" % re.escape(name), msg)
    assert m, msg
    return int(m.group(1))


def _fcn_calls(eng):
    eng.run(_image((1, 48, 16)), want_logits=True)                   # the host-array forward stages its image and all three outputs
    return 1, 48, 16


def _lstm_calls(eng):
    from ukbb_cardiac_amd import engine
    eng.run_seq(_image((1, 9, 16, 48)))
    sizes = {raw: eng.activation(raw).size * 4 for raw in RAW}      # the raw working buffers answer after a sequence call
    assert all(sizes.values()), sizes
    assert sizes == {raw: _payload_bytes(eng, buf) for raw, buf in RAW.items()}
    low = engine.cine_min_scratch_bytes(eng.arch, 'fp32', 13, 16, 48, 1)
    assert 0 < engine.cine_chunk_windows(eng.arch, 'fp32', 13, 16, 48, 1, low) < 13      # chunks: the frame run goes through lstm_img
    eng.set_scratch_budget(low)
    eng.run_cine(_image((13, 16, 48)))
    return 13, 16, 48


def _t3d_calls(eng):
    eng.run_cine(_image((13, 16, 48)))
    return 13 * 9, 16, 48                                            # every window in one chunk


@pytest.mark.parametrize('model,calls,allocated', [
    ('FCN_sa', _fcn_calls, ('io_image', 'io_logits', 'io_prob', 'io_pred')),
    # lstm_probw stands in for a NULL prob of ukbb_fcn_forward_seq, and Engine.run_seq always passes prob: none of engine.py's calls
    # allocates it, so on every handle here the name is known and "is not allocated"
    ('UNet-LSTM_ao', _lstm_calls, ('lstm_gx', 'lstm_c1', 'lstm_h1', 'lstm_c', 'lstm_hall', 'lstm_aux', 'lstm_img')),
    ('Temporal-UNet_ao', _t3d_calls, ('t3d_aux', 't3d_probw'))])
def test_every_handle_buffer_is_named_guarded_and_poisoned(model, calls, allocated):
    """The 14 buffers a handle owns besides its weights and activation maps, under the names check_guards reports them: every handle
    knows all 14 names, the calls above allocate the listed ones (each of the 14 but lstm_probw on some handle) and a damaged back
    guard of each is reported under its name; poison() refills the allocated ones a call rewrites and the activation maps."""
    import torch
    from ukbb_cardiac_amd import engine
    with _engine(model, PATTERNS[0]) as eng:                          # a throw-away handle: its guards end up damaged
        shape = calls(eng)                                            # the largest batch the handle planned for
        _guards_intact(eng, model)
        size = {name: _payload_bytes(eng, name) for name in HANDLE_BUFS}
        assert tuple(name for name in HANDLE_BUFS if size[name] is not None) == allocated, size
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        maps = ['act%d%s' % (i, ':' + a['name'] if a['name'] else '') for i, a in enumerate(engine.plan_layout(eng.arch, 'fp32', *shape, cus)['acts'])]
        n_maps = sum(_payload_bytes(eng, name) is not None for name in maps)
        assert n_maps == len(maps) > 0
        assert eng.poison(PATTERNS[1]) == len([name for name in allocated if name not in KEPT]) + n_maps
        for name in allocated:
            eng.damage_guard(name, size[name])
        bad, report = eng.check_guards()
        assert bad == len(allocated) and sorted(report.splitlines()) == sorted('%s back %d %d' % (name, size[name], size[name]) for name in allocated), report


# ---- f. caller-owned outputs ----------------------------------------------------------------------------------------------------------

MARGIN = 1 << 16                                                     # bytes on either side of a carved region
SENTINELS = (0xCD, 0x32)                                             # every case runs with both: a byte an entry leaves unwritten cannot equal the reference twice


class Carved:
    """``nbytes`` of device memory in the middle of a larger torch tensor: MARGIN bytes before it, MARGIN (+ up to 15) behind it,
    all filled with the byte ``fill`` (or float32 NaN for ``fill='nan'``); the region itself holds ``payload`` if given."""

    def __init__(self, nbytes, fill, payload=None):
        import torch
        self.nbytes = int(nbytes)
        host = np.empty(2 * MARGIN + -(-self.nbytes // 16) * 16, np.uint8)
        if fill == 'nan':
            host.view(np.float32)[:] = np.nan
        else:
            host[:] = fill
        if payload is not None:
            raw = np.ascontiguousarray(payload.ravel(order='K')).view(np.uint8)     # memory order of a C- or F-contiguous array
            assert raw.size == self.nbytes
            host[MARGIN:MARGIN + self.nbytes] = raw
        self.before = host.copy()
        self.t = torch.from_numpy(host).cuda()
        self.ptr = self.t.data_ptr() + MARGIN

    def read(self, what):
        """The region's bytes now; everything around it must be as it was."""
        import torch
        torch.cuda.synchronize()
        now = self.t.cpu().numpy()
        end = MARGIN + self.nbytes
        assert np.array_equal(now[:MARGIN], self.before[:MARGIN]), (what, 'bytes in front of the region changed', np.flatnonzero(now[:MARGIN] != self.before[:MARGIN])[[0, -1]] - MARGIN)
        assert np.array_equal(now[end:], self.before[end:]), (what, 'bytes behind the region changed', np.flatnonzero(now[end:] != self.before[end:])[[0, -1]])
        return now[MARGIN:end]

    def untouched(self, what):
        assert np.array_equal(self.read(what), self.before[MARGIN:MARGIN + self.nbytes]), (what, 'an input was written')


def _volume(shape, dtype, seed, order):
    """MR-like magnitudes with background ties, in the dtype's range (int16: negative values too; uint16: above 32767), as the
    volumes of tests/test_device_pipeline.py and tests/test_integer_volumes_gpu.py."""
    rng = np.random.default_rng(seed)
    v = rng.gamma(1.5, 1.0, size=shape)
    v[rng.random(shape) < 0.08] = 0.0
    if dtype == np.float32:
        return np.asarray(np.round(v * 120.0), dtype=np.float32, order=order)
    v = v * 40.0 if dtype == np.uint8 else v * 3000.0 - 2000.0 if dtype == np.int16 else v * 12000.0
    info = np.iinfo(dtype)
    return np.asarray(np.clip(np.round(v), info.min, info.max).astype(dtype), order=order)


def _strides(a):
    return tuple(s // a.itemsize for s in a.strides)


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


@pytest.mark.parametrize('dtype', [np.float32, np.uint8, np.int16, np.uint16])
@pytest.mark.parametrize('order', ['F', 'C'])
@pytest.mark.parametrize('shape', [(37, 29, 1, 7), (65, 33, 2, 3)])
def test_prep_entries_write_their_outputs_and_nothing_else(shape, order, dtype):
    """rescale_pack(_t), zscore_pack(_t), unpack_labels, roi_compact(_t), label_max and label_compact on carved device pointers,
    against the host references the existing tests use (image_utils, the numpy mirror of the deploy loop, aorta_qc.stats_host)."""
    from ukbb_cardiac_amd import _lib, aorta_qc, device_pipeline as dp
    from ukbb_cardiac_amd.image_utils import normalise_intensity, rescale_intensity
    from ukbb_cardiac_amd.pipeline import pad_amounts, pad_amounts_fixed
    X, Y, Z, T = shape
    dtype = np.dtype(dtype)
    code = 16 if dtype == np.float32 else dp.NIFTI_DATATYPE[dtype]
    vol = _volume(shape, dtype, X + Y + dtype.itemsize, order)
    assert vol.flags.f_contiguous if order == 'F' else vol.flags.c_contiguous
    n_class = 3
    rng = np.random.default_rng(X * Y)
    # references (host)
    lo, hi = np.percentile(vol, (1, 99))
    X2, Y2, x_pre, x_post, y_pre, y_post = pad_amounts(X, Y)
    scaled = rescale_intensity(vol.copy(order='K'), (1, 99))
    want_rescale = np.transpose(np.pad(scaled, ((x_pre, x_post), (y_pre, y_post), (0, 0), (0, 0)), 'constant'), (3, 2, 0, 1)).reshape(T * Z, X2, Y2).astype(np.float32)
    val_l = np.percentile(vol, 10.0)
    roi = vol >= val_l
    mu, den = np.mean(vol[roi]), np.std(vol[roi]) + 1e-6
    F2, G2, fx_pre, fx_post, fy_pre, fy_post = pad_amounts_fixed(X, Y)
    norm = normalise_intensity(vol, 10.0)
    want_zscore = np.transpose(np.pad(norm, ((fx_pre, fx_post), (fy_pre, fy_post), (0, 0), (0, 0)), 'constant'), (3, 2, 0, 1)).reshape(T * Z, F2, G2).astype(np.float32)
    lab = rng.integers(0, n_class, size=(T * Z, X2, Y2)).astype(np.int32)
    want_vol = np.asfortranarray(lab.reshape(T, Z, X2, Y2).transpose(2, 3, 1, 0)[x_pre:x_pre + X, y_pre:y_pre + Y].astype(np.uint8))
    want_counts = np.stack([[np.sum(want_vol[..., t] == c) for c in range(n_class)] for t in range(T)]).astype(np.uint64)
    want_roi = vol[roi]
    seg = np.asfortranarray(rng.integers(0, n_class, size=shape).astype(np.uint8))            # NIfTI order, what unpack_labels writes
    seg[..., T - 1][seg[..., T - 1] == 2] = 0                                                    # an empty mask: -inf
    stats = aorta_qc.stats_host(vol, seg, n_class)
    for s in SENTINELS:
        src = Carved(vol.nbytes, 'nan' if dtype == np.float32 else 0x7F, vol)
        st = _strides(vol)
        # rescale_pack / rescale_pack_t
        out = Carved(want_rescale.nbytes, s)
        dp.pack_rescaled(src.ptr, dtype, shape, st, lo, hi, (X2, Y2, x_pre, y_pre), out.ptr, 0)
        assert np.array_equal(out.read('rescale_pack'), _bytes(want_rescale)), 'rescale_pack'
        # zscore_pack / zscore_pack_t
        out = Carved(want_zscore.nbytes, s)
        dp.zscore_pack(src.ptr, dtype, shape, st, mu, den, (F2, G2, fx_pre, fy_pre), out.ptr, 0)
        assert np.array_equal(out.read('zscore_pack'), _bytes(want_zscore)), 'zscore_pack'
        # roi_compact / roi_compact_t: the first n elements are the entry's to write
        out = Carved(vol.nbytes, s)
        n = C.c_uint64(0)
        if dtype == np.float32:
            _lib.check(_lib.lib.ukbb_fcn_roi_compact(src.ptr, X, Y, Z, T, *st, float(val_l), out.ptr, C.byref(n), 0), 'roi_compact')
        else:
            _lib.check(_lib.lib.ukbb_fcn_roi_compact_t(src.ptr, code, X, Y, Z, T, *st, float(val_l), out.ptr, C.byref(n), 0), 'roi_compact_t')
        assert n.value == want_roi.size and 0 < n.value < vol.size
        assert np.array_equal(out.read('roi_compact')[:want_roi.nbytes], _bytes(want_roi)), 'roi_compact'
        # unpack_labels
        pred = Carved(lab.nbytes, 0x7F, lab)
        out, cnt = Carved(want_vol.nbytes, s), Carved(want_counts.nbytes, s)
        _lib.check(_lib.lib.ukbb_fcn_unpack_labels(pred.ptr, X, Y, Z, T, X2, Y2, x_pre, y_pre, n_class, out.ptr, cnt.ptr, 0), 'unpack_labels')
        assert np.array_equal(out.read('unpack_labels volume'), want_vol.ravel(order='F')), 'unpack_labels volume'
        assert np.array_equal(cnt.read('unpack_labels counts'), _bytes(want_counts)), 'unpack_labels counts'
        pred.untouched('unpack_labels pred')
        # label_max, label_compact
        labels = Carved(seg.nbytes, 0x01, seg)                                                  # a label read from beside the volume would count
        mx = Carved(T * n_class * 8, s)
        _lib.check(_lib.lib.ukbb_fcn_label_max(src.ptr, code, X, Y, Z, T, *st, labels.ptr, n_class, mx.ptr, 0), 'label_max')
        got_max = mx.read('label_max').view(np.float64).reshape(T, n_class)
        assert np.array_equal(got_max, stats['max'], equal_nan=True) and np.isneginf(got_max[T - 1, 2]), 'label_max'
        for k in range(1, n_class):
            want_k = vol[..., 0][seg[..., 0] == k]
            out = Carved(X * Y * Z * dtype.itemsize, s)
            _lib.check(_lib.lib.ukbb_fcn_label_compact(src.ptr, code, X, Y, Z, *st[:3], labels.ptr, k, out.ptr, C.byref(n), 0), 'label_compact')
            assert n.value == want_k.size > 0
            assert np.array_equal(out.read('label_compact')[:want_k.nbytes], _bytes(want_k)), 'label_compact'
            with np.errstate(all='ignore'):
                assert want_k.mean() == stats['mean_ed'][k]                                      # the reference the compacted voxels feed
        src.untouched('the volume')
        labels.untouched('the labels')


@pytest.mark.parametrize('model,prec', [('FCN_sa', 'fp32'), ('FCN_sa', 'bf16'), ('FCN_sa', 'f32x3'), ('FCN_la_4ch_seg4', 'fp32'), ('UNet_ao', 'fp32'), ('UNet_ao', 'bf16'),
                                        ('FCN_sa', 'bf16_store'), ('FCN_sa', 'bf16_full'), ('FCN_la_4ch_seg4', 'bf16_full'), ('FCN_sa', 'f32x3+convs')])
def test_device_pointer_forward_writes_only_the_callers_outputs(guarded, model, prec):
    """ukbb_fcn_forward with the image between NaNs and logits / prob / pred each between sentinels: the bits of the host-array call."""
    eng = guarded(model)
    _set_precision(eng, prec)
    ncls = eng.arch.n_class
    for shape in [(3, 80, 112), (1, 16, 16), (2, 48, 400)]:
        n, h, w = shape
        img = _image(shape)
        want = eng.run(img, want_logits=True)
        for s in SENTINELS:
            eng.poison(PATTERNS[0])
            x = Carved(img.nbytes, 'nan', img)
            lg, pr, pd = Carved(img.nbytes * ncls, s), Carved(img.nbytes * ncls, s), Carved(img.nbytes, s)
            eng.run_device(x.ptr, n, h, w, logits_ptr=lg.ptr, prob_ptr=pr.ptr, pred_ptr=pd.ptr, stream=0)
            what = (model, prec, shape, s)
            assert np.array_equal(lg.read(what + ('logits',)), _bytes(want['logits'])), what
            assert np.array_equal(pr.read(what + ('prob',)), _bytes(want['prob'])), what
            assert np.array_equal(pd.read(what + ('pred',)), _bytes(want['pred'])), what
            x.untouched(what + ('image',))
            _guards_intact(eng, what)


SEQ_MODELS = [('UNet-LSTM_ao', 'fp32'), ('UNet-LSTM_ao', 'bf16'), ('Temporal-UNet_ao', 'fp32'), ('Temporal-UNet_ao', 'bf16_3d')]


@pytest.mark.parametrize('model,prec', SEQ_MODELS)
def test_forward_seq_writes_only_the_callers_outputs(guarded, model, prec):
    """ukbb_fcn_forward_seq on carved pointers: all three outputs, then logits = NULL, then prob alone.  A NULL output has no region;
    every region passed holds the bits a fresh plain handle returns, under both sentinels; the frames stay untouched."""
    eng = guarded(model)
    _set_precision(eng, prec)
    shape = (2, 9, 32, 48)
    n, t, h, w = shape
    assert t == eng.arch.n_step
    ncls = eng.arch.n_class
    img = _image(shape)
    want = _fresh_plain(model, prec, shape)
    size = {'logits': img.nbytes * ncls, 'prob': img.nbytes * ncls, 'pred': img.nbytes}
    for s in SENTINELS:
        for outputs in (('logits', 'prob', 'pred'), ('prob', 'pred'), ('prob',)):
            eng.poison(PATTERNS[0])
            x = Carved(img.nbytes, 'nan', img)
            out = {k: Carved(size[k], s) for k in outputs}
            eng.run_seq_device(x.ptr, n, h, w, stream=0, **{k + '_ptr': r.ptr for k, r in out.items()})
            what = (model, prec, s, outputs)
            for k, r in out.items():
                assert np.array_equal(r.read(what + (k,)), _bytes(want[k])), what + (k,)
            x.untouched(what + ('frames',))
            _guards_intact(eng, what)


@pytest.mark.parametrize('model,prec', SEQ_MODELS)
def test_forward_cine_writes_only_the_callers_outputs(guarded, model, prec, monkeypatch):
    """ukbb_fcn_forward_cine on carved pointers, the bits of Engine.run_cine on a fresh plain handle: 13 frames whole, in chunks (the
    UNet-LSTM under its minimum scratch budget, the Temporal-UNet one window at a time), with pred = NULL, and 12 frames at time_step 10,
    where frame 5 lies in neither window: its prob must be WRITTEN as NaN and its pred as 0, whatever the regions held."""
    from ukbb_cardiac_amd import engine
    monkeypatch.delenv('UKBB_TEMPORAL_CHUNK_WINDOWS', raising=False)
    eng = guarded(model)
    _set_precision(eng, prec)
    lstm = model.startswith('UNet-LSTM')
    H, W, ncls, T = 32, 48, eng.arch.n_class, eng.arch.n_step
    low = engine.cine_min_scratch_bytes(eng.arch, prec, 13, H, W, 1) if lstm else 0
    if lstm:
        assert low > 0 and 0 < engine.cine_chunk_windows(eng.arch, prec, 13, H, W, 1, low) < 13         # really chunked
    unreached = sorted(set(range(12)) - {(c - (T - 1) // 2 + k) % 12 for c in range(0, 12, 10) for k in range(T)})
    assert unreached == [5]
    try:
        for F, ts, chunked, with_pred in ((13, 1, False, True), (13, 1, True, True), (12, 10, False, True), (13, 1, False, False)):
            frames = _image((F, H, W))
            want = _plain_cine(model, prec, F, H, W, ts)
            eng.set_scratch_budget(low if chunked and lstm else 0)
            if chunked and not lstm:
                monkeypatch.setenv('UKBB_TEMPORAL_CHUNK_WINDOWS', '1')
            else:
                monkeypatch.delenv('UKBB_TEMPORAL_CHUNK_WINDOWS', raising=False)
            for s in SENTINELS:
                eng.poison(PATTERNS[0])
                x = Carved(frames.nbytes, 'nan', frames)
                pr, pd = Carved(frames.nbytes * ncls, s), Carved(frames.nbytes, s) if with_pred else None
                eng.run_cine_device(x.ptr, F, H, W, pr.ptr, pd.ptr if pd else 0, time_step=ts, stream=0)
                what = (model, prec, F, ts, chunked, with_pred, s)
                got_prob = pr.read(what + ('prob',))
                assert np.array_equal(got_prob, _bytes(want[0])), what
                if pd:
                    got_pred = pd.read(what + ('pred',))
                    assert np.array_equal(got_pred, _bytes(want[1])), what
                if ts == 10:
                    assert np.isnan(got_prob.view(np.float32).reshape(F, H, W, ncls)[unreached]).all(), what
                    assert not got_pred.view(np.int32).reshape(F, H, W)[unreached].any(), what
                    assert np.isfinite(np.delete(want[0], unreached, axis=0)).all()
                else:
                    assert np.isfinite(want[0]).all() and want[0].std() > 0
                x.untouched(what + ('frames',))
                _guards_intact(eng, what)
    finally:
        eng.set_scratch_budget(0)


def _blobs(shape, n_class, seed):
    """A label volume (uint8, NIfTI order) of blocks of 1 .. 6 voxels a side with single voxels flipped: components of every size,
    many around the default threshold, some that join only through a diagonal neighbour or across z."""
    X, Y, Z, T = shape
    rng = np.random.default_rng(seed)
    lab = np.zeros(shape, np.uint8)
    for t in range(T):
        for z in range(Z):
            b = int(rng.integers(1, 7))
            coarse = rng.integers(0, n_class, size=(-(-X // b), -(-Y // b))).astype(np.uint8)
            lab[:, :, z, t] = np.kron(coarse, np.ones((b, b), np.uint8))[:X, :Y]
    flip = rng.random(shape) < 0.05
    lab[flip] = rng.integers(0, n_class, size=int(flip.sum())).astype(np.uint8)
    return np.asfortranarray(lab)


@pytest.mark.parametrize('shape', [(37, 29, 1, 7), (65, 33, 2, 3)])
def test_label_components_writes_its_outputs_and_nothing_else(shape):
    """ukbb_fcn_label_components on carved pointers: the labels lie between bytes of label value 1 (a read beside the volume would
    join a component), d_work is exactly the 2*X*Y*Z*T int32 the contract asks for, d_n_large exactly T x n_class int32.  Against
    aorta_qc.count_large_components for min_size 0 and the default; a second call on the same, now dirty, d_work gives the same."""
    from ukbb_cardiac_amd import _lib, aorta_qc
    X, Y, Z, T = shape
    n_class = 3
    seg = _blobs(shape, n_class, X + Y)
    for min_size in (0, aorta_qc.PIXEL_THRES):
        want = aorta_qc.count_large_components(seg, n_class, min_size)
        assert want.dtype == np.int32 and want.shape == (T, n_class) and not want[:, 0].any()
        assert (want[:, 1:] > 0).any() and len(np.unique(want[:, 1:])) > 2                       # a grading signal
        for s in SENTINELS:
            labels = Carved(seg.nbytes, 0x01, seg)
            work = Carved(4 * 2 * X * Y * Z * T, s)
            for call in range(2):
                out = Carved(want.nbytes, s)
                _lib.check(_lib.lib.ukbb_fcn_label_components(labels.ptr, X, Y, Z, T, n_class, min_size, work.ptr, out.ptr, 0), 'label_components')
                what = (shape, min_size, s, call)
                got = out.read(what + ('n_large',)).view(np.int32).reshape(T, n_class)
                assert np.array_equal(got, want), what
                work.read(what + ('work',))                                                      # nothing beside d_work changed
                labels.untouched(what + ('labels',))
    assert not np.array_equal(aorta_qc.count_large_components(seg, n_class, 0), aorta_qc.count_large_components(seg, n_class))
