"""forward_cine under a scratch budget (ABI 11) on the GPU: the windows run in chunks and give the bits of the unchunked call, the
handle holds what the host-only planner predicts and no more than the budget, a cine of any length fits a few GB.
Every case uses a FRESH engine (the planner predicts a fresh handle's plan); ukbb_fcn_set_scratch_budget with a new non-zero value
releases the handle's activation and cine buffers, so the budget-0 reference run on the same handle leaves nothing behind."""
import numpy as np
import pytest

from oracle import fcn_oracle as O

pytestmark = pytest.mark.gpu


def _arch():
    from ukbb_cardiac_amd.arch import MODELS
    return MODELS['UNet-LSTM_ao']


def _params(head, seed=1234):
    from ukbb_cardiac_amd.weights import embed_unidirectional_lstm, synthetic_params
    arch = _arch()
    p = synthetic_params(arch, seed)
    if head == 'bi':
        return p
    rng = np.random.default_rng(seed)
    uni = {k: v for k, v in p.items() if not k.startswith('lstm')}
    uni['lstm'] = p['lstm_fw']
    uni['lstm_conv'] = {'kernel': rng.normal(0, 0.4, size=(1, 1, arch.same_dim, arch.n_class)).astype(np.float32),
                        'bias': rng.normal(0, 0.1, size=arch.n_class).astype(np.float32)}
    return embed_unidirectional_lstm(uni, arch.same_dim)


def _budget_for(arch, prec, F, H, W, ts, want_wc):
    """The smallest budget under which the planner runs chunks of want_wc windows (bisection of the host-only planner)."""
    from ukbb_cardiac_amd import engine
    lo, hi = engine.cine_min_scratch_bytes(arch, prec, F, H, W, ts), engine.cine_scratch_bytes(arch, prec, F, H, W, ts, 0)
    assert engine.cine_chunk_windows(arch, prec, F, H, W, ts, lo) <= want_wc, 'the minimum budget already runs larger chunks'
    while lo < hi:
        mid = (lo + hi) // 2
        if engine.cine_chunk_windows(arch, prec, F, H, W, ts, mid) >= want_wc:
            hi = mid
        else:
            lo = mid + 1
    assert engine.cine_chunk_windows(arch, prec, F, H, W, ts, lo) == want_wc
    return lo


def _frames(F, H, W, seed):
    from ukbb_cardiac_amd.phantom import cine_phantom
    return ((cine_phantom(F, H, W, seed=seed)[..., 0] - 0.3) / 0.25).astype(np.float32)


def _bits(prob):
    return np.ascontiguousarray(prob).view(np.uint32)


def _wanted_chunks(Wn):
    """Wc = 1, 2, an odd Wc that does not divide Wn, Wn - 1 (those that are real chunk plans for this Wn)."""
    odd = next((c for c in (3, 5, 7, 9, 11) if c < Wn and Wn % c), None)
    return sorted({c for c in (1, 2, odd, Wn - 1) if c and 1 <= c < Wn})


def _check_budgets(eng, arch, prec, frames, ts, chunks):
    from ukbb_cardiac_amd import engine
    F, H, W = frames.shape
    prob0, pred0 = eng.run_cine(frames, time_step=ts)                        # budget 0: graded against the fp64 oracle by tests/test_unet_lstm_gpu.py
    whole = engine.cine_scratch_bytes(arch, prec, F, H, W, ts, 0)
    assert eng.scratch_bytes() == whole                                      # a fresh handle's first call: exactly the documented footprint
    for wc in chunks:
        b = _budget_for(arch, prec, F, H, W, ts, wc)
        eng.set_scratch_budget(b)
        prob, pred = eng.run_cine(frames, time_step=ts)
        held, want = eng.scratch_bytes(), engine.cine_scratch_bytes(arch, prec, F, H, W, ts, b)
        print('F %d %dx%d ts %d %s Wc %d: budget %d held %d predicted %d unchunked %d' % (F, H, W, ts, prec, wc, b, held, want, whole))
        assert np.array_equal(_bits(prob), _bits(prob0)), 'prob differs with Wc = %d' % wc
        assert np.array_equal(pred, pred0), 'pred differs with Wc = %d' % wc
        assert held == want and held <= b
    return prob0, pred0


SMALL = [(4, 64, 64, 1), (9, 48, 80, 1), (10, 64, 64, 2), (10, 48, 80, 1), (25, 48, 80, 1), (25, 64, 64, 3), (50, 64, 64, 1), (50, 48, 80, 2),
         (25, 64, 64, 12), (50, 48, 80, 3)]


@pytest.mark.parametrize('head', ['bi', 'uni'])
@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('F,H,W,ts', SMALL)
def test_chunked_cine_has_the_bits_of_the_unchunked_one(prec, head, F, H, W, ts):
    from ukbb_cardiac_amd.engine import Engine
    arch = _arch()
    Wn = -(-F // ts)
    with Engine(arch, _params(head)) as eng:
        eng.set_precision(prec)
        prob0, pred0 = _check_budgets(eng, arch, prec, _frames(F, H, W, 7 * F + ts), ts, _wanted_chunks(Wn))
    if ts > 9:
        assert np.isnan(prob0).any() and not np.isnan(prob0).all()           # frames no window reaches: NaN in both, compared as bits
    else:
        assert not np.isnan(prob0).any()
    assert len(np.unique(pred0)) > 1


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
def test_chunked_cine_100_frames_of_256x256(prec):
    from ukbb_cardiac_amd.engine import Engine
    arch = _arch()
    with Engine(arch, _params('bi')) as eng:
        eng.set_precision(prec)
        _check_budgets(eng, arch, prec, _frames(100, 256, 256, 3), 1, [7, 99])


def test_chunked_cine_against_the_fp64_oracle():
    """A Wc = 2 result against the numpy restatement itself (network_ao.py:255-399 per window in float64, the tiling of
    deploy_network_ao.py:129-183), with the probability tolerance of tests/test_unet_lstm_gpu.py -- not only against the one-pass kernel."""
    from ukbb_cardiac_amd.engine import Engine
    arch = _arch()
    params = _params('bi')
    F, H, W = 10, 32, 32
    frames = _frames(F, H, W, 11)
    with Engine(arch, params) as eng:
        eng.set_scratch_budget(_budget_for(arch, 'fp32', F, H, W, 1, 2))
        prob, pred = eng.run_cine(frames)
    acc = np.zeros((F, H, W, arch.n_class))
    weight = np.zeros(F)
    w = O.aortic_window_weights(5, 0.1)
    for t in range(F):
        idx = O.aortic_window_indices(t, F, 5)
        logits = O.unet_lstm(frames[idx][None, ..., None], params, arch.n_hidden, n_block=arch.n_block, dtype=np.float64)
        acc[idx] += O.softmax(logits)[0] * w[:, None, None, None]
        weight[idx] += w
    want = acc / weight[:, None, None, None]
    err = np.abs(prob - want).max()
    print('Wc = 2 cine vs fp64 oracle: max |prob - ref| = %.3e' % err)
    assert err < 1e-4
    assert np.array_equal(pred, np.argmax(prob, -1))


def test_400_frames_fit_4_gb():
    """About 66 GB unchunked (52 GB of ConvLSTM scratch by the header's formula + the U-Net's maps): under a 4 GB budget the handle
    holds <= 4e9 bytes, and the first and last 50 frames have the bits of the same call under 8 GB (other chunk sizes)."""
    from ukbb_cardiac_amd import engine
    from ukbb_cardiac_amd.engine import Engine
    arch = _arch()
    params = _params('bi')
    F, H, W = 400, 256, 256
    assert engine.cine_scratch_bytes(arch, 'fp32', F, H, W, 1, 0) > 60e9
    frames = _frames(F, H, W, 5)
    got = {}
    for gb in (4, 8):
        b = gb * 10 ** 9
        with Engine(arch, params) as eng:
            eng.set_scratch_budget(b)
            prob, pred = eng.run_cine(frames)
            held = eng.scratch_bytes()
        wc = engine.cine_chunk_windows(arch, 'fp32', F, H, W, 1, b)
        print('400 x 256x256 fp32, %d GB budget: Wc %d, %d chunks, held %d bytes' % (gb, wc, -(-F // wc), held))
        assert held <= b and held == engine.cine_scratch_bytes(arch, 'fp32', F, H, W, 1, b)
        got[gb] = (np.concatenate([prob[:50], prob[350:]]), np.concatenate([pred[:50], pred[350:]]))
        del prob, pred
    assert engine.cine_chunk_windows(arch, 'fp32', F, H, W, 1, 4 * 10 ** 9) != engine.cine_chunk_windows(arch, 'fp32', F, H, W, 1, 8 * 10 ** 9)
    assert np.array_equal(_bits(got[4][0]), _bits(got[8][0]))
    assert np.array_equal(got[4][1], got[8][1])
    assert not np.isnan(got[4][0]).any() and len(np.unique(got[4][1])) > 1


def test_budget_below_the_minimum_is_refused_and_the_handle_stays_usable():
    from ukbb_cardiac_amd import _lib, engine
    from ukbb_cardiac_amd.engine import Engine
    arch = _arch()
    params = _params('bi')
    F, H, W = 25, 64, 64
    frames = _frames(F, H, W, 2)
    low = engine.cine_min_scratch_bytes(arch, 'fp32', F, H, W, 1)
    with Engine(arch, params) as ref:
        prob0, pred0 = ref.run_cine(frames)
    with Engine(arch, params) as eng:
        eng.set_scratch_budget(low - 1)
        with pytest.raises(_lib.UkbbFcnError, match=str(low)) as ei:
            eng.run_cine(frames)
        assert '(-1)' in str(ei.value)                                       # UKBB_EINVAL
        eng.set_scratch_budget(0)
        prob, pred = eng.run_cine(frames)
        assert np.array_equal(_bits(prob), _bits(prob0)) and np.array_equal(pred, pred0)
        eng.set_scratch_budget(low)                                          # the minimum itself runs
        prob, pred = eng.run_cine(frames)
        assert np.array_equal(_bits(prob), _bits(prob0)) and np.array_equal(pred, pred0)
        assert eng.scratch_bytes() == low
        with pytest.raises(ValueError):
            eng.set_scratch_budget(-5)


def test_frame_wise_models_ignore_the_budget():
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.engine import Engine
    from ukbb_cardiac_amd.weights import synthetic_params
    arch = MODELS['UNet_ao']
    x = np.random.default_rng(1).standard_normal((3, 32, 48, 1)).astype(np.float32)
    with Engine(arch, synthetic_params(arch, 3)) as eng:
        a = eng.run(x)
        held = eng.scratch_bytes()
        assert held > 0
        eng.set_scratch_budget(1000)                                         # accepted, ignored: nothing is released
        assert eng.scratch_bytes() == held
        b = eng.run(x)
    assert np.array_equal(a['prob'], b['prob']) and np.array_equal(a['pred'], b['pred'])


def test_temporal_unet_takes_the_budget(monkeypatch):
    """A budget that yields Wc = 3: the bits of the default call and of UKBB_TEMPORAL_CHUNK_WINDOWS=3; the variable wins over the budget."""
    from ukbb_cardiac_amd import engine
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.engine import Engine
    from ukbb_cardiac_amd.weights import synthetic_params
    arch = MODELS['Temporal-UNet_ao']
    F, H, W = 13, 32, 48
    frames = np.random.default_rng(3).standard_normal((F, H, W)).astype(np.float32)
    b3 = _budget_for(arch, 'fp32', F, H, W, 1, 3)
    monkeypatch.delenv('UKBB_TEMPORAL_CHUNK_WINDOWS', raising=False)
    with Engine(arch, synthetic_params(arch, 1234)) as eng:
        prob0, pred0 = eng.run_cine(frames)
        assert eng.scratch_bytes() == engine.cine_scratch_bytes(arch, 'fp32', F, H, W, 1, 0)
        monkeypatch.setenv('UKBB_TEMPORAL_CHUNK_WINDOWS', '3')
        prob_e, pred_e = eng.run_cine(frames)
        monkeypatch.delenv('UKBB_TEMPORAL_CHUNK_WINDOWS')
        eng.set_scratch_budget(b3)
        prob, pred = eng.run_cine(frames)
        assert eng.scratch_bytes() == engine.cine_scratch_bytes(arch, 'fp32', F, H, W, 1, b3) <= b3
        for p, q in ((prob, pred), (prob_e, pred_e)):
            assert np.array_equal(_bits(p), _bits(prob0)) and np.array_equal(q, pred0)
        monkeypatch.setenv('UKBB_TEMPORAL_CHUNK_WINDOWS', '2')               # both given: the variable wins (two windows' buffers)
        eng.set_scratch_budget(b3 + 1)
        prob, pred = eng.run_cine(frames)
        assert eng.scratch_bytes() == engine.cine_scratch_bytes(arch, 'fp32', F, H, W, 1, _budget_for(arch, 'fp32', F, H, W, 1, 2))
        assert np.array_equal(_bits(prob), _bits(prob0)) and np.array_equal(pred, pred0)
        monkeypatch.delenv('UKBB_TEMPORAL_CHUNK_WINDOWS')
        eng.set_scratch_budget(engine.cine_min_scratch_bytes(arch, 'fp32', F, H, W, 1) - 1)
        with pytest.raises(Exception, match='one window'):
            eng.run_cine(frames)


def test_aortic_script_with_cine_scratch_gb_writes_the_same_files(tmp_path, capsys):
    """deploy_network_ao.py on two subjects with a budget that forces several chunks per cine: the segmentations and the table are
    byte-identical to a run without the flag, with the pre-processing on the device and on the host."""
    import shutil
    from ukbb_cardiac_amd import deploy_network_ao, engine, nifti
    from ukbb_cardiac_amd.weights import save_blob
    arch = _arch()
    mp = str(tmp_path / 'UNet-LSTM_ao')
    save_blob(mp + '.ukbbw', arch, _params('bi'))
    rng = np.random.default_rng(77)
    src = tmp_path / 'src'
    for name, shape in (('s1', (96, 80, 1, 14)), ('s2', (90, 70, 1, 11))):
        (src / name).mkdir(parents=True)
        vol = np.round(100 * rng.gamma(2.0, 1.0, size=shape)).astype(np.float32)
        nifti.save(vol, str(src / name / 'ao.nii.gz'), np.diag([1.6, 1.6, 6.0, 1.0]), pixdim=[1, 1.6, 1.6, 6, 0.01, 0, 0, 0])
    # the script pads every cine to the network's 256 x 256 (deploy_network_ao.py:105): 5 chunks of the 14 windows, 3-4 of the 11
    gb = (_budget_for(arch, 'fp32', 14, 256, 256, 1, 3) + 4096) / 1e9
    assert engine.cine_chunk_windows(arch, 'fp32', 11, 256, 256, 1, int(gb * 1e9)) in (3, 4)
    out = {}
    for pre in ('--device_preproc', '--nodevice_preproc'):
        for budget in ([], ['--cine_scratch_gb', repr(gb)]):
            work = tmp_path / ('run_%s_%d' % (pre.strip('-'), len(budget)))
            shutil.copytree(src, work)
            deploy_network_ao.main(['--data_dir', str(work), '--model_path', mp, '--output_csv', str(work / 'ao.csv'), pre] + budget)
            out[pre, len(budget)] = {p.relative_to(work).as_posix(): p.read_bytes() for p in sorted(work.rglob('*')) if p.is_file() and p.name != 'ao.nii.gz'}
    ref = out['--device_preproc', 0]
    assert sorted(ref) == ['ao.csv', 's1/seg_ao.nii.gz', 's2/seg_ao.nii.gz']
    for k, v in out.items():
        assert v == ref, k
    capsys.readouterr()
    arch_u = __import__('ukbb_cardiac_amd.arch', fromlist=['MODELS']).MODELS['UNet_ao']
    from ukbb_cardiac_amd.weights import synthetic_params
    mu = str(tmp_path / 'UNet_ao')
    save_blob(mu + '.ukbbw', arch_u, synthetic_params(arch_u, 5))
    work = tmp_path / 'run_unet'
    shutil.copytree(src, work)
    deploy_network_ao.main(['--data_dir', str(work), '--model_path', mu, '--model', 'UNet', '--cine_scratch_gb', '1'])
    assert '--cine_scratch_gb is ignored' in capsys.readouterr().out
    assert (work / 's1' / 'seg_ao.nii.gz').exists()
