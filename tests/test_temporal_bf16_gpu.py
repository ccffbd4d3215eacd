"""The Temporal-UNet under precision 'bf16_3d' (UKBB_PREC_BF16_3D) end to end on the GPU: cines against the deploy loop, precision switches on one
handle, the deploy script, two engines on two streams.  The launches themselves are graded in tests/test_temporal_bf16_launches_gpu.py.

Dice of the deploy script's label volume against the fp32 run of the same phantom cine, measured on an MI355X (profiles/temporal_bf16.txt): see
DICE_MEASURED (0.9977 and 0.9913); the bound is the lower of 0.98 (what the project holds its other bf16 modes to, tests/test_fcn_bf16_store_gpu.py)
and the measured value - 0.01, that is 0.98."""
import os
import shutil
import threading

import numpy as np
import pytest

import temporal_unet_ref as R

pytestmark = pytest.mark.gpu
PRECISION = 'bf16_3d'
DICE_MEASURED = {1: 0.9977, 2: 0.9913}  # per class on an MI355X, profiles/temporal_bf16.txt (248 of 69300 voxels differ)
DICE_BOUND = min(0.98, min(DICE_MEASURED.values()) - 0.01)


def _model():
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.weights import synthetic_params
    arch = MODELS['Temporal-UNet_ao']
    return arch, synthetic_params(arch, 1234)


@pytest.fixture(scope='module')
def bf16_engine():
    from ukbb_cardiac_amd.engine import Engine
    arch, params = _model()
    with Engine(arch, params) as eng:
        eng.set_precision(PRECISION)
        yield arch, eng


@pytest.fixture(scope='module')
def cines(bf16_engine):
    """{time_step: (frames, the deploy loop's prob from single-window run_seq calls on the same handle)}: computed once, shared, left unchanged."""
    arch, eng = bf16_engine
    frames = np.random.default_rng(12).standard_normal((12, 32, 32)).astype(np.float32)
    os.environ.pop('UKBB_TEMPORAL_CHUNK_WINDOWS', None)
    return {step: (frames, R.deploy_tiling(frames, lambda w: eng.run_seq(w)['prob'], step)) for step in (1, 10)}


def _assert_cine(prob, pred, exact):
    np.testing.assert_array_equal(prob, exact)                           # NaNs (frames no window reaches) compare equal here
    np.testing.assert_array_equal(pred, np.argmax(exact, -1).astype(np.int32))


@pytest.mark.parametrize('time_step', [1, 10])
@pytest.mark.parametrize('chunk', [None, '1', '4'])
def test_cine_is_the_deploy_loop_bit_for_bit_whatever_the_chunk(bf16_engine, cines, time_step, chunk, monkeypatch):
    arch, eng = bf16_engine
    frames, exact = cines[time_step]
    if chunk is None:
        monkeypatch.delenv('UKBB_TEMPORAL_CHUNK_WINDOWS', raising=False)
    else:
        monkeypatch.setenv('UKBB_TEMPORAL_CHUNK_WINDOWS', chunk)
    prob, pred = eng.run_cine(frames, time_step=time_step)
    assert np.isnan(exact).any() == (time_step == 10)                    # time_step 10 leaves frames no window reaches
    _assert_cine(prob, pred, exact)
    assert len(np.unique(pred)) > 1


def test_cine_under_a_scratch_budget_that_forces_several_chunks(cines, monkeypatch):
    from ukbb_cardiac_amd import engine
    from ukbb_cardiac_amd.engine import Engine
    arch, params = _model()
    frames, exact = cines[1]
    F, H, W = frames.shape
    monkeypatch.delenv('UKBB_TEMPORAL_CHUNK_WINDOWS', raising=False)
    budget = engine.cine_scratch_bytes(arch, PRECISION, F, H, W, budget=0) // 3
    cw = engine.cine_chunk_windows(arch, PRECISION, F, H, W, budget=budget)
    assert 1 <= cw < F // 2, cw                                          # more than two chunks
    assert cw >= engine.cine_chunk_windows(arch, 'fp32', F, H, W, budget=budget)
    with Engine(arch, params) as eng:
        eng.set_precision(PRECISION)
        eng.set_scratch_budget(budget)
        prob, pred = eng.run_cine(frames, time_step=1)
        held = eng.scratch_bytes()
    assert held == engine.cine_scratch_bytes(arch, PRECISION, F, H, W, budget=budget) <= budget
    _assert_cine(prob, pred, exact)


def test_precision_switches_on_one_handle_give_the_bits_of_fresh_handles():
    from ukbb_cardiac_amd.engine import Engine
    arch, params = _model()
    x = np.random.default_rng(5).standard_normal((2, arch.fc, 32, 48, 1)).astype(np.float32)
    fresh = {}
    for prec in ('fp32', PRECISION):
        with Engine(arch, params) as eng:
            eng.set_precision(prec)
            fresh[prec] = eng.run_seq(x, want_logits=True)
    with Engine(arch, params) as eng:
        for prec in ('fp32', PRECISION, 'fp32', PRECISION):
            eng.set_precision(prec)
            out = eng.run_seq(x, want_logits=True)
            for k in ('logits', 'prob', 'pred'):
                assert np.array_equal(out[k].view(np.uint32), fresh[prec][k].view(np.uint32)), (prec, k)
            c2 = eng.activation('conv2_1')                               # NHWC float either way; bf16 values under bf16_3d only
            assert (not (c2.view(np.uint32) & 0xffff).any()) == (prec == PRECISION)
    assert not np.array_equal(fresh['fp32']['logits'], fresh[PRECISION]['logits'])
    scale = float(np.abs(fresh['fp32']['logits']).max())
    d = float(np.abs(fresh['fp32']['logits'] - fresh[PRECISION]['logits']).max())
    print('temporal-bf16 switch: max |bf16_3d - fp32| logits %.3g of scale %.3g; %d of %d labels differ' % (
        d, scale, int((fresh['fp32']['pred'] != fresh[PRECISION]['pred']).sum()), fresh['fp32']['pred'].size))


def test_forward_stays_refused_under_the_code(bf16_engine):
    from ukbb_cardiac_amd import _lib
    arch, eng = bf16_engine
    with pytest.raises(_lib.UkbbFcnError, match='sequences'):
        eng.run(np.zeros((1, 32, 32, 1), np.float32))
    for prec in ('bf16', 'bf16_store'):
        with pytest.raises(_lib.UkbbFcnError, match=r'fp32 only'):
            eng.set_precision(prec)
    x = np.random.default_rng(1).standard_normal((1, arch.fc, 32, 32, 1)).astype(np.float32)
    assert eng.run_seq(x)['pred'].shape == (1, arch.fc, 32, 32)         # the handle still works, still in bf16_3d
    assert not (eng.activation('up0_1').view(np.uint32) & 0xffff).any()


def test_deploy_script_under_bf16_3d(tmp_path):
    """A phantom cine through deploy_network_ao.main --model Temporal-UNet in fp32 and in bf16_3d: the pipelined, sequential and --nodevice_preproc
    loops write the same bytes under the flag; --output_csv and --confidence_csv are written; Dice per class against the fp32 run."""
    from ukbb_cardiac_amd import deploy_network_ao, nifti
    from ukbb_cardiac_amd.image_utils import np_categorical_dice
    from ukbb_cardiac_amd.phantom import cine_phantom
    from ukbb_cardiac_amd.weights import save_blob
    arch, params = _model()
    mp = str(tmp_path / 'Temporal-UNet_ao')
    save_blob(mp + '.ukbbw', arch, params)
    X, Y, T = 70, 90, 11
    vol = np.round(cine_phantom(T, X, Y, seed=8)[..., 0].reshape(T, 1, X, Y).transpose(2, 3, 1, 0) * 1000.0).astype(np.float32)
    src = tmp_path / 'src' / 'subj1'
    src.mkdir(parents=True)
    nifti.save(vol, str(src / 'ao.nii.gz'), np.diag([1.6, 1.6, 6.0, 1.0]), pixdim=[1, 1.6, 1.6, 6, 0.03, 0, 0, 0])
    runs = [('fp32', 'fp32', []), ('pipelined', PRECISION, []), ('sequential', PRECISION, ['--io_threads', '0']), ('host', PRECISION, ['--nodevice_preproc']),
            ('budget', PRECISION, ['--cine_scratch_gb', '0.4'])]        # the script pads to 256 x 256: two of the 11 windows per chunk
    seg, raw, csvs = {}, {}, {}
    for tag, prec, extra in runs:
        work = tmp_path / tag
        shutil.copytree(str(tmp_path / 'src'), str(work))
        conf, table = str(tmp_path / (tag + '_conf.csv')), str(tmp_path / (tag + '_ao.csv'))
        deploy_network_ao.main(['--data_dir', str(work), '--model_path', mp, '--model', 'Temporal-UNet', '--precision', prec, '--time_step', '1',
                                '--confidence_csv', conf, '--output_csv', table, '--noaortic_qc'] + extra)     # every segmented subject gets a row
        raw[tag] = open(str(work / 'subj1' / 'seg_ao.nii.gz'), 'rb').read()
        seg[tag] = nifti.load(str(work / 'subj1' / 'seg_ao.nii.gz')).get_data()
        csvs[tag] = [open(conf, newline='').read(), open(table, newline='').read()]
        assert seg[tag].shape == vol.shape
        assert all(len(t.splitlines()) >= 2 for t in csvs[tag]), tag                       # a header and rows
    assert raw['pipelined'] == raw['sequential'] == raw['host'] == raw['budget']
    assert csvs['pipelined'] == csvs['sequential'] == csvs['budget']
    present = [k for k in range(1, arch.n_class) if (seg['fp32'] == k).any()]
    assert present, 'the fp32 run labels no foreground class'
    dice = {k: float(np_categorical_dice(seg['pipelined'], seg['fp32'], k)) for k in present}
    print('temporal-bf16 deploy: Dice against the fp32 run per class %s, %d of %d voxels differ' % (
        {k: round(v, 4) for k, v in dice.items()}, int((seg['pipelined'] != seg['fp32']).sum()), seg['fp32'].size))
    assert all(v >= DICE_BOUND for v in dice.values()), dice


@pytest.mark.parametrize('model_flag,model_name', [('UNet', 'UNet_ao'), ('UNet-LSTM', 'UNet-LSTM_ao')])
def test_the_other_aortic_models_refuse_the_flag(tmp_path, model_flag, model_name):
    from ukbb_cardiac_amd import deploy_network_ao
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.weights import save_blob, synthetic_params
    mp = str(tmp_path / model_name)
    save_blob(mp + '.ukbbw', MODELS[model_name], synthetic_params(MODELS[model_name], 7))
    (tmp_path / 'data').mkdir()
    with pytest.raises(SystemExit) as e:
        deploy_network_ao.main(['--data_dir', str(tmp_path / 'data'), '--model_path', mp, '--model', model_flag, '--precision', PRECISION])
    assert 'Temporal-UNet' in str(e.value)


def test_two_engines_on_two_streams_one_per_thread_equal_the_single_stream_labels():
    import torch
    from ukbb_cardiac_amd.engine import Engine
    arch, params = _model()
    F, H, W, rounds = 12, 64, 64, 6
    dev = torch.device('cuda', 0)
    xs = [torch.from_numpy(np.random.default_rng(30 + i).standard_normal((F, H, W)).astype(np.float32)).to(dev) for i in range(2)]
    engs = [Engine(arch, params) for _ in range(2)]
    try:
        for e in engs:
            e.set_precision(PRECISION)
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
