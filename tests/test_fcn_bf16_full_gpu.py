"""--precision bf16_full (UKBB_PREC_BF16_FULL) end to end on the GPU: the drop-in script, precision switches on one handle, two engines on two streams,
and the refusal on the other kinds.  The launches themselves are graded in tests/test_fcn_bf16_full_launches_gpu.py.

Dice against the fp32 run of the same phantom cine is held to >= 0.98 per class, the project's bound for its bf16 modes.
Measured on an MI355X (profiles/fcn_bf16_full.txt): sa 0.9897 / 0.9956 / 0.9972 (classes 1-3, 2431 of 459000 voxels differ), la_2ch 0.9955 (585 of 153000)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DICE_BOUND = 0.98
PREC = 'bf16_full'


def _model(tmp_path, name):
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.weights import save_blob, synthetic_params
    arch = MODELS[name]
    params = synthetic_params(arch, 1234)
    mp = str(tmp_path / name)
    save_blob(mp + '.ukbbw', arch, params)
    return arch, params, mp


def _cine(tmp_path, seq, Z, T, seed):
    """A phantom cine [X, Y, Z, T] as src/subj1/<seq>.nii.gz."""
    from ukbb_cardiac_amd import nifti
    from ukbb_cardiac_amd.phantom import cine_phantom
    X, Y = 150, 170
    vol = np.round(cine_phantom(Z * T, X, Y, seed=seed)[..., 0].reshape(T, Z, X, Y).transpose(2, 3, 1, 0) * 1000.0).astype(np.float32)
    src = tmp_path / 'src' / 'subj1'
    src.mkdir(parents=True)
    nifti.save(vol, str(src / (seq + '.nii.gz')), np.diag([1.8, 1.8, 10.0, 1.0]), pixdim=[1, 1.8, 1.8, 10, 0.03, 0, 0, 0])
    return vol


@pytest.mark.parametrize('seq,model,Z', [('sa', 'FCN_sa', 3), ('la_2ch', 'FCN_la_2ch', 1)])
def test_deploy_script_under_bf16_full(tmp_path, seq, model, Z):
    """A phantom cine through deploy_network.main in fp32 and in bf16_full: complete files, per-class Dice >= 0.98; the sequential, pipelined and
    --device_inflate loops write the same bytes under the flag; --confidence_csv and --output_csv work under it."""
    from ukbb_cardiac_amd import deploy_network, nifti
    from ukbb_cardiac_amd.image_utils import np_categorical_dice
    arch, params, mp = _model(tmp_path, model)
    vol = _cine(tmp_path, seq, Z, 6, seed=8)
    files = ['seg_%s.nii.gz' % seq, '%s_ED.nii.gz' % seq, '%s_ES.nii.gz' % seq, 'seg_%s_ED.nii.gz' % seq, 'seg_%s_ES.nii.gz' % seq]
    runs = [('fp32', 'fp32', []), ('pipelined', PREC, []), ('sequential', PREC, ['--io_threads', '0']), ('inflate', PREC, ['--device_inflate', '2'])]
    seg, raw, csvs = {}, {}, {}
    for tag, prec, extra in runs:
        work = tmp_path / tag
        shutil.copytree(str(tmp_path / 'src'), str(work))
        conf = str(tmp_path / (tag + '_conf.csv'))
        tables = ['--confidence_csv', conf] + (['--output_csv', str(tmp_path / (tag + '_vol.csv'))] if seq == 'sa' else [])
        deploy_network.main(['--seq_name', seq, '--data_dir', str(work), '--model_path', mp, '--precision', prec] + tables + extra)
        for f in files:
            assert os.path.getsize(str(work / 'subj1' / f)) > 0, (tag, f)
        raw[tag] = [open(str(work / 'subj1' / f), 'rb').read() for f in files]
        seg[tag] = nifti.load(str(work / 'subj1' / files[0])).get_data()
        csvs[tag] = [open(conf, newline='').read()] + ([open(str(tmp_path / (tag + '_vol.csv')), newline='').read()] if seq == 'sa' else [])
        assert seg[tag].shape == vol.shape and seg[tag].dtype == np.float64
        assert all(len(t.splitlines()) >= 2 for t in csvs[tag]), tag                       # a header and rows
    assert raw['pipelined'] == raw['sequential'] == raw['inflate'] and csvs['pipelined'] == csvs['sequential'] == csvs['inflate']
    present = [k for k in range(1, arch.n_class) if (seg['fp32'] == k).any()]
    assert present, 'the fp32 run labels no foreground class'
    dice = {k: float(np_categorical_dice(seg['pipelined'], seg['fp32'], k)) for k in present}
    print('fcn-bf16-full deploy %s: Dice against the fp32 run per class %s, %d of %d voxels differ' % (
        seq, {k: round(v, 4) for k, v in dice.items()}, int((seg['pipelined'] != seg['fp32']).sum()), seg['fp32'].size))
    assert all(v >= DICE_BOUND for v in dice.values()), dice


def test_precision_switches_on_one_handle_give_the_bits_of_fresh_handles():
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.engine import Engine
    from ukbb_cardiac_amd.phantom import cine_phantom
    from ukbb_cardiac_amd.weights import synthetic_params
    arch = MODELS['FCN_sa']
    params = synthetic_params(arch, 7)
    img = cine_phantom(5, 80, 112, seed=3)
    order = ('fp32', PREC, 'bf16_store', PREC)
    fresh = {}
    for prec in set(order):
        with Engine(arch, params) as eng:
            eng.set_precision(prec)
            fresh[prec] = eng.run(img, want_logits=True)
            fresh[prec]['maps'] = {k: eng.activation(k).copy() for k in ('conv0', 'conv4', 'g1', 'g4')}
    with Engine(arch, params) as eng:
        for prec in order:
            eng.set_precision(prec)
            out = eng.run(img, want_logits=True)
            for k in ('logits', 'prob', 'pred'):
                assert np.array_equal(out[k].view(np.uint32), fresh[prec][k].view(np.uint32)), (prec, k)
            names, cfgs = eng.kernel_names(), eng.kernel_configs()       # the plan that ran: re-planned at every switch
            assert names[0] == 'conv0_0+conv0_1' and (cfgs[0] == -1) == (prec != 'fp32') and names[-2:] == ['sqg1-4', 'head']
            assert all(c >= 230 for c in cfgs[1:12]) == (prec != 'fp32')
    # the encoder and the squeeze of the new mode are bf16_store's, bit for bit; its head is not
    for k, a in fresh[PREC]['maps'].items():
        assert np.array_equal(a.view(np.uint32), fresh['bf16_store']['maps'][k].view(np.uint32)), k
    assert not np.array_equal(fresh[PREC]['logits'], fresh['bf16_store']['logits']) and not np.array_equal(fresh[PREC]['logits'], fresh['fp32']['logits'])


def test_two_engines_on_two_streams_equal_the_single_stream_labels():
    """In a child process (tools/two_stream_check.py): two bf16_full engines on two streams, four batches in flight on each."""
    env = {k: v for k, v in os.environ.items() if not k.startswith('UKBB_')}
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    env['PREC'] = PREC
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'two_stream_check.py'), 'FCN_sa', '17', '96', '112', '24'], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout[-500:])
    assert r.returncode == 0 and r.stdout.strip().endswith('OK') and 'FCN_sa bf16_full 17x96x112: 24 forwards per stream on two streams, 0 with differing labels' in r.stdout, r.stdout[-3000:]


@pytest.mark.parametrize('model', ['UNet_ao', 'UNet-LSTM_ao', 'Temporal-UNet_ao'])
def test_the_other_kinds_refuse_the_code_on_a_live_handle(model):
    from ukbb_cardiac_amd import _lib
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.engine import Engine
    from ukbb_cardiac_amd.weights import synthetic_params
    arch = MODELS[model]
    with Engine(arch, synthetic_params(arch, 1234)) as eng:
        with pytest.raises(_lib.UkbbFcnError) as e:
            eng.set_precision(PREC)
        assert 'failed (-2)' in str(e.value) and 'UKBB_PREC_BF16_FULL' in str(e.value)
        eng.set_precision('fp32')                                  # ... and the handle still takes its own modes
