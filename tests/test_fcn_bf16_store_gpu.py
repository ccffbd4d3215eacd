"""--precision bf16_store (UKBB_PREC_BF16_STORE) end to end on the GPU: the drop-in script, precision switches on one handle, two engines on two
streams, and the refusal on the U-Net kinds.  The launches themselves are graded in tests/test_fcn_bf16_store_launches_gpu.py.

Dice against the fp32 run of the same phantom cine is held to >= 0.98 per class, the bound tests/test_deploy_gpu.py holds the bf16-storage U-Net to.
Measured on an MI355X (profiles/fcn_bf16_store.txt): sa 0.9901 / 0.9954 / 0.9973 (classes 1-3, 2417 of 459000 voxels differ), la_2ch 0.9975 (328 of 153000)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DICE_BOUND = 0.98


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
def test_deploy_script_under_bf16_store(tmp_path, seq, model, Z):
    """A phantom cine through deploy_network.main in fp32 and in bf16_store: complete files, per-class Dice >= 0.98; the sequential, pipelined and
    --device_inflate loops write the same bytes under the flag; --confidence_csv and --output_csv work under it."""
    from ukbb_cardiac_amd import deploy_network, nifti
    from ukbb_cardiac_amd.image_utils import np_categorical_dice
    arch, params, mp = _model(tmp_path, model)
    vol = _cine(tmp_path, seq, Z, 6, seed=8)
    files = ['seg_%s.nii.gz' % seq, '%s_ED.nii.gz' % seq, '%s_ES.nii.gz' % seq, 'seg_%s_ED.nii.gz' % seq, 'seg_%s_ES.nii.gz' % seq]
    runs = [('fp32', 'fp32', []), ('pipelined', 'bf16_store', []), ('sequential', 'bf16_store', ['--io_threads', '0']), ('inflate', 'bf16_store', ['--device_inflate', '2'])]
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
    print('fcn-bf16-store deploy %s: Dice against the fp32 run per class %s, %d of %d voxels differ' % (
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
    order = ('fp32', 'bf16_store', 'bf16', 'fp32')
    fresh = {}
    for prec in set(order):
        with Engine(arch, params) as eng:
            eng.set_precision(prec)
            fresh[prec] = eng.run(img, want_logits=True)
    with Engine(arch, params) as eng:
        for prec in order:
            eng.set_precision(prec)
            out = eng.run(img, want_logits=True)
            for k in ('logits', 'prob', 'pred'):
                assert np.array_equal(out[k].view(np.uint32), fresh[prec][k].view(np.uint32)), (prec, k)
            names, cfgs = eng.kernel_names(), eng.kernel_configs()       # the plan that ran: re-planned at every switch
            assert names[0] == 'conv0_0+conv0_1' and (cfgs[0] == -1) == (prec == 'bf16_store')            # the fused stem | a fused first-layer tiling
            assert all(c >= 230 for c in cfgs[1:12]) == (prec == 'bf16_store') and all(200 <= c < 230 for c in cfgs[1:12]) == (prec == 'bf16')
            # the FCN's bf16 maps come back as NHWC float holding bf16 values; G_l stays fp32
            c2 = eng.activation('conv2').reshape(5, 20, 28, 64)
            assert (not (c2.view(np.uint32) & 0xffff).any()) == (prec == 'bf16_store')
            assert (eng.activation('g2').view(np.uint32) & 0xffff).any()
    # the three modes are three different results
    assert not np.array_equal(fresh['fp32']['logits'], fresh['bf16_store']['logits']) and not np.array_equal(fresh['bf16']['logits'], fresh['bf16_store']['logits'])


def test_two_engines_on_two_streams_equal_the_single_stream_labels():
    """In a child process (tools/two_stream_check.py): two bf16_store engines on two streams, four batches in flight on each."""
    env = {k: v for k, v in os.environ.items() if not k.startswith('UKBB_')}
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    env['PREC'] = 'bf16_store'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'two_stream_check.py'), 'FCN_sa', '17', '96', '112', '24'], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout[-500:])
    assert r.returncode == 0 and r.stdout.strip().endswith('OK') and 'FCN_sa bf16_store 17x96x112: 24 forwards per stream on two streams, 0 with differing labels' in r.stdout, r.stdout[-3000:]


@pytest.mark.parametrize('model', ['UNet_ao', 'UNet-LSTM_ao'])
def test_a_unet_handle_refuses_the_code(model):
    from ukbb_cardiac_amd import _lib
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.engine import Engine
    from ukbb_cardiac_amd.weights import synthetic_params
    arch = MODELS[model]
    with Engine(arch, synthetic_params(arch, 1234)) as eng:
        with pytest.raises(_lib.UkbbFcnError) as e:
            eng.set_precision('bf16_store')
        assert 'failed (-2)' in str(e.value) and 'the U-Net kinds already store bf16 under UKBB_PREC_BF16' in str(e.value)
        eng.set_precision('bf16')                                  # ... and that still works
