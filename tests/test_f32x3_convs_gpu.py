"""ukbb_fcn_set_f32x3_convs end to end on the GPU: parity with the oracle under the rules of tests/test_gpu_parity.py's f32x3 tests, stability (batch
independence, switching on one handle, two engines on two streams) and the drop-in script.  The launches themselves are graded in
tests/test_f32x3_convs_launches_gpu.py.

Parity: the committed goldens (numpy float64) and one 2 x 32 x 48 batch against oracle/fcn_oracle.c -- logits within 1e-3 of their scale, no label
differing from the float64 argmax where the float64 top-two margin exceeds 1e-4.
Files: deploy_network.py --precision f32x3 --f32x3_convs writes the files of --precision f32x3 up to voxels next to a tie of the two largest logits
(float64 margin <= 1e-4 on the oracle), and its three loops write the same bytes."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_parity import FCN_GOLDENS, GOLD, LOGIT_RTOL, NEAR_TIE, _grade_vs_c_oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def x3_engine(arch, params, convs=True):
    from ukbb_cardiac_amd.engine import Engine
    eng = Engine(arch, params)
    eng.set_precision('f32x3')
    eng.set_f32x3_convs(convs)
    return eng


@pytest.fixture(scope='module')
def engines_x3c():
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.weights import synthetic_params
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = x3_engine(MODELS[name], synthetic_params(MODELS[name], 1234))
        return cache[name]
    yield get
    for e in cache.values():
        e.close()


@pytest.mark.parametrize('tag', FCN_GOLDENS)
def test_goldens_under_the_switch(engines_x3c, tag):
    g = np.load(os.path.join(GOLD, tag + '.npz'))
    eng = engines_x3c(str(g['model']))
    out = eng.run(g['image'], want_logits=True, want_prob=True, want_pred=True)
    assert set(eng.kernel_configs()[1:12]) <= set(range(330, 346))                     # the plan that ran is the switch's
    ref = g['logits64']
    scale = np.abs(ref).max()
    err = np.abs(out['logits'] - ref).max()
    bad = out['pred'] != g['pred64']
    print('f32x3-convs golden %-26s logits err/scale %.2e, %d labels differ from float64, %d of them away from a near-tie' % (
        tag, err / scale, int(bad.sum()), int((bad & (g['margin64'] > NEAR_TIE)).sum())))
    assert err <= LOGIT_RTOL * scale
    assert not np.any(bad & (g['margin64'] > NEAR_TIE))
    assert bad.sum() <= max(1, int((g['margin64'] <= NEAR_TIE).sum()))
    assert np.array_equal(np.argmax(out['prob'], -1).astype(np.int32), out['pred'])


def test_2x32x48_batch_against_the_c_oracle(engines_x3c):
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.phantom import uniform_slices
    from ukbb_cardiac_amd.weights import synthetic_params
    arch = MODELS['FCN_sa']
    rows = []
    _grade_vs_c_oracle(engines_x3c('FCN_sa'), arch, synthetic_params(arch, 1234), uniform_slices(2, 32, 48, seed=1), lambda **kw: rows.append(kw))
    print('f32x3-convs c-oracle 2x32x48: %s' % {k: rows[0][k] for k in ('rel_err', 'label_flips', 'flips_away_from_tie')})


def test_a_slice_is_bit_identical_in_batches_of_1_3_and_17(engines_x3c):
    from ukbb_cardiac_amd.phantom import uniform_slices
    eng = engines_x3c('FCN_sa')
    img = uniform_slices(17, 80, 112, seed=4)
    ref = [eng.run(img[i:i + 1], want_logits=True) for i in range(3)]
    for n in (3, 17):
        out = eng.run(img[:n], want_logits=True)
        for i in range(3):
            for k in ('logits', 'prob', 'pred'):
                assert np.array_equal(out[k][i].view(np.uint32), ref[i][k][0].view(np.uint32)), (n, i, k)
    again = eng.run(img[:1], want_logits=True)
    assert np.array_equal(again['logits'], ref[0]['logits'])


def test_switching_on_off_on_equals_fresh_handles():
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.phantom import cine_phantom
    from ukbb_cardiac_amd.weights import synthetic_params
    arch = MODELS['FCN_sa']
    params = synthetic_params(arch, 7)
    img = cine_phantom(5, 80, 112, seed=3)
    fresh = {}
    for convs in (True, False):
        with x3_engine(arch, params, convs) as eng:
            fresh[convs] = eng.run(img, want_logits=True)
            fresh[convs]['maps'] = {k: eng.activation(k).copy() for k in ('conv0', 'conv1', 'conv4', 'g4')}
    with x3_engine(arch, params, False) as eng:
        eng.set_precision('fp32')
        eng.set_f32x3_convs(True)                                  # kept and ignored under fp32
        kept = eng.run(img, want_logits=True)
        assert not set(eng.kernel_configs()) & set(range(330, 346))
        eng.set_precision('f32x3')                                 # ... and in effect once the precision is f32x3
        for convs in (True, False, True):
            eng.set_f32x3_convs(convs)
            out = eng.run(img, want_logits=True)
            assert (set(eng.kernel_configs()[1:12]) <= set(range(330, 346))) == convs
            for k in ('logits', 'prob', 'pred'):
                assert np.array_equal(out[k].view(np.uint32), fresh[convs][k].view(np.uint32)), (convs, k)
    with x3_engine(arch, params, False) as eng:
        eng.set_precision('fp32')
        plain = eng.run(img, want_logits=True)
    assert np.array_equal(kept['logits'].view(np.uint32), plain['logits'].view(np.uint32))
    # the stem is the fp32 launch of the f32x3 plan, bit for bit; the three-piece layers take another instruction sequence to the same fp32 accuracy
    assert np.array_equal(fresh[True]['maps']['conv0'].view(np.uint32), fresh[False]['maps']['conv0'].view(np.uint32))
    for k in ('conv1', 'conv4', 'g4'):
        a, b = fresh[True]['maps'][k], fresh[False]['maps'][k]
        assert not np.array_equal(a, b) and np.abs(a - b).max() <= 2e-5 * np.abs(b).max(), k
    assert np.abs(fresh[True]['logits'] - fresh[False]['logits']).max() <= 2e-5 * np.abs(fresh[False]['logits']).max()


def test_two_engines_on_two_streams_equal_the_single_stream_labels():
    """In a child process (tools/two_stream_check.py): two switch-on engines on two streams, four batches in flight on each."""
    env = {k: v for k, v in os.environ.items() if not k.startswith('UKBB_')}
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    env['PREC'] = 'f32x3'
    env['F32X3_CONVS'] = '1'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'two_stream_check.py'), 'FCN_sa', '17', '96', '112', '24'], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout[-500:])
    assert r.returncode == 0 and r.stdout.strip().endswith('OK') and 'FCN_sa f32x3+convs 17x96x112: 24 forwards per stream on two streams, 0 with differing labels' in r.stdout, r.stdout[-3000:]


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


def test_deploy_script_under_the_flag(tmp_path):
    """A phantom short-axis cine through deploy_network.main under --precision f32x3 with and without --f32x3_convs: complete files; the label volumes
    differ only at voxels where the float64 oracle's top-two margin is <= 1e-4; the sequential, pipelined and --device_inflate loops write the same
    bytes under the flag."""
    from oracle import fcn_oracle as O
    from ukbb_cardiac_amd import deploy_network, nifti, pipeline
    seq = 'sa'
    arch, params, mp = _model(tmp_path, 'FCN_sa')
    vol = _cine(tmp_path, seq, 3, 4, seed=8)
    files = ['seg_%s.nii.gz' % seq, '%s_ED.nii.gz' % seq, '%s_ES.nii.gz' % seq, 'seg_%s_ED.nii.gz' % seq, 'seg_%s_ES.nii.gz' % seq]
    runs = [('plain', [], []), ('pipelined', ['--f32x3_convs'], []), ('sequential', ['--f32x3_convs'], ['--io_threads', '0']),
            ('inflate', ['--f32x3_convs'], ['--device_inflate', '2'])]
    seg, raw = {}, {}
    for tag, flag, extra in runs:
        work = tmp_path / tag
        shutil.copytree(str(tmp_path / 'src'), str(work))
        deploy_network.main(['--seq_name', seq, '--data_dir', str(work), '--model_path', mp, '--precision', 'f32x3'] + flag + extra)
        for f in files:
            assert os.path.getsize(str(work / 'subj1' / f)) > 0, (tag, f)
        raw[tag] = [open(str(work / 'subj1' / f), 'rb').read() for f in files]
        seg[tag] = nifti.load(str(work / 'subj1' / files[0])).get_data()
        assert seg[tag].shape == vol.shape and seg[tag].dtype == np.float64
    assert raw['pipelined'] == raw['sequential'] == raw['inflate']
    differ = seg['pipelined'] != seg['plain']
    print('f32x3-convs deploy %s: %d of %d voxels differ from the --precision f32x3 run' % (seq, int(differ.sum()), differ.size))
    if differ.any():                                               # every differing voxel sits next to a tie of the float64 oracle's two largest logits
        Z_ = vol.shape[2]
        need = {int(t) * Z_ + int(z) for _, _, z, t in np.argwhere(differ)}     # slice order of pipeline.segment_sequence: frame-major

        def near_tie(batch):                                       # stands for the forward: 1 where the float64 margin of the slice is a near-tie
            mask = np.ones(batch.shape[:3], np.int32)
            for i in sorted(need):
                ref64 = O.build_FCN(np.asarray(batch[i:i + 1], np.float32), params, arch.n_class, dtype=np.float64)
                mask[i] = O.top2_margin(ref64)[0] <= NEAR_TIE
            return {'pred': mask}
        tie = pipeline.segment_sequence(vol.copy(), near_tie, 128, False)
        assert tie.shape == differ.shape and (tie[differ] == 1).all(), int((tie[differ] != 1).sum())
    assert differ.sum() <= max(2, 40 * differ.size // 1000000)
