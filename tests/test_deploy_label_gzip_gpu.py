"""deploy_network --device_label_gzip against the run without the flag, file by file, with both code sets of --label_gzip: under the
'threshold' weights (compact regions; tests/test_device_label_gzip.py asserts on the CPU that these subjects compress below
nifti.NOISE_FRACTION and fit the encoder's capacity) every subject must take the device encoder, under random weights (noise
labels) every subject must fall back -- and every output file is byte-identical either way."""
import os
import shutil

import numpy as np
import pytest

import deploy_label_gzip_fixtures as F

pytestmark = pytest.mark.gpu
FILES = ['seg_sa.nii.gz', 'sa_ED.nii.gz', 'sa_ES.nii.gz', 'seg_sa_ED.nii.gz', 'seg_sa_ES.nii.gz']


def make_cohort(src, weights):
    from ukbb_cardiac_amd import nifti
    subjects, volume, _ = F.cohort(weights)
    for name, shape, seed in subjects:
        os.makedirs(str(src / name))
        nifti.save(volume(shape, seed), str(src / name / 'sa.nii.gz'), F.AFFINE, F.PIXDIM)
    return subjects


def deploy(cohort, work, model_path, extra, io_threads=2):
    from ukbb_cardiac_amd import deploy_network, nifti
    from ukbb_cardiac_amd.sequence_run import SequenceRun
    shutil.copytree(str(cohort), str(work))
    mode = nifti.LABEL_GZIP_MODE
    try:
        deploy_network.main(['--seq_name', 'sa', '--data_dir', str(work), '--model_path', model_path, '--io_threads', str(io_threads)] + extra)
    finally:
        nifti.set_label_gzip(mode)
    return dict(SequenceRun.last_phases)


@pytest.mark.parametrize('weights,taken', [('threshold', True), ('random', False)])
def test_same_files_with_and_without_the_flag(tmp_path, weights, taken):
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.weights import save_blob
    arch = MODELS[F.MODEL]
    mp = str(tmp_path / F.MODEL)
    save_blob(mp + '.ukbbw', arch, F.cohort(weights)[2])
    cohort = tmp_path / 'cohort'
    subjects = make_cohort(cohort, weights)
    n = len(subjects)
    for code in ('small', 'fast'):
        off = deploy(cohort, tmp_path / ('off_' + code), mp, ['--label_gzip', code])
        on = deploy(cohort, tmp_path / ('on_' + code), mp, ['--label_gzip', code, '--device_label_gzip'])
        assert 'label_gzip_device' not in off
        print(weights, code, {k: on[k] for k in ('label_gzip_device', 'label_gzip_fallback')})
        assert (on['label_gzip_device'], on['label_gzip_fallback']) == ((n, 0) if taken else (0, n)), (code, on)
        for name, _, _ in subjects:
            for nm in FILES:
                a, b = tmp_path / ('off_' + code) / name / nm, tmp_path / ('on_' + code) / name / nm
                assert a.exists() and b.exists() and a.read_bytes() == b.read_bytes(), (code, name, nm)
            assert sorted(os.listdir(str(tmp_path / ('on_' + code) / name))) == sorted(FILES + ['sa.nii.gz']), name      # no temporary left


def test_a_larger_subject_leaves_the_pipeline_and_the_files_stay_the_same(tmp_path):
    """Mixed sizes with the flag on: one reader thread, so the first (small) subject sizes the pipeline; the larger third subject is
    segmented on the one-subject path and written by the host writer, the three others take the device encoder, before and behind
    it.  Every file equals the run without the flag."""
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.weights import save_blob
    mp = str(tmp_path / F.MODEL)
    save_blob(mp + '.ukbbw', MODELS[F.MODEL], F.cohort('mixed')[2])
    cohort = tmp_path / 'cohort'
    subjects = make_cohort(cohort, 'mixed')
    assert max(int(np.prod(sh)) for _, sh, _ in subjects) > int(np.prod(subjects[0][1]))
    off = deploy(cohort, tmp_path / 'off', mp, [], io_threads=1)
    on = deploy(cohort, tmp_path / 'on', mp, ['--device_label_gzip'], io_threads=1)
    assert 'label_gzip_device' not in off
    assert (on['label_gzip_device'], on['label_gzip_fallback']) == (len(subjects) - 1, 0), on
    for name, _, _ in subjects:
        for nm in FILES:
            assert (tmp_path / 'off' / name / nm).read_bytes() == (tmp_path / 'on' / name / nm).read_bytes(), (name, nm)
        assert sorted(os.listdir(str(tmp_path / 'on' / name))) == sorted(FILES + ['sa.nii.gz']), name


def test_the_flag_is_ignored_with_zlib_and_outside_the_pipelined_loop(tmp_path, capsys):
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.weights import save_blob, threshold_params
    arch = MODELS[F.MODEL]
    mp = str(tmp_path / F.MODEL)
    save_blob(mp + '.ukbbw', arch, threshold_params(arch))
    cohort = tmp_path / 'cohort'
    make_cohort(cohort, 'threshold')
    ref = deploy(cohort, tmp_path / 'ref', mp, ['--label_gzip', 'zlib'])
    assert capsys.readouterr().out.count('--device_label_gzip ignored') == 0
    phases = deploy(cohort, tmp_path / 'zlib', mp, ['--label_gzip', 'zlib', '--device_label_gzip'])
    assert 'label_gzip_device' not in phases and 'label_gzip_device' not in ref
    assert capsys.readouterr().out.count('--device_label_gzip ignored') == 1
    for name, _, _ in F.SUBJECTS:
        for nm in FILES:
            assert (tmp_path / 'zlib' / name / nm).read_bytes() == (tmp_path / 'ref' / name / nm).read_bytes(), (name, nm)
    seq = deploy(cohort, tmp_path / 'sequential', mp, ['--device_label_gzip'], io_threads=0)
    assert 'label_gzip_device' not in seq and capsys.readouterr().out.count('--device_label_gzip ignored') == 1
