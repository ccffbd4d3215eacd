"""The parallel formulation of the label-volume gzip writer (ukbb_fcn_gzip_labels_parallel_host: what the device encoder runs, step
by step on the host) against the serial writer ukbb_fcn_gzip_labels_mode: equal bytes over the corpus of tests/label_gzip_corpus.py,
for every datatype and both code sets; every member also against zlib alone; the two declines with a guard band behind out_cap; the
NIfTI prefix helper; the stand-alone sanitizer program; and the condition the deploy test of the device path rests on."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import label_gzip_corpus as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def library():
    from ukbb_cardiac_amd import _lib
    return _lib.lib


def geometry():
    g = (C.c_uint32 * 4)()
    library().ukbb_fcn_gzip_labels_device_geometry(C.byref(g))
    return tuple(int(v) for v in g)


_CORPUS = {}


def corpus():
    if not _CORPUS:
        _CORPUS.update(K.corpus(geometry()))
    return _CORPUS


NAMES = ['run_lengths', 'one_voxel', 'zeros_70001', 'threes_70001', 'noise_0_3', 'noise_0_255', 'blob_phantom', 'scan_borders',
         'last_run_single', 'window_crossing', 'adjacent_long_runs']


def test_corpus_names():
    assert list(corpus()) == NAMES
    g = geometry()
    assert K.n_runs(corpus()['scan_borders']) > 3 * g[1] and corpus()['window_crossing'].size * 8 // 258 * 14 > 4 * g[2]


def test_adjacent_long_runs_are_what_the_case_says():
    """At one and at eight bytes a voxel: runs the whole workgroup fills (>= geometry[3] (258, E) tokens) directly next to each
    other, and pairs of them with one short run between; all of them in one workgroup's span of runs; the fills of the first eight
    at least 2 bits x 1024 tokens = 64 words long (no token is shorter than 2 bits)."""
    lab, g = corpus()['adjacent_long_runs'], geometry()
    starts = np.flatnonzero(np.r_[True, lab[1:] != lab[:-1]])
    lens = np.diff(np.r_[starts, lab.size])
    assert len(lens) <= g[1]
    for E in (1, 8):
        long_ = (lens - 1) * E // 258 >= g[3]
        assert int(np.count_nonzero(long_[1:] & long_[:-1])) >= 8 and int(np.count_nonzero(long_[2:] & long_[:-2] & ~long_[1:-1])) >= 2, E
        assert int(np.count_nonzero((lens - 1) * E // 258 >= 1024)) >= 8, E


@pytest.mark.parametrize('mode', [K.FIXED, K.DYNAMIC])
@pytest.mark.parametrize('name', NAMES)
def test_equal_bytes(name, mode):
    lib, lab, prefix = library(), corpus()[name], K.prefix_of(name)
    for datatype in K.DATATYPES:
        want = K.host_writer(lib, lab, datatype, mode, prefix)
        assert isinstance(want, bytes), (datatype, want)
        got, blob, guard_ok = K.parallel_host(lib, lab, datatype, mode, len(want), K.n_runs(lab), prefix)
        assert got == len(want) and blob == want and guard_ok, (datatype, got, len(want))
        K.check_independently(blob, lab, datatype, prefix)


@pytest.mark.parametrize('mode', [K.FIXED, K.DYNAMIC])
def test_declines_leave_the_guard_band(mode):
    lib = library()
    for name in ('run_lengths', 'noise_0_3', 'zeros_70001'):
        lab = corpus()[name]
        for datatype in K.DATATYPES:
            size = len(K.host_writer(lib, lab, datatype, mode))
            got, _, guard_ok = K.parallel_host(lib, lab, datatype, mode, size - 1, K.n_runs(lab))      # out_cap one byte short
            assert got == K.NO_ROOM and guard_ok, (name, datatype, got)
            if K.n_runs(lab) > 1:                                                                      # one run more than max_runs
                got, _, guard_ok = K.parallel_host(lib, lab, datatype, mode, size, K.n_runs(lab) - 1)
                assert got == K.TOO_MANY_RUNS and guard_ok, (name, datatype, got)
    assert K.NO_ROOM != K.TOO_MANY_RUNS and K.NO_ROOM < 0 and K.TOO_MANY_RUNS < 0


def test_bad_arguments():
    lib = library()
    lab, out = np.zeros(8, np.uint8), np.zeros(4096, np.uint8)
    call = lambda n, dt, mode, runs: lib.ukbb_fcn_gzip_labels_parallel_host(lab.ctypes.data, n, dt, K.PREFIX, len(K.PREFIX), mode, out.ctypes.data, out.size, runs)
    assert call(8, 64, K.DYNAMIC, 8) > 0
    assert call(0, 64, K.DYNAMIC, 8) == -1 and call(8, 3, K.DYNAMIC, 8) == -1 and call(8, 64, 2, 8) == -1 and call(8, 64, K.DYNAMIC, 0) == -1


def test_prefix_helper_equals_the_saved_header(tmp_path):
    from ukbb_cardiac_amd import nifti
    rng = np.random.default_rng(2)
    affine = np.eye(4)
    affine[:3, :3] = rng.normal(size=(3, 3))
    affine[:3, 3] = (-10.5, 20.25, 3.0)
    pixdim = np.array([1, 1.8, 1.8, 10, 0.031, 1, 1, 1], np.float32)
    for shape, dtype, pd in (((6, 5, 4, 3), np.float64, pixdim), ((6, 5, 4), np.int16, None), ((7, 3), np.uint8, None)):
        lab = rng.integers(0, 4, shape).astype(np.uint8)
        path = str(tmp_path / 'v.nii.gz')
        nifti.save(lab, path, affine, pd, as_dtype=dtype)
        with open(path, 'rb') as f:
            raw = zlib.decompress(f.read(), 31)
        assert nifti.header_prefix(shape, affine, pd, dtype) == raw[:352]
    with pytest.raises(ValueError):
        nifti.header_prefix((4, 4), np.eye(3), None, np.uint8)


def test_save_gzip_blob_is_atomic_and_verbatim(tmp_path):
    from ukbb_cardiac_amd import nifti
    path = str(tmp_path / 'b.nii.gz')
    nifti.save_gzip_blob(b'abc' * 100, path)
    assert open(path, 'rb').read() == b'abc' * 100 and os.listdir(str(tmp_path)) == ['b.nii.gz']
    nifti.save_gzip_blob(np.frombuffer(b'xyz', np.uint8), path)
    assert open(path, 'rb').read() == b'xyz'


def test_every_way_the_flag_is_dropped_has_a_reason(monkeypatch):
    """sequence_run.device_label_gzip_mode: a code set or the reason deploy_network logs, never neither with the flag on."""
    from types import SimpleNamespace
    from ukbb_cardiac_amd import nifti
    from ukbb_cardiac_amd.sequence_run import device_label_gzip_mode
    on = SimpleNamespace(device_label_gzip=True, save_seg=True)
    assert device_label_gzip_mode(SimpleNamespace(device_label_gzip=False, save_seg=True)) == (None, None)
    for mode in ('small', 'fast'):
        monkeypatch.setattr(nifti, 'LABEL_GZIP_MODE', mode)
        assert device_label_gzip_mode(on) == (mode, None)
    mode, why = device_label_gzip_mode(SimpleNamespace(device_label_gzip=True, save_seg=False))
    assert mode is None and 'save_seg' in why
    monkeypatch.setattr(nifti, 'LABEL_FAST_PATH', False)
    mode, why = device_label_gzip_mode(on)
    assert mode is None and 'LABEL_FAST_PATH' in why
    monkeypatch.setattr(nifti, 'LABEL_FAST_PATH', True)
    monkeypatch.setattr(nifti, 'LABEL_GZIP_MODE', 'zlib')
    mode, why = device_label_gzip_mode(on)
    assert mode is None and '--label_gzip zlib keeps the host writer' in why


def write_corpus_file(path):
    """For tests/cpp/label_gzip_core_asan.cpp: uint32 count, then per case uint64 n_voxels, uint64 prefix_len, the prefix, the labels."""
    with open(path, 'wb') as f:
        f.write(struct.pack('<I', len(NAMES)))
        for name in NAMES:
            lab, prefix = corpus()[name], K.prefix_of(name)
            f.write(struct.pack('<QQ', lab.size, len(prefix)) + prefix + lab.tobytes())
    return len(NAMES)


def test_parallel_host_under_sanitizers(tmp_path):
    """A stand-alone program built with -fsanitize=address,undefined runs the parallel formulation and the serial writer over the
    corpus, every datatype and both code sets, labels and output in heap blocks of exactly their size."""
    exe, data = str(tmp_path / 'label_gzip_core_asan'), str(tmp_path / 'corpus.bin')
    n = write_corpus_file(data)
    csrc = os.path.join(ROOT, 'ukbb_cardiac_amd', 'csrc')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', csrc,
                           '-o', exe, os.path.join(ROOT, 'tests', 'cpp', 'label_gzip_core_asan.cpp'), os.path.join(csrc, 'label_gzip.cpp')])
    out = subprocess.run([exe, data], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert 'label_gzip_core ok: %d volumes' % n in out


def test_deploy_fixtures_compress_below_the_noise_fraction():
    """tests/test_deploy_label_gzip_gpu.py demands that every subject takes the device encoder under the 'threshold' weights: the
    host writer's ratio on the oracle's labels of those very subjects must lie below nifti.NOISE_FRACTION (else the subject would
    rightly fall back), and with either code set the member must fit the capacity, and its runs the run table, the pipeline gives
    the encoder."""
    from ukbb_cardiac_amd import nifti
    from ukbb_cardiac_amd.subject_pipeline import label_gzip_capacity, label_gzip_max_runs
    import deploy_label_gzip_fixtures as F
    for name, lab in F.oracle_labels():
        assert len(np.unique(lab)) > 1, name
        prefix = nifti.header_prefix(lab.shape, F.AFFINE, F.PIXDIM, np.float64)
        raw = len(prefix) + lab.size * 8
        runs = K.n_runs(lab.reshape(-1, order='F'))
        print(name, 'runs', runs, 'of', lab.size, 'voxels, run table', label_gzip_max_runs(lab.size))
        assert runs <= label_gzip_max_runs(lab.size), name
        for mode in (K.DYNAMIC, K.FIXED):
            blob = K.host_writer(library(), lab.reshape(-1, order='F'), 64, mode, prefix)
            print(name, 'mode', mode, 'ratio %.4f' % (len(blob) / raw), 'bytes', len(blob), 'capacity', label_gzip_capacity(lab.size, 8, len(prefix)))
            assert len(blob) <= label_gzip_capacity(lab.size, 8, len(prefix)), (name, mode)
            if mode == K.DYNAMIC:
                assert len(blob) / raw < nifti.NOISE_FRACTION, (name, len(blob) / raw)


def test_deploy_noise_fixtures_fall_back():
    """... and that every subject falls back under random weights: on the oracle's labels the 'small' member is larger than
    nifti.NOISE_FRACTION of the raw stream or the volume has more runs than the run table, and the 'fast' member exceeds the
    capacity or the run table."""
    from ukbb_cardiac_amd import nifti
    from ukbb_cardiac_amd.subject_pipeline import label_gzip_capacity, label_gzip_max_runs
    import deploy_label_gzip_fixtures as F
    for name, lab in F.oracle_labels('random'):
        prefix = nifti.header_prefix(lab.shape, F.AFFINE, F.PIXDIM, np.float64)
        raw = len(prefix) + lab.size * 8
        flat = lab.reshape(-1, order='F')
        too_many = K.n_runs(flat) > label_gzip_max_runs(lab.size)
        small, fast = (len(K.host_writer(library(), flat, 64, mode, prefix)) for mode in (K.DYNAMIC, K.FIXED))
        print(name, 'runs', K.n_runs(flat), 'of', lab.size, 'small ratio %.4f' % (small / raw), 'fast bytes', fast, 'capacity', label_gzip_capacity(lab.size))
        assert too_many or small / raw > nifti.NOISE_FRACTION, name
        assert too_many or fast > label_gzip_capacity(lab.size), name
