"""ukbb_fcn_gzip_labels_device on the MI355X against the host writer ukbb_fcn_gzip_labels_mode: equal length and equal bytes over
the corpus of tests/label_gzip_corpus.py (what the parallel formulation has passed on the host, under the sanitizers too), every
datatype and both code sets, with guard bands behind d_out and behind the scratch (whose last part is the run table) that must
not change -- in the success and in both decline cases; and SubjectPipeline with the option on and off."""
import numpy as np
import pytest

import label_gzip_corpus as K
from test_device_label_gzip import NAMES, corpus, library

pytestmark = pytest.mark.gpu
_WANT = {}


def host_blob(name, datatype, mode):
    key = (name, datatype, mode)
    if key not in _WANT:
        _WANT[key] = K.host_writer(library(), corpus()[name], datatype, mode, K.prefix_of(name))
    return _WANT[key]


def device_gzip(lab, datatype, mode, cap, max_runs, prefix=K.PREFIX, shift=0):
    """-> (*d_len, the out_cap bytes, guards untouched?).  shift: misalignment of the label pointer (the byte-wise loads)."""
    import torch
    from ukbb_cardiac_amd import _lib
    d_all = torch.zeros(lab.size + 16, dtype=torch.uint8, device='cuda')
    d_lab = d_all[shift:shift + lab.size]
    d_lab.copy_(torch.from_numpy(np.ascontiguousarray(lab)))
    d_pre = torch.from_numpy(np.frombuffer(prefix, np.uint8).copy()).cuda()
    pad = (-cap) % 4                                                    # the guard starts at out_cap, whatever its alignment
    d_out = torch.full((cap + K.GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    scratch = int(_lib.lib.ukbb_fcn_gzip_labels_device_scratch(lab.size, max_runs))
    assert scratch > 0 and pad >= 0
    d_scr = torch.full((scratch + K.GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    d_len = torch.zeros(1, dtype=torch.int64, device='cuda')
    _lib.check(_lib.lib.ukbb_fcn_gzip_labels_device(d_lab.data_ptr(), lab.size, datatype, d_pre.data_ptr(), len(prefix), mode, d_out.data_ptr(), cap,
                                                    d_scr.data_ptr(), max_runs, d_len.data_ptr(), torch.cuda.current_stream().cuda_stream),
               'ukbb_fcn_gzip_labels_device')
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    guards = bool((out[cap:] == 0xA5).all()) and bool((d_scr[scratch:] == 0xA5).all().item())
    return int(d_len.item()), out[:cap], guards


@pytest.mark.parametrize('mode', [K.FIXED, K.DYNAMIC])
@pytest.mark.parametrize('name', NAMES)
def test_equal_bytes(name, mode):
    lab = corpus()[name]
    for datatype in K.DATATYPES:
        want = host_blob(name, datatype, mode)
        # exactly the member's length and exactly the volume's run count: the tightest buffers that succeed
        got, out, guards = device_gzip(lab, datatype, mode, len(want), K.n_runs(lab), K.prefix_of(name))
        assert got == len(want), (datatype, got, len(want))
        assert out.tobytes() == want, datatype
        assert guards, datatype


@pytest.mark.parametrize('shift', [1, 7])
def test_roomy_buffers_and_unaligned_labels(shift):
    for name in ('run_lengths', 'scan_borders', 'blob_phantom'):
        lab = corpus()[name]
        want = host_blob(name, 64, K.DYNAMIC)
        got, out, guards = device_gzip(lab, 64, K.DYNAMIC, len(want) + 4099, lab.size, shift=shift)
        assert got == len(want) and out[:got].tobytes() == want and guards, name
        assert not out[got:].any(), name                                # the room behind the member holds the chain's zeros


@pytest.mark.parametrize('mode', [K.FIXED, K.DYNAMIC])
def test_declines(mode):
    for name in ('run_lengths', 'noise_0_3', 'zeros_70001', 'window_crossing'):
        lab = corpus()[name]
        for datatype in (2, 64):
            size = len(host_blob(name, datatype, mode))
            got, _, guards = device_gzip(lab, datatype, mode, size - 1, K.n_runs(lab))            # out_cap one byte short
            assert got == K.NO_ROOM and guards, (name, datatype, got)
            if K.n_runs(lab) > 1:
                got, _, guards = device_gzip(lab, datatype, mode, size, K.n_runs(lab) - 1)        # one run more than max_runs
                assert got == K.TOO_MANY_RUNS and guards, (name, datatype, got)
    got, _, guards = device_gzip(corpus()['noise_0_255'], 64, mode, 100, 7)                       # not even the head fits; few table entries
    assert got in (K.NO_ROOM, K.TOO_MANY_RUNS) and guards


def test_bad_arguments_are_refused_without_a_launch():
    import torch
    from ukbb_cardiac_amd import _lib
    t = torch.zeros(4096, dtype=torch.uint8, device='cuda')
    p = t.data_ptr()
    call = lambda n, dt, mode, out, runs: _lib.lib.ukbb_fcn_gzip_labels_device(p, n, dt, p, 352, mode, out, 1024, p, runs, p, 0)
    assert call(0, 64, 1, p, 8) == -1 and call(8, 3, 1, p, 8) == -1 and call(8, 64, 2, p, 8) == -1 and call(8, 64, 1, p + 2, 8) == -1
    assert call(8, 64, 1, p, 0) == -1 and 'gzip_labels_device' in _lib.last_error()
    assert _lib.lib.ukbb_fcn_gzip_labels_device_scratch(0, 8) == 0


def test_subject_pipeline_with_the_option_on_and_off():
    """Same counts and statistics, a blob equal to the host writer's on the labels the plain pipeline collects, label_frames equal
    to those labels' frames; a noise-like subject and one without gz_header come back with ordinary labels."""
    import torch
    import deploy_label_gzip_fixtures as F
    from ukbb_cardiac_amd import device_pipeline as dp, nifti
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.engine import Engine
    from ukbb_cardiac_amd.subject_pipeline import SubjectPipeline
    from ukbb_cardiac_amd.weights import threshold_params
    arch = MODELS[F.MODEL]
    vols = [np.asfortranarray(F.volume(shape, seed)) for _, shape, seed in F.SUBJECTS]
    X = vols[0].shape[0]                                                # stripes three voxels wide: a run every third voxel, too many for the run table
    noise = np.asfortranarray(np.broadcast_to((1000.0 * ((np.arange(X) // 3) % 2))[:, None, None, None], vols[0].shape).astype(np.float32))
    vols.append(noise)
    biggest = max((v.shape for v in vols), key=lambda sh: int(np.prod(sh)))
    with Engine(arch, threshold_params(arch), device=0) as eng:
        stats = (dp.GateStats('sa', False),)
        plain = SubjectPipeline(eng, biggest, batch_slices=8, depth=3, extra_inputs=1, stats=stats)
        want = []
        for v in vols:
            plain.submit(v)
            r = plain.collect()
            want.append((r.labels, r.counts, r.stats))
            r.done()
        for mode, code in (('small', K.DYNAMIC), ('fast', K.FIXED)):
            pipe = SubjectPipeline(eng, biggest, batch_slices=8, depth=3, extra_inputs=4, stats=stats, device_label_gzip=mode)
            header = lambda i: (F.AFFINE, F.PIXDIM) if i != 1 else None       # subject 1 goes without: ordinary labels
            results = []
            pipe.submit(vols[0], None, header(0))
            pipe.submit(vols[1], None, header(1))
            results.append((0, pipe.collect()))                         # two in flight, as the deploy loop keeps them
            pipe.submit(vols[2], None, header(2))
            first = results[0][1]
            frames = first.label_frames(0, vols[0].shape[3] - 1)        # two submits later: the slot still holds the labels
            assert np.array_equal(frames[0], want[0][0][..., 0]) and np.array_equal(frames[1], want[0][0][..., -1])
            for i in range(3, len(vols)):
                results.append((i - 2, pipe.collect()))
                pipe.submit(vols[i], None, header(i))
            while pipe.pending():
                results.append((len(results), pipe.collect()))
            for k, r in results:
                lab, cnt, st = want[k]
                assert np.array_equal(r.counts, cnt)
                assert set(r.stats) == set(st) == {'qc'} and set(r.stats['qc']) == set(st['qc'])
                assert all(np.array_equal(r.stats['qc'][key], st['qc'][key]) for key in st['qc']), k
                if k == 1 or k == len(vols) - 1:
                    assert r.gz_blob is None and np.array_equal(r.labels, lab), k
                    assert k == 1 or len(np.unique(lab)) > 1
                    r.done()
                    continue
                prefix = nifti.header_prefix(lab.shape, F.AFFINE, F.PIXDIM, np.float64)
                assert r.labels is None and r.gz_blob == K.host_writer(library(), lab.reshape(-1, order='F'), 64, code, prefix), (mode, k)
                r.done()
            try:                                                        # depth more submits: the slot has been reused and says so,
                late = first.label_frames(0)
            except RuntimeError:
                pass
            else:                                                       # or was re-made for another shape, and its buffers live on with the result
                assert np.array_equal(late[0], want[0][0][..., 0])
    torch.cuda.synchronize()
