"""ukbb_fcn_inflate_device on the MI355X: the corpus of tests/test_device_inflate.py (what the host-compiled core has passed under
the sanitizers) in batches of very different sizes, byte for byte against zlib with guard bytes between the output regions; the
malformed list mixed into a batch of good streams; the CRC kernel around its chunk size; segment_sequence_tensor against
segment_sequence_device; deploy_network --device_inflate against the run without the flag, file by file; and the host path, the
sequential device path, the pipelined loop and the inflate rounds against each other: files, tables and log lines per subject."""
import gzip
import os
import re
import shutil
import struct
import zlib

import numpy as np
import pytest

from test_device_inflate import E_DATA, E_INPUT, E_OUTPUT, corpus, deflate, malformed

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 256


def crc_chunk():
    hdr = open(os.path.join(ROOT, 'include', 'ukbb_fcn.h')).read()
    return int(re.search(r'#define UKBB_INFLATE_CRC_CHUNK (\d+)', hdr).group(1))


def inflate_batch(streams):
    """streams: [(raw, dst_cap)] -> (written int64[n], crc uint32[n], [output region bytes]); asserts that no byte outside the
    regions changed.  Stream and region offsets are deliberately of every alignment."""
    import torch
    from ukbb_cardiac_amd import _lib
    n = len(streams)
    tab = (_lib.GzStream * n)()
    so, do = 0, GUARD
    for i, (raw, cap) in enumerate(streams):
        tab[i].src_off, tab[i].src_len, tab[i].dst_off, tab[i].dst_cap = so, len(raw), do, cap
        so += len(raw) + (i % 7)
        do += cap + GUARD + (i % 5)
    src = np.zeros(so + 16, np.uint8)
    for i, (raw, _) in enumerate(streams):
        src[tab[i].src_off:tab[i].src_off + len(raw)] = np.frombuffer(raw, np.uint8)
    d_src = torch.from_numpy(src).cuda()
    d_dst = torch.full((do,), 0xA5, dtype=torch.uint8, device='cuda')
    d_w = torch.zeros(n, dtype=torch.int64, device='cuda')
    d_c = torch.zeros(n, dtype=torch.int32, device='cuda')
    _lib.check(_lib.lib.ukbb_fcn_inflate_device(d_src.data_ptr(), d_dst.data_ptr(), tab, n, d_w.data_ptr(), d_c.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream), 'ukbb_fcn_inflate_device')
    torch.cuda.synchronize()
    dst, w = d_dst.cpu().numpy(), d_w.cpu().numpy()
    outside = np.ones(len(dst), bool)
    regions = []
    for i, (_, cap) in enumerate(streams):
        o = int(tab[i].dst_off)
        outside[o:o + cap] = False
        regions.append(dst[o:o + cap])
    assert (dst[outside] == 0xA5).all(), 'a byte outside the output regions changed'
    return w, d_c.cpu().numpy().view(np.uint32), regions


def check_good(streams_with_content, w, crc, regions, which=None):
    for i, (raw, cap, content) in enumerate(streams_with_content):
        if which is not None and i not in which:
            continue
        assert w[i] == len(content), (i, w[i], len(content))
        assert regions[i][:len(content)].tobytes() == content, i
        assert (regions[i][len(content):] == 0xA5).all(), i       # room beyond the content stays untouched
        assert crc[i] == zlib.crc32(content), i


def test_one_stream():
    name, raw, content = corpus()[1]
    w, crc, regions = inflate_batch([(raw, len(content))])
    check_good([(raw, len(content), content)], w, crc, regions)


def test_five_streams_of_very_different_length():
    rng = np.random.default_rng(9)
    text = bytes(rng.integers(97, 110, 400 * 1024, dtype=np.uint8))
    items = [(deflate(text[:k]), k + (3 if k == 100 else 0), text[:k]) for k in (0, 1, 100, 70 * 1024, 400 * 1024)]
    w, crc, regions = inflate_batch([(raw, cap) for raw, cap, _ in items])
    check_good(items, w, crc, regions)


def test_more_streams_than_the_grid():
    """More streams than the launch has workgroups (the grid is capped at 2 per CU), so every workgroup decodes a second and a
    third stream over the LDS the one before left behind -- among them malformed streams (the fixed list) in front of good ones:
    stream i and stream i + grid run in the same workgroup."""
    import torch
    grid = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    n = 2 * grid + 76
    rng = np.random.default_rng(10)
    bad = malformed()
    items, kinds = [], []
    for i in range(n):
        if i < grid and i % 9 == 4:                             # workgroup i: a refused stream first, good ones behind it
            _, raw, cap, want = bad[(i // 9) % len(bad)]
            items.append((raw, cap, None)); kinds.append(want)
        elif grid <= i < 2 * grid and i % 9 == 6:               # ... or between two good ones
            _, raw, cap, want = bad[(i // 9 + 5) % len(bad)]
            items.append((raw, cap, None)); kinds.append(want)
        else:
            content = bytes(rng.integers(0, 4 + i % 60, 1900 + i % 300, dtype=np.uint8))
            items.append((deflate(content, 1 + i % 9, zlib.Z_FIXED if i % 11 == 3 else zlib.Z_DEFAULT_STRATEGY), len(content), content))
            kinds.append(None)
    assert n > grid and sum(k is not None for k in kinds) > 2 * len(bad)
    assert any(kinds[i] is not None and kinds[i + grid] is None for i in range(grid))
    w, crc, regions = inflate_batch([(raw, cap) for raw, cap, _ in items])
    for i, want in enumerate(kinds):
        if want is not None:
            assert w[i] == want and crc[i] == 0, (i, w[i], want)
    check_good(items, w, crc, regions, which={i for i, k in enumerate(kinds) if k is None})


def test_whole_corpus_as_one_batch():
    items = [(raw, len(content) + (i % 3), content) for i, (_, raw, content) in enumerate(corpus())]
    w, crc, regions = inflate_batch([(raw, cap) for raw, cap, _ in items])
    check_good(items, w, crc, regions)


def test_malformed_streams_among_good_ones():
    """The fixed list the host-compiled core has passed under the sanitizers, nothing else."""
    good = [(raw, len(content), content) for _, raw, content in corpus()[:8]]
    bad = malformed()
    assert sorted({c for _, _, _, c in bad}) == [E_OUTPUT, E_DATA, E_INPUT]
    items, kinds = [], []
    for i, (name, raw, cap, want) in enumerate(bad):
        items.append(good[i % len(good)]); kinds.append(None)
        items.append((raw, cap, None)); kinds.append(want)
    items.append(good[-1]); kinds.append(None)
    w, crc, regions = inflate_batch([(raw, cap) for raw, cap, _ in items])
    for i, want in enumerate(kinds):
        if want is not None:
            assert w[i] == want, (bad[i // 2][0], w[i], want)
            assert crc[i] == 0
    check_good(items, w, crc, regions, which={i for i, k in enumerate(kinds) if k is None})


def test_crc_kernel_around_its_chunk():
    chunk = crc_chunk()
    rng = np.random.default_rng(12)
    data = bytes(rng.integers(0, 256, 3 * chunk + 17, dtype=np.uint8))
    items = [(deflate(data[:k], 0), k, data[:k]) for k in (0, 1, chunk - 1, chunk, chunk + 1, 3 * chunk + 17)]
    w, crc, regions = inflate_batch([(raw, cap) for raw, cap, _ in items])
    check_good(items, w, crc, regions)


def _engine():
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.engine import Engine
    from ukbb_cardiac_amd.weights import synthetic_params
    arch = MODELS['FCN_sa']
    return Engine(arch, synthetic_params(arch, 1234))


def _cine(shape, dtype, seed):
    from ukbb_cardiac_amd.phantom import cine_phantom
    X, Y, Z, T = shape
    v = cine_phantom(Z * T, X, Y, seed=seed)[..., 0].reshape(T, Z, X, Y).transpose(2, 3, 1, 0) * 2500.0 - 150.0
    return np.asfortranarray(np.round(v).astype(dtype))


@pytest.mark.parametrize('dtype', [np.float32, np.int16])
def test_segment_sequence_tensor_equals_segment_sequence_device(dtype, tmp_path):
    """The volume inflated on the device (DeviceInflater) through segment_sequence_tensor against the same host array through
    segment_sequence_device: labels, counts and clip bounds."""
    from ukbb_cardiac_amd import device_pipeline as dp, nifti
    from ukbb_cardiac_amd.device_inflate import DeviceInflater, Inflated
    vol = _cine((162, 204, 2, 3), dtype, 31)
    p = str(tmp_path / 'sa.nii.gz')
    nifti.save(vol, p, np.diag([1.8, 1.8, 10.0, 1.0]))
    eng = _engine()
    try:
        got, = DeviceInflater(eng, 4).inflate([open(p, 'rb').read()])
        assert isinstance(got, Inflated), got
        assert got.volume.data_ptr() % 16 == 0
        assert np.array_equal(got.volume.cpu().numpy(), vol)
        a, aux_a = dp.segment_sequence_tensor(got.volume, got.plan.dtype, got.plan.shape, eng, 4, return_aux=True)
        b, aux_b = dp.segment_sequence_device(vol, eng, 4, return_aux=True)
    finally:
        eng.close()
    assert np.array_equal(a, b) and a.dtype == b.dtype and a.shape == b.shape
    assert np.array_equal(aux_a['counts'], aux_b['counts']) and aux_a['clip'] == aux_b['clip']
    with pytest.raises(TypeError):
        dp.segment_sequence_tensor(got.volume, np.float64, got.plan.shape, None)


def test_no_room_is_asked_again_in_a_further_launch(tmp_path):
    """What does not fit max_bytes comes back as Declined(NO_ROOM), it and everything behind it, and inflates in the next call."""
    from ukbb_cardiac_amd import nifti
    from ukbb_cardiac_amd.device_inflate import NO_ROOM, Declined, DeviceInflater, Inflated
    vols, blobs = [], []
    for i in range(3):
        vols.append(_cine((40, 30, 2, 3), np.int16, 70 + i))
        p = str(tmp_path / ('v%d.nii.gz' % i))
        nifti.save(vols[i], p, np.eye(4))
        blobs.append(open(p, 'rb').read())
    one = 352 + vols[0].nbytes
    eng = _engine()
    try:
        inf = DeviceInflater(eng, 8, max_bytes=2 * one + 40)
        a = inf.inflate(blobs)
        assert [type(r) for r in a] == [Inflated, Inflated, Declined] and a[2].reason == NO_ROOM
        assert np.array_equal(a[1].volume.cpu().numpy(), vols[1])
        b, = inf.inflate(blobs[2:])
        assert isinstance(b, Inflated) and np.array_equal(b.volume.cpu().numpy(), vols[2])
        assert DeviceInflater(eng, 1).inflate(blobs[:2])[1] == Declined(NO_ROOM)
    finally:
        eng.close()


FILES = ('seg_sa.nii.gz', 'sa_ED.nii.gz', 'sa_ES.nii.gz', 'seg_sa_ED.nii.gz', 'seg_sa_ES.nii.gz')


@pytest.fixture(scope='module')
def cohort(tmp_path_factory):
    """5 subjects of 100 x 90 x 3 x 4: three int16, one float32, one int16 with scl_slope = 2 (declined: it takes the host reader)"""
    from ukbb_cardiac_amd import nifti
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.weights import save_blob, synthetic_params
    root = tmp_path_factory.mktemp('inflate_cohort')
    arch = MODELS['FCN_sa']
    model = str(root / 'FCN_sa')
    save_blob(model + '.ukbbw', arch, synthetic_params(arch, 1234))
    src = root / 'src'
    for i, dt in enumerate([np.int16, np.int16, np.float32, np.int16, np.int16]):
        d = src / ('s%d' % i)
        d.mkdir(parents=True)
        nifti.save(_cine((100, 90, 3, 4), dt, 60 + i), str(d / 'sa.nii.gz'), np.diag([1.8, 1.8, 10.0, 1.0]), pixdim=[1, 1.8, 1.8, 10, 0.03, 0, 0, 0])
    p = str(src / 's4' / 'sa.nii.gz')
    raw = bytearray(gzip.open(p).read())
    raw[112:116] = struct.pack('<f', 2.0)                        # scl_slope
    open(p, 'wb').write(gzip.compress(bytes(raw), 1, mtime=0))
    assert nifti.load(p).get_data().dtype == np.float64
    return root, model, src


def _run(root, model, src, name, extra, with_csv=True):
    from ukbb_cardiac_amd import deploy_network
    work = root / name
    shutil.copytree(str(src), str(work))
    csv = str(root / (name + '.csv'))
    deploy_network.main(['--seq_name', 'sa', '--data_dir', str(work), '--model_path', model, '--io_threads', '2'] +
                        (['--output_csv', csv] if with_csv else []) + extra)
    return work, csv


def test_deploy_with_device_inflate_writes_the_same_files(cohort, monkeypatch):
    from ukbb_cardiac_amd import device_inflate
    root, model, src = cohort
    declined = []
    real = device_inflate.DeviceInflater.inflate

    def spy(self, blobs):
        out = real(self, blobs)
        declined.extend(type(o).__name__ for o in out)
        return out
    monkeypatch.setattr(device_inflate.DeviceInflater, 'inflate', spy)
    runs = {}
    for name, extra in (('k1', ['--device_inflate', '1']), ('k4', ['--device_inflate', '4']), ('off', [])):
        declined.clear()
        work, csv = _run(root, model, src, name, extra)
        runs[name] = ({(s, f): open(str(work / s / f), 'rb').read() for s in sorted(os.listdir(str(src))) for f in FILES}, open(csv).read())
        if extra:
            assert sorted(declined) == ['Declined'] + ['Inflated'] * 4, declined
        else:
            assert not declined
    for name in ('k1', 'k4'):
        assert runs[name][0].keys() == runs['off'][0].keys() and len(runs[name][0]) == 25
        for key in runs['off'][0]:
            assert runs[name][0][key] == runs['off'][0][key], (name, key)
        assert runs[name][1] == runs['off'][1] and runs[name][1].count('\n') >= 5


FOUR_MODES = {'host': ['--io_threads', '0', '--nodevice_preproc'], 'sequential': ['--io_threads', '0'], 'pipelined': ['--io_threads', '2'],
              'rounds': ['--io_threads', '2', '--device_inflate', '2']}


def test_four_loops_write_the_same_files_tables_and_log_blocks(cohort):
    """The cohort plus a directory without a cine and a subject an earlier run segmented, through deploy_network.run on the host
    path, the sequential device path, the pipelined loop and the inflate rounds: 25 files and both tables byte for byte, and per
    subject the same block of log lines (time figures masked) -- the declined subject's with its Reading line in every mode."""
    from ukbb_cardiac_amd import deploy_network, nifti
    root, model, src = cohort
    full = root / 'src_four'
    shutil.copytree(str(src), str(full))
    (full / 'n_nocine').mkdir()
    (full / 'e_earlier').mkdir()
    shutil.copyfile(str(src / 's0' / 'sa.nii.gz'), str(full / 'e_earlier' / 'sa.nii.gz'))
    earlier = np.zeros((100, 90, 3, 4))
    earlier[30:60, 30:60] = 2
    earlier[38:52, 38:52] = 1
    earlier[20:28, 40:60] = 3
    nifti.save(earlier, str(full / 'e_earlier' / 'seg_sa.nii.gz'), np.diag([1.8, 1.8, 10.0, 1.0]), pixdim=[1, 1.8, 1.8, 10, 0.03, 0, 0, 0])
    names = sorted(os.listdir(str(full)))
    eng = _engine()
    forward = lambda b: {'pred': eng.run(b, want_prob=False)['pred']}
    seen = {}
    try:
        for mode, extra in FOUR_MODES.items():
            work = root / ('four_' + mode)
            shutil.copytree(str(full), str(work))
            lines = []

            def log(*a):
                line = ' '.join(str(x) for x in a).replace(str(work), 'DIR')
                lines.append(re.sub(r'\d+\.\d+s', '#s', line) if ('time =' in line or 'it took' in line) else line)
            FLAGS, _ = deploy_network.define_flags().parse(['--seq_name', 'sa', '--data_dir', str(work), '--model_path', model, '--output_csv',
                                                            str(work) + '.csv', '--qc_csv', str(work) + '.qc.csv'] + extra)
            processed = deploy_network.run(FLAGS, forward, log=log, engine=eng)
            assert sorted(processed) == ['s0', 's1', 's2', 's3', 's4'], mode
            tail = next(i for i, l in enumerate(lines) if l.startswith('Clinical measures of'))
            blocks = {}
            for line in lines[:tail]:
                if line in names:
                    assert line not in blocks, (mode, line)
                    blocks[line] = current = []
                current.append(line)
            files = {(s, f): open(str(work / s / f), 'rb').read() for s in names if s != 'n_nocine' for f in FILES if s != 'e_earlier' or f == FILES[0]}
            # a failing gate's message names the subject's file
            seen[mode] = (files, open(str(work) + '.csv').read(), open(str(work) + '.qc.csv').read().replace(str(work), 'DIR'), blocks, lines[tail:])
    finally:
        eng.close()
    files, csv, qc, blocks, tail = seen['host']
    assert len(files) == 25 + 1 and csv.count('\n') == 7 and qc.count('\n') == 7
    assert set(blocks) == set(names) and blocks['e_earlier'] == ['e_earlier'] and len(blocks['n_nocine']) == 2
    assert blocks['s0'][:4] == ['s0', '  Reading DIR/s0/sa.nii.gz ...', '  Segmenting full sequence ...', '  Segmentation time = #s']
    assert blocks['s0'][4].startswith('  ED frame = 0, ES frame = ') and blocks['s0'][-1] == '  Saving segmentation ...'
    for mode in FOUR_MODES:
        m_files, m_csv, m_qc, m_blocks, m_tail = seen[mode]
        assert m_files.keys() == files.keys()
        for key in files:
            assert m_files[key] == files[key], (mode, key)
        assert m_csv == csv and m_qc == qc, mode
        assert m_blocks.keys() == blocks.keys(), mode
        for name in blocks:
            assert m_blocks[name] == blocks[name], (mode, name, m_blocks[name], blocks[name])
        assert '  Reading DIR/s4/sa.nii.gz ...' in m_blocks['s4'], mode
        assert m_tail == tail, mode


def test_deploy_flag_needs_device_preproc(cohort):
    root, model, src = cohort
    with pytest.raises(ValueError, match='device_inflate'):
        _run(root, model, src, 'noprep', ['--device_inflate', '2', '--nodevice_preproc'], with_csv=False)


def test_damaged_file_is_left_to_the_existing_reader(cohort):
    """A sixth subject whose CRC-32 trailer is wrong: the device path declines it, nifti.load decides -- as without the flag --
    and the other five subjects are complete."""
    root, model, src = cohort
    bad_src = root / 'src_bad'
    shutil.copytree(str(src), str(bad_src))
    (bad_src / 'zz').mkdir()
    blob = bytearray(open(str(src / 's0' / 'sa.nii.gz'), 'rb').read())
    blob[-8] ^= 0x55
    open(str(bad_src / 'zz' / 'sa.nii.gz'), 'wb').write(bytes(blob))
    raised = {}
    for name, extra in (('bad_off', []), ('bad_k4', ['--device_inflate', '4'])):
        with pytest.raises(Exception) as e:
            _run(root, model, bad_src, name, extra)
        raised[name] = e.type
    assert raised['bad_k4'] is raised['bad_off']
    for s in ('s0', 's1', 's2', 's3', 's4'):
        for f in FILES:
            assert os.path.exists(str(root / 'bad_k4' / s / f)), (s, f)
    assert not os.path.exists(str(root / 'bad_k4' / 'zz' / 'seg_sa.nii.gz'))
