"""What deploy_network_ao.py writes and logs on the host path, pinned byte for byte: six command lines (five in sequence mode with
--output_csv, one in ED/ES mode) over a tiny cohort of 40 x 36 x 1 x 6 cines with stub networks that return prepared discs.  Every
CSV, the full list of log lines (time figures masked, the data directory replaced by DIR) and the inflated bytes of every
segmentation written are compared with the record under tests/golden/aortic_table/, and --io_threads 0 and 2 must give the same
record.  The record was made on the commit before the aortic table moved into label_tables.py;
``PYTHONPATH=. python tests/test_aortic_table.py`` rewrites it."""
import hashlib
import os
import pathlib
import sys

import numpy as np

from ukbb_cardiac_amd import deploy_network_ao as DA, nifti

import test_host_pipeline as TH
from test_label_tables import masked

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'aortic_table')
SHAPE = (40, 36, 1, 6)
# one directory listing: a passing subject, one per quality-control criterion 1 / 3 / 2, one the pressure spreadsheet does not
# hold, a directory without a cine, a stray file
SUBJECTS = ['5001', '5002_dao_lost', '5003_dao_two_pieces', '5004_noisy_frame', '5005']
NO_IMAGE, STRAY = '5006_no_image', 'notes.txt'
PRESSURE = ('eid,Central pulse pressure during PWA,Central pulse pressure during PWA\n,12678-2.0,12678-2.1\n'
            '5001,40,44\n5002_dao_lost,30,30\n5003_dao_two_pieces,,38\n5004_noisy_frame,41,43\n')
LOST = 'The area of DAo is 0 at time frame 2.'
PIECES = 'The segmentation has at least two connected components with more than 10 pixels at time frame 2.'
NOISY = 'The image becomes very noisy at time frame 3.'

CSV = ['--output_csv', 'ao.csv']
INVOCATIONS = {
    'unet': ['--model', 'UNet'] + CSV + ['--pressure_csv', 'pp.csv'],
    'unet_full': ['--model', 'UNet'] + CSV + ['--pressure_csv', 'pp.csv', '--aortic_qc_full'],
    'unet_noqc': ['--model', 'UNet'] + CSV + ['--pressure_csv', 'pp.csv', '--aortic_qc_full', '--noaortic_qc'],
    'unet_rescale_full': ['--model', 'UNet'] + CSV + ['--aortic_qc_full', '--noz_score'],
    'lstm_step2': ['--model', 'UNet-LSTM'] + CSV + ['--time_step', '2'],
    'ed_es': ['--model', 'UNet', '--noprocess_seq'],
}


def write_cohort(root):
    """Cines of steady intensity (a gamma volume as test_host_pipeline.make_volume's would fail criterion 2 in every frame), frame 3
    of one subject scaled x10; ED / ES frames for the first two subjects only."""
    root = pathlib.Path(root)
    root.mkdir()
    rng = np.random.default_rng(31)
    for i, name in enumerate(SUBJECTS):
        d, affine, pixdim = TH._write_subject(root, name, 'ao', SHAPE, 40 + i)
        cine = rng.uniform(100, 120, size=SHAPE).astype(np.float32)
        if name == '5004_noisy_frame':
            cine[..., 3] *= 10.0
        nifti.save(cine, str(d / 'ao.nii.gz'), affine, pixdim)
        if i < 2:
            for fr, t in (('ED', 0), ('ES', 3)):
                nifti.save(cine[..., t], str(d / ('ao_%s.nii.gz' % fr)), affine, pixdim)
    (root / NO_IMAGE).mkdir()
    (root / STRAY).write_text('not a subject directory')


def stubs(state):
    """The frame-wise and the windowed stand-in networks: steady centred discs (the 40 x 36 cine sits centred in the 256 x 256 pad,
    48 x 48 in ED/ES mode); frame 2 of one subject without its DAo, frame 2 of another with a separate 16-voxel piece of DAo."""
    def labels(shape, first):
        n = shape[0]
        pred = np.zeros(shape, np.int32)
        cy, cx = shape[1] // 2, shape[2] // 2
        pred[:, cy - 16:cy - 6, cx - 14:cx - 4] = 1
        pred[:, cy + 2:cy + 12, cx + 2:cx + 10] = 2
        for k in range(n):
            if first + k == 2 and state['subject'] == '5002_dao_lost':
                pred[k][pred[k] == 2] = 0
            if first + k == 2 and state['subject'] == '5003_dao_two_pieces':
                pred[k, cy + 14:cy + 18, cx - 14:cx - 10] = 2
        return pred

    def one_hot(pred):
        prob = np.zeros(pred.shape + (3,), np.float32)
        np.put_along_axis(prob, pred[..., None], 1.0, axis=-1)
        return prob

    def forward(batch):
        pred = labels(batch.shape[:3], state['frame'])
        state['frame'] += batch.shape[0]
        return {'prob': one_hot(pred), 'pred': pred}

    def cine_forward(frames, weight_R, weight_r, time_step=1):
        assert frames.shape == (SHAPE[3], 256, 256)
        state['windowed'].append((weight_R, weight_r, time_step))
        return one_hot(labels(frames.shape, 0))
    return forward, cine_forward


def observe(name, io_threads):
    """file name under GOLDEN -> text, of one invocation in the current directory."""
    data_dir = 'data_%s_%d' % (name, io_threads)
    write_cohort(data_dir)
    with open('pp.csv', 'w') as f:
        f.write(PRESSURE)
    state = {'subject': None, 'frame': 0, 'windowed': []}
    lines = []

    def log(*a):                                                   # the script prints the subject's name before it works on it
        line = ' '.join(str(x) for x in a)
        lines.append(masked(line).replace(data_dir, 'DIR'))
        if line in SUBJECTS:
            state['subject'], state['frame'] = line, 0
    forward, cine_forward = stubs(state)
    argv = INVOCATIONS[name] + ['--data_dir', data_dir, '--model_path', 'x', '--io_threads', str(io_threads), '--batch_slices', '4']
    FLAGS, _ = DA.define_flags().parse(argv)
    if os.path.exists('ao.csv'):
        os.remove('ao.csv')
    processed = DA.run(FLAGS, forward, log=log, cine_forward=cine_forward)
    assert processed == (SUBJECTS[:2] if name == 'ed_es' else SUBJECTS)
    assert state['windowed'] == ([(5, 0.1, 2)] * len(SUBJECTS) if name == 'lstm_step2' else [])
    got = {name + '.log': ''.join(l + '\n' for l in lines)}
    if name != 'ed_es':
        got[name + '.csv'] = open('ao.csv', newline='').read()
    segs = []
    for p in sorted(pathlib.Path(data_dir).rglob('seg_*.nii.gz')):
        nim = nifti.load(str(p))
        data = np.asarray(nim.get_data())
        digest = hashlib.sha256(np.asfortranarray(data).tobytes(order='F') + np.asarray(nim.header['pixdim']).tobytes()
                                + np.asarray(nim.affine, np.float64).tobytes()).hexdigest()
        segs.append('%s %s %s %s\n' % (p.relative_to(data_dir).as_posix(), data.dtype, data.shape, digest))
    got[name + '.segs'] = ''.join(segs)
    return got


def test_tables_log_lines_and_segmentations_are_the_recorded_ones(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    seen = set()
    for name in INVOCATIONS:
        sequential, threaded = observe(name, 0), observe(name, 2)
        assert sequential == threaded, name
        for fname, text in sequential.items():
            with open(os.path.join(GOLDEN, fname), newline='') as f:
                assert text == f.read(), fname
            seen.add(fname)
    assert seen == set(os.listdir(GOLDEN)) and len(seen) == 3 * len(INVOCATIONS) - 1

    # the record is not vacuous
    def golden(fname):
        return open(os.path.join(GOLDEN, fname)).read().splitlines()
    counts = {n: [golden(n + '.log').count(m) for m in (LOST, PIECES, NOISY)] for n in INVOCATIONS}
    assert counts == {'unet': [1, 0, 0], 'unet_full': [1, 1, 1], 'unet_noqc': [0, 0, 0], 'unet_rescale_full': [1, 1, 1],
                      'lstm_step2': [1, 0, 0], 'ed_es': [0, 0, 0]}
    warning = '  Warning: subject 5005 is not in the pressure spreadsheet: distensibility left empty.'
    for n in INVOCATIONS:
        warned = [l for l in golden(n + '.log') if 'pressure spreadsheet' in l]
        assert warned == ([warning] if n in ('unet', 'unet_full', 'unet_noqc') else []), n
    passing = ['5001', '5005']
    table = golden('unet.csv')
    assert [r.split(',')[0] for r in table[1:]] == ['5001', '5003_dao_two_pieces', '5004_noisy_frame', '5005']
    assert golden('unet_full.csv') == [table[0]] + [r for r in table[1:] if r.split(',')[0] in passing]
    assert [r.split(',')[0] for r in golden('unet_noqc.csv')[1:]] == SUBJECTS
    assert [r.split(',')[0] for r in golden('unet_rescale_full.csv')[1:]] == passing
    assert table[1].split(',')[3] != '' and table[4].split(',')[3] == ''          # distensibility needs the pulse pressure
    for n in INVOCATIONS:
        log = golden(n + '.log')
        assert log.count(STRAY) == 1 and sum('does not contain an image' in l and NO_IMAGE in l for l in log) == 1
        assert len(golden(n + '.segs')) == (4 if n == 'ed_es' else len(SUBJECTS))
    assert golden('ed_es.log')[-1].startswith('Including image I/O') and not any('written to' in l for l in golden('ed_es.log'))
    assert golden('unet.log')[-2] == 'Aortic areas of 4 subjects written to ao.csv'


if __name__ == '__main__':
    import tempfile
    os.makedirs(GOLDEN, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        for name in INVOCATIONS:
            for fname, text in observe(name, 0).items():
                with open(os.path.join(GOLDEN, fname), 'w', newline='') as f:
                    f.write(text)
    sys.exit(0)
