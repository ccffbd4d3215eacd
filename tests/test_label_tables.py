"""What deploy_network.py --output_csv / --qc_csv / --atrial_csv write and log on the host path, pinned byte for byte: three command
lines over a tiny cohort (32 x 48 frames, a stub network that returns prepared labels), each run twice -- the second run finds every
subject segmented and fills every table from the files.  Every CSV and the full list of log lines are compared with the record under
tests/golden/label_tables/ (time figures masked).  The record was made on the commit before
the tables moved into label_tables.py; ``PYTHONPATH=. python tests/test_label_tables.py`` rewrites it."""
import os
import re
import sys

import numpy as np

from ukbb_cardiac_amd import deploy_network, nifti

import test_atrial as TA
import test_qc_gates as TQ

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'label_tables')
T_LA = 4


def la_labels(seq, bad=None):
    """(32, 48, 1, T_LA) labels of a beating left atrium (and a right one for la_4ch).  bad: 'empty' -- no LA in frame 1; 'abrupt' --
    frame 2 a third of the area."""
    seg = np.zeros((32, 48, 1, T_LA), np.int32)
    for t in range(T_LA):
        s = 1.0 + 0.08 * np.sin(2 * np.pi * t / T_LA)
        f = np.where(TA.ellipse(32, 48, 10.3, 14.2, 6.1 * s, 4.2 * s, 0.5), 1, 0)
        if seq == 'la_4ch':
            f = np.where(TA.ellipse(32, 48, 21.4, 33.6, 5.3 * s, 4.9 * s, 2.0), 2, f)
        seg[:, :, 0, t] = f
    if bad == 'empty':
        seg[:, :, 0, 1][seg[:, :, 0, 1] == 1] = 0
    if bad == 'abrupt':
        seg[:, :, 0, 2] = np.where(TA.ellipse(32, 48, 10.3, 14.2, 3.4, 2.3, 0.5), 1, np.where(seg[:, :, 0, 2] == 2, 2, 0))
    return seg


def cohort(seq):
    """name -> (labels, segmented by an earlier run?, has sa.nii.gz?): subjects to segment (one of them failing its gate), subjects of
    an earlier run, subjects without sa.nii.gz.  s0 fails its gate and is gated from its file only after the atrial table has been
    filled: its message comes after those of s2 and s3."""
    if seq == 'sa':
        c = TQ.cli_subjects('sa', False)
        return {'1001': (c['1001'], False, True), '1002': (c['1002'], False, True), '1003': (c['1003'], True, True),
                '1004': (None, False, False)}
    return {'s1_good': (la_labels(seq), False, True), 's2_area_zero': (la_labels(seq, 'empty'), False, True),
            's3_earlier_abrupt': (la_labels(seq, 'abrupt'), True, True), 's4_no_sa': (la_labels(seq), False, False),
            's0_earlier_no_sa': (la_labels(seq, 'empty'), True, False)}


def write_cohort(seq, root):
    rng = np.random.default_rng(9)
    sa_pixdim = np.array([1, 1.8, 1.8, 10, 0.03, 0, 0, 0], np.float32)
    for i, (name, (lab, earlier, has_sa)) in enumerate(sorted(cohort(seq).items())):
        d = os.path.join(root, name)
        os.makedirs(d)
        affine, sa_affine = TA.AFFINES[i % 3]
        if seq == 'sa':
            affine, pixdim = sa_affine, sa_pixdim
        else:
            pixdim = TA.PIXDIM
            if has_sa:
                nifti.save(np.zeros((4, 4, 2, 1), np.float32), os.path.join(d, 'sa.nii.gz'), sa_affine, sa_pixdim)
        if lab is None:
            continue
        nifti.save(rng.uniform(10, 200, size=lab.shape).astype(np.float32), os.path.join(d, seq + '.nii.gz'), affine, pixdim)
        if earlier:
            nifti.save(lab, os.path.join(d, 'seg_%s.nii.gz' % seq), affine, pixdim, as_dtype=np.float64)


def masked(line):
    return re.sub(r'\d+\.\d+s', '#s', line) if ('time =' in line or 'it took' in line) else line


INVOCATIONS = {'sa': ('sa', ('output_csv', 'qc_csv')), 'la_2ch': ('la_2ch', ('qc_csv', 'atrial_csv')), 'la_4ch': ('la_4ch', ('atrial_csv',))}


def observe(name):
    """file name under GOLDEN -> text, of the two runs of one invocation in the current directory."""
    seq, tables = INVOCATIONS[name]
    subjects = cohort(seq)
    write_cohort(seq, 'data_' + name)
    state = {'subject': None}
    got = {}
    for run in (1, 2):
        lines = []

        def log(*a):
            line = ' '.join(str(x) for x in a)
            lines.append(masked(line))
            if line in subjects:
                state['subject'] = line

        def forward(batch):                                                    # the whole sequence in one call: [T*Z][32][48]
            lab = subjects[state['subject']][0]
            pred = np.ascontiguousarray(lab.transpose(3, 2, 0, 1).reshape((-1,) + lab.shape[:2]))
            assert pred.shape == batch.shape[:3]
            return {'pred': pred}
        argv = ['--seq_name', seq, '--data_dir', 'data_' + name, '--model_path', 'x', '--io_threads', '0', '--batch_slices', '1000']
        for t in tables:
            argv += ['--' + t, '%s_run%d_%s' % (name, run, t)]
        FLAGS, _ = deploy_network.define_flags().parse(argv)
        processed = deploy_network.run(FLAGS, forward, log=log)
        assert len(processed) == (sum(1 for lab, earlier, _ in subjects.values() if lab is not None and not earlier) if run == 1 else 0)
        got['%s_run%d.log' % (name, run)] = ''.join(l + '\n' for l in lines)
        for t in tables:
            got['%s_run%d_%s' % (name, run, t)] = open('%s_run%d_%s' % (name, run, t), newline='').read()
    return got


def test_tables_and_log_lines_are_the_recorded_ones(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    seen = set()
    for name in INVOCATIONS:
        for fname, text in observe(name).items():
            with open(os.path.join(GOLDEN, fname), newline='') as f:
                assert text == f.read(), fname
            seen.add(fname)
    assert seen == set(os.listdir(GOLDEN)) and len(seen) == 16
    # the record is not vacuous: a failing gate is logged when the subject is segmented and again when its file is gated, the atrial
    # rows of the back-filled subject carry the verdict, the subject without sa.nii.gz has a verdict and no atrial rows
    log1, log2 = (open(os.path.join(GOLDEN, 'la_2ch_run%d.log' % r)).read().splitlines() for r in (1, 2))
    assert log1.count('The area of LA is 0 at time frame 1.') == 2 and log1.count('There is abrupt change of area at time frame 2.') == 1
    assert log2[5:9] == ['The area of LA is 0 at time frame 1.', 'There is abrupt change of area at time frame 2.',
                         'Atrial measures of 12 frames and labels written to la_2ch_run2_atrial_csv', 'The area of LA is 0 at time frame 1.']
    assert not any('Segmenting' in l for l in log2)
    for r in (1, 2):
        atrial = open(os.path.join(GOLDEN, 'la_2ch_run%d_atrial_csv' % r)).read().splitlines()
        assert sum(l.startswith('s3_earlier_abrupt,') and l.endswith(',False') for l in atrial) == T_LA
        assert not any(l.startswith(('s4_no_sa', 's0_earlier_no_sa')) for l in atrial)
        qc = open(os.path.join(GOLDEN, 'la_2ch_run%d_qc_csv' % r)).read().splitlines()
        assert len(qc) == 6 and qc[1].startswith('s0_earlier_no_sa,') and qc[5].startswith('s4_no_sa,')
    assert open(os.path.join(GOLDEN, 'sa_run1_output_csv')).read() == open(os.path.join(GOLDEN, 'sa_run2_output_csv')).read()


if __name__ == '__main__':
    import tempfile
    os.makedirs(GOLDEN, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        for name in INVOCATIONS:
            for fname, text in observe(name).items():
                with open(os.path.join(GOLDEN, fname), 'w', newline='') as f:
                    f.write(text)
    sys.exit(0)
