"""sequence_run.SequenceRun without a GPU: the lazy walk over the subjects (what is yielded, logged and claimed, and when), and the
finisher fed the way the device loops feed it -- labels, counts, statistics, clip bounds and a getter of unclipped frames --
against deploy_network.run on the host path and the record under tests/golden/label_tables/."""
import os
import re
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from ukbb_cardiac_amd import deploy_network, measures, nifti, sequence_run
from ukbb_cardiac_amd.label_tables import LabelTables
from ukbb_cardiac_amd.sequence_run import SequenceRun

import test_label_tables as TL

FILES = ('{seq}_ED.nii.gz', '{seq}_ES.nii.gz', 'seg_{seq}_ED.nii.gz', 'seg_{seq}_ES.nii.gz', 'seg_{seq}.nii.gz')


class StandInQueue:
    """A ClaimQueue that records what is asked of it.  ``held``: subjects another worker holds for good; ``late``: held when first
    asked, free on the second pass."""

    def __init__(self, held, late, again):
        self.held, self.late, self.again = set(held), set(late), list(again)
        self.record = []
        self.lock = threading.Lock()

    def note(self, *what):
        with self.lock:
            self.record.append(what)

    def take(self, name):
        ok = name not in self.held and not (name in self.late and ('second_chance',) not in self.record)
        self.note('take', name, ok)
        return ok

    def done(self, name):
        self.note('done', name)

    def second_chance(self):
        self.note('second_chance')
        return list(self.again)

    def release_all(self):
        self.note('release_all')


SHAPE = (6, 5, 2, 3)


def walk_cohort(root):
    """A stray file, a directory without a cine, a subject segmented earlier, two open subjects, one that another worker holds and
    one that it held only when the walk first came by."""
    rng = np.random.default_rng(3)
    (root / 'a_file').write_text('stray')
    (root / 'b_nocine').mkdir()
    for name in ('c_done', 'd_open', 'e_held', 'f_open', 'g_late'):
        (root / name).mkdir()
        nifti.save(rng.uniform(0, 100, SHAPE).astype(np.float32), str(root / name / 'sa.nii.gz'), np.eye(4))
    nifti.save(np.zeros(SHAPE), str(root / 'c_done' / 'seg_sa.nii.gz'), np.eye(4))
    return sorted(os.listdir(str(root)))


def make_run(root, extra=()):
    FLAGS, _ = deploy_network.define_flags().parse(['--seq_name', 'sa', '--data_dir', str(root), '--io_threads', '0'] + list(extra))
    queue = StandInQueue(held=['e_held'], late=['g_late'], again=['b_nocine', 'c_done', 'g_late'])
    lines = []
    return SequenceRun(FLAGS, None, LabelTables(FLAGS), queue, lines.append, walk_cohort(root)), queue, lines


def item_of(root, name):
    return (name, os.path.join(str(root), name), os.path.join(str(root), name) + '/sa.nii.gz')


def test_walk_yields_logs_and_claims_lazily(tmp_path):
    run, queue, lines = make_run(tmp_path)
    walk = run.walk()
    assert queue.record == [] and lines == []                                   # nothing happens before the first item is asked for
    takes = lambda: [r[1:] for r in queue.record if r[0] == 'take']
    skipped = ['a_file', 'b_nocine',
               '  Directory {0} does not contain an image with file name sa.nii.gz. Skip.'.format(os.path.join(str(tmp_path), 'b_nocine')), 'c_done']
    assert next(walk) == item_of(tmp_path, 'd_open')
    assert takes() == [('d_open', True)] and lines == skipped
    assert next(walk) == item_of(tmp_path, 'f_open')
    assert takes() == [('d_open', True), ('e_held', False), ('f_open', True)] and ('second_chance',) not in queue.record
    assert next(walk) == item_of(tmp_path, 'g_late')                            # the second pass: skipped subjects are not logged again
    assert takes() == [('d_open', True), ('e_held', False), ('f_open', True), ('g_late', False), ('g_late', True)]
    assert queue.record.index(('second_chance',)) == queue.record.index(('take', 'g_late', False)) + 1
    assert next(walk, None) is None
    assert lines == skipped and len(takes()) == 5                               # a subject held elsewhere is not logged at all
    assert not any(r[0] in ('done', 'release_all') for r in queue.record)       # releasing is the finisher's and run()'s


@pytest.mark.parametrize('threads', [0, 2])
def test_claim_is_released_once_after_the_write_returned(tmp_path, monkeypatch, threads):
    run, queue, lines = make_run(tmp_path)
    real = sequence_run.save_sequence_outputs

    def save(data_dir, *a):
        real(data_dir, *a)
        queue.note('written', os.path.basename(data_dir))
    monkeypatch.setattr(sequence_run, 'save_sequence_outputs', save)

    def loop():
        if threads:
            run.writers = ThreadPoolExecutor(threads)
        for item in run.walk():
            nim = nifti.load(item[2])
            image = nim.get_data()
            run.finish(item, nim, 0.25, np.zeros(SHAPE, np.uint8), np.zeros((SHAPE[3], 4), np.int64), {}, None, lambda k: image[:, :, :, k])
    processed, table_time = run.run(loop)
    assert processed == ['d_open', 'f_open', 'g_late'] and table_time == [0.25] * 3
    for name in processed:
        assert [r for r in queue.record if r[0] == 'done'].count(('done', name)) == 1
        assert queue.record.index(('written', name)) < queue.record.index(('done', name))
        assert all(os.path.exists(os.path.join(str(tmp_path), name, f.format(seq='sa'))) for f in FILES)
    assert sum(r[0] == 'done' for r in queue.record) == 3 and queue.record[-1] == ('release_all',)
    assert lines[4:10] == ['d_open', '  Reading {0} ...'.format(item_of(tmp_path, 'd_open')[2]), '  Segmenting full sequence ...',
                           '  Segmentation time = 0.250000s', '  ED frame = 0, ES frame = 0', '  Saving segmentation ...']


def test_without_save_seg_the_claim_is_released_at_once(tmp_path):
    run, queue, lines = make_run(tmp_path, ['--nosave_seg'])

    def loop():
        for item in run.walk():
            run.finish(item, nifti.load(item[2]), 0.5, np.zeros(SHAPE, np.uint8), np.zeros((SHAPE[3], 4), np.int64), {}, None, None)
            assert queue.record[-1] == ('done', item[0])
    assert run.run(loop)[0] == ['d_open', 'f_open', 'g_late']
    assert not os.path.exists(os.path.join(str(tmp_path), 'd_open', 'seg_sa.nii.gz')) and '  Saving segmentation ...' not in lines


def test_release_all_when_the_consumer_raises(tmp_path):
    run, queue, lines = make_run(tmp_path)

    def loop():
        for item in run.walk():
            raise KeyError(item[0])
    with pytest.raises(KeyError, match='d_open'):
        run.run(loop)
    assert queue.record == [('take', 'd_open', True), ('release_all',)]


# ---- the finisher from a device-shaped source ----------------------------------------------------------------------------------
def overlapped_order(lines):
    """The host log with the line LabelTables.subject_args emits moved in front of its subject's name: the overlapped loops ask
    for a subject's arguments when they submit it, and log the subject when its result arrives."""
    out, name_at = [], 0
    for line in lines:
        if not line.startswith(' ') and ' ' not in line:
            name_at = len(out)
        if re.match(r'  Directory \S+ does not contain sa\.nii\.gz', line):
            out.insert(name_at, line)
        else:
            out.append(line)
    return out


def device_shaped(subjects, dtype, threads):
    """A loop for SequenceRun.run that hands the finisher what a device loop does: prepared labels as ``dtype``, the counts and
    statistics LabelTables.from_labels gives for them, the unclipped image with the percentiles the host path clips it to."""
    def loop(self, forward=None):
        if threads:
            self.writers = ThreadPoolExecutor(threads)
        for item in self.walk():
            nim = nifti.load(item[2])
            image = nim.get_data()
            lab = subjects[item[0]][0]
            args = self.tables.subject_args(item[1], nim, self.log)
            counts, stats = self.tables.from_labels(lab, args, self.tables.n_class)
            if counts is None:                                                  # a device loop always has them: the ES pick needs them
                counts = measures.counts_from_labels(lab, 4)
            clip = tuple(np.percentile(image, (1, 99)))                         # image_utils.rescale_intensity
            self.finish(item, nim, 0.125, np.asfortranarray(lab.astype(dtype)), counts, stats, clip, lambda k: image[:, :, :, k])
    return loop


@pytest.mark.parametrize('name', sorted(TL.INVOCATIONS))
def test_finisher_from_a_device_shaped_source_equals_the_host_run(name, tmp_path, monkeypatch):
    seq, tables = TL.INVOCATIONS[name]
    subjects = TL.cohort(seq)
    todo = sorted(n for n, (lab, earlier, _) in subjects.items() if lab is not None and not earlier)
    csvs = ['%s_run1_%s' % (name, t) for t in tables]

    def outputs(where, lines):
        got = {c: open(str(where / c), newline='').read() for c in csvs}
        got.update({(n, f): open(str(where / ('data_' + name) / n / f.format(seq=seq)), 'rb').read() for n in todo for f in FILES})
        return lines, got

    (tmp_path / 'host').mkdir()
    monkeypatch.chdir(tmp_path / 'host')
    observed = TL.observe(name)                                                 # deploy_network.run --io_threads 0 with the stub forward
    host_lines, host = outputs(tmp_path / 'host', observed['%s_run1.log' % name].splitlines())
    golden = lambda f: open(os.path.join(TL.GOLDEN, f), newline='').read()
    if name in ('sa', 'la_2ch'):
        assert host_lines == golden('%s_run1.log' % name).splitlines()
    for c in csvs:
        assert host[c] == golden(c)
    for dtype, threads in ((np.uint8, 2), (np.float64, 0)):
        where = tmp_path / np.dtype(dtype).name
        where.mkdir()
        monkeypatch.chdir(where)
        TL.write_cohort(seq, 'data_' + name)
        argv = ['--seq_name', seq, '--data_dir', 'data_' + name, '--model_path', 'x', '--io_threads', '0']
        for t in tables:
            argv += ['--' + t, '%s_run1_%s' % (name, t)]
        lines = []
        with monkeypatch.context() as m:
            m.setattr(SequenceRun, 'sequential', device_shaped(subjects, dtype, threads))
            processed = deploy_network.run(deploy_network.define_flags().parse(argv)[0], None, log=lambda *a: lines.append(TL.masked(' '.join(map(str, a)))))
        assert processed == todo
        lines, got = outputs(where, lines)
        assert lines == overlapped_order(host_lines)
        assert got.keys() == host.keys() and len(got) == len(csvs) + 5 * len(todo)
        for key in host:
            assert got[key] == host[key], (np.dtype(dtype).name, key)
    if 'atrial_csv' in tables:                                                  # the cohort does make subject_args speak: s4_no_sa has no long axis
        moved = overlapped_order(host_lines)
        assert 'does not contain sa.nii.gz' in moved[moved.index('s4_no_sa') - 1] and moved != host_lines
