"""Exactly once, at the level of the deploy loop: workers started by shard.launch share one cohort, run deploy_network.run with a
stub forward, and each appends the subjects it segmented to a file of its own.  Across the workers every subject appears once, the
merged tables are the single-worker tables byte for byte, and nothing of the claim protocol or of a writer stays behind -- with
label files saved (work stealing) and without (no label file, nothing marks a subject done: the static split).  No GPU."""
import os
import shutil

import numpy as np
import pytest

from ukbb_cardiac_amd import deploy_network as DN, deploy_network_ao as DA, measures, nifti, seg_score, shard
from ukbb_cardiac_amd.label_tables import LabelTables
from ukbb_cardiac_amd.sequence_run import SequenceRun

from test_host_pipeline import _write_subject, stub_forward

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = ('output_csv', 'qc_csv', 'score_csv', 'confidence_csv')          # the tables of the host path for --seq_name sa
FRAMES = (3, 6, 4, 3, 5, 3, 6, 4, 3)                                        # subject i: 20 x 28 x 2 x FRAMES[i]
NAMES = ['subj%02d' % i for i in range(len(FRAMES))]

# argv: data_dir, directory of this launch (ready files, logs), 'ok' | 'die', then flags of deploy_network.py
WORKER = '''
import os, sys, time
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, 'tests'))
from test_host_pipeline import stub_forward
from ukbb_cardiac_amd import deploy_network as DN
rank, world = int(os.environ['UKBB_SHARD_INDEX']), int(os.environ['UKBB_NUM_SHARDS'])
data, here, mode = sys.argv[1:4]
F, _ = DN.define_flags().parse(['--data_dir', data] + sys.argv[4:])
assert (F.num_shards, F.shard_index, F.work_stealing) == (world, rank, True)
one_subject = DN._sequence_subject
def logged(self, item, *args, **kwargs):                       # every subject that is segmented takes this path on the host
    out = one_subject(self, item, *args, **kwargs)
    with open(os.path.join(here, 'segmented%d' % rank), 'a') as f:
        f.write(item[0] + '\\n')
    return out
DN._sequence_subject = logged
open(os.path.join(here, 'segmented%d' % rank), 'a').close()
# all workers up before any takes a subject (as the dying worker of test_shard.py)
open(os.path.join(here, 'ready%d' % rank), 'w').close()
t0 = time.time()
while not all(os.path.exists(os.path.join(here, 'ready%d' % r)) for r in range(world)) and time.time() - t0 < 60:
    time.sleep(0.01)
calls = [0]
def forward(batch):
    calls[0] += 1
    if mode == 'die' and rank == 0 and calls[0] == 2:                  # one call per subject of these sizes
        os._exit(9)                                            # mid-subject (its second), no cleanup of any kind
    if rank == (1 if mode == 'die' else 0):
        time.sleep(0.05)                                       # the slow worker: the others are through their shares first
    return stub_forward(batch)
DN.run(F, forward, log=lambda *_: None)
'''


# the score table makes a worker import torch (device_pipeline, for the planes the device form holds): more than a second per
# process, so it rides along where two workers run and the launches of three keep to the other tables
NO_SCORE = tuple(t for t in TABLES if t != 'score_csv')


def table_flags(where, tables=TABLES):
    flags = ['--score_against', 'label_sa'] if 'score_csv' in tables else []
    for t in tables:
        flags += ['--' + t, os.path.join(str(where), t)]
    return flags


@pytest.fixture(scope='module')
def cohort(tmp_path_factory):
    """The cohort, written once, and the tables of one worker over a copy of it: (directory, {table: text}, worker script)."""
    root = tmp_path_factory.mktemp('cohort')
    data = root / 'data'
    data.mkdir()
    rng = np.random.default_rng(5)
    for i, name in enumerate(NAMES):
        d, affine, pixdim = _write_subject(data, name, 'sa', (20, 28, 2, FRAMES[i]), 60 + i)
        nifti.save(rng.integers(0, 4, size=(20, 28, 2, FRAMES[i])).astype(np.uint8), str(d / 'label_sa.nii.gz'), affine, pixdim)
    single = root / 'single'
    shutil.copytree(str(data), str(single / 'data'))
    F, _ = DN.define_flags().parse(['--data_dir', 'data', '--num_shards', '1', '--shard_index', '0'] + table_flags(single))
    back = os.getcwd()
    os.chdir(str(single))                                       # the gate's messages name the label file: 'data/...' in every run
    try:
        assert DN.run(F, stub_forward, log=lambda *_: None) == NAMES
    finally:
        os.chdir(back)
    want = {t: open(str(single / t), newline='').read() for t in TABLES}
    for t in TABLES:                                            # every table holds rows of every subject
        assert {line.split(',')[0] for line in want[t].splitlines()[1:]} == set(NAMES), t
    script = root / 'worker.py'
    script.write_text(WORKER.format(root=ROOT))
    return data, want, str(script)


def merged(where, n, tables=TABLES):
    """The tables of a launch of n workers.  shard.launch has merged --output_csv; the gate and score tables have a merge of their
    own; the confidence table has none (its frame column holds 'all' next to numbers): its parts are put together here the same
    way -- subjects sorted, the rows of a subject in the order its worker wrote them, one copy of a subject two workers hold."""
    where = str(where)
    assert measures.merge_shard_csv(os.path.join(where, 'qc_csv'), n)
    assert 'score_csv' not in tables or seg_score.merge_csv(os.path.join(where, 'score_csv'), n)
    header, by_subject = None, {}
    for i in range(n):
        part = measures.shard_csv_name(os.path.join(where, 'confidence_csv'), i, n)
        lines = open(part, newline='').read().splitlines(True)
        os.remove(part)
        header, mine = lines[0], {}
        for line in lines[1:]:
            mine.setdefault(line.split(',')[0], []).append(line)
        for name, rows in mine.items():
            assert by_subject.setdefault(name, rows) == rows, name          # two workers, one text
    got = {t: open(os.path.join(where, t), newline='').read() for t in tables if t != 'confidence_csv'}
    got['confidence_csv'] = header + ''.join(''.join(by_subject[name]) for name in sorted(by_subject))
    return got


def segmented(where, n):
    return [open(os.path.join(str(where), 'segmented%d' % r)).read().split() for r in range(n)]


def nothing_left_behind(data, where):
    for name in NAMES:
        assert not [f for f in os.listdir(str(data / name)) if f.startswith('.claim') or '.tmp.' in f], name
    assert not [f for f in os.listdir(str(where)) if '.tmp.' in f or '.shard' in f]


def launch(cohort, tmp_path, monkeypatch, tag, n, extra, mode='ok', tables=TABLES):
    data, want, script = cohort
    where = tmp_path / tag
    where.mkdir()
    if not (tmp_path / 'data').exists():
        shutil.copytree(str(data), str(tmp_path / 'data'))
    monkeypatch.chdir(tmp_path)
    rc = shard.launch(n, [script, 'data', str(where), mode] + table_flags(where, tables) + list(extra))
    return rc, where


@pytest.mark.parametrize('save_seg', [True, False], ids=['save_seg', 'nosave_seg'])
@pytest.mark.parametrize('workers', [2, 3])
def test_every_subject_once_and_the_tables_of_one_worker(cohort, tmp_path, monkeypatch, workers, save_seg):
    extra = [] if save_seg else ['--save_seg=false']
    tables = TABLES if workers == 2 else NO_SCORE
    want = {t: cohort[1][t] for t in tables}
    rc, where = launch(cohort, tmp_path, monkeypatch, 'first', workers, extra, tables=tables)
    assert rc == 0
    by_worker = segmented(where, workers)
    assert sorted(sum(by_worker, [])) == NAMES, by_worker                       # complete, and nobody's work done twice
    assert merged(where, workers, tables) == want
    nothing_left_behind(tmp_path / 'data', where)
    done = [name for name in NAMES if os.path.exists(str(tmp_path / 'data' / name / 'seg_sa.nii.gz'))]
    assert done == (NAMES if save_seg else [])
    if save_seg:
        return
    assert by_worker == [shard.subjects_for_shard(NAMES, r, workers) for r in range(workers)]      # no label file, no stealing
    if workers != 3:                                                            # once is enough, and cheapest without the score table
        return
    # the same command again: no output, so nothing is done (the reference's rule) -- whatever kept the subjects apart within the
    # first launch must not outlive it
    rc, where = launch(cohort, tmp_path, monkeypatch, 'again', workers, extra, tables=tables)
    assert rc == 0
    assert sorted(sum(segmented(where, workers), [])) == NAMES
    assert merged(where, workers, tables) == want
    nothing_left_behind(tmp_path / 'data', where)


def test_a_worker_that_dies_without_save_seg_loses_its_share_and_the_rerun_segments_everything(cohort, tmp_path, monkeypatch, capfd):
    """The --save_seg=false twin of test_shard.py's dying worker.  Nothing on disk says what is done, so the survivor keeps to its
    share, the launcher reports the dead worker, and the rerun starts over."""
    rc, where = launch(cohort, tmp_path, monkeypatch, 'die', 2, ['--save_seg=false'], mode='die', tables=NO_SCORE)
    assert rc == 9 and 'shard 0 of 2' in capfd.readouterr().err
    dead, survivor = segmented(where, 2)
    assert survivor == shard.subjects_for_shard(NAMES, 1, 2) and dead == NAMES[:1]         # it died in its second subject
    for name in NAMES:
        assert sorted(os.listdir(str(tmp_path / 'data' / name))) == ['label_sa.nii.gz', 'sa.nii.gz']
    rc, where = launch(cohort, tmp_path, monkeypatch, 'rerun', 2, ['--save_seg=false'], tables=NO_SCORE)
    assert rc == 0 and segmented(where, 2) == [shard.subjects_for_shard(NAMES, r, 2) for r in range(2)]
    assert merged(where, 2, NO_SCORE) == {t: cohort[1][t] for t in NO_SCORE}
    nothing_left_behind(tmp_path / 'data', where)


# ---- the walk: what is done is decided while the claim is held -----------------------------------------------------------------
def test_a_subject_finished_between_the_look_and_the_claim_is_not_segmented_again(cohort, tmp_path):
    data = tmp_path / 'data'
    shutil.copytree(str(cohort[0]), str(data))
    F, _ = DN.define_flags().parse(['--data_dir', str(data), '--num_shards', '2', '--shard_index', '0', '--io_threads', '0'])

    class Queue(shard.ClaimQueue):
        """Another worker writes subj02's label file and releases its claim right before this one's take succeeds."""
        def take(self, name):
            ok = super().take(name)
            if ok and name == 'subj02':
                nifti.save(np.zeros((20, 28, 2, 4)), str(data / name / 'seg_sa.nii.gz'), np.eye(4))
            return ok
    queue = Queue(str(data), NAMES, 0, 2, 'seg_sa', stealing=True)
    lines = []
    run = SequenceRun(F, None, LabelTables(F), queue, lines.append, list(queue))
    seen = []
    for item in run.walk():
        seen.append(item[0])
        assert os.path.exists(shard.claim_path(item[1], 'seg_sa'))
        queue.done(item[0])
    assert 'subj02' not in seen and sorted(seen) == sorted(set(NAMES) - {'subj02'})
    assert not os.path.exists(shard.claim_path(str(data / 'subj02'), 'seg_sa')) and not queue.held
    assert lines.count('subj02') == 1                                           # logged like any subject found done


# ---- a claim names the process, not only the pid ---------------------------------------------------------------------------------
def _start_time(pid):
    stat = open('/proc/%d/stat' % pid).read()
    return stat[stat.rindex(')') + 2:].split()[19]


def test_a_live_pid_with_another_start_time_is_a_reused_pid(tmp_path):
    d, parent = str(tmp_path), os.getppid()
    path = shard.claim_path(d, 'seg_sa')

    def plant(text):
        with open(path, 'w') as f:
            f.write(text)
    plant('%s %d %s\n' % (nifti._host_tag(), parent, _start_time(parent)))     # the live process itself: respected
    assert not shard.try_claim(d, 'seg_sa')
    plant('%s %d\n' % (nifti._host_tag(), parent))                              # a claim of the two-field format: the pid alone decides
    assert not shard.try_claim(d, 'seg_sa')
    plant('%s %d -\n' % (nifti._host_tag(), parent))                            # written where /proc did not tell: likewise
    assert not shard.try_claim(d, 'seg_sa')
    plant('%s %d %d\n' % (nifti._host_tag(), parent, int(_start_time(parent)) - 1))      # same pid, started at another time: its writer is gone
    assert shard.try_claim(d, 'seg_sa')
    assert open(path).read().split() == [nifti._host_tag(), str(os.getpid()), _start_time(os.getpid())]
    shard.release_claim(d, 'seg_sa')
    assert os.listdir(d) == []
    assert shard._pid_start(parent) == _start_time(parent) and shard._pid_start(os.getpid()) == _start_time(os.getpid())


def test_subjects_left_to_a_foreign_claim_are_named(cohort, tmp_path):
    data = tmp_path / 'data'
    shutil.copytree(str(cohort[0]), str(data))
    parent = os.getppid()
    with open(shard.claim_path(str(data / 'subj03'), 'seg_sa'), 'w') as f:      # a live process that is no worker of this run
        f.write('%s %d %s\n' % (nifti._host_tag(), parent, _start_time(parent)))
    F, _ = DN.define_flags().parse(['--data_dir', str(data), '--num_shards', '2', '--shard_index', '1', '--io_threads', '0'])
    lines = []
    done = DN.run(F, stub_forward, log=lambda *a: lines.append(' '.join(map(str, a))))
    assert sorted(done) == sorted(set(NAMES) - {'subj03'})
    assert [line for line in lines if 'not segmented here' in line] == \
        ['Left to the worker whose claim (.claim.seg_sa) they carry, not segmented here: subj03']
    assert os.path.exists(shard.claim_path(str(data / 'subj03'), 'seg_sa'))     # and the claim is still its owner's


# ---- UKBB_IO_THREADS -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('text,ventricular,aortic', [('', 8, 2), ('abc', 8, 2), ('-3', 8, 2), ('0', 8, 2), ('5', 5, 2), ('1', 1, 1), (None, 8, 2)])
def test_a_malformed_io_threads_variable_leaves_the_defaults(monkeypatch, text, ventricular, aortic):
    if text is None:
        monkeypatch.delenv('UKBB_IO_THREADS', raising=False)
    else:
        monkeypatch.setenv('UKBB_IO_THREADS', text)
    assert DN.define_flags().parse(['--data_dir', 'x'])[0].io_threads == ventricular
    assert DA.define_flags().parse(['--data_dir', 'x'])[0].io_threads == aortic
    assert shard.io_threads_from_env(8) == ventricular
