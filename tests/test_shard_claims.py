"""The claim protocol of shard.py (try_claim / release_claim) under every order in which the system calls of several workers can
reach the file system.

Each simulated worker runs the real ``try_claim`` in a thread of its own.  The module-level calls of shard.py that touch the file
system -- exclusive create, read, remove -- are replaced by versions that stop at a gate first; a scheduler opens exactly one gate
per step, following a schedule (a list of worker names).  A worker's thread runs from one gate to the next while every other thread
stands still, so a schedule decides the outcome: no sleeps, no timing.  Behind the gate the real call runs on a real directory.

Gated: ``_create_excl``, ``_remove``, ``_read_text`` -- the first call of a staleness judgement -- and the owner's 'work' step.  Not
gated: ``_mtime`` and the pid probes of the same judgement, which run in the step of its read.  A judgement therefore sees one state
of the file system.  What that leaves out are orders in which the file changes between the read and the mtime call: the mtime then
fails (not stale) or is that of a younger file (not stale by age either, and age decides nothing for a same-host claim), so only
orders in which a sweeper backs off.

After every step the invariants are checked:
  * at most one worker has been told that it owns the subject and has not released it;
  * that worker's claim file exists and names it;
  * no worker removes a file that names another live worker;
and after the last step, once every owner has released: no file of the protocol is left in the subject's directory.

``remove_then_create`` is the take-over shard.py had before (remove the stale claim, create again): the checker must fail on it.
"""
import os
import random
import threading

import pytest

from ukbb_cardiac_amd import nifti, shard

WHAT = 'seg_sa'
DEAD_PID = 4000000                                          # above any pid_max in use: the planted claim's writer
PIDS = {'X': 4000001, 'Y': 4000002, 'Z': 4000003}


def remove_then_create(subject_dir, what):
    """The known-bad protocol: try_claim as it was, on the same gated calls."""
    path = shard.claim_path(subject_dir, what)
    for attempt in range(2):
        try:
            shard._create_excl(path, shard._claim_text())
        except FileExistsError:
            if attempt == 0 and shard._claim_is_stale(path):
                try:
                    shard._remove(path)
                except OSError:
                    pass
                continue
            return False
        except OSError:
            return False
        return True
    return False


class Actor(threading.Thread):
    def __init__(self, world, name, body):
        super().__init__(name=name, daemon=True)
        self.world, self.body = world, body
        self.go = threading.Semaphore(0)
        self.finished, self.owns, self.told, self.error = False, False, None, None

    def run(self):
        try:
            self.body(self)
        except BaseException as e:                          # noqa: B902  (reported by the scheduler's thread)
            self.error = e
        finally:
            self.finished = True
            self.world.back.release()


class World:
    """One subject directory, its workers and the gates between them."""

    def __init__(self, directory, monkeypatch, claim=shard.try_claim):
        self.dir, self.claim = str(directory), claim
        self.path = shard.claim_path(self.dir, WHAT)
        self.back = threading.Semaphore(0)
        self.actors, self.trace, self.violations = {}, [], []
        real = {n: getattr(shard, n) for n in ('_create_excl', '_read_text', '_remove')}

        def me():
            return self.actors.get(threading.current_thread().name)

        def gated(name):
            def call(path, *args):
                actor = me()
                if actor is None or path.startswith('/proc/'):
                    return real[name](path, *args)
                self.gate(actor, name, path)
                before = self.names(path) if name == '_remove' else None
                try:
                    out = real[name](path, *args)
                except OSError as e:
                    self.trace[-1] += '->' + type(e).__name__
                    raise
                if before in PIDS and before != actor.name:
                    self.violations.append('%s removed %s, which named the live worker %s' % (actor.name, os.path.basename(path), before))
                return out
            return call
        for n in real:
            monkeypatch.setattr(shard, n, gated(n))
        monkeypatch.setattr(shard, '_own_pid', lambda: PIDS[me().name] if me() else os.getpid())
        monkeypatch.setattr(shard, '_pid_alive', lambda pid: pid in PIDS.values())
        monkeypatch.setattr(shard, '_pid_start', lambda pid: 'started%d' % pid)

    def names(self, path):
        """The worker a file names, '?' for any other content, None for no file."""
        try:
            parts = open(path).read().split()
        except OSError:
            return None
        by_pid = {str(p): n for n, p in PIDS.items()}
        return by_pid.get(parts[1], '?') if len(parts) > 1 else '?'

    def gate(self, actor, op, path):
        actor.pending = '%s.%s%s' % (actor.name, op.strip('_'), '' if path in ('', self.path) else ':' + os.path.basename(path)[len('.claim.' + WHAT):])
        self.back.release()
        actor.go.acquire()
        self.trace.append(actor.pending)

    # ---- what the workers do
    def sweeper(self, actor):
        actor.told = self.claim(self.dir, WHAT)
        actor.owns = bool(actor.told)

    def owner(self, actor):
        """Claims, works and releases."""
        self.sweeper(actor)
        if actor.owns:
            self.gate(actor, 'work', '')
            actor.owns = False                              # from here on the file may name it, but it no longer counts on that
            shard.release_claim(self.dir, WHAT)

    # ---- the scheduler
    def check(self):
        owners = [a.name for a in self.actors.values() if a.owns]
        if len(owners) > 1:
            self.violations.append('%s were all told that they own the subject' % ' and '.join(owners))
        elif owners and self.names(self.path) != owners[0]:
            self.violations.append('%s owns the subject, its claim file names %s' % (owners[0], self.names(self.path)))

    def run(self, bodies, pick):
        """bodies: {name: body}.  pick(step, runnable names) -> the name whose gate opens.  Returns (trace, choices, runnable sets)."""
        self.actors = {n: Actor(self, n, b) for n, b in bodies.items()}
        for a in self.actors.values():
            a.start()
        for _ in self.actors:
            self.back.acquire()
        choices, offered = [], []
        while True:
            runnable = sorted(n for n, a in self.actors.items() if not a.finished)
            if not runnable:
                break
            name = pick(len(choices), runnable)
            choices.append(name)
            offered.append(runnable)
            self.actors[name].go.release()
            self.back.acquire()
            for a in self.actors.values():
                if a.error is not None:
                    raise a.error
            self.check()
        for a in self.actors.values():                      # everybody releases; nothing of the protocol may stay behind
            a.join()
            if a.owns:
                shard.release_claim(self.dir, WHAT)
                a.owns = False
        left = sorted(os.listdir(self.dir))
        if left:
            self.violations.append('left behind: %s' % ' '.join(left))
            for f in left:
                os.remove(os.path.join(self.dir, f))
        return self.trace, choices, offered


def plant_stale_claim(directory):
    with open(shard.claim_path(str(directory), WHAT), 'w') as f:
        f.write('%s %d started%d\n' % (nifti._host_tag(), DEAD_PID, DEAD_PID))


def one_schedule(directory, monkeypatch, claim, roles, pick, plant=True):
    with monkeypatch.context() as m:
        world = World(directory, m, claim)
        if plant:
            plant_stale_claim(directory)
        trace, choices, offered = world.run({n: getattr(world, r) for n, r in roles.items()}, pick)
        told = {n: a.told for n, a in world.actors.items()}
    return trace, choices, offered, world.violations, told


def every_interleaving(directory, monkeypatch, claim, roles):
    """Depth first over the tree of schedules: run a prefix, then always the first runnable worker, and queue every other choice
    that was open behind the prefix.  Every complete schedule comes up exactly once."""
    todo, out = [[]], []
    while todo:
        prefix = todo.pop()
        trace, choices, offered, violations, told = one_schedule(directory, monkeypatch, claim, roles, lambda i, names: prefix[i] if i < len(prefix) else names[0])
        out.append((trace, violations, told))
        for i in range(len(prefix), len(choices)):
            todo.extend(choices[:i] + [other] for other in offered[i] if other != choices[i])
    return out


SWEEPERS = {'X': 'sweeper', 'Y': 'sweeper'}
# the order of the calls that lets both sweepers own the subject under remove-then-create
BOTH_OWN = ['X.create_excl->FileExistsError', 'Y.create_excl->FileExistsError', 'X.read_text', 'Y.read_text',
            'X.remove', 'X.create_excl', 'Y.remove', 'Y.create_excl']


def test_two_sweepers_on_one_stale_claim_every_interleaving(tmp_path, monkeypatch):
    runs = every_interleaving(tmp_path, monkeypatch, shard.try_claim, SWEEPERS)
    assert 200 <= len(runs) <= 5000 and len({tuple(t) for t, _, _ in runs}) == len(runs), len(runs)
    bad = [(t, v) for t, v, _ in runs if v]
    assert not bad, '%d of %d schedules, the first: %s' % (len(bad), len(runs), bad[0])
    # the set holds the schedules in which both have judged the claim stale before either sweeps: the ones remove-then-create loses
    assert sum(t[:4] == BOTH_OWN[:4] for t, _, _ in runs) > 1
    # and in every one of them the subject ends up with exactly one owner: a stale claim does not cost the visit
    assert all(sorted(told.values()) == [False, True] for _, _, told in runs)


def test_the_checker_fails_remove_then_create(tmp_path, monkeypatch):
    runs = every_interleaving(tmp_path, monkeypatch, remove_then_create, SWEEPERS)
    by_calls = {tuple(t): (v, told) for t, v, told in runs}
    assert tuple(BOTH_OWN) in by_calls, len(runs)
    violations, told = by_calls[tuple(BOTH_OWN)]
    assert told == {'X': True, 'Y': True}
    assert any('removed .claim.seg_sa, which named the live worker X' in v for v in violations), violations
    assert any('were all told that they own' in v for v in violations), violations
    # the same schedule, given as a schedule, against the real protocol: one owner, nothing to report
    order = iter(''.join(c[0] for c in BOTH_OWN) + 'XY' * 8)

    def pick(i, names):
        want = next(order)
        return want if want in names else names[0]
    trace, _, _, violations, told = one_schedule(tmp_path, monkeypatch, shard.try_claim, SWEEPERS, pick)
    assert trace[:4] == BOTH_OWN[:4] and not violations and sorted(told.values()) == [False, True], (trace, violations)


# seeds of the random three-worker schedules: step i opens the gate of runnable[int(random() * len(runnable))], and random.Random(seed)
# .random() is the one generator whose sequence Python promises to keep
SEEDS = range(1100)
THREE = {'an owner that claims, works and releases': ({'X': 'sweeper', 'Y': 'sweeper', 'Z': 'owner'}, None),
         'a third claimer that comes late': ({'X': 'sweeper', 'Y': 'sweeper', 'Z': 'sweeper'}, 'Z')}


@pytest.mark.parametrize('case', sorted(THREE))
def test_three_workers_seeded_schedules(tmp_path, monkeypatch, case):
    roles, late = THREE[case]
    seen, bad, outcomes = set(), [], set()
    for seed in SEEDS:
        rng = random.Random(seed)
        hold = 2 + seed % 9                                 # the late one's first call waits for this many calls of the others

        def pick(i, names):
            if late in names and i < hold and len(names) > 1:
                names = [n for n in names if n != late]
            return names[int(rng.random() * len(names))]
        trace, _, _, violations, told = one_schedule(tmp_path, monkeypatch, shard.try_claim, roles, pick)
        seen.add(tuple(trace))
        outcomes.add(tuple(sorted(n for n, t in told.items() if t)))
        if violations:
            bad.append((seed, trace, violations))
    assert not bad, '%d of %d schedules, the first: %s' % (len(bad), len(SEEDS), bad[0])
    assert len(seen) >= 500, len(seen)                      # the seeds do spread over the tree
    if late is None:
        assert ('X', 'Z') in outcomes or ('Y', 'Z') in outcomes          # one after the other is fine: Z released in between
    assert {o for o in outcomes if len(o) == 1} >= {('X',), ('Y',), ('Z',)}, outcomes


def test_three_workers_schedules_catch_remove_then_create(tmp_path, monkeypatch):
    """The seeded schedules are no weaker a net than the enumeration: remove-then-create falls through them too."""
    roles, late = THREE['a third claimer that comes late']
    caught = 0
    for seed in SEEDS[:200]:
        rng = random.Random(seed)
        violations = one_schedule(tmp_path, monkeypatch, remove_then_create, roles, lambda i, names: names[int(rng.random() * len(names))])[3]
        caught += bool(violations)
    assert caught >= 5, caught


def test_an_abandoned_sweep_file_costs_one_visit(tmp_path, monkeypatch):
    """A sweeper that died between taking the sweep file and giving it back: the next visit removes that file and leaves the subject,
    the visit after that takes the subject over.  A sweep file of a live worker is left alone."""
    d = str(tmp_path)
    path = shard.claim_path(d, WHAT)
    plant_stale_claim(tmp_path)
    monkeypatch.setattr(shard, '_pid_alive', lambda pid: pid != DEAD_PID)
    monkeypatch.setattr(shard, '_pid_start', lambda pid: 'started%d' % pid)
    with open(path + '.sweep', 'w') as f:
        f.write('%s %d started%d\n' % (nifti._host_tag(), os.getppid(), os.getppid()))
    assert not shard.try_claim(d, WHAT) and not shard.try_claim(d, WHAT) and os.path.exists(path + '.sweep')
    with open(path + '.sweep', 'w') as f:
        f.write('%s %d started%d\n' % (nifti._host_tag(), DEAD_PID, DEAD_PID))
    assert not shard.try_claim(d, WHAT) and not os.path.exists(path + '.sweep')
    assert shard.try_claim(d, WHAT) and open(path).read().split()[1] == str(os.getpid())
    shard.release_claim(d, WHAT)
    assert os.listdir(d) == []
