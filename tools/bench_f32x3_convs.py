"""What ukbb_fcn_set_f32x3_convs (Engine.set_f32x3_convs, deploy_network.py --f32x3_convs) does to the FCN step: the labels-only forward of ONE engine
per model at the headline shape (FCN_sa, 64 x 192 x 208) and at the long-axis shape (FCN_la_2ch, 64 x 176 x 208) in fp32, in f32x3 and in f32x3 with
the switch ('f32x3+convs') -- the three taken in turn --rounds times (>= 5), every sample --reps steps between two device events after a warm-up of
the freshly built plan (tools/bench_fcn_bf16_store.py's Step and in_turn), reported as RANGES (min .. max) with the median; win or loss of the switch
against f32x3 and against fp32 by the project's all-runs rule (every sample of the one against every sample of the other), per step and per layer;
the per-kernel times of the three plans (ukbb_fcn_set_timing); the share of the timed batch's voxels whose label differs from fp32's; and, with
--parent_root (a built tree of the parent commit, run in a fresh process that imports that tree's package and library), the parent's fp32 and f32x3
steps with this build's again right after, and whether the labels of the timed batch are bit-identical between the two builds.

GPU box only.   python tools/bench_f32x3_convs.py [--reps 30] [--rounds 7] [--parent_root DIR] [--out FILE]"""
import argparse
import hashlib
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_fcn_bf16_store import SHAPES, Step, in_turn            # noqa: E402  (puts UKBB_BENCH_ROOT or this tree on sys.path)

SWITCH = 'f32x3+convs'
MODES = ('fp32', 'f32x3', SWITCH)
SHARED = ('fp32', 'f32x3')                                         # what the parent commit has too: must not move
SAMPLES = 5                                                        # per-kernel samples of --reps timed launches each


class ModeStep(Step):
    """Step whose 'precision' may be SWITCH: f32x3 with the conv stack on three bf16 pieces as well."""

    def set_mode(self, mode):
        if hasattr(self.eng, 'set_f32x3_convs'):                   # (the parent commit's engine has no switch, and is asked for SHARED only)
            self.eng.set_f32x3_convs(mode == SWITCH)
        self.eng.set_precision('f32x3' if mode == SWITCH else mode)

    def sample(self, mode, reps):
        import torch
        from bench_fcn_bf16_store import timed
        self.set_mode(mode)
        for _ in range(5):
            self()
        torch.cuda.synchronize()
        return timed(self, reps)

    def labels(self, mode):
        import torch
        self.set_mode(mode)
        self()
        torch.cuda.synchronize()
        return self.pred.cpu().numpy().copy()

    def per_kernel(self, mode, reps, samples=SAMPLES):
        """[(name, tiling, [us per launch, one figure per sample])] with events around every launch."""
        import torch
        self.set_mode(mode)
        for _ in range(3):
            self()
        eng = self.eng
        rows = None
        for _ in range(samples):
            eng.set_timing(True)
            for _ in range(reps):
                self()
            torch.cuda.synchronize()
            ms, cnt = eng.kernel_times()
            eng.set_timing(False)
            us = [1e3 * t / max(c, 1) for t, c in zip(ms, cnt)]
            if rows is None:
                rows = [(name, cfg, []) for name, cfg in zip(eng.kernel_names(), eng.kernel_configs())]
            for r, v in zip(rows, us):
                r[2].append(v)
        return rows


def digest(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def fmt(v):
    return '%7.4f .. %7.4f ms (median %7.4f)' % (min(v), max(v), float(np.median(v)))


def verdict(mine, other):
    """The all-runs rule: a win only if every sample of `mine` is below every sample of `other`, a loss only the other way round."""
    if max(mine) < min(other):
        return 'WIN'
    if min(mine) > max(other):
        return 'LOSS'
    return 'no difference (ranges overlap)'


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--parent_root', default='', help='a built tree of the parent commit: its fp32 and f32x3 steps are timed in a fresh process')
    ap.add_argument('--out', default='', help='also write the report here')
    ap.add_argument('--only_shared', default='', help='(the child process) MODEL,N,H,W: time fp32 and f32x3 alone, print samples and label digests')
    args = ap.parse_args(argv)
    if args.rounds < 5:
        sys.exit('bench_f32x3_convs: at least 5 rounds')
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_f32x3_convs: needs a GPU')
    if args.only_shared:
        model, n, H, W = args.only_shared.split(',')
        step = ModeStep(model, int(n), int(H), int(W))
        got = in_turn(step, SHARED, args.reps, args.rounds)
        for p in SHARED:
            print('SHARED_MS %s %s %s' % (p, digest(step.labels(p)), ' '.join('%.6f' % v for v in got[p])))
        return
    lines = []

    def say(text=''):
        print(text, flush=True)
        lines.append(text)
    say('bench_f32x3_convs: labels-only step, one engine per model, the modes in turn; %d steps per sample, %d samples each: min .. max (median)' % (args.reps, args.rounds))
    for model, n, H, W in SHAPES:
        step = ModeStep(model, n, H, W)
        got = in_turn(step, MODES, args.reps, args.rounds)
        say('%s %d x %d x %d' % (model, n, H, W))
        for p in MODES:
            v = got[p]
            say('  %-12s %s   %7.0f .. %7.0f slices/s' % (p, fmt(v), n / (max(v) * 1e-3), n / (min(v) * 1e-3)))
        for other in ('f32x3', 'fp32'):
            say('  step, %s against %s: %s (slowest %.4f / fastest %.4f ms against fastest %.4f / slowest %.4f ms; medians %.3fx)' % (
                SWITCH, other, verdict(got[SWITCH], got[other]), max(got[SWITCH]), min(got[SWITCH]), min(got[other]), max(got[other]),
                float(np.median(got[other]) / np.median(got[SWITCH]))))
        lab = {p: step.labels(p) for p in MODES}
        if args.parent_root:
            env = dict(os.environ, UKBB_BENCH_ROOT=os.path.abspath(args.parent_root))
            cmd = [sys.executable, os.path.abspath(__file__), '--only_shared', '%s,%d,%d,%d' % (model, n, H, W), '--reps', str(args.reps), '--rounds', str(args.rounds)]
            out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            rows = [ln.split() for ln in out.stdout.splitlines() if ln.startswith('SHARED_MS')]
            if out.returncode or len(rows) != len(SHARED):
                say('  tree of the parent commit: the child process failed (%d): %s' % (out.returncode, out.stderr.strip()[-300:]))
            else:
                again = in_turn(step, SHARED, args.reps, args.rounds)
                for r in rows:
                    p, v = r[1], [float(t) for t in r[3:]]
                    say('  %-12s tree of the parent commit %s; this build again, right after: %s; labels of the timed batch %s' % (
                        p, fmt(v), fmt(again[p]), 'bit-identical' if r[2] == digest(lab[p]) else 'DIFFER'))
        say('  labels of the timed batch differing from fp32: f32x3 %.4f %%, %s %.4f %% of %d voxels' % (
            100.0 * float((lab['f32x3'] != lab['fp32']).mean()), SWITCH, 100.0 * float((lab[SWITCH] != lab['fp32']).mean()), lab['fp32'].size))
        # per-kernel times (events around every launch: the launches no longer overlap their neighbours' ramps)
        per = {p: step.per_kernel(p, args.reps) for p in MODES}
        say('  per kernel, us per launch, min .. max over %d samples of %d timed launches: the %s plan | the same layer in the f32x3 plan (fp32 convs) | verdict by the all-runs rule' % (
            SAMPLES, args.reps, SWITCH))
        for (name, cfg, us), (_, cfg_p, us_p) in zip(per[SWITCH], per['f32x3']):
            say('    %-18s tiling %3d  %7.1f .. %7.1f  | tiling %3d  %7.1f .. %7.1f  | %s' % (
                name, cfg, min(us), max(us), cfg_p, min(us_p), max(us_p), verdict(us, us_p) if cfg != cfg_p else 'the same launch'))
        for p in MODES:
            say('    sum of the medians, %-12s %7.1f us' % (p, sum(float(np.median(r[2])) for r in per[p])))
        step.eng.close()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
