"""What --precision bf16_full (UKBB_PREC_BF16_FULL) does to the FCN step: the labels-only forward of ONE engine per model at the headline shape (FCN_sa,
64 x 192 x 208) and at the long-axis shape (FCN_la_2ch, 64 x 176 x 208) in fp32, bf16 (operands only), bf16_store and bf16_full -- the four taken in turn
--rounds times (>= 5), every sample --reps steps between two device events after a warm-up of the freshly built plan (tools/bench_fcn_bf16_store.py's
Step and in_turn), reported as RANGES (min .. max) with the median; whether EVERY bf16_full sample beat every bf16_store sample (the project's all-runs
rule); the per-kernel times of the bf16_full plan next to bf16_store's head; the share of the timed batch's voxels whose label differs from fp32's; and,
with --parent_root (a built tree of the parent commit, run in a fresh process that imports that tree's package and library), the parent's fp32 and
bf16_store steps with this build's again right after, and whether the labels of the timed batch are bit-identical between the two builds.
--test_log FILE ... appends the head's figures and the Dice lines from the printed output of tests/test_fcn_bf16_full_launches_gpu.py /
tests/test_fcn_bf16_full_gpu.py (pytest -s).

GPU box only.   python tools/bench_fcn_bf16_full.py [--reps 30] [--rounds 7] [--parent_root DIR] [--test_log FILE ...] [--out profiles/fcn_bf16_full.txt]"""
import argparse
import hashlib
import os
import re
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_fcn_bf16_store import SHAPES, Step, in_turn            # noqa: E402  (puts UKBB_BENCH_ROOT or this tree on sys.path)

PRECS = ('fp32', 'bf16', 'bf16_store', 'bf16_full')
SHARED = ('fp32', 'bf16_store')                                    # what the parent commit has too: must not move


def digest(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def fmt(v):
    return '%7.4f .. %7.4f ms (median %7.4f)' % (min(v), max(v), float(np.median(v)))


def summary_of_test_logs(paths):
    rows, worst, dice = 0, [1.0, 0.0, 0.0, 0.0], []
    sq = {}
    for path in paths:
        with open(path) as f:
            for ln in f:
                m = re.search(r'fcn-bf16-full (\S+)\s+head\s+zero-slack pixels ([\d.]+), worst err/scale on them (\S+), worst \(err - slack\)/scale (\S+),', ln)
                if m:
                    rows += 1
                    worst = [min(worst[0], float(m.group(2))), max(worst[1], float(m.group(3))), max(worst[2], float(m.group(4))), worst[3]]
                m = re.search(r'fcn-bf16-full (\S+)\s+(g\d|prob)\s+(\S+) \(bound (\S+)\)', ln)
                if m:
                    sq[m.group(2)] = max(sq.get(m.group(2), 0.0), float(m.group(3)))
                if 'fcn-bf16-full deploy' in ln:
                    dice.append(ln[ln.index('fcn-bf16-full deploy'):].strip())
    out = []
    if rows:
        out.append('head launches against the float64 interval model (tests/fcn_bf16_full_grading.py), worst over %d graded cases: smallest share of zero-slack '
                   'pixels %.3f (floor 0.40); worst |logits - model| / scale on zero-slack pixels %.2e (bound 1e-05); worst (|logits - model| - slack) / scale over '
                   'all pixels %.2e (bound 1e-05)' % (rows, worst[0], worst[1], worst[2]))
    for k in sorted(sq):
        out.append('  %-5s worst over the cases %.2e (bound %s)' % (k, sq[k], '1e-06' if k == 'prob' else '1e-05'))
    return out + dice


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--parent_root', default='', help='a built tree of the parent commit: its fp32 and bf16_store steps are timed in a fresh process')
    ap.add_argument('--test_log', nargs='*', default=[], help='printed output of the two GPU test files (pytest -s): their figures are appended')
    ap.add_argument('--out', default='', help='also write the report here')
    ap.add_argument('--only_shared', default='', help='(the child process) MODEL,N,H,W: time fp32 and bf16_store alone, print samples and label digests')
    args = ap.parse_args(argv)
    if args.rounds < 5:
        sys.exit('bench_fcn_bf16_full: at least 5 rounds')
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_fcn_bf16_full: needs a GPU')
    if args.only_shared:
        model, n, H, W = args.only_shared.split(',')
        step = Step(model, int(n), int(H), int(W))
        got = in_turn(step, SHARED, args.reps, args.rounds)
        for p in SHARED:
            print('SHARED_MS %s %s %s' % (p, digest(step.labels(p)), ' '.join('%.6f' % v for v in got[p])))
        return
    lines = []

    def say(text=''):
        print(text, flush=True)
        lines.append(text)
    say('bench_fcn_bf16_full: labels-only step, one engine per model, the precisions in turn; %d steps per sample, %d samples each: min .. max (median)' % (args.reps, args.rounds))
    for model, n, H, W in SHAPES:
        step = Step(model, n, H, W)
        got = in_turn(step, PRECS, args.reps, args.rounds)
        say('%s %d x %d x %d' % (model, n, H, W))
        for p in PRECS:
            v = got[p]
            say('  %-10s %s   %7.0f .. %7.0f slices/s' % (p, fmt(v), n / (max(v) * 1e-3), n / (min(v) * 1e-3)))
        every = max(got['bf16_full']) < min(got['bf16_store'])
        say('  every bf16_full sample %s every bf16_store sample (slowest bf16_full %.4f ms, fastest bf16_store %.4f ms; medians %.3fx)' % (
            'beat' if every else 'did NOT beat', max(got['bf16_full']), min(got['bf16_store']), float(np.median(got['bf16_store']) / np.median(got['bf16_full']))))
        lab = {p: step.labels(p) for p in PRECS}
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
                    say('  %-10s tree of the parent commit %s; this build again, right after: %s; labels of the timed batch %s' % (
                        p, fmt(v), fmt(again[p]), 'bit-identical' if r[2] == digest(lab[p]) else 'DIFFER'))
        say('  labels of the timed batch differing from fp32: bf16 %.4f %%, bf16_store %.4f %%, bf16_full %.4f %% of %d voxels; bf16_full from bf16_store %.4f %%' % (
            100.0 * float((lab['bf16'] != lab['fp32']).mean()), 100.0 * float((lab['bf16_store'] != lab['fp32']).mean()),
            100.0 * float((lab['bf16_full'] != lab['fp32']).mean()), lab['fp32'].size, 100.0 * float((lab['bf16_full'] != lab['bf16_store']).mean())))
        # per-kernel times (events around every launch: the launches no longer overlap their neighbours' ramps)
        eng = step.eng
        per = {}
        for p in ('bf16_store', 'bf16_full'):
            eng.set_precision(p)
            for _ in range(3):
                step()
            eng.set_timing(True)
            for _ in range(args.reps):
                step()
            torch.cuda.synchronize()
            ms, cnt = eng.kernel_times()
            eng.set_timing(False)
            per[p] = [(name, cfg, 1e3 * t / max(c, 1)) for name, cfg, t, c in zip(eng.kernel_names(), eng.kernel_configs(), ms, cnt)]
        say('  bf16_full plan, per kernel (mean of %d timed launches; in brackets the same launch of the bf16_store plan):' % args.reps)
        for (name, cfg, us), (_, _, us_s) in zip(per['bf16_full'], per['bf16_store']):
            say('    %-18s tiling %3d  %7.1f us  (%7.1f)' % (name, cfg, us, us_s))
        say('    sum %7.1f us  (%7.1f)' % (sum(r[2] for r in per['bf16_full']), sum(r[2] for r in per['bf16_store'])))
        step.eng.close()
    for ln in summary_of_test_logs(args.test_log):
        say(ln)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
