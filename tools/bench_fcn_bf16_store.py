"""What --precision bf16_store (UKBB_PREC_BF16_STORE) does to the FCN step: the labels-only forward of ONE engine per model at the headline shape
(FCN_sa, 64 x 192 x 208) and at the long-axis shape (FCN_la_2ch, 64 x 176 x 208) in fp32, bf16 (operands only) and bf16_store -- the three taken in turn
--rounds times (>= 5), every sample --reps steps between two device events after a warm-up of the freshly built plan, reported as RANGES (min .. max)
with the median; whether EVERY bf16_store sample beat every fp32 sample and every bf16 sample (the project's all-runs rule); the fp32 step of a built
tree of the parent commit (--parent_root, a fresh process that imports that tree's package and library), with this build's fp32 step again right
after it; the per-kernel times of the bf16_store plan (ukbb_fcn_set_timing); and how the labels of the timed batch differ from the fp32 labels.
--test_log FILE ... appends the worst figure per tiling and per squeeze / head launch, and the Dice lines, from the printed output of
tests/test_fcn_bf16_store_launches_gpu.py / tests/test_fcn_bf16_store_gpu.py (pytest -s).

GPU box only.   python tools/bench_fcn_bf16_store.py [--reps 30] [--rounds 7] [--parent_root DIR] [--test_log FILE ...] [--out profiles/fcn_bf16_store.txt]"""
import argparse
import collections
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.environ.get('UKBB_BENCH_ROOT') or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))   # the child of --parent_root: that tree
sys.path.insert(0, ROOT)

SHAPES = [('FCN_sa', 64, 192, 208), ('FCN_la_2ch', 64, 176, 208)]
PRECS = ('fp32', 'bf16', 'bf16_store')


def timed(fn, reps):
    """ms per call of fn over ``reps`` calls between two device events."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


class Step:
    """The labels-only forward of one engine on one seeded batch."""

    def __init__(self, model, n, H, W):
        import torch
        from ukbb_cardiac_amd.arch import MODELS
        from ukbb_cardiac_amd.engine import Engine
        from ukbb_cardiac_amd.phantom import cine_phantom
        from ukbb_cardiac_amd.weights import synthetic_params
        self.arch = MODELS[model]
        self.n, self.H, self.W = n, H, W
        self.eng = Engine(self.arch, synthetic_params(self.arch, 1234), device=0)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.x = torch.from_numpy(cine_phantom(n, H, W, seed=3)).cuda()
        self.pred = torch.empty((n, H, W), dtype=torch.int32, device='cuda')

    def __call__(self):
        self.eng.run_device(self.x.data_ptr(), self.n, self.H, self.W, pred_ptr=self.pred.data_ptr(), stream=self.stream)

    def sample(self, prec, reps):
        """One sample: switch (re-plan, re-pack: outside the window), warm the new plan up, time ``reps`` steps."""
        import torch
        self.eng.set_precision(prec)
        for _ in range(5):
            self()
        torch.cuda.synchronize()
        return timed(self, reps)

    def labels(self, prec):
        import torch
        self.eng.set_precision(prec)
        self()
        torch.cuda.synchronize()
        return self.pred.cpu().numpy().copy()


def in_turn(step, precs, reps, rounds):
    got = {p: [] for p in precs}
    for r in range(rounds + 1):                          # the first turn is a warm-up of everything (code objects, allocations)
        for p in precs:
            ms = step.sample(p, reps)
            if r:
                got[p].append(ms)
    return got


def summary_of_test_logs(paths):
    """Lines for the report: per tiling the smallest half-ulp share and the largest deviation over the bound, per squeeze / head launch the worst figure."""
    enc, tail, dice = collections.defaultdict(lambda: [1.0, 0.0, 0]), collections.defaultdict(lambda: [0.0, '', 0]), []
    for path in paths:
        with open(path) as f:
            for ln in f:
                m = re.search(r'bf16-launch (FCN\S+ \S+)\s+(\S+)\s+tiling\s+(-?\d+)\s+(.*?)\s+within half an ulp ([\d.]+)\s+worst / bound ([\d.]+)', ln)
                if m:
                    key = 'stem (conv0_0+conv0_1)' if m.group(3) == '-1' else 'tiling %s' % m.group(3)
                    e = enc[key]
                    e[0], e[1], e[2] = min(e[0], float(m.group(5))), max(e[1], float(m.group(6))), e[2] + 1
                m = re.search(r'fcn-bf16-store (FCN\S+ \S+)\s+(g\d|logits|prob)\s+(\S+) \(bound (\S+)\)', ln)
                if m:
                    t = tail[m.group(2)]
                    if float(m.group(3)) >= t[0]:
                        t[0], t[1] = float(m.group(3)), m.group(4)
                    t[2] += 1
                if 'fcn-bf16-store deploy' in ln:
                    dice.append(ln[ln.index('fcn-bf16-store deploy'):].strip())
    out = []
    if enc:
        out.append('encoder launches against the float64 rounding model, figures against the half-ulp tolerance (half a bf16 ulp + 2^-18 |exact| + 2^-20 scale) every conv launch is held to; the stem is graded as a unit: 4 ulps + the slack of ambiguous conv0_0 roundings for every element, 99.5 % within half an ulp (tests/test_bf16_launches_gpu.py stem_reference):')
        for k in sorted(enc):
            out.append('  %-24s %4d launches  smallest share within half an ulp %.6f  largest deviation / bound %.3f' % (k, enc[k][2], enc[k][0], enc[k][1]))
    if tail:
        out.append('squeeze and head launches against the fp32 models on the stored values (worst over the cases):')
        for k in ('g1', 'g2', 'g3', 'g4', 'logits', 'prob'):
            if k in tail:
                out.append('  %-7s %4d launches  %.2e (bound %s)' % (k, tail[k][2], tail[k][0], tail[k][1]))
    return out + dice


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--parent_root', default='', help='a built tree of the parent commit: its fp32 step is timed in a fresh process')
    ap.add_argument('--test_log', nargs='*', default=[], help='printed output of the two GPU test files (pytest -s): their figures are appended')
    ap.add_argument('--out', default='', help='also write the report here')
    ap.add_argument('--only_fp32', default='', help='(the child process) MODEL,N,H,W: time the fp32 step alone and print its samples')
    args = ap.parse_args(argv)
    if args.rounds < 5:
        sys.exit('bench_fcn_bf16_store: at least 5 rounds')
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_fcn_bf16_store: needs a GPU')
    if args.only_fp32:
        model, n, H, W = args.only_fp32.split(',')
        got = in_turn(Step(model, int(n), int(H), int(W)), ('fp32',), args.reps, args.rounds)['fp32']
        print('FP32_MS ' + ' '.join('%.6f' % v for v in got))
        return
    lines = []

    def say(text=''):
        print(text, flush=True)
        lines.append(text)
    say('bench_fcn_bf16_store: labels-only step, one engine per model, the precisions in turn; %d steps per sample, %d samples each: min .. max (median)' % (args.reps, args.rounds))
    for model, n, H, W in SHAPES:
        step = Step(model, n, H, W)
        got = in_turn(step, PRECS, args.reps, args.rounds)
        say('%s %d x %d x %d' % (model, n, H, W))
        for p in PRECS:
            v = got[p]
            say('  %-10s %7.4f .. %7.4f ms (median %7.4f)   %7.0f .. %7.0f slices/s' % (p, min(v), max(v), float(np.median(v)), n / (max(v) * 1e-3), n / (min(v) * 1e-3)))
        for other in ('fp32', 'bf16'):
            every = max(got['bf16_store']) < min(got[other])
            say('  every bf16_store sample %s every %s sample (slowest bf16_store %.4f ms, fastest %s %.4f ms; medians %.2fx)' % (
                'beat' if every else 'did NOT beat', other, max(got['bf16_store']), other, min(got[other]), float(np.median(got[other]) / np.median(got['bf16_store']))))
        if args.parent_root:
            env = dict(os.environ, UKBB_BENCH_ROOT=os.path.abspath(args.parent_root))
            cmd = [sys.executable, os.path.abspath(__file__), '--only_fp32', '%s,%d,%d,%d' % (model, n, H, W), '--reps', str(args.reps), '--rounds', str(args.rounds)]
            out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            line = [l for l in out.stdout.splitlines() if l.startswith('FP32_MS')]
            if out.returncode or not line:
                say('  fp32, tree of the parent commit: the child process failed (%d): %s' % (out.returncode, out.stderr.strip()[-300:]))
            else:
                v = [float(t) for t in line[0].split()[1:]]
                again = in_turn(step, ('fp32',), args.reps, args.rounds)['fp32']
                say('  fp32, tree of the parent commit  %7.4f .. %7.4f ms (median %7.4f); this build again, right after: %7.4f .. %7.4f ms (median %7.4f)' % (
                    min(v), max(v), float(np.median(v)), min(again), max(again), float(np.median(again))))
        # results at the timed size: how the label maps of the three modes differ
        lab = {p: step.labels(p) for p in PRECS}
        say('  labels of the timed batch differing from fp32: bf16 %.4f %%, bf16_store %.4f %% of %d voxels' % (
            100.0 * float((lab['bf16'] != lab['fp32']).mean()), 100.0 * float((lab['bf16_store'] != lab['fp32']).mean()), lab['fp32'].size))
        # per-kernel times of the bf16_store plan (events around every launch: the launches no longer overlap their neighbours' ramps)
        eng = step.eng
        eng.set_precision('bf16_store')
        for _ in range(3):
            step()
        eng.set_timing(True)
        for _ in range(args.reps):
            step()
        torch.cuda.synchronize()
        ms, cnt = eng.kernel_times()
        eng.set_timing(False)
        say('  bf16_store plan, per kernel (mean of %d timed launches):' % args.reps)
        for name, cfg, t, c in zip(eng.kernel_names(), eng.kernel_configs(), ms, cnt):
            say('    %-18s tiling %3d  %7.1f us' % (name, cfg, 1e3 * t / max(c, 1)))
        say('    sum %7.1f us' % (1e3 * sum(t / max(c, 1) for t, c in zip(ms, cnt))))
        step.eng.close()
    for ln in summary_of_test_logs(args.test_log):
        say(ln)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
