"""What --confidence_csv costs the network: the forward at the headline shape (64 x 192 x 208, FCN_sa, fp32) three ways -- labels only (what
every run without the flag issues), labels and probabilities (the head also stores 4 float32 per voxel), and the same with
ukbb_fcn_confidence_cells queued behind it -- alternating, medians of --rounds samples of --reps steps each, device events; the first
again from a built tree of the parent commit (--parent_root, a fresh process that imports that tree's package and library); the new kernel alone on those
probabilities and on synthetic ones for the other class counts; and the HBM rate a plain device copy reaches in the same process, the
yardstick for the byte arithmetic printed next to every figure.

GPU box only.   python tools/bench_confidence.py [--batch 64] [--height 192] [--width 208] [--reps 50] [--rounds 7] [--parent_root DIR] [--out FILE]"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.environ.get('UKBB_BENCH_ROOT') or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))   # the child of --parent_root: that tree
sys.path.insert(0, ROOT)


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


def alternating(variants, reps, rounds):
    """{name: median ms per call}, the variants taken in turn ``rounds`` times after one warm-up turn."""
    got = {name: [] for name, _ in variants}
    for r in range(rounds + 1):
        for name, fn in variants:
            ms = timed(fn, reps)
            if r:
                got[name].append(ms)
    return {name: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for name, v in got.items()}


def hbm_rate(reps):
    """TB/s of a 1 GiB device-to-device copy (bytes read + bytes written)."""
    import torch
    src = torch.empty(1 << 28, dtype=torch.float32, device='cuda').normal_()
    dst = torch.empty_like(src)
    timed(lambda: dst.copy_(src), 3)
    ms = float(np.median([timed(lambda: dst.copy_(src), reps) for _ in range(5)]))
    return 2 * src.numel() * 4 / (ms * 1e-3) / 1e12


def forward_variants(args):
    import torch
    from ukbb_cardiac_amd import _lib
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.engine import Engine
    from ukbb_cardiac_amd.phantom import cine_phantom
    from ukbb_cardiac_amd.weights import synthetic_params
    arch = MODELS['FCN_sa']
    n, H, W, C = args.batch, args.height, args.width, arch.n_class
    Z = 10                                               # slices per frame of a short-axis subject: the launch adds into ceil(n / Z) frames
    eng = Engine(arch, synthetic_params(arch, 1234), device=0)
    stream = torch.cuda.current_stream().cuda_stream
    x = torch.from_numpy(cine_phantom(n, H, W, seed=3)).cuda()
    pred = torch.empty((n, H, W), dtype=torch.int32, device='cuda')
    prob = torch.empty((n, H, W, C), dtype=torch.float32, device='cuda')
    cells = torch.zeros((-(-n // Z), C, 20), dtype=torch.int64, device='cuda')

    def base():
        eng.run_device(x.data_ptr(), n, H, W, pred_ptr=pred.data_ptr(), stream=stream)

    def with_prob():
        eng.run_device(x.data_ptr(), n, H, W, prob_ptr=prob.data_ptr(), pred_ptr=pred.data_ptr(), stream=stream)

    def kernel():
        _lib.check(_lib.lib.ukbb_fcn_confidence_cells(prob.data_ptr(), pred.data_ptr(), n, H, W, Z, -(-n // Z), H, W, 0, 0, C, 0, cells.data_ptr(), stream),
                   'ukbb_fcn_confidence_cells')

    def with_cells():
        with_prob()
        kernel()
    return eng, dict(base=base, with_prob=with_prob, with_cells=with_cells, kernel=kernel), (prob, pred, cells)


def kernel_alone(n, H, W, C, reps, prob=None, pred=None):
    """(ms, GB read) of ukbb_fcn_confidence_cells on [n, H, W, C] probabilities: those given, or seeded softmax values."""
    import torch
    from ukbb_cardiac_amd import _lib
    stream = torch.cuda.current_stream().cuda_stream
    if prob is None:
        g = torch.Generator(device='cuda').manual_seed(C)
        prob = torch.softmax(3.0 * torch.randn((n, H, W, C), device='cuda', generator=g), dim=-1).contiguous()
        pred = prob.argmax(dim=-1).to(torch.int32)
    Z, T = 10, -(-n // 10)
    cells = torch.zeros((T, C, 20), dtype=torch.int64, device='cuda')

    def call():
        _lib.check(_lib.lib.ukbb_fcn_confidence_cells(prob.data_ptr(), pred.data_ptr(), n, H, W, Z, T, H, W, 0, 0, C, 0, cells.data_ptr(), stream),
                   'ukbb_fcn_confidence_cells')
    timed(call, 20)
    ms = float(np.median([timed(call, reps) for _ in range(5)]))
    return ms, n * H * W * (4 * C + 4) / 1e9


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--height', type=int, default=192)
    ap.add_argument('--width', type=int, default=208)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--parent_root', default='', help='a built tree of the parent commit: the labels-only forward is timed from it in a fresh process')
    ap.add_argument('--out', default='', help='also write the report here')
    ap.add_argument('--only_base', action='store_true', help='(the child process) time the labels-only forward and print its ms')
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_confidence: needs a GPU')
    eng, fn, (prob, pred, _) = forward_variants(args)
    n, H, W = args.batch, args.height, args.width
    if args.only_base:
        ms = alternating([('base', fn['base'])], args.reps, args.rounds)['base']
        print('BASE_MS %.6f %.6f %.6f' % ms)
        return
    lines = []

    def say(text=''):
        print(text, flush=True)
        lines.append(text)
    C = eng.arch.n_class
    say('bench_confidence: FCN_sa fp32, batch %d x %d x %d, %d classes; %d steps per sample, median (min .. max) of %d samples, alternating' % (n, H, W, C, args.reps, args.rounds))
    tb = hbm_rate(20)
    say('HBM rate of a 1 GiB device copy (read + written bytes): %.2f TB/s' % tb)
    res = alternating([(k, fn[k]) for k in ('base', 'with_prob', 'with_cells')], args.reps, args.rounds)
    store, read = n * H * W * 4 * C / 1e6, n * H * W * (4 * C + 4) / 1e6
    for key, what in (('base', 'labels only (no flag)'), ('with_prob', 'labels + probabilities'), ('with_cells', 'labels + probabilities + confidence cells')):
        med, lo, hi = res[key]
        say('  %-44s %8.4f ms (%.4f .. %.4f)  %8.0f slices/s  %+6.2f %% against labels only' % (what, med, lo, hi, n / (med * 1e-3), 100.0 * (med / res['base'][0] - 1.0)))
    say('  byte arithmetic: the head writes %.1f MB more (%.1f us at the copy rate), the new kernel reads %.1f MB (%.1f us): %.2f %% of the labels-only step'
        % (store, store / tb, read, read / tb, 100.0 * (store + read) / tb * 1e-3 / res['base'][0]))
    say('  measured: probabilities %+.1f us, cells %+.1f us' % (1e3 * (res['with_prob'][0] - res['base'][0]), 1e3 * (res['with_cells'][0] - res['with_prob'][0])))
    if args.parent_root:
        env = dict(os.environ, UKBB_BENCH_ROOT=os.path.abspath(args.parent_root))
        cmd = [sys.executable, os.path.abspath(__file__), '--only_base', '--batch', str(n), '--height', str(H), '--width', str(W), '--reps', str(args.reps),
               '--rounds', str(args.rounds)]
        out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        got = [l for l in out.stdout.splitlines() if l.startswith('BASE_MS')]
        if out.returncode or not got:
            say('  parent commit: the child process failed (%d): %s' % (out.returncode, out.stderr.strip()[-300:]))
        else:
            med, lo, hi = (float(v) for v in got[0].split()[1:])
            again = alternating([('base', fn['base'])], args.reps, args.rounds)['base']
            say('  labels only, tree of the parent commit         %8.4f ms (%.4f .. %.4f)  %8.0f slices/s; this build again, right after: %.4f ms' % (med, lo, hi, n / (med * 1e-3), again[0]))
    say('the new kernel alone (median of 5 samples of %d launches):' % args.reps)
    ms, gb = kernel_alone(n, H, W, C, args.reps, prob, pred)
    say('  %d classes, the probabilities of the forward      %8.2f us  %6.1f MB  %5.2f TB/s  (%.0f %% of the copy rate)' % (C, ms * 1e3, gb * 1e3, gb / ms, 100.0 * gb / ms / tb))
    for c in (2, 3, 4, 6):
        ms, gb = kernel_alone(n, H, W, c, args.reps)
        say('  %d classes, seeded softmax values                 %8.2f us  %6.1f MB  %5.2f TB/s  (%.0f %% of the copy rate)' % (c, ms * 1e3, gb * 1e3, gb / ms, 100.0 * gb / ms / tb))
    big = 8 * n                                            # beyond the 256 MiB on-die cache: the rate from HBM itself
    ms, gb = kernel_alone(big, H, W, 4, max(5, args.reps // 5))
    say('  4 classes, %d slices (%.0f MB, past the on-die cache) %8.2f us  %5.2f TB/s  (%.0f %% of the copy rate)' % (big, gb * 1e3, ms * 1e3, gb / ms, 100.0 * gb / ms / tb))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
