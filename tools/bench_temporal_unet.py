#!/usr/bin/env python3
"""Stand-alone timing of the aortic Temporal-UNet (network_ao.py:67-114) on the HIP engine.

    python tools/bench_temporal_unet.py [--precision fp32|bf16_3d] [--frames 100] [--size 256] [--time_step 1] [--reps 3] [--json out.json]
    python tools/bench_temporal_unet.py --ab 7          fp32 and bf16_3d in turn on ONE engine build, 7 samples each (the all-runs rule)

* time per cine: ukbb_fcn_forward_cine on a [frames, size, size] cine on the device (every window runs the 3-D network),
  median of --reps after one warm-up, against the algorithmic estimate FLOP / (0.40 x the fp32 MFMA peak);
* per kernel: one chunk of windows through forward_seq with per-launch timing (Engine.set_timing): ms, algorithmic MACs,
  MACs issued to the matrix pipe (tile padding included), the issued-MFMA fraction of the precision's matrix peak at the measured clock
  (fp32: v_mfma_f32_32x32x2_f32; bf16_3d: the dense v_mfma_f32_32x32x16_bf16 rate) and the bytes of the maps the launch reads and writes
  against the HBM rate.
Synthetic weights (weights.synthetic_params); the numbers do not depend on them.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP32_MFMA_FLOP_PER_CLK = 256 * 4 * 64          # CUs x SIMDs x FLOP / clock / SIMD (v_mfma_f32_32x32x2_f32)
BF16_MFMA_FLOP_PER_CLK = 256 * 4 * 1024        # v_mfma_f32_32x32x16_bf16: 32 x 32 x 16 MACs = 32768 FLOP in 32 cycles per SIMD, 16 x the fp32 form (~2.5 PFLOP/s at 2.4 GHz)
MFMA_FLOP_PER_CLK = {'fp32': FP32_MFMA_FLOP_PER_CLK, 'bf16_3d': BF16_MFMA_FLOP_PER_CLK}
HBM_BYTES_PER_S = 6.3e12                       # MI355X HBM3E as a streaming kernel reaches it (8.0 TB/s nominal)


def ab(args):
    """fp32 and bf16_3d cines in turn on one engine: --ab samples of each, alternating; the all-runs rule (every bf16_3d sample beats every fp32 one)."""
    import torch
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.engine import Engine
    from ukbb_cardiac_amd.weights import synthetic_params
    arch = MODELS['Temporal-UNet_ao']
    eng = Engine(arch, synthetic_params(arch, 1234))
    dev = torch.device('cuda', eng.device)
    stream = torch.cuda.current_stream(dev).cuda_stream
    F, S = args.frames, args.size
    frames = torch.randn((F, S, S), dtype=torch.float32, device=dev)
    prob = torch.empty((F, S, S, arch.n_class), dtype=torch.float32, device=dev)
    pred = torch.empty((F, S, S), dtype=torch.int32, device=dev)
    times = {'fp32': [], 'bf16_3d': []}
    for i in range(args.ab + 1):                                     # round 0 warms both plans up (packing, workspace) and is dropped
        for prec in ('fp32', 'bf16_3d'):
            eng.set_precision(prec)
            eng.run_cine_device(frames.data_ptr(), F, S, S, prob.data_ptr(), pred.data_ptr(), 5, 0.1, args.time_step, stream)   # re-plans, re-reserves
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.run_cine_device(frames.data_ptr(), F, S, S, prob.data_ptr(), pred.data_ptr(), 5, 0.1, args.time_step, stream)
            torch.cuda.synchronize()
            if i:
                times[prec].append(time.perf_counter() - t0)
    eng.close()
    for prec, t in times.items():
        print('%-8s cine %d x %dx%d time_step %d: %d samples %.4f .. %.4f s, median %.4f  (%s)' % (
            prec, F, S, S, args.time_step, len(t), min(t), max(t), float(np.median(t)), ', '.join('%.4f' % v for v in t)))
    ratio = float(np.median(times['fp32'])) / float(np.median(times['bf16_3d']))
    win = max(times['bf16_3d']) < min(times['fp32'])
    print('ratio of the medians fp32 / bf16_3d %.2f; all-runs rule (every bf16_3d sample beats every fp32 sample): %s' % (ratio, 'WIN' if win else 'no win'))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump({'frames': F, 'size': S, 'time_step': args.time_step, 'times': times, 'ratio_of_medians': ratio, 'all_runs_win': win}, f, indent=1)
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--frames', type=int, default=100)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--time_step', type=int, default=1)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--seq_windows', type=int, default=10, help='windows of the per-kernel forward_seq pass')
    ap.add_argument('--json', default='')
    ap.add_argument('--precision', choices=sorted(MFMA_FLOP_PER_CLK), default='fp32')
    ap.add_argument('--ab', type=int, default=0, help='time fp32 and bf16_3d in turn on one engine, this many samples each (no per-kernel table)')
    args = ap.parse_args(argv)
    if args.ab:
        return ab(args)

    import torch
    from ukbb_cardiac_amd import _lib
    from ukbb_cardiac_amd.arch import MODELS, fcn_macs_per_slice
    from ukbb_cardiac_amd.engine import Engine, plan_layout
    from ukbb_cardiac_amd.weights import synthetic_params

    arch = MODELS['Temporal-UNet_ao']
    eng = Engine(arch, synthetic_params(arch, 1234))
    eng.set_precision(args.precision)
    flop_per_clk = MFMA_FLOP_PER_CLK[args.precision]
    dev = torch.device('cuda', eng.device)
    stream = torch.cuda.current_stream(dev).cuda_stream
    F, S, T = args.frames, args.size, arch.fc
    frames = torch.randn((F, S, S), dtype=torch.float32, device=dev)
    prob = torch.empty((F, S, S, arch.n_class), dtype=torch.float32, device=dev)
    pred = torch.empty((F, S, S), dtype=torch.int32, device=dev)

    def cine():
        eng.run_cine_device(frames.data_ptr(), F, S, S, prob.data_ptr(), pred.data_ptr(), 5, 0.1, args.time_step, stream)

    cine()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        cine()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    mhz = _lib.clock_probe_mhz(eng.device)
    t_cine = float(np.median(times))
    windows = (F + args.time_step - 1) // args.time_step
    m3, m1 = fcn_macs_per_slice(arch, S, S)
    flop = 2.0 * (m3 + m1) * windows * T
    peak_nominal = flop_per_clk * 2400e6
    estimate = flop / (0.40 * peak_nominal)
    print('cine %d x %dx%d, time_step %d: %d windows, %.3f TFLOP; %.4f s per cine (median of %d: %s); estimate at 0.40 of '
          'the %s MFMA peak %.4f s -> ratio %.2f; %.1f TFLOP/s; shader clock %.0f MHz'
          % (F, S, S, args.time_step, windows, flop / 1e12, t_cine, args.reps, ', '.join('%.4f' % t for t in times),
             args.precision, estimate, t_cine / estimate, flop / t_cine / 1e12, mhz))

    # per kernel: one forward_seq of seq_windows windows, every launch timed
    n = args.seq_windows
    x = torch.randn((n, T, S, S), dtype=torch.float32, device=dev)
    import ctypes as C

    def seq():
        _lib.check(_lib.lib.ukbb_fcn_forward_seq(eng._h, C.c_void_p(x.data_ptr()), n, S, S, None, C.c_void_p(prob.data_ptr()) if n * T <= F else None,
                                                 None, C.c_void_p(stream)), 'ukbb_fcn_forward_seq')
    seq()
    torch.cuda.synchronize()
    eng.set_timing(True)
    for _ in range(args.reps):
        seq()
    ms, cnt = eng.kernel_times()
    eng.set_timing(False)
    peak_clk = flop_per_clk * mhz * 1e6
    # bytes of the maps a launch reads and writes (weights, the fp32 image and the fp32 outputs of the logits launch not counted)
    plan = plan_layout(arch, args.precision, n * T, S, S)
    act_bytes = [a['per_image'] * a['bytes_per_element'] * n * T for a in plan['acts']]
    io_bytes = {o['name']: sum(act_bytes[i] for i in (o['in0'], o['in1'], o['out']) if i >= 0) for o in plan['ops']}
    rows = []
    tot_ms = tot_issued = 0.0
    print('%-8s %9s %10s %10s %7s %9s %7s' % ('kernel', 'ms', 'GMAC', 'issued', 'mfma%', 'map MB', 'hbm%'))
    for name, t, c, macs, issued in zip(eng.kernel_names(), ms, cnt, eng.kernel_macs(), eng.kernel_mfma_macs_issued()):
        t = t / max(c, 1)
        frac = 2.0 * issued / (t * 1e-3) / peak_clk if t > 0 else 0.0
        hbm = io_bytes[name] / (t * 1e-3) / HBM_BYTES_PER_S if t > 0 else 0.0
        rows.append({'kernel': name, 'ms': t, 'gmac': macs / 1e9, 'gmac_issued': issued / 1e9, 'mfma_fraction': frac, 'map_bytes': io_bytes[name], 'hbm_fraction': hbm})
        tot_ms += t
        tot_issued += issued
        print('%-8s %9.3f %10.2f %10.2f %6.1f%% %9.1f %6.1f%%' % (name, t, macs / 1e9, issued / 1e9, 100 * frac, io_bytes[name] / 1e6, 100 * hbm))
    print('forward_seq of %d windows: %.3f ms, issued-MFMA fraction %.3f of the %s peak at %.0f MHz'
          % (n, tot_ms, 2.0 * tot_issued / (tot_ms * 1e-3) / peak_clk, args.precision, mhz))
    res = {'precision': args.precision, 'frames': F, 'size': S, 'time_step': args.time_step, 'windows': windows, 'tflop_per_cine': flop / 1e12,
           's_per_cine': t_cine, 'times': times, 'estimate_s': estimate, 'ratio_to_estimate': t_cine / estimate,
           'shader_mhz': mhz, 'seq_windows': n, 'kernels': rows}
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(res, f, indent=1)
    eng.close()
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
