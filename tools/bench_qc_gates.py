"""What deploy_network.py --qc_csv adds to a subject on the device path: the statistics of the quality-control gates
(device_pipeline.GateStats: ukbb_fcn_plane_components for sa and la_4ch --seg4, ukbb_fcn_label_components for the atrial
gate) on labels already in HBM, timed with HIP events after warm-up, for one full-size short-axis subject (192x208x10x50: the
10 planes of the ED frame) and one la_4ch cine (208x187x1x50), beside qc_gates.stats_host on the same labels, and the device-path
time of the whole short-axis subject (device_pipeline.segment_sequence_device, synthetic weights) with and without the gate.
GPU box only.   python tools/bench_qc_gates.py [--reps 50]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def heart_like(shape, n_class, seed):
    """Per plane concentric discs (cavity inside myocardium), further discs for the other classes, 2 % speckle."""
    rng = np.random.default_rng(seed)
    X, Y, Z, T = shape
    seg = np.zeros(shape, np.uint8)
    xx, yy = np.meshgrid(np.arange(X), np.arange(Y), indexing='ij')
    for t in range(T):
        r = 20.0 * (1 + 0.15 * np.sin(2 * np.pi * t / T))
        for z in range(Z):
            d2 = (xx - 0.45 * X) ** 2 + (yy - 0.5 * Y) ** 2
            if n_class > 2:
                seg[..., z, t][d2 <= (r + 6) ** 2] = 2
            seg[..., z, t][d2 <= r * r] = 1
            for k in range(3, n_class):
                seg[..., z, t][(xx - (0.2 + 0.15 * k) * X) ** 2 + (yy - 0.8 * Y) ** 2 <= (0.6 * r) ** 2] = k
            sp = rng.random((X, Y)) < 0.02
            seg[..., z, t][sp] = rng.integers(0, n_class, size=int(sp.sum()))
    return seg


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    args = ap.parse_args()
    import torch
    from ukbb_cardiac_amd import device_pipeline as dp
    from ukbb_cardiac_amd import qc_gates
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.engine import Engine
    from ukbb_cardiac_amd.weights import synthetic_params
    dev = torch.device('cuda', 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for what, seq, seg4, shape, n_class in (('sa subject', 'sa', False, (192, 208, 10, 50), 4),
                                            ('la_4ch --seg4 cine', 'la_4ch', True, (208, 187, 1, 50), 6),
                                            ('la_4ch cine', 'la_4ch', False, (208, 187, 1, 50), 3)):
        seg = heart_like(shape, n_class, 1)
        lab = torch.from_numpy(np.ascontiguousarray(seg.reshape(-1, order='F'))).to(dev)
        gate = dp.GateStats(seq, seg4)
        n_work, n_out = gate.sizes(shape, n_class)
        work = torch.empty(n_work, dtype=torch.int32, device=dev)
        out = torch.empty(n_out, dtype=torch.int32, device=dev)
        counts = np.stack([[int((seg[..., t] == k).sum()) for k in range(n_class)] for t in range(shape[3])])
        for _ in range(5):
            gate.launch(lab.data_ptr(), shape, n_class, work.data_ptr(), out.data_ptr(), stream)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            gate.launch(lab.data_ptr(), shape, n_class, work.data_ptr(), out.data_ptr(), stream)
        e1.record()
        torch.cuda.synchronize()
        dev_ms = e0.elapsed_time(e1) / args.reps
        got = gate.decode(out.cpu().numpy(), shape, n_class, counts)
        t0 = time.perf_counter()
        want = qc_gates.stats_host(seg, seq, seg4, n_class)
        host_ms = (time.perf_counter() - t0) * 1e3
        same = all(np.array_equal(got[k], want[k]) for k in want)
        verdict = qc_gates.gate_from_stats(got, seq, seg4, 'bench')
        print('%-20s %dx%dx%dx%d  gate statistics %.3f ms on the device (HIP events, %d reps), %d result bytes   stats_host %.1f ms   '
              'equal: %s   verdict: %s' % ((what,) + shape + (dev_ms, args.reps, 4 * n_out, host_ms, same, verdict[0])), flush=True)
    # the whole short-axis subject on the device path, with and without the gate
    arch = MODELS['FCN_sa']
    rng = np.random.default_rng(2)
    image = np.asfortranarray((1000.0 * rng.gamma(2.0, 1.0, size=(192, 208, 10, 50))).astype(np.float32))
    with Engine(arch, synthetic_params(arch, 1234), device=0) as eng:
        for qc in (None, ('sa', False), None, ('sa', False)):
            for i in range(4):
                if i == 1:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                dp.segment_sequence_device(image, eng, 128, return_aux=True, stats=[dp.GateStats(*qc)] if qc else ())
            torch.cuda.synchronize()
            print('segment_sequence_device 192x208x10x50 %-16s %.2f ms per subject (wall clock, 3 subjects after 1 warm-up)' %
                  ('with the sa gate' if qc else 'without a gate', (time.perf_counter() - t0) * 1e3 / 3), flush=True)
