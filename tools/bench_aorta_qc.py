"""Cost of the full aortic quality control per 240x196x1x100 cine (deploy_network_ao.py --aortic_qc_full):
device_pipeline.device_qc_stats on a cine and labels already in HBM (the launches of ukbb_fcn_label_components,
ukbb_fcn_label_max, ukbb_fcn_label_compact and the two pairwise sums, with their host round trips), timed with HIP events after
warm-up, for every voxel type; and aorta_qc.stats_host on the same cine, for the record.
GPU box only.   python tools/bench_aorta_qc.py [--reps 50]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def aorta_like(X, Y, T, seed):
    """Two discs whose radii pulse over the cycle, plus 2 % speckle: the label map of a segmented aortic cine."""
    rng = np.random.default_rng(seed)
    seg = np.zeros((X, Y, 1, T), np.uint8)
    xx, yy = np.meshgrid(np.arange(X), np.arange(Y), indexing='ij')
    for t in range(T):
        for k, cx, cy, r0 in ((1, 0.4 * X, 0.45 * Y, 12.0), (2, 0.6 * X, 0.55 * Y, 9.0)):
            r = r0 * (1 + 0.15 * np.sin(2 * np.pi * t / T))
            seg[..., 0, t][(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = k
        speck = rng.random((X, Y)) < 0.02
        seg[..., 0, t][speck] = rng.integers(0, 3, size=int(speck.sum()))
    return seg


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    args = ap.parse_args()
    import torch
    from ukbb_cardiac_amd import aorta_qc
    from ukbb_cardiac_amd import device_pipeline as dp
    X, Y, T = 240, 196, 100
    dev = torch.device('cuda', 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    seg = aorta_like(X, Y, T, 1)
    lab = torch.from_numpy(np.ascontiguousarray(seg.reshape(-1, order='F'))).to(dev)
    rng = np.random.default_rng(2)
    print('aortic QC statistics per %dx%dx1x%d cine (classes 1, 2: %d and %d voxels in frame 0)' %
          (X, Y, T, int((seg[..., 0] == 1).sum()), int((seg[..., 0] == 2).sum())), flush=True)
    for dtype in (np.float32, np.uint8, np.int16, np.uint16):
        if dtype == np.float32:
            image = np.asfortranarray((1000.0 * rng.gamma(2.0, 1.0, size=seg.shape)).astype(np.float32))
        else:
            image = np.asfortranarray(rng.integers(0, min(4000, np.iinfo(dtype).max), size=seg.shape).astype(dtype))
        vol = dp._to_device(image, dev)
        for _ in range(5):
            got = dp.device_qc_stats(vol, lab, dtype, 3, stream)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            dp.device_qc_stats(vol, lab, dtype, 3, stream)
        e1.record()
        torch.cuda.synchronize()
        dev_ms = e0.elapsed_time(e1) / args.reps
        t0 = time.perf_counter()
        want = aorta_qc.stats_host(image, seg)
        host_ms = (time.perf_counter() - t0) * 1e3
        same = (np.array_equal(got['n_large'], want['n_large']) and np.array_equal(got['max'], want['max'], equal_nan=True)
                and got['mean_ed'].tobytes() == want['mean_ed'].tobytes())
        print('   %-7s device_qc_stats %.3f ms per cine (HIP events, %d reps)   stats_host %.1f ms   equal: %s' %
              (np.dtype(dtype).name, dev_ms, args.reps, host_ms, same), flush=True)
