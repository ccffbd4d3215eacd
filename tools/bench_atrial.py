"""What the atrial measures cost: ukbb_fcn_atrial_area_length (device_pipeline.AtrialStats) on labels already in HBM, timed
with HIP events after warm-up, for T = 50 frames of 208x176 phantom atria (both labels of la_4ch), beside atrial.frame_stats_host
and the literal atrial.area_length_reference on the same labels; then the per-subject wall time of the pipelined la_4ch deploy
loop (synthetic weights, --nosave_seg) with and without --atrial_csv.
GPU box only.   python tools/bench_atrial.py [--reps 50] [--subjects 8]"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def phantom_cine(X, Y, T, seed):
    """(X, Y, T) labels: a left and a right atrium that breathe over the cycle, with stray specks."""
    import test_atrial as TA
    seg = np.zeros((X, Y, T), np.uint8)
    for t in range(T):
        s = 1.0 + 0.12 * np.sin(2 * np.pi * t / T)
        la = TA.phantom_atrium(X, Y, seed, 1, (0.35, 0.4), 0.8 * s)
        ra = TA.phantom_atrium(X, Y, seed + 1000, 2, (0.68, 0.62), 0.7 * s)
        seg[..., t] = np.where(la != 0, la, ra)
    return seg


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--subjects', type=int, default=8)
    args = ap.parse_args()
    import torch
    import test_atrial as TA
    from ukbb_cardiac_amd import atrial, deploy_network, nifti
    from ukbb_cardiac_amd import device_pipeline as dp
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.phantom import cine_phantom
    from ukbb_cardiac_amd.weights import save_blob, synthetic_params
    dev = torch.device('cuda', 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    X, Y, T, n_class = 208, 176, 50, 3
    affine, long_axis = TA.geometry(0)
    seg = phantom_cine(X, Y, T, 3)
    shape = (X, Y, 1, T)
    lab = torch.from_numpy(np.ascontiguousarray(seg.reshape(-1, order='F'))).to(dev)
    stat = dp.AtrialStats()
    n_work, n_out = stat.sizes(shape, n_class)
    work = torch.empty(n_work, dtype=torch.int32, device=dev)
    out = torch.empty(n_out, dtype=torch.int32, device=dev)
    for _ in range(5):
        stat.launch(lab.data_ptr(), shape, n_class, work.data_ptr(), out.data_ptr(), stream, (affine, long_axis))
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.reps):
        stat.launch(lab.data_ptr(), shape, n_class, work.data_ptr(), out.data_ptr(), stream, (affine, long_axis))
    e1.record()
    torch.cuda.synchronize()
    dev_ms = e0.elapsed_time(e1) / args.reps
    got = stat.decode(out.cpu().numpy(), shape, n_class)
    t0 = time.perf_counter()
    want = atrial.frame_stats_host(seg, n_class, affine, long_axis)
    host_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    ref = [atrial.area_length_reference(seg[..., t], affine, TA.PIXDIM, long_axis) for t in range(T)]
    ref_ms = (time.perf_counter() - t0) * 1e3
    same_ref = all(TA._same(ref[t], atrial.frame_measures(got[t], affine, TA.PIXDIM)) for t in range(T))
    print('la_4ch labels %dx%dx1x%d, %d classes, mean component %d voxels: ukbb_fcn_atrial_area_length %.3f ms on the device (HIP events, '
          '%d reps), %d result bytes   frame_stats_host %.1f ms   area_length_reference %.1f ms   device == host: %s   '
          'device == reference: %s' % (X, Y, T, n_class, int(got[:, 1:, 0].mean()), dev_ms, args.reps, 4 * n_out, host_ms, ref_ms,
                                       np.array_equal(got, want), same_ref), flush=True)
    # the pipelined deploy loop of la_4ch with and without the per-frame record
    arch = MODELS['FCN_la_4ch']
    with tempfile.TemporaryDirectory() as tmp:
        mp = os.path.join(tmp, 'FCN_la_4ch')
        save_blob(mp + '.ukbbw', arch, synthetic_params(arch, 1234))
        data = os.path.join(tmp, 'data')
        pixdim_sa = np.array([1, 1.8, 1.8, 10, 0.03, 0, 0, 0], np.float32)
        for i in range(args.subjects):
            d = os.path.join(data, '%04d' % i)
            os.makedirs(d)
            cine = np.round(cine_phantom(T, X, Y, seed=i)[..., 0].reshape(T, 1, X, Y).transpose(2, 3, 1, 0) * 1000.0).astype(np.float32)
            nifti.save(cine, os.path.join(d, 'la_4ch.nii.gz'), TA.AFFINES[i % 3][0], TA.PIXDIM)
            nifti.save(np.zeros((4, 4, 2, 1), np.float32), os.path.join(d, 'sa.nii.gz'), TA.AFFINES[i % 3][1], pixdim_sa)
        base = ['--seq_name', 'la_4ch', '--data_dir', data, '--model_path', mp, '--nosave_seg']
        devnull = open(os.devnull, 'w')
        for what, extra in (('warm-up', []), ('without --atrial_csv', []), ('with --atrial_csv', ['--atrial_csv', os.path.join(tmp, 'a.csv')]),
                            ('without --atrial_csv', []), ('with --atrial_csv', ['--atrial_csv', os.path.join(tmp, 'a.csv')])):
            stdout, sys.stdout = sys.stdout, devnull
            try:
                t0 = time.perf_counter()
                deploy_network.main(base + extra)
                dt = time.perf_counter() - t0
            finally:
                sys.stdout = stdout
            if what != 'warm-up':
                print('deploy_network.py la_4ch %dx%dx1x%d pipelined, %d subjects, %-21s %.2f ms per subject (wall clock of the whole run, '
                      'engine creation included)' % (X, Y, T, args.subjects, what, dt * 1e3 / args.subjects), flush=True)
