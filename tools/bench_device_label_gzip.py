"""Deflate of label volumes on the GPU (deploy_network.py --device_label_gzip) against the host writer.

(a) one full-size subject (192x208x10xT): the device chain ukbb_fcn_gzip_labels_device on phantom-like labels (the engine's, 'threshold'
    weights) and on noise labels, HIP events around the whole chain, median of --reps after a warm-up, and the bytes it sends to the
    host; against ukbb_fcn_gzip_labels_mode on one core and the pinned D2H copy of the label volume.  Per-launch times: run this
    part under `rocprofv3 --kernel-trace --stats -- python tools/bench_device_label_gzip.py --only chain`.
(b) the cohort of tools/shard_rehearsal.py (phantom cines, 'threshold' weights) through deploy_network.run in this process, flag off
    (the host writer) and on, alternating, --runs times each, with SequenceRun.phases of every run; --io_threads 8
(c) the same with --io_threads 4.

GPU box only.   python tools/bench_device_label_gzip.py [--frames 50] [--cohort 256] [--unique 4] [--reps 5] [--runs 3] [--only chain|cohort]"""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def chain(lab, label, mode, reps):
    import torch
    from ukbb_cardiac_amd import _lib, nifti
    from ukbb_cardiac_amd.subject_pipeline import label_gzip_capacity, label_gzip_max_runs
    lib = _lib.lib
    flat = np.ascontiguousarray(lab.reshape(-1, order='F'))
    n = flat.size
    prefix = nifti.header_prefix(lab.shape, np.diag([1.8, 1.8, 10.0, 1.0]), None, np.float64)
    cap, max_runs = label_gzip_capacity(n), label_gzip_max_runs(n)
    d_lab = torch.from_numpy(flat).cuda()
    d_pre = torch.from_numpy(np.frombuffer(prefix, np.uint8).copy()).cuda()
    d_out = torch.empty((cap + 3) & ~3, dtype=torch.uint8, device='cuda')
    d_scr = torch.empty(int(lib.ukbb_fcn_gzip_labels_device_scratch(n, max_runs)), dtype=torch.uint8, device='cuda')
    d_len = torch.zeros(1, dtype=torch.int64, device='cuda')
    pin_lab = torch.empty(n, dtype=torch.uint8, pin_memory=True)
    pin_out = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
    stream = torch.cuda.current_stream().cuda_stream

    def timed(fn):
        ms = []
        for r in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r:
                ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))

    t_chain = timed(lambda: _lib.check(lib.ukbb_fcn_gzip_labels_device(d_lab.data_ptr(), n, 64, d_pre.data_ptr(), len(prefix), mode, d_out.data_ptr(), cap,
                                                                       d_scr.data_ptr(), max_runs, d_len.data_ptr(), stream), 'ukbb_fcn_gzip_labels_device'))
    got = int(d_len.item())
    t_d2h_lab = timed(lambda: pin_lab.copy_(d_lab, non_blocking=True))
    t_d2h_out = timed(lambda: pin_out.copy_(d_out[:cap], non_blocking=True))
    out = np.empty(int(lib.ukbb_fcn_gzip_labels_bound(n, 64, len(prefix))), np.uint8)
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        want = lib.ukbb_fcn_gzip_labels_mode(flat.ctypes.data, n, 64, prefix, len(prefix), out.ctypes.data, out.size, mode)
        host.append((time.perf_counter() - t0) * 1e3)
    runs = int(1 + np.count_nonzero(flat[1:] != flat[:-1]))
    same = got == want and bytes(pin_out.numpy()[:got]) == bytes(out[:want]) if got > 0 else None
    print('   %-8s %-5s  runs %8d (table %8d)  member %9d B (capacity %8d)  d_len %9d  equal bytes: %s' %
          (label, 'fixed' if mode == 0 else 'small', runs, max_runs, want, cap, got, same), flush=True)
    print('      device chain %7.3f ms   D2H of the member at capacity %6.3f ms (%d B + 8)   |   host writer, one core %7.1f ms   D2H of the %d B label volume %6.3f ms' %
          (t_chain, t_d2h_out, cap, float(np.median(host)), n, t_d2h_lab), flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=50, help='frames per subject (50: the full-size 192x208x10x50)')
    ap.add_argument('--cohort', type=int, default=256)
    ap.add_argument('--unique', type=int, default=4, help='distinct subjects; the cohort holds hard links to them')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--only', default='')
    args = ap.parse_args()
    from ukbb_cardiac_amd import deploy_network, nifti, sequence_run
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.engine import Engine
    from ukbb_cardiac_amd.phantom import cine_phantom
    from ukbb_cardiac_amd.subject_pipeline import SubjectPipeline
    from ukbb_cardiac_amd.weights import save_blob, threshold_params
    X, Y, Z, T = 192, 208, 10, args.frames
    arch = MODELS['FCN_sa']
    params = threshold_params(arch)
    eng = Engine(arch, params)
    root = tempfile.mkdtemp(prefix='ukbb_labelgz_')
    try:
        t0 = time.time()
        vols = [np.asfortranarray(np.round(cine_phantom(Z * T, X, Y, seed=1000 + i)[..., 0].reshape(T, Z, X, Y).transpose(2, 3, 1, 0) * 1000.0).astype(np.float32))
                for i in range(args.unique)]
        print('%d subjects of %dx%dx%dx%d made in %.1f s' % (args.unique, X, Y, Z, T, time.time() - t0), flush=True)
        if args.only in ('', 'chain'):
            pipe = SubjectPipeline(eng, vols[0].shape)
            pipe.submit(vols[0])
            res = pipe.collect()
            phantom_like = res.labels
            res.done()
            del pipe
            noise = np.asfortranarray(np.random.default_rng(1).integers(0, 4, (X, Y, Z, T)).astype(np.uint8))
            print('(a) one subject, float64 label file of %.1f MB raw:' % (X * Y * Z * T * 8 / 1e6), flush=True)
            for label, lab in (('phantom', phantom_like), ('noise', noise)):
                for mode in (1, 0):
                    chain(lab, label, mode, args.reps)
        if args.only in ('', 'cohort'):
            mp = os.path.join(root, 'FCN_sa')
            save_blob(mp + '.ukbbw', arch, params)
            src = os.path.join(root, 'src')
            os.makedirs(src)
            aff = np.diag([1.8269, 1.8269, 10.0, 1.0])
            pixdim = np.array([1, 1.8269, 1.8269, 10.0, 0.0305, 0, 0, 0], np.float32)
            for i, v in enumerate(vols):
                nifti.save(v, os.path.join(src, 'vol%d.nii.gz' % i), aff, pixdim)
            forward = lambda b: {'pred': eng.run(b, want_prob=False)['pred']}
            eng.run(np.zeros((1, X, Y, 1), np.float32), want_prob=False)        # plan + workspace outside the timed runs
            for part, io in (('(b)', 8), ('(c)', 4)):
                print('%s %d subjects (%d distinct), threshold weights, --io_threads %d, %d alternating runs per arm:' % (part, args.cohort, args.unique, io, args.runs), flush=True)
                rates = {False: [], True: []}
                for run in range(args.runs):
                    for on in (False, True):
                        work = os.path.join(root, 'run')
                        for i in range(args.cohort):           # fresh directories, the same input files (hard links)
                            d = os.path.join(work, 's%03d' % i)
                            os.makedirs(d)
                            os.link(os.path.join(src, 'vol%d.nii.gz' % (i % args.unique)), os.path.join(d, 'sa.nii.gz'))
                        flags = deploy_network.define_flags().parse(['--seq_name', 'sa', '--data_dir', work, '--model_path', mp, '--io_threads', str(io)] +
                                                                    (['--device_label_gzip'] if on else []))[0]
                        t0 = time.perf_counter()
                        done = deploy_network.run(flags, forward, log=lambda *_: None, engine=eng)
                        dt = time.perf_counter() - t0
                        assert len(done) == args.cohort, len(done)
                        rates[on].append(args.cohort / dt)
                        print('   run %d  flag %-3s  %7.2f s = %6.2f subjects/s   phases %s' %
                              (run, 'on' if on else 'off', dt, args.cohort / dt,
                               {k: (round(v, 3) if isinstance(v, float) else v) for k, v in sequence_run.SequenceRun.last_phases.items()}), flush=True)
                        shutil.rmtree(work)
                print('   off: %s   on: %s subjects/s   every on-run above every off-run: %s' %
                      (' '.join('%.2f' % r for r in rates[False]), ' '.join('%.2f' % r for r in rates[True]), min(rates[True]) > max(rates[False])), flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    eng.close()
