"""Inflate of gzip NIfTI cines on the GPU (deploy_network.py --device_inflate K) against the host readers.

1. kernel alone: K = 1, 16, 64, 256 copies of one sa.nii.gz (int16 and float32, the subjects of tools/bench_integer_cohort.py) in one
   ukbb_fcn_inflate_device launch, without and with the CRC launch: HIP events, median of --reps launches after a warm-up;
2. end to end: a cohort of --cohort subjects through deploy_network.run with --device_inflate 64 and 256 against --device_inflate 0
   (SequenceRun.pipelined, the host readers) on the same files, alternating, --runs times each;
3. where a round's time goes (sequence_run.SequenceRun.last_phases of the last run of each K).

GPU box only.   python tools/bench_device_inflate.py [--frames 50] [--cohort 256] [--io_threads 8] [--reps 5] [--runs 3] [--skip kernel|e2e] [--once]"""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_integer_cohort as bic                           # noqa: E402


def kernel_alone(blob, label, reps, Ks=(1, 16, 64, 256), warmup=1, crc_too=True):
    import torch
    from ukbb_cardiac_amd import _lib
    from ukbb_cardiac_amd.device_inflate import gzip_member_layout, plan_subject
    plan = plan_subject(blob)
    off, ln, crc, _ = gzip_member_layout(blob, plan.total)
    print(' %s: sa.nii.gz %.1f MB -> %.1f MB' % (label, len(blob) / 1e6, plan.total / 1e6), flush=True)
    stream = torch.cuda.current_stream().cuda_stream
    for K in Ks:
        src_stride, dst_stride = (ln + 15) & ~15, (plan.total + 15) & ~15
        src = torch.from_numpy(np.frombuffer(blob, np.uint8, ln, off).copy()).cuda()
        d_src = torch.empty(K * src_stride, dtype=torch.uint8, device='cuda')
        for k in range(K):
            d_src[k * src_stride:k * src_stride + ln] = src
        d_dst = torch.empty(K * dst_stride, dtype=torch.uint8, device='cuda')
        d_w = torch.empty(K, dtype=torch.int64, device='cuda')
        d_c = torch.empty(K, dtype=torch.int32, device='cuda')
        tab = (_lib.GzStream * K)()
        for k in range(K):
            tab[k].src_off, tab[k].src_len, tab[k].dst_off, tab[k].dst_cap = k * src_stride, ln, k * dst_stride, plan.total
        ms = {}
        for with_crc in ((False, True) if crc_too else (True,)):
            times = []
            for r in range(reps + warmup):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _lib.check(_lib.lib.ukbb_fcn_inflate_device(d_src.data_ptr(), d_dst.data_ptr(), tab, K, d_w.data_ptr(),
                                                            d_c.data_ptr() if with_crc else None, stream), 'ukbb_fcn_inflate_device')
                e1.record()
                e1.synchronize()
                if r >= warmup:
                    times.append(e0.elapsed_time(e1))
            ms[with_crc] = float(np.median(times))
        assert (d_w.cpu().numpy() == plan.total).all() and (d_c.cpu().numpy().view(np.uint32) == crc).all()
        t = ms[not crc_too] / 1e3
        if crc_too:
            print('   K = %3d   inflate %9.1f ms   + CRC %7.2f ms   %6.2f MB/s per stream   %8.1f MB/s in all   (median of %d)' %
                  (K, ms[False], ms[True] - ms[False], plan.total / 1e6 / t, K * plan.total / 1e6 / t, reps), flush=True)
        else:
            print('   K = %3d   inflate + CRC %9.1f ms   %6.2f MB/s per stream   %8.1f MB/s in all   (%d launch%s, no warm-up)' %
                  (K, ms[True], plan.total / 1e6 / t, K * plan.total / 1e6 / t, reps, '' if reps == 1 else 'es'), flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=50, help='frames per subject (50: the full-size 192x208x10x50)')
    ap.add_argument('--cohort', type=int, default=256)
    ap.add_argument('--io_threads', type=int, default=8)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--skip', default='')
    ap.add_argument('--once', action='store_true', help='kernel alone: one launch of K = 1 and of K = 256 per dtype, no warm-up (a full-size launch takes 10-15 s)')
    args = ap.parse_args()
    from ukbb_cardiac_amd import deploy_network, nifti, sequence_run
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.engine import Engine
    from ukbb_cardiac_amd.weights import save_blob, synthetic_params
    bic.SHAPE = bic.SHAPE[:3] + (args.frames,)
    arch = MODELS['FCN_sa']
    params = synthetic_params(arch, 1234)
    eng = Engine(arch, params)
    root = tempfile.mkdtemp(prefix='ukbb_inflate_')
    try:
        mp = os.path.join(root, 'FCN_sa')
        save_blob(mp + '.ukbbw', arch, params)
        t0 = time.time()
        vols = [bic.subject(90 + i) for i in range(4)]
        files = []
        for i, v in enumerate(vols):
            p = os.path.join(root, 'vol%d.nii.gz' % i)
            nifti.save(v, p, np.diag([1.8, 1.8, 10.0, 1.0]), pixdim=[1, 1.8, 1.8, 10, 0.03, 0, 0, 0])
            files.append(p)
        p32 = os.path.join(root, 'vol_f32.nii.gz')
        nifti.save(vols[0].astype(np.float32), p32, np.diag([1.8, 1.8, 10.0, 1.0]), pixdim=[1, 1.8, 1.8, 10, 0.03, 0, 0, 0])
        print('subjects of %s made in %.1f s' % ('x'.join(map(str, bic.SHAPE)), time.time() - t0), flush=True)
        if 'kernel' not in args.skip:
            print('1. kernel alone (LDS 56 368 B per workgroup of one wave, 2 workgroups per CU):', flush=True)
            kw = dict(Ks=(1, 256), warmup=0, crc_too=False) if args.once else {}
            kernel_alone(open(files[0], 'rb').read(), 'int16', 1 if args.once else args.reps, **kw)
            kernel_alone(open(p32, 'rb').read(), 'float32', 1 if args.once else args.reps, **kw)
        if 'e2e' not in args.skip:
            src = os.path.join(root, 'src')
            for i in range(args.cohort):
                d = os.path.join(src, 's%03d' % i)
                os.makedirs(d)
                shutil.copyfile(files[i % len(files)], os.path.join(d, 'sa.nii.gz'))
            print('2. end to end: %d int16 subjects, sa.nii.gz %.1f MB, --io_threads %d, %d alternating runs per arm' %
                  (args.cohort, os.path.getsize(files[0]) / 1e6, args.io_threads, args.runs), flush=True)
            forward = lambda b: {'pred': eng.run(b, want_prob=False)['pred']}
            eng.run(np.zeros((1, 192, 208, 1), np.float32), want_prob=False)     # plan + workspace outside the timed runs
            rates, phases = {}, {}
            for run in range(args.runs):
                for K in (0, 64, 256):
                    work = os.path.join(root, 'run')
                    for i in range(args.cohort):               # fresh directories, the same input files (hard links)
                        d = os.path.join(work, 's%03d' % i)
                        os.makedirs(d)
                        os.link(os.path.join(src, 's%03d' % i, 'sa.nii.gz'), os.path.join(d, 'sa.nii.gz'))
                    flags = deploy_network.define_flags().parse(['--seq_name', 'sa', '--data_dir', work, '--model_path', mp, '--io_threads',
                                                                 str(args.io_threads), '--device_inflate', str(K)])[0]
                    t0 = time.perf_counter()
                    done = deploy_network.run(flags, forward, log=lambda *_: None, engine=eng)
                    dt = time.perf_counter() - t0
                    assert len(done) == args.cohort, len(done)
                    rates.setdefault(K, []).append(args.cohort / dt)
                    if K:
                        phases[K] = dict(sequence_run.SequenceRun.last_phases, total=dt)
                    print('   run %d  --device_inflate %3d  %7.2f s = %6.2f subjects/s' % (run, K, dt, args.cohort / dt), flush=True)
                    shutil.rmtree(work)
            base = float(np.median(rates[0]))
            for K in (0, 64, 256):
                m = float(np.median(rates[K]))
                print('   --device_inflate %3d: median %6.2f subjects/s   ratio to the host readers %.2f' % (K, m, m / base), flush=True)
            print('3. where a run\'s time goes (seconds of the GPU thread, last run of each K):', flush=True)
            for K, ph in phases.items():
                print('   K = %3d  ' % K + '  '.join('%s %.2f' % kv for kv in ph.items()), flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    eng.close()
