"""Short-axis cohort of int16 files against the same cohort as float32 files, through the drop-in script end to end
(deploy_network.run: gzip NIfTI in, the five output files out).  Full-size subjects (192x208x10x50), phantom intensities
scaled into the int16 range; the float32 files hold the same values.  Three runs, each on a fresh copy of the files:

    float32            device pre-processing (subject pipeline)
    int16              device pre-processing (subject pipeline, the *_t kernels)
    int16 host         --nodevice_preproc: numpy percentile / clip / rescale / pad / transposes on the host

GPU box only.   python tools/bench_integer_cohort.py [--cohort 8] [--io_threads 8] [--only float32,int16,int16_host]
Under `rocprofv3 --kernel-trace --stats -- python tools/bench_integer_cohort.py --only float32,int16` the stats table holds
the prep kernels of both dtypes side by side (template names: sel_hist_kernel<2, float> / <2, short>, ...)."""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPE = (192, 208, 10, 50)


def subject(seed):
    from ukbb_cardiac_amd.phantom import cine_phantom
    X, Y, Z, T = SHAPE
    v = cine_phantom(Z * T, X, Y, seed=seed)[..., 0].reshape(T, Z, X, Y).transpose(2, 3, 1, 0)
    v = v / max(float(v.max()), 1e-6) * 30000.0 - 500.0              # into the int16 range, a few negative values
    return np.asfortranarray(np.clip(np.round(v), -32768, 32767).astype(np.int16))


def time_prep_kernels(reps):
    """The prep kernels of one subject, int16 beside float32 (same values), alone on one stream: median of `reps` timings of
    the exact (1, 99) percentiles (radix select + its two result copies) and of the clip / rescale / pad / transpose."""
    import torch
    from ukbb_cardiac_amd import device_pipeline as dp
    from ukbb_cardiac_amd.pipeline import pad_amounts
    X, Y, Z, T = SHAPE
    X2, Y2, x_pre, _, y_pre, _ = pad_amounts(X, Y)
    batch = torch.empty((T * Z, X2, Y2), dtype=torch.float32, device='cuda')
    v16 = subject(90)
    s = torch.cuda.current_stream()
    for v in (v16.astype(np.float32, order='F'), v16):
        t = torch.from_numpy(v).cuda()
        lo, hi = dp.device_percentiles(t, (1, 99), s.cuda_stream, v.dtype)
        times = {'select': [], 'rescale_pack': []}
        for _ in range(reps):
            e0, e1, e2 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dp.device_percentiles(t, (1, 99), s.cuda_stream, v.dtype)
            e1.record()
            dp.pack_rescaled(t.data_ptr(), v.dtype, SHAPE, t.stride(), lo, hi, (X2, Y2, x_pre, y_pre), batch.data_ptr(), s.cuda_stream)
            e2.record()
            e2.synchronize()
            times['select'].append(e0.elapsed_time(e1))
            times['rescale_pack'].append(e1.elapsed_time(e2))
        print('   %-7s  percentiles (select) %.3f ms   rescale_pack %.3f ms   (median of %d)' %
              (v.dtype, np.median(times['select']), np.median(times['rescale_pack']), reps), flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--cohort', type=int, default=8)
    ap.add_argument('--io_threads', type=int, default=8)
    ap.add_argument('--only', default='float32,int16,int16_host')
    ap.add_argument('--kernels', type=int, default=0, help='only time the prep kernels of one subject, this many repetitions')
    args = ap.parse_args()
    if args.kernels:
        print('prep kernels of one %s subject, float32 and int16:' % 'x'.join(map(str, SHAPE)), flush=True)
        time_prep_kernels(args.kernels)
        sys.exit(0)
    from ukbb_cardiac_amd import deploy_network, nifti
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.engine import Engine
    from ukbb_cardiac_amd.weights import save_blob, synthetic_params
    arch = MODELS['FCN_sa']
    params = synthetic_params(arch, 1234)
    eng = Engine(arch, params)
    root = tempfile.mkdtemp(prefix='ukbb_int_')
    try:
        mp = os.path.join(root, 'FCN_sa')
        save_blob(mp + '.ukbbw', arch, params)
        vols = [subject(90 + i) for i in range(min(args.cohort, 4))]
        for dt in ('int16', 'float32'):
            for i in range(args.cohort):
                d = os.path.join(root, 'src_' + dt, 's%03d' % i)
                os.makedirs(d)
                nifti.save(vols[i % len(vols)].astype(dt), os.path.join(d, 'sa.nii.gz'), np.diag([1.8, 1.8, 10.0, 1.0]),
                           pixdim=[1, 1.8, 1.8, 10, 0.03, 0, 0, 0])
        size = {dt: os.path.getsize(os.path.join(root, 'src_' + dt, 's000', 'sa.nii.gz')) / 1e6 for dt in ('int16', 'float32')}
        print('short-axis cohort: %d subjects of %s, sa.nii.gz %.1f MB (int16) / %.1f MB (float32), --io_threads %d' %
              (args.cohort, 'x'.join(map(str, SHAPE)), size['int16'], size['float32'], args.io_threads), flush=True)
        forward = lambda b: {'pred': eng.run(b, want_prob=False)['pred']}
        eng.run(np.zeros((1, 192, 208, 1), np.float32), want_prob=False)     # plan + workspace outside the timed runs
        rates = {}
        for mode in args.only.split(','):
            dt = mode.split('_')[0]
            work = os.path.join(root, 'run_' + mode)
            shutil.copytree(os.path.join(root, 'src_' + dt), work)
            argv = ['--seq_name', 'sa', '--data_dir', work, '--model_path', mp, '--io_threads', str(args.io_threads)]
            if mode.endswith('_host'):
                argv.append('--nodevice_preproc')
            flags = deploy_network.define_flags().parse(argv)[0]
            t0 = time.perf_counter()
            done = deploy_network.run(flags, forward, log=lambda *_: None, engine=eng)
            dt_s = time.perf_counter() - t0
            assert len(done) == args.cohort, done
            rates[mode] = args.cohort / dt_s
            print('   %-11s %6.2f s = %5.2f subjects/s, files included' % (mode, dt_s, rates[mode]), flush=True)
            shutil.rmtree(work)
        if 'int16' in rates and 'float32' in rates:
            print('   int16 / float32 = %.2f' % (rates['int16'] / rates['float32']), flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    eng.close()
