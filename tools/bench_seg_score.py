"""What scoring a segmentation against a second one costs (deploy_network.py --score_against / --score_csv, eval_segmentation.py).

(a) one full-size subject (192x208x10xT): the engine's labels of a phantom cine ('threshold' weights) against a copy with a seeded
    fraction of its voxels redrawn -- ukbb_fcn_score_planes with both volumes in HBM and device_pipeline.ScoreStats.launch (the
    upload of the truth volume included), HIP events, median of --reps after a warm-up; seg_score.stats_host on the same pair; the
    reference's distance_metric with its literal double loop (M[i, j] = np.linalg.norm(...)) on the contour points of ONE frame,
    multiplied by the number of frames: that figure is EXTRAPOLATED.
(b) the worst case for the contour count: two uniform 4-label noise subjects of the same size (the background of every class
    connects, so nearly every labelled pixel is a contour pixel), and every second line of x against every second line of y
    (X*Y/2 contour pixels on either side of every cell): the device only, the host twin's all-pairs minima are not run on them.
(c) the cohort of tools/shard_rehearsal.py (phantom cines, 'threshold' weights, every subject with a label_sa.nii.gz) through
    deploy_network.run in this process, the two flags absent (the path of the parent commit) and present, alternating, --runs times
    each.

GPU box only.   python tools/bench_seg_score.py [--frames 50] [--cohort 256] [--unique 4] [--reps 5] [--runs 3] [--only chain|cohort]"""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def perturbed(lab, fraction, n_class, seed):
    rng = np.random.default_rng(seed)
    out = lab.copy(order='F')
    hit = rng.random(lab.shape) < fraction
    out[hit] = rng.integers(0, n_class, size=int(hit.sum()), dtype=np.uint8)
    return out


def timed(fn, reps):
    import torch
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


def device_times(pred, truth, n_class, reps):
    """(ms of ukbb_fcn_score_planes alone, ms of ScoreStats.launch with the upload, the decoded statistic)"""
    import torch
    from ukbb_cardiac_amd import _lib
    from ukbb_cardiac_amd import device_pipeline as dp
    X, Y, Z, T = pred.shape
    stream = torch.cuda.current_stream().cuda_stream
    d_pred, d_truth = (torch.from_numpy(np.ascontiguousarray(v.reshape(-1, order='F'))).cuda() for v in (pred, truth))
    stat = dp.ScoreStats()
    n_work, n_out = stat.sizes(pred.shape, n_class)
    work = torch.empty(n_work, dtype=torch.int32, device='cuda')
    out = torch.empty(n_out, dtype=torch.int32, device='cuda')
    P = Z * T
    t_kernel = timed(lambda: _lib.check(_lib.lib.ukbb_fcn_score_planes(d_pred.data_ptr(), d_truth.data_ptr(), X, Y, P, n_class, work.data_ptr(), out.data_ptr(),
                                                                       out.data_ptr() + 32 * P * n_class, stream), 'ukbb_fcn_score_planes'), reps)
    t_launch = timed(lambda: stat.launch(d_pred.data_ptr(), pred.shape, n_class, work.data_ptr(), out.data_ptr(), stream, truth), reps)
    return t_kernel, t_launch, stat.decode(out.cpu().numpy(), pred.shape, n_class), 4 * n_work, 4 * n_out


def literal_frame_seconds(pred, truth, n_class, t):
    """The reference's distance_metric on frame t, class by class, with its double loop over the two point lists (the contour
    pixels of seg_score.contour_mask: OpenCV is not a dependency)."""
    from ukbb_cardiac_amd import seg_score
    t0 = time.perf_counter()
    pairs = 0
    for k in range(1, n_class):
        for z in range(pred.shape[2]):
            a, b = pred[:, :, z, t] == k, truth[:, :, z, t] == k
            if a.sum() > 0 and b.sum() > 0:
                pts_a, pts_b = np.argwhere(seg_score.contour_mask(a)), np.argwhere(seg_score.contour_mask(b))
                M = np.zeros((len(pts_a), len(pts_b)))
                for i in range(len(pts_a)):
                    for j in range(len(pts_b)):
                        M[i, j] = np.linalg.norm(pts_a[i] - pts_b[j])
                pairs += M.size
                0.5 * (np.mean(np.min(M, axis=0)) + np.mean(np.min(M, axis=1)))
    return time.perf_counter() - t0, pairs


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=50, help='frames per subject (50: the full-size 192x208x10x50)')
    ap.add_argument('--cohort', type=int, default=256)
    ap.add_argument('--unique', type=int, default=4, help='distinct subjects; the cohort holds hard links to them')
    ap.add_argument('--fraction', type=float, default=0.01, help='voxels of the truth volume redrawn')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--only', default='')
    args = ap.parse_args()
    from ukbb_cardiac_amd import deploy_network, nifti, seg_score, sequence_run
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.engine import Engine
    from ukbb_cardiac_amd.phantom import cine_phantom
    from ukbb_cardiac_amd.subject_pipeline import SubjectPipeline
    from ukbb_cardiac_amd.weights import save_blob, threshold_params
    X, Y, Z, T = 192, 208, 10, args.frames
    arch = MODELS['FCN_sa']
    n_class = arch.n_class
    params = threshold_params(arch)
    eng = Engine(arch, params)
    root = tempfile.mkdtemp(prefix='ukbb_score_')
    try:
        t0 = time.time()
        vols = [np.asfortranarray(np.round(cine_phantom(Z * T, X, Y, seed=1000 + i)[..., 0].reshape(T, Z, X, Y).transpose(2, 3, 1, 0) * 1000.0).astype(np.float32))
                for i in range(args.unique)]
        pipe = SubjectPipeline(eng, vols[0].shape)
        labels = []
        for v in vols:
            pipe.submit(v)
            res = pipe.collect()
            labels.append(res.labels)
            res.done()
        del pipe
        truths = [perturbed(lab, args.fraction, n_class, 7 + i) for i, lab in enumerate(labels)]
        print('%d subjects of %dx%dx%dx%d made and segmented in %.1f s' % (args.unique, X, Y, Z, T, time.time() - t0), flush=True)
        if args.only in ('', 'chain'):
            pred, truth = labels[0], truths[0]
            t_kernel, t_launch, got, b_work, b_out = device_times(pred, truth, n_class, args.reps)
            defined = got['cells'][:, 1:, 0] == 1
            print('(a) labels of a phantom cine against a copy with %.1f %% of the voxels redrawn: %d of %d cells defined, contour pixels per defined '
                  'cell %.0f (pred) %.0f (truth), d_work %.1f MB, %d result bytes' %
                  (100 * args.fraction, int(defined.sum()), defined.size, got['cells'][:, 1:, 4][defined].mean(), got['cells'][:, 1:, 5][defined].mean(),
                   b_work / 1e6, b_out), flush=True)
            print('    ukbb_fcn_score_planes, both volumes in HBM %8.3f ms   ScoreStats.launch, upload of the %.1f MB truth volume included %8.3f ms   '
                  '(HIP events, median of %d)' % (t_kernel, truth.nbytes / 1e6, t_launch, args.reps), flush=True)
            t0 = time.perf_counter()
            want = seg_score.stats_host(pred, truth, n_class)
            t_host = time.perf_counter() - t0
            same = np.array_equal(got['cells'], want['cells']) and np.array_equal(got['sums'].view(np.uint64), want['sums'].view(np.uint64))
            print('    seg_score.stats_host %8.1f ms   device == host in every field and bit: %s' % (t_host * 1e3, same), flush=True)
            t_lit, pairs = literal_frame_seconds(pred, truth, n_class, 0)
            print('    distance_metric, literal double loop: frame 0 alone %.1f s (%d point pairs); x %d frames = %.0f s per subject, EXTRAPOLATED' %
                  (t_lit, pairs, T, t_lit * T), flush=True)
            print('(b) worst cases for the contour count, device only:', flush=True)
            rng = np.random.default_rng(5)
            noise = [np.asfortranarray(rng.integers(0, n_class, (X, Y, Z, T), dtype=np.uint8)) for _ in range(2)]
            lines_x = np.zeros((X, Y, Z, T), np.uint8, order='F')
            lines_x[::2] = 1
            lines_y = np.zeros((X, Y, Z, T), np.uint8, order='F')
            lines_y[:, ::2] = 1
            for what, a, b, nc in (('uniform %d-label noise against noise' % n_class, noise[0], noise[1], n_class),
                                   ('lines of x against lines of y, 2 classes', lines_x, lines_y, 2)):
                t_kernel, t_launch, got, _, _ = device_times(a, b, nc, args.reps)
                print('    %-45s contour pixels per cell %6.0f / %6.0f (plane %d)   ukbb_fcn_score_planes %8.3f ms   ScoreStats.launch %8.3f ms' %
                      (what, got['cells'][:, 1:, 4].mean(), got['cells'][:, 1:, 5].mean(), X * Y, t_kernel, t_launch), flush=True)
        if args.only in ('', 'cohort'):
            mp = os.path.join(root, 'FCN_sa')
            save_blob(mp + '.ukbbw', arch, params)
            src = os.path.join(root, 'src')
            os.makedirs(src)
            aff = np.diag([1.8269, 1.8269, 10.0, 1.0])
            pixdim = np.array([1, 1.8269, 1.8269, 10.0, 0.0305, 0, 0, 0], np.float32)
            for i, v in enumerate(vols):
                nifti.save(v, os.path.join(src, 'vol%d.nii.gz' % i), aff, pixdim)
                nifti.save(truths[i], os.path.join(src, 'label%d.nii.gz' % i), aff, pixdim)
            forward = lambda b: {'pred': eng.run(b, want_prob=False)['pred']}
            eng.run(np.zeros((1, X, Y, 1), np.float32), want_prob=False)        # plan + workspace outside the timed runs
            print('(c) %d subjects (%d distinct), threshold weights, --io_threads 8, %d alternating runs per arm:' % (args.cohort, args.unique, args.runs), flush=True)
            rates = {False: [], True: []}
            for run in range(args.runs):
                for on in (False, True):
                    work = os.path.join(root, 'run')
                    for i in range(args.cohort):           # fresh directories, the same input files (hard links)
                        d = os.path.join(work, 's%03d' % i)
                        os.makedirs(d)
                        os.link(os.path.join(src, 'vol%d.nii.gz' % (i % args.unique)), os.path.join(d, 'sa.nii.gz'))
                        os.link(os.path.join(src, 'label%d.nii.gz' % (i % args.unique)), os.path.join(d, 'label_sa.nii.gz'))
                    csv = os.path.join(root, 'score.csv')
                    flags = deploy_network.define_flags().parse(['--seq_name', 'sa', '--data_dir', work, '--model_path', mp, '--io_threads', '8'] +
                                                                (['--score_against', 'label_sa', '--score_csv', csv] if on else []))[0]
                    t0 = time.perf_counter()
                    done = deploy_network.run(flags, forward, log=lambda *_: None, engine=eng)
                    dt = time.perf_counter() - t0
                    assert len(done) == args.cohort, len(done)
                    rows = sum(1 for _ in open(csv)) - 1 if on else 0
                    rates[on].append(args.cohort / dt)
                    print('   run %d  flags %-3s  %7.2f s = %6.2f subjects/s   table rows %d   phases %s' %
                          (run, 'on' if on else 'off', dt, args.cohort / dt, rows,
                           {k: (round(v, 3) if isinstance(v, float) else v) for k, v in sequence_run.SequenceRun.last_phases.items()}), flush=True)
                    shutil.rmtree(work)
            print('   off: %s   on: %s subjects/s   every off-run above every on-run: %s' %
                  (' '.join('%.2f' % r for r in rates[False]), ' '.join('%.2f' % r for r in rates[True]), min(rates[False]) > max(rates[True])), flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    eng.close()
