#!/usr/bin/env python3
"""Score label volumes against a second set of label volumes: for every subject under ``--data_dir`` that has
``<seg_name>.nii.gz`` and ``<truth_name>.nii.gz``, one row per (subject, annotated frame, label) with the Dice overlap, the mean
contour distance and the Hausdorff distance (mm) -- the table ``deploy_network.py --score_against ... --score_csv ...`` writes, from
two files per subject::

    python -m ukbb_cardiac_amd.eval_segmentation --data_dir DIR --seg_name seg_sa --truth_name label_sa --output_csv FILE

Works for any pair of label files of one shape (seg_ao / label_ao, the long-axis names); 3-D files count as one frame.  The number
of classes is the largest label of the pair + 1 (``--n_class``: at least that many, for the rows of a class neither file holds).  The arithmetic is ukbb_cardiac_amd/seg_score.py (np_categorical_dice and
distance_metric of the reference's common/image_utils.py); the label maps go to the GPU as uint8 and ukbb_fcn_score_planes
computes the statistics there; ``--host`` computes the same integers and sums in numpy (seg_score.stats_host), as does a subject
whose planes the device form does not hold."""
import argparse
import os
import sys

import numpy as np

if __package__ in (None, ''):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ukbb_cardiac_amd import nifti, seg_score   # noqa: E402


def pair_stats(seg, truth, n_class, host=False, log=print):
    """seg_score.stats_host of two uint8 (X,Y,Z,T) volumes: on the device, or in numpy with ``host``."""
    if not host:
        import torch
        from ukbb_cardiac_amd import device_pipeline as dp
        if not torch.cuda.is_available():
            raise RuntimeError('no GPU: the scores are computed on the device (--host computes them in numpy)')
        if dp.ScoreStats.fits(seg.shape, n_class):
            lab = torch.from_numpy(np.ascontiguousarray(seg.reshape(-1, order='F'))).cuda()
            return dp.label_statistics(lab, seg.shape, n_class, [dp.ScoreStats()], {'score': truth}, torch.cuda.current_stream().cuda_stream)['score']
        log('  {0} x {1} planes are larger than the device scores: scored on the host.'.format(*seg.shape[:2]))
    return seg_score.stats_host(seg, truth, n_class)


def rows_from_files(data_path, seg_name, truth_name, host=False, log=print, min_classes=2):
    """[(subject, [seg_score.SCORE_COLUMNS values])] of the subjects that have both files, in sorted order."""
    table = []
    for data in sorted(os.listdir(data_path)):
        data_dir = os.path.join(data_path, data)
        names = ['{0}/{1}.nii.gz'.format(data_dir, n) for n in (seg_name, truth_name)]
        if not all(os.path.exists(n) for n in names):
            continue
        log(data)
        nim = nifti.load(names[0])
        seg, truth = nim.get_data(), nifti.load(names[1]).get_data()
        if seg.ndim == 3 and truth.ndim == 3:
            seg, truth = seg[..., None], truth[..., None]
        if seg.ndim != 4:
            log('  {0}: expected a 3-D or 4-D label volume, found shape {1}. Skip.'.format(names[0], seg.shape))
            continue
        try:
            n_class = max(2, min_classes, int(max(seg.max(), truth.max())) + 1)
            if n_class > seg_score.MAX_CLASSES:
                raise ValueError('label %d: label maps of at most %d classes are scored' % (n_class - 1, seg_score.MAX_CLASSES))
            seg = seg_score.check_truth(seg, seg.shape, n_class)
            truth = seg_score.check_truth(truth, seg.shape, n_class)
        except ValueError as e:
            log('  {0} and {1} cannot be scored: {2}. Skip.'.format(names[0], names[1], e))
            continue
        table += [(data, r) for r in seg_score.frame_rows(pair_stats(seg, truth, n_class, host, log), nim.header['pixdim'])]
    return table


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--data_dir', metavar='dir_name', required=True)
    parser.add_argument('--seg_name', metavar='stem', default='seg_sa', help='the segmentation to score, <subject>/<stem>.nii.gz')
    parser.add_argument('--truth_name', metavar='stem', default='label_sa', help='the label file to score it against')
    parser.add_argument('--output_csv', metavar='csv_name', required=True)
    parser.add_argument('--host', action='store_true', help='compute the statistics in numpy instead of on the GPU')
    parser.add_argument('--n_class', type=int, default=2, help='score at least this many classes (default: the largest label of the pair + 1)')
    args = parser.parse_args(argv)
    seg_score.write_csv(args.output_csv, rows_from_files(args.data_dir, args.seg_name, args.truth_name, args.host, min_classes=args.n_class))


if __name__ == '__main__':
    main()
