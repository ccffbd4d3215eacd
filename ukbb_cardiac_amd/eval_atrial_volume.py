#!/usr/bin/env python3
"""Drop-in for the reference's ``long_axis/eval_atrial_volume.py``: the left atrial bi-plane and right atrial single-plane
volumes of every subject under ``--data_dir`` that has ``seg_la_2ch.nii.gz``, ``seg_la_4ch.nii.gz`` and ``sa.nii.gz``, written to
``--output_csv`` with the reference's eight columns.  Same command line (``--data_dir``, ``--output_csv``), same arithmetic
(ukbb_cardiac_amd/atrial.py), same skips and messages: a subject failing atrium_pass_quality_control on either file is left out.

The label maps go to the GPU as uint8; the gate statistics and the per-frame areas and lengths are computed there
(ukbb_fcn_label_components, ukbb_fcn_atrial_area_length) and only a few kilobytes come back.  ``--host`` computes the same
integers in numpy (atrial.frame_stats_host).  ``--frames_2ch A.csv --frames_4ch B.csv`` builds the table from two files written
by ``deploy_network.py --atrial_csv`` without touching a label file.

Not written: the ``lm_la_*_00.vtk`` landmark files (VTK is not a dependency; the landmarks are columns of --atrial_csv).  Where
the reference raises IndexError -- a 4-chamber sequence with fewer frames than the 2-chamber one -- the subject is skipped with
a message."""
import argparse
import os
import sys

import numpy as np

if __package__ in (None, ''):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ukbb_cardiac_amd import atrial, measures, nifti, qc_gates   # noqa: E402

SEQS = ('la_2ch', 'la_4ch')


def _n_class(seg, seq):
    n_class = max(qc_gates.min_classes(seq), int(seg.max()) + 1)
    if n_class > 16:
        raise ValueError('label %d: the atrial measures take label maps of at most 16 classes' % (n_class - 1))
    return n_class


def sequence_stats(seg, seq, affine, long_axis, host):
    """(gate statistics, atrial statistics [T, n_class, 8]) of an (X,Y,1,T) label volume: on the device, or in numpy with ``host``."""
    n_class = _n_class(seg, seq)
    if host:
        return qc_gates.stats_host(seg, seq, False, n_class), atrial.frame_stats_host(seg[:, :, 0, :], n_class, affine, long_axis)
    import torch
    from ukbb_cardiac_amd import device_pipeline as dp
    if not torch.cuda.is_available():
        raise RuntimeError('no GPU: the atrial measures run on the device (--host computes them in numpy)')
    stream = torch.cuda.current_stream().cuda_stream
    lab = torch.from_numpy(np.ascontiguousarray(seg.astype(np.uint8).reshape(-1, order='F'))).cuda()
    return (dp.device_gate_stats(lab, seg.shape, seq, False, n_class, stream),
            dp.device_atrial_stats(lab, seg.shape, n_class, affine, long_axis, stream))


def rows_from_files(data_path, host=False, log=print):
    """[(subject, the eight values)] as eval_atrial_volume.py:35-163 collects them."""
    table = []
    for data in sorted(os.listdir(data_path)):
        data_dir = os.path.join(data_path, data)
        names = {seq: '{0}/seg_{1}.nii.gz'.format(data_dir, seq) for seq in SEQS}
        sa_name = '{0}/sa.nii.gz'.format(data_dir)
        if not (os.path.exists(names['la_2ch']) and os.path.exists(names['la_4ch']) and os.path.exists(sa_name)):
            continue
        log(data)
        long_axis = atrial.long_axis_from_sa(nifti.load_header(sa_name)['affine'])
        frames, T, pixdim4 = {}, None, None
        for seq in SEQS:
            nim = nifti.load(names[seq])
            seg = nim.get_data()
            if seg.ndim != 4 or seg.shape[2] != 1:
                log('{0} seg_{1}: expected an (X, Y, 1, T) label volume, found shape {2}. Skip.'.format(data, seq, seg.shape))
                break
            if seq == 'la_2ch':
                T = seg.shape[3]                       # the 2-chamber file's, for both loops (:63, :114)
            elif seg.shape[3] < T:
                log('{0} seg_la_4ch has {1} frames, seg_la_2ch {2}: the 4-chamber loop would run past its end. Skip.'.format(
                    data, seg.shape[3], T))
                break
            gate, stats = sequence_stats(seg, seq, nim.affine, long_axis, host)
            passed, message = qc_gates.gate_from_stats(gate, seq, False, names[seq])
            if not passed:
                log(message)
                log('{0} seg_{1} does not atrium_pass_quality_control.'.format(data, seq))
                break
            frames[seq] = atrial.frames_from_stats(stats, nim.affine, nim.header['pixdim'])
            pixdim4 = nim.header['pixdim'][4]
        else:
            table.append((data, atrial.atrial_row(atrial.atrial_volumes(frames['la_2ch'], frames['la_4ch'], pixdim4, T)['val'])))
    return table


def rows_from_frames(frames_2ch, frames_4ch, log=print):
    """The same table from two --atrial_csv files (atrial.read_frames_csv): the subjects both hold, the verdicts they carry."""
    two, four = atrial.read_frames_csv(frames_2ch), atrial.read_frames_csv(frames_4ch)
    table = []
    for data in sorted(set(two) & set(four)):
        log(data)
        if not two[data]['gate']:
            log('{0} seg_la_2ch does not atrium_pass_quality_control.'.format(data))
            continue
        if not four[data]['gate']:
            log('{0} seg_la_4ch does not atrium_pass_quality_control.'.format(data))
            continue
        T = len(two[data]['frames'])
        if len(four[data]['frames']) < T:
            log('{0} seg_la_4ch has {1} frames, seg_la_2ch {2}: the 4-chamber loop would run past its end. Skip.'.format(
                data, len(four[data]['frames']), T))
            continue
        # the frame duration is not in the per-frame record; it enters the heart rate alone, which the table does not hold
        table.append((data, atrial.atrial_row(atrial.atrial_volumes(two[data]['frames'], four[data]['frames'], float('nan'), T)['val'])))
    return table


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--data_dir', metavar='dir_name', default='')
    parser.add_argument('--output_csv', metavar='csv_name', default='', required=True)
    parser.add_argument('--host', action='store_true', help='compute the statistics in numpy instead of on the GPU')
    parser.add_argument('--frames_2ch', metavar='csv_name', default='', help='deploy_network.py --seq_name la_2ch --atrial_csv file')
    parser.add_argument('--frames_4ch', metavar='csv_name', default='', help='deploy_network.py --seq_name la_4ch --atrial_csv file')
    args = parser.parse_args(argv)
    if bool(args.frames_2ch) != bool(args.frames_4ch):
        parser.error('--frames_2ch and --frames_4ch go together')
    if args.frames_2ch:
        table = rows_from_frames(args.frames_2ch, args.frames_4ch)
    else:
        if not args.data_dir:
            parser.error('--data_dir is required (or --frames_2ch and --frames_4ch)')
        table = rows_from_files(args.data_dir, args.host)
    measures.write_csv(args.output_csv, atrial.ATRIAL_COLUMNS, table)


if __name__ == '__main__':
    main()
