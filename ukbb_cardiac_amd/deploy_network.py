#!/usr/bin/env python3
"""Drop-in for the reference's ``common/deploy_network.py``: short-axis and
long-axis cine segmentation, NIfTI in -> label-map NIfTI out, with the network
evaluated by the MI355X HIP engine instead of a TensorFlow session.

Accepts the reference's command line verbatim (``demo_pipeline.py:63-64,89-96``)::

    python3 ukbb_cardiac_amd/deploy_network.py --seq_name sa --data_dir demo_image \
        --model_path trained_model/FCN_sa
    ... --seq_name la_4ch --seg4 ...

and writes the same files (``deploy_network.py:136-151,207-216``):
``seg_{seq}.nii.gz`` (float64, affine + pixdim of the input), ``{seq}_ED/ES.nii.gz``,
``seg_{seq}_ED/ES.nii.gz``; prefix ``seg4_`` with ``la_4ch --seg4``.
``--model_path`` names ``<model_path>.ukbbw``.

Extra flags (not in the reference): ``--device``, ``--batch_slices``,
``--num_shards`` / ``--shard_index`` (multi-GPU batch split), ``--output_csv``, ``--qc_csv``,
``--atrial_csv``, ``--score_against`` / ``--score_csv`` (Dice and contour distances against a second segmentation), ``--confidence_csv`` (how sure the network was, per frame and class), ``--device_inflate`` (gzip inputs inflated on the GPU), ``--device_label_gzip`` (label
volumes deflated on the GPU).
"""
import os
import sys
import time

import numpy as np

if __package__ in (None, ''):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ukbb_cardiac_amd import nifti, pipeline                      # noqa: E402
from ukbb_cardiac_amd.flags import FlagError, FlagSet              # noqa: E402
from ukbb_cardiac_amd.label_tables import LabelTables              # noqa: E402
# pipelined_on_device and sequence_on_device are not used here: they keep the names under which callers and tests ask this script
# how it routes a subject
from ukbb_cardiac_amd.sequence_run import (SequenceRun, device_label_gzip_mode, device_path, pipelined_on_device, seg_prefix,   # noqa: E402,F401
                                            sequence_on_device)
from ukbb_cardiac_amd.shard import (ClaimQueue, apply_cpu_set_from_env, claim_path, default_device, io_threads_from_env,   # noqa: E402
                                    shard_from_env)


def define_flags():
    fs = FlagSet()                                      # reference: deploy_network.py:25-40
    fs.DEFINE_enum('seq_name', 'sa', ['sa', 'la_2ch', 'la_4ch'], 'Sequence name.')
    fs.DEFINE_string('data_dir', 'ukbb_cardiac_demo',
                     'Path to the data set directory, under which images are organised in '
                     'subdirectories for each subject.')
    fs.DEFINE_string('model_path', '', 'Path to the saved trained model.')
    fs.DEFINE_boolean('process_seq', True, 'Process a time sequence of images.')
    fs.DEFINE_boolean('save_seg', True, 'Save segmentation.')
    fs.DEFINE_boolean('seg4', False, 'Segment all the 4 chambers in long-axis 4 chamber view.')
    env_idx, env_cnt = shard_from_env()
    fs.DEFINE_integer('device', default_device(), 'HIP device ordinal (after HIP_VISIBLE_DEVICES); defaults to '
                      'LOCAL_RANK under torch.distributed.run.')
    fs.DEFINE_integer('batch_slices', 128, 'Slices per forward call.')
    fs.DEFINE_boolean('device_preproc', True, 'Percentile rescale, padding, transposes and label counting on the GPU '
                      '(float32, uint8, int16 and uint16 sequences; results identical to the host path).')
    fs.DEFINE_boolean('numpy1_casting', False, 'Rescale intensities with the float32 arithmetic numpy 1.x used when the reference '
                      'was written (1 ulp from numpy 2; host pre-processing only; INTEGRATION.md section 5).')
    fs.DEFINE_integer('io_threads', io_threads_from_env(8), 'Reader threads (gzip NIfTI -> pinned staging) and writer threads (float64 label volume, gzip) '
                      'around the GPU in sequence mode; 0 = strictly sequential subjects as in the reference.')
    fs.DEFINE_integer('device_inflate', 0, 'Sequence mode with --device_preproc: inflate the gzip NIfTI inputs on the GPU, up to this many subjects per '
                      'launch (one wave per file; the readers only read).  0 = off: the reader threads inflate.  A file the device path declines '
                      '(scaled / big-endian / float64 voxels, several gzip members, anything its strict decoder or the CRC-32 check refuses) '
                      'takes the host reader as before.  Same output files.')
    fs.DEFINE_enum('precision', 'fp32', ['fp32', 'f32x3', 'bf16_store', 'bf16_full'], 'Arithmetic of the matrix products: fp32 MFMA (default), fp32 results from three '
                   'bf16 pieces per operand (UKBB_PREC_F32X3, include/ukbb_fcn.h; same labels, faster head), or bf16_store: the encoder on bf16 '
                   'matrix instructions with its maps stored as bf16, squeeze and head in fp32 on the stored values (UKBB_PREC_BF16_STORE; labels '
                   'differ from fp32 next to class borders, Dice >= 0.98 per class on the test phantoms), or bf16_full: bf16_store with the '
                   'head\'s three matrix products on bf16 matrix instructions too -- their weights rounded to bf16 once when packed, the two '
                   'hidden activations once in registers; biases, the upsampled G_l sum, accumulators, logits, softmax and labels stay fp32 '
                   '(UKBB_PREC_BF16_FULL; same Dice bound).')
    fs.DEFINE_boolean('f32x3_convs', False, 'With --precision f32x3: the eleven 3x3 layers conv1_0 .. conv4_2 from three bf16 pieces per operand as '
                      'well (ukbb_fcn_set_f32x3_convs, include/ukbb_fcn.h): fp32 maps, fp32 accumulation, bias, ReLU and stores; same output files '
                      'up to voxels next to a tie of the two largest logits.  A flag error under any other --precision.')
    fs.DEFINE_enum('label_gzip', 'small', list(nifti.LABEL_GZIP_MODES), 'Deflate of the label volumes: small = run-length tokens + dynamic Huffman '
                   '(typically below the size of zlib level 1, ~20x less CPU), fast = fixed Huffman (2-4x larger files), zlib = as nibabel. Same inflated bytes.')
    fs.DEFINE_boolean('device_label_gzip', False, 'Sequence mode, pipelined loop (--device_preproc with --io_threads > 0, without --device_inflate): '
                      'deflate the float64 label volume seg_{seq}.nii.gz on the GPU, with the code set of --label_gzip small | fast, and copy back the '
                      'gzip member instead of the labels.  Same output files, byte for byte.  A subject the device encoder declines (more runs or more '
                      'output than its buffers hold, noise-like labels) takes the host writer.  Ignored with --label_gzip zlib; the sequential loop '
                      '(--io_threads 0, host pre-processing) and the --device_inflate rounds keep the host writer.')
    fs.DEFINE_string('output_csv', '', '--seq_name sa, sequence mode: also write the spreadsheet of short_axis/eval_ventricular_volume.py '
                     '(same columns, same arithmetic) from the per-frame class counts the GPU leaves behind -- no second pass over '
                     'seg_sa.nii.gz.  Subjects already segmented by an earlier run are measured from their files.')
    fs.DEFINE_string('qc_csv', '', 'Sequence mode: also write the verdict of the quality-control gate the reference applies to this '
                     'segmentation before its strain / wall-thickness / atrial-volume stages (sa: sa_pass_quality_control on the ED frame; '
                     'la_4ch --seg4: la_pass_quality_control; la_2ch, la_4ch: atrium_pass_quality_control), from component statistics of '
                     'the labels while they are on the GPU: columns gate, passed, message.  Subjects already segmented by an earlier '
                     'run are gated from their files.')
    fs.DEFINE_string('atrial_csv', '', '--seq_name la_2ch or la_4ch (without --seg4), sequence mode: also write what '
                     'cardiac_utils.evaluate_atrial_area_length measures on every frame -- one row per (subject, frame, label): the component '
                     'size, the status, the two end pixels of the long-axis intersection, area (cm2), length (cm), the two landmarks in world '
                     'coordinates and the verdict of the atrial gate -- from the labels while they are on the GPU.  The long axis comes from '
                     '<subject>/sa.nii.gz; a subject without it gets no rows.  eval_atrial_volume.py --frames_2ch / --frames_4ch turns two '
                     'such files into the table of long_axis/eval_atrial_volume.py.')
    fs.DEFINE_string('score_against', '', 'With --score_csv: the stem of the label file to score every segmentation against, '
                     '<subject>/<STEM>.nii.gz (label_sa: the manual annotations in the layout of data/prepare_data_ukbb2964.py; seg_sa of another '
                     'directory tree linked in: another tool\'s result).')
    fs.DEFINE_string('score_csv', '', 'Sequence mode, with --score_against: also write one row per (subject, annotated frame, label) with the '
                     'Dice overlap, the mean contour distance and the Hausdorff distance (mm) of common/image_utils.py np_categorical_dice and '
                     'distance_metric, from the labels while they are on the GPU.  A subject without the file, or whose file has another '
                     'shape or a label the model does not have, gets no rows; frames without a non-zero truth label give none.  Subjects '
                     'already segmented by an earlier run are scored from their files.')
    fs.DEFINE_string('confidence_csv', '', 'Sequence mode: also write one row per (subject, frame, label), and one per (subject, label) over all frames, '
                     'saying how sure the network was: the voxels of the label, their mean winning probability, their mean margin to the '
                     'runner-up, the shares of them whose winning probability lies below 0.5 and below 0.75, and the soft volume (the sum of the '
                     'label\'s probability over all voxels) -- integer reductions of the softmax while a chunk of slices is on the GPU '
                     '(confidence.py).  The forward then stores its probabilities, one chunk at a time; off by default.  Subjects already '
                     'segmented by an earlier run get no rows: their probabilities are gone.')
    fs.DEFINE_integer('num_shards', env_cnt, 'Number of workers sharing data_dir.')
    fs.DEFINE_integer('shard_index', env_idx, 'This worker: subjects i with i % num_shards == shard_index.')
    fs.DEFINE_boolean('work_stealing', True, 'With num_shards > 1: after its own share a worker takes subjects of the other shards that '
                      'nobody has claimed yet (claim file <subject>/.claim.<seg>_<seq>, created with O_EXCL; claims of dead workers are swept). '
                      'Sequence mode with --save_seg only: the saved label file is what marks a subject done, so a run that saves none '
                      '(--nosave_seg, tables only) keeps the strict split and says so.  --nowork_stealing = the strict i % num_shards split.')
    return fs


_sequence_subject = SequenceRun.on_this_thread           # one subject start to finish on this thread, under the name it has here


class _SequenceRun(SequenceRun):
    """The loops of this script reach the one-subject path through ``_sequence_subject``: whoever replaces that name -- a test that
    proves that no subject leaves the pipeline -- sees every subject that takes it, from whichever loop."""

    def on_this_thread(self, *args, **kwargs):
        return _sequence_subject(self, *args, **kwargs)


def run(FLAGS, forward, log=print, engine=None):
    """The subject loop of deploy_network.py:52-225 with ``forward`` standing for sess.run.  Sequence mode is a SequenceRun
    (sequence_run.py): with ``engine`` and --device_preproc, float32 and integer sequences take one of its device loops."""
    start_time = time.time()
    seq, pre = FLAGS.seq_name, seg_prefix(FLAGS)
    # the static split (subject i -> shard i mod num_shards) and, on top of it, claim-file work stealing in sequence mode -- with
    # --save_seg only: a claim says "someone is on it" and is gone when the subject is finished; what then says "done" is the label
    # file.  Without one a finished subject would look open again to every other worker
    stealing = bool(getattr(FLAGS, 'work_stealing', False)) and FLAGS.process_seq and FLAGS.save_seg
    if FLAGS.num_shards > 1 and getattr(FLAGS, 'work_stealing', False) and FLAGS.process_seq and not stealing:
        log('--work_stealing off, the static split i % num_shards instead: no label file is saved (--save_seg off) to mark a subject done')
    queue = ClaimQueue(FLAGS.data_dir, sorted(os.listdir(FLAGS.data_dir)), FLAGS.shard_index, FLAGS.num_shards, '%s_%s' % (pre, seq), stealing=stealing)
    data_list = list(queue)
    processed, table_time = [], []
    tables = LabelTables(FLAGS, engine)                 # --output_csv, --qc_csv, --atrial_csv, --score_csv, --confidence_csv: flag checks first
    shard_subjects = list(queue.static)                 # whose earlier-run results this worker measures for the tables
    on_device = device_path(FLAGS, engine)
    inflate = int(getattr(FLAGS, 'device_inflate', 0) or 0) > 0
    if inflate and not on_device:
        raise ValueError('--device_inflate needs sequence mode (--process_seq) with --device_preproc and without --numpy1_casting')

    def one_subject(data):
        """One entry of the walk in ED / ES mode (deploy_network.py:153-216)."""
        data_dir = os.path.join(FLAGS.data_dir, data)
        log(data)
        if not os.path.isdir(data_dir):
            return
        if os.path.exists('{0}/{1}_{2}.nii.gz'.format(data_dir, pre, seq)):
            return                                   # already segmented: idempotent / resumable (:62-67)
        names = {fr: '{0}/{1}_{2}.nii.gz'.format(data_dir, seq, fr) for fr in ('ED', 'ES')}
        if not all(os.path.exists(p) for p in names.values()):
            log('  Directory {0} does not contain an image with file name {1} or {2}. Skip.'.format(
                data_dir, os.path.basename(names['ED']), os.path.basename(names['ES'])))
            return
        for fr in ('ED', 'ES'):
            log('  Reading {} ...'.format(names[fr]))
            nim = nifti.load(names[fr])
            image = nim.get_data()
            log('  Segmenting {} frame ...'.format(fr))
            t0 = time.time()
            pred = pipeline.segment_frame(image, forward, FLAGS.batch_slices, bool(getattr(FLAGS, 'numpy1_casting', False)))
            seg_time = time.time() - t0
            log('  Segmentation time = {:3f}s'.format(seg_time))
            table_time.append(seg_time)
            processed.append(data)
            if FLAGS.save_seg:
                log('  Saving segmentation ...')
                nifti.save(pred, '{0}/{1}_{2}_{3}.nii.gz'.format(data_dir, pre, seq, fr), nim.affine,
                           nim.header['pixdim'])
    if getattr(FLAGS, 'device_label_gzip', False):
        pipelined = FLAGS.process_seq and not inflate and on_device and getattr(FLAGS, 'io_threads', 0) > 0
        reason = device_label_gzip_mode(FLAGS)[1] if pipelined else \
            'it takes effect in the pipelined sequence loop only (--device_preproc, --io_threads > 0, no --device_inflate)'
        if reason:
            log('--device_label_gzip ignored: %s' % reason)
    if FLAGS.process_seq:
        seq_run = _SequenceRun(FLAGS, engine, tables, queue, log, data_list)
        if inflate:
            processed, table_time = seq_run.run(seq_run.inflate_rounds)
        elif on_device and getattr(FLAGS, 'io_threads', 0) > 0:
            processed, table_time = seq_run.run(seq_run.pipelined)
        else:
            processed, table_time = seq_run.run(seq_run.sequential, forward)
        busy = [data for data in queue.still_busy() if not os.path.exists('{0}/{1}/{2}_{3}.nii.gz'.format(FLAGS.data_dir, data, pre, seq))]
        if busy:                                        # never silently: a claim that no rule sweeps would hide its subject on every rerun
            log('Left to the worker whose claim ({0}) they carry, not segmented here: {1}'.format(os.path.basename(claim_path('', queue.what)), ' '.join(busy)))
    else:
        for data in data_list:
            one_subject(data)
    tables.write(shard_subjects, log)
    if table_time:
        log('Average segmentation time = {:.3f}s per {}'.format(float(np.mean(table_time)),
                                                               'sequence' if FLAGS.process_seq else 'frame'))
    process_time = time.time() - start_time
    if processed:
        log('Including image I/O and device resource allocation, it took {:.3f}s for processing {:d} subjects '
            '({:.3f}s per subjects).'.format(process_time, len(processed), process_time / len(processed)))
    return processed


def main(argv=None):
    fs = define_flags()
    try:
        FLAGS, rest = fs.parse(sys.argv[1:] if argv is None else argv)
    except FlagError as e:
        sys.exit('FATAL Flags parsing error: %s\n%s' % (e, fs.usage()))
    if FLAGS.f32x3_convs and FLAGS.precision != 'f32x3':
        sys.exit('FATAL Flags parsing error: --f32x3_convs needs --precision f32x3 (got --precision %s)\n%s' % (FLAGS.precision, fs.usage()))
    if 'CUDA_VISIBLE_DEVICES' in os.environ and 'HIP_VISIBLE_DEVICES' not in os.environ:
        os.environ['HIP_VISIBLE_DEVICES'] = os.environ['CUDA_VISIBLE_DEVICES']   # demo_pipeline.py:25,63
    apply_cpu_set_from_env()                             # shard.launch's per-worker CPU set, before the first GPU call starts threads
    from ukbb_cardiac_amd.engine import Session          # raises if the HIP library is missing
    with Session(FLAGS.model_path, device=FLAGS.device) as sess:
        if FLAGS.precision != 'fp32':
            sess.engine.set_precision(FLAGS.precision)
        if FLAGS.f32x3_convs:
            sess.engine.set_f32x3_convs(True)
        nifti.set_label_gzip(FLAGS.label_gzip)
        print('Start deployment on the data set ...')

        def forward(batch):
            if FLAGS.confidence_csv:                     # the host path forms the table from the probabilities of every chunk
                prob, pred = sess.run(['prob:0', 'pred:0'], feed_dict={'image:0': batch, 'training:0': False})
                return {'prob': prob, 'pred': pred}
            pred = sess.run('pred:0', feed_dict={'image:0': batch, 'training:0': False})
            return {'pred': pred}
        run(FLAGS, forward, engine=sess.engine)


if __name__ == '__main__':
    main()
