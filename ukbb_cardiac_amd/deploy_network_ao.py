#!/usr/bin/env python3
"""Drop-in for the reference's ``common/deploy_network_ao.py`` (aortic cine
segmentation) on the MI355X HIP engine.

Command line as in ``demo_pipeline.py:116-117``.  Implemented: ``--model UNet``
(frame-wise 2-D U-Net, ``deploy_network_ao.py:111-128``) in sequence and ED/ES
mode, the reference's default ``--model UNet-LSTM`` (U-Net features +
bidirectional ConvLSTM over circular 9-frame windows with weighted tiling,
``:129-183``) and ``--model Temporal-UNet`` (3-D convolutions over the same
windows, ``network_ao.py:67-114``; fp32, or ``--precision bf16_3d``) in sequence mode, any ``--time_step``.

Output: ``seg_ao.nii.gz`` int32 with the input's affine and pixdim (``:189-196``).
"""
import collections
import os
import sys
import time

import numpy as np

if __package__ in (None, ''):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ukbb_cardiac_amd import nifti, pipeline                      # noqa: E402
from ukbb_cardiac_amd.flags import FlagError, FlagSet              # noqa: E402
from ukbb_cardiac_amd.label_tables import AorticTable             # noqa: E402
from ukbb_cardiac_amd.shard import default_device, io_threads_from_env, shard_from_env, subjects_for_shard  # noqa: E402


def define_flags():
    fs = FlagSet()                                      # reference: deploy_network_ao.py:25-49
    fs.DEFINE_integer('time_step', 1, 'Time step during deployment of LSTM.')
    fs.DEFINE_enum('seq_name', 'ao', ['ao'], 'Sequence name.')
    fs.DEFINE_enum('model', 'UNet-LSTM', ['UNet', 'UNet-LSTM', 'Temporal-UNet'], 'Model name.')
    fs.DEFINE_string('data_dir', 'Biobank_ao/validation',
                     'Path to the test set directory, under which images are organised in '
                     'subdirectories for each subject.')
    fs.DEFINE_string('model_path', '', 'Path to the saved trained model.')
    fs.DEFINE_boolean('process_seq', True, 'Process a time sequence of images.')
    fs.DEFINE_boolean('save_seg', True, 'Save segmentation.')
    fs.DEFINE_boolean('z_score', True, 'Normalise the image intensity to z-score. Otherwise, rescale the intensity.')
    fs.DEFINE_integer('weight_R', 5, 'Radius of the weighting window.')
    fs.DEFINE_float('weight_r', 0.1, 'Power of weight for the seq2seq loss. 0: uniform; 1: linear; 2: square.')
    env_idx, env_cnt = shard_from_env()
    fs.DEFINE_integer('device', default_device(), 'HIP device ordinal (after HIP_VISIBLE_DEVICES); defaults to '
                      'LOCAL_RANK under torch.distributed.run.')
    fs.DEFINE_integer('batch_slices', 64, 'Slices per forward call.')
    fs.DEFINE_integer('io_threads', min(2, io_threads_from_env(2)), 'Sequence mode: threads that read (inflate) the next cines ahead of the GPU and threads that '
                      'write finished segmentations behind it; 0 = strictly sequential subjects as in the reference.')
    fs.DEFINE_boolean('device_preproc', True, 'Sequences: z-score, padding, transposes and the argmax on the GPU '
                      '(float32, uint8, int16 and uint16 cines; bit-identical to the host path; --nodevice_preproc restores it).')
    fs.DEFINE_enum('precision', 'fp32', ['fp32', 'bf16', 'bf16_3d'], 'Arithmetic of the U-Net convolutions: fp32 MFMA (default) or bf16 MFMA operands with fp32 '
                   'accumulation (UKBB_PREC_BF16, include/ukbb_fcn.h; --model UNet: bf16 activations in HBM too, 2.8x the fp32 rate, '
                   'Dice 0.99 against fp32; BASELINE config 5.  Default UNet-LSTM model: the same U-Net plan, ConvLSTM on the bf16 matrix '
                   'instruction with bf16 hidden maps and fp32 cell state, 2.3x the fp32 rate, Dice >= 0.98 against fp32), or bf16_3d '
                   '(--model Temporal-UNet only, UKBB_PREC_BF16_3D: its 3-D convolutions on the bf16 matrix instruction, every 3-D map '
                   'bf16 in HBM, logits and softmax fp32; bf16 itself stays refused on that model).')
    fs.DEFINE_float('cine_scratch_gb', 0.0, 'UNet-LSTM and Temporal-UNet: device memory (GB, 1e9 bytes) the engine may hold for the per-cine scratch of the '
                    'windowed forward (hidden maps, gate pre-activations, cell state, network activations).  The windows of a cine then run in '
                    'chunks that fit, with the same bits as the unchunked run; a cine of any length fits a few GB, at the price of recomputing '
                    'the frames neighbouring chunks share.  0 (default): no budget (UNet-LSTM: the whole cine at once, 16.6 GB fp32 / 10.7 GB '
                    'bf16 for 100 frames of 256x256; Temporal-UNet: 4 GB chunks).  Several workers per GPU (shard.py --shards_per_gpu) should set '
                    'it to their share of the HBM.  A value below what one window needs stops at the first cine with the minimum in the message.',
                    lower_bound=0.0)
    fs.DEFINE_enum('label_gzip', 'small', list(nifti.LABEL_GZIP_MODES), 'Deflate of the label volumes: small = run-length tokens + dynamic Huffman '
                   '(typically below the size of zlib level 1; never above it on segmentation-like volumes), fast = fixed Huffman (larger files), zlib = as nibabel.  Same inflated bytes.')
    fs.DEFINE_string('output_csv', '', 'Sequence mode: also write the spreadsheet of aortic/eval_aortic_area.py (same columns and arithmetic) from '
                     'the per-frame class counts the GPU leaves behind.  Of the evaluation script\'s quality control '
                     '(cardiac_utils.aorta_pass_quality_control, eval_aortic_area.py:68-69) the criteria that need only the areas are applied '
                     '(1: zero area in a frame, 4: abrupt change between adjacent frames, 5: max / min >= 2) and a failing subject is dropped with '
                     'the script\'s message; criteria 2 (image noise) and 3 (connected components) are applied only with --aortic_qc_full.')
    fs.DEFINE_boolean('aortic_qc', True, 'With --output_csv: apply the count-only quality-control criteria above (false: every segmented subject gets a row).')
    fs.DEFINE_boolean('aortic_qc_full', False, 'With --output_csv and --aortic_qc: apply all five criteria of aorta_pass_quality_control in the script\'s '
                      'order, adding 2 (max intensity of a frame / mean ED intensity under the label >= 3) and 3 (two or more '
                      '18-connected components of more than 10 pixels in a frame); computed on the GPU next to the labels on the device '
                      'path (aorta_qc.py).')
    fs.DEFINE_string('pressure_csv', '', 'With --output_csv: the blood-pressure spreadsheet of eval_aortic_area.py:41-46 for the distensibility columns '
                     '(left empty without it).')
    fs.DEFINE_string('confidence_csv', '', 'Sequence mode, every model: also write one row per (subject, frame, label), and one per (subject, label) over '
                     'all frames, saying how sure the network was: the pixels of the label, their mean winning probability, their mean margin to '
                     'the runner-up, the shares of them whose winning probability lies below 0.5 and below 0.75, and the soft area (the sum of '
                     'the label\'s probability over all pixels) -- integer reductions of the softmax (UNet) or of the averaged window '
                     'probabilities (UNet-LSTM, Temporal-UNet) while they are on the GPU (confidence.py).  Off by default.')
    fs.DEFINE_integer('num_shards', env_cnt, 'Number of workers sharing data_dir.')
    fs.DEFINE_integer('shard_index', env_idx, 'This worker: subjects i with i % num_shards == shard_index.')
    return fs


def sequence_on_device(FLAGS, engine, image, log=print):
    """Does this cine take the device pre-processing?  Needs an engine, --device_preproc, --z_score, a 4-D float32, uint8,
    int16 or uint16 volume, and the once-per-dtype check that the device z-score reproduces this numpy (it mirrors numpy
    internals; a mismatch keeps the host path and is logged)."""
    if engine is None or not getattr(FLAGS, 'device_preproc', False) or not FLAGS.z_score or image.ndim != 4:
        return False
    from ukbb_cardiac_amd import device_pipeline
    if not device_pipeline.device_dtype_ok(image.dtype):
        return False
    return device_pipeline.device_zscore_matches_numpy(engine, warn=log, dtype=image.dtype)


class _ReadAhead:
    """nifti.load of the cines of a subject list on reader threads: asking for subject idx first schedules every read up to
    subject idx + threads; names[i] is None for a subject without a cine."""
    def __init__(self, names, threads):
        from concurrent.futures import ThreadPoolExecutor
        self.names, self.threads, self.pool = names, threads, ThreadPoolExecutor(threads)
        self.pending, self.ahead = collections.deque(), 0           # (index, future) in ascending order; reads scheduled so far

    def load(self, idx, name):
        upto = min(idx + 1 + self.threads, len(self.names))
        for i in range(self.ahead, upto):
            if self.names[i] is not None:
                self.pending.append((i, self.pool.submit(nifti.load, self.names[i])))
        self.ahead = upto
        while self.pending and self.pending[0][0] < idx:
            self.pending.popleft()                                     # a cine that vanished between the listing and its turn
        return self.pending.popleft()[1].result() if self.pending and self.pending[0][0] == idx else nifti.load(name)


def _sequence_subject(FLAGS, data, data_dir, nim, forward, cine_forward, engine, log, table, save):
    """One cine of sequence mode (deploy_network_ao.py:92-196): device function or host function, file, table line."""
    window = (FLAGS.weight_R, FLAGS.weight_r, FLAGS.time_step) if FLAGS.model in ('UNet-LSTM', 'Temporal-UNet') else None
    image = nim.get_data()
    log('  Segmenting full sequence ...')
    t0 = time.time()
    if sequence_on_device(FLAGS, engine, image, log):
        from ukbb_cardiac_amd.device_pipeline import aortic_sequence_device
        pred, aux = aortic_sequence_device(image, engine, FLAGS.batch_slices, window, return_aux=True, qc=table.qc_full,
                                           confidence=table.confidence is not None)
        counts, qc_stats, cells = aux['counts'], aux.get('qc'), aux.get('confidence')
    else:
        # rescale_intensity clips `image` in place; the script's quality control reads the file
        image_qc = image.copy() if table.qc_full and not FLAGS.z_score else image
        if window is not None:
            prob = pipeline.aortic_lstm_prob_sequence(image, cine_forward, FLAGS.z_score, FLAGS.weight_R, FLAGS.weight_r,
                                                      time_step=FLAGS.time_step)
        else:
            prob = pipeline.aortic_prob_sequence(image, forward, FLAGS.z_score, FLAGS.batch_slices)
        pred = np.argmax(prob, axis=-1).astype(np.int32)      # host argmax, as :189
        counts, qc_stats = table.from_labels(image_qc, pred)
        cells = None
        if table.confidence is not None:
            from ukbb_cardiac_amd import confidence
            cells = confidence.cells_from_volume(prob, pred)
    if FLAGS.save_seg:
        log('  Saving segmentation ...')
        save(pred, '{0}/seg_{1}.nii.gz'.format(data_dir, FLAGS.seq_name), nim.affine, nim.header['pixdim'])
    log('  Segmentation time = {:3f}s'.format(time.time() - t0))
    table.record(data, nim.header['pixdim'], counts, qc_stats, log)
    table.record_confidence(data, cells)


def _frames_subject(FLAGS, data_dir, forward, log):
    """The ED and ES frames of one subject (ED/ES mode, deploy_network_ao.py:206-258); False: a frame is missing, skipped."""
    seq = FLAGS.seq_name
    names = {fr: '{0}/{1}_{2}.nii.gz'.format(data_dir, seq, fr) for fr in ('ED', 'ES')}
    if not all(os.path.exists(p) for p in names.values()):
        log('  Directory {0} does not contain an image with file name {1} or {2}. Skip.'.format(
            data_dir, os.path.basename(names['ED']), os.path.basename(names['ES'])))
        return False
    for fr in ('ED', 'ES'):
        log('  Reading {} ...'.format(names[fr]))
        nim = nifti.load(names[fr])
        t0 = time.time()
        pred = pipeline.aortic_segment_frame(nim.get_data(), forward, FLAGS.z_score, FLAGS.batch_slices)
        log('  Segmentation time = {:3f}s'.format(time.time() - t0))
        if FLAGS.save_seg:
            log('  Saving segmentation ...')
            nifti.save(pred, '{0}/seg_{1}_{2}.nii.gz'.format(data_dir, seq, fr), nim.affine, nim.header['pixdim'])
    return True


def run(FLAGS, forward, log=print, cine_forward=None, engine=None):
    """``forward`` stands for the frame-wise sess.run ('UNet'); ``cine_forward`` for the windowed one ('UNet-LSTM', 'Temporal-UNet').
    With ``engine`` (and --device_preproc, --z_score) sequences take device_pipeline.aortic_sequence_device."""
    windowed = FLAGS.model in ('UNet-LSTM', 'Temporal-UNet')
    if FLAGS.model == 'Temporal-UNet' and cine_forward is None:
        # NotImplementedError (not ValueError): a Temporal-UNet needs the windowed forward, frame-wise calls cannot serve it
        raise NotImplementedError('--model Temporal-UNet needs a Temporal-UNet model (cine_forward)')
    if windowed:
        if cine_forward is None:
            raise ValueError('--model UNet-LSTM needs a UNet-LSTM model (cine_forward)')
        if FLAGS.time_step < 1:
            raise ValueError('--time_step %d: range(0, T, time_step) needs a positive step '
                             '(common/deploy_network_ao.py:147)' % FLAGS.time_step)
    start_time = time.time()
    data_list = subjects_for_shard(sorted(os.listdir(FLAGS.data_dir)), FLAGS.shard_index, FLAGS.num_shards)
    processed = []
    table = AorticTable(FLAGS)                                  # --output_csv, --confidence_csv: flag checks first
    # Sequence mode with --io_threads > 0: the next cines are read (inflated) by reader threads while the GPU works on this one,
    # and the segmentation files are written behind it; order of subjects, log lines and files are those of the sequential loop.
    nthr = int(getattr(FLAGS, 'io_threads', 0)) if FLAGS.process_seq else 0
    reader = writers = None
    writes = []
    if nthr > 0:
        from concurrent.futures import ThreadPoolExecutor
        names = ['{0}/{1}.nii.gz'.format(os.path.join(FLAGS.data_dir, d), FLAGS.seq_name) for d in data_list]
        reader = _ReadAhead([n if os.path.isdir(os.path.dirname(n)) and os.path.exists(n) else None for n in names], nthr)
        writers = ThreadPoolExecutor(nthr)

    def save(*args):
        if writers is not None:
            writes.append(writers.submit(nifti.save, *args))
        else:
            nifti.save(*args)

    try:
        for idx, data in enumerate(data_list):
            log(data)
            data_dir = os.path.join(FLAGS.data_dir, data)
            if not os.path.isdir(data_dir):
                continue
            if not FLAGS.process_seq:
                if windowed:                                           # reference: deploy_network_ao.py:202-205
                    log('{0} does not support frame-wise segmentation. Please use the -process_seq flag.'.format(FLAGS.model))
                    return processed
                if _frames_subject(FLAGS, data_dir, forward, log):
                    processed.append(data)
                continue
            image_name = '{0}/{1}.nii.gz'.format(data_dir, FLAGS.seq_name)
            if not os.path.exists(image_name):
                log('  Directory {0} does not contain an image with file name {1}. Skip.'.format(
                    data_dir, os.path.basename(image_name)))
                continue
            log('  Reading {} ...'.format(image_name))
            nim = reader.load(idx, image_name) if reader is not None else nifti.load(image_name)
            _sequence_subject(FLAGS, data, data_dir, nim, forward, cine_forward, engine, log, table, save)
            processed.append(data)
        for w in writes:
            w.result()
    finally:
        if reader is not None:
            reader.pool.shutdown(wait=True)
            writers.shutdown(wait=True)
    table.write(data_list, log)
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
    if 'CUDA_VISIBLE_DEVICES' in os.environ and 'HIP_VISIBLE_DEVICES' not in os.environ:
        os.environ['HIP_VISIBLE_DEVICES'] = os.environ['CUDA_VISIBLE_DEVICES']
    if FLAGS.model == 'Temporal-UNet' and FLAGS.precision not in ('fp32', 'bf16_3d'):
        sys.exit('Error: --model Temporal-UNet runs in fp32 only (no bf16 plan for its 3-D convolutions) under --precision %s; '
                 'its bf16 mode is --precision bf16_3d.' % FLAGS.precision)
    if FLAGS.model != 'Temporal-UNet' and FLAGS.precision == 'bf16_3d':
        sys.exit('Error: --precision bf16_3d is the bf16 mode of --model Temporal-UNet (3-D convolutions); --model %s takes --precision bf16.' % FLAGS.model)
    from ukbb_cardiac_amd.shard import apply_cpu_set_from_env
    apply_cpu_set_from_env()                             # shard.launch's per-worker CPU set, before the first GPU call starts threads
    from ukbb_cardiac_amd.arch import KIND_TEMPORAL_UNET, KIND_UNET_LSTM
    from ukbb_cardiac_amd.engine import Session
    nifti.set_label_gzip(FLAGS.label_gzip)
    with Session(FLAGS.model_path, device=FLAGS.device) as sess:
        want = {'UNet-LSTM': KIND_UNET_LSTM, 'Temporal-UNet': KIND_TEMPORAL_UNET}.get(FLAGS.model)     # 'UNet': any frame-wise model
        have = sess.engine.arch.kind
        if (want is not None or have in (KIND_UNET_LSTM, KIND_TEMPORAL_UNET)) and have != want:
            sys.exit('Error: --model %s but %s holds a %s model.' % (FLAGS.model, FLAGS.model_path, sess.engine.arch.name))
        if FLAGS.precision != 'fp32':
            sess.engine.set_precision(FLAGS.precision)
        if FLAGS.cine_scratch_gb > 0:
            if want is None:
                print('--cine_scratch_gb is ignored with --model UNet (frame-wise batches hold no per-cine scratch; see --batch_slices).')
            else:
                sess.engine.set_scratch_budget(int(FLAGS.cine_scratch_gb * 1e9))
        print('Start evaluating on the test set ...')

        def forward(batch):
            prob, pred = sess.run(['prob:0', 'pred:0'], feed_dict={'image:0': batch, 'training:0': False})
            return {'prob': prob, 'pred': pred}

        def cine_forward(frames, weight_R, weight_r, time_step=1):
            return sess.engine.run_cine(frames, weight_R, weight_r, time_step)[0]
        run(FLAGS, forward, cine_forward=cine_forward, engine=sess.engine)


if __name__ == '__main__':
    main()
