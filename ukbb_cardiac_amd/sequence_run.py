"""Sequence mode of deploy_network.py (common/deploy_network.py:52-151) for one worker: what a run shares (``SequenceRun``), one
lazy walk over the subjects still to segment (``walk``), one way from a subject's labels to its log lines, table rows, five files
and released claim (``finish``), and the three sources of labels that differ in nothing else:

    sequential        subject after subject on this thread (``on_this_thread``): the host path of the reference, or
                      device_pipeline.segment_sequence_device for one subject
    pipelined         reader threads, subject_pipeline.SubjectPipeline with up to two subjects in flight, writer threads
    inflate_rounds    --device_inflate K: the readers only read, device_inflate.DeviceInflater inflates K files per launch

A subject the two overlapped sources cannot take (float64 voxels, a declined stream, a volume larger than the staging buffers)
goes through ``on_this_thread``.  Same files, byte for byte, whichever source a subject takes.
"""
import os
import time
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import nifti, pipeline
from .device_inflate import NO_ROOM, Declined, DeviceInflater, frame_to_host, header_image


def seg_prefix(FLAGS):
    return 'seg4' if (FLAGS.seq_name == 'la_4ch' and FLAGS.seg4) else 'seg'


def save_sequence_outputs(data_dir, pre, seq, affine, pixdim, pred, frames, blob=None):
    """The five files of deploy_network.py:136-151.  pred: (X,Y,Z,T) labels, stored as float64 (:92); frames: {'ED'|'ES':
    (image frame, label frame)}.  blob: seg_{seq}.nii.gz ready-made (the member the device encoder wrote: the bytes nifti.save
    gives for pred), written in pred's place."""
    for fr, (img_fr, seg_fr) in frames.items():
        nifti.save(img_fr, '{0}/{1}_{2}.nii.gz'.format(data_dir, seq, fr), affine)
        nifti.save(seg_fr, '{0}/{1}_{2}_{3}.nii.gz'.format(data_dir, pre, seq, fr), affine)
    # seg_{seq}.nii.gz doubles as the 'already segmented, skip' marker (:66-67), so it is written LAST and -- like every
    # file nifti.save writes -- appears under its name only when complete (tmp file + os.replace): a worker killed
    # anywhere in here leaves a subject that the rerun segments again, never a half-written one that it skips.
    if blob is not None:
        nifti.save_gzip_blob(blob, '{0}/{1}_{2}.nii.gz'.format(data_dir, pre, seq))
    else:
        nifti.save(pred, '{0}/{1}_{2}.nii.gz'.format(data_dir, pre, seq), affine, pixdim, as_dtype=np.float64)


def device_path(FLAGS, engine):
    """Does this run pre-process on the device?  Sequence mode with an engine and --device_preproc, without --numpy1_casting (its
    float32 arithmetic is host only)."""
    return bool(FLAGS.process_seq and engine is not None and getattr(FLAGS, 'device_preproc', False)
                and not getattr(FLAGS, 'numpy1_casting', False))


def sequence_on_device(FLAGS, engine, image):
    """on_this_thread: device pre-processing (device_pipeline.segment_sequence_device) for this subject?  A run on the device
    path and a dtype the device reproduces."""
    if not device_path(FLAGS, engine):
        return False
    from . import device_pipeline
    return device_pipeline.device_dtype_ok(image.dtype)


def pipelined_on_device(image):
    """pipelined: does this subject go through the subject pipeline (else: drain, then on_this_thread)?  4-D float32, uint8,
    int16 or uint16 volumes; float64 (every file with a non-trivial scl_slope) and the other integer types stay on the host."""
    from . import device_pipeline
    return image.ndim == 4 and device_pipeline.device_dtype_ok(image.dtype)


def device_label_gzip_mode(FLAGS):
    """pipelined: the code set --device_label_gzip gives the device encoder, or why the flag has no effect there:
    ('small' | 'fast', None) or (None, reason); (None, None) without the flag.  deploy_network logs the reason."""
    if not getattr(FLAGS, 'device_label_gzip', False):
        return None, None
    if not FLAGS.save_seg:
        return None, 'no label volume is saved (--save_seg off)'
    if not nifti.LABEL_FAST_PATH:
        return None, "the run-length writer is switched off (nifti.LABEL_FAST_PATH), zlib's output is not what the device encoder writes"
    if nifti.LABEL_GZIP_MODE not in ('small', 'fast'):
        return None, '--label_gzip %s keeps the host writer' % nifti.LABEL_GZIP_MODE
    return nifti.LABEL_GZIP_MODE, None


class SequenceRun:
    """What the sequence-mode run of one worker shares.  ``run(loop)`` takes one of the three loops below to the end."""
    last_phases = {}                                    # for tools/bench_device_inflate.py: ``phases`` of the last completed run

    def __init__(self, FLAGS, engine, tables, queue, log, data_list):
        self.FLAGS, self.engine, self.tables, self.queue, self.log, self.data_list = FLAGS, engine, tables, queue, log, data_list
        self.seq, self.pre = FLAGS.seq_name, seg_prefix(FLAGS)
        self.processed, self.table_time = [], []
        self.readers = self.writers = None              # start_threads(); without writers a subject's files are written inline
        self.writes = []                                # futures of the writers
        self.phases = {}                                # seconds of this thread by phase (inflate_rounds; writer_wait: run); pipelined with
        #                                                 --device_label_gzip: subjects by label_gzip_device / label_gzip_fallback

    def start_threads(self):
        """The reader and writer pools of the overlapped loops, --io_threads each."""
        n = max(1, int(self.FLAGS.io_threads))
        self.readers, self.writers = ThreadPoolExecutor(n), ThreadPoolExecutor(n)
        return n

    def run(self, loop, *args):
        """``loop(*args)`` to its end and the writers to theirs -> (processed, table_time).  However the loop ends, the threads
        are joined and every claim still held is released."""
        try:
            loop(*args)
            t0 = time.time()
            for w in self.writes:
                w.result()
            self.phases['writer_wait'] = time.time() - t0
        finally:
            for pool in (self.readers, self.writers):
                if pool is not None:
                    pool.shutdown(wait=True)
            self.queue.release_all()                    # an exception above must not leave live-looking claims behind
        SequenceRun.last_phases = self.phases
        return self.processed, self.table_time

    def walk(self):
        """(data, data_dir, image_name) of the subjects still to segment, in walk order, then of those another worker held when
        this one first came by (--work_stealing: finished by now -- skipped -- or orphaned).  Lazy: a subject is claimed when the
        loop asks for it, right before its read is scheduled, so a worker never holds more claims than its read-ahead and the
        rest of the list stays open.  Subjects that are skipped are logged on the first pass only."""
        def candidates(names, first):
            for data in names:
                data_dir = os.path.join(self.FLAGS.data_dir, data)
                if not os.path.isdir(data_dir) or os.path.exists('{0}/{1}_{2}.nii.gz'.format(data_dir, self.pre, self.seq)):
                    if first:
                        self.log(data)
                    continue                            # already segmented: idempotent / resumable (:62-67)
                image_name = '{0}/{1}.nii.gz'.format(data_dir, self.seq)
                if not os.path.exists(image_name):
                    if first:
                        self.log(data)
                        self.log('  Directory {0} does not contain an image with file name {1}. Skip.'.format(data_dir, os.path.basename(image_name)))
                    continue
                if self.queue.take(data):               # else another worker is on it: its name appears where it is segmented
                    # its owner may have written the label file and released the claim between the look above and the take:
                    # what is done is decided while the claim is held
                    if os.path.exists('{0}/{1}_{2}.nii.gz'.format(data_dir, self.pre, self.seq)):
                        self.queue.done(data)
                        if first:
                            self.log(data)
                        continue
                    yield (data, data_dir, image_name)
        yield from candidates(self.data_list, True)
        yield from candidates(self.queue.second_chance(), False)

    def finish(self, item, nim, seg_time, labels, counts, stats, clip, frame, done=None, ed_es=None, announce=True, gz_blob=None,
               label_frames=None):
        """Everything behind a subject's labels, once (deploy_network.py:118-151).  nim: its header (affine, pixdim); labels:
        (X,Y,Z,T) uint8 or float64; counts, stats: as LabelTables.record takes them; frame(k): image frame k, to be clipped to
        ``clip`` (lo, hi) -- the saved frames are the CLIPPED intensities (alias quirk) -- or clipped already
        (clip None); done(): called once the ED and ES frames have been copied out (the staging buffer goes back).  ed_es: the
        two frames where no counts exist to pick them from; announce=False: the caller has logged the three lines in front of the
        segmentation as it went.  gz_blob, label_frames: a subject whose label file was deflated on the device (labels None):
        seg_{seq}.nii.gz ready-made, and label_frames(k_ed, k_es) -> its two uint8 label frames.  The claim is released behind the
        subject's last file, by whoever writes it."""
        data, data_dir, image_name = item
        FLAGS, log = self.FLAGS, self.log
        if ed_es is None:
            from .device_pipeline import pick_ed_es_from_counts
            ed_es = pick_ed_es_from_counts(counts, self.seq, FLAGS.seg4)
        k_ed, k_es = ed_es
        if announce:
            log(data)
            log('  Reading {} ...'.format(image_name))
            log('  Segmenting full sequence ...')
        log('  Segmentation time = {:3f}s'.format(seg_time))
        log('  ED frame = {:d}, ES frame = {:d}'.format(k_ed, k_es))
        self.table_time.append(seg_time)
        self.processed.append(data)
        self.tables.record(data, data_dir, nim, counts, stats, log)
        if FLAGS.save_seg:
            log('  Saving segmentation ...')
            seg_frames = label_frames(k_ed, k_es) if labels is None else (labels[:, :, :, k_ed], labels[:, :, :, k_es])
            frames = {fr: (frame(k), np.asarray(seg_fr, np.float64)) for (fr, k), seg_fr in zip((('ED', k_ed), ('ES', k_es)), seg_frames)}
            if clip is not None:
                from .device_pipeline import clip_like_reference
                frames = {fr: (clip_like_reference(img_fr, clip), seg_fr) for fr, (img_fr, seg_fr) in frames.items()}
        if done is not None:
            done()
        if not FLAGS.save_seg:
            self.queue.done(data)
            return
        affine, pixdim = nim.affine, nim.header['pixdim']

        def write_then_release():                       # uint8 labels are expanded to the float64 volume here, by nifti.save
            try:
                save_sequence_outputs(data_dir, self.pre, self.seq, affine, pixdim, labels, frames, gz_blob)
            finally:
                self.queue.done(data)                   # the claim outlives the subject's last file (seg_{seq}.nii.gz, written last)
        if self.writers is None:
            write_then_release()
        else:
            self.writes.append(self.writers.submit(write_then_release))

    # ---- the three sources of labels -------------------------------------------------------------------
    def sequential(self, forward=None):
        for item in self.walk():
            self.on_this_thread(item, forward)

    def on_this_thread(self, item, forward=None, nim=None, truth=None):
        """One subject start to finish on this thread (deploy_network.py:80-131): the host path -- pipeline.segment_sequence
        through ``forward`` (default: the engine) -- or, per sequence_on_device, device pre-processing of this one subject.
        nim: its file where a reader thread has loaded it already; truth: what LabelTables.read_truth gave that thread."""
        data, data_dir, image_name = item
        FLAGS, log, tables = self.FLAGS, self.log, self.tables
        log(data)
        log('  Reading {} ...'.format(image_name))
        if nim is None:
            nim = nifti.load(image_name)
        image = nim.get_data()
        if image.ndim != 4:
            log('  {0}: expected a 4-D sequence, found shape {1}. Skip.'.format(image_name, image.shape))
            self.queue.done(data)
            return
        log('  Segmenting full sequence ...')
        t0 = time.time()
        args = tables.subject_args(data_dir, nim, log, truth)
        if sequence_on_device(FLAGS, self.engine, image):
            from . import device_pipeline
            pred, aux = device_pipeline.segment_sequence_device(image, self.engine, FLAGS.batch_slices, return_aux=True, stats=tables.statistics(),
                                                                stat_args=args)
            seg_time = time.time() - t0
            counts, stats, clip, ed_es = aux['counts'], aux['stats'], aux['clip'], None
        else:
            want_prob = tables.confidence is not None       # --confidence_csv: the forward returns the probabilities too
            if forward is None:
                forward = lambda b: self.engine.run(b, want_prob=want_prob)
            host_cells = None
            if want_prob:                                   # confidence.cells_host of every chunk of slices, as the device adds them
                from . import confidence
                X2, Y2, x_pre, _, y_pre, _ = pipeline.pad_amounts(*image.shape[:2])
                plain = forward

                def forward(batch):
                    nonlocal host_cells
                    out = plain(batch)
                    if 'prob' not in out:
                        raise ValueError('--confidence_csv: the forward of the host path has to return prob next to pred')
                    if host_cells is None:
                        host_cells = confidence.HostCells(image.shape, (X2, Y2, x_pre, y_pre), out['prob'].shape[-1])
                    host_cells.add(out['prob'], out['pred'])
                    return out
            pred = pipeline.segment_sequence(image, forward, FLAGS.batch_slices, bool(getattr(FLAGS, 'numpy1_casting', False)))   # clips `image` in place
            seg_time = time.time() - t0
            (counts, stats), clip, ed_es = tables.from_labels(pred, args, tables.n_class), None, pipeline.pick_ed_es(pred, self.seq, FLAGS.seg4)
            if host_cells is not None:
                stats['confidence'] = host_cells.cells
        self.finish(item, nim, seg_time, pred, counts, stats, clip, lambda k: image[:, :, :, k], ed_es=ed_es, announce=False)

    def pipelined(self):
        """Subjects overlapped: reader threads decompress the next files into pinned staging buffers, the GPU thread (this one)
        keeps up to two subjects in flight on three streams (subject_pipeline.SubjectPipeline), writer threads expand the uint8
        labels to the reference's float64 volume, gzip and save.  The log lines of a subject are emitted together when its result
        arrives."""
        import threading
        from . import device_pipeline
        from .subject_pipeline import SubjectPipeline
        FLAGS, tables = self.FLAGS, self.tables
        window = self.start_threads() + 1               # reads allowed to run ahead of the GPU thread
        depth = 3
        # --device_label_gzip: the code set of --label_gzip on the device; 'zlib', the fast path switched off or nothing to save keep the
        # host writer (deploy_network has logged which)
        gz_mode = device_label_gzip_mode(FLAGS)[0]
        if gz_mode:
            self.phases.update(label_gzip_device=0, label_gzip_fallback=0)
        pipes = []                                      # the SubjectPipeline, once the first volume has sized it
        truths = {}                                     # subject -> what its reader got from LabelTables.read_truth
        mk = threading.Lock()

        def alloc(shape, dt):
            if len(shape) == 4 and device_pipeline.device_dtype_ok(dt):
                with mk:
                    if not pipes:                       # sized by the first volume; bigger ones fall back below
                        pipes.append(SubjectPipeline(self.engine, shape, FLAGS.batch_slices, depth=depth, extra_inputs=window, stats=tables.statistics(),
                                                     device_label_gzip=gz_mode))
                try:
                    return pipes[0].stage(shape, dt).array, SubjectPipeline.HEADROOM
                except ValueError:
                    pass
            return np.empty(shape, dt, order='F'), 0

        def read(item):
            handed = []

            def alloc_tracked(shape, dt):
                a, headroom = alloc(shape, dt)
                handed.append(a)
                return a, headroom
            try:
                nim = nifti.load(item[2], alloc=alloc_tracked)
                truths[item[0]] = tables.read_truth(item[1], nim.shape, self.log)    # --score_csv: the second file of the subject, inflated here too
                return nim
            except BaseException:
                for a in handed:                        # a truncated / corrupt file: the pinned buffer goes back to the pool
                    if pipes:
                        pipes[0].release(a)
                raise

        todo = self.walk()
        ahead = deque()                                 # (item, future of its read), in walk order
        inflight = deque()                              # (item, nim, t_submit)

        def top_up():
            while len(ahead) < window:
                item = next(todo, None)
                if item is None:
                    return
                ahead.append((item, self.readers.submit(read, item)))

        def collect():
            item, nim, t0 = inflight.popleft()
            res = pipes[0].collect()
            if gz_mode:
                self.phases['label_gzip_device' if res.gz_blob is not None else 'label_gzip_fallback'] += 1
            self.finish(item, nim, time.time() - t0, res.labels, res.counts, res.stats, res.clip, lambda k: res.image[:, :, :, k], done=res.done,
                        gz_blob=res.gz_blob, label_frames=res.label_frames)

        top_up()
        while ahead:
            item, fut = ahead.popleft()
            nim = fut.result()
            image = nim.get_data()
            if not pipelined_on_device(image) or not pipes or not pipes[0].fits(image):
                while inflight:                         # odd subject: drain, then this thread alone
                    collect()
                truth = truths.pop(item[0], None)
                self.on_this_thread(item, nim=nim, **({} if truth is None else {'truth': truth}))
            else:
                if len(inflight) >= depth - 1:
                    collect()
                pipes[0].submit(image, tables.subject_args(item[1], nim, self.log, truths.pop(item[0], None)), (nim.affine, nim.header['pixdim']) if gz_mode else None)
                inflight.append((item, nim, time.time()))
            top_up()
        while inflight:
            collect()

    def inflate_rounds(self):
        """--device_inflate K: rounds of up to K subjects.  The readers read the files of round r + 1 (a read(), no decoding)
        while the GPU works on round r: one copy of the compressed bytes, one inflate launch, one CRC launch, then subject by
        subject segment_sequence_tensor.  A declined subject takes nifti.load and on_this_thread."""
        from . import device_pipeline
        FLAGS, tables = self.FLAGS, self.tables
        K = int(FLAGS.device_inflate)
        self.start_threads()
        inflater = DeviceInflater(self.engine, max_streams=K)
        phases = self.phases = dict.fromkeys(('read_wait', 'pack', 'h2d', 'inflate_crc', 'results_d2h', 'segment', 'frames_tables', 'writer_wait'), 0.0)
        todo = self.walk()

        def read(item):
            with open(item[2], 'rb') as f:
                return f.read()

        def schedule():
            items = []
            for item in todo:
                items.append((item, self.readers.submit(read, item)))
                if len(items) >= K:
                    break
            return items

        def one(item, got):
            if isinstance(got, Declined):
                return self.on_this_thread(item)
            plan, nim = got.plan, header_image(got.plan)
            t0 = time.time()
            pred, aux = device_pipeline.segment_sequence_tensor(got.volume, plan.dtype, plan.shape, self.engine, FLAGS.batch_slices, return_aux=True,
                                                                stats=tables.statistics(), stat_args=tables.subject_args(item[1], nim, self.log))
            t1 = time.time()
            phases['segment'] += t1 - t0
            # the saved frames are copied back from the device volume
            self.finish(item, nim, t1 - t0, pred, aux['counts'], aux['stats'], aux['clip'], lambda k: frame_to_host(got.volume, k, plan.dtype))
            phases['frames_tables'] += time.time() - t1

        nxt = schedule()
        while nxt:
            cur = nxt
            t0 = time.time()
            blobs = [fut.result() for _, fut in cur]
            phases['read_wait'] += time.time() - t0
            nxt = schedule()                            # the readers fill the next round while the GPU works on this one
            while cur:
                results = inflater.inflate(blobs)
                tm = inflater.timing
                phases['pack'] += tm.get('pack', 0.0)
                phases['h2d'] += tm.get('h2d', 0.0)
                phases['inflate_crc'] += tm.get('inflate_crc', 0.0)
                phases['results_d2h'] += tm.get('device', 0.0) - tm.get('h2d', 0.0) - tm.get('inflate_crc', 0.0)
                inflater.timing = {}
                # what found no room in this launch (max_streams, max_bytes) gets a launch of its own once the others are through;
                # a single subject that no launch can hold is declined for good
                rest = [k for k, got in enumerate(results) if isinstance(got, Declined) and got.reason == NO_ROOM]
                if rest and rest[0] == 0:
                    results[0] = Declined('larger than the output buffer')
                    rest = rest[1:]
                for k, ((item, _), got) in enumerate(zip(cur, results)):
                    if k not in rest:
                        one(item, got)
                cur, blobs = [cur[k] for k in rest], [blobs[k] for k in rest]
            blobs = None
