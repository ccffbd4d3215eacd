"""The tables deploy_network.py derives from a label map while it segments: ``--output_csv`` (ventricular volumes, measures.py),
``--qc_csv`` (the sa / la / atrium gate, qc_gates.py), ``--atrial_csv`` (atrial areas and lengths per frame, atrial.py),
``--score_csv`` (Dice and contour distances against the label file --score_against names, seg_score.py) and ``--confidence_csv`` (how
sure the network was, from the softmax behind the label map: confidence.py).

One ``LabelTables`` is made per run from the flags.  It checks the flags, names the device statistics the run needs of every
label volume (``statistics``), gives the per-subject arguments of those statistics (``subject_args``), turns one subject's class
counts and statistics into rows (``record``) and at the end writes the tables, measuring the subjects an earlier run segmented
from their files (``write``).  Statistics arrive as ``{key: value}`` -- 'qc': qc_gates.stats_host or device_pipeline.GateStats,
'atrial': atrial.frame_stats_host or device_pipeline.AtrialStats, 'score': seg_score.stats_host or device_pipeline.ScoreStats, 'confidence': confidence.cells_host or device_pipeline.ConfidenceStats -- from
the device (SubjectPipeline, segment_sequence_device) or from the host twins (``from_labels``).

``AorticTable`` is the same for deploy_network_ao.py --output_csv (aortic areas and distensibility, measures.py): it checks the
flags, applies the quality control of --aortic_qc / --aortic_qc_full to the class counts and aorta_qc statistics of a subject
(``record``; ``from_labels``: the host twins) and writes the table.  The aortic run never skips a segmented subject: no back-fill."""
import os

from . import aorta_qc, atrial, confidence, measures, nifti, qc_gates, seg_score


class LabelTables:
    def __init__(self, FLAGS, engine=None):
        self.FLAGS = FLAGS
        self.seq, self.seg4 = seq, seg4 = FLAGS.seq_name, FLAGS.seg4
        self.n_class = n_class = None if engine is None else engine.arch.n_class
        self.device = None if engine is None else getattr(engine, 'device', None)
        self.output_csv, self.qc_csv, self.atrial_csv = (getattr(FLAGS, f, '') for f in ('output_csv', 'qc_csv', 'atrial_csv'))
        if self.output_csv and (seq != 'sa' or not FLAGS.process_seq):
            raise ValueError('--output_csv writes the table of short_axis/eval_ventricular_volume.py: it needs --seq_name sa in sequence mode')
        if self.qc_csv:
            if not FLAGS.process_seq:
                raise ValueError('--qc_csv gates the segmentation of a whole sequence: it needs sequence mode (--process_seq)')
            if n_class is not None and n_class < qc_gates.min_classes(seq, seg4):
                raise ValueError('--qc_csv: the gate of --seq_name {0}{1} reads {2} classes, the model has {3}'.format(
                    seq, ' --seg4' if seg4 else '', qc_gates.min_classes(seq, seg4), n_class))
        if self.atrial_csv:
            if seq not in ('la_2ch', 'la_4ch') or seg4 or not FLAGS.process_seq:
                raise ValueError('--atrial_csv measures the atria of long_axis/eval_atrial_volume.py: it needs --seq_name la_2ch or la_4ch '
                                 'without --seg4, in sequence mode')
            if n_class is not None and n_class < qc_gates.min_classes(seq):
                raise ValueError('--atrial_csv: --seq_name {0} has {1} classes, the model has {2}'.format(seq, qc_gates.min_classes(seq), n_class))
        self.score_against, self.score_csv = (getattr(FLAGS, f, '') for f in ('score_against', 'score_csv'))
        if bool(self.score_against) != bool(self.score_csv):
            raise ValueError('--score_against names the label file to score against and --score_csv the table to write: they need each other')
        if self.score_csv and not FLAGS.process_seq:
            raise ValueError('--score_csv scores the segmentation of a whole sequence: it needs sequence mode (--process_seq)')
        self.confidence_csv = getattr(FLAGS, 'confidence_csv', '')
        if self.confidence_csv and not FLAGS.process_seq:
            raise ValueError('--confidence_csv summarises the probabilities of a whole sequence: it needs sequence mode (--process_seq)')
        # subject -> row(s).  The atrial rows carry the gate's verdict: gated, though no --qc_csv is written
        self.volumes = {} if self.output_csv else None
        self.gate = {} if self.qc_csv or self.atrial_csv else None
        self.atrial = {} if self.atrial_csv else None
        self.score = {} if self.score_csv else None
        self.confidence = {} if self.confidence_csv else None
        self._unscored = set()                          # data_dirs whose truth file is absent or refused: logged once, no back-fill
        self._no_prob = set()                           # subjects an earlier run segmented: their probabilities are gone, logged once

    def statistics(self):
        """The device statistics this run needs of every label volume.  Device paths only: device_pipeline loads the HIP library."""
        from . import device_pipeline
        return ([device_pipeline.GateStats(self.seq, self.seg4)] if self.gate is not None else []) + \
            ([device_pipeline.AtrialStats()] if self.atrial is not None else []) + \
            ([device_pipeline.ScoreStats(self.device)] if self.score is not None else []) + \
            ([device_pipeline.ConfidenceStats(getattr(self.FLAGS, 'batch_slices', 128), self.n_class)] if self.confidence is not None else [])

    def subject_args(self, data_dir, nim, log, truth=None):
        """{key: argument} of the statistics that take one per subject.  --atrial_csv: (affine of the long-axis image, long axis), the
        long axis from the short-axis header as eval_atrial_volume.py:45-48 -- absent, and logged, for a subject without sa.nii.gz (the
        reference skips it) or with more than one slice.  --score_csv: the truth volume <subject>/<--score_against>.nii.gz as uint8 --
        absent, and logged, for a subject without the file (the reference's loops ``continue``) or whose file has another shape
        than the image, non-integral values or a label the model does not have.  A subject whose planes the device form does not
        hold gets no argument either: it is scored from its label file when the tables are written.  truth: what ``read_truth`` gave
        for this subject on a reader thread, where the loop has such threads."""
        args = self._atrial_args(data_dir, nim, log)
        if truth is None:
            truth = self.read_truth(data_dir, nim.shape, log)
        if truth is not None:
            from . import device_pipeline
            if device_pipeline.ScoreStats.fits(truth.shape, self.n_class or 2):
                args['score'] = truth
            else:
                log('  {0} x {1} planes are larger than the device scores: scored on the host from the label file.'.format(*truth.shape[:2]))
        return args

    def read_truth(self, data_dir, shape, log):
        """The truth volume of --score_against for a subject whose image has ``shape``, checked, as uint8; None, and logged once, for a
        subject that has none or whose file is refused.  Reads and inflates a file: for the reader threads."""
        if self.score is None or data_dir in self._unscored:
            return None
        name = '{0}/{1}.nii.gz'.format(data_dir, self.score_against)
        if not os.path.exists(name):
            log('  Directory {0} does not contain {1}.nii.gz: nothing to score against.'.format(data_dir, self.score_against))
            self._unscored.add(data_dir)
            return None
        try:
            return seg_score.check_truth(nifti.load(name).get_data(), shape, self.n_class or seg_score.MAX_CLASSES)
        except Exception as e:                          # a shape or label check_truth refuses, a file nifti.load cannot read
            log('  {0} cannot be scored against: {1}. Skip.'.format(name, e))
            self._unscored.add(data_dir)
            return None

    def _atrial_args(self, data_dir, nim, log):
        if self.atrial is None:
            return {}
        sa_name = '{0}/sa.nii.gz'.format(data_dir)
        if not os.path.exists(sa_name):
            log('  Directory {0} does not contain sa.nii.gz: no long axis, no atrial measures.'.format(data_dir))
            return {}
        if nim.shape[2] != 1:
            log('  {0} slices: the atrial measures read a single-slice long-axis sequence. Skip.'.format(nim.shape[2]))
            return {}
        return {'atrial': (nim.affine, atrial.long_axis_from_sa(nifti.load_header(sa_name)['affine']))}

    def from_labels(self, seg, args, n_class):
        """(counts, statistics) of an (X,Y,Z,T) label volume for ``record`` from the host twins, each only if its table is on.  n_class:
        the model's, or None for a label file."""
        counts = None if self.volumes is None else measures.counts_from_labels(seg, n_class or 4)
        stats = {}
        if self.gate is not None:
            stats['qc'] = qc_gates.stats_host(seg, self.seq, self.seg4, n_class)
        if 'atrial' in args:
            stats['atrial'] = atrial.frame_stats_host(seg[:, :, 0, :], self.n_class or qc_gates.min_classes(self.seq), *args['atrial'])
        if 'score' in args:
            stats['score'] = seg_score.stats_host(seg, args['score'], self.n_class or max(2, int(max(seg.max(), args['score'].max())) + 1))
        return counts, stats

    def record(self, data, data_dir, nim, counts, stats, log):
        """The rows of one subject from its per-frame class counts and statistics; nim: its image (affine and voxel size).  The gate comes
        first -- the atrial rows carry its verdict -- and the message of a failing subject is logged the way the reference prints it."""
        if self.volumes is not None and counts is not None:
            self.volumes[data] = measures.sa_row(counts, nim.header['pixdim'])
        if 'qc' in stats:
            name = '{0}/{1}'.format(data_dir, qc_gates.seg_file_name(self.seq, self.seg4))
            self.gate[data] = passed, message = qc_gates.gate_from_stats(stats['qc'], self.seq, self.seg4, name)
            if not passed:
                log(message)
        if 'atrial' in stats:
            self.atrial[data] = atrial.frame_rows(stats['atrial'], nim.affine, nim.header['pixdim'], self.gate[data][0])
        if 'score' in stats:
            self.score[data] = seg_score.frame_rows(stats['score'], nim.header['pixdim'])
        if 'confidence' in stats:
            self.confidence[data] = confidence.frame_rows(stats['confidence'])

    def _back_fill(self, rows, data, log):
        """A subject segmented by an earlier run (skipped by this one) into ``rows`` from its label file, the way the evaluation scripts
        read it: the volumes need image and segmentation (eval_ventricular_volume.py:35), the atria an sa.nii.gz for the long axis."""
        data_dir = os.path.join(self.FLAGS.data_dir, data)
        seg_name = '{0}/{1}_{2}.nii.gz'.format(data_dir, 'seg4' if self.seq == 'la_4ch' and self.seg4 else 'seg', self.seq)
        sa_name = '{0}/sa.nii.gz'.format(data_dir)
        if rows is self.confidence:                     # nothing to measure from: a label file holds no probabilities
            if os.path.exists(seg_name) and data not in self._no_prob:
                log('  {0} was segmented by an earlier run: its probabilities are gone, no confidence rows.'.format(data))
                self._no_prob.add(data)
            return
        if not os.path.exists(seg_name) or (rows is not self.gate and rows is not self.score and not os.path.exists(sa_name)):
            return
        nim = nifti.load(seg_name)
        seg = nim.get_data()
        if rows is self.volumes:
            head = nifti.load_header(sa_name)               # the voxel size is the image's (:40-47)
            self.record(data, data_dir, nifti.NiftiImage(None, head['affine'], head['pixdim']), measures.counts_from_labels(seg, 4), {}, log)
        elif rows is self.score:
            truth = self.read_truth(data_dir, seg.shape, log) if seg.ndim == 4 else None
            if truth is not None:
                self.record(data, data_dir, nim, None, {'score': self.from_labels(seg, {'score': truth}, self.n_class)[1]['score']}, log)
        elif seg.ndim == 4:
            args = self._atrial_args(data_dir, nim, log) if rows is self.atrial else {}
            if args or rows is self.gate:
                stats = self.from_labels(seg, args, None)[1]
                if data in self.gate:
                    del stats['qc']
                self.record(data, data_dir, nim, None, stats, log)

    def write(self, shard_subjects, log):
        """The tables of this worker's subjects, sorted (the order of the evaluation scripts): volumes, atria, scores, confidence, gate -- verdicts the
        atrial table had to produce land in the gate table, logged once.  The gate table is written only with --qc_csv."""
        F = self.FLAGS
        for rows, csv in ((self.volumes, self.output_csv), (self.atrial, self.atrial_csv), (self.score, self.score_csv),
                          (self.confidence, self.confidence_csv), (self.gate, self.qc_csv)):
            if not csv:
                continue
            # with --work_stealing this worker may also have segmented subjects of other shards (their rows are in ``rows``), and
            # another worker may have taken some of this one's: both then hold a row for it -- identical text -- and the merge keeps one
            subjects = sorted(set(shard_subjects) | set(rows))
            for data in subjects:
                if data not in rows:
                    self._back_fill(rows, data, log)
            path = measures.shard_csv_name(csv, F.shard_index, F.num_shards)
            if rows is self.atrial:
                out = [(data, r) for data in subjects for r in rows.get(data, [])]
                atrial.write_frames_csv(path, out)
                log('Atrial measures of {0} frames and labels written to {1}'.format(len(out), path))
                continue
            if rows is self.score:
                out = [(data, r) for data in subjects for r in rows.get(data, [])]
                seg_score.write_csv(path, out)
                log('Scores of {0} frames and labels against {1} written to {2}'.format(len(out), self.score_against, path))
                continue
            if rows is self.confidence:
                out = [(data, r) for data in subjects for r in rows.get(data, [])]
                confidence.write_csv(path, out)
                log('Confidence of {0} frames and labels written to {1}'.format(len(out), path))
                continue
            out = [(data, rows[data]) for data in subjects if data in rows]
            if rows is self.volumes:
                measures.write_csv(path, measures.SA_COLUMNS, out)
                log('Clinical measures of {0} subjects written to {1}'.format(len(out), path))
            else:
                qc_gates.write_csv(path, self.seq, self.seg4, out)
                log('Quality-control verdicts of {0} subjects written to {1}'.format(len(out), path))


class AorticTable:
    def __init__(self, FLAGS):
        self.FLAGS = FLAGS
        self.rows = {} if getattr(FLAGS, 'output_csv', '') else None       # subject -> row; none for one the quality control drops
        self.qc = getattr(FLAGS, 'aortic_qc', True)
        self.qc_full = bool(self.rows is not None and self.qc and getattr(FLAGS, 'aortic_qc_full', False))   # needs the aorta_qc statistics
        self.confidence_csv = getattr(FLAGS, 'confidence_csv', '')
        if self.confidence_csv and not FLAGS.process_seq:
            raise ValueError('--confidence_csv summarises the probabilities of a whole sequence: it needs sequence mode (--process_seq)')
        self.confidence = {} if self.confidence_csv else None           # subject -> confidence.frame_rows
        if self.rows is not None:
            if not FLAGS.process_seq:
                raise ValueError('--output_csv writes the table of aortic/eval_aortic_area.py: it needs sequence mode')
            self.central_pp = measures.read_central_pp(FLAGS.pressure_csv) if getattr(FLAGS, 'pressure_csv', '') else {}

    def _pp(self, data, log):
        """central_pp.loc[int(data)] of eval_aortic_area.py:80; None (no distensibility) when no spreadsheet was given."""
        if not self.central_pp:
            return None
        try:
            key = str(int(data))
        except ValueError:
            key = str(data)
        if key not in self.central_pp:
            # the reference's central_pp.loc[int(data)] raises KeyError here and the whole evaluation stops; this script keeps the areas
            log('  Warning: subject {0} is not in the pressure spreadsheet: distensibility left empty.'.format(data))
        return self.central_pp.get(key, float('nan'))

    def from_labels(self, image, pred):
        """(counts, qc_stats) of a cine and its (X,Y,Z,T) label volume for ``record`` from the host twins, each only if needed."""
        if self.rows is None:
            return None, None
        return measures.counts_from_labels(pred, 3), aorta_qc.stats_host(image, pred) if self.qc_full else None

    def record(self, data, pixdim, counts, qc_stats, log):
        """The subject's table line from its per-frame class counts, or none when the quality control drops it (the script's own
        message is logged); qc_stats: the aorta_qc statistics, needed with --aortic_qc_full."""
        if self.rows is None:
            return
        pp = self._pp(data, log)
        if self.qc:
            ok, why = aorta_qc.aorta_qc_full(counts, qc_stats) if self.qc_full else measures.aorta_qc_from_counts(counts)
            if not ok:
                log(why)
                return
        self.rows[data] = measures.ao_row(counts, pixdim, pp)

    def record_confidence(self, data, cells):
        """--confidence_csv: the subject's lines from its cells (confidence.cells_host or device_pipeline.ConfidenceStats)."""
        if self.confidence is not None and cells is not None:
            self.confidence[data] = confidence.frame_rows(cells)

    def write(self, data_list, log):
        """The table of this worker's subjects in their order; a dropped subject has no line, as eval_aortic_area.py:68-69.  The
        confidence table likewise, whatever the quality control says of a subject."""
        if self.confidence is not None:
            out = [(data, r) for data in data_list for r in self.confidence.get(data, [])]
            path = measures.shard_csv_name(self.confidence_csv, self.FLAGS.shard_index, self.FLAGS.num_shards)
            confidence.write_csv(path, out)
            log('Confidence of {0} frames and labels written to {1}'.format(len(out), path))
        if self.rows is None:
            return
        rows = [(data, self.rows[data]) for data in data_list if data in self.rows]
        path = measures.shard_csv_name(self.FLAGS.output_csv, self.FLAGS.shard_index, self.FLAGS.num_shards)
        measures.write_csv(path, measures.AO_COLUMNS, rows)
        log('Aortic areas of {0} subjects written to {1}'.format(len(rows), path))
