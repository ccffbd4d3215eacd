"""Subject-level software pipeline of the sequence loop (common/deploy_network.py:80-131) on one GPU.

``device_pipeline.segment_sequence_device`` runs one subject start to finish: pageable H2D copy of the 80 MB volume,
percentiles, pack, forward, unpack, D2H, float64 expansion -- 54 ms per 500-slice subject in round 1 for 11 ms of
network time.  Here consecutive subjects overlap on three HIP streams with pinned staging buffers:

    copy-in stream    H2D of subject k+1 (pinned -> HBM) and its exact percentiles (radix select)
    compute stream    clip / rescale / pad / transpose, the FCN forward over all T*Z slices, label unpack + class counts of subject k
    copy-out stream   D2H of subject k-1's uint8 label volume (20 MB instead of 160 MB of float64) and counts

``device_label_gzip='small' | 'fast'`` (opt-in): the label volume is deflated on the compute stream behind the statistics
(ukbb_fcn_gzip_labels_device: the very bytes nifti.save would write for the float64 volume) and the copy-out stream carries the
gzip member -- d_out to its capacity, the host path's first guess, so that no host wait sits between the chain and the copy --
instead of the label volume; ``Result.label_frames`` fetches the two frames the loop saves.  A subject the encoder declines, or
whose member is larger than nifti.NOISE_FRACTION of the raw stream ('small': where the host writer would try zlib too), comes
back with ordinary ``labels``.

Slots (device buffers + pinned label buffer + events) rotate round-robin; a slot is reused only after its result has
been collected.  Pinned INPUT buffers form a pool of their own so that reader threads can decompress the next files
straight into them (``stage()`` + ``nifti.load(path, alloc=...)``) while earlier subjects are still on the GPU; a
buffer stays with its subject until the result has been taken (the ED / ES image frames the reference saves are cut
from it, deploy_network.py:145) and returns to the pool on ``Result.done()``.  The float64 volume the reference writes (deploy_network.py:92,136) is produced by whoever saves the file
(``labels_as_float64``), off this thread.  Results are identical to ``pipeline.segment_sequence`` (tests).

PyTorch is used for what the task allows it for: pinned / device memory, streams and events.
"""
import queue

import numpy as np

from .device_pipeline import device_dtype_ok, device_percentiles, forward_and_unpack, pack_rescaled, stat_skipped
from .pipeline import pad_amounts


class _Slot:
    pass


GZ_DATATYPE, GZ_ITEMSIZE, GZ_PREFIX_LEN = 64, 8, 352      # seg_{seq}.nii.gz: float64 voxels behind the NIfTI-1 header


def label_gzip_capacity(n_vox, itemsize=GZ_ITEMSIZE, prefix_len=GZ_PREFIX_LEN):
    """The output capacity nifti.save tries first for a label volume (nifti._save_labels_gz): what the device encoder gets."""
    return max(1 << 16, prefix_len * 2 + n_vox * itemsize // 24)


def label_gzip_max_runs(n_vox):
    """Run-table entries per slot: a segmentation has a handful of runs per image row, far fewer than voxels / 8 (12 bytes of scratch
    each); a volume with more is noise and falls back."""
    return max(4096, n_vox // 8)


class Staged:
    """A pinned input buffer on loan from the pipeline: ``array`` is its (X,Y,Z,T) Fortran-ordered view (float32, uint8,
    int16 or uint16)."""

    def __init__(self, array, buf):
        self.array, self.buf = array, buf


class SubjectPipeline:
    HEADROOM = 4096                                         # bytes of writable pinned memory in front of every staged array

    def __init__(self, engine, max_shape, batch_slices=128, depth=3, thres=(1, 99), extra_inputs=2, pinned_inputs=True, stats=(),
                 device_label_gzip=None):
        """max_shape: largest (X, Y, Z, T) expected (buffers are sized for it; larger volumes re-allocate).
        stats: label statistics (the classes of device_pipeline with sizes / launch / decode) to compute from every subject's labels on the compute
        stream, right behind the unpack; ``Result.stats`` holds them by key.  One that takes a per-subject argument is computed for
        the subjects submitted with it (``submit(image, {key: arg})``).
        extra_inputs: pinned input buffers beyond ``depth`` (one per reader thread that may hold one).
        pinned_inputs=False: no pinned input pool at all -- for cohorts whose volumes are produced on the device
        (``submit_generated``; ``stage`` / ``submit`` of host arrays then block forever and must not be used).
        device_label_gzip: None, or the code set ('small' = dynamic Huffman, 'fast' = fixed) with which subjects submitted with a
        ``gz_header`` get their float64 label file deflated on the device."""
        import torch
        if device_label_gzip not in (None, 'small', 'fast'):
            raise ValueError("device_label_gzip: None, 'small' or 'fast' (got %r)" % (device_label_gzip,))
        self.device_label_gzip = device_label_gzip
        self.torch = torch
        self.engine = engine
        self.batch_slices = int(batch_slices)
        self.thres = tuple(thres)
        self.stats = tuple(stats)
        self.dev = torch.device('cuda', engine.device)
        self.s_in = torch.cuda.Stream(self.dev)
        self.s_cmp = torch.cuda.Stream(self.dev)
        self.s_out = torch.cuda.Stream(self.dev)
        self.depth = int(depth)
        self.slots = [self._make_slot(max_shape) for _ in range(self.depth)]
        self._next = 0
        self._inflight = []                                   # slots in submission order
        self._in_cap = int(np.prod(max_shape))
        self._in_free = queue.Queue()
        for _ in range(self.depth + int(extra_inputs) if pinned_inputs else 0):
            # HEADROOM bytes in front of every buffer: nifti.load's whole-file decoder writes the 352-byte NIfTI header there and the
            # voxels straight behind it, i.e. into the array stage() hands out (the view keeps the whole allocation alive)
            self._in_free.put(torch.empty(self._in_cap + self.HEADROOM // 4, dtype=torch.float32, pin_memory=True)[self.HEADROOM // 4:])
        import threading
        self._lock = threading.Lock()
        self._staged = {}                                     # id(array) -> Staged, for arrays handed out by stage()

    # ---- buffers ----------------------------------------------------------------------------------
    def _make_slot(self, shape):
        torch = self.torch
        X, Y, Z, T = shape
        X2, Y2 = pad_amounts(X, Y)[:2]
        s = _Slot()
        s.cap_vox, s.cap_pix = X * Y * Z * T, X2 * Y2 * Z * T
        s.pin_lab = torch.empty(s.cap_vox, dtype=torch.uint8, pin_memory=True)
        s.pin_cnt = torch.empty(T * 16, dtype=torch.int64, pin_memory=True)
        s.d_vol = torch.empty(s.cap_vox, dtype=torch.float32, device=self.dev)
        s.d_batch = torch.empty(s.cap_pix, dtype=torch.float32, device=self.dev)
        s.d_pred = torch.empty(s.cap_pix, dtype=torch.int32, device=self.dev)
        s.d_lab = torch.empty(s.cap_vox, dtype=torch.uint8, device=self.dev)
        s.d_cnt = torch.empty(T * 16, dtype=torch.int64, device=self.dev)
        s.stats = []                                          # (statistic, d_work, d_out, pin_out, capacity)
        for stat in self.stats:
            cap = stat.sizes(shape, 16)                       # n_class <= 16, as d_cnt
            s.stats.append((stat, torch.empty(cap[0], dtype=torch.int32, device=self.dev), torch.empty(cap[1], dtype=torch.int32, device=self.dev),
                            torch.empty(cap[1], dtype=torch.int32, pin_memory=True), cap))
        s.ev_in, s.ev_cmp, s.ev_out = torch.cuda.Event(), torch.cuda.Event(), torch.cuda.Event()
        s.busy = False
        s.serial = 0
        s.gz = False
        if self.device_label_gzip:
            from ._lib import lib
            s.gz_cap = (label_gzip_capacity(s.cap_vox) + 3) & ~3
            s.gz_max_runs = label_gzip_max_runs(s.cap_vox)
            s.d_gz = torch.empty(s.gz_cap, dtype=torch.uint8, device=self.dev)
            s.pin_gz = torch.empty(s.gz_cap, dtype=torch.uint8, pin_memory=True)
            s.d_gz_scratch = torch.empty(int(lib.ukbb_fcn_gzip_labels_device_scratch(s.cap_vox, s.gz_max_runs)), dtype=torch.uint8, device=self.dev)
            s.d_gz_len = torch.zeros(1, dtype=torch.int64, device=self.dev)
            s.pin_gz_len = torch.zeros(1, dtype=torch.int64, pin_memory=True)
            s.d_prefix = torch.empty(GZ_PREFIX_LEN, dtype=torch.uint8, device=self.dev)
            s.pin_prefix = torch.empty(GZ_PREFIX_LEN, dtype=torch.uint8, pin_memory=True)
        return s

    def stage(self, shape, dtype=np.float32, timeout=None):
        """Borrow a pinned input buffer (thread-safe; blocks while all are in use): ``Staged.array`` is a Fortran-ordered
        (X,Y,Z,T) view of the dtype to fill -- e.g. ``nifti.load(path, alloc=lambda sh, dt: pipe.stage(sh, dt).array)`` makes
        the file decompress straight into pinned memory.  Pass the Staged object (or its array) to ``submit``.
        dtype: float32, uint8, int16 or uint16 (the pool's buffers viewed as bytes: an int16 volume fills, and copies to the
        device, half the bytes of a float32 one)."""
        dtype = np.dtype(dtype)
        if not device_dtype_ok(dtype):
            raise TypeError('the device pipeline is exact for float32, uint8, int16 and uint16 volumes only (got %s)' % dtype)
        n = int(np.prod(shape))
        if len(shape) != 4 or n > self._in_cap:
            raise ValueError('volume %s does not fit the staging buffers sized for %d voxels' % (shape, self._in_cap))
        buf = self._in_free.get(timeout=timeout)            # returned by Result.done()
        st = Staged(buf.numpy().view(np.uint8)[:n * dtype.itemsize].view(dtype).reshape(shape, order='F'), buf)
        with self._lock:
            self._staged[id(st.array)] = st
        return st

    def fits(self, image):
        """Does a volume fit the pinned staging buffers (``stage`` raises for one that does not)?"""
        return image.size <= self._in_cap

    def release(self, array):
        """Give back a buffer ``stage()`` handed out that will not be submitted after all (its file failed to load)."""
        with self._lock:
            st = self._staged.pop(id(array), None)
        if st is not None:
            self._in_free.put(st.buf)
            return True
        return False

    @staticmethod
    def _fits(slot, shape):
        """Do the slot's buffers -- volume, batch, counts and every statistic's -- hold a subject of this shape?"""
        X, Y, Z, T = shape
        X2, Y2 = pad_amounts(X, Y)[:2]
        return (X * Y * Z * T <= slot.cap_vox and X2 * Y2 * Z * T <= slot.cap_pix and T * 16 <= slot.pin_cnt.numel()
                and all(need <= have for stat, _, _, _, cap in slot.stats for need, have in zip(stat.sizes(shape, 16), cap)))

    def _acquire(self, shape):
        slot = self.slots[self._next]
        if slot.busy:
            raise RuntimeError('pipeline full: collect() a result before staging another subject (depth %d)' % self.depth)
        if not self._fits(slot, shape):
            self.torch.cuda.synchronize(self.dev)
            self.slots[self._next] = slot = self._make_slot(shape)
        return slot

    # ---- submit / collect -----------------------------------------------------------------------------
    def submit(self, image, stat_args=None, gz_header=None):
        """Enqueue one (X,Y,Z,T) float32 / uint8 / int16 / uint16 volume: a ``Staged`` object / the array ``stage()`` handed
        out (used in place), or any other array (copied into a pinned buffer first: one host memcpy).  Returns once the exact
        percentiles of the volume are known (the copy-in stream is waited for, the compute stream is not).  Subjects of
        different dtypes may follow each other: the select and pack kernels are chosen per subject.
        stat_args = {key: arg}: this subject's arguments of the statistics that take one.
        gz_header = (affine, pixdim) of the label file (pipelines made with device_label_gzip): deflate this subject's float64 label
        volume on the device; its Result then carries ``gz_blob`` in place of ``labels``."""
        if gz_header is not None and not self.device_label_gzip:
            raise ValueError('this pipeline was made without device_label_gzip')
        unknown = set(stat_args or ()) - {stat.key for stat in self.stats}
        if unknown:
            raise ValueError('this pipeline was made without the statistics %s' % sorted(unknown))
        if isinstance(image, Staged):
            st = image
            with self._lock:
                self._staged.pop(id(st.array), None)
        else:
            with self._lock:
                st = self._staged.pop(id(image), None)
            if st is None:
                if image.ndim != 4 or not device_dtype_ok(image.dtype):
                    raise TypeError('expected a 4-D float32, uint8, int16 or uint16 (X,Y,Z,T) volume')
                st = self.stage(image.shape, image.dtype)
                with self._lock:
                    self._staged.pop(id(st.array), None)
                st.array[...] = image
        self._enqueue(st.array.shape, st, None, stat_args, gz_header)

    def submit_generated(self, shape, fill):
        """Enqueue one (X,Y,Z,T) float32 volume that is PRODUCED ON THE DEVICE: ``fill(d_ptr, n, stream)`` enqueues, on the copy-in
        stream it is given, whatever writes the n voxels (x fastest, like the file) to device address d_ptr -- it takes the place
        of the H2D copy; everything behind it (percentiles, pack, forward, unpack, labels to pinned host memory) is the same code.
        The Result of such a subject has no ``image``."""
        if len(shape) != 4:
            raise ValueError('expected an (X,Y,Z,T) shape, got %s' % (shape,))
        self._enqueue(tuple(int(v) for v in shape), None, fill)

    def _enqueue(self, shape, st, fill, stat_args=None, gz_header=None):
        torch = self.torch
        X, Y, Z, T = shape
        slot = self._acquire(shape)
        n = X * Y * Z * T
        slot.busy = True
        slot.serial += 1
        slot.gz = gz_header is not None
        if slot.gz:
            from . import nifti
            prefix = nifti.header_prefix(shape, gz_header[0], gz_header[1], np.float64)
            slot.pin_prefix.numpy()[:] = np.frombuffer(prefix, np.uint8)
        slot.shape = shape
        slot.staged = st
        slot.live = [entry for entry in slot.stats if not stat_skipped(entry[0], stat_args)]
        self._next = (self._next + 1) % self.depth
        n_class = self.engine.arch.n_class
        X2, Y2, x_pre, _, y_pre, _ = pad_amounts(X, Y)
        dtype = np.dtype(np.float32) if st is None else st.array.dtype
        with torch.cuda.stream(self.s_in):
            if st is not None:
                nb = n * dtype.itemsize                     # an int16 volume copies half the bytes of a float32 one
                slot.d_vol.view(torch.uint8)[:nb].copy_(st.buf.view(torch.uint8)[:nb], non_blocking=True)
            else:
                # the slot's previous subject was collected (its pack kernel, the last reader of d_vol, has finished long ago)
                fill(slot.d_vol.data_ptr(), n, self.s_in.cuda_stream)
            if slot.gz:
                slot.d_prefix.copy_(slot.pin_prefix, non_blocking=True)
            # exact np.percentile(volume, (1, 99)): two neighbouring order statistics per percentile from the device
            # (radix select on the voxel type; synchronises the copy-in stream only), numpy's own interpolation on the host
            lo, hi = device_percentiles(slot.d_vol, self.thres, self.s_in.cuda_stream, dtype, n=n)
            slot.ev_in.record(self.s_in)
        slot.clip = (lo, hi)
        with torch.cuda.stream(self.s_cmp):
            self.s_cmp.wait_event(slot.ev_in)
            cs = self.s_cmp.cuda_stream
            # element strides of the Fortran-ordered (X,Y,Z,T) volume
            pack_rescaled(slot.d_vol.data_ptr(), dtype, (X, Y, Z, T), (1, X, X * Y, X * Y * Z), lo, hi, (X2, Y2, x_pre, y_pre),
                          slot.d_batch.data_ptr(), cs)
            # the statistics of the probabilities run chunk by chunk behind the forward, adding into outputs zeroed here
            per_chunk = [entry for entry in slot.live if entry[0].per_chunk]
            for stat, _, d_out, _, _ in per_chunk:
                d_out[:stat.sizes(shape, n_class)[1]].zero_()
            forward_and_unpack(self.engine, slot.d_batch.data_ptr(), slot.d_pred.data_ptr(), shape, (X2, Y2, x_pre, y_pre), self.batch_slices,
                               slot.d_lab.data_ptr(), slot.d_cnt.data_ptr(), cs,
                               [(stat, d_work.data_ptr(), d_out.data_ptr()) for stat, d_work, d_out, _, _ in per_chunk])
            for stat, d_work, d_out, _, _ in slot.live:
                if stat.per_chunk:
                    continue
                stat.launch(slot.d_lab.data_ptr(), shape, n_class, d_work.data_ptr(), d_out.data_ptr(), cs, (stat_args or {}).get(stat.key))
            if slot.gz:
                from ._lib import check, lib
                slot.gz_out_cap = label_gzip_capacity(n)        # this subject's own first guess, as on the host
                check(lib.ukbb_fcn_gzip_labels_device(slot.d_lab.data_ptr(), n, GZ_DATATYPE, slot.d_prefix.data_ptr(), GZ_PREFIX_LEN,
                                                      0 if self.device_label_gzip == 'fast' else 1, slot.d_gz.data_ptr(), slot.gz_out_cap,
                                                      slot.d_gz_scratch.data_ptr(), slot.gz_max_runs, slot.d_gz_len.data_ptr(), cs),
                      'ukbb_fcn_gzip_labels_device')
            slot.ev_cmp.record(self.s_cmp)
        with torch.cuda.stream(self.s_out):
            self.s_out.wait_event(slot.ev_cmp)
            if slot.gz:                                       # the member to its capacity (no host wait for its length), not the labels
                slot.pin_gz_len.copy_(slot.d_gz_len, non_blocking=True)
                slot.pin_gz[:slot.gz_out_cap].copy_(slot.d_gz[:slot.gz_out_cap], non_blocking=True)
            else:
                slot.pin_lab[:n].copy_(slot.d_lab[:n], non_blocking=True)
            slot.pin_cnt[:T * n_class].copy_(slot.d_cnt[:T * n_class], non_blocking=True)
            for stat, _, d_out, pin_out, _ in slot.live:
                n_out = stat.sizes(shape, n_class)[1]         # this shape's own count, not the slot's capacity
                pin_out[:n_out].copy_(d_out[:n_out], non_blocking=True)
            slot.ev_out.record(self.s_out)
        self._inflight.append(slot)

    def pending(self):
        return len(self._inflight)

    def collect(self, copy=True):
        """Oldest submitted subject -> Result (labels uint8 (X,Y,Z,T), counts int64 [T, n_class], clip (lo, hi), stats = {key: the
        decoded statistic}, image = the staged input volume).  Call ``Result.done()`` when the image is no longer needed.
        copy=False: ``labels`` is a view of the slot's pinned buffer, valid only until ``depth`` more subjects have been submitted
        (for callers that consume or drop it at once)."""
        slot = self._inflight.pop(0)
        slot.ev_out.synchronize()
        X, Y, Z, T = slot.shape
        n = X * Y * Z * T
        n_class = self.engine.arch.n_class
        blob = None
        if slot.gz:
            from . import nifti
            got = int(slot.pin_gz_len[0])
            small = self.device_label_gzip == 'small'
            if 0 < got <= slot.gz_out_cap and not (small and got > nifti.NOISE_FRACTION * (GZ_PREFIX_LEN + n * GZ_ITEMSIZE)):
                blob = bytes(memoryview(slot.pin_gz.numpy())[:got])
            else:                                              # declined, or where the host writer would try zlib as well: the labels after all
                with self.torch.cuda.stream(self.s_out):
                    slot.pin_lab[:n].copy_(slot.d_lab[:n], non_blocking=True)
                    slot.ev_out.record(self.s_out)
                slot.ev_out.synchronize()
        lab = None
        if blob is None:
            lab = slot.pin_lab.numpy()[:n].reshape(slot.shape, order='F')
            if copy:
                lab = lab.copy(order='F')
        cnt = slot.pin_cnt.numpy()[:T * n_class].reshape(T, n_class).copy()
        stats = {stat.key: stat.decode(pin_out.numpy()[:stat.sizes(slot.shape, n_class)[1]], slot.shape, n_class, cnt)
                 for stat, _, _, pin_out, _ in slot.live}
        st, slot.staged = slot.staged, None
        slot.busy = False
        return Result(self, lab, cnt, slot.clip, st, stats, blob, (slot, slot.serial) if blob is not None else None)

    def run(self, volumes):
        """Generator: segment an iterable of volumes with up to depth-1 subjects in flight; yields Results in order
        (each already ``done()``: the staged image of a result is only valid until the next one is requested)."""
        last = None
        for v in volumes:
            if self.pending() >= self.depth - 1:
                if last is not None:
                    last.done()
                last = self.collect()
                yield last
            self.submit(v)
        while self.pending():
            if last is not None:
                last.done()
            last = self.collect()
            yield last
        if last is not None:
            last.done()


class Result:
    def __init__(self, pipe, labels, counts, clip, staged, stats, gz_blob=None, slot=None):
        """gz_blob: the finished seg_{seq}.nii.gz of a subject deflated on the device; ``labels`` is then None and the labels stay
        in the slot's device buffer, from where ``label_frames`` copies single frames."""
        self._pipe, self.labels, self.counts, self.clip, self._staged, self.stats = pipe, labels, counts, clip, staged, stats
        self.gz_blob, self._slot = gz_blob, slot

    def label_frames(self, *frames):
        """uint8 (X,Y,Z) label frames k, ... of a subject that carries ``gz_blob``, copied from the slot's device labels.  Valid
        until ``depth`` more subjects have been submitted (the slot is then reused: RuntimeError)."""
        if self._slot is None:
            raise RuntimeError('label_frames: this result holds its labels')
        slot, serial = self._slot
        if slot.serial != serial:
            raise RuntimeError('label_frames: the slot has been reused (depth more subjects were submitted)')
        X, Y, Z, T = slot.shape
        m = X * Y * Z
        torch = self._pipe.torch
        with torch.cuda.stream(self._pipe.s_out):
            got = [slot.d_lab[int(k) * m:(int(k) + 1) * m].to('cpu', non_blocking=False) for k in frames]
        return [g.numpy().reshape((X, Y, Z), order='F') for g in got]

    @property
    def image(self):
        """The input volume as staged (NOT clipped; the reference's saved frames are, see device_pipeline.clip_like_reference);
        None for a subject generated on the device."""
        return None if self._staged is None else self._staged.array

    def done(self):
        if self._staged is not None:
            self._pipe._in_free.put(self._staged.buf)
            self._staged = None


def labels_as_float64(lab_u8):
    """The array the reference saves as seg_{seq}.nii.gz: np.zeros(image.shape) filled with int32 predictions
    (deploy_network.py:92,116) = float64 labels."""
    out = np.zeros(lab_u8.shape)
    out[...] = lab_u8
    return out
