"""gzip NIfTI cines inflated on the GPU, many subjects per launch (include/ukbb_fcn.h: ``ukbb_fcn_inflate_device``).

The host only reads the files: the compressed bytes go up in one copy, one wave decodes one file, one more launch forms every
file's CRC-32, and the voxels are handed to ``device_pipeline.segment_sequence_tensor`` where they lie.  Nothing here decides
whether a file is valid: a subject that ``plan_subject`` / ``gzip_member_layout`` / ``DeviceInflater`` declines -- for whatever
reason: scaled or big-endian voxels, several gzip members, a stream the strict decoder refuses, a byte count, ISIZE or CRC-32
that disagrees -- is read by ``nifti.load``, which accepts or raises exactly as it always did.

No reference counterpart (it leaves gzip to nibabel, common/deploy_network.py:80-83).
"""
import struct
import zlib
from collections import namedtuple

import numpy as np

from . import nifti

Plan = namedtuple('Plan', 'shape dtype vox_offset affine pixdim header total')
Inflated = namedtuple('Inflated', 'volume plan')          # volume: 4-D device tensor (X,Y,Z,T), Fortran strides, valid until the next inflate()
Declined = namedtuple('Declined', 'reason')
NO_ROOM = 'no room in this launch'                        # the only reason that says nothing about the file: ask again in a launch of its own


def _head(blob):
    """The first 352 inflated bytes of a .gz file image, or None (as nifti._load_gz_whole takes them)."""
    try:
        head = zlib.decompressobj(31).decompress(bytes(blob[:1 << 16]), 352)
    except zlib.error:
        return None
    return head if len(head) >= 352 else None


def plan_subject(blob):
    """Header fields of a ``.nii.gz`` file image and the size its inflated content must have (``vox_offset + nbytes``), or None
    unless the voxels are native-endian, unscaled, 4-D and of a dtype the device pre-processing takes."""
    from .device_pipeline import device_dtype_ok
    head = _head(blob)
    if head is None:
        return None
    try:
        shape, dt, off, scale, affine, pixdim, hdr = nifti._parse_header(head, '<memory>')
    except ValueError:
        return None
    if scale is not None or not dt.isnative or len(shape) != 4 or min(shape) < 1 or not device_dtype_ok(dt):
        return None
    return Plan(shape, dt, off, affine, pixdim, hdr, off + int(np.prod(shape, dtype=np.int64)) * dt.itemsize)


def gzip_member_layout(blob, expect_size=None):
    """``(deflate_offset, deflate_len, crc32, isize)`` of a single-member gzip file image (RFC 1952): where its raw deflate stream
    lies and what its trailer promises.  FEXTRA, FNAME and FCOMMENT are skipped.  None for FHCRC, reserved flag bits, a method
    other than 8, and whenever the trailer -- the last 8 bytes in front of optional zero padding -- does not announce
    ``expect_size`` bytes (default: the size the NIfTI header at the start of the content implies): a second member or trailing
    bytes that are not padding cannot be found without decoding, but they put something else where ISIZE is looked for.  The
    caller still checks the decoded byte count and CRC-32."""
    blob = memoryview(blob).cast('B')
    n = len(blob)
    if n < 18 or blob[0] != 0x1f or blob[1] != 0x8b or blob[2] != 8:
        return None
    flg = blob[3]
    if flg & 0xe2:                                            # reserved bits, or FHCRC (left to the host reader)
        return None
    p = 10
    if flg & 4:                                               # FEXTRA
        if n - p < 2:
            return None
        p += 2 + (blob[p] | (blob[p + 1] << 8))
    for f in (8, 16):                                         # FNAME, FCOMMENT: zero-terminated
        if flg & f:
            while p < n and blob[p] != 0:
                p += 1
            p += 1
    if p + 8 > n:
        return None
    if expect_size is None:
        plan = plan_subject(blob)
        if plan is None:
            return None
        expect_size = plan.total
    end = n
    while True:                                               # the trailer ends the file, or zero padding follows it
        if end - 8 < p + 1:
            return None
        crc, isize = struct.unpack('<II', blob[end - 8:end])
        if isize == (expect_size & 0xffffffff):
            return p, end - 8 - p, crc, isize
        if blob[end - 1] != 0:
            return None
        end -= 1


class _HeaderImage(nifti.NiftiImage):
    """What nifti.load returns, without voxels on the host: affine, header['pixdim'], shape."""

    def __init__(self, plan):
        super().__init__(None, plan.affine, plan.pixdim, plan.header)
        self._shape = plan.shape

    @property
    def shape(self):
        return self._shape

    def get_data(self):
        raise RuntimeError('the voxels of this subject are on the device only')


def header_image(plan):
    return _HeaderImage(plan)


class DeviceInflater:
    """Inflates a list of ``.nii.gz`` file images on ``engine``'s device: pinned staging for the compressed bytes, one device buffer
    for them and one for the outputs (grown to what a call needs, at most ``max_bytes``), each volume's first voxel 16-byte aligned.
    ``inflate(blobs)`` returns per blob ``Inflated(volume, plan)`` or ``Declined(reason)``; the volumes are views of the output
    buffer and hold until the next call.  Once a volume does not fit ``max_streams`` / ``max_bytes`` it and every later blob of the
    call come back as ``Declined(NO_ROOM)``: hand those to a further call."""

    def __init__(self, engine, max_streams=256, max_bytes=1 << 34):
        import torch
        self.torch = torch
        self.dev = torch.device('cuda', engine.device)
        self.max_streams, self.max_bytes = int(max_streams), int(max_bytes)
        self._pin = self._src = self._dst = None
        self.timing = {}                                      # seconds of the last call, see inflate()

    def _room(self, name, nbytes, pinned=False):
        buf = getattr(self, name)
        if buf is None or buf.numel() < nbytes:
            nbytes = max(int(nbytes), 1 << 20)
            buf = self.torch.empty(nbytes, dtype=self.torch.uint8, pin_memory=True) if pinned else \
                self.torch.empty(nbytes, dtype=self.torch.uint8, device=self.dev)
            setattr(self, name, buf)
        return buf

    def inflate(self, blobs):
        import time
        from . import _lib
        torch = self.torch
        t0 = time.time()
        out = [None] * len(blobs)
        todo = []                                             # (index, plan, layout, src_off, dst_off)
        src_end = dst_end = 0
        full = False
        for i, blob in enumerate(blobs):
            plan = plan_subject(blob)
            if plan is None:
                out[i] = Declined('not a native-endian, unscaled 4-D volume of a device dtype')
                continue
            lay = gzip_member_layout(blob, plan.total)
            if lay is None:
                out[i] = Declined('not a single plain gzip member of the size the header implies')
                continue
            dst_off = ((dst_end + 15) & ~15) + (-plan.vox_offset) % 16      # first voxel 16-byte aligned
            if full or len(todo) >= self.max_streams or dst_off + plan.total > self.max_bytes:
                full = True                                   # and so is everything behind it: the subjects keep their order
                out[i] = Declined(NO_ROOM)
                continue
            src_off = (src_end + 15) & ~15
            todo.append((i, plan, lay, src_off, dst_off))
            src_end, dst_end = src_off + lay[1], dst_off + plan.total
        if not todo:
            return out
        n = len(todo)
        pin = self._room('_pin', src_end, pinned=True)
        pin_np = pin.numpy()
        tab = (_lib.GzStream * n)()
        for k, (i, plan, lay, src_off, dst_off) in enumerate(todo):
            pin_np[src_off:src_off + lay[1]] = np.frombuffer(blobs[i], np.uint8, lay[1], lay[0])
            tab[k].src_off, tab[k].src_len, tab[k].dst_off, tab[k].dst_cap = src_off, lay[1], dst_off, plan.total
        t1 = time.time()
        with torch.cuda.device(self.dev):
            src = self._room('_src', src_end)
            dst = self._room('_dst', dst_end)
            stream = torch.cuda.current_stream(self.dev).cuda_stream
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            src[:src_end].copy_(pin[:src_end], non_blocking=True)
            ev[1].record()
            written = torch.empty(n, dtype=torch.int64, device=self.dev)
            crc = torch.empty(n, dtype=torch.int32, device=self.dev)
            _lib.check(_lib.lib.ukbb_fcn_inflate_device(src.data_ptr(), dst.data_ptr(), tab, n, written.data_ptr(), crc.data_ptr(), stream),
                       'ukbb_fcn_inflate_device')
            ev[2].record()
            written_h = written.cpu().numpy()
            crc_h = crc.cpu().numpy().view(np.uint32)
        # h2d and inflate_crc from events on the stream (the one entry point issues the inflate and the CRC launch back to back);
        # device = the host's wait for all of it, the copy back of the per-stream results included
        self.timing = {'pack': t1 - t0, 'device': time.time() - t1, 'h2d': ev[0].elapsed_time(ev[1]) / 1e3,
                       'inflate_crc': ev[1].elapsed_time(ev[2]) / 1e3, 'streams': n, 'src_bytes': src_end, 'dst_bytes': dst_end}
        for k, (i, plan, lay, src_off, dst_off) in enumerate(todo):
            if written_h[k] < 0:
                out[i] = Declined('the device decoder refused the stream (%d)' % written_h[k])
            elif written_h[k] != plan.total:
                out[i] = Declined('%d bytes inflated, the header implies %d' % (written_h[k], plan.total))
            elif int(crc_h[k]) != lay[2]:
                out[i] = Declined('CRC-32 mismatch')
            else:
                out[i] = Inflated(self._view(dst, dst_off + plan.vox_offset, plan), plan)
        return out

    def _view(self, dst, first, plan):
        torch = self.torch
        tdt = {'float32': torch.float32, 'uint8': torch.uint8, 'int16': torch.int16, 'uint16': torch.int16}[plan.dtype.name]
        X, Y, Z, T = plan.shape
        flat = dst[first:first + X * Y * Z * T * plan.dtype.itemsize].view(tdt)
        return flat.as_strided((X, Y, Z, T), (1, X, X * Y, X * Y * Z))


def frame_to_host(volume, k, dtype):
    """Frame k of a device volume as a host array of the file's dtype (a uint16 volume is an int16 tensor on the device)."""
    a = volume[:, :, :, k].cpu().numpy()
    return a.view(np.uint16) if np.dtype(dtype) == np.uint16 else a
