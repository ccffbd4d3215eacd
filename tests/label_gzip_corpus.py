"""Label volumes for the device label-gzip tests (tests/test_device_label_gzip*.py): the smallest inputs at which each piece of
the encoder can go wrong, and the host writer they are all compared with."""
import zlib

import numpy as np

DATATYPES = {2: '<u1', 4: '<i2', 8: '<i4', 16: '<f4', 64: '<f8'}
FIXED, DYNAMIC = 0, 1
NO_ROOM, TOO_MANY_RUNS = -4, -5
PREFIX = bytes((i * 7 + 3) & 0xff for i in range(348)) + b'\x00\x00\x00\x00'      # 352 bytes, as a NIfTI-1 header has
# ... and one as nifti.save writes it: mostly zeros, so that the dynamic code gives the zero byte one or two bits
HEADER_LIKE = bytearray(352)
HEADER_LIKE[0:4] = (348).to_bytes(4, 'little')
HEADER_LIKE[40:50] = np.array([4, 192, 208, 10, 50], '<i2').tobytes()
HEADER_LIKE[70:74] = np.array([64, 64], '<i2').tobytes()
HEADER_LIKE[76:92] = np.array([1, 1.8, 1.8, 10], '<f4').tobytes()
HEADER_LIKE[108:112] = np.array([352], '<f4').tobytes()
HEADER_LIKE[344:348] = b'n+1\0'
HEADER_LIKE = bytes(HEADER_LIKE)
PREFIXES = {'adjacent_long_runs': HEADER_LIKE}                            # every other case goes with PREFIX
GUARD = 4096


def prefix_of(name):
    return PREFIXES.get(name, PREFIX)


def run_lengths():
    """Every run length 1..600, each followed by a different label: tails 0, 1, 2, 3..258, 259, 260 and the 258 k borders for every
    voxel size; 180 300 voxels."""
    lens = np.arange(1, 601)
    return np.repeat((np.arange(600) % 5).astype(np.uint8), lens)


def blob_phantom(shape=(64, 64, 4, 5)):
    X, Y, Z, T = shape
    x, y = np.meshgrid(np.arange(X), np.arange(Y), indexing='ij')
    lab = np.zeros(shape, np.uint8)
    for t in range(T):
        for z in range(Z):
            r = np.hypot(x - X / 2 - z, y - Y / 2 + t)
            lab[:, :, z, t] = np.where(r < 8 + t, 1, np.where(r < 13 + t, 2, 0))
            lab[:, :, z, t][np.hypot(x - X / 4, y - Y / 3) < 5 + z] = 3
    return lab.reshape(-1, order='F')


def border_volume(geometry):
    """Run starts on both sides of every workgroup border of the run scan (geometry[0] voxels each) and enough runs that their
    indices cross the borders of the per-run launches (geometry[1] runs each) several times: single-voxel runs around every border,
    long runs between."""
    vox_block, run_block = int(geometry[0]), int(geometry[1])
    n = vox_block * 6 + 5
    lab = np.zeros(n, np.uint8)
    lab[vox_block * 2 + 7:vox_block * 3 - 9] = 2                        # a run wholly inside one block
    for b in range(1, 7):
        at = b * vox_block
        for k, d in enumerate((-2, -1, 0, 1)):                           # starts at border - 2, - 1, border, border + 1
            if 0 <= at + d < n:
                lab[at + d] = 1 + (k + b) % 3 if (k % 2 == 0) else 0
    # run indices across the per-run workgroup borders: alternate labels over 3 * run_block + 1 voxels in the first block
    m = min(3 * run_block + 1, vox_block - 8)
    lab[3:3 + m] = (np.arange(m) % 2 + 1).astype(np.uint8)
    return lab


def adjacent_long_runs(geometry):
    """Long runs directly next to each other, and pairs with one short run between: every run here but the short ones is filled by
    the whole workgroup, and where one fill ends the next begins a few bits later (the opening literals of a voxel that is mostly
    zero bytes under a code built from a header that is mostly zero bytes), mostly in the same 32-bit word.  Run lengths 1 + 258 m
    leave no tail for any voxel size; m is large enough that a fill spans more words than a wave has lanes, whatever the token's
    length, so the two threads that meet in the shared word are of different waves; it differs from run to run, so the shared
    words fall everywhere.  Some runs have a tail."""
    coop = int(geometry[3])
    assert coop <= 1030
    parts = []
    for i in range(8):
        m = 1030 + 37 * i
        parts.append(np.full(1 + 258 * m + (0, 0, 5, 1)[i % 4], (0, 1, 0, 2)[i % 4], np.uint8))
        if i % 3 == 2:
            parts.append(np.full(1 + i % 2, 3, np.uint8))                 # one short run between two long ones
    # the same with fills of just coop tokens at every voxel size (258 coop bytes of matches: 1 + 258 coop voxels of one byte)
    for i in range(6):
        parts.append(np.full(1 + 258 * (coop + i), (1, 0)[i % 2], np.uint8))
    return np.concatenate(parts)


def corpus(geometry):
    rng = np.random.default_rng(11)
    last_single = np.zeros(5000, np.uint8)
    last_single[-1] = 2                                                   # a last run at n - 1 with length 1
    crossing = np.zeros(int(geometry[2]) * 24, np.uint8)                  # one run whose tokens fill several emission windows,
    crossing[len(crossing) // 2:len(crossing) // 2 + 3] = (1, 1, 2)       # short runs in the middle, a second long run behind them
    return [
        ('run_lengths', run_lengths()),
        ('one_voxel', np.array([3], np.uint8)),
        ('zeros_70001', np.zeros(70001, np.uint8)),
        ('threes_70001', np.full(70001, 3, np.uint8)),
        ('noise_0_3', rng.integers(0, 4, 50000).astype(np.uint8)),
        ('noise_0_255', rng.integers(0, 256, 50000).astype(np.uint8)),
        ('blob_phantom', blob_phantom()),
        ('scan_borders', border_volume(geometry)),
        ('last_run_single', last_single),
        ('window_crossing', crossing),
        ('adjacent_long_runs', adjacent_long_runs(geometry)),
    ]


def n_runs(lab):
    return int(1 + np.count_nonzero(lab[1:] != lab[:-1]))


def raw_stream(lab, datatype, prefix=PREFIX):
    return prefix + lab.astype(DATATYPES[datatype]).tobytes()


def host_writer(lib, lab, datatype, mode, prefix=PREFIX, cap=None):
    """ukbb_fcn_gzip_labels_mode -> bytes (or its negative return value)."""
    lab = np.ascontiguousarray(lab)
    if cap is None:
        cap = int(lib.ukbb_fcn_gzip_labels_bound(lab.size, datatype, len(prefix)))
    out = np.empty(cap, np.uint8)
    got = lib.ukbb_fcn_gzip_labels_mode(lab.ctypes.data, lab.size, datatype, prefix, len(prefix), out.ctypes.data, cap, mode)
    return bytes(out[:got]) if got >= 0 else int(got)


def parallel_host(lib, lab, datatype, mode, cap, max_runs, prefix=PREFIX):
    """ukbb_fcn_gzip_labels_parallel_host into a buffer with a guard band behind out_cap -> (return value, bytes, guard untouched?)."""
    lab = np.ascontiguousarray(lab)
    buf = np.full(cap + GUARD, 0xA5, np.uint8)
    got = lib.ukbb_fcn_gzip_labels_parallel_host(lab.ctypes.data, lab.size, datatype, prefix, len(prefix), mode, buf.ctypes.data, cap, max_runs)
    return int(got), (bytes(buf[:got]) if got >= 0 else None), bool((buf[cap:] == 0xA5).all())


def check_independently(blob, lab, datatype, prefix=PREFIX):
    """The member against zlib alone: inflated content, CRC-32 and ISIZE."""
    raw = raw_stream(lab, datatype, prefix)
    assert blob[:10] == bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 4, 0xff])
    assert zlib.decompress(blob[10:-8], -15) == raw
    assert int.from_bytes(blob[-8:-4], 'little') == zlib.crc32(raw)
    assert int.from_bytes(blob[-4:], 'little') == len(raw) & 0xffffffff
