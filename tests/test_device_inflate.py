"""The deflate decoder core that the GPU inflate kernel and ukbb_fcn_inflate_core_host share (csrc/inflate_core.h), on the CPU:
byte for byte against Python's zlib on a seeded corpus (every block type, strategy and flush zlib emits, plus hand-assembled
streams for what it never emits), the error class of every malformed stream of a fixed list, guard bytes around the output,
the gzip member layout and NIfTI plan of device_inflate.py, CRC-32 combination -- and the same corpus through the core under
AddressSanitizer / UBSan in a stand-alone program.  tests/test_device_inflate_gpu.py runs the same corpus on the device."""
import functools
import gzip
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INPUT, E_DATA, E_OUTPUT = -1, -2, -3


def ll_root():
    """first-level width of the literal / length table, from csrc/inflate_core.h"""
    src = open(os.path.join(ROOT, 'ukbb_cardiac_amd', 'csrc', 'inflate_core.h')).read()
    return int(re.search(r'constexpr int LL_ROOT = (\d+)', src).group(1))


# ---- a bit writer for streams zlib does not emit ---------------------------------------------------------------------------
class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, v, n):                                    # n bits of v, least significant first (header fields, extra bits)
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):                                    # a Huffman code: most significant bit first
        self.bits(int('{:0{}b}'.format(c, n)[::-1], 2), n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, b):
        assert self.n == 0
        self.out += b

    def done(self):
        self.align()
        return bytes(self.out)


def canonical(lens):
    """{symbol: (code, length)} of the canonical Huffman code with these lengths (RFC 1951 3.2.2)"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def fixed_ll():
    return canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]


def put_tokens(w, tokens, ll, dd):
    """tokens: ints (literals), ('m', length, distance), 'eob', ('sym', s) a bare literal/length symbol, ('dsym', s) a bare distance symbol"""
    for t in tokens:
        if isinstance(t, int):
            w.code(*ll[t])
        elif t == 'eob':
            w.code(*ll[256])
        elif t[0] == 'sym':
            w.code(*ll[t[1]])
        elif t[0] == 'dsym':
            w.code(*dd[t[1]])
        else:
            _, length, dist = t
            ls = max(i for i in range(29) if LEN_BASE[i] <= length and (i == 28 or length < 258))
            w.code(*ll[257 + ls])
            w.bits(length - LEN_BASE[ls], LEN_EXTRA[ls])
            ds = max(i for i in range(30) if DIST_BASE[i] <= dist)
            w.code(*dd[ds])
            w.bits(dist - DIST_BASE[ds], DIST_EXTRA[ds])


def fixed_block(w, tokens, final):
    w.bits(1 if final else 0, 1)
    w.bits(1, 2)
    put_tokens(w, tokens, fixed_ll(), {s: (s, 5) for s in range(32)})


def stored_block(w, data, final, nlen=None):
    w.bits(1 if final else 0, 1)
    w.bits(0, 2)
    w.align()
    w.raw(struct.pack('<HH', len(data), (len(data) ^ 0xffff) if nlen is None else nlen))
    w.raw(data)


CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def dynamic_header(w, final, ll_lens, d_lens, cl_lens=None, cl_syms=None, hlit=None):
    """A dynamic block's header with every code length written on its own (no repeats) unless cl_syms gives the symbol list
    [(symbol, extra value), ...] itself.  cl_lens: the 19 lengths of the code-length code (default: 4 bits for 0..15)."""
    cl_lens = cl_lens or [4] * 16 + [0, 0, 0]
    cl = canonical(cl_lens)
    w.bits(1 if final else 0, 1)
    w.bits(2, 2)
    w.bits(len(ll_lens) - 257 if hlit is None else hlit, 5)
    w.bits(len(d_lens) - 1, 5)
    w.bits(19 - 4, 4)
    for s in CL_ORDER:
        w.bits(cl_lens[s], 3)
    syms = cl_syms if cl_syms is not None else [(l, 0) for l in list(ll_lens) + list(d_lens)]
    for s, extra in syms:
        w.code(*cl[s])
        if s >= 16:
            w.bits(extra, {16: 2, 17: 3, 18: 7}[s])


def dynamic_block(w, tokens, final, ll_lens, d_lens):
    dynamic_header(w, final, ll_lens, d_lens)
    put_tokens(w, tokens, canonical(ll_lens), canonical(d_lens))


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=()):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out, last = b'', 0
    for at in flush_at:
        out += c.compress(data[last:at]) + c.flush(zlib.Z_FULL_FLUSH)
        last = at
    return out + c.compress(data[last:]) + c.flush()


def long_code_lens():
    """literal / length code with lengths 1..14 and two of 15 (complete): 'A'..'M' 1..13, end-of-block 14, 'N' and length symbol 257 at 15"""
    ll = [0] * 258
    for i in range(13):
        ll[ord('A') + i] = i + 1
    ll[256] = 14
    ll[ord('N')], ll[257] = 15, 15
    return ll


@functools.lru_cache(maxsize=None)
def corpus():
    """[(name, raw deflate stream, content)] -- seeded, about 4 MB of content in all; content is what zlib inflates the stream to"""
    from ukbb_cardiac_amd.phantom import cine_phantom
    rng = np.random.default_rng(20240607)
    text = bytes(rng.integers(97, 105, 60000, dtype=np.uint8))
    mixed = text[:20000] + bytes(rng.integers(0, 256, 20000, dtype=np.uint8)) + text[:30000]
    cine = cine_phantom(2 * 3, 162, 204, seed=11)[..., 0].reshape(3, 2, 162, 204).transpose(2, 3, 1, 0)      # (X,Y,Z,T), values 0..1
    cine16 = np.asfortranarray((cine * 1800).astype(np.int16))
    cine32 = np.asfortranarray(cine16.astype(np.float32))
    items = []
    for lv in (1, 6, 9):
        items.append(('level%d' % lv, deflate(mixed, lv)))
    items.append(('stored', deflate(text[:1000], 0)))
    items.append(('stored_multi', deflate(mixed + mixed, 0)))                   # > 65 535 bytes: several stored blocks
    for name, st in (('fixed', zlib.Z_FIXED), ('huffman_only', zlib.Z_HUFFMAN_ONLY), ('rle', zlib.Z_RLE)):
        items.append((name, deflate(mixed, 6, st)))
    items.append(('full_flush', deflate(mixed, 6, flush_at=(100, 100, 30000))))  # several blocks, empty stored blocks in between
    items.append(('empty', deflate(b'')))
    items.append(('one_byte', deflate(b'x')))
    items.append(('cine_int16', deflate(cine16.tobytes(order='F'), 6)))
    items.append(('cine_float32', deflate(cine32.tobytes(order='F'), 1)))
    items.append(('zeros', deflate(bytes(300 * 1024), 6)))                       # distance 1
    items.append(('period3', deflate(b'xyz' * 30000, 9)))                        # distance < length
    w = BitWriter()                                                               # a distance zlib never emits
    stored_block(w, bytes(rng.integers(0, 256, 32768, dtype=np.uint8)), False)
    fixed_block(w, [('m', 258, 32768), 'eob'], True)
    items.append(('distance_32768', w.done()))
    w = BitWriter()                                                               # codes longer than the first-level table is wide
    ll = long_code_lens()
    dynamic_block(w, list(b'ABCDEFGHIJKLMNNMLKJIHGFEDCBA') + [('m', 3, 2), ord('N'), ('m', 3, 1), 'eob'], True, ll, [1, 1])
    items.append(('long_codes', w.done()))
    w = BitWriter()                                                               # the one incomplete code RFC 1951 allows
    dynamic_block(w, list(b'ABCABC') + [('m', 3, 1), 'eob'], True, ll, [1])
    items.append(('single_distance_code', w.done()))
    w = BitWriter()                                                               # a match that reaches back across a block boundary
    fixed_block(w, list(b'abcdefgh') + ['eob'], False)
    fixed_block(w, [('m', 8, 8), ('m', 20, 3), 'eob'], True)
    items.append(('across_blocks', w.done()))
    return [(name, raw, zlib.decompress(raw, -15)) for name, raw in items]


@functools.lru_cache(maxsize=None)
def malformed():
    """[(name, stream, output capacity, expected class)] -- a fixed list"""
    good = corpus()[1]
    out = [('cut_in_half', good[1][:len(good[1]) // 2], len(good[2]), E_INPUT)]
    w = BitWriter(); w.bits(1, 1); w.bits(3, 2); w.bits(0, 29)
    out.append(('block_type_3', w.done(), 64, E_DATA))
    w = BitWriter(); stored_block(w, b'hello', True, nlen=5)
    out.append(('stored_len_nlen', w.done(), 64, E_DATA))
    w = BitWriter(); fixed_block(w, [('m', 3, 1), 'eob'], True)
    out.append(('match_first', w.done() + bytes(4), 64, E_DATA))
    ll = [0] * 257
    ll[0] = ll[1] = ll[2] = ll[256] = 1
    w = BitWriter(); dynamic_block(w, [0, 'eob'], True, ll, [1, 1])
    out.append(('oversubscribed', w.done() + bytes(4), 64, E_DATA))
    ll = [0] * 257
    ll[0], ll[256] = 1, 2
    w = BitWriter(); dynamic_block(w, [0, 'eob'], True, ll, [1, 1])
    out.append(('incomplete_literal_code', w.done() + bytes(4), 64, E_DATA))
    w = BitWriter()
    dynamic_header(w, True, [0] * 257, [1, 1], cl_lens=[4] * 15 + [5, 5, 0, 0], cl_syms=[(16, 0)] + [(1, 0)] * 8)
    out.append(('repeat_first', w.done() + bytes(8), 64, E_DATA))
    w = BitWriter(); dynamic_header(w, True, [8] * 257, [1, 1], hlit=30)
    out.append(('hlit_287', w.done() + bytes(8), 64, E_DATA))
    w = BitWriter(); fixed_block(w, [ord('a'), ('sym', 286), 'eob'], True)
    out.append(('symbol_286', w.done() + bytes(4), 64, E_DATA))
    w = BitWriter(); fixed_block(w, [ord('a'), ('sym', 257), ('dsym', 30), 'eob'], True)
    out.append(('distance_symbol_30', w.done() + bytes(4), 64, E_DATA))
    out.append(('one_byte_short', good[1], len(good[2]) - 1, E_OUTPUT))
    out.append(('byte_behind_the_last_block', good[1] + b'\x00', len(good[2]), E_DATA))    # src_len is the stream, no more
    return out


GUARD = 256


def core_host(raw, cap, align=0):
    """ukbb_fcn_inflate_core_host with 256 guard bytes of 0xA5 on both sides of the output: (result, output bytes)"""
    from ukbb_cardiac_amd import _lib
    src = np.zeros(len(raw) + 8, np.uint8)
    off = (-src.ctypes.data) % 4 + align
    src[off:off + len(raw)] = np.frombuffer(raw, np.uint8)
    dst = np.full(cap + 2 * GUARD, 0xA5, np.uint8)
    r = _lib.lib.ukbb_fcn_inflate_core_host(src.ctypes.data + off, len(raw), dst.ctypes.data + GUARD, cap)
    assert (dst[:GUARD] == 0xA5).all() and (dst[GUARD + cap:] == 0xA5).all(), 'guard bytes changed'
    return r, dst[GUARD:GUARD + max(r, 0)].tobytes()


def test_corpus_covers_what_it_claims():
    names = [n for n, _, _ in corpus()]
    assert len(set(names)) == len(names) == 19
    by = {n: (raw, content) for n, raw, content in corpus()}
    assert max(long_code_lens()) > ll_root()                     # second-level tables are reached
    assert by['long_codes'][1] == b'ABCDEFGHIJKLMNNMLKJIHGFEDCBA' + b'BABNNNN'
    assert len(by['stored_multi'][1]) > 65535 and len(by['empty'][1]) == 0 and len(by['one_byte'][1]) == 1
    assert by['distance_32768'][1][-258:] == by['distance_32768'][1][:258]
    assert by['across_blocks'][1] == b'abcdefgh' * 2 + b'fghfghfghfghfghfghfg'
    assert by['single_distance_code'][1] == b'ABCABCCCC'
    assert 390000 < len(by['cine_int16'][1]) < 410000 and len(by['cine_float32'][1]) == 2 * len(by['cine_int16'][1])


@pytest.mark.parametrize('align', [0, 1, 2, 3])
def test_core_host_equals_zlib(align):
    for name, raw, content in corpus():
        r, out = core_host(raw, len(content) + 100, align)
        assert r == len(content) and out == content, name
        r, out = core_host(raw, len(content), align)            # dst_cap exactly the content length
        assert r == len(content) and out == content, name


def test_core_host_error_classes():
    for name, raw, cap, want in malformed():
        r, _ = core_host(raw, cap)
        assert r == want, (name, r, want)
    for name, raw, content in corpus():                          # zlib agrees that the valid ones are valid, and that cutting any of them is not
        if len(raw) > 8:
            r, _ = core_host(raw[:len(raw) // 2], len(content))
            assert r in (E_INPUT, E_DATA), name


def _nifti_bytes(tmp_path, vol):
    from ukbb_cardiac_amd import nifti
    p = str(tmp_path / 'plain.nii')
    nifti.save(vol, p, np.eye(4))
    with open(p, 'rb') as f:
        return f.read()


def test_gzip_member_layout(tmp_path):
    from ukbb_cardiac_amd import _lib, nifti
    from ukbb_cardiac_amd.device_inflate import gzip_member_layout, plan_subject
    rng = np.random.default_rng(3)
    vol = np.asfortranarray(rng.integers(0, 900, (20, 18, 2, 3)).astype(np.int16))
    content = _nifti_bytes(tmp_path, vol)
    blobs = {'gzip': gzip.compress(content, 6, mtime=0)}
    p = str(tmp_path / 'named.nii.gz')
    with gzip.GzipFile(p, 'wb', 6) as g:                         # FNAME
        g.write(content)
    blobs['gzip_fname'] = open(p, 'rb').read()
    assert blobs['gzip_fname'][3] & 8 and not blobs['gzip'][3] & 8
    p = str(tmp_path / 'saved.nii.gz')
    nifti.save(vol, p, np.eye(4))
    blobs['nifti_save'] = open(p, 'rb').read()
    labels = np.ascontiguousarray(rng.integers(0, 4, vol.size).astype(np.uint8))
    lab_content = content[:70] + struct.pack('<hh', 64, 64) + content[74:352] + labels.astype(np.float64).tobytes()
    cap = _lib.lib.ukbb_fcn_gzip_labels_bound(labels.size, 64, 352)
    out = np.empty(cap, np.uint8)
    head = np.frombuffer(lab_content[:352], np.uint8).copy()
    n = _lib.lib.ukbb_fcn_gzip_labels(labels.ctypes.data, labels.size, 64, head.ctypes.data, 352, out.ctypes.data, cap)
    assert n > 0
    for name, blob, want in [(k, v, content) for k, v in blobs.items()] + [('gzip_labels', out[:n].tobytes(), lab_content)]:
        lay = gzip_member_layout(blob, len(want))
        assert lay is not None, name
        off, ln, crc, isize = lay
        assert zlib.decompress(blob[off:off + ln], -15) == want and crc == zlib.crc32(want) and isize == len(want), name
        r, got = core_host(blob[off:off + ln], len(want))
        assert r == len(want) and got == want, name
    blob = blobs['gzip']
    assert gzip_member_layout(blob) == gzip_member_layout(blob, len(content))        # size from the NIfTI header inside
    assert gzip_member_layout(blob + bytes(5)) == gzip_member_layout(blob)           # zero padding
    fhcrc = bytes([0x1f, 0x8b, 8, 2]) + blob[4:10] + struct.pack('<H', zlib.crc32(bytes([0x1f, 0x8b, 8, 2]) + blob[4:10]) & 0xffff) + blob[10:]
    assert zlib.decompress(fhcrc, 31) == content                  # a valid file, left to the host reader
    assert gzip_member_layout(fhcrc) is None
    two = gzip.compress(content[:3000], 6, mtime=0) + gzip.compress(content[3000:], 6, mtime=0)
    assert zlib.decompressobj(31).decompress(two) == content[:3000] and gzip.decompress(two) == content
    assert gzip_member_layout(two) is None                       # two members
    assert gzip_member_layout(blob + b'abc') is None             # trailing garbage
    # bytes between the end of the stream and a plausible trailer: the layout cannot see them, the decoder refuses the stream
    off, ln, _, _ = gzip_member_layout(blob)
    junk = blob[:off + ln] + b'junk' + blob[off + ln:]
    assert gzip_member_layout(junk, len(content)) == (off, ln + 4, zlib.crc32(content), len(content))
    assert core_host(junk[off:off + ln + 4], len(content))[0] == E_DATA
    assert gzip_member_layout(blob[:3] + b'\x40' + blob[4:]) is None and gzip_member_layout(blob[:2] + b'\x07' + blob[3:]) is None
    assert gzip_member_layout(blob[:12]) is None
    plan = plan_subject(blob)
    assert plan.shape == vol.shape and plan.dtype == np.int16 and plan.vox_offset == 352 and plan.total == len(content)
    for bad in (vol.astype(np.float64), vol.astype(np.int32), vol[:, :, :, 0], vol.astype('>i2')):
        p = str(tmp_path / 'bad.nii.gz')
        nifti.save(bad, p, np.eye(4))
        if bad.dtype.byteorder == '>':                           # nifti.save writes little-endian: swap the header and the voxels by hand
            raw = bytearray(_nifti_bytes(tmp_path, vol))
            raw[0:4] = struct.pack('>i', 348)
            raw[40:56] = struct.pack('>8h', *struct.unpack('<8h', raw[40:56]))
            raw[70:74] = struct.pack('>2h', *struct.unpack('<2h', raw[70:74]))
            raw[252:256] = struct.pack('>2h', *struct.unpack('<2h', raw[252:256]))
            assert plan_subject(gzip.compress(bytes(raw))) is None
            continue
        assert plan_subject(open(p, 'rb').read()) is None
    scaled = bytearray(content)
    scaled[112:116] = struct.pack('<f', 2.0)                     # scl_slope
    assert plan_subject(gzip.compress(bytes(scaled))) is None
    assert plan_subject(b'not gzip at all') is None and plan_subject(gzip.compress(b'short')) is None


def test_crc_combine():
    from ukbb_cardiac_amd import _lib
    rng = np.random.default_rng(5)
    data = bytes(rng.integers(0, 256, 1 << 20, dtype=np.uint8))
    for split in (0, 1, 4095, 4096, 4097, 1 << 19, (1 << 20) - 1, 1 << 20):
        a, b = data[:split], data[split:]
        assert _lib.lib.ukbb_fcn_gzip_crc_combine(zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(data), split
    assert _lib.lib.ukbb_fcn_gzip_crc(0, np.frombuffer(data, np.uint8).ctypes.data, len(data)) == zlib.crc32(data)


def write_corpus_file(path):
    """The corpus and the malformed list for tests/cpp/inflate_core_asan.cpp: count, then per case src_len, dst_cap, expected result
    (int64, little-endian), the stream and -- when the result is not negative -- the expected output."""
    cases = [(raw, len(c), len(c), c) for _, raw, c in corpus()] + [(raw, len(c) + 7, len(c), c) for _, raw, c in corpus()]
    cases += [(raw, cap, want, b'') for _, raw, cap, want in malformed()]
    with open(path, 'wb') as f:
        f.write(struct.pack('<I', len(cases)))
        for raw, cap, want, content in cases:
            f.write(struct.pack('<QQq', len(raw), cap, want) + raw + content)
    return len(cases)


def test_core_under_sanitizers(tmp_path):
    """The host-compiled core in a stand-alone program built with -fsanitize=address,undefined: input and output live in heap blocks
    of exactly src_len and dst_cap bytes, so one byte read or written outside either ends the program."""
    exe, data = str(tmp_path / 'inflate_core_asan'), str(tmp_path / 'corpus.bin')
    n = write_corpus_file(data)
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-I', os.path.join(ROOT, 'ukbb_cardiac_amd', 'csrc'), '-o', exe,
                           os.path.join(ROOT, 'tests', 'cpp', 'inflate_core_asan.cpp')])
    out = subprocess.run([exe, data], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert 'inflate_core ok: %d cases' % n in out
