"""The host-side weight packers live once, in ukbb_cardiac_amd/csrc/pack.{h,cpp}: host arithmetic on the standard library alone.  No GPU.

Bytes: tools/pack_digest.cpp (built through `make pack_digest`, linking pack.cpp and nothing else) runs every packer on fixed inputs and prints a
digest per case; tests/golden/pack_digests.txt holds the same program's output linked against the packers as they stood in the kernel files, so a
packed layout cannot move by a byte.  Rounding: the one host bf16 rounding, bf16_rne, on finite values, ties, infinities and NaNs.  Source scan
(in the manner of tests/test_device_prims.py): no packer and no private rounding comes back into a kernel file, and the unit stays free of HIP."""
import os
import re
import subprocess

import numpy as np
import pytest

from launch_grading import bf16_round

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'ukbb_cardiac_amd', 'csrc')
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'pack_digests.txt')
ROUNDING_LIST = ('3f808000 3f818000 3f808001 7f7fffff 7f800000 ff800000 7fc00000 7f800001 7fffffff 00000001 00008000 80000000').split()


@pytest.fixture(scope='module')
def digest_lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('pack') / 'pack_digest')
    subprocess.check_call(['make', '-C', CSRC, '-s', 'pack_digest', 'PACK_DIGEST=' + exe])
    return subprocess.run([exe], check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout.splitlines()


def test_every_packed_layout_keeps_its_bytes(digest_lines):
    with open(GOLDEN) as f:
        golden = f.read().splitlines()
    assert len(golden) == 43 and len({line.split()[0] for line in golden}) == 20        # 20 functions, every case of each
    assert digest_lines[:-1] == golden


def test_the_host_bf16_rounding(digest_lines):
    words = digest_lines[-1].split()
    assert words[0] == 'bf16_rne'
    got = dict(w.split(':') for w in words[1:])
    assert list(got) == ROUNDING_LIST
    got = {int(k, 16): int(v, 16) for k, v in got.items()}
    for u in (0x3f808000, 0x3f818000, 0x3f808001, 0x7f7fffff, 0x00000001, 0x00008000, 0x80000000):     # the finite ones: the graders' rounding model
        want = int(bf16_round(np.array([u], np.uint32).view(np.float32)).view(np.uint32)[0]) >> 16
        assert got[u] == want, '%08x' % u
    assert got[0x3f808000] == 0x3f80 and got[0x3f818000] == 0x3f82                          # ties go to the even neighbour: down, up
    assert got[0x7f7fffff] == 0x7f80                                                        # the largest finite value rounds to infinity
    assert got[0x7f800000] == 0x7f80 and got[0xff800000] == 0xff80                          # the infinities keep their pattern
    for u in (0x7fc00000, 0x7f800001, 0x7fffffff):                                          # a NaN stays a NaN, a full mantissa included
        assert got[u] & 0x7f80 == 0x7f80 and got[u] & 0x007f, '%08x -> %04x' % (u, got[u])


def sources():
    for name in sorted(os.listdir(CSRC)):
        if name.endswith(('.hip', '.cpp', '.h')):
            with open(os.path.join(CSRC, name)) as f:
                yield name, f.read()


def test_no_kernel_file_packs_or_rounds_on_the_host():
    hips = [(name, src) for name, src in sources() if name.endswith('.hip')]
    assert len(hips) >= 11
    for name, src in hips:
        # a definition: the name at the start of a declarator, its parameter list, then a body (calls and comments do not match)
        assert not re.search(r'^[\w:\s\*&]*\b(pack_\w+|tconv_as_conv2x2|wst_pack_order)\s*\([^;{}]*\)\s*\{', src, re.M), '%s defines a packer' % name
        assert '0x7fffu +' not in src, '%s holds a host bf16 rounding of its own' % name
    assert sum(src.count('0x7fffu +') for name, src in sources()) == 1                      # the one in pack.cpp


def test_the_packers_need_no_hip():
    src = dict(sources())
    for name in ('pack.h', 'pack.cpp'):
        assert not re.search(r'#\s*include\s*[<"]hip/', src[name]), name
        for inc in re.findall(r'#\s*include\s*"([^"]+)"', src[name]):
            assert inc == 'pack.h', '%s includes %s' % (name, inc)
