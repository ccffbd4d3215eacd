"""The device primitives of the kernel files exist once, in ukbb_cardiac_amd/csrc/device_prims.h: vector typedefs, the compile-time loop and the
bf16 MFMA wrappers.  A source scan (no GPU, no compiler) that keeps a kernel file from growing a private copy again."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'ukbb_cardiac_amd', 'csrc')
HEADER = 'device_prims.h'


def sources():
    for name in sorted(os.listdir(CSRC)):
        if name.endswith(('.hip', '.cpp', '.h')):
            with open(os.path.join(CSRC, name)) as f:
                yield name, f.read()


def test_vector_typedefs_live_in_the_header_only():
    seen = {name for name, src in sources() if 'ext_vector_type' in src}
    assert seen == {HEADER}, sorted(seen)


def test_no_kernel_file_has_a_private_unroll_or_bf16_mfma_wrapper():
    hips = [(name, src) for name, src in sources() if name.endswith('.hip')]
    assert len(hips) >= 11
    for name, src in hips:
        # the body of the compile-time loop: f(integral_constant<int, I>{}); next<N, I + 1>(f)
        assert not re.search(r'integral_constant<\s*int\s*,\s*I\s*>\s*\{\s*\}', src), '%s defines a compile-time loop of its own' % name
        assert not re.search(r'__builtin_amdgcn_mfma_f32_(32x32x16|16x16x32)_bf16', src), '%s calls the bf16 MFMA builtin directly' % name
    header = dict(sources())[HEADER]
    assert len(re.findall(r'integral_constant<int, I>\{\}', header)) == 1
    assert len(re.findall(r'__builtin_amdgcn_mfma_f32_32x32x16_bf16\(', header)) == 2      # the f32x4 and the u32x4 overload
    assert len(re.findall(r'__builtin_amdgcn_mfma_f32_16x16x32_bf16\(', header)) == 1
