"""What the graders of the Temporal-UNet's bf16 mode share (precision 'bf16_3d', UKBB_PREC_BF16_3D, kernels_conv3d_bf16.hip): the cases, the
rounding model of one launch in float64 and the mirror of the new launchers' grid arithmetic.  A helper module like tests/launch_grading.py (which
stays as it is): no tests of its own, ukbb_cardiac_amd imported inside the functions that need it.

THE ROUNDING MODEL of one launch (layer3d_bf16): the engine's float32 BN fold (launch_grading.fold), the folded kernel rounded ONCE to bf16, ties to
even (launch_grading.bf16_round), the stored bf16-valued input taken as it is, the sum exact (float64), + the float32 bias, ReLU; the engine rounds
that once to bf16 as it stores it.  conv0_0 (C_in = 1) is launch_grading.layer3d on the float32 image with the UNROUNDED fold; conv_out is
launch_grading.layer3d on the stored up0_1 (no rounding of its kernel, bias, no ReLU) and stays float32.

A launch is graded by launch_grading.grade(..., ulps=0.5, fraction=1.0): every element within half a bf16 ulp of the exact value of that model (+ the
2^-18 relative and 2^-20-of-scale slack for fp32 accumulation that the bf16 U-Net graders allow), scale = the layer's largest exact activation.

THE LAUNCHERS.  launch_conv3d_bf16 keeps launch_conv3d's item decomposition (one wave = 32 pixels of one frame x 32 CB output channels, CB = 2 where
the padded channel count is a multiple of 64, four items per workgroup, blockIdx.y = sub-pixel phase), so launch_grading.conv3d_launch is its mirror
too; launcher_lines() reads the lines from the new source.  launch_conv3d_first_bf16 starts one thread per pixel with no cap (no loop to wrap)."""
import dataclasses
import os
import re

import numpy as np

import launch_grading as G

PRECISION = 'bf16_3d'
SOURCE = os.path.join(G.ROOT, 'ukbb_cardiac_amd', 'csrc', 'kernels_conv3d_bf16.hip')

WIDE = dict(n_filter=(16, 32, 96, 160, 96), n_block=(2, 2, 3, 2, 2))
ARCH_CHANGES = {'default': {}, 'fc3c2': dict(fc=3, n_class=2), 'fc1c4': dict(fc=1, n_class=4), 'wide': WIDE}

# architecture, windows, H, W: the twelve of tests/test_temporal_launches_gpu.py -- the new launcher has that launcher's decomposition, and
# tests/test_temporal_bf16_launch_coverage.py shows that they reach every situation of it, none idle
CASES = [
    ('fc1c4', 1, 16, 16), ('fc3c2', 5, 16, 16), ('wide', 1, 16, 16), ('default', 2, 16, 16), ('fc3c2', 1, 48, 48), ('fc1c4', 5, 48, 48),
    ('fc3c2', 1, 32, 48), ('fc1c4', 5, 32, 48), ('wide', 5, 16, 16), ('default', 1, 32, 48), ('wide', 1, 16, 48), ('default', 1, 48, 48),
]


def arch_of(key):
    from ukbb_cardiac_amd.arch import MODELS
    return dataclasses.replace(MODELS['Temporal-UNet_ao'], **ARCH_CHANGES[key])


def layer3d_bf16(x, p, stride=1, transposed=False, relu=True):
    """One 3x3x3 unit of the bf16 mode in float64 on its stored (bf16-valued) input x [N,T,H,W,C]: the float32 fold, the kernel rounded to bf16."""
    import temporal_unet_ref as R3
    w, b = G.fold(p, transposed)
    w = G.bf16_round(w)
    x, w = np.asarray(x, np.float64), w.astype(np.float64)
    y = (R3.conv3d_transpose_same(x, w, stride) if transposed else R3.conv3d_same(x, w, stride)) + b.astype(np.float64)
    return np.maximum(y, 0.0) if relu else y


def exact_of(lname, xin, p, stride, transposed, relu):
    """The exact value of the specified arithmetic of launch `lname` on the input the engine stored in front of it."""
    if lname in ('conv0_0', 'logits'):
        return G.layer3d(xin, p, stride, transposed, relu)
    return layer3d_bf16(xin, p, stride, transposed, relu)


def launcher_lines():
    """(body of launch_conv3d_bf16, body of conv3d_bf16_kernel, body of launch_conv3d_first_bf16, body of conv3d_first_bf16_kernel)."""
    with open(SOURCE) as f:
        src = f.read()
    return (re.search(r'hipError_t launch_conv3d_bf16\(.*?\n}\n', src, re.S).group(0), re.search(r'void conv3d_bf16_kernel\(.*?\n}\n', src, re.S).group(0),
            re.search(r'hipError_t launch_conv3d_first_bf16\(.*?\n}\n', src, re.S).group(0), re.search(r'void conv3d_first_bf16_kernel\(.*?\n}\n', src, re.S).group(0))
