"""Every convolution launch the default fp32 plans of FCN_sa and UNet_ao can make, one launch at a time, against float64 on the engine's OWN stored input.

tests/test_fp32_layers_gpu.py grades the encoder of three small-batch cases this way (tilings 134, 120, 123, 29, 141, 142, 301, 303, 305).  This file
does it for every (model, layer, tiling) combination the recorded default plans hold (tests/golden/plan_layouts.json: 121 of them over 7 x 8 x 6
records): the large-batch kernels the benchmark runs on (stride-2 producer/consumer 124 and 145, Winograd F(2x4) 304 and 307, F(2x2) 300 and 302), and
the whole aortic U-Net plan -- fused first layer 130, transposed convs 60 / 62, the two-source skip-concat convs, up0_* on 11 and the logits launch.
tests/test_fp32_launch_coverage.py shows on the CPU that CASES reaches all of them, and which maps they are reached on.

The method is the graders' common one (tests/launch_grading.py: one forward per case, every stored map recomputed in float64 from the map or maps
the engine stored in front of it, a batch of copies of three rough images with slices 0-2 graded and every other slice bit-identical to its copy,
the plan that ran being the plan counted).  Here the fused first layer (conv0_0 + conv0_1) is graded as a unit from the image, the skip-concat convs
from concatenate([skip, upL_t]), the logits from the stored up0 with bias and no ReLU; the copy identity also holds across the U-Net's half-batch
split (levels >= 1 run as two chains on two streams), which falls between copies.  The FCN squeeze and head launches are graded in
tests/test_head_launches_gpu.py.
Bound, as in tests/test_fp32_layers_gpu.py: max |engine - float64| <= 1e-5 x the layer's largest activation, for every launch.

CASES: the smallest maps (H and W multiples of 16, N = 1 or 17 = the first recorded batch above plan.h SMALL_BATCH = 16) found by searching
plan_layout for each combination, reduced to a cover in which every case is needed.  A stride-2 or Winograd combination counts as reached only with
its tiles dividing the map, or not, as some recorded plan has it; so the straight-line producers of 124 / 141 / 142 / 145 are graded on maps they
divide, which for conv4_0 means 192 x 208, 176 x 208 and 208 x 256 themselves.  Pixels = N x H x W of the launch; float64 pixels = min(N, 3) x H x W.

    case  model     N    H    W    pixels  float64 pixels  weights  batch-1 image
       0  FCN_sa    1   64   16      1024            1024     1234  phantom
       1  FCN_sa    1   16  144      2304            2304        7  uniform
       2  FCN_sa    1  208   64     13312           13312     1234  normal
       3  FCN_sa    1   96  208     19968           19968        7  phantom
       4  FCN_sa    1  176  208     36608           36608     1234  uniform
       5  FCN_sa    1  192  208     39936           39936        7  normal
       6  FCN_sa    1  208  256     53248           53248     1234  phantom
       7  FCN_sa   17   16   64     17408            3072        7  -
       8  FCN_sa   17   48  208    169728           29952     1234  -
       9  FCN_sa   17  128  256    557056           98304        7  -
      10  FCN_sa   17  192  208    678912          119808     1234  -
      11  UNet_ao   1   32   32      1024            1024        7  normal
      12  UNet_ao   1  144   16      2304            2304     1234  phantom
      13  UNet_ao   1   16  208      3328            3328        7  uniform
      14  UNet_ao   1   32  256      8192            8192     1234  normal
      15  UNet_ao   1  128  256     32768           32768        7  phantom
      16  UNet_ao   1  176  208     36608           36608     1234  uniform
      17  UNet_ao   1  192  208     39936           39936        7  normal
      18  UNet_ao   1  208  256     53248           53248     1234  phantom
      19  UNet_ao  17   48   16     13056            2304        7  -
      20  UNet_ao  17   16   64     17408            3072     1234  -
      21  UNet_ao  17   64   96    104448           18432        7  -
      22  UNet_ao  17  192  208    678912          119808     1234  -
    all                           2580736          738560

Measured on an MI355X (profiles/fp32_launches.txt, one row per launch, worst launch per tiling in its last block): 8e-8 .. 1.5e-6 of the layer's
scale, no copy differing; the 23 cases take 5 s together, the largest 0.1 s of forward and read-back and 0.3 s of float64."""
import time

import numpy as np
import pytest

from launch_grading import SEEDS, assert_plan_ran, batch_of_copies, check_copies, launches, layer, plan_cfgs, rel_err

pytestmark = pytest.mark.gpu
BOUND = 1e-5

CASES = [
    ('FCN_sa', 1, 64, 16), ('FCN_sa', 1, 16, 144), ('FCN_sa', 1, 208, 64), ('FCN_sa', 1, 96, 208), ('FCN_sa', 1, 176, 208), ('FCN_sa', 1, 192, 208),
    ('FCN_sa', 1, 208, 256), ('FCN_sa', 17, 16, 64), ('FCN_sa', 17, 48, 208), ('FCN_sa', 17, 128, 256), ('FCN_sa', 17, 192, 208),
    ('UNet_ao', 1, 32, 32), ('UNet_ao', 1, 144, 16), ('UNet_ao', 1, 16, 208), ('UNet_ao', 1, 32, 256), ('UNet_ao', 1, 128, 256), ('UNet_ao', 1, 176, 208),
    ('UNet_ao', 1, 192, 208), ('UNet_ao', 1, 208, 256), ('UNet_ao', 17, 48, 16), ('UNet_ao', 17, 16, 64), ('UNet_ao', 17, 64, 96), ('UNet_ao', 17, 192, 208),
]


@pytest.mark.parametrize('index', range(len(CASES)), ids=['%s-%dx%dx%d' % c for c in CASES])
def test_each_fp32_launch_against_float64_on_its_own_input(index):
    from ukbb_cardiac_amd import engine
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.weights import synthetic_params
    model, n, H, W = CASES[index]
    seed = SEEDS[index % 2]
    arch = MODELS[model]
    params = synthetic_params(arch, seed)
    img, nd = batch_of_copies(index, n, H, W)
    plan = engine.plan_layout(arch, 'fp32', n, H, W)
    graph = launches(arch)
    t0 = time.perf_counter()
    with engine.Engine(arch, params) as eng:
        out = eng.run(img, want_logits=True)
        assert_plan_ran(eng, plan)                                       # the plan tests/test_fp32_launch_coverage.py counted for this case
        stored = {'logits': out['logits']}
        for lname, sname, l, _, _, _, _ in graph:
            if lname not in ('conv0_0', 'logits'):                       # conv0_0 lives inside conv0_1's launch
                stored[sname] = eng.activation(sname).reshape(n, H >> l, W >> l, -1)
    t_gpu = time.perf_counter() - t0
    cfg_of = {part: cfg for o, cfg in zip(plan['ops'], plan_cfgs(plan['ops'])) for part in o['name'].split('+')}
    assert stored['logits'].shape[:3] == (n, H, W)
    # every slice is a bit-identical copy of the graded slice of its image, in every stored map and in the logits
    for sname, a in stored.items():
        check_copies(sname, a, nd, '(tiling %s)' % cfg_of.get(sname))
    t0 = time.perf_counter()
    rows = []
    fused_first = None
    for lname, sname, l, srcs, stride, transposed, relu in graph:
        if lname == 'logits' and model.startswith('FCN'):
            continue
        if lname == 'conv0_0':                                           # fused first layer: conv0_0 in float64 from the image, then conv0_1, as a unit
            fused_first = layer(img[:nd], params[lname])
            continue
        x = fused_first if lname == 'conv0_1' else np.concatenate([stored[s][:nd] for s in srcs], axis=-1)
        ex = layer(x, params[lname], stride, transposed, relu)
        err, where = rel_err(stored[sname][:nd], ex)
        rows.append((lname, cfg_of[lname], err, where))
    t_ref = time.perf_counter() - t0
    for lname, cfg, err, where in rows:
        print('fp32-launch %-8s %2dx%3dx%3d seed %4d  %-8s tiling %3d  err/scale %.2e  worst at %s' % (model, n, H, W, seed, lname, cfg, err, where))
    print('fp32-launch %-8s %2dx%3dx%3d forward + read-back %.2f s, float64 reference %.2f s' % (model, n, H, W, t_gpu, t_ref))
    bad = [r for r in rows if not r[2] <= BOUND]
    assert not bad, 'launches over %g of their layer\'s scale (layer, tiling, error, worst element [slice, y, x, channel]): %s' % (BOUND, bad)
