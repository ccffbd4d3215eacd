"""Every convolution launch the default fp32 plans of FCN_sa and UNet_ao can make, one launch at a time, against float64 on the engine's OWN stored input.

tests/test_fp32_layers_gpu.py grades the encoder of three small-batch cases this way (tilings 134, 120, 123, 29, 141, 142, 301, 303, 305).  This file
does it for every (model, layer, tiling) combination the recorded default plans hold (tests/golden/plan_layouts.json: 121 of them over 7 x 8 x 6
records): the large-batch kernels the benchmark runs on (stride-2 producer/consumer 124 and 145, Winograd F(2x4) 304 and 307, F(2x2) 300 and 302), and
the whole aortic U-Net plan -- fused first layer 130, transposed convs 60 / 62, the two-source skip-concat convs, up0_* on 11 and the logits launch.
tests/test_fp32_launch_coverage.py shows on the CPU that CASES reaches all of them, and which maps they are reached on.

One forward per case.  Each stored map is recomputed in numpy float64 (oracle/fcn_oracle.py conv2d_same / conv2d_transpose_same, the float32 BN fold of
engine.cpp create()) from the map or maps the engine stored in front of it, so a launch's deviation is its kernel's own; the fused first layer
(conv0_0 + conv0_1) is graded as a unit from the image, the skip-concat convs from concatenate([skip, upL_t]), the logits from the stored up0 with bias
and no ReLU.  The FCN squeeze and head launches are graded in tests/test_head_launches_gpu.py.
Bound, as in tests/test_fp32_layers_gpu.py: max |engine - float64| <= 1e-5 x the layer's largest activation, for every launch.

A batch is made of copies of at most three distinct images, img[i] = distinct[i % 3]: a phantom slice, a uniform-noise slice and a standard-normal
noise image scaled to the phantom's range (rough inputs, so that a wrong tap is not hidden by a smooth image).  Slices 0, 1, 2 are graded in float64
-- the float64 cost does not grow with the batch -- and every other slice of every stored map and of the logits must be BIT-IDENTICAL to the graded
copy of its image.  That grades all N slices, asserts batch independence inside every large-batch tiling, and across the U-Net's half-batch split
(levels >= 1 run as two chains on two streams), which falls between copies.  Batch-1 cases take one of the three images in turn.

Each case also asserts that the plan it ran is the one the CPU test computed for it: kernel_names() / kernel_configs() equal plan_layout's.

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
import numpy as np
import pytest

from oracle import fcn_oracle as O

pytestmark = pytest.mark.gpu
BOUND = 1e-5
SEEDS = (1234, 7)

CASES = [
    ('FCN_sa', 1, 64, 16), ('FCN_sa', 1, 16, 144), ('FCN_sa', 1, 208, 64), ('FCN_sa', 1, 96, 208), ('FCN_sa', 1, 176, 208), ('FCN_sa', 1, 192, 208),
    ('FCN_sa', 1, 208, 256), ('FCN_sa', 17, 16, 64), ('FCN_sa', 17, 48, 208), ('FCN_sa', 17, 128, 256), ('FCN_sa', 17, 192, 208),
    ('UNet_ao', 1, 32, 32), ('UNet_ao', 1, 144, 16), ('UNet_ao', 1, 16, 208), ('UNet_ao', 1, 32, 256), ('UNet_ao', 1, 128, 256), ('UNet_ao', 1, 176, 208),
    ('UNet_ao', 1, 192, 208), ('UNet_ao', 1, 208, 256), ('UNet_ao', 17, 48, 16), ('UNet_ao', 17, 16, 64), ('UNet_ao', 17, 64, 96), ('UNet_ao', 17, 192, 208),
]

BN_EPS = np.float32(1e-3)


def fold(p, transposed=False):
    """engine.cpp create(): sc = gamma / sqrtf(var + eps); W' = W * sc; b' = beta - mean * sc, all float32 (as tests/test_bf16_layers_gpu.py fold;
    for a conv identical to tests/test_fp32_layers_gpu.py fold).  A layer without BN keeps its kernel and bias."""
    k = p['kernel'].astype(np.float32)
    if 'gamma' not in p:
        return k, p['bias'].astype(np.float32)
    sc = (p['gamma'].astype(np.float32) / np.sqrt(p['var'].astype(np.float32) + BN_EPS)).astype(np.float32)
    ms = (p['mean'].astype(np.float32) * sc).astype(np.float32)
    b = (p['beta'].astype(np.float32) - ms).astype(np.float32)
    return (k * (sc[None, None, :, None] if transposed else sc[None, None, None, :])).astype(np.float32), b


def layer(x, p, stride=1, transposed=False, relu=True):
    """One conv2d_bn_relu / conv2d_transpose_bn_relu / biased conv in float64 on the given input."""
    w, b = fold(p, transposed)
    x, w = np.asarray(x, np.float64), w.astype(np.float64)
    y = (O.conv2d_transpose_same(x, w, stride) if transposed else O.conv2d_same(x, w, stride)) + b.astype(np.float64)
    return np.maximum(y, 0.0) if relu else y


def distinct_images(H, W):
    """The three input kinds, [3, H, W, 1] float32: a phantom slice, a uniform-noise slice, standard-normal noise scaled to the phantom's range."""
    from ukbb_cardiac_amd.phantom import cine_phantom, uniform_slices
    ph = cine_phantom(1, H, W, seed=17)[0]
    un = uniform_slices(1, H, W, seed=5)[0]
    z = np.random.default_rng(29).standard_normal((H, W, 1))
    lo, hi = float(ph.min()), float(ph.max())
    nz = (lo + (z - z.min()) / (z.max() - z.min()) * (hi - lo)).astype(np.float32)
    return np.stack([ph, un, nz]).astype(np.float32)


def batch_of_copies(index, n, H, W):
    """img[i] = distinct[i % 3]; a batch of one takes the three kinds in turn over the case list.  Returns (batch, number of distinct images)."""
    d = distinct_images(H, W)
    if n == 1:
        return d[index % 3:index % 3 + 1].copy(), 1
    return np.stack([d[i % 3] for i in range(n)]), min(n, 3)


def launches(arch):
    """The graph, launch by launch, as the reference defines it (common/network.py build_FCN's encoder, network_ao.py build_UNet):
    (layer name, stored name, level, input stored names, stride, transposed, relu).  '' as the input is the image."""
    nb = arch.n_block

    def stored(kind, l, i):
        return '%s%d' % (kind, l) if i == nb[l] - 1 else '%s%d_%d' % (kind, l, i)
    out = []
    for l in range(arch.n_level):
        for i in range(nb[l]):
            src = '' if (l, i) == (0, 0) else stored('conv', l - 1, nb[l - 1] - 1) if i == 0 else stored('conv', l, i - 1)
            out.append(('conv%d_%d' % (l, i), stored('conv', l, i), l, [src], 2 if (l > 0 and i == 0) else 1, False, True))
    if arch.name.startswith('UNet'):
        below = stored('conv', arch.n_level - 1, nb[-1] - 1)
        for l in range(arch.n_level - 2, -1, -1):
            out.append(('up%d_t' % l, 'up%d_t' % l, l, [below], 2, True, True))
            for i in range(nb[l]):
                src = [stored('conv', l, nb[l] - 1), 'up%d_t' % l] if i == 0 else [stored('up', l, i - 1)]      # skip first (network_ao.py:51)
                out.append(('up%d_%d' % (l, i), stored('up', l, i), l, src, 1, False, True))
            below = stored('up', l, nb[l] - 1)
        out.append(('logits', 'logits', 0, [below], 1, False, False))
    return out


def rel_err(got, ex):
    """(max |got - ex| / max |ex|, index of the worst element)."""
    d = np.abs(np.asarray(got, np.float64) - ex)
    return float(d.max()) / float(np.abs(ex).max()), tuple(int(v) for v in np.unravel_index(int(d.argmax()), d.shape))


@pytest.mark.parametrize('index', range(len(CASES)), ids=['%s-%dx%dx%d' % c for c in CASES])
def test_each_fp32_launch_against_float64_on_its_own_input(index):
    import time
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
        names, cfgs = eng.kernel_names(), eng.kernel_configs()
        stored = {'logits': out['logits']}
        for lname, sname, l, _, _, _, _ in graph:
            if lname not in ('conv0_0', 'logits'):                       # conv0_0 lives inside conv0_1's launch
                stored[sname] = eng.activation(sname).reshape(n, H >> l, W >> l, -1)
    t_gpu = time.perf_counter() - t0
    # the plan that ran is the one tests/test_fp32_launch_coverage.py counted for this case
    assert names == [o['name'] for o in plan['ops']], (names, [o['name'] for o in plan['ops']])
    assert cfgs == [o['cfg'] if o['kind'] in ('conv', 'tconv') else -1 for o in plan['ops']], (cfgs, plan['ops'])
    cfg_of = {}
    for o in plan['ops']:
        for part in o['name'].split('+'):
            cfg_of[part] = o['cfg'] if o['kind'] in ('conv', 'tconv') else -1
    assert stored['logits'].shape[:3] == (n, H, W)
    # every slice is a bit-identical copy of the graded slice of its image, in every stored map and in the logits
    for sname, a in stored.items():
        for i in range(nd, n):
            assert np.array_equal(a[i], a[i % nd]), '%s: slice %d differs from slice %d of the same image (tiling %s)' % (sname, i, i % nd, cfg_of.get(sname))
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
