"""Every bf16-operand conv launch of the FCN plans (--precision bf16 on an FCN handle: UKBB_PREC_BF16, plan.cpp plan_mode: Bf16Mode::Operands), one launch at a time,
against float64 on the engine's OWN stored input.

On an FCN handle UKBB_PREC_BF16 keeps fp32 activations in HBM and takes ConvFamily::Bf16Operands, the tilings UKBB_BF_CONFIGS 200-221 of kernels_conv.hip:
the BF && !BFIO branch of conv_mfma_kernel, which exists nowhere else -- every staged float4 through pack_bf16x2 (RNE) into LDS at a halo pixel
stride of KC / 2 + 4, weights rounded on the host by the bf16 weight packer, one bf16 MFMA per tap and chunk, fp32 NHWC stores.  The other graders
stop in front of it (tests/test_fp32_launches_gpu.py: fp32 plans; tests/test_bf16_launches_gpu.py: the bf16-STORAGE U-Net, ConvFamily::Bf16Store / Bf16StoreWs), and the tests
that run this mode compare it with itself.  A bf16 x bf16 product is exact in fp32, so one launch differs from float64 on the rounded operands only
by its fp32 accumulation:

    convBF16_... launch     expected  relu(conv(bf16_round(x stored), bf16_round(fold(w))) + b)   in float64 (layer with round_w and round_x)
    any other launch        expected  the fp32 model of tests/test_fp32_launches_gpu.py (130: the fused first layer conv0_0 + conv0_1, from the image)

The model is decided per launch from its tiling's name (ukbb_fcn_conv_config_name), not from the mode.  Per launch max |engine - model| <= BOUND x
the layer's largest activation (rel_err); per bf16-tiling launch the engine's map must ALSO be >= 10 x BOUND away from the fp32 model of the same
launch (operands not rounded), which a layer that quietly ran an fp32 tiling would not be; and every conv from conv1_0 on must be on a convBF16_
tiling, as the recorded plans say.  The plan that ran (kernel_names() / kernel_configs()) must be the one the CPU test counted (plan_layout on 256
compute units).  Method, inputs and helpers are the graders' common ones (tests/launch_grading.py), as tests/test_fp32_launches_gpu.py uses them:
one forward per case with want_logits, every stored encoder map and the logits under the copy identity.  The squeeze and head launches behind this
encoder are graded in tests/test_head_launches_gpu.py (mode 'bf16').

CASES: FCN_sa (the records of FCN_la_2ch / FCN_la_4ch / FCN_la_4ch_seg4 are identical, tests/test_bf16_operand_launch_coverage.py), N = 1 or 17 =
plan.h SMALL_BATCH + 1, H and W multiples of 16: a greedy cover, cheapest first (pixels + 25 x float64 pixels), of the 25 (layer, tiling)
combinations of the recorded knob-less bf16 plans -- 130 for the fused first layer, 211 / 210 for the stride-2 layers, 200 / 201 / 202 for the
stride-1 layers -- each on a map its tiles divide, or not (whole tiles and a ragged last one, or one partial tile only), as some recorded plan of
that combination has it, and of every (tiling, fit, batch up to / above SMALL_BATCH) the records hold: 53 requirements; reduced until dropping any one
case leaves a requirement unmet (the CPU test prints what only each case reaches).  None is the benchmark's batch.  Pixels = N x H x W; float64 pixels =
min(N, 3) x H x W.

    case   N    H    W    pixels  float64 pixels  weights  batch-1 image
       0   1   48   16       768             768     1234  phantom
       1   1   32   32      1024            1024        7  uniform
       2   1   80   16      1280            1280     1234  normal
       3   1   16  160      2560            2560        7  phantom
       4   1  208   16      3328            3328     1234  uniform
       5   1  192  208     39936           39936        7  normal
       6  17   48   16     13056            2304     1234  -
       7  17   32   32     17408            3072        7  -
       8  17   80   16     21760            3840     1234  -
       9  17   16  112     30464            5376        7  -
      10  17   16  160     43520            7680     1234  -
      11  17  192  208    678912          119808        7  -
    all                   854016          190976

FORCED_CASES: tilings 203 (3x3 s1, 16 x 16, w2x2) and 212 (3x3 s2, 8 x 16, w2x2) are registered, but no recorded plan takes them; one fresh child
process with UKBB_CONV_CFG naming 203 for every stride-1 layer from conv1_1 on and 212 for every stride-2 layer grades two cases with the same code
and bound: 1 x 256 x 256 (the 16 x 16 and 8 x 16 tiles divide the map of every level, 16 x 16 at level 4) and 1 x 80 x 112 (they divide none: 20 x 28,
10 x 14, 5 x 7; 40 x 56 at level 1).  Both tilings compute 64 output channels per workgroup (w2x2: two 32-row blocks), so cfg_valid refuses them for
the 32-channel layers of level 1 and the override is ignored there: conv1_0 and conv1_1 stay on 211 / 202 in the child, and it asserts exactly that
-- 212 / 203 on every layer with Cout % 64 == 0, a convBF16_ tiling on the other two.

BOUND = 1e-5, the project's fp32 launch bound: the reference is the float64 rounding model, never another run of the engine, and what is left of a
bf16-operand launch is its fp32 accumulation.  Measured on an MI355X (profiles/bf16_operand_launches.txt, one row per launch, worst launch per tiling
in its last block): 8e-8 .. 8.4e-7 of the layer's scale over the 12 cases and the child (worst per tiling: 130 4.0e-7, 200 8.4e-7, 201 5.2e-7,
202 4.2e-7, 203 5.0e-7, 210 3.6e-7, 211 2.6e-7, 212 3.1e-7) -- below 2.5e-6, so the bound keeps the fourfold margin the fp32 file has; every
bf16-tiling launch 1.5e-3 .. 5e-3 from the fp32 model of the launch, no copy differing.  The file takes 6 s, 2.5 s of it the child starting Python; the
largest case 0.02 s of forward and read-back and 0.2 s of float64.  With the weight packer truncating instead of rounding (a throw-away build) all 13
tests fail: each of the 143 bf16-tiling launches that ran (the child stops after its first case) misses the bound, at 2.7e-3 .. 7.0e-3, and the 130
launches still pass."""
import json
import os
import time

import pytest

from launch_grading import CUS, SEEDS, assert_plan_ran, batch_of_copies, check_copies, config_name, launches, layer, rel_err, run_in_child, tile_of

pytestmark = pytest.mark.gpu
BOUND = 1e-5
APART = 10 * BOUND                      # a bf16-tiling launch is at least this far from the fp32 model of the same launch
MODEL = 'FCN_sa'
BF_PREFIX = 'convBF16_'

CASES = [(1, 48, 16), (1, 32, 32), (1, 80, 16), (1, 16, 160), (1, 208, 16), (1, 192, 208), (17, 48, 16), (17, 32, 32), (17, 80, 16), (17, 16, 112), (17, 16, 160),
         (17, 192, 208)]

# the registered ConvFamily::Bf16Operands tilings no recorded plan reaches: forced in one child process
FORCED_CASES = [(1, 256, 256), (1, 80, 112)]
FORCED_S1, FORCED_S2 = 203, 212


def is_bf16_tiling(cfg):
    return cfg >= 0 and config_name(cfg).startswith(BF_PREFIX)


def grade_forward(index, n, H, W):
    """One bf16 forward of FCN_sa, every conv launch graded.  Prints one row per launch and returns the rows
    (layer, tiling, err/scale against the launch's model, worst element, distance from the fp32 model or None, tag)."""
    from ukbb_cardiac_amd import engine
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.weights import synthetic_params
    seed = SEEDS[index % 2]
    arch = MODELS[MODEL]
    params = synthetic_params(arch, seed)
    img, nd = batch_of_copies(index, n, H, W)
    plan = engine.plan_layout(arch, 'bf16', n, H, W, CUS)
    graph = [g for g in launches(arch) if g[0] != 'logits']
    t0 = time.perf_counter()
    with engine.Engine(arch, params) as eng:
        eng.set_precision('bf16')
        out = eng.run(img, want_logits=True)
        assert_plan_ran(eng, plan)                                       # the plan tests/test_bf16_operand_launch_coverage.py counted for this case
        stored = {'logits': out['logits']}
        for lname, sname, l, _, _, _, _ in graph:
            if lname != 'conv0_0':                                       # conv0_0 lives inside conv0_1's launch
                stored[sname] = eng.activation(sname).reshape(n, H >> l, W >> l, -1)
    t_gpu = time.perf_counter() - t0
    cfg_of = {part: o['cfg'] for o in plan['ops'] if o['kind'] == 'conv' for part in o['name'].split('+')}
    assert set(cfg_of) == {g[0] for g in graph}, (sorted(cfg_of), graph)
    not_bf = [(k, c) for k, c in cfg_of.items() if k not in ('conv0_0', 'conv0_1') and not is_bf16_tiling(c)]
    assert not not_bf, 'convs of a bf16 plan on a tiling that is no %s tiling: %s' % (BF_PREFIX, not_bf)
    assert stored['logits'].shape == (n, H, W, arch.n_class)
    # every slice is a bit-identical copy of the graded slice of its image, in every stored map and in the logits
    for sname, a in stored.items():
        check_copies(sname, a, nd, '(tiling %s)' % cfg_of.get(sname))
    t0 = time.perf_counter()
    tag = '%-8s %2dx%3dx%3d' % (MODEL, n, H, W)
    rows = []
    fused_first = None
    for lname, sname, l, srcs, stride, transposed, relu in graph:
        cfg = cfg_of[lname]
        if lname == 'conv0_0':                                           # fused first layer: conv0_0 in float64 from the image, then conv0_1, as a unit
            assert not is_bf16_tiling(cfg) and cfg == cfg_of['conv0_1']
            fused_first = layer(img[:nd], params[lname])
            continue
        x = fused_first if lname == 'conv0_1' else stored[srcs[0]][:nd]
        fp32_model = layer(x, params[lname], stride)
        if is_bf16_tiling(cfg):
            err, where = rel_err(stored[sname][:nd], layer(x, params[lname], stride, round_w=True, round_x=True))
            apart = rel_err(stored[sname][:nd], fp32_model)[0]
        else:
            (err, where), apart = rel_err(stored[sname][:nd], fp32_model), None
        rows.append((lname, cfg, err, where, apart, tag))
        print('bf16op-launch %s seed %4d  %-8s tiling %3d  err/scale %.2e  worst at %s  from the fp32 model %s' % (
            tag, seed, lname, cfg, err, where, '-' if apart is None else '%.2e' % apart))
    print('bf16op-launch %s forward + read-back %.2f s, float64 reference %.2f s' % (tag, t_gpu, time.perf_counter() - t0))
    return rows


def check_rows(rows):
    bad = [r[:4] for r in rows if not r[2] <= BOUND]
    assert not bad, 'launches over %g of their layer\'s scale (layer, tiling, error, worst element [slice, y, x, channel]): %s' % (BOUND, bad)
    fp32_like = [(r[0], r[1], r[4]) for r in rows if r[4] is not None and not r[4] >= APART]
    assert not fp32_like, 'bf16-tiling launches closer than %g to the fp32 model of the launch: operands not rounded? (layer, tiling, distance) %s' % (APART, fp32_like)


@pytest.mark.parametrize('index', range(len(CASES)), ids=['%dx%dx%d' % c for c in CASES])
def test_each_bf16_operand_launch_against_float64_on_its_own_input(index):
    rows = grade_forward(index, *CASES[index])
    assert len(rows) == 12 and sum(r[4] is not None for r in rows) == 11                # the fused first layer and conv1_0 .. conv4_2
    check_rows(rows)


# ---- tilings 203 and 212: one child process with UKBB_CONV_CFG ------------------------------------------------------------------------------------------
def forced_spec():
    """UKBB_CONV_CFG for the child: 203 for every stride-1 layer from conv1_1 on, 212 for every stride-2 layer."""
    from ukbb_cardiac_amd.arch import MODELS
    return ','.join('%s:%d' % (g[0], FORCED_S2 if g[4] == 2 else FORCED_S1) for g in launches(MODELS[MODEL]) if g[0] not in ('conv0_0', 'conv0_1', 'logits'))


def forced_expectation():
    """{layer: the tiling the child must run}: the forced one where cfg_valid admits it (64 output channels per workgroup), None (any convBF16_
    tiling but the forced ones) at the 32-channel level 1."""
    from ukbb_cardiac_amd.arch import MODELS
    arch = MODELS[MODEL]
    return {g[0]: (FORCED_S2 if g[4] == 2 else FORCED_S1) if arch.n_filter[g[2]] % 64 == 0 else None
            for g in launches(arch) if g[0] not in ('conv0_0', 'conv0_1', 'logits')}


def run_child(path):
    """In a process started with UKBB_CONV_CFG = forced_spec(): assert that 203 / 212 ran, grade FORCED_CASES."""
    from ukbb_cardiac_amd import engine
    from ukbb_cardiac_amd.arch import MODELS
    assert os.environ.get('UKBB_CONV_CFG') == forced_spec() and not [k for k in os.environ if k.startswith('UKBB_') and k != 'UKBB_CONV_CFG']
    out = []
    for index, (n, H, W) in enumerate(FORCED_CASES):
        rows = grade_forward(index, n, H, W)                              # asserts kernel_configs() == plan_layout's, here under the same knob
        ran = {r[0]: r[1] for r in rows}
        want = forced_expectation()
        assert len(want) == 11 and sum(v is not None for v in want.values()) == 9
        for lname, cfg in want.items():
            assert ran[lname] == cfg if cfg is not None else (is_bf16_tiling(ran[lname]) and ran[lname] not in (FORCED_S1, FORCED_S2)), (lname, ran[lname], cfg)
        fits = set()
        for o in engine.plan_layout(MODELS[MODEL], 'bf16', n, H, W, CUS)['ops']:
            if o['cfg'] in (FORCED_S1, FORCED_S2):
                th, tw = (16, 16) if o['cfg'] == FORCED_S1 else (8, 16)
                assert tile_of(o['cfg']) == (th, tw)
                fits.add(o['Ho'] % th == 0 and o['Wo'] % tw == 0)
        assert fits == {index == 0}, (n, H, W, fits)                       # case 0: the tiles divide every map; case 1: none
        check_rows(rows)
        out += [(index,) + r[:3] + (r[4],) for r in rows]
    with open(path, 'w') as f:
        json.dump(out, f)


def test_forced_tilings_203_and_212_against_float64(tmp_path):
    path = str(tmp_path / 'rows.json')
    r = run_in_child('test_bf16_operand_launches_gpu', 'run_child', [path], {'UKBB_CONV_CFG': forced_spec()})
    print(''.join('UKBB_CONV_CFG=203/212 ' + ln + '\n' for ln in r.stdout.splitlines() if ln.startswith('bf16op-launch')), end='')
    assert r.returncode == 0, r.stdout[-3000:]
    with open(path) as f:
        rows = json.load(f)
    assert len(rows) == 12 * len(FORCED_CASES)
    assert sorted(r[2] for r in rows if r[2] in (FORCED_S1, FORCED_S2)) == sorted([FORCED_S2] * 3 * 2 + [FORCED_S1] * 6 * 2)
