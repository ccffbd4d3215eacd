"""What tests/test_fp32_launches_gpu.py covers, checked without a GPU (engine.plan_layout: the host-only planner, built first as for
tests/test_plan_layout.py), and that its 1e-5 bound can tell a wrong kernel from a right one.

Completeness: every (model, layer, tiling) combination in the recorded default fp32 plans of FCN_sa and UNet_ao (tests/golden/plan_layouts.json: knob
'', rc 0; 121 combinations) is planned by some entry of CASES.  A stride-2 or Winograd combination counts only where the case reaches it in a
situation -- tiles dividing the map, or not -- that some recorded plan of that combination has: the stride-2 producer/consumer tilings run a
straight-line producer where their tiles divide the map (csrc/plan.cpp choose_cfg_raw), and every recorded plan of 124 / 141 / 142 / 145 does.
Per tiling, CASES also reaches it on a map its tiles divide, and on one they do not, wherever the recorded plans contain both.  Tile sizes are read
from the tiling's name (ukbb_fcn_conv_config_name of the plan op's `cfg`: "..._t<rows>x<columns>...") and the op's Ho / Wo.
No case is idle: dropping any one entry of CASES leaves one of these requirements unmet."""
import collections
import os
import re

import numpy as np
import pytest

import launch_grading as G
import test_fp32_launches_gpu as L
from oracle import fcn_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS_GRADED = ('FCN_sa', 'UNet_ao')


def reached(model, n, H, W):
    """{(model, layer, tiling): 'div' | 'nodiv' | None} of the default fp32 plan; None for what is neither a stride-2 nor a Winograd conv."""
    from ukbb_cardiac_amd import engine
    from ukbb_cardiac_amd.arch import MODELS
    out = {}
    for o in engine.plan_layout(MODELS[model], 'fp32', n, H, W)['ops']:
        if o['kind'] not in ('conv', 'tconv') or o['cfg'] < 0:
            continue
        fit = None
        if o['kind'] == 'conv' and (o['stride'] == 2 or 'winograd' in G.config_name(o['cfg'])):
            fit = 'div' if G.fit_of(o) == 'div' else 'nodiv'
        out[(model, o['name'], o['cfg'])] = fit
    return out


@pytest.fixture(scope='module')
def recorded():
    """{combination: set of situations} over the recorded default fp32 plans of the two models (G.replay_records)."""
    rec = collections.defaultdict(set)
    for model in MODELS_GRADED:
        for _, _, _, got in G.replay_records(model, 'fp32', lambda n, H, W: reached(model, n, H, W)):
            for k, fit in got.items():
                rec[k].add(fit)
    return dict(rec)


def requirements(rec):
    """The combinations, and per stride-2 / Winograd tiling the situations the recorded plans contain."""
    return set(rec) | {(k[2], fit) for k, fits in rec.items() for fit in fits if fit}


def covered(cases, rec):
    got = set()
    for c in cases:
        for k, fit in reached(*c).items():
            if k in rec and fit in rec[k]:
                got.add(k)
            if fit:
                got.add((k[2], fit))
    return got


def test_cases_reach_every_recorded_combination(recorded):
    assert len(recorded) == 121
    assert len(set(L.CASES)) == len(L.CASES) and all(m in MODELS_GRADED and H % 16 == 0 and W % 16 == 0 for m, n, H, W in L.CASES)
    missing = set(recorded) - covered(L.CASES, recorded)
    assert not missing, sorted(missing, key=str)
    # the tilings the issue names, where it names them
    ids = {k[2] for k in recorded}
    assert {124, 145, 304, 307, 300, 302, 130, 60, 62, 11} <= ids
    assert all(recorded[k] == {'div'} for k in recorded if k[2] in (124, 141, 142, 145))


def test_cases_reach_every_tiling_on_maps_its_tiles_divide_and_do_not(recorded):
    want = {r for r in requirements(recorded) if len(r) == 2}
    assert {t for t, fit in want if fit == 'div'} >= {124, 145, 142, 307, 304} and (300, 'nodiv') in want
    missing = want - covered(L.CASES, recorded)
    assert not missing, sorted(missing)


def test_no_case_is_idle(recorded):
    G.no_case_is_idle(L.CASES, lambda c: covered([c], recorded), requirements(recorded))


def test_large_batch_cases_are_above_the_small_batch_threshold():
    with open(os.path.join(ROOT, 'ukbb_cardiac_amd', 'csrc', 'plan.h')) as f:
        small = int(re.search(r'constexpr int SMALL_BATCH = (\d+);', f.read()).group(1))
    assert {n for _, n, _, _ in L.CASES} == {1, small + 1}


def test_graph_lists_every_planned_conv_launch():
    """launches() names exactly the conv / transposed conv / logits launches of the plans (the FCN squeeze and head stay out)."""
    from ukbb_cardiac_amd import engine
    from ukbb_cardiac_amd.arch import MODELS
    for model, n, H, W in L.CASES:
        ops = engine.plan_layout(MODELS[model], 'fp32', n, H, W)['ops']
        planned = [part for o in ops if o['kind'] in ('conv', 'tconv', 'logits') for part in o['name'].split('+')]
        graph = [g[0] for g in G.launches(MODELS[model]) if not (g[0] == 'logits' and model.startswith('FCN'))]
        assert planned == graph, (model, planned, graph)
        stored = {a['name'] for a in engine.plan_layout(MODELS[model], 'fp32', n, H, W)['acts']}
        assert {g[1] for g in G.launches(MODELS[model]) if g[0] not in ('conv0_0', 'logits')} <= stored


def test_batch_of_copies():
    img, nd = G.batch_of_copies(0, 17, 32, 48)
    assert img.shape == (17, 32, 48, 1) and nd == 3 and img.dtype == np.float32
    assert all(np.array_equal(img[i], img[i % 3]) for i in range(17)) and not np.array_equal(img[0], img[1]) and not np.array_equal(img[1], img[2])
    d = G.distinct_images(32, 48)
    assert d[2].min() == d[0].min() and d[2].max() == d[0].max()
    assert [float(G.batch_of_copies(i, 1, 32, 48)[0].sum()) for i in range(3)] == [float(d[i].sum()) for i in range(3)]


def test_bound_tells_a_wrong_tap_and_a_shifted_input():
    """The bound is not vacuous: on one small layer (FCN_sa conv1_1, 32 -> 32 channels, on conv0_0 -> conv1_0 of each of the three input kinds)
    a float64 reference with any one of the nine taps zeroed, or fed its input shifted by one pixel, misses 1e-5 of the layer's scale against the
    full reference -- by orders of magnitude, so a kernel with that defect cannot pass -- while the full reference evaluated in float32 passes."""
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.weights import synthetic_params
    params = synthetic_params(MODELS['FCN_sa'], G.SEEDS[0])
    w, b = G.fold(params['conv1_1'])
    w64, b64 = w.astype(np.float64), b.astype(np.float64)
    for kind, img in enumerate(G.distinct_images(48, 32)):
        x = G.layer(G.layer(img[None], params['conv0_0']), params['conv1_0'], stride=2).astype(np.float32).astype(np.float64)
        full = G.layer(x, params['conv1_1'])
        assert full.shape == (1, 24, 16, 32) and full.max() > 0
        f32 = np.maximum(O.conv2d_same(x.astype(np.float32), w, 1) + b, np.float32(0))
        assert G.rel_err(f32, full)[0] <= L.BOUND
        for ky in range(3):
            for kx in range(3):
                wz = w64.copy()
                wz[ky, kx] = 0.0
                err, _ = G.rel_err(np.maximum(O.conv2d_same(x, wz, 1) + b64, 0.0), full)
                assert err > 100 * L.BOUND, (kind, ky, kx, err)
        for axis in (1, 2):
            shifted = np.zeros_like(x)
            sl = [slice(None)] * 4
            src = list(sl)
            sl[axis], src[axis] = slice(1, None), slice(0, -1)
            shifted[tuple(sl)] = x[tuple(src)]
            err, _ = G.rel_err(G.layer(shifted, params['conv1_1']), full)
            assert err > 100 * L.BOUND, (kind, axis, err)
