"""What tests/test_custom_arch_launches_gpu.py covers, checked without a GPU (engine.plan_layout: the host-only planner on 256 compute units, built first
as for tests/test_plan_layout.py), that every descriptor of tests/custom_archs.py plans or is refused with a reason, and that the bounds the grader
imports can tell a wrong kernel from a right one at the channel counts no named model has.

UNIVERSE: the plans of every architecture of custom_archs.ARCHS in every precision its kind takes, over the shapes of tests/golden/plan_layouts.json (the
SHAPES of tests/test_plan_layout.py) at batches 1 and plan.h SMALL_BATCH + 1, computed live.  A launch's SITUATION is custom_archs.situation_of's
tuple.  NAMED: the situations of the named models' default plans -- for the precisions the golden file records (fp32, bf16) its knob-less records,
replayed and checked against the record (launch_grading.replay_records); for bf16_store, bf16_full and f32x3 with set_f32x3_convs, which it does not
record, the same shapes and batches planned live.  REQUIREMENT: every situation of the universe that is not in NAMED is reached by a case of the GPU file;
no case is idle (dropping any one leaves a situation unreached)."""
import json
import os
import re

import numpy as np
import pytest

import custom_archs as A
import launch_grading as G
import test_custom_arch_launches_gpu as L
from oracle import fcn_oracle as O

ROOT = G.ROOT
RECORDED_PRECISIONS = ('fp32', 'bf16')
MAX_H, MAX_W = 96, 128
KNOWN_KINDS = {'first', 'stem', 'conv', 'tconv', 'logits', 'tail', 'sqg', 'sqg_multi', 'head'}


def small_batch():
    with open(os.path.join(ROOT, 'ukbb_cardiac_amd', 'csrc', 'plan.h')) as f:
        return int(re.search(r'constexpr int SMALL_BATCH = (\d+);', f.read()).group(1))


def golden_axes():
    """(shapes, batches) of the recorded knob-less plans."""
    with open(G.GOLDEN) as f:
        recs = [r for r in json.load(f)['records'] if r[5] == '']
    return sorted({(r[2], r[3]) for r in recs}), sorted({r[4] for r in recs})


def accepted():
    return [k for k in A.ARCHS if k not in A.REFUSED]


@pytest.fixture(scope='module')
def universe():
    """(NAMED, {situation of the universe: [(architecture, precision, n, H, W, op names)]})."""
    from ukbb_cardiac_amd import _lib
    shapes, batches = golden_axes()
    assert len(shapes) == 8 and batches == [1, 10, 16, 17, 64, 100]
    named = set()
    for kind, models in A.NAMED.items():
        for m in models:
            for prec in A.PRECISIONS[kind]:
                if prec in RECORDED_PRECISIONS:
                    got = G.replay_records(m, prec, lambda n, H, W: set(A.situations(m, prec, n, H, W)))
                    assert got, (m, prec)
                    named |= set().union(*(g[3] for g in got))
                else:
                    for H, W in shapes:
                        for n in batches:
                            try:
                                named |= set(A.situations(m, prec, n, H, W))
                            except _lib.UkbbFcnError:
                                pass
    uni = {}
    for name in accepted():
        for prec in A.PRECISIONS[A.kind_of(name)]:
            for H, W in shapes:
                for n in (1, small_batch() + 1):
                    for s, ops in A.situations(name, prec, n, H, W).items():
                        uni.setdefault(s, []).append((name, prec, n, H, W, ops))
    return named, uni


def new_situations(universe):
    named, uni = universe
    return {s for s in uni if s not in named}


def reached(case):
    return set(A.situations(*case))


def test_cases_take_the_allowed_values(universe):
    """N = 1 or SMALL_BATCH + 1 (a UNet-LSTM: one or two sequences, below and above SMALL_BATCH frames), H and W multiples of 16; a map larger than
    96 x 128 only where the case reaches a new situation that no allowed map of any architecture and precision reaches."""
    new = new_situations(universe)
    assert len(set(L.CASES)) == len(L.CASES)
    within = set()
    for name in accepted():
        for prec in A.PRECISIONS[A.kind_of(name)]:
            for n in ((9, 18) if A.kind_of(name) == 'UNet-LSTM' else (1, small_batch() + 1)):
                for H in range(16, MAX_H + 1, 16):
                    for W in range(16, MAX_W + 1, 16):
                        within |= reached((name, prec, n, H, W)) & new
    print('custom-arch-coverage %d of the %d new situations are reached by no map within %d x %d' % (len(new - within), len(new), MAX_H, MAX_W))
    for name, prec, n, H, W in L.CASES:
        kind = A.kind_of(name)
        assert name in accepted() and prec in A.PRECISIONS[kind] and H % 16 == 0 and W % 16 == 0, (name, prec, H, W)
        assert n in ((9, 18) if kind == 'UNet-LSTM' else (1, small_batch() + 1)) and (kind != 'UNet-LSTM' or A.arch_of(name).fc == 9), (name, n)
        if H > MAX_H or W > MAX_W:
            assert n * H * W <= 9 * 208 * 256 and reached((name, prec, n, H, W)) & (new - within), (name, prec, n, H, W)


def test_cases_reach_every_new_situation_and_none_is_idle(universe):
    named, uni = universe
    new = new_situations(universe)
    print('custom-arch-coverage %d situations in the universe, %d of them in no named model\'s plan' % (len(uni), len(new)))
    # what the issue names is among them: `first`, the per-level sqg launches, the separate bf16 logits, the fused-logits tilings, the new class counts,
    # three- and five-group Winograd, two-source convs with K = 192 and 320 channels, transposed convs across an unequal pyramid
    kinds = {(s[0], s[1], s[2]) for s in new}
    assert {(k, p, 'first') for k in A.KIND_NAMES for p in A.PRECISIONS[k]} <= kinds
    assert {('FCN', p, 'sqg') for p in A.PRECISIONS['FCN']} <= kinds and ('UNet', 'bf16', 'logits') in kinds
    assert {s[3] for s in new if s[9] and s[2] == 'conv'} == {325, 404}
    assert {(s[2], s[9]) for s in new if s[9]} >= {('head', 5), ('logits', 2), ('logits', 4), ('tail', 2), ('tail', 4)}
    assert {(s[3], s[6]) for s in new if s[1] == 'fp32'} >= {(301, 96), (303, 96), (301, 160)}
    assert {(s[4], s[5]) for s in new if s[5]} >= {(96, 96), (160, 160)}
    assert {(s[4], s[6]) for s in new if s[2] == 'tconv'} >= {(160, 96), (96, 160), (96, 32)}
    only = G.no_case_is_idle(L.CASES, reached, new)
    for c, o in zip(L.CASES, only):
        print('custom-arch-case %-10s %-10s %2dx%3dx%3d  reaches %2d new situations, only it: %s' % (c + (len(reached(c) & new), '; '.join(map(str, o)))))


def test_grader_knows_every_planned_launch():
    """Every op of a case's plan is of a kind run_case grades, and names layers of launch_grading.launches' graph; a stored map is an input of no launch
    unless the plan stores it."""
    for case in L.CASES:
        name = case[0]
        p = A.plan(*case)
        stored = {a['name'] for a in p['acts']}
        graph = {g[0]: g for g in G.launches(A.arch_of(name))}
        for o in p['ops']:
            assert o['kind'] in KNOWN_KINDS, o
            if o['kind'] in ('sqg', 'sqg_multi', 'head'):
                continue
            for part in o['name'].split('+'):
                assert part in graph, (case, o)
            first = graph[o['name'].split('+')[0]]
            assert all(s in stored or s == '' for s in first[3]), (case, o, first)


def sqg_instances():
    """The C_in launch_sqg has an instance for, per input format: the case labels of its two switches (kernels_head.hip)."""
    with open(os.path.join(ROOT, 'ukbb_cardiac_amd', 'csrc', 'kernels_head.hip')) as f:
        body = re.search(r'hipError_t launch_sqg\(const SqgArgs &a, hipStream_t s\) \{.*?\n}\n', f.read(), re.S).group(0)
    switches = re.findall(r'switch \(a\.cin\) \{(.*?)default: return hipErrorInvalidValue;', body, re.S)
    assert len(switches) == 2, body
    sets = [set(map(int, re.findall(r'case (\d+):', s))) for s in switches]
    assert sets[0] == sets[1] and sets[0], sets
    return sets[0]


def test_every_descriptor_plans_or_is_refused_with_a_reason():
    """plan_layout returns a plan or raises UkbbFcnError carrying supported()'s reason; every sqg op of a returned plan has a C_in launch_sqg has an
    instance for (sqg_multi takes the standard pyramid only).  No descriptor create accepts may fail inside a forward."""
    from ukbb_cardiac_amd import _lib
    inst = sqg_instances()
    assert inst == {32, 64, 128, 256}
    shapes, _ = golden_axes()
    for name in A.ARCHS:
        arch = A.arch_of(name)
        for prec in A.PRECISIONS[A.kind_of(name)]:
            for H, W in ((32, 48), (64, 96), shapes[-1]):
                for n in (1, small_batch() + 1):
                    try:
                        p = A.plan(name, prec, n, H, W)
                    except _lib.UkbbFcnError as e:
                        assert name in A.REFUSED and '(-2)' in str(e) and A.REFUSED[name] in str(e), (name, prec, str(e))
                        continue
                    assert name not in A.REFUSED, name
                    for o in p['ops']:
                        if o['kind'] == 'sqg':
                            assert p['acts'][o['in0']]['channels'] in inst, (name, prec, o)
                        elif o['kind'] == 'sqg_multi':
                            assert tuple(arch.n_filter[1:]) == (32, 64, 128, 256), (name, o)
    assert sorted(A.REFUSED) == ['FCN-big', 'FCN-wide']


# ---- the bounds tell a defect at the new channel counts ----------------------------------------------------------------------------------------------
def bf16_trunc(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return (u & np.uint32(0xffff0000)).view(np.float32)


def rough(shape, seed):
    """A non-negative, rough stored map (what a ReLU layer leaves), float32."""
    z = np.random.default_rng(seed).standard_normal(shape)
    return np.maximum(z, 0.0).astype(np.float32)


# layer of UNet-wide, its sources' channels, map (rows, columns) of the INPUT, transposed
STAND_IN_LAYERS = [('conv2_1', (96,), (12, 8), False), ('conv3_1', (160,), (6, 4), False), ('up3_0', (160, 160), (6, 4), False),
                   ('up2_0', (96, 96), (12, 8), False), ('up2_t', (160,), (6, 4), True)]


def launch32(x, p, transposed, round_w=False):
    """The specified arithmetic of one launch in float32 numpy (before any rounding of the output)."""
    w, b = G.fold(p, transposed)
    if round_w:
        w = G.bf16_round(w)
    x = np.ascontiguousarray(x, np.float32)
    y = (O.conv2d_transpose_same(x, w, 2) if transposed else O.conv2d_same(x, w, 1)) + b
    assert y.dtype == np.float32
    return np.maximum(y, np.float32(0))


def shifted(x, axis):
    out = np.zeros_like(x)
    dst, src = [slice(None)] * 4, [slice(None)] * 4
    dst[axis], src[axis] = slice(1, None), slice(0, -1)
    out[tuple(dst)] = x[tuple(src)]
    return out


def defects(x, srcs, p, transposed, round_w):
    """{defect: float64 result of the launch with it planted}."""
    stride = 2 if transposed else 1
    w, b = G.fold(p, transposed)
    if round_w:
        w = G.bf16_round(w)
    w64, b64 = w.astype(np.float64), b.astype(np.float64)
    conv = O.conv2d_transpose_same if transposed else O.conv2d_same
    x64 = x.astype(np.float64)
    full = np.maximum(conv(x64, w64, stride) + b64, 0.0)
    out = {}
    for t in (0, 4, 8):
        wz = w64.copy()
        wz[t // 3, t % 3] = 0.0
        out['tap %d zeroed' % t] = np.maximum(conv(x64, wz, stride) + b64, 0.0)
    for axis in (1, 2):
        out['input shifted along axis %d' % axis] = np.maximum(conv(shifted(x64, axis), w64, stride) + b64, 0.0)
    if len(srcs) == 2:                                                   # [up, skip] instead of [skip, up] (network_ao.py:51)
        out['sources swapped'] = np.maximum(conv(np.concatenate([x64[..., srcs[0]:], x64[..., :srcs[0]]], axis=-1), w64, stride) + b64, 0.0)
    g = full.copy()
    g[..., 64:96] = full[..., 32:64]
    out['third 32-channel group holds the second'] = g
    return out


@pytest.mark.parametrize('lname,srcs,hw,transposed', STAND_IN_LAYERS, ids=[s[0] for s in STAND_IN_LAYERS])
def test_bounds_tell_a_defect_at_the_new_channel_counts(lname, srcs, hw, transposed):
    """C_out = 96 and 160, two sources of 96 + 96 and 160 + 160 (K = 9 x 192, 9 x 320), the transposed conv 160 -> 96.  fp32: the specified arithmetic
    in float32 numpy stays inside the grader's 1e-5 against float64, every planted defect misses it by more than 100 times.  bf16 storage (bf16 values
    in, bf16-rounded weights, the result rounded once): the float32 stand-in passes grade(0.5, 1.0) -- every element; every planted defect puts its worst
    element more than 100 times the tolerance away; truncation instead of round-to-nearest-even on the store (at most one ulp, against half) leaves at
    most 60 % of the non-zero elements inside."""
    from ukbb_cardiac_amd.weights import synthetic_params
    p = synthetic_params(A.arch_of('UNet-wide'), G.SEEDS[0])[lname]
    x = rough((3,) + hw + (sum(srcs),), 11)
    stride = 2 if transposed else 1
    # fp32
    full = G.layer(x, p, stride, transposed)
    assert full.shape[-1] in (96, 160) and full.max() > 0
    err = G.rel_err(launch32(x, p, transposed), full)[0]
    print('custom-arch-stand-in %-8s fp32 stand-in err/scale %.2e (bound %.0e)' % (lname, err, L.BOUND))
    assert err <= L.BOUND
    for d, y in defects(x, srcs, p, transposed, False).items():
        e = G.rel_err(y, full)[0]
        assert e > 100 * L.BOUND, (lname, d, e)
    # bf16 storage
    xb = G.bf16_round(x)
    full = G.layer(xb, p, stride, transposed, round_w=True)
    sc = float(np.abs(full).max())
    pre = launch32(xb, p, transposed, round_w=True)
    share, worst = G.measure(G.bf16_round(pre), full, sc)
    print('custom-arch-stand-in %-8s bf16 stand-in within half an ulp %.6f, worst / bound %.3f' % (lname, share, worst))
    G.grade(lname, G.bf16_round(pre), full, sc, ulps=0.5, fraction=1.0)
    planted = {d: G.bf16_round(y.astype(np.float32)) for d, y in defects(xb, srcs, p, transposed, True).items()}
    planted['truncating store'] = bf16_trunc(pre)
    for d, y in planted.items():
        share, worst = G.measure(y, full, sc)
        if d == 'truncating store':                                      # off by up to one ulp, downwards: about half of the non-zero elements miss
            pos = full > 0
            inside = float(np.mean(np.abs(y.astype(np.float64) - full)[pos] <= G.tolerance(full, sc, 0.5)[pos]))
            assert inside <= 0.6 and worst > 1.5, (lname, d, inside, worst)
        else:
            assert share < 1.0 and worst > 100, (lname, d, share, worst)
