"""Every launch of the FCN plans under --precision bf16_store (UKBB_PREC_BF16_STORE, include/ukbb_fcn.h), one launch at a time, against float64 on the
engine's OWN stored inputs.

The mode runs the FCN encoder on the bf16-storage kernels of the aortic U-Net (the fused stem of kernels_stem.hip, the tile-per-workgroup tilings
230-248 and the weight-stationary walkers 400 / 401 / 402 of kernels_ws.hip), stores every encoder map as bf16, channel-blocked, and feeds the squeeze
launches and the head through their bf16 loaders (kernels_head.hip bf16_block_to_k), behind which they are the fp32 launches.  So:

    conv0_0+conv0_1   the stem as a unit, with its intermediate rounding: stem_reference / grade_stem of tests/test_bf16_launches_gpu.py
    conv1_0 .. conv4_2  float64 on the stored bf16 input with the bf16-rounded folded kernel (layer(round_w=True) of tests/launch_grading.py), the result rounded once:
                      grade(ulps = 0.5, fraction = 1.0) of that file -- half a bf16 ulp + 2^-18 |exact| + 2^-20 scale, for EVERY element
    g1 .. g4          the fp32 squeeze model of tests/test_head_launches_gpu.py (squeeze_map) on the stored conv_l, max |engine - f64| <= 1e-5 max |f64|
    logits            the head as a unit (head_logits of that file) from the stored conv0 and the stored g1..g4, <= 1e-5 of the logits' scale
    prob              within 1e-6 of a float64 softmax of the engine's own logits;  pred == argmax(prob) exactly, over all slices

The method is the graders' common one (tests/launch_grading.py) on a guarded, poisoned engine, as in tests/test_bf16_launches_gpu.py: a tile nobody
wrote holds NaN.  The plan that ran (kernel_names() / kernel_configs()) must be the planner's (engine.plan_layout on 256 compute units), which is what
tests/test_fcn_bf16_store.py counts.  Inputs: normalised_copies; slices 0..2 are graded and every further slice of every stored map, of g1..g4, logits,
prob and pred must be bit-identical to the graded copy of its image.  Every encoder map holds bf16 values only, no map holds NaN, no guard is
damaged.  Weights from seeds 1234 and 7 in turn; the four models (4, 2, 3 and 6 classes) in turn.

CASES: a greedy cover, cheapest first (pixels + 25 x float64 pixels) and then reduced until no case is idle, of the 88 (layer, tiling, fit, walker
round class) situations the bf16_store plans of the four models hold over the SHAPES x BATCHES of tests/test_plan_layout.py; tests/test_fcn_bf16_store.py
computes them, prints what only each case reaches and shows that the grade tells planted defects.

Non-default launches: the squeeze and head knobs are latched per process, so for each of UKBB_SIDE_STREAM=1 (the stand-alone squeeze kernels behind the
bf16 loader), UKBB_HEAD_DIRECT_GATHER=1 and UKBB_HEAD_INLINE_TAIL=1 (the head's other two fp32 forms behind it) one fresh child process grades
CHILD_CASES in the same way, after asserting that the form meant ran.

Measured on an MI355X: profiles/fcn_bf16_store.txt (worst figure per tiling and per squeeze / head launch): every encoder element of every case within the
half-ulp grade; g1..g4 <= 4.3e-7, logits <= 5.5e-7 of their scale, prob <= 2.1e-7.  The 22 cases take 14 s together, the largest 1.5 s; each child 3 s."""
import os
import time

import numpy as np
import pytest

import test_bf16_launches_gpu as B                                 # the stem as a unit: stem_reference, grade_stem
import test_head_launches_gpu as HL                                # the squeeze and head models, their bounds and knobs
from launch_grading import (CUS, POISON, SEEDS, Report, assert_plan_ran, check_copies, fetcher, fit_of, grade, guarded_engine, launch_class, launches, layer,
                            normalised_copies, rel_err, run_in_child, stem_launch)

pytestmark = pytest.mark.gpu
PREC = 'bf16_store'
MODELS_IN_TURN = ('FCN_sa', 'FCN_la_2ch', 'FCN_la_4ch', 'FCN_la_4ch_seg4')
BOUND = HL.BOUND                                                   # 1e-5: squeeze and head, of the launch's scale
PROB_ATOL = HL.PROB_ATOL                                           # 1e-6

KNOBS = HL.KNOBS                                                   # UKBB_SIDE_STREAM, UKBB_HEAD_DIRECT_GATHER, UKBB_HEAD_INLINE_TAIL
CHILD_CASES = (0, 1, 3, 6)                                         # one small case per model (4, 2, 6 and 3 classes)
DEFAULT_TAIL = ('sqg1-4', 'head')

CASES = [(1, 48, 16), (1, 32, 32), (1, 32, 48), (1, 16, 112), (1, 112, 16), (1, 48, 80), (1, 80, 144), (1, 144, 144), (1, 192, 208), (1, 208, 256),
         (1, 256, 256), (129, 16, 224), (129, 16, 256), (128, 32, 224), (129, 64, 208), (129, 64, 256), (129, 128, 208), (9, 256, 256), (16, 256, 256),
         (17, 256, 256), (128, 128, 256), (129, 128, 256)]


def model_of(index):
    return MODELS_IN_TURN[index % 4]


# ---- the situation of a launch (host arithmetic; tests/test_fcn_bf16_store.py counts them) ----
def situations(n, H, W, model='FCN_sa'):
    """{(layer, tiling, fit, walker round class)} of the bf16_store plan's encoder launches ('-' where there is no tile fit / no walker)."""
    from ukbb_cardiac_amd import engine
    from ukbb_cardiac_amd.arch import MODELS
    p = engine.plan_layout(MODELS[model], PREC, n, H, W, CUS)
    out = set()
    for o in p['ops']:
        if o['kind'] == 'stem':
            out.add((o['name'], -1, '-', stem_launch(n, H, W)['cls']))
        elif o['kind'] == 'conv':
            out.add((o['name'], o['cfg'], fit_of(o), launch_class(o, p['acts'], n)))
    return out


# ---- grading ----
def grade_fcn(arch, params, ops, img, conv, g, out, report):
    """Every launch on the graded slices.  img [nd, H, W, 1]; conv[sname] / g[l] the stored maps of those slices; out: logits, prob, pred of ALL slices.
    Returns the squeeze / head rows [(launch, figure, bound)]."""
    nd = img.shape[0]
    first = [o for o in ops if 'conv0_0' in o['name'].split('+')]
    assert len(first) == 1 and first[0]['name'] == 'conv0_0+conv0_1' and first[0]['kind'] == 'stem', first
    for lname, sname, l, srcs, stride, transposed, relu in launches(arch):
        if lname in ('conv0_0', 'logits'):
            continue
        if lname == 'conv0_1':
            ex, slack, n_amb = B.stem_reference(img, params, 'stem')
            sc = float(np.abs(ex).max())
            report.row(lname, conv[sname], ex, sc)
            B.grade_stem(conv[sname], ex, sc, slack)
            continue
        ex = layer(conv[srcs[0]], params[lname], stride, round_w=True)
        sc = float(np.abs(ex).max())
        report.row(lname, conv[sname], ex, sc)
        grade('%s (tiling %d)' % (lname, report.op_of[lname]['cfg']), conv[sname], ex, sc, ulps=0.5, fraction=1.0)
    rows = []
    for l in range(1, 5):
        rows.append(('g%d' % l, rel_err(g[l], HL.squeeze_map(conv['conv%d' % l], params, l))[0], BOUND))
    ex_logits = HL.head_logits(conv['conv0'], g, params)
    rows.append(('logits', rel_err(out['logits'][:nd], ex_logits)[0], BOUND))
    rows.append(('prob', float(np.abs(out['prob'].astype(np.float64) - HL.softmax64(out['logits'])).max()), PROB_ATOL))
    for launch, fig, bound in rows:
        print('fcn-bf16-store %-26s %-7s %.2e (bound %.0e)' % (report.tag, launch, fig, bound))
    assert np.array_equal(out['pred'], np.argmax(out['prob'], axis=-1).astype(np.int32)), 'pred != argmax(prob)'
    bad = [r for r in rows if not r[1] <= r[2]]
    assert not bad, 'squeeze / head launches over their bound (launch, figure, bound): %s' % (bad,)
    return rows


def run_case(index, monkeypatch, want_tail=DEFAULT_TAIL):
    """One guarded, poisoned forward of case ``index``, every launch graded; returns (report rows of the encoder, squeeze / head rows).
    want_tail: the plan's squeeze and head ops."""
    from ukbb_cardiac_amd import engine
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.weights import synthetic_params
    n, H, W = CASES[index]
    model = model_of(index)
    arch = MODELS[model]
    params = synthetic_params(arch, SEEDS[index % 2])
    img, nd = normalised_copies(index, n, H, W)
    plan = engine.plan_layout(arch, PREC, n, H, W, CUS)
    ops = plan['ops']
    tag = '%s %dx%dx%d' % (model, n, H, W)
    t0 = time.perf_counter()
    conv, g = {}, {}
    with guarded_engine(monkeypatch, arch, params, PREC) as eng:
        eng.reserve(n, H, W)
        eng.poison(POISON)
        out = eng.run(img, want_logits=True, want_prob=True, want_pred=True)
        t_fwd = time.perf_counter() - t0
        assert_plan_ran(eng, plan)
        assert [o['name'] for o in ops if o['kind'] in ('sqg', 'sqg_multi', 'head')] == list(want_tail) and plan['bfio']
        level = {gr[1]: gr[2] for gr in launches(arch)}
        fetch = fetcher(eng, lambda s: (n, H >> level[s], W >> level[s], -1), nd, conv, tag)     # bf16 values, no poison, copies identical
        for gr in launches(arch):
            if gr[0] not in ('conv0_0', 'logits'):
                fetch(gr[1])
        for l in range(1, 5):
            a = eng.activation('g%d' % l).reshape(n, H >> l, W >> l, 64)
            check_copies('g%d' % l, a, nd, tag)
            g[l] = a[:nd].copy()
        damaged, where = eng.check_guards()
        assert damaged == 0, where
    assert out['logits'].shape == (n, H, W, arch.n_class) and out['prob'].shape == out['logits'].shape and out['pred'].shape == (n, H, W)
    for k in ('logits', 'prob', 'pred'):
        check_copies(k, out[k], nd, tag)
    t_gpu = time.perf_counter() - t0
    t0 = time.perf_counter()
    report = Report(tag, ops, plan['acts'], n)
    try:
        tail_rows = grade_fcn(arch, params, ops, img[:nd], conv, g, out, report)
    finally:
        print('fcn-bf16-store %-26s forward %.2f s, + read-back and identity %.2f s, float64 %.2f s' % (tag, t_fwd, t_gpu, time.perf_counter() - t0))
    return report.rows, tail_rows


@pytest.mark.parametrize('index', range(len(CASES)), ids=['%s-%dx%dx%d' % ((model_of(i),) + c) for i, c in enumerate(CASES)])
def test_each_bf16_store_launch_against_its_specified_arithmetic(index, monkeypatch):
    enc, tail = run_case(index, monkeypatch)
    assert len(enc) == 12 and len(tail) == 6                      # the stem, conv1_0 .. conv4_2; g1 .. g4, logits, prob


# ---- non-default squeeze and head forms: one child process per knob ---------------------------------------------------------------------------------
def run_child(knob):
    """In a process started with ``knob``=1: grade CHILD_CASES, after checking that the form meant is the one that runs."""
    from ukbb_cardiac_amd import _lib
    assert os.environ.get(knob) == '1' and not [k for k in os.environ if k.startswith('UKBB_') and k != knob]
    side = knob == 'UKBB_SIDE_STREAM'
    mp = pytest.MonkeyPatch()
    try:
        for index in CHILD_CASES:
            enc, tail = run_case(index, mp, ('sqg1', 'sqg2', 'sqg3', 'sqg4', 'head') if side else DEFAULT_TAIL)
            assert len(enc) == 12 and len(tail) == 6
            # the head reports the in-stage form (1) under either head knob, the deferred default (0) otherwise (kernels_head.hip launch_head_pc_nc)
            assert int(_lib.lib.ukbb_fcn_head_tail_form()) == (0 if side else 1)
    finally:
        mp.undo()
    print('child done')


@pytest.mark.parametrize('knob', KNOBS)
def test_non_default_squeeze_and_head_forms_against_float64(knob):
    r = run_in_child('test_fcn_bf16_store_launches_gpu', 'run_child', [knob], {knob: '1'})
    print(''.join(knob + '=1 ' + ln + '\n' for ln in r.stdout.splitlines() if ln.startswith(('fcn-bf16-store', 'bf16-launch'))), end='')
    assert r.returncode == 0 and r.stdout.strip().endswith('child done'), r.stdout[-3000:]
    assert r.stdout.count('forward ') == len(CHILD_CASES)
