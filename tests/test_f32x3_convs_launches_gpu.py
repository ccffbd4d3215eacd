"""Every launch of the plan ukbb_fcn_set_f32x3_convs makes, one launch at a time, against float64 on the engine's OWN stored inputs -- the graders'
common method (tests/launch_grading.py), the model, grades and cases of tests/f32x3_convs_grading.py.

One forward per case on an engine created under UKBB_DEBUG_GUARD and poisoned in front of the forward (guarded_engine: guards intact afterwards, no
poison left in any map or output); the plan that ran is the planner's (assert_plan_ran).  From what the engine stored, in numpy:

    conv1_0 .. conv4_2   the eleven three-piece launches (tilings 330-345), each recomputed alone in float64 from the map stored in front of it:
                         grade 1  every element within 1e-5 of the layer's scale (the bound of the fp32 launch graders);
                         grade 2  RMS error <= R x the RMS error of the numpy fp32 model of the same launch on the same input (R: the constant of
                                  f32x3_convs_grading.py, fixed on the CPU from the model and its planted defects, never from what the engine gives)
    conv0_0+conv0_1      the fp32 stem, within 1e-5 of its scale
    g1 .. g4, logits, prob, pred   the fp32 squeeze launches and the three-piece head, held to the bounds of tests/test_head_launches_gpu.py

A batch is copies of three rough images (batch_of_copies); slices 0-2 are graded and every other slice of every stored map and output must be
BIT-IDENTICAL to the graded copy of its image.  Weights from seeds 1234 and 7 in turn.  CASES and what they reach: tests/test_f32x3_convs.py.
The U-Net kinds refuse the switch with UKBB_EARCH on a live handle."""
import time

import numpy as np
import pytest

import f32x3_convs_grading as X
import test_head_launches_gpu as HL                                # the squeeze and head models and their bounds
from launch_grading import POISON, SEEDS, assert_plan_ran, batch_of_copies, check_copies, fit_of, guarded_engine, launches, layer, rel_err

pytestmark = pytest.mark.gpu


def run_case(index, monkeypatch):
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.weights import synthetic_params
    model, n, H, W = X.CASES[index]
    arch = MODELS[model]
    params = synthetic_params(arch, SEEDS[index % 2])
    img, nd = batch_of_copies(index, n, H, W)
    plan = X.plan(model, n, H, W)
    assert plan.get('conv_x3') is True
    op_of = {part: o for o in plan['ops'] for part in o['name'].split('+')}
    tag = 'f32x3-convs %-11s %2dx%3dx%3d' % (model, n, H, W)
    t0 = time.perf_counter()
    conv, g = {}, {}
    with guarded_engine(monkeypatch, arch, params, 'f32x3') as eng:
        eng.set_f32x3_convs(True)
        eng.reserve(n, H, W)
        eng.poison(POISON)
        out = eng.run(img, want_logits=True, want_prob=True, want_pred=True)
        names, cfgs = assert_plan_ran(eng, plan)
        assert [c for nm, c in zip(names, cfgs) if nm in X.LAYERS] == [op_of[k]['cfg'] for k in X.LAYERS] and set(cfgs) & set(X.X3_TILINGS)
        for lname, sname, l, srcs, stride, transposed, relu in launches(arch):
            if lname == 'conv0_0':
                continue
            a = eng.activation(sname).reshape(n, H >> l, W >> l, -1)
            check_copies(sname, a, nd, tag)                        # no poison (NaN) left, every copy bit-identical
            conv[sname] = a[:nd].copy()
        for l in range(1, 5):
            a = eng.activation('g%d' % l).reshape(n, H >> l, W >> l, 64)
            check_copies('g%d' % l, a, nd, tag)
            g[l] = a[:nd].copy()
        only = eng.run(img, want_logits=False, want_prob=False, want_pred=True)
        damaged, where = eng.check_guards()
        assert damaged == 0, where
    for k in ('logits', 'prob', 'pred'):
        check_copies(k, out[k], nd, tag)
    assert np.array_equal(only['pred'], out['pred'])
    t_gpu = time.perf_counter() - t0
    t0 = time.perf_counter()
    failures, rows = [], []
    x0 = img[:nd]
    for lname, sname, l, srcs, stride, transposed, relu in launches(arch):
        if lname == 'conv0_0':
            continue
        if lname == 'conv0_1':                                     # the fused fp32 stem, as a unit
            ex = layer(layer(x0, params['conv0_0']).astype(np.float32), params['conv0_1'])
            err = rel_err(conv[sname], ex)[0]
            print('%s %-16s tiling %3d  err/scale %.2e' % (tag, 'conv0_0+conv0_1', op_of[lname]['cfg'], err))
            if not err <= X.BOUND:
                failures.append((lname, err))
            continue
        x = conv[srcs[0]]
        ex = layer(x, params[lname], stride)
        err, ratio = X.grades(conv[sname], ex, X.fp32_launch(x, params[lname], stride))
        o = op_of[lname]
        rows.append((lname, o['cfg'], fit_of(o), err, ratio))
        print('%s %-16s tiling %3d %-7s err/scale %.2e (bound %.0e)  rms / rms of the fp32 model %.2f (bound %.2f)' % (tag, lname, o['cfg'], fit_of(o), err, X.BOUND, ratio, X.R))
        if not (err <= X.BOUND and ratio <= X.R):
            failures.append((lname, o['cfg'], err, ratio))
    tail = [('g%d' % l, rel_err(g[l], HL.squeeze_map(conv['conv%d' % l], params, l))[0], HL.BOUND) for l in range(1, 5)]
    ex_logits = HL.head_logits(conv['conv0'], g, params)
    tail.append(('logits', rel_err(out['logits'][:nd], ex_logits)[0], HL.BOUND))
    tail.append(('prob', float(np.abs(out['prob'].astype(np.float64) - HL.softmax64(out['logits'])).max()), HL.PROB_ATOL))
    differ = out['pred'][:nd] != np.argmax(ex_logits, axis=-1)
    margin = HL.top2_gap(ex_logits) / float(np.abs(ex_logits).max())
    tail.append(('pred', float(margin[differ].max()) if differ.any() else 0.0, HL.LABEL_MARGIN))
    for launch, fig, bound in tail:
        print('%s %-16s %.2e (bound %.0e)' % (tag, launch, fig, bound))
        if not fig <= bound:
            failures.append((launch, fig, bound))
    assert np.array_equal(out['pred'], np.argmax(out['prob'], axis=-1).astype(np.int32)), 'pred != argmax(prob)'
    clear = HL.top2_gap(out['logits']) >= np.float32(HL.NEAR_TIE_GAP)
    assert np.array_equal(out['pred'][clear], np.argmax(out['logits'], axis=-1).astype(np.int32)[clear])
    print('%s forward, read-back and identity %.2f s, float64 and the fp32 model %.2f s' % (tag, t_gpu, time.perf_counter() - t0))
    assert not failures, 'launches over their bounds: %s' % (failures,)
    return rows


@pytest.mark.parametrize('index', range(len(X.CASES)), ids=['%s-%dx%dx%d' % c for c in X.CASES])
def test_each_launch_of_the_switch_on_plan_against_float64(index, monkeypatch):
    rows = run_case(index, monkeypatch)
    assert [r[0] for r in rows] == list(X.LAYERS)
    assert {(r[0], r[1], r[2], X.batch_class(X.CASES[index][1])) for r in rows} == X.reached(*X.CASES[index])       # what the CPU file counted


@pytest.mark.parametrize('model', ['UNet_ao', 'UNet-LSTM_ao', 'Temporal-UNet_ao'])
def test_unet_kinds_refuse_the_switch_on_a_handle(model):
    from ukbb_cardiac_amd import _lib
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.engine import Engine
    from ukbb_cardiac_amd.weights import synthetic_params
    with Engine(MODELS[model], synthetic_params(MODELS[model], 1234)) as eng:
        for on in (True, False):
            with pytest.raises(_lib.UkbbFcnError) as e:
                eng.set_f32x3_convs(on)
            assert '(-2)' in str(e.value) and 'FCN models only' in str(e.value)
