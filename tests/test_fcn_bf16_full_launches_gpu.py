"""Every launch of the FCN plans under --precision bf16_full (UKBB_PREC_BF16_FULL, include/ukbb_fcn.h), one forward per case on a guarded, NaN-poisoned
engine, against float64 on the engine's OWN stored inputs.  The shared parts and the method are in tests/fcn_bf16_full_grading.py.

    conv0_0+conv0_1 .. conv4_2, g1 .. g4   bf16_store's launches, held to exactly its grades (the stem as a unit, every further encoder element within
                      half a bf16 ulp of the specified arithmetic, the squeeze maps within 1e-5 of their scale)
    logits            the head as a unit against the float64 interval model of the specification (bf16 weights, S and P rounded once), evaluated on the
                      stored conv0 and g1..g4:  |logits - model| <= 1e-5 scale + slack  at every pixel, slack zero wherever no S / P element of the pixel
                      lies next to a bf16 rounding midpoint; at least 40 % of the graded pixels must carry zero slack
    prob              within 1e-6 of a float64 softmax of the engine's own logits;  pred == argmax(prob) exactly, over all slices

The plan that ran (kernel_names() / kernel_configs()) must be the planner's, with the head flag set; slices 0..2 are graded and every further slice of
every stored map, of g1..g4, logits, prob and pred must be bit-identical to the graded copy of its image; every encoder map holds bf16 values only, no
map holds the poison, no guard is damaged.  CASES: the launcher situations of tests/test_head_launches_gpu.py (tests/test_fcn_bf16_full.py shows that
none is idle and that the grade tells planted defects), weights from seeds 1234 and 7 in turn.  UKBB_HEAD_DIRECT_GATHER and UKBB_HEAD_INLINE_TAIL do
not apply to this mode, so there are no child processes.

Measured on an MI355X (profiles/fcn_bf16_full.txt), worst over the 11 cases: 57-80 % of a case's graded pixels carry zero slack; |logits - model| on them
<= 2.1e-7 of the logits' scale; no pixel outside 1e-5 scale + slack (worst (err - slack) / scale 2.1e-7); g1..g4 <= 4.2e-7 of their scale; prob <= 1.9e-7;
every encoder element inside bf16_store's grades.  The 11 cases take 8 s together."""
import time

import numpy as np
import pytest

import fcn_bf16_full_grading as F
from launch_grading import CUS, POISON, Report, assert_plan_ran, check_copies, fetcher, guarded_engine, launches

pytestmark = pytest.mark.gpu


def run_case(index, monkeypatch):
    """One guarded, poisoned forward of case `index`, every launch graded.  Returns (encoder rows, squeeze rows, head figures)."""
    from ukbb_cardiac_amd import _lib, engine
    model, n, H, W = F.CASES[index]
    arch, params, img, nd = F.case_inputs(index)
    plan = engine.plan_layout(arch, F.PREC, n, H, W, CUS)
    ops = plan['ops']
    tag = F.CASE_IDS[index]
    t0 = time.perf_counter()
    conv, g = {}, {}
    with guarded_engine(monkeypatch, arch, params, F.PREC) as eng:
        eng.reserve(n, H, W)
        eng.poison(POISON)
        out = eng.run(img, want_logits=True, want_prob=True, want_pred=True)
        t_fwd = time.perf_counter() - t0
        assert_plan_ran(eng, plan)
        assert [o['name'] for o in ops if o['kind'] in ('sqg', 'sqg_multi', 'head')] == list(F.TAIL_OPS) and plan['bfio'] and plan['head_bf16']
        assert int(_lib.lib.ukbb_fcn_head_tail_form()) == 1                                  # the mode's one form finishes a block inside its stage
        level = {gr[1]: gr[2] for gr in launches(arch)}
        fetch = fetcher(eng, lambda s: (n, H >> level[s], W >> level[s], -1), nd, conv, tag)    # bf16 values, no poison, copies identical
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
        check_copies(k, out[k], nd, tag)                                                    # bit-identical copies, no poison left
    t_gpu = time.perf_counter() - t0
    t0 = time.perf_counter()
    report = Report(tag, ops, plan['acts'], n)
    try:
        sq_rows = F.grade_encoder_and_squeeze(arch, params, img[:nd], conv, g, report)
        head = F.grade_outputs(tag, out, nd, F.head_model(conv['conv0'], g, params))
    finally:
        print('fcn-bf16-full %-30s forward %.2f s, + read-back and identity %.2f s, float64 %.2f s' % (tag, t_fwd, t_gpu, time.perf_counter() - t0))
    return report.rows, sq_rows, head


@pytest.mark.parametrize('index', range(len(F.CASES)), ids=F.CASE_IDS)
def test_each_bf16_full_launch_against_its_specified_arithmetic(index, monkeypatch):
    enc, sq, head = run_case(index, monkeypatch)
    assert len(enc) == 12 and len(sq) == 4 and len(head) == 4                                # the stem, conv1_0 .. conv4_2; g1 .. g4; the head's figures and prob
