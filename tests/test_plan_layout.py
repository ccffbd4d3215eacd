"""The host-only planner (csrc/plan.cpp, through engine.plan_layout) makes the plans the engine made before the planner was split
from it: tests/golden/plan_layouts.json holds what a live handle of that build reported on an MI355X (tools/record_plan_layouts.py:
op names, conv tilings, the three MAC figures, the workspace size) for every model x precision x shape x batch and for the A/B knobs,
and the forward_cine footprints ukbb_fcn_cine_scratch_bytes gave.  No GPU needed; knobs are cached per process, so every knob
setting (and the plain setting, with every knob cleared) is replayed in a child process of its own."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'plan_layouts.json')

ARCHS = ['FCN_sa', 'FCN_la_2ch', 'FCN_la_4ch', 'FCN_la_4ch_seg4', 'UNet_ao', 'UNet-LSTM_ao', 'Temporal-UNet_ao']
PRECS = ['fp32', 'bf16', 'f32x3']
SHAPES = [(192, 208), (176, 208), (208, 256), (256, 256), (80, 112), (64, 96), (32, 48), (48, 16)]
BATCHES = [1, 10, 16, 17, 64, 100]
KNOBS = ['UKBB_NO_FUSE_FIRST=1', 'UKBB_NO_FUSE_STEM=1', 'UKBB_NO_FUSE_TAIL=1', 'UKBB_NO_FUSE_LOGITS=1', 'UKBB_NO_WINOGRAD24=1',
         'UKBB_NO_WINOGRAD_FIRST=1', 'UKBB_SMALL_BATCH_TILINGS=1', 'UKBB_NO_SMALL_BATCH_SIBLINGS=1', 'UKBB_SQG1_SEPARATE=1',
         'UKBB_SIDE_STREAM=1', 'UKBB_CONV_CFG=conv4_1:301']
KNOB_MODELS = [('FCN_sa', (192, 208)), ('UNet_ao', (256, 256)), ('UNet-LSTM_ao', (256, 256))]
CINE_FRAMES = [10, 16, 17, 50, 100]
CINE_MODELS = [('UNet-LSTM_ao', 'fp32'), ('UNet-LSTM_ao', 'bf16'), ('Temporal-UNet_ao', 'fp32')]


def _expected_keys():
    keys = {(a, p, H, W, n, '') for a in ARCHS for p in PRECS for H, W in SHAPES for n in BATCHES}
    keys |= {(a, p, H, W, n, k) for k in KNOBS for a, (H, W) in KNOB_MODELS for p in PRECS for n in BATCHES}
    return keys


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_file_covers_the_whole_matrix():
    g = _golden()
    keys = [tuple(r[:6]) for r in g['records']]
    assert len(keys) == len(set(keys)) == len(_expected_keys()) == 1602
    assert set(keys) == _expected_keys()
    assert g['cine_frames'] == CINE_FRAMES
    assert {tuple(c[:4]) for c in g['cine']} == {(a, p, H, W) for a, p in CINE_MODELS for H, W in SHAPES}
    accepted = [r for r in g['records'] if r[6] == 0]
    assert len(accepted) > 1400 and all(r[6] < 0 for r in g['records'] if r[6] != 0)
    # MAC figures were recorded on every accepted plan but the batch-1 plans of the sequence models (no forward that small exists)
    assert all(r[7] > 0 or (r[4] == 1 and r[0] in ('UNet-LSTM_ao', 'Temporal-UNet_ao')) or r[5] == 'UKBB_NO_WINOGRAD24=1' for r in accepted)


def _kind_ok(arch_kind, name, kind):
    """What an op's name says about its kind (the recorded build exposes no kinds; conv / tconv are pinned by a tiling id as well)."""
    d3 = '3d' if arch_kind == 3 else ''
    if name == 'head' or name == 'logits':
        return kind == name
    if name.startswith('sqg'):
        return kind == ('sqg_multi' if '-' in name else 'sqg')
    if name == 'up0_0+up0_1+logits':
        return kind == 'tail'
    if name == 'conv0_0+conv0_1':
        return kind in ('conv', 'stem')
    if name == 'conv0_0':
        return kind == 'first' + d3
    if name.endswith('_t'):
        return kind == 'tconv' + d3
    return kind == 'conv' + d3


def replay(knob):
    """Every record of one knob setting against engine.plan_layout(cus=256); returns (records replayed, list of mismatches)."""
    from ukbb_cardiac_amd import _lib, engine
    from ukbb_cardiac_amd.arch import MODELS
    g = _golden()
    bad, n_seen = [], 0
    for r in g['records']:
        name, prec, H, W, n, k, rc, last_n = r[:8]
        if k != knob:
            continue
        n_seen += 1
        tag = '%s %s %dx%d n=%d %s' % (name, prec, H, W, n, k or '-')
        try:
            plan = engine.plan_layout(MODELS[name], prec, n, H, W, cus=256)
        except _lib.UkbbFcnError as e:
            got = int(re.search(r'failed \((-?\d+)\)', str(e)).group(1))
            if got != rc:
                bad.append('%s: rejected with %d, recorded %d (%s)' % (tag, got, rc, e))
            continue
        if rc != 0:
            bad.append('%s: accepted, recorded as rejected with %d' % (tag, rc))
            continue
        ops = plan['ops']
        names, cfgs, macs = g['names'][r[8]], g['cfgs'][r[9]], g['macs'][r[10]]
        if [o['name'] for o in ops] != names:
            bad.append('%s: ops %s, recorded %s' % (tag, [o['name'] for o in ops], names))
            continue
        if [o['cfg'] if o['kind'] in ('conv', 'tconv') else -1 for o in ops] != cfgs:
            bad.append('%s: tilings %s, recorded %s' % (tag, [o['cfg'] for o in ops], cfgs))
        for o in ops:
            if not _kind_ok(MODELS[name].kind, o['name'], o['kind']):
                bad.append('%s: op %s has kind %s' % (tag, o['name'], o['kind']))
        got = [[o['macs'] * last_n, o['mfma_macs'] * last_n, o['issued_macs'] * last_n] for o in ops]      # exact: the same double product
        if got != macs:
            bad.append('%s: MACs x %d %s, recorded %s' % (tag, last_n, got, macs))
        if 4 * n * sum(a['per_image'] for a in plan['acts']) != r[11]:
            bad.append('%s: workspace %d bytes, recorded %d' % (tag, 4 * n * sum(a['per_image'] for a in plan['acts']), r[11]))
    if not knob:
        for name, prec, H, W, want in g['cine']:
            got = [engine.cine_scratch_bytes(MODELS[name], prec, F, H, W, 1, 0) for F in g['cine_frames']]
            n_seen += 1
            if got != want:
                bad.append('cine %s %s %dx%d: %s, recorded %s' % (name, prec, H, W, got, want))
    return n_seen, bad


@pytest.mark.parametrize('knob', [''] + KNOBS)
def test_plans_equal_the_recorded_ones(knob):
    env = {k: v for k, v in os.environ.items() if not k.startswith('UKBB_') or k == 'UKBB_FCN_LIB'}
    if knob:
        k, v = knob.split('=', 1)
        env[k] = v
    want = len([k for k in _expected_keys() if k[5] == knob]) + (0 if knob else len(CINE_MODELS) * len(SHAPES))
    res = subprocess.run([sys.executable, os.path.abspath(__file__), knob], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0 and ('replayed %d records, 0 mismatches' % want) in res.stdout, res.stdout[-6000:]


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    seen, mismatches = replay(sys.argv[1])
    for m in mismatches[:40]:
        print(m)
    print('replayed %d records, %d mismatches' % (seen, len(mismatches)))
    sys.exit(1 if mismatches else 0)
