"""Record the launch plans a build of the engine makes, as tests/golden/plan_layouts.json (tests/test_plan_layout.py replays them on the
host-only planner).  Needs an MI355X.  Run it against the build whose plans are the reference (UKBB_FCN_LIB selects the library):

    UKBB_FCN_LIB=/path/to/parent/libukbb_fcn.so python tools/record_plan_layouts.py [--out tests/golden/plan_layouts.json]

It uses only what every build since ABI 11 exports: reserve, one forward per handle (the MAC accessors scale with the batch of the last
forward, `last_n`, which later re-plans keep), kernel_names / kernel_configs / kernel_macs / kernel_mfma_macs / kernel_mfma_macs_issued
and ukbb_fcn_scratch_bytes.  MAC figures are stored as the accessors return them (per image x last_n), so the replay multiplies instead
of dividing and equality stays exact.  A batch below the smallest forward a model accepts (n = 1 of the sequence models) is planned
on a handle that never ran: its last_n and MAC figures are 0.

Several A/B knobs are read once per process, so every knob gets a fresh child process."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARCHS = ['FCN_sa', 'FCN_la_2ch', 'FCN_la_4ch', 'FCN_la_4ch_seg4', 'UNet_ao', 'UNet-LSTM_ao', 'Temporal-UNet_ao']
PRECS = ['fp32', 'bf16', 'f32x3']
SHAPES = [(192, 208), (176, 208), (208, 256), (256, 256), (80, 112), (64, 96), (32, 48), (48, 16)]
BATCHES = [1, 10, 16, 17, 64, 100]
KNOBS = ['UKBB_NO_FUSE_FIRST=1', 'UKBB_NO_FUSE_STEM=1', 'UKBB_NO_FUSE_TAIL=1', 'UKBB_NO_FUSE_LOGITS=1', 'UKBB_NO_WINOGRAD24=1',
         'UKBB_NO_WINOGRAD_FIRST=1', 'UKBB_SMALL_BATCH_TILINGS=1', 'UKBB_NO_SMALL_BATCH_SIBLINGS=1', 'UKBB_SQG1_SEPARATE=1',
         'UKBB_SIDE_STREAM=1', 'UKBB_CONV_CFG=conv4_1:301']
KNOB_MODELS = [('FCN_sa', (192, 208)), ('UNet_ao', (256, 256)), ('UNet-LSTM_ao', (256, 256))]
CINE_FRAMES = [10, 16, 17, 50, 100]
PREC_CODE = {'fp32': 0, 'bf16': 1, 'f32x3': 2}


def matrix(knob):
    """[(arch name, [shapes])] a child records."""
    return [(a, SHAPES) for a in ARCHS] if not knob else [(a, [s]) for a, s in KNOB_MODELS]


def n_records():
    return len(ARCHS) * len(PRECS) * len(SHAPES) * len(BATCHES) + len(KNOBS) * len(KNOB_MODELS) * len(PRECS) * len(BATCHES)


def _first_forward(eng, arch):
    """One small forward; returns the batch run_plan saw (0: every form failed, e.g. a knob that leaves the fp32 ConvLSTM without its kernel)."""
    import torch
    from ukbb_cardiac_amd import _lib
    from ukbb_cardiac_amd.arch import KIND_TEMPORAL_UNET, KIND_UNET_LSTM
    dev = torch.device('cuda', 0)
    h = w = 64
    try:
        if arch.kind == KIND_UNET_LSTM:
            n = 4
            x = torch.zeros((n, h, w), dtype=torch.float32, device=dev)
            pr = torch.empty((n, h, w, arch.n_class), dtype=torch.float32, device=dev)
            eng.run_cine_device(x.data_ptr(), n, h, w, pr.data_ptr(), 0)
        elif arch.kind == KIND_TEMPORAL_UNET:
            n = arch.fc
            x = torch.zeros((n, h, w), dtype=torch.float32, device=dev)
            pr = torch.empty((n, h, w, arch.n_class), dtype=torch.float32, device=dev)
            _lib.check(_lib.lib.ukbb_fcn_forward_seq(eng._h, C.c_void_p(x.data_ptr()), 1, h, w, None, C.c_void_p(pr.data_ptr()), None, None),
                       'ukbb_fcn_forward_seq')
        else:
            n = 1
            x = torch.zeros((n, h, w), dtype=torch.float32, device=dev)
            lg = torch.empty((n, h, w, arch.n_class), dtype=torch.float32, device=dev)
            pr = torch.empty((n, h, w, arch.n_class), dtype=torch.float32, device=dev)
            pd = torch.empty((n, h, w), dtype=torch.int32, device=dev)
            eng.run_device(x.data_ptr(), n, h, w, logits_ptr=lg.data_ptr(), prob_ptr=pr.data_ptr(), pred_ptr=pd.data_ptr())
        torch.cuda.synchronize()
    except _lib.UkbbFcnError:
        return 0
    if arch.kind in (KIND_UNET_LSTM, KIND_TEMPORAL_UNET):      # drop the cine buffers: scratch_bytes then counts the plan's workspace alone
        eng.set_scratch_budget(1 << 40)
        eng.set_scratch_budget(0)
    return n


def child(knob, out):
    from ukbb_cardiac_amd import _lib
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.engine import Engine, cine_scratch_bytes
    from ukbb_cardiac_amd.weights import synthetic_params
    tables = {'names': [], 'cfgs': [], 'macs': []}
    index = {k: {} for k in tables}

    def intern(kind, value):
        key = json.dumps(value)
        if key not in index[kind]:
            index[kind][key] = len(tables[kind])
            tables[kind].append(value)
        return index[kind][key]

    records, cine = [], []
    for name, shapes in matrix(knob):
        arch = MODELS[name]
        params = synthetic_params(arch, 1234)
        for prec in PRECS:
            warm = Engine(arch, params, device=0)
            rc = _lib.lib.ukbb_fcn_set_precision(warm._h, PREC_CODE[prec])
            if rc < 0:
                records += [[name, prec, H, W, n, knob, rc, 0, -1, -1, -1, 0] for n in BATCHES for H, W in shapes]
                warm.close()
                continue
            last_n = _first_forward(warm, arch)
            if not last_n:                                     # the failed attempt already raised the handle's largest batch: start over
                warm.close()
                warm = Engine(arch, params, device=0)
                _lib.check(_lib.lib.ukbb_fcn_set_precision(warm._h, PREC_CODE[prec]), 'ukbb_fcn_set_precision')
            cold = None
            for n in BATCHES:                                  # ascending: a handle plans for the largest batch it has seen
                eng, ln = warm, last_n
                if n < last_n:                                 # a handle that never ran (its largest batch so far: none)
                    if cold is None:
                        cold = Engine(arch, params, device=0)
                        _lib.check(_lib.lib.ukbb_fcn_set_precision(cold._h, PREC_CODE[prec]), 'ukbb_fcn_set_precision')
                    eng, ln = cold, 0
                for H, W in shapes + ([(64, 64)] if len(shapes) == 1 else []):      # a shape change forces the re-plan
                    rc = _lib.lib.ukbb_fcn_reserve(eng._h, n, H, W)
                    if (H, W) not in shapes:
                        continue
                    if rc < 0:
                        records.append([name, prec, H, W, n, knob, rc, 0, -1, -1, -1, 0])
                        continue
                    macs = [list(t) for t in zip(eng.kernel_macs(), eng.kernel_mfma_macs(), eng.kernel_mfma_macs_issued())]
                    records.append([name, prec, H, W, n, knob, 0, ln, intern('names', eng.kernel_names()), intern('cfgs', eng.kernel_configs()),
                                    intern('macs', macs), eng.scratch_bytes()])
            warm.close()
            if cold is not None:
                cold.close()
            if not knob and arch.kind in (2, 3) and prec != 'f32x3':
                cine += [[name, prec, H, W, [cine_scratch_bytes(arch, prec, F, H, W, 1, 0) for F in CINE_FRAMES]] for H, W in shapes]
            print('recorded %s %s %s: %d records so far' % (name, prec, knob or '-', len(records)), flush=True)
    with open(out, 'w') as f:
        json.dump({'records': records, 'cine': cine, **tables}, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'plan_layouts.json'))
    ap.add_argument('--child', default=None, help='internal: record one knob setting ("" = none) into --out')
    args = ap.parse_args()
    if args.child is not None:
        child(args.child, args.out)
        return 0
    merged = {'cine_frames': CINE_FRAMES, 'records': [], 'cine': [], 'names': [], 'cfgs': [], 'macs': []}
    for knob in [''] + KNOBS:
        env = dict(os.environ)
        if knob:
            k, v = knob.split('=', 1)
            env[k] = v
        part = args.out + '.part'
        subprocess.run([sys.executable, os.path.abspath(__file__), '--child', knob, '--out', part], env=env, check=True,
                       timeout=600 if not knob else 240)       # a child that fails or hangs ends the recording: nothing more is started
        with open(part) as f:
            got = json.load(f)
        os.remove(part)
        base = {k: len(merged[k]) for k in ('names', 'cfgs', 'macs')}
        for k in base:
            merged[k] += got[k]
        for r in got['records']:
            if r[6] == 0:
                r[8] += base['names']; r[9] += base['cfgs']; r[10] += base['macs']
            merged['records'].append(r)
        merged['cine'] += got['cine']
    # the children interned their tables separately: once more over the union
    final = {'cine_frames': CINE_FRAMES, 'records': [], 'cine': merged['cine'], 'names': [], 'cfgs': [], 'macs': []}
    seen = {k: {} for k in ('names', 'cfgs', 'macs')}
    for r in merged['records']:
        if r[6] == 0:
            for pos, k in ((8, 'names'), (9, 'cfgs'), (10, 'macs')):
                key = json.dumps(merged[k][r[pos]])
                if key not in seen[k]:
                    seen[k][key] = len(final[k])
                    final[k].append(merged[k][r[pos]])
                r[pos] = seen[k][key]
        final['records'].append(r)
    assert len(final['records']) == n_records(), (len(final['records']), n_records())
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(final, f, separators=(',', ':'))
    print('wrote %s: %d records, %d bytes' % (args.out, len(final['records']), os.path.getsize(args.out)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
