"""The level-4 Winograd stage loop (kernels_wino.hip, wino_pc_kernel<4, *>) against the one it replaced, bit for bit.

The 64-channel-per-item instances of the F(2x2) producer/consumer kernel (tilings 300 and 302) queue their weight fragments eight k positions
ahead instead of four, and their producer waves share the input transform of a half region's 16 real tiles.  Neither may change an
operand or the order of a sum: the engine promises a slice the same bits whatever batch it is in.  UKBB_WINO_STAGE_PARENT=1 launches the
stage loop as it was, so two child processes, one with the knob and one without, run the same forwards and the parent process compares
SHA-256 digests of the stored level-4 maps (conv4_1, and conv4 = conv4_2 where the model has it), of the logits and of the label map.

Cases (model, N, H, W) and the tiling the level-4 layers run on (Engine.kernel_configs(), recorded by the children and asserted below):

    FCN_sa   1 x 192 x 208   12 x 13 map, a full and a half region          301 (small-batch sibling: 32 channels per item, one form only)
    FCN_sa  17 x 192 x 208   the same map on the large-batch tiling         300
    FCN_sa  33 x 192 x 208   264 items on 256 workgroups: eight of them walk from one item into the next, as the benchmark's all do     300
    FCN_sa   2 x  32 x  48   2 x 3 map, a single partly filled region       305 (F(2x4), kernels_wino24.hip; level 2 runs 301)
    FCN_sa   1 x 208 x 256   13 x 16 map                                    305
    UNet_ao  1 x 256 x 256   16 x 16 level-4 map                            305
    FCN_sa  17 x 144 x  16   9 x 1 map, one half region of 16 x 8 pixels    302

Three of the maps asked for plan F(2x4) at level 4, which this knob does not reach; they are compared all the same, and the last case is
there because without it no case reaches 302.  The ConvLSTM gate convolutions of forward_cine run launch_wino24_lstm (kernels_wino24.hip),
not this instance, so there is no cine case.  Together the ids 300, 301 and 302 are all reached.

The two children take about 7 s together on an MI355X (profiles/r13_notes.md)."""
import hashlib
import json

import numpy as np
import pytest

from launch_grading import run_in_child

pytestmark = pytest.mark.gpu
KNOB = 'UKBB_WINO_STAGE_PARENT'

CASES = [('FCN_sa', 1, 192, 208), ('FCN_sa', 17, 192, 208), ('FCN_sa', 33, 192, 208), ('FCN_sa', 2, 32, 48), ('FCN_sa', 1, 208, 256),
         ('UNet_ao', 1, 256, 256), ('FCN_sa', 17, 144, 16)]
LEVEL4_TILING = [301, 300, 300, 305, 305, 305, 302]


def run_cases(path):
    """Per case, with the stage loop this process's environment selects: the tilings that ran and SHA-256 digests of the level-4 maps, the logits and the labels."""
    from ukbb_cardiac_amd import engine
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.weights import synthetic_params
    out = []
    for i, (model, n, H, W) in enumerate(CASES):
        arch = MODELS[model]
        img = np.random.default_rng(100 + i).standard_normal((n, H, W, 1)).astype(np.float32)
        with engine.Engine(arch, synthetic_params(arch, 1234)) as eng:
            res = eng.run(img, want_logits=True)
            cfg = dict(zip(eng.kernel_names(), eng.kernel_configs()))
            maps = {'logits': res['logits'], 'pred': res['pred']}
            last = arch.n_block[4] - 1
            for b in range(1, last + 1):
                name = 'conv4' if b == last else 'conv4_%d' % b
                maps['conv4_%d' % b] = eng.activation(name)
        out.append({'cfg': {k: v for k, v in cfg.items() if k.startswith('conv4_')},
                    'all_cfg': sorted(set(cfg.values())),
                    'sha': {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in maps.items()},
                    'nonzero': {k: int(np.count_nonzero(v)) for k, v in maps.items()}})
    with open(path, 'w') as f:
        json.dump(out, f)


def run_child(knob_value, path):
    r = run_in_child('test_wino_level4_gpu', 'run_cases', [path], {} if knob_value is None else {KNOB: knob_value}, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:]
    with open(path) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def both(tmp_path_factory):
    d = tmp_path_factory.mktemp('wino_level4')
    return run_child(None, str(d / 'new.json')), run_child('1', str(d / 'parent.json'))


def test_cases_reach_tilings_300_301_302(both):
    new, parent = both
    reached = set()
    for case, want, a, b in zip(CASES, LEVEL4_TILING, new, parent):
        assert a['cfg'] == b['cfg'] and a['all_cfg'] == b['all_cfg'], 'the knob changed the plan of %s' % (case,)
        assert 'conv4_1' in a['cfg'] and set(a['cfg'][k] for k in a['cfg'] if k != 'conv4_0') == {want}, (case, a['cfg'])
        reached |= set(a['all_cfg'])
    assert {300, 301, 302} <= reached, sorted(reached)


@pytest.mark.parametrize('index', range(len(CASES)), ids=['%s-%dx%dx%d' % c for c in CASES])
def test_level4_maps_and_pred_bit_identical_to_parent_stage_loop(both, index):
    new, parent = both
    a, b = new[index], parent[index]
    assert 'conv4_1' in a['sha'] and 'pred' in a['sha'] and 'logits' in a['sha']
    assert a['nonzero']['conv4_1'] > 0, 'conv4_1 of %s is all zero' % (CASES[index],)
    for name in sorted(a['sha']):
        assert a['sha'][name] == b['sha'][name], '%s of %s differs between the stage loops (tiling %s)' % (name, CASES[index], a['cfg'])
