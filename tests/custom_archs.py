"""The 2-D architectures ukbb_fcn_create accepts beyond the named entries of arch.MODELS, as tests/test_custom_arch_launches_gpu.py grades them and
tests/test_custom_arch_launch_coverage.py counts them: one closed list (ARCHS), each built with dataclasses.replace on its MODELS entry -- the descriptors
tf_checkpoint.infer_arch makes from a user's checkpoint (FCN_custom, UNet_custom, UNet-LSTM_custom).  A plain helper module, as tests/launch_grading.py.

A launch's SITUATION (situations): kind of model, precision, op kind, tiling (-1 for what is no conv / transposed conv), the channels of the op's in0, in1
and out maps (0 where the op names none: the image, the squeeze maps, an output buffer), stride, how the tiling's tile fits the output map ('div' /
'nodiv' for a tile-per-workgroup conv tiling, as tests/test_fp32_launch_coverage.py counts it; '-' elsewhere), and the class count of a launch that
computes logits (head, logits, tail, a conv with the logits in its epilogue; 0 elsewhere): their kernels are instantiated per class count."""
import dataclasses

import launch_grading as G

# name -> (MODELS entry, fields replaced)
ARCHS = {
    'FCN-c5': ('FCN_sa', dict(n_class=5)),
    'FCN-nb1': ('FCN_sa', dict(n_block=(1, 1, 1, 1, 1))),
    'FCN-nb3': ('FCN_sa', dict(n_block=(3, 2, 4, 1, 2))),
    'FCN-flat': ('FCN_sa', dict(n_filter=(16, 32, 32, 64, 64))),
    'FCN-wide': ('FCN_sa', dict(n_filter=(16, 32, 96, 160, 96), n_block=(2, 2, 3, 2, 2))),
    'FCN-big': ('FCN_sa', dict(n_filter=(16, 64, 128, 256, 512))),
    'UNet-c2': ('UNet_ao', dict(n_class=2)),
    'UNet-c4': ('UNet_ao', dict(n_class=4)),
    'UNet-nb1': ('UNet_ao', dict(n_block=(1, 1, 1, 1, 1))),
    'UNet-nb3': ('UNet_ao', dict(n_block=(3, 1, 2, 3, 1))),
    'UNet-wide': ('UNet_ao', dict(n_filter=(16, 32, 96, 160, 96), n_block=(2, 2, 3, 2, 2))),
    'UNet-flat': ('UNet_ao', dict(n_filter=(16, 32, 32, 64, 64))),
    'LSTM-wide': ('UNet-LSTM_ao', dict(n_filter=(16, 32, 96, 160, 96), n_block=(2, 2, 3, 2, 2))),
    'LSTM-nb': ('UNet-LSTM_ao', dict(n_block=(1, 2, 1, 2, 3))),
}
# refused by plan.cpp supported(): launch_sqg (kernels_head.hip) has no instance for these widths, and sqg_body's load loop covers no other
REFUSED = {'FCN-wide': 'FCN squeeze kernels are built for n_filter[l>0] in {32, 64, 128, 256}',
           'FCN-big': 'FCN squeeze kernels are built for n_filter[l>0] in {32, 64, 128, 256}'}
KIND_NAMES = ('FCN', 'UNet', 'UNet-LSTM')
PRECISIONS = {'FCN': ('fp32', 'bf16', 'bf16_store', 'bf16_full', 'f32x3c'), 'UNet': ('fp32', 'bf16'), 'UNet-LSTM': ('fp32', 'bf16')}
NAMED = {'FCN': ('FCN_sa', 'FCN_la_2ch', 'FCN_la_4ch', 'FCN_la_4ch_seg4'), 'UNet': ('UNet_ao',), 'UNet-LSTM': ('UNet-LSTM_ao',)}


def arch_of(name):
    """The descriptor of an ARCHS entry, or the MODELS entry of that name."""
    from ukbb_cardiac_amd.arch import MODELS
    if name in MODELS:
        return MODELS[name]
    base, changes = ARCHS[name]
    return dataclasses.replace(MODELS[base], name=name, **changes)


def kind_of(name):
    return KIND_NAMES[arch_of(name).kind]


def plan(name, precision, n, H, W):
    """plan_layout on 256 compute units; precision 'f32x3c' is 'f32x3' on a handle with set_f32x3_convs(True).  n counts images (frames, for a UNet-LSTM)."""
    from ukbb_cardiac_amd import engine
    if precision == 'f32x3c':
        return engine.plan_layout(arch_of(name), 'f32x3', n, H, W, G.CUS, f32x3_convs=True)
    return engine.plan_layout(arch_of(name), precision, n, H, W, G.CUS)


def situation_of(kind, precision, o, acts, n_class):
    def ch(i):
        return acts[i]['channels'] if i >= 0 else 0
    conv = o['kind'] in ('conv', 'tconv')
    cfg = o['cfg'] if conv else -1
    fit = '-'
    if o['kind'] == 'conv' and 0 <= cfg < 400:
        fit = 'div' if G.fit_of(o) == 'div' else 'nodiv'
    classes = n_class if o['kind'] in ('head', 'logits', 'tail') or o['name'].endswith('+logits') else 0
    return (kind, precision, o['kind'], cfg, ch(o['in0']), ch(o['in1']), ch(o['out']), o['stride'], fit, classes)


def situations(name, precision, n, H, W):
    """{situation: [op names]} of one plan."""
    p = plan(name, precision, n, H, W)
    out = {}
    for o in p['ops']:
        out.setdefault(situation_of(kind_of(name), precision, o, p['acts'], arch_of(name).n_class), []).append(o['name'])
    return out
