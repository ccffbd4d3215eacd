"""What tests/test_temporal_bf16_launches_gpu.py covers, checked without a GPU (engine.plan_layout under precision 'bf16_3d': the host-only planner),
following tests/test_temporal_launch_coverage.py.

Every 3x3x3 unit of the Temporal-UNet but the first runs on conv3d_bf16_kernel<CB> (kernels_conv3d_bf16.hip) under this precision.  The kernel keeps
conv3d_kernel's decomposition -- one wave = one ITEM = 32 pixels of one frame x 32 CB output channels, item -> (channel group, pixel tile, frame),
four items per workgroup, blockIdx.y = sub-pixel phase of a transposed conv -- so a launch's SITUATION is computed from the plan op's map by the same
mirror, launch_grading.conv3d_launch; the lines it mirrors are read from the NEW source here and asserted.  The kernel has no item or round classes
beyond that: no grid-stride loop, no workgroup-level staging, one item per wave.

    kind      stride-1, stride-2 (onto maps of a partial tile too: 12 x 12 -> 6 x 6, 6 x 6 -> 3 x 3), two-source (skip concat; 96 + 96 channels on the 'wide'
              architecture) or transposed (all 4 sub-pixel phases over the INPUT map: gridDim.y = 4 in every transposed launch)
    CB        2 where the padded channel count is a multiple of 64, else 1; the number of channel groups (C_out 16 -> padded MFMA rows, 32, 96 -> 3
              groups, 160 -> 5 groups)
    padded    C_out < C_out padded (16 channels on the 32-row MFMA: level 0) or not
    fit       the map's pixels in 32-pixel tiles: divides / whole tiles and a partial one / one partial tile (a map smaller than a tile) / a single pixel
    idle      items % 4: the waves of the last workgroup that return at once
    T         windows of 1 frame (only the middle time tap runs), of 3, of 5 or more (9)
    windows   one, or several (a window edge inside the batch)

SITUATIONS counted per launch are those of the fp32 coverage file: for its (kind, CB): (fit, T), (idle, windows), (T, windows), the number of channel
groups, and per kind whether the channels are padded; for the first layer (T, windows) -- conv3d_first_bf16_kernel starts one thread per pixel, whole
workgroups always (H and W are multiples of 16), no cap; for the logits launch the class count.  SEARCHED: the four architectures x 1, 2, 4, 5
windows x the maps 16 x 16, 16 x 48, 48 x 16, 32 x 48, 48 x 48 and 48 x 80.  CASES reaches every situation any searched case holds, and dropping any
one case leaves some situation unreached."""
import os

import pytest

import launch_grading as G
import temporal_bf16_grading as B

WINDOWS = (1, 2, 4, 5)
MAPS = ((16, 16), (16, 48), (48, 16), (32, 48), (48, 48), (48, 80))


def plan(key, N, H, W):
    from ukbb_cardiac_amd import engine
    arch = B.arch_of(key)
    return arch, engine.plan_layout(arch, B.PRECISION, N * arch.fc, H, W, G.CUS)


def reached(case):
    key, N, H, W = case
    arch, p = plan(key, N, H, W)
    T = arch.fc
    out = set()
    for o in p['ops']:
        if o['kind'] in ('conv3d', 'tconv3d'):
            d = G.conv3d_launch(o, p['acts'], N * T, T)
            k = (d['kind'], d['cb'])
            out |= {('fit',) + k + (d['fit'], d['T']), ('idle',) + k + (d['idle'], d['windows']), ('T',) + k + (d['T'], d['windows']),
                    ('groups',) + k + (d['cgroups'],), ('padded', d['kind'], d['padded'])}
        elif o['kind'] == 'first3d':
            assert (N * T * H * W) % 256 == 0                            # whole workgroups: the kernel's `id >= total` guard never splits one
            d = G.conv3d_launch(dict(o, kind='conv3d'), p['acts'], N * T, T)
            out.add(('first', d['T'], d['windows']))
        else:
            assert o['kind'] == 'logits', o
            out.add(('logits', arch.n_class))
    return out


@pytest.fixture(scope='module')
def searched():
    return {c: reached(c) for c in [(key, N, H, W) for key in B.ARCH_CHANGES for N in WINDOWS for H, W in MAPS]}


def test_launcher_lines_are_the_ones_mirrored():
    launcher, kern, first_launcher, first_kern = B.launcher_lines()
    assert 'const int cb = a.Cout_pad %% %d == 0 ? 2 : 1;' % (2 * G.C3D_COB) in launcher
    assert 'const long long items = (long long)a.N * ((a.Hg * a.Wg + %d) / %d) * (a.Cout_pad / %d / cb);' % (G.C3D_PIX - 1, G.C3D_PIX, G.C3D_COB) in launcher
    assert 'const long long blocks = (items + %d) / %d;' % (G.C3D_WAVES - 1, G.C3D_WAVES) in launcher and 'dim3 g((unsigned)blocks, (unsigned)a.nph), t(256)' in launcher
    assert 'ptiles = (npix + 31) / 32, ncob = a.Cout_pad / 32, cgroups = ncob / CB;' in kern
    assert 'const long long item = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);' in kern
    assert 'if (item >= (long long)a.N * ptiles * cgroups) return;' in kern
    assert 'if (co >= a.Cout) continue;' in kern                          # padded MFMA rows store nothing
    # the first layer: one thread per pixel, no cap and no loop
    assert 'const long long blocks = (total + 255) / 256;' in first_launcher and 'blocks = 256' not in first_launcher
    assert 'const long long id = (long long)blockIdx.x * 256 + threadIdx.x;' in first_kern and 'if (id >= total) return;' in first_kern
    assert 'gridDim' not in first_kern and 'gridDim' not in kern
    # the engine hands both launchers the same arguments: the output map of a conv, the INPUT map of a transposed conv
    with open(os.path.join(G.ROOT, 'ukbb_cardiac_amd', 'csrc', 'engine.cpp')) as f:
        eng = f.read()
    assert 'e = bfio ? launch_conv3d_bf16(ca, s) : launch_conv3d(ca, s);' in eng
    assert 'e = bfio ? launch_conv3d_first_bf16(fa, s) : launch_conv3d_first(fa, s);' in eng
    assert 'ca.Hg = op.Ho; ca.Wg = op.Wo; ca.stride = op.stride;' in eng and 'ca.Hg = op.H; ca.Wg = op.W; ca.stride = 1; ca.up = 2;' in eng
    assert 'ca.Cout = L.cout; ca.Cout_pad = round_up(L.cout, 32);' in eng and 'ca.nph = 4;' in eng


def test_the_architectures_span_the_channel_counts_windows_and_class_counts():
    archs = {k: B.arch_of(k) for k in B.ARCH_CHANGES}
    assert {a.fc for a in archs.values()} == {1, 3, 9} and {a.n_class for a in archs.values()} == {2, 3, 4}
    assert {c[0] for c in B.CASES} == set(archs)
    _, p = plan('wide', 1, 16, 48)
    by = {o['name']: G.conv3d_launch(o, p['acts'], 9, 9) for o in p['ops'] if o['kind'] in ('conv3d', 'tconv3d')}
    couts = {p['acts'][o['out']]['channels'] for o in p['ops'] if o['kind'] in ('conv3d', 'tconv3d')}
    assert couts == {16, 32, 96, 160}
    assert {(d['cb'], d['cgroups']) for d in by.values()} >= {(1, 1), (1, 3), (1, 5)}
    assert by['up2_0']['kind'] == 'two-source' and (by['up2_0']['cb'], by['up2_0']['cgroups']) == (1, 3)        # 96 + 96 channels in
    assert by['conv0_1']['padded'] and by['up0_t']['padded'] and not by['conv1_0']['padded']
    assert {o['name'] for o in p['ops'] if o['kind'] == 'tconv3d'} == {'up3_t', 'up2_t', 'up1_t', 'up0_t'}


def test_launches_names_the_plans_launches_and_stored_maps():
    for key in B.ARCH_CHANGES:
        arch, p = plan(key, 2, 32, 48)
        graph = G.launches(arch)
        assert [g[0] for g in graph] == [o['name'] for o in p['ops']]
        stored = {a['name']: a for a in p['acts']}
        for lname, sname, l, srcs, stride, transposed, relu in graph[:-1]:
            o = [o for o in p['ops'] if o['name'] == lname][0]
            assert stored[sname]['per_image'] == (32 >> l) * (48 >> l) * arch.n_filter[l] and p['acts'][o['out']]['name'] == sname
            assert stored[sname]['bytes_per_element'] == 2
            assert [p['acts'][i]['name'] for i in (o['in0'], o['in1']) if i >= 0] == [s for s in srcs if s]
            assert (o['kind'] == 'tconv3d') == transposed and (o['stride'] == 2) == (stride == 2 and not transposed)


def test_cases_reach_every_searched_situation_and_none_is_idle(searched):
    assert len(set(B.CASES)) == len(B.CASES) and set(B.CASES) <= set(searched)
    want = set().union(*searched.values())
    only = G.no_case_is_idle(B.CASES, searched.__getitem__, want)
    for c, mine in zip(B.CASES, only):
        print('temporal-bf16-coverage %-7s %d x %2d x %2d alone reaches %d of %d situations, e.g. %s' % (c + (len(mine), len(want), mine[0])))
    assert {(H, W) for _, _, H, W in B.CASES} >= {(16, 16), (16, 48), (32, 48), (48, 48)}
    assert {N for _, N, _, _ in B.CASES} >= {1, 2, 5}
    assert {k[3] for k in want if k[0] == 'fit'} == {'divides', 'whole tiles and a partial one', 'one partial tile', 'single pixel'}
    assert {k[3] for k in want if k[0] == 'idle'} == {0, 1, 2, 3} and {k[3] for k in want if k[0] == 'groups' and k[2] == 1} == {1, 3, 5}
    assert {k[1] for k in want if k[0] == 'kind' or k[0] == 'fit'} == {'stride-1', 'stride-2', 'two-source', 'transposed'}
    # stride 2 onto maps that are no whole number of tiles (12 x 12 -> 6 x 6, 6 x 6 -> 3 x 3, 2 x 2 -> 1 x 1) as well as onto ones that are
    assert {k[3] for k in want if k[0] == 'fit' and k[1] == 'stride-2'} == {'divides', 'whole tiles and a partial one', 'one partial tile', 'single pixel'}
    assert {k[3] for k in want if k[0] == 'T'} == {'T=1', 'T=3', 'T>=5'} and {k[4] for k in want if k[0] == 'T'} == {'one window', 'several windows'}
    assert {k[1] for k in want if k[0] == 'logits'} == {2, 3, 4} and {k[1] for k in want if k[0] == 'first'} == {'T=1', 'T=3', 'T>=5'}
    assert all(H <= 48 and W <= 48 and B.arch_of(k).fc <= 9 for k, _, H, W in B.CASES)            # nothing larger than 48 x 48 is graded per launch
