"""Two workers of shard.launch on one device, running deploy_network.main on the real engine: a run that saves no label file
(--save_seg=false --output_csv) segments every subject exactly once, and its merged table is the one-worker table byte for byte.
Each launch is a child process under a time limit; its workers are fresh children of the launcher and the only processes of the
test that open the GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['subj%02d' % i for i in range(6)]

# argv: directory for the per-worker logs, then the command line of deploy_network.py
WORKER = '''
import os, sys
sys.path.insert(0, {root!r})
from ukbb_cardiac_amd import deploy_network
from ukbb_cardiac_amd.sequence_run import SequenceRun
mine = os.path.join(sys.argv[1], 'segmented%s' % os.environ.get('UKBB_SHARD_INDEX', '0'))
open(mine, 'a').close()
finish = SequenceRun.finish
def logged(self, item, *args, **kwargs):                       # every loop hands every subject it has segmented to finish(), once
    with open(mine, 'a') as f:
        f.write(item[0] + '\\n')
    return finish(self, item, *args, **kwargs)
SequenceRun.finish = logged
deploy_network.main(sys.argv[2:])
'''


def test_two_workers_on_one_device_without_label_files_segment_every_subject_once(tmp_path):
    from ukbb_cardiac_amd import nifti
    from ukbb_cardiac_amd.arch import MODELS
    from ukbb_cardiac_amd.weights import save_blob, synthetic_params
    arch = MODELS['FCN_sa']                                                     # the model of tests/test_deploy_gpu.py
    model = str(tmp_path / 'FCN_sa')
    save_blob(model + '.ukbbw', arch, synthetic_params(arch, 1234))
    data = tmp_path / 'data'
    affine = np.diag([1.8, 1.8, 10.0, 1.0])
    pixdim = np.array([1, 1.8, 1.8, 10.0, 0.03, 0, 0, 0], np.float32)
    for i, name in enumerate(NAMES):
        (data / name).mkdir(parents=True)
        vol = (1000.0 * np.random.default_rng(80 + i).gamma(2.0, 1.0, size=(20, 28, 2, 3))).astype(np.float32)
        nifti.save(vol, str(data / name / 'sa.nii.gz'), affine, pixdim)
    script = tmp_path / 'worker.py'
    script.write_text(WORKER.format(root=ROOT))

    def run(tag, launcher):
        where = tmp_path / tag
        where.mkdir()
        flags = ['--seq_name', 'sa', '--data_dir', str(data), '--model_path', model, '--save_seg=false', '--output_csv', str(where / 'sa.csv')]
        env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
        r = subprocess.run(['timeout', '-k', '10', '120', sys.executable] + launcher + [str(script), str(where)] + flags, env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-3000:]
        return where, r.stdout

    two, out = run('two', ['-m', 'ukbb_cardiac_amd.shard', '--gpus', '1', '--shards_per_gpu', '2', '--'])
    by_worker = [open(str(two / ('segmented%d' % r))).read().split() for r in range(2)]
    assert sorted(by_worker[0] + by_worker[1]) == NAMES, by_worker              # complete, and nobody's work done twice
    assert by_worker[0] and by_worker[1]
    assert out.count('Segmenting full sequence') == len(NAMES)
    one, _ = run('one', [])
    assert open(str(one / 'segmented0')).read().split() == NAMES
    table = open(str(two / 'sa.csv'), 'rb').read()
    assert table == open(str(one / 'sa.csv'), 'rb').read()
    assert [line.split(b',')[0] for line in table.splitlines()[1:]] == [n.encode() for n in NAMES]
    for name in NAMES:                                                          # no label file, no claim, no writer's temporary file
        assert os.listdir(str(data / name)) == ['sa.nii.gz']
    assert sorted(os.listdir(str(two))) == ['sa.csv', 'segmented0', 'segmented1']
