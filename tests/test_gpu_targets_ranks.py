"""`topaz extract --gpus 2 --targets`: two rank processes of the real command sharing GPU 0 (TOPAZ_AMD_SHARE_GPU=1, collectives
over gloo on host tensors, like tests/test_gpu_parallel.py) against the one-process run of the same command -- same device,
same kernels, so the radius lines are equal as strings and the pick file byte for byte -- and against the stdout of the
reference's own CLI on the same micrographs and labels (tests/golden/cli, the bar of tests/test_gpu_cli.py)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
CLI = os.path.join(GOLDEN, 'cli')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _topaz(argv, cwd, ranks_share_gpu=False):
    env = dict(os.environ)
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    if ranks_share_gpu:
        env.update(TOPAZ_AMD_SHARE_GPU='1', TOPAZ_AMD_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0')
    return subprocess.run([sys.executable, '-m', 'topaz_amd'] + argv, env=env, capture_output=True, text=True, timeout=300,
                          cwd=cwd)


def _inputs(tmp_path):
    """the two labelled micrographs (the table names mic_b first) and one 384 x 384 micrograph of blobs the table does not
    name: three inputs over two ranks, rank 0 holds mic_a and the unlabelled one, rank 1 mic_b"""
    from topaz_amd.utils.image import save_image
    for n in ('mic_a.mrc', 'mic_b.mrc', 'targets.txt'):
        shutil.copy(os.path.join(CLI, n), tmp_path / n)
    rs = np.random.RandomState(500)
    x = rs.randn(384, 384).astype(np.float32)
    yy, xx = np.mgrid[0:384, 0:384].astype(np.float32)
    for cy, cx in rs.randint(20, 364, size=(10, 2)):
        x -= 2.5 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * 6.0 ** 2)).astype(np.float32)
    save_image(x, str(tmp_path / 'mic_00.mrc'))
    return ['mic_a.mrc', 'mic_b.mrc', 'mic_00.mrc']


def _radius_text(stdout):
    return [line for line in stdout.split('\n') if line.startswith('# radius=')]


def _own_stdout(stdout):
    """stdout without the connection banner the gloo library prints for each rank"""
    return [line for line in stdout.split('\n') if not line.startswith('[Gloo]')]


def _radius_rows(lines):
    return [{k: float(v) for k, v in (kv.split('=') for kv in line[2:].split(', '))} for line in lines]


def _check_against_reference(lines, golden):
    got, ref = _radius_rows(lines), _radius_rows(_radius_text(open(os.path.join(CLI, golden)).read()))
    assert len(got) == len(ref) > 0
    for g, r in zip(got, ref):
        assert (g['radius'], g['recall'], g['targets']) == (r['radius'], r['recall'], r['targets'])
        assert abs(g['auprc'] - r['auprc']) <= 1e-6 and abs(g['rmse'] - r['rmse']) <= 1e-6


def test_two_ranks_radius_search_equals_one_process(gpu_ctx, tmp_path):
    mics = _inputs(tmp_path)
    base = ['extract', '-m', 'resnet8_u32', '--targets', 'targets.txt', '--min-radius', '4', '--max-radius', '16',
            '--step-radius', '4']
    one = _topaz(base + ['-o', 'one.txt'] + mics, tmp_path)
    assert one.returncode == 0, one.stderr[-2000:]
    two = _topaz(base + ['--gpus', '2', '-o', 'two.txt'] + mics, tmp_path, ranks_share_gpu=True)
    assert two.returncode == 0, two.stderr[-2000:]
    lines = _radius_text(two.stdout)
    assert [ln.split(',')[0] for ln in lines] == ['# radius=4', '# radius=8', '# radius=12', '# radius=16']   # rank 0 alone
    assert lines == _radius_text(one.stdout)
    assert _own_stdout(two.stdout) == _own_stdout(one.stdout)     # nothing else on stdout either
    assert two.stderr.count('Optimal radius found') == 1 and two.stderr.count('Finding optimal radius') == 1
    a = open(tmp_path / 'one.txt', 'rb').read()
    assert a.count(b'\n') > 40 and all(n[:-4].encode() + b'\t' in a for n in mics)
    assert open(tmp_path / 'two.txt', 'rb').read() == a            # every rank extracted at the broadcast radius
    # the unlabelled micrograph takes no part in the figures: they are those of the reference's CLI on mic_a and mic_b
    _check_against_reference(lines, 'targets_search_stdout.txt')


def test_two_ranks_validation_equals_one_process(gpu_ctx, tmp_path):
    mics = _inputs(tmp_path)
    base = ['extract', '-m', 'resnet8_u32', '-r', '8', '--assignment-radius', '5', '--targets', 'targets.txt', '--only-validate']
    one = _topaz(base + ['-o', 'one.txt'] + mics, tmp_path)
    assert one.returncode == 0, one.stderr[-2000:]
    two = _topaz(base + ['--gpus', '2', '-o', 'two.txt'] + mics, tmp_path, ranks_share_gpu=True)
    assert two.returncode == 0, two.stderr[-2000:]
    lines = _radius_text(two.stdout)
    assert len(lines) == 1 and lines == _radius_text(one.stdout)
    assert _own_stdout(two.stdout) == _own_stdout(one.stdout)
    assert not os.path.exists(tmp_path / 'one.txt') and not os.path.exists(tmp_path / 'two.txt')
    _check_against_reference(lines, 'targets_validate_stdout.txt')


RCCL_SCRIPT = r'''
import os, sys
import numpy as np
import torch
from topaz_amd import parallel
rank, local_rank, world = parallel.init_from_env()          # backend nccl (RCCL)
assert torch.distributed.get_backend() == "nccl"
dev = parallel.collective_device(local_rank)
assert dev.type == "cuda"
rs = np.random.RandomState(3)
def rec(n, t):
    return ((rs.rand(n) < 0.5).astype(np.float32), np.sort(rs.randn(n).astype(np.float32))[::-1].copy(), float(rs.rand()) * 1e3, t)
sweep = [[rec(5, 3), rec(0, 2), rec(1001, 400)], [rec(4, 3), rec(2, 2), rec(0, 400)]]
sweep[0][0][1][1] = -0.0                                      # bit patterns travel unchanged
out = parallel.gather_radius_records(sweep, [2, 0, 1], dev)
assert len(out) == 2
for got, sent in zip(out, sweep):
    want = [sent[1], sent[2], sent[0]]                       # sorted by image position
    assert len(got) == 3
    for g, w in zip(got, want):
        assert g[0].dtype == np.float32 and g[0].tobytes() == w[0].tobytes() and g[1].tobytes() == w[1].tobytes()
        assert g[2] == w[2] and type(g[2]) is float and g[3] == w[3] and type(g[3]) is int
assert parallel.gather_radius_records([[], []], [], dev) == [[], []]       # a rank without labelled maps
assert parallel.broadcast_int(12, 0, dev) == 12
torch.distributed.destroy_process_group()
print("RCCL_OK")
'''


def test_radius_records_over_a_one_rank_rccl_group(gpu_ctx):
    """the exchange step of the sweep on device tensors over the real backend: a 1-rank 'nccl' (= RCCL) group runs the size
    all_gather, the one int64 gather and the broadcast that a multi-GPU node would otherwise meet first"""
    from topaz_amd import parallel
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''), RANK='0', LOCAL_RANK='0',
               WORLD_SIZE='1', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(parallel.free_port()), TOPAZ_AMD_FORCE_DIST='1',
               HSA_ENABLE_IPC_MODE_LEGACY='0')
    r = subprocess.run([sys.executable, '-c', RCCL_SCRIPT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'RCCL_OK' in r.stdout, r.stdout + r.stderr[-2000:]
