"""`topaz denoise --stack --gpus 2`: the sections of one stack dealt to two rank processes that write one file.
Both ranks drive GPU 0 and meet over gloo, as in tests/test_gpu_parallel.py: two rank processes and no more."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_denoise_options import CUTOFF, SIGMA, _write_stack, mic, model

pytestmark = pytest.mark.gpu
RANK_ENV = dict(TOPAZ_AMD_SHARE_GPU='1', TOPAZ_AMD_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0')
OPTIONS = ['-m', 'unet-small', '--pixel-cutoff', str(CUTOFF), '--gaussian', str(SIGMA), '--stack']


def _topaz(argv, env=None):
    e = dict(os.environ, **(env or {}))
    e['PYTHONPATH'] = ROOT + os.pathsep + e.get('PYTHONPATH', '')
    r = subprocess.run([sys.executable, '-m', 'topaz_amd', 'denoise'] + [str(a) for a in argv], env=e, capture_output=True,
                       text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def _sections_by_rank(stderr):
    """{rank: [sections]} from the one line every rank prints"""
    found = re.findall(r'# rank (\d+) of (\d+): stack sections \[([0-9, ]*)\] of (\d+)', stderr)
    return {int(r): [int(k) for k in s.split(',') if k.strip()] for r, _, s, _ in found}, found


@pytest.mark.parametrize('nz', [3, 1])
def test_two_ranks_write_the_file_of_one_process(gpu_ctx, tmp_path, nz):
    from topaz_amd.denoise import denoise_stack
    from topaz_amd.filters import GaussianDenoise
    sections = [mic('mic_a'), mic('mic_b'), mic('mic_a')[::-1]][:nz]
    _write_stack(tmp_path / 's.mrc', sections, extended=bytes(range(40)))
    one, two = tmp_path / 'one.mrc', tmp_path / 'two.mrc'
    with open(two, 'wb') as f:                                   # a longer file of an earlier run must not shine through
        f.write(b'\xff' * (1024 + 40 + (nz + 1) * 160 * 200 * 4))
    # the one-process file, written in this process with the arguments the command line passes
    denoise_stack(str(tmp_path / 's.mrc'), str(one), [model('unet-small')], 1, CUTOFF, GaussianDenoise(SIGMA), None, False, 1,
                  1024, 500, False, True)
    r2 = _topaz(OPTIONS + ['--gpus', '2', '-o', two, tmp_path / 's.mrc'], env=RANK_ENV)
    a, b = open(one, 'rb').read(), open(two, 'rb').read()
    assert len(a) == 1024 + 40 + nz * 160 * 200 * 4
    assert a == b
    got = np.frombuffer(a[1024 + 40:], dtype=np.float32).reshape(nz, 160, 200)
    assert all(np.abs(s).max() > 0 for s in got)                 # no section left as the zeros rank 0 laid down
    by_rank, lines = _sections_by_rank(r2.stderr)
    assert len(lines) == 2, r2.stderr[-2000:]                    # one line per rank
    assert by_rank == ({0: [0, 2], 1: [1]} if nz == 3 else {0: [0], 1: []})
    assert sorted(k for s in by_rank.values() for k in s) == list(range(nz))
