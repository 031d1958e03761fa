"""`topaz extract --preprocess S` against the two-command flow it replaces -- `topaz preprocess -s S -o proc/` (or `topaz
normalize`), then `topaz extract proc/*.mrc`: the same kernels see the same bits (a float32 MRC round-trips exactly), so the pick
files are byte-identical."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
CLI = os.path.join(GOLDEN, 'cli')
EXTRACT = ['extract', '-m', 'resnet8_u32', '-r', '4', '-t', '-100', '-d', '0']       # (a low threshold: every local maximum is a pick)


def _run(argv):
    from topaz_amd.main import main
    main(argv)


def _raw(tmp_path):
    mics = []
    for n in ('mic_a.mrc', 'mic_b.mrc'):
        shutil.copy(os.path.join(CLI, n), tmp_path / n)
        mics.append(str(tmp_path / n))
    return mics


def _two_commands(tmp_path, mics, pre_args, extract_args, command='preprocess'):
    proc = tmp_path / 'proc'
    _run([command] + pre_args + ['-o', str(proc)] + mics)
    staged = [str(proc / os.path.basename(p)) for p in mics]
    assert all(os.path.exists(p) for p in staged)
    _run(EXTRACT + extract_args + staged)


@pytest.mark.parametrize('fused,pre,command', [
    (['--preprocess', '2', '--preprocess-sample', '1'], ['-s', '2', '--sample', '1'], 'preprocess'),
    (['--preprocess', '2', '--preprocess-sample', '1', '--preprocess-affine'], ['-s', '2', '--sample', '1', '--affine'], 'preprocess'),
    (['--preprocess', '1', '--preprocess-sample', '1'], ['--sample', '1'], 'normalize'),
])
def test_fused_pick_file_equals_two_commands_byte_for_byte(gpu_ctx, tmp_path, fused, pre, command):
    mics = _raw(tmp_path)
    one, two = tmp_path / 'fused.txt', tmp_path / 'two_step.txt'
    _run(EXTRACT + fused + ['-o', str(one)] + mics)
    _two_commands(tmp_path, mics, pre, ['-o', str(two)], command)
    a, b = open(one, 'rb').read(), open(two, 'rb').read()
    assert a.count(b'\n') > 20 and b'mic_a\t' in a and b'mic_b\t' in a
    assert a == b
    if fused[1] == '2':
        # picks live in the frame of the scored 80 x 100 image, not of the raw 160 x 200 one
        t = pd.read_csv(one, sep='\t')
        assert t.x_coord.max() < 100 and t.y_coord.max() < 80
        # ... and differ from picking on the raw frames
        _run(EXTRACT + ['-o', str(tmp_path / 'raw.txt')] + mics)
        assert open(tmp_path / 'raw.txt', 'rb').read() != a


def test_fused_per_micrograph_star_equals_two_commands(gpu_ctx, tmp_path):
    mics = _raw(tmp_path)
    fused_dir, two_dir = tmp_path / 'fused', tmp_path / 'two'
    os.makedirs(fused_dir)
    os.makedirs(two_dir)
    tail = ['--per-micrograph', '--format', 'star']
    _run(EXTRACT + ['--preprocess', '2', '--preprocess-sample', '1'] + tail + ['-o', str(fused_dir)] + mics)
    _two_commands(tmp_path, mics, ['-s', '2', '--sample', '1'], tail + ['-o', str(two_dir)])
    names = sorted(os.listdir(fused_dir))
    assert names == ['mic_a.star', 'mic_b.star'] == sorted(os.listdir(two_dir))
    for n in names:
        a = open(fused_dir / n, 'rb').read()
        assert a.count(b'\n') > 10 and a == open(two_dir / n, 'rb').read(), n


def test_up_scale_moves_the_picks_back_to_the_raw_frame(gpu_ctx, tmp_path):
    mics = _raw(tmp_path)
    fused = ['--preprocess', '2', '--preprocess-sample', '1']
    _run(EXTRACT + fused + ['-o', str(tmp_path / 'x1.txt')] + mics)
    _run(EXTRACT + fused + ['-x', '2', '-o', str(tmp_path / 'x2.txt')] + mics)
    a, b = pd.read_csv(tmp_path / 'x1.txt', sep='\t'), pd.read_csv(tmp_path / 'x2.txt', sep='\t')
    assert len(a) == len(b) > 20 and a.image_name.tolist() == b.image_name.tolist()
    assert np.array_equal(b[['x_coord', 'y_coord']].values, np.round(a[['x_coord', 'y_coord']].values * 2).astype(int))
    assert np.array_equal(a.score.values, b.score.values)


def test_sampled_fit_gives_identical_score_maps_in_process(gpu_ctx, tmp_path):
    """sample = 10 draws from the global NumPy RNG: seeded alike, the fused flow draws in the order the stream does"""
    from topaz_amd import stats as tstats
    from topaz_amd.extract import score_images
    mics = _raw(tmp_path)
    np.random.seed(21)
    pre = tstats.DevicePreprocess(2, False, 100, 900, 1, 10)
    fused = [(p, s.clone()) for p, s in score_images('resnet8_u32', mics, keep_on_device=True, preprocess=pre)]
    assert pre.last_meta['sample'] == 10 and len(pre.last_meta['mus']) == 12
    np.random.seed(21)
    proc = tmp_path / 'proc'
    tstats.normalize_images(mics, str(proc), 0, 2, False, 100, 900, 1, 10, False, ['mrc'])
    staged = [str(proc / os.path.basename(p)) for p in mics]
    two = [(p, s.clone()) for p, s in score_images('resnet8_u32', staged, keep_on_device=True)]
    assert len(fused) == len(two) == 2
    for (pa, a), (pb, b) in zip(fused, two):
        assert os.path.basename(pa) == os.path.basename(pb) and tuple(a.shape) == tuple(b.shape) == (80, 100)
        assert torch.equal(a, b)
    # (another seed fits other pixels: the maps move -- the equality above is not vacuous)
    np.random.seed(22)
    other = [s.clone() for _, s in score_images('resnet8_u32', mics, keep_on_device=True, preprocess=pre)]
    assert not torch.equal(other[0], fused[0][1])


def _topaz(argv, env=None, timeout=600):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ if env is None else env)
    e['PYTHONPATH'] = root + os.pathsep + e.get('PYTHONPATH', '')
    return subprocess.run([sys.executable, '-m', 'topaz_amd'] + argv, env=e, capture_output=True, text=True, timeout=timeout,
                          cwd=root)


def test_two_ranks_share_the_gpu_fused_extract_is_byte_identical(gpu_ctx, tmp_path):
    """`topaz extract --preprocess 2 --gpus 2`: two rank processes on GPU 0 (TOPAZ_AMD_SHARE_GPU=1, gloo) against one process
    (--preprocess-sample 1: no RNG draw depends on the sharding)"""
    mics = _raw(tmp_path)
    one, two = str(tmp_path / 'one.txt'), str(tmp_path / 'two.txt')
    fused = ['--preprocess', '2', '--preprocess-sample', '1']
    _run(EXTRACT + fused + ['-o', one] + mics)
    env = dict(os.environ, TOPAZ_AMD_SHARE_GPU='1', TOPAZ_AMD_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0')
    assert EXTRACT[-2:] == ['-d', '0']                                 # (the ranks take their device from the launcher)
    r = _topaz(EXTRACT[:-2] + fused + ['--gpus', '2', '-o', two] + mics, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    a = open(one, 'rb').read()
    assert a.count(b'\n') > 20 and a == open(two, 'rb').read()
