"""`topaz extract --particle-stack` against the two-command flow it replaces -- `topaz extract -o picks.txt`, then `topaz
particle_stack picks.txt --image-root DIR`: the same crop / standardise / resize kernels see the same pixels at the same
coordinates, so the stack and its STAR file are byte-identical, on one process and on two ranks.

All on tests/golden/cli/mic_a.mrc and mic_b.mrc (160 x 200) with `extract -m resnet8_u32 -r 8`: the 88 picks of
tests/golden/cli/extract_picks.txt, whose 32-pixel boxes cross all four image edges."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
CLI = os.path.join(GOLDEN, 'cli')
META = os.path.join(GOLDEN, 'particle_stack', 'meta_ab.star')
EXTRACT = ['extract', '-m', 'resnet8_u32', '-r', '8', '-d', '0']


def _run(argv):
    from topaz_amd.main import main
    main(argv)


def _bytes(path):
    with open(path, 'rb') as f:
        return f.read()


@pytest.fixture(scope='module')
def raw(tmp_path_factory):
    """the raw directory and the pick table of the plain command, made once and left unchanged"""
    d = tmp_path_factory.mktemp('raw')
    mics = []
    for n in ('mic_a.mrc', 'mic_b.mrc'):
        shutil.copy(os.path.join(CLI, n), d / n)
        mics.append(str(d / n))
    picks = str(tmp_path_factory.mktemp('plain') / 'picks.txt')
    _run(EXTRACT + ['-o', picks] + mics)
    t = pd.read_csv(picks, sep='\t')
    # the picks of the golden table: at S = 32 (half 16) boxes hang over the left, right, top and bottom edge of the 160 x 200
    # images -- no test below can pass on interior boxes only
    assert len(t) == 88
    assert (t.x_coord.min(), t.x_coord.max(), t.y_coord.min(), t.y_coord.max()) == (11, 186, 7, 151)
    assert t.x_coord.min() - 16 < 0 and t.x_coord.max() + 16 > 200 and t.y_coord.min() - 16 < 0 and t.y_coord.max() + 16 > 160
    return str(d), mics, picks


def _fused(out_dir, mics, stack_args, extract_args=(), name='stack.mrcs'):
    os.makedirs(out_dir, exist_ok=True)
    picks, stack = os.path.join(out_dir, 'picks.txt'), os.path.join(out_dir, name)
    _run(EXTRACT + list(extract_args) + ['-o', picks, '--particle-stack', stack] + list(stack_args) + list(mics))
    return picks, stack, os.path.splitext(stack)[0] + '.star'


def _two_commands(out_dir, picks, image_root, ps_args, name='stack.mrcs'):
    os.makedirs(out_dir, exist_ok=True)
    stack = os.path.join(out_dir, name)
    _run(['particle_stack', picks, '--image-root', image_root, '--image-ext', '.mrc', '-o', stack] + list(ps_args))
    return stack, os.path.splitext(stack)[0] + '.star'


@pytest.mark.parametrize('S,R,meta', [(32, None, False), (33, None, False), (32, 16, True), (32, 15, False)])
def test_fused_equals_two_commands_byte_for_byte(gpu_ctx, raw, tmp_path, S, R, meta):
    d, mics, plain = raw
    fused_args, ps_args = ['--particle-size', str(S)], ['--size', str(S)]
    if R:
        fused_args += ['--particle-resize', str(R)]
        ps_args += ['--resize', str(R)]
    if meta:
        fused_args += ['--particle-metadata', META]
        ps_args += ['--metadata', META]
    picks, stack, star = _fused(tmp_path / 'fused', mics, fused_args)
    assert _bytes(picks) == _bytes(plain)                           # the table is what it is without the flag
    two_stack, two_star = _two_commands(tmp_path / 'two', plain, d, ps_args)
    a = _bytes(stack)
    assert len(a) == 1024 + 4 * 88 * (R or S) ** 2 and a[:1024] != bytes(1024)
    assert a == _bytes(two_stack)
    assert _bytes(star) == _bytes(two_star) and _bytes(star).count(b'\n') >= 88 + 2 + 5
    assert np.isfinite(np.frombuffer(a[1024:], np.float32)).all()


def test_per_micrograph_tables_are_unchanged_and_the_stack_is_the_same(gpu_ctx, raw, tmp_path):
    d, mics, plain = raw
    with_dir, without_dir = tmp_path / 'with', tmp_path / 'without'
    os.makedirs(with_dir)
    os.makedirs(without_dir)
    stack = str(tmp_path / 'stack.mrcs')
    _run(EXTRACT + ['--per-micrograph', '-o', str(with_dir), '--particle-stack', stack, '--particle-size', '32'] + mics)
    _run(EXTRACT + ['--per-micrograph', '-o', str(without_dir)] + mics)
    assert sorted(os.listdir(with_dir)) == sorted(os.listdir(without_dir)) == ['mic_a.coord', 'mic_b.coord']
    for n in os.listdir(with_dir):
        assert _bytes(with_dir / n) == _bytes(without_dir / n)
    two_stack, two_star = _two_commands(tmp_path / 'two', plain, d, ['--size', '32'])
    assert _bytes(stack) == _bytes(two_stack) and _bytes(tmp_path / 'stack.star') == _bytes(two_star)


def test_threshold_filters_the_stack_not_the_table(gpu_ctx, raw, tmp_path):
    d, mics, plain = raw
    T = float(np.median(pd.read_csv(plain, sep='\t').score.values))
    picks, stack, star = _fused(tmp_path / 'fused', mics, ['--particle-size', '32', '--particle-threshold', repr(T)])
    assert _bytes(picks) == _bytes(plain)
    kept = (len(_bytes(stack)) - 1024) // (4 * 32 * 32)
    print('threshold', T, 'kept', kept)
    assert 0 < kept < 88
    two_stack, two_star = _two_commands(tmp_path / 'two', plain, d, ['--size', '32', '--threshold', repr(T)])
    assert _bytes(stack) == _bytes(two_stack) and _bytes(star) == _bytes(two_star)
    # nothing survives: an error that names the threshold, no stack, no STAR -- and the table all the same
    out = tmp_path / 'none'
    with pytest.raises(ValueError, match='1000'):
        _fused(out, mics, ['--particle-size', '32', '--particle-threshold', '1000'])
    assert sorted(os.listdir(out)) == ['picks.txt'] and _bytes(out / 'picks.txt') == _bytes(plain)


def test_raw_frames_are_cut_under_preprocess(gpu_ctx, raw, tmp_path):
    """`--preprocess 2 -x 2`: picked on the 80 x 100 normalised image, cut from the 160 x 200 raw frame"""
    d, mics, _ = raw
    pre = ['--preprocess', '2', '--preprocess-sample', '1', '-x', '2']
    picks, stack, star = _fused(tmp_path / 'fused', mics, ['--particle-size', '32'], pre)
    plain = str(tmp_path / 'plain.txt')
    _run(EXTRACT + pre + ['-o', plain] + mics)
    assert _bytes(picks) == _bytes(plain)
    two_stack, two_star = _two_commands(tmp_path / 'two', plain, d, ['--size', '32'])
    a = _bytes(stack)
    assert len(a) > 1024 + 10 * 4 * 32 * 32 and a == _bytes(two_stack) and _bytes(star) == _bytes(two_star)
    # ... and not from the image that was scored: the same table over the preprocessed micrographs gives another first particle
    proc = tmp_path / 'proc'
    _run(['preprocess', '-s', '2', '--sample', '1', '-o', str(proc)] + mics)
    other, _ = _two_commands(tmp_path / 'proc_stack', plain, str(proc), ['--size', '32'])
    first = slice(1024, 1024 + 4 * 32 * 32)
    assert a[first] != _bytes(other)[first]


def test_integer_micrographs_give_the_stack_of_their_float32_twins(gpu_ctx, tmp_path):
    from topaz_amd import mrc
    with open(os.path.join(CLI, 'mic_a.mrc'), 'rb') as f:
        x, _, _ = mrc.parse(f.read())
    q = np.round(100 * x)
    assert np.abs(q).max() < 32767 and len(np.unique(q)) > 100
    stacks = {}
    for dtype in (np.int16, np.float32):
        d = tmp_path / np.dtype(dtype).name
        os.makedirs(d)
        v = q.astype(dtype)
        with open(d / 'mic_q.mrc', 'wb') as f:
            f.write(mrc.header_struct.pack(*list(mrc.make_header(v[None].shape, (1, 1, 1), (0, 0, 0), dtype=dtype))))
            f.write(v.tobytes())
        with open(d / 'mic_q.mrc', 'rb') as f:
            assert mrc.parse_header(f.read(1024)).mode == (1 if dtype is np.int16 else 2)
        picks, stack, star = _fused(d / 'out', [str(d / 'mic_q.mrc')], ['--particle-size', '32'], ['-t', '-100'])
        stacks[dtype] = (_bytes(stack), _bytes(star), _bytes(picks))
    assert len(stacks[np.int16][0]) > 1024 + 10 * 4 * 32 * 32
    assert stacks[np.int16] == stacks[np.float32]


def _topaz(argv, env=None, timeout=600):
    e = dict(os.environ if env is None else env)
    e['PYTHONPATH'] = ROOT + os.pathsep + e.get('PYTHONPATH', '')
    return subprocess.run([sys.executable, '-m', 'topaz_amd'] + argv, env=e, capture_output=True, text=True, timeout=timeout,
                          cwd=ROOT)


@pytest.fixture(scope='module')
def three(raw, tmp_path_factory):
    """three inputs (mic_a again under a third name): on two ranks the last round is ragged.  One-process results, made once."""
    d, mics, _ = raw
    d3 = tmp_path_factory.mktemp('three')
    for n in ('mic_a.mrc', 'mic_b.mrc'):
        shutil.copy(os.path.join(d, n), d3 / n)
    shutil.copy(os.path.join(d, 'mic_a.mrc'), d3 / 'mic_c.mrc')
    mics3 = [str(d3 / n) for n in ('mic_a.mrc', 'mic_b.mrc', 'mic_c.mrc')]
    picks, stack, star = _fused(str(tmp_path_factory.mktemp('one')), mics3, ['--particle-size', '32', '--particle-resize', '16'])
    n_a = int((pd.read_csv(raw[2], sep='\t').image_name == 'mic_a').sum())
    assert 0 < n_a < 88 and len(_bytes(stack)) == 1024 + 4 * (88 + n_a) * 16 * 16
    return str(d3), mics3, picks, stack, star


RANK_ENV = dict(TOPAZ_AMD_SHARE_GPU='1', TOPAZ_AMD_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0')


def test_two_ranks_share_the_gpu_fused_extract_is_byte_identical(gpu_ctx, three, tmp_path):
    d3, mics3, picks, stack, star = three
    out_picks, out_stack = str(tmp_path / 'picks.txt'), str(tmp_path / 'stack.mrcs')
    assert EXTRACT[-2:] == ['-d', '0']                                 # (the ranks take their device from the launcher)
    r = _topaz(EXTRACT[:-2] + ['--gpus', '2', '-o', out_picks, '--particle-stack', out_stack, '--particle-size', '32',
                               '--particle-resize', '16'] + mics3, env=dict(os.environ, **RANK_ENV))
    assert r.returncode == 0, r.stderr[-2000:]
    assert _bytes(out_picks) == _bytes(picks)
    assert _bytes(out_stack) == _bytes(stack)
    assert _bytes(tmp_path / 'stack.star') == _bytes(star)


def test_two_ranks_share_the_gpu_particle_stack_is_byte_identical(gpu_ctx, three, tmp_path):
    d3, mics3, picks, stack, star = three
    args = ['particle_stack', picks, '--image-root', d3, '--size', '32', '--resize', '16']
    os.makedirs(tmp_path / 'one')
    _run(args + ['-o', str(tmp_path / 'one' / 'stack.mrcs')])
    r = _topaz(args + ['--gpus', '2', '-o', str(tmp_path / 'stack.mrcs')], env=dict(os.environ, **RANK_ENV))
    assert r.returncode == 0, r.stderr[-2000:]
    assert _bytes(tmp_path / 'stack.mrcs') == _bytes(tmp_path / 'one' / 'stack.mrcs') == _bytes(stack)
    assert _bytes(tmp_path / 'stack.star') == _bytes(tmp_path / 'one' / 'stack.star') == _bytes(star)


@pytest.mark.parametrize('R,per_micrograph', [(None, 1), (16, 4)])
def test_one_launch_per_micrograph_four_with_resize(gpu_ctx, raw, tmp_path, R, per_micrograph):
    """a micrograph's particles fit one chunk here: cutting them inside `extract` still is one launch, or four with resize"""
    d, mics, _ = raw
    gpu_ctx.prof_enable(1)
    gpu_ctx.prof_reset()
    try:
        _fused(tmp_path / 'fused', mics, ['--particle-size', '32'] + (['--particle-resize', str(R)] if R else []))
        gpu_ctx.sync()
        counts = {name: n for name, ms, n, fl in gpu_ctx.prof_kernels() if name.startswith('particle_')}
    finally:
        gpu_ctx.prof_enable(0)
    print(counts)
    assert len(counts) == per_micrograph and sum(counts.values()) == per_micrograph * len(mics)
