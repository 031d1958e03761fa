"""`--float16` on every command that writes MRC: the file is mode 12, its header the float32 file's with only the
mode changed, its pixels the bytes of astype(np.float16) of the float32 file's -- whichever way the result left the device (the
result ring, two ranks writing one file, tpz_encode on a resident volume).  PNG / JPEG output, quantised on the device, keeps its
bytes.  Overflow is reported on stderr.  All on the fixtures of tests/golden/cli and tests/golden/particle_stack."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
CLI = os.path.join(GOLDEN, 'cli')
PS = os.path.join(GOLDEN, 'particle_stack')
RANK_ENV = dict(TOPAZ_AMD_SHARE_GPU='1', TOPAZ_AMD_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0')
EXTRACT = ['extract', '-m', 'resnet8_u32', '-r', '8', '-d', '0']
DENOISE3D = ['denoise3d', '-m', os.path.join(CLI, 'unet3d_nf8_state.sav'), '--base-kernel-width', '7', '-s', '32', '-p', '16',
             '-d', '0']


def _run(argv):
    from topaz_amd.main import main
    main([str(a) for a in argv])


def _topaz(argv, env=None):
    e = dict(os.environ, **(env or {}))
    e['PYTHONPATH'] = ROOT + os.pathsep + e.get('PYTHONPATH', '')
    r = subprocess.run([sys.executable, '-m', 'topaz_amd'] + [str(a) for a in argv], env=e, capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def _bytes(path):
    with open(path, 'rb') as f:
        return f.read()


def _half(x):
    with np.errstate(over='ignore', invalid='ignore'):
        return x.astype(np.float16)


def assert_float16_twin(path16, path32):
    """the three properties of a --float16 file against the file the same command writes without the flag"""
    from topaz_amd import mrc
    a, b = _bytes(path16), _bytes(path32)
    h16, h32 = mrc.parse_header(a[:1024]), mrc.parse_header(b[:1024])
    assert h32.mode == 2 and h16.mode == 12
    assert h16 == h32._replace(mode=12)
    n = h32.nx * h32.ny * h32.nz
    assert a[1024:1024 + h32.next] == b[1024:1024 + h32.next]                       # the extended header
    assert len(b) == 1024 + h32.next + 4 * n and len(a) == 1024 + h32.next + 2 * n
    x32 = np.frombuffer(b[1024 + h32.next:], dtype=np.float32)
    x16 = np.frombuffer(a[1024 + h32.next:], dtype=np.uint16)
    assert np.array_equal(x16, _half(x32).view(np.uint16))
    assert np.abs(x32[np.isfinite(x32)]).max() > 0
    return x32


@pytest.fixture(scope='module')
def mics(tmp_path_factory):
    d = tmp_path_factory.mktemp('mics')
    for n in ('mic_a.mrc', 'mic_b.mrc', 'tomo.mrc'):
        shutil.copy(os.path.join(CLI, n), d / n)
    return d


@pytest.fixture(scope='module')
def preprocessed(mics, tmp_path_factory):
    """`preprocess -s 2 --sample 1` of the two micrographs without and with the flag, made once and only read"""
    out = tmp_path_factory.mktemp('pre')
    args = ['preprocess', '-s', '2', '--sample', '1', mics / 'mic_a.mrc', mics / 'mic_b.mrc']
    _run(args + ['-o', out / 'f32', '--metadata'])
    _run(args + ['-o', out / 'f16', '--metadata', '--float16'])
    return out


def test_preprocess(gpu_ctx, preprocessed):
    for name in ('mic_a', 'mic_b'):
        x = assert_float16_twin(preprocessed / 'f16' / (name + '.mrc'), preprocessed / 'f32' / (name + '.mrc'))
        assert x.size == 80 * 100
        assert _bytes(preprocessed / 'f16' / (name + '.metadata.json')) == _bytes(preprocessed / 'f32' / (name + '.metadata.json'))
    assert sorted(os.listdir(preprocessed / 'f16')) == sorted(os.listdir(preprocessed / 'f32'))


@pytest.mark.parametrize('extra', [[], ['--affine']])
def test_normalize(gpu_ctx, mics, tmp_path, extra):
    args = ['normalize', '--sample', '1', mics / 'mic_a.mrc'] + extra
    _run(args + ['-o', tmp_path / 'f32'])
    _run(args + ['-o', tmp_path / 'f16', '--float16'])
    assert_float16_twin(tmp_path / 'f16' / 'mic_a.mrc', tmp_path / 'f32' / 'mic_a.mrc')


def test_downsample(gpu_ctx, mics, tmp_path):
    _run(['downsample', '-s', '2', '-o', tmp_path / 'f32.mrc', mics / 'mic_a.mrc'])
    _run(['downsample', '-s', '2', '-o', tmp_path / 'f16.mrc', '--float16', mics / 'mic_a.mrc'])
    assert assert_float16_twin(tmp_path / 'f16.mrc', tmp_path / 'f32.mrc').size == 80 * 100


def test_denoise_files(gpu_ctx, mics, tmp_path):
    args = ['denoise', '-m', 'unet-small', '-d', '0', mics / 'mic_a.mrc', mics / 'mic_b.mrc']
    _run(args + ['-o', tmp_path / 'f32'])
    _run(args + ['-o', tmp_path / 'f16', '--float16'])
    for name in ('mic_a.mrc', 'mic_b.mrc'):
        assert_float16_twin(tmp_path / 'f16' / name, tmp_path / 'f32' / name)


@pytest.fixture(scope='module')
def stacks(tmp_path_factory):
    """`denoise --stack` of frames3.mrc (three 96 x 128 sections, below the ring's threshold) and of a three-section stack of the
    160 x 200 micrographs with an extended header (through the ring), one process, without and with the flag"""
    from topaz_amd import mrc
    from topaz_amd.denoise import RING_MIN_BYTES
    d = tmp_path_factory.mktemp('stacks')
    shutil.copy(os.path.join(PS, 'frames3.mrc'), d / 'frames3.mrc')
    a, header, _ = mrc.parse(_bytes(os.path.join(CLI, 'mic_a.mrc')))
    b = mrc.parse(_bytes(os.path.join(CLI, 'mic_b.mrc')))[0]
    big = np.stack([np.tile(a, (2, 2)), np.tile(b, (2, 2)), np.tile(a[::-1], (2, 2))])           # 3 x 320 x 400: 512 000 bytes
    big = np.concatenate([big, big[:, :, ::-1]], axis=2)                                         # 3 x 320 x 800: 1 024 000
    big = np.concatenate([big, big[:, :8]], axis=1)                                              # 3 x 328 x 800
    assert 4 * big[0].size >= RING_MIN_BYTES > 4 * 96 * 128
    ext = bytes(range(40))
    with open(d / 'big.mrc', 'wb') as f:
        mrc.write(f, big, header=header._replace(nx=800, ny=328, nz=3, next=len(ext)), extended_header=ext)
    for name in ('frames3', 'big'):
        args = ['denoise', '-m', 'unet-small', '-d', '0', '--stack', d / (name + '.mrc')]
        _run(args + ['-o', d / (name + '_f32.mrc')])
        _run(args + ['-o', d / (name + '_f16.mrc'), '--float16'])
    return d


@pytest.mark.parametrize('name', ['frames3', 'big'])
def test_denoise_stack(gpu_ctx, stacks, name):
    x = assert_float16_twin(stacks / (name + '_f16.mrc'), stacks / (name + '_f32.mrc'))
    assert x.size == (3 * 96 * 128 if name == 'frames3' else 3 * 328 * 800)


@pytest.mark.parametrize('name', ['frames3', 'big'])
def test_denoise_stack_two_ranks_write_the_file_of_one_process(gpu_ctx, stacks, tmp_path, name):
    out = tmp_path / 'two.mrc'
    with open(out, 'wb') as f:                                   # a longer file of an earlier run must not shine through
        f.write(b'\xff' * (len(_bytes(stacks / (name + '_f32.mrc'))) + 100))
    r = _topaz(['denoise', '-m', 'unet-small', '--stack', '--gpus', '2', '--float16', '-o', out, stacks / (name + '.mrc')],
               env=RANK_ENV)
    assert _bytes(out) == _bytes(stacks / (name + '_f16.mrc'))
    assert r.stderr.count('stack sections') == 2


def test_denoise3d(gpu_ctx, mics, tmp_path):
    _run(DENOISE3D + ['-o', tmp_path / 'f32', mics / 'tomo.mrc'])
    _run(DENOISE3D + ['-o', tmp_path / 'f16', '--float16', mics / 'tomo.mrc'])
    assert assert_float16_twin(tmp_path / 'f16' / 'tomo.mrc', tmp_path / 'f32' / 'tomo.mrc').size == 36 * 40 * 44


@pytest.mark.parametrize('picks,root,size,resize,meta', [
    (os.path.join(CLI, 'extract_picks.txt'), CLI, 32, None, None),
    (os.path.join(CLI, 'extract_picks.txt'), CLI, 32, 16, os.path.join(PS, 'meta_ab.star')),
    (os.path.join(PS, 'picks3.txt'), PS, 9, None, os.path.join(PS, 'meta3.star')),      # three frames; a particle of NaN
])
def test_particle_stack(gpu_ctx, tmp_path, picks, root, size, resize, meta):
    args = ['particle_stack', picks, '--image-root', root, '--size', size]
    args += (['--resize', resize] if resize else []) + (['--metadata', meta] if meta else [])
    _run(args + ['-o', tmp_path / 'f32.mrcs'])
    _run(args + ['-o', tmp_path / 'f16.mrcs', '--float16'])
    x = assert_float16_twin(tmp_path / 'f16.mrcs', tmp_path / 'f32.mrcs')
    assert _bytes(tmp_path / 'f16.star').replace(b'f16.mrcs', b'f32.mrcs') == _bytes(tmp_path / 'f32.star')
    if root == PS:
        assert np.isnan(x).sum() == 243                          # NaN payloads follow numpy's rule too
    if root == CLI and resize:                                   # two ranks write the same float16 file
        os.makedirs(tmp_path / 'two')
        _topaz(args + ['-o', tmp_path / 'two' / 'f16.mrcs', '--float16', '--gpus', '2'], env=RANK_ENV)
        assert _bytes(tmp_path / 'two' / 'f16.mrcs') == _bytes(tmp_path / 'f16.mrcs')
        assert _bytes(tmp_path / 'two' / 'f16.star') == _bytes(tmp_path / 'f16.star')


@pytest.fixture(scope='module')
def fused(mics, tmp_path_factory):
    """`extract --particle-stack` over mic_a, mic_b and mic_a under a third name (a ragged last round on two ranks), one process,
    without and with the flag"""
    d = tmp_path_factory.mktemp('fused')
    shutil.copy(mics / 'mic_a.mrc', d / 'mic_a.mrc')
    shutil.copy(mics / 'mic_b.mrc', d / 'mic_b.mrc')
    shutil.copy(mics / 'mic_a.mrc', d / 'mic_c.mrc')
    paths = [d / 'mic_a.mrc', d / 'mic_b.mrc', d / 'mic_c.mrc']
    for kind, flag in (('f32', []), ('f16', ['--float16'])):
        os.makedirs(d / kind)
        _run(EXTRACT + ['-o', d / kind / 'picks.txt', '--particle-stack', d / kind / 'stack.mrcs', '--particle-size', '32',
                        '--particle-resize', '16'] + flag + paths)
    return d, paths


def test_extract_particle_stack(gpu_ctx, fused):
    d, _ = fused
    x = assert_float16_twin(d / 'f16' / 'stack.mrcs', d / 'f32' / 'stack.mrcs')
    assert x.size > 88 * 16 * 16
    assert _bytes(d / 'f16' / 'stack.star') == _bytes(d / 'f32' / 'stack.star')
    assert _bytes(d / 'f16' / 'picks.txt') == _bytes(d / 'f32' / 'picks.txt')


def test_extract_particle_stack_two_ranks_write_the_file_of_one_process(gpu_ctx, fused, tmp_path):
    d, paths = fused
    _topaz(EXTRACT[:-2] + ['--gpus', '2', '-o', tmp_path / 'picks.txt', '--particle-stack', tmp_path / 'stack.mrcs',
                           '--particle-size', '32', '--particle-resize', '16', '--float16'] + paths, env=RANK_ENV)
    assert _bytes(tmp_path / 'stack.mrcs') == _bytes(d / 'f16' / 'stack.mrcs')
    assert _bytes(tmp_path / 'stack.star') == _bytes(d / 'f16' / 'stack.star')
    assert _bytes(tmp_path / 'picks.txt') == _bytes(d / 'f16' / 'picks.txt')


def test_extract_reads_the_float16_preprocess_output(gpu_ctx, preprocessed, tmp_path):
    """the next command gets float16 input for free: its picks are those of the float32 files rounded to float16"""
    from topaz_amd import mrc
    os.makedirs(tmp_path / 'rounded')
    for name in ('mic_a.mrc', 'mic_b.mrc'):
        x, header, extended = mrc.parse(_bytes(preprocessed / 'f32' / name))
        with open(tmp_path / 'rounded' / name, 'wb') as f:
            mrc.write(f, x.astype(np.float16).astype(np.float32)[None], header=header, extended_header=extended)
    tables = {}
    for kind, d in (('f16', preprocessed / 'f16'), ('rounded', tmp_path / 'rounded')):
        _run(EXTRACT + ['-o', tmp_path / (kind + '.txt'), d / 'mic_a.mrc', d / 'mic_b.mrc'])
        tables[kind] = _bytes(tmp_path / (kind + '.txt'))
    assert tables['f16'] == tables['rounded'] and tables['f16'].count(b'\n') > 3


@pytest.mark.parametrize('fmt', ['png', 'jpg'])
def test_denoise_eight_bit_formats_keep_their_bytes(gpu_ctx, mics, tmp_path, fmt):
    """the uint8 image is made on the device now; the file is what save_image writes from the float32 result of the same run"""
    from topaz_amd.denoise import Denoise, denoise_stream
    from topaz_amd.utils.image import save_image
    src = [str(mics / 'mic_a.mrc'), str(mics / 'mic_b.mrc')]
    _run(['denoise', '-m', 'unet-small', '-d', '0', '--format', fmt, '-o', tmp_path / 'cli'] + src)
    # the float32 results of the same run: return_images keeps the ring on float32 (the command does not ask for them)
    images = denoise_stream(src, str(tmp_path / 'f32'), format=fmt, models=[Denoise('unet-small')], deconvolve=False,
                            normalize=True, return_images=True)
    for path, image in zip(src, images):
        name = os.path.splitext(os.path.basename(path))[0] + '.' + fmt
        assert image.dtype == np.float32 and image.shape == (160, 200)
        save_image(image, str(tmp_path / ('host_' + name)))
        assert _bytes(tmp_path / 'cli' / name) == _bytes(tmp_path / ('host_' + name)) == _bytes(tmp_path / 'f32' / name)
        assert len(_bytes(tmp_path / 'cli' / name)) > 1000


def test_normalize_mrc_and_png_puts_the_image_once_per_stored_type(gpu_ctx, mics, tmp_path):
    from topaz_amd import mrc
    from topaz_amd.utils.image import save_image
    _run(['normalize', '--sample', '1', '--format', 'mrc,png', '--metadata', '-o', tmp_path / 'both', mics / 'mic_a.mrc'])
    _run(['normalize', '--sample', '1', '--format', 'mrc', '--metadata', '-o', tmp_path / 'mrc', mics / 'mic_a.mrc'])
    _run(['preprocess', '--sample', '1', '--format', 'png', '-o', tmp_path / 'png', mics / 'mic_a.mrc'])
    assert sorted(os.listdir(tmp_path / 'both')) == ['mic_a.metadata.json', 'mic_a.mrc', 'mic_a.png']
    assert _bytes(tmp_path / 'both' / 'mic_a.mrc') == _bytes(tmp_path / 'mrc' / 'mic_a.mrc')
    assert _bytes(tmp_path / 'both' / 'mic_a.metadata.json') == _bytes(tmp_path / 'mrc' / 'mic_a.metadata.json')
    x = mrc.parse(_bytes(tmp_path / 'mrc' / 'mic_a.mrc'))[0]
    save_image(x, str(tmp_path / 'host.png'))
    assert _bytes(tmp_path / 'both' / 'mic_a.png') == _bytes(tmp_path / 'host.png') == _bytes(tmp_path / 'png' / 'mic_a.png')
    assert os.listdir(tmp_path / 'png') == ['mic_a.png']


@pytest.mark.parametrize('options', [[], ['--pixel-cutoff', '1e9']], ids=['host-pass-through', 'device-ring'])
def test_overflow_is_reported_and_stored_as_inf(gpu_ctx, tmp_path, capsys, options):
    """three pixels of 1e6 through `denoise -m none` (the host loop) and through the filter-only device path (a cutoff nothing
    reaches): stderr names the file and the count, the file holds inf there and the float16 of the float32 file elsewhere"""
    from topaz_amd import mrc
    x, header, _ = mrc.parse(_bytes(os.path.join(CLI, 'mic_a.mrc')))
    x = x.copy()
    spots = [(3, 5), (80, 100), (159, 199)]
    for i, j in spots:
        x[i, j] = 1e6
    with open(tmp_path / 'hot.mrc', 'wb') as f:
        mrc.write(f, x[None], header=header)
    args = ['denoise', '-m', 'none', '-d', '0'] + options + [tmp_path / 'hot.mrc']
    _run(args + ['-o', tmp_path / 'f32'])
    capsys.readouterr()
    _run(args + ['-o', tmp_path / 'f16', '--float16'])
    err = capsys.readouterr().err
    lines = [ln for ln in err.split('\n') if 'float16 range' in ln]
    assert len(lines) == 1, err
    assert str(tmp_path / 'f16' / 'hot.mrc') in lines[0] and ': 3 finite value' in lines[0]
    y32 = assert_float16_twin(tmp_path / 'f16' / 'hot.mrc', tmp_path / 'f32' / 'hot.mrc').reshape(160, 200)
    y16 = mrc.parse(_bytes(tmp_path / 'f16' / 'hot.mrc'))[0]
    assert all(np.isposinf(y16[i, j]) and np.isfinite(y32[i, j]) for i, j in spots)
    assert np.isinf(y16).sum() == 3
