"""`topaz segment` as a device-resident stream: the maps against model(x) and against the parent's writer, two ranks
sharing the files, --preprocess, --format mrc [--float16], the maps read back by `extract -m none`, patches, a volume."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
CLI = os.path.join(GOLDEN, 'cli')


def _run(argv):
    from topaz_amd.main import main
    main([str(a) for a in argv])


def _pixels(path):
    from topaz_amd.utils.image import load_image
    return np.asarray(load_image(str(path), make_image=False, return_header=False))


def _tiff(path):
    from PIL import Image
    return np.array(Image.open(path))


@pytest.fixture(scope='module')
def inputs(tmp_path_factory):
    """mic_a, mic_b and an int16 copy of mic_a's (rounded) pixels in a directory of their own"""
    from test_cpu_stored_types import write_stored
    d = tmp_path_factory.mktemp('segment_inputs')
    for n in ('mic_a.mrc', 'mic_b.mrc'):
        shutil.copy(os.path.join(CLI, n), d / n)
    a = _pixels(d / 'mic_a.mrc')
    scale = 3000.0 / max(1e-6, float(np.abs(a).max()))
    write_stored(d / 'mic_i16.mrc', np.round(a * scale).astype(np.int16))
    return d, [str(d / n) for n in ('mic_a.mrc', 'mic_b.mrc', 'mic_i16.mrc')]


@pytest.fixture(scope='module')
def model(gpu_ctx):
    from topaz_amd.model.factory import load_model
    m = load_model('resnet8_u32')
    m.eval(); m.fill(); m.cuda(0)
    return m


@pytest.fixture(scope='module')
def one_process(gpu_ctx, inputs, tmp_path_factory):
    """`topaz segment` on the three files, in this process: the directory of the maps"""
    out = tmp_path_factory.mktemp('segment_one')
    _run(['segment', '-m', 'resnet8_u32', '-o', out] + inputs[1])
    return out


def test_tiffs_are_the_models_maps_and_the_parents_bytes(one_process, inputs, model, tmp_path):
    from topaz_amd.commands.segment import MapSink
    for path in inputs[1]:
        x = _pixels(path).astype(np.float32)
        with torch.no_grad():
            want = model(torch.from_numpy(x)[None, None].cuda())[0, 0].cpu().numpy()
        got = _tiff(one_process / (os.path.splitext(os.path.basename(path))[0] + '.tiff'))
        assert got.dtype == np.float32 and got.shape == x.shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), path
        if path.endswith('mic_a.mrc'):
            # the parent's code path: MapSink.write on the array model(x) came back as
            ref = MapSink(str(tmp_path / 'parent'), False).write(path, want)
            assert ref.endswith('mic_a.tiff')
            assert open(ref, 'rb').read() == open(one_process / 'mic_a.tiff', 'rb').read()
    assert sorted(os.listdir(one_process)) == ['mic_a.tiff', 'mic_b.tiff', 'mic_i16.tiff']


def test_two_ranks_write_every_file_once_with_the_same_bytes(one_process, inputs, tmp_path):
    """`segment --gpus 2`: two rank processes on GPU 0 (TOPAZ_AMD_SHARE_GPU=1, gloo), rank r scoring files r, r + 2"""
    env = dict(os.environ, TOPAZ_AMD_SHARE_GPU='1', TOPAZ_AMD_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0')
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    out = tmp_path / 'two'
    r = subprocess.run([sys.executable, '-m', 'topaz_amd', 'segment', '-m', 'resnet8_u32', '-v', '--gpus', '2', '-o', str(out)]
                       + inputs[1], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    names = sorted(os.listdir(out))
    assert names == ['mic_a.tiff', 'mic_b.tiff', 'mic_i16.tiff']
    for n in names:
        assert open(out / n, 'rb').read() == open(one_process / n, 'rb').read(), n
        assert r.stdout.count('# saving: ' + str(out / n[:-5]) + '\n') == 1          # written by exactly one rank


def test_preprocess_flag_equals_segment_of_the_preprocessed_file(gpu_ctx, inputs, tmp_path):
    mic = inputs[1][0]
    _run(['preprocess', '-s', '2', '--sample', '1', '-o', tmp_path / 'pre', mic])
    _run(['segment', '-m', 'resnet8_u32', '-o', tmp_path / 'staged', tmp_path / 'pre' / 'mic_a.mrc'])
    _run(['segment', '-m', 'resnet8_u32', '--preprocess', '2', '--preprocess-sample', '1', '-o', tmp_path / 'fused', mic])
    a, b = _tiff(tmp_path / 'staged' / 'mic_a.tiff'), _tiff(tmp_path / 'fused' / 'mic_a.tiff')
    assert a.shape == (80, 100) and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert open(tmp_path / 'staged' / 'mic_a.tiff', 'rb').read() == open(tmp_path / 'fused' / 'mic_a.tiff', 'rb').read()


def test_format_mrc_and_float16(one_process, inputs, tmp_path, capfd):
    from topaz_amd import mrc
    mic = inputs[1][0]
    want = _tiff(one_process / 'mic_a.tiff')
    _run(['segment', '-m', 'resnet8_u32', '--format', 'mrc', '-o', tmp_path / 'f32', mic])
    got, header, _ = mrc.parse(open(tmp_path / 'f32' / 'mic_a.mrc', 'rb').read())
    _, source, _ = mrc.parse(open(mic, 'rb').read())
    assert header.mode == 2 and (header.nz, header.ny, header.nx) == (1,) + want.shape
    assert header._replace(mode=source.mode) == source                               # the input's header, mode updated
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    _run(['segment', '-m', 'resnet8_u32', '--format', 'mrc', '--float16', '-o', tmp_path / 'f16', mic])
    half, header, _ = mrc.parse(open(tmp_path / 'f16' / 'mic_a.mrc', 'rb').read())
    assert header.mode == 12 and (header.nz, header.ny, header.nx) == (1,) + want.shape
    assert half.dtype == np.float16 and np.array_equal(half.view(np.uint16), want.astype(np.float16).view(np.uint16))
    assert 'beyond the float16 range' not in capfd.readouterr().err                  # (logits: nothing overflows)
    _run(['segment', '-m', 'resnet8_u32', '--format', 'npy', '-o', tmp_path / 'npy', mic])
    assert np.array_equal(np.load(tmp_path / 'npy' / 'mic_a.npy').view(np.uint32), want.view(np.uint32))


def test_extract_from_the_maps_equals_extract_from_the_micrograph(one_process, inputs, tmp_path):
    mic = inputs[1][0]
    _run(['segment', '-m', 'resnet8_u32', '--format', 'mrc', '-o', tmp_path / 'maps', mic])
    base = ['extract', '-r', '8', '-d', '0']
    _run(base + ['-m', 'resnet8_u32', '-o', tmp_path / 'direct.txt', mic])
    _run(base + ['-m', 'none', '-o', tmp_path / 'from_mrc.txt', tmp_path / 'maps' / 'mic_a.mrc'])
    _run(base + ['-m', 'none', '-o', tmp_path / 'from_tiff.txt', one_process / 'mic_a.tiff'])
    want = open(tmp_path / 'direct.txt', 'rb').read()
    assert want.count(b'\n') > 5
    assert open(tmp_path / 'from_mrc.txt', 'rb').read() == want
    assert open(tmp_path / 'from_tiff.txt', 'rb').read() == want


def test_patches_equal_predict_in_patches(gpu_ctx, inputs, model, tmp_path):
    from topaz_amd.model.utils import predict_in_patches
    mic = inputs[1][0]
    _run(['segment', '-m', 'resnet8_u32', '-p', '48', '-o', tmp_path / 'segp', mic])
    got = _tiff(tmp_path / 'segp' / 'mic_a.tiff')
    x = torch.from_numpy(_pixels(mic).astype(np.float32))[None, None]
    want = predict_in_patches(model, x, patch_size=96, is_3d=False, use_cuda=True)[0, 0]
    assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want)


def test_a_volume_writes_the_npy_of_score_map(gpu_ctx, tmp_path):
    from topaz_amd.commands.segment import score_map
    from topaz_amd.model.factory import load_model
    sav = os.path.join(GOLDEN, 'user_model_resnet8_3d_u8.sav')
    shutil.copy(os.path.join(CLI, 'tomo.mrc'), tmp_path / 'tomo.mrc')
    _run(['segment', '-m', sav, '-o', tmp_path / 'seg3', tmp_path / 'tomo.mrc'])
    assert os.listdir(tmp_path / 'seg3') == ['tomo.npy']
    got = np.load(tmp_path / 'seg3' / 'tomo.npy')
    m = load_model(sav)
    m.eval(); m.fill(); m.cuda(0)
    pixels = _pixels(tmp_path / 'tomo.mrc')
    want = score_map(m, pixels)
    assert pixels.ndim == 3 and got.dtype == np.float32 and got.shape == pixels.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # and as an MRC volume that `extract -m none --dims 3` reads back through the feed
    _run(['segment', '-m', sav, '--format', 'mrc', '-o', tmp_path / 'seg3m', tmp_path / 'tomo.mrc'])
    base = ['extract', '--dims', '3', '-r', '4', '-t', '-100', '-d', '0', '-m', 'none']
    _run(base + ['-o', tmp_path / 'a.txt', tmp_path / 'seg3' / 'tomo.npy'])
    _run(base + ['-o', tmp_path / 'b.txt', tmp_path / 'seg3m' / 'tomo.mrc'])
    a = open(tmp_path / 'a.txt', 'rb').read()
    assert a.count(b'\n') > 1 and a == open(tmp_path / 'b.txt', 'rb').read()
