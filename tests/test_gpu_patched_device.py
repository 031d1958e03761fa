"""Patched scoring left on the device: predict_in_patches_device against the reference's golden and, bit for bit,
against a restatement that pads with np.pad, slices, scores every tile and stitches in numpy -- 2-D and 3-D, clipped tiles on
every axis --; the all-zero-tile IndexError raised before any tile is scored; predict_in_patches and Scorer on top of it."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden_sd, load_golden

pytestmark = pytest.mark.gpu
ATOL = 1e-4                                            # (tests/test_gpu_scoring.py)


def _filled(model):
    model.eval(); model.fill(); model.cuda()
    return model


def _restated(model, x, patch_size):
    """topaz/model/utils.py:110-193 in numpy around model(tile): float64 map"""
    from topaz_amd.model.utils import tile_origins
    pad, dims = model.width // 2, x.ndim
    padded = np.pad(x, pad)
    canvas = np.zeros(x.shape)
    crop = (slice(pad, -pad),) * dims
    for origin in tile_origins(x.shape, patch_size - 2 * pad):
        grid = tuple(o for o in origin if o is not None)
        tile = np.ascontiguousarray(padded[tuple(slice(o, o + patch_size) for o in grid)])
        with torch.no_grad():
            s = model(torch.from_numpy(tile)[None, None].cuda())[0, 0].cpu().numpy()
        piece = s[crop]
        canvas[tuple(slice(o, o + n) for o, n in zip(grid, piece.shape))] = piece
    return canvas


@pytest.fixture(scope='module')
def patched_2d(gpu_ctx):
    """(model, golden, patch size given to predict_in_patches, the device map, the restated map): computed once"""
    from topaz_amd.model.factory import load_model
    from topaz_amd.model.utils import predict_in_patches_device
    z = load_golden('score_patched_resnet8_u32')
    m = _filled(load_model('resnet8_u32'))
    size = int(z['patch']) + 2 * (m.width // 2)
    x = torch.from_numpy(z['x0']).cuda()
    y = predict_in_patches_device(m, x, size)
    return m, z, size, y, _restated(m, z['x0'], size)


def test_device_map_against_the_golden_and_the_restatement(patched_2d):
    m, z, size, y, restated = patched_2d
    assert z['x0'].shape == (200, 260) and int(z['patch']) == 96
    assert y.is_cuda and y.dtype == torch.float32 and tuple(y.shape) == z['y0'].shape
    got = y.cpu().numpy()
    assert np.abs(got - z['y0']).max() <= ATOL
    assert np.array_equal(got.astype(np.float64), restated)


def test_float64_canvas_and_predict_in_patches(patched_2d):
    from topaz_amd.model.utils import predict_in_patches, predict_in_patches_device
    m, z, size, y, restated = patched_2d
    x = torch.from_numpy(z['x0'])[None, None]
    y64 = predict_in_patches_device(m, x.cuda(), size, out_dtype=torch.float64)
    assert y64.dtype == torch.float64 and tuple(y64.shape) == tuple(x.shape)
    assert np.array_equal(y64.cpu().numpy()[0, 0], restated)
    host = predict_in_patches(m, x, size, use_cuda=True)
    assert isinstance(host, np.ndarray) and host.dtype == np.float64 and host.shape == tuple(x.shape)
    assert np.array_equal(host[0, 0], restated) and np.array_equal(host[0, 0], y.cpu().numpy().astype(np.float64))


def test_volume_with_clipped_tiles_on_every_axis(gpu_ctx):
    from topaz_amd.model.classifier import LinearClassifier
    from topaz_amd.model.utils import predict_in_patches, predict_in_patches_device, tile_windows
    z = load_golden('score_resnet8_3d_u8')
    m = _filled(LinearClassifier(str(z['arch']), golden_sd(z)))
    assert m.dims == 3
    shape, size = (12, 40, 33), 21 + 2 * (m.width // 2)
    windows = tile_windows(shape, size, m.width // 2)
    for axis in range(3):                                                   # a tile shorter than the patch on every axis
        assert any(w.extent[axis] < size for w in windows)
    assert len(windows) == 4
    x = np.random.RandomState(12).randn(*shape).astype(np.float32)
    restated = _restated(m, x, size)
    y = predict_in_patches_device(m, torch.from_numpy(x).cuda(), size, is_3d=True)
    assert y.dtype == torch.float32 and tuple(y.shape) == shape
    assert np.array_equal(y.cpu().numpy().astype(np.float64), restated)
    host = predict_in_patches(m, torch.from_numpy(x)[None, None], size, is_3d=True)
    assert host.dtype == np.float64 and np.array_equal(host[0, 0], restated)
    # (and the stitched map is the network's: the whole volume in one pass, to the tolerance of the scoring tests)
    with torch.no_grad():
        whole = m(torch.from_numpy(x)[None, None].cuda())[0, 0].cpu().numpy()
    assert np.abs(y.cpu().numpy() - whole).max() <= ATOL


def test_an_all_zero_tile_raises_before_any_tile_is_scored(patched_2d, gpu_ctx):
    from topaz_amd.model.utils import predict_in_patches, predict_in_patches_device
    m, z, size, _, _ = patched_2d
    x = z['x0'].copy()
    # the windows of tiles (96, 96) and (192, 96) are rows [61, 227) / [157, 235) by columns [61, 227): all zero, both
    x[40:250, 40:250] = 0
    x[170, 100] = -0.0
    dev = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    before = gpu_ctx.launches()
    with pytest.raises(IndexError):
        predict_in_patches_device(m, dev, size)
    assert gpu_ctx.launches() - before == 1                                 # tpz_tile_flags, and nothing after it
    with pytest.raises(IndexError):
        predict_in_patches(m, torch.from_numpy(x)[None, None], size)
    x[170, 100] = 1.0                                                       # one pixel in both windows: nothing is skipped
    y = predict_in_patches_device(m, torch.from_numpy(x).cuda(), size)
    assert tuple(y.shape) == x.shape


def test_scorer_picks_from_the_device_map_equal_picks_from_the_float64_map(gpu_ctx):
    from topaz_amd.algorithms import non_maximum_suppression
    from topaz_amd.extract import Scorer
    from topaz_amd.model.utils import predict_in_patches
    from topaz_amd.utils.image import load_image
    x = np.asarray(load_image(os.path.join(GOLDEN, 'cli', 'mic_a.mrc'), make_image=False, return_header=False), dtype=np.float32)
    scorer = Scorer('resnet8_u32', 0)
    patch = 48
    y = scorer(torch.from_numpy(x).cuda(), patch)
    assert y.is_cuda and y.dtype == torch.float32 and tuple(y.shape) == x.shape
    y64 = predict_in_patches(scorer.model, torch.from_numpy(x)[None, None], patch + 2 * (scorer.model.width // 2))[0, 0]
    assert np.array_equal(y.cpu().numpy().astype(np.float64), y64)
    s, c = non_maximum_suppression(y, 8, threshold=-6.0)
    s64, c64 = non_maximum_suppression(y64, 8, threshold=-6.0)
    assert len(s) > 5 and np.array_equal(c, c64) and np.array_equal(s, s64)
