"""The host side of patched scoring on the device: tile_windows against a numpy restatement of get_patches /
reconstruct_from_patches that pads with np.pad and slices, as the reference does; the `segment` parser and its refusals; the
rank sharding of segment_images.  No GPU."""
import os
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN

SHAPES_2D = [(1, 1), (7, 9), (200, 260), (96, 96)]
PAD_PATCH_2D = [(3, 10), (35, 166), (35, 71)]                 # (the last: step 1)
SHAPES_3D = [(5, 7, 9), (12, 40, 33)]
PAD_PATCH_3D = [(2, 8)]
CASES = [(s, p, q) for s in SHAPES_2D for p, q in PAD_PATCH_2D] + [(s, p, q) for s in SHAPES_3D for p, q in PAD_PATCH_3D]


def _window_of(x, origin, extent):
    """the window of x at origin (may leave x), zero outside: numpy's statement of what tpz_tile_cut makes"""
    out = np.zeros(extent, dtype=x.dtype)
    src, dst = [], []
    for o, e, n in zip(origin, extent, x.shape):
        lo, hi = max(o, 0), min(o + e, n)
        if lo >= hi:
            return out
        src.append(slice(lo, hi))
        dst.append(slice(lo - o, hi - o))
    out[tuple(dst)] = x[tuple(src)]
    return out


@pytest.mark.parametrize('shape,pad,patch', CASES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_tile_windows_against_pad_and_slice(shape, pad, patch):
    from topaz_amd.model.utils import tile_origins, tile_windows
    dims = len(shape)
    x = (np.arange(int(np.prod(shape)), dtype=np.int64) + 1).reshape(shape)          # (no zero: padding is told from content)
    padded = np.pad(x, pad)
    step = patch - 2 * pad
    origins = tile_origins(shape, step)
    windows = tile_windows(shape, patch, pad)
    assert len(windows) == len(origins)
    crop = (slice(pad, -pad),) * dims
    canvas = np.zeros(shape, dtype=np.int64)
    covered = np.zeros(shape, dtype=np.int32)
    for origin, w in zip(origins, windows):
        k, i, j = origin
        grid = (i, j) if k is None else (k, i, j)                                    # the order equals tile_origins
        assert w.paste == grid and w.origin == tuple(o - pad for o in grid)
        ref = padded[tuple(slice(o, o + patch) for o in grid)]                        # the reference's tile: a slice, clipped
        assert w.extent == ref.shape
        tile = _window_of(x, w.origin, w.extent)
        assert np.array_equal(tile, ref)
        piece = ref[crop]                                                             # what the reference stitches
        assert w.pasted == piece.shape and min(w.pasted) >= 1
        box = tuple(slice(o, o + n) for o, n in zip(w.paste, w.pasted))
        assert canvas[box].shape == piece.shape                                       # (inside the canvas: nothing is clipped)
        canvas[box] = tile[crop]
        covered[box] += 1
    assert (covered == 1).all()                                                       # the pasted boxes tile the canvas once
    assert np.array_equal(canvas, x)


@pytest.mark.parametrize('shape', [(7, 9), (5, 7, 9)])
def test_tile_windows_refuses_a_step_that_is_not_positive(shape):
    from topaz_amd.model.utils import tile_windows
    for pad, patch in ((3, 6), (3, 5), (35, 70)):
        with pytest.raises(ValueError):
            tile_windows(shape, patch, pad)


def test_predict_in_patches_device_keeps_the_existing_value_error():
    from topaz_amd.model.utils import predict_in_patches_device
    model = types.SimpleNamespace(width=71)
    for is_3d in (False, True):
        with pytest.raises(ValueError, match='does not exceed the receptive field 71'):
            predict_in_patches_device(model, torch.zeros(1, 1, 8, 8, 8), 70, is_3d)


# ---- the `segment` parser ----------------------------------------------------------------------------------------------
def _parse(argv):
    from topaz_amd.commands import segment
    return segment.add_arguments().parse_args(argv)


def test_segment_parser_defaults_and_new_flags():
    s = _parse(['-o', 'seg/', 'm.mrc'])
    assert (s.model, s.device, s.patch_size, s.destdir, s.paths, s.verbose, s.gpus, s.num_threads, s.precision_check) == \
        ('resnet16', 0, None, 'seg/', ['m.mrc'], False, 0, 0, 'auto')
    assert (s.preprocess, s.preprocess_affine, s.preprocess_sample, s.preprocess_niters, s.preprocess_alpha, s.preprocess_beta) == \
        (0, False, 10, 100, 900, 1)
    assert s.format is None and s.float16 is False
    s = _parse(['-o', 'seg/', '--preprocess', '4', '--preprocess-sample', '1', '--preprocess-affine', '--format', 'mrc', '--float16',
                '--gpus', '2', '-p', '48', 'a.mrc', 'b.mrc'])
    assert (s.preprocess, s.preprocess_sample, s.preprocess_affine, s.format, s.float16, s.gpus, s.patch_size) == \
        (4, 1, True, 'mrc', True, 2, 48)
    for fmt in ('tiff', 'mrc', 'npy'):
        assert _parse(['--format', fmt, 'm.mrc']).format == fmt
    with pytest.raises(SystemExit):
        _parse(['--format', 'png', 'm.mrc'])


REFUSED = [
    (['--float16'], 'mrc'),
    (['--float16', '--format', 'tiff'], 'mrc'),
    (['--float16', '--format', 'npy'], 'mrc'),
    (['--preprocess', '2', '--preprocess-sample', '1'], 'micrographs'),                  # (the input is a volume)
    (['--preprocess', '-1'], 'reduction factor'),
]


@pytest.mark.parametrize('extra,match', REFUSED)
def test_segment_refusals_touch_no_gpu(monkeypatch, tmp_path, extra, match):
    from topaz_amd import cuda, parallel, streaming
    from topaz_amd.commands import segment
    from topaz_amd.model import factory

    def boom(*a, **k):
        raise AssertionError('nothing may be loaded before the arguments are checked')

    monkeypatch.setattr(cuda, 'set_device', boom)
    monkeypatch.setattr(factory, 'load_model', boom)
    monkeypatch.setattr(parallel, 'init_from_env', boom)
    monkeypatch.setattr(streaming, 'stream_images', boom)
    args = _parse(['-m', 'resnet8_u32', '-o', str(tmp_path / 'seg')] + extra + [os.path.join(GOLDEN, 'cli', 'tomo.mrc')])
    with pytest.raises(ValueError, match=match):
        segment.main(args)
    assert not (tmp_path / 'seg').exists()


def test_float16_needs_mrc_in_segment_images_too():
    from topaz_amd.commands import segment
    with pytest.raises(ValueError, match='mrc'):
        segment.segment_images(object(), ['a.mrc'], 'nowhere', True, False, float16=True)


# ---- the ranks ---------------------------------------------------------------------------------------------------------
class _FakeScorer:
    device_model = types.SimpleNamespace(ctx=None)

    def __call__(self, x):
        return x * 2


def test_segment_images_shards_the_paths_over_the_ranks(monkeypatch, tmp_path):
    """five paths, WORLD_SIZE=2: rank r scores and writes paths r, r + 2, ... and no other; together, each exactly once"""
    from PIL import Image
    from topaz_amd import parallel, streaming
    from topaz_amd.commands import segment
    paths = [f'/data/mic_{i}.mrc' for i in range(5)]
    seen = {}

    def fake_stream(items, ctx, process, write, on_overflow=None):
        for p in items:
            put = process(p, torch.full((4, 5), float(paths.index(p))), None, None)
            assert put.encode is None
            write(put.tensor.numpy(), *put.payload)

    monkeypatch.setattr(streaming, 'stream_images', fake_stream)
    monkeypatch.setenv('WORLD_SIZE', '2')
    for rank in (0, 1):
        monkeypatch.setenv('RANK', str(rank))
        monkeypatch.setenv('LOCAL_RANK', str(rank))
        monkeypatch.setattr(parallel, 'init_from_env', lambda backend=None, rank=rank: (rank, rank, 2))
        out = tmp_path / f'rank{rank}'
        segment.segment_images(_FakeScorer(), paths, str(out), True, False)
        seen[rank] = sorted(os.listdir(out))
    assert seen[0] == ['mic_0.tiff', 'mic_2.tiff', 'mic_4.tiff'] and seen[1] == ['mic_1.tiff', 'mic_3.tiff']
    for rank in (0, 1):
        for name in seen[rank]:
            got = np.array(Image.open(tmp_path / f'rank{rank}' / name))
            assert got.dtype == np.float32 and (got == 2.0 * int(name[4])).all()
