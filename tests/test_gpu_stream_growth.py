"""Mixed image sizes through the two real loops on top of streaming.stream_images: the second file's result (520 x 520 float32,
1.08 MB) does not fit the 1 MiB slots the first one made, so the pinned result ring is drained, closed and made anew between
them, and the third file goes through the larger ring.  Every comparison is bit for bit against the per-file path."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(40, 40), (520, 520), (40, 48)]


@pytest.fixture
def micrographs(tmp_path):
    from topaz_amd.utils.image import save_image
    paths = []
    for i, shape in enumerate(SHAPES):
        rs = np.random.RandomState(40 + i)
        x = (rs.randn(*shape) * 40 + 900).astype(np.float32)
        yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
        for cy, cx in rs.randint(5, 35, size=(6, 2)):
            x -= (110 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * 3.0 ** 2))).astype(np.float32)
        paths.append(str(tmp_path / f'mic_{i}.mrc'))
        save_image(x, paths[-1])
    return paths


@pytest.fixture
def stages(monkeypatch):
    """every rt.Stage made, in order; each notes how many two-slot rings (the result rings) were open when it was made"""
    from topaz_amd import runtime as rt
    made = []

    class Stage(rt.Stage):
        def __init__(self, ctx, slot_bytes, depth=2):
            self.open_result_rings = sum(1 for s in made if s.depth == 2 and s.handle)
            super().__init__(ctx, slot_bytes, depth)
            made.append(self)

    monkeypatch.setattr(rt, 'Stage', Stage)
    return made


def _grew_once(stages):
    rings = [s for s in stages if s.depth == 2]
    assert [s.slot_bytes for s in rings] == [1 << 20, 2 << 20]
    assert [s.open_result_rings for s in rings] == [0, 0]                  # the outgrown ring was closed before the next was made
    assert all(s.handle is None for s in stages)                           # and nothing is left open


def _tree(d):
    return {name: open(os.path.join(d, name), 'rb').read() for name in sorted(os.listdir(d))}


def test_normalize_stream_writes_the_per_file_bytes_across_a_ring_growth(gpu_ctx, tmp_path, micrographs, stages):
    from topaz_amd import stats as tstats
    a, b = str(tmp_path / 'stream'), str(tmp_path / 'per_file')
    tstats.normalize_images(micrographs, a, 0, scale=1, affine=False, niters=100, alpha=900, beta=1, sample=1, metadata=True,
                            formats=['mrc'])
    _grew_once(stages)
    os.makedirs(b)
    worker = tstats.Normalize(b, 1, False, 100, 900, 1, 1, True, ['mrc'])
    for p in micrographs:
        worker(p)
    got, want = _tree(a), _tree(b)
    assert sorted(got) == sorted(want) and len(want) == 6
    for name in want:
        assert got[name] == want[name], name


def test_denoise_stream_returns_the_per_image_arrays_across_a_ring_growth(gpu_ctx, tmp_path, micrographs, stages):
    from topaz_amd.denoise import denoise_image_device, denoise_stream
    from topaz_amd.utils.image import load_image
    out = denoise_stream(micrographs, str(tmp_path / 'out'), models=[], pixel_cutoff=2.5, return_images=True)
    _grew_once(stages)
    assert len(out) == 3
    for path, got, shape in zip(micrographs, out, SHAPES):
        x = torch.from_numpy(load_image(path, make_image=False, return_header=False).astype(np.float32)).cuda()
        # (the options denoise_stream passes on by default)
        want = denoise_image_device(x, [], 1024, 500, True, lowpass=1, deconvolve=True, deconv_patch=1, cutoff=2.5).cpu().numpy()
        assert got.shape == shape and got.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), path
        written = np.ascontiguousarray(load_image(str(tmp_path / 'out' / os.path.basename(path)), make_image=False,
                                                  return_header=False), dtype=np.float32)
        assert np.array_equal(written.view(np.uint32), want.view(np.uint32)), path
