"""The device-resident `topaz preprocess` / `topaz normalize` stream against the per-file path that stays in the tree
(`Normalize`, `normalize`, `norm_fit`, `downsample`, `tpz_gmm_fit`) and against numpy: every comparison is bit for bit."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

from topaz_amd import stats as tstats  # noqa: E402

PIS = np.array(tstats.INIT_PIS, dtype=np.float64)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ---- order statistics ------------------------------------------------------------------------------------------------
def _order_inputs(n):
    rs = np.random.RandomState(n % 9973)
    yield 'randn', rs.randn(n).astype(np.float32)
    yield 'counts', rs.poisson(5000, n).astype(np.float32)                                        # heavy ties
    yield 'constant', np.full(n, -7.5, dtype=np.float32)
    x = (rs.randn(n) * 10.0 ** rs.randint(-44, 3, n)).astype(np.float32)                          # mixed signs, subnormals
    x[::5] = 0
    yield 'mixed', x


@pytest.mark.parametrize('n', [1, 2, 255, 256, 257, 65537, 1000003])
def test_order_stats_and_quantiles_equal_numpy(gpu_ctx, n):
    from topaz_amd import runtime as rt
    for name, x in _order_inputs(n):
        xd = _dev(x)
        want = np.quantile(x, 1 - PIS)
        got = tstats.quantiles_device(xd, 1 - PIS)
        assert got.dtype == np.float64 and np.array_equal(got, want), (name, n, got, want)
        ranks = np.unique(np.concatenate([[0, n - 1, n // 2, n // 3], np.random.RandomState(3).randint(0, n, 20)]))
        assert np.array_equal(rt.order_stats(xd, ranks), np.sort(x)[ranks]), (name, n)


def test_order_stats_nan_and_bad_rank(gpu_ctx):
    from topaz_amd import runtime as rt
    from topaz_amd._lib import TopazHipError
    x = np.random.RandomState(0).randn(65537).astype(np.float32)
    x[40000] = np.nan
    assert np.isnan(np.quantile(x, 1 - PIS)).all()
    assert np.isnan(tstats.quantiles_device(_dev(x), 1 - PIS)).all()
    assert np.isnan(rt.order_stats(_dev(x), [0, 5, 65536])).all()
    with pytest.raises(TopazHipError):
        rt.order_stats(_dev(x), [65537])
    with pytest.raises(TopazHipError):
        rt.order_stats(_dev(x), list(range(33)))


# ---- fused fit -------------------------------------------------------------------------------------------------------
_FIT_CACHE = {}


def _fit_pixels(name):
    if name not in _FIT_CACHE:
        if name.startswith('normalize_'):
            g = load_golden(name)
            x, sample = g['x'], int(g['sample'])
            if sample > 1:
                np.random.seed(int(g['seed']))
                x, _ = tstats._fit_pixels(x, sample)
            x = np.ascontiguousarray(x.ravel())
        else:
            n = {'bimodal': 1000003, 'small': 300}[name]             # 1 000 003: more than 256 blocks and a ragged tail
            rs = np.random.RandomState(n)
            x = np.where(rs.rand(n) < 0.85, rs.randn(n), 3.5 + 0.8 * rs.randn(n)).astype(np.float32)
        _FIT_CACHE[name] = (_dev(x), np.quantile(x, 1 - PIS).astype(np.float64))
    return _FIT_CACHE[name]


@pytest.mark.parametrize('scale', [1, 10])
@pytest.mark.parametrize('num_iters', [1, 100])
@pytest.mark.parametrize('name', ['normalize_s1', 'normalize_s4', 'bimodal', 'small'])
def test_fused_fit_equals_gmm_fit_bit_for_bit(gpu_ctx, name, num_iters, scale):
    from topaz_amd import runtime as rt
    xd, splits = _fit_pixels(name)
    want = rt.gmm_fit(xd, PIS, splits, alpha=900, beta=1, scale=scale, num_iters=num_iters)
    *got, n_passes = rt.gmm_fit_fused(xd, PIS, splits, alpha=900, beta=1, scale=scale, num_iters=num_iters)
    for key, a, b in zip(('mus', 'stds', 'pis', 'logps'), got, want):
        assert np.array_equal(_bits(a), _bits(b)), (key, a, b)
    # one pass for the moments, one for the hard split, one first E-step, at most num_iters more
    assert 3 <= n_passes <= num_iters + 3, n_passes


def test_fused_fit_with_more_initialisations_than_one_launch_holds(gpu_ctx):
    """25 initialisations: three launches per pass (11 + 11 + 2 two-component ones) and a single-component one in the middle"""
    from topaz_amd import runtime as rt
    xd, _ = _fit_pixels('small')
    pis = np.concatenate([np.linspace(0.04, 0.96, 12), [1.0], np.linspace(0.07, 0.93, 12)])
    splits = np.quantile(xd.cpu().numpy(), 1 - pis).astype(np.float64)
    want = rt.gmm_fit(xd, pis, splits, num_iters=30)
    *got, n_passes = rt.gmm_fit_fused(xd, pis, splits, num_iters=30)
    for key, a, b in zip(('mus', 'stds', 'pis', 'logps'), got, want):
        assert np.array_equal(_bits(a), _bits(b)), (key, a, b)
    assert 3 <= n_passes <= 33


@pytest.mark.parametrize('method,sample', [('gmm', 1), ('gmm', 10), ('affine', 1)])
def test_normalize_device_equals_normalize(gpu_ctx, method, sample):
    x = load_golden('normalize_s1')['x'] * np.float32(37.5) + np.float32(900)
    np.random.seed(5)
    want, meta_want = tstats.normalize(x.copy(), sample=sample, method=method)
    np.random.seed(5)
    got, meta_got = tstats.normalize_device(_dev(x), sample=sample, method=method)
    assert got.is_cuda and np.array_equal(_bits(got.cpu().numpy()), _bits(want))
    assert list(meta_got) == list(meta_want)
    for key in meta_want:
        assert type(meta_got[key]) is type(meta_want[key]), key
        assert np.array_equal(_bits(np.asarray(meta_got[key], dtype=np.float64)), _bits(np.asarray(meta_want[key], dtype=np.float64))), key


# ---- elementwise, gather, downsample ---------------------------------------------------------------------------------
def test_normalize_f64_equals_numpy_with_float64_scalars(gpu_ctx):
    from topaz_amd import runtime as rt
    x = np.random.RandomState(2).poisson(5000, (613, 1031)).astype(np.float32)                    # raw counts: |mu| >> std
    mu, std = np.float64(5003.3712345678), np.float64(70.710678118654755)
    want = ((x - mu) / std).astype(np.float32)
    assert np.array_equal(_bits(rt.normalize_f64(_dev(x), mu, std).cpu().numpy()), _bits(want))
    with np.errstate(divide='ignore', invalid='ignore'):
        want0 = ((x - np.float64(5000.0)) / np.float64(0.0)).astype(np.float32)
    got0 = rt.normalize_f64(_dev(x), 5000.0, 0.0).cpu().numpy()
    assert np.isnan(want0).any() and np.isinf(want0).any()
    assert np.array_equal(got0, want0, equal_nan=True)


def test_gather_equals_fancy_indexing(gpu_ctx):
    from topaz_amd import runtime as rt
    from topaz_amd._lib import TopazHipError
    x = np.random.RandomState(4).randn(333, 517).astype(np.float32)
    idx = np.random.RandomState(5).permutation(x.size)[:x.size // 10]
    assert np.array_equal(_bits(rt.gather(_dev(x), idx).cpu().numpy()), _bits(x.ravel()[idx]))
    idx = np.array([x.size - 1, 0, 0, 77], dtype=np.int64)
    assert np.array_equal(_bits(rt.gather(_dev(x), idx).cpu().numpy()), _bits(x.ravel()[idx]))
    for bad in (x.size, -1):
        with pytest.raises(TopazHipError):
            rt.gather(_dev(x), [0, bad, 1])


@pytest.mark.parametrize('case', ['even_f2', 'even_f4', 'odd_f3', 'odd_f8'])
def test_downsample_device_equals_downsample(gpu_ctx, case):
    from topaz_amd.utils.image import downsample, downsample_device
    g = load_golden('downsample_cases')
    x, factor = g[case + ':x'], int(g[case + ':factor'])
    want = downsample(x, factor)
    got = downsample_device(_dev(x), factor)
    assert got.is_cuda and np.array_equal(_bits(got.cpu().numpy()), _bits(want))


# ---- the stream against the per-file path ----------------------------------------------------------------------------
def _micrographs(tmp_path):
    """five inputs of different sizes (the output ring has to grow), formats and pixel types"""
    from PIL import Image
    from topaz_amd import mrc
    from topaz_amd.utils.image import save_image
    paths = []
    for i, shape in enumerate([(256, 256), (320, 352), (300, 280), (416, 384), (288, 400)]):
        rs = np.random.RandomState(70 + i)
        x = (rs.randn(*shape) * 40 + 900).astype(np.float32)
        yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
        for cy, cx in rs.randint(15, 240, size=(25, 2)):
            x -= (110 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * 5.0 ** 2))).astype(np.float32)
        if i == 2:                                                    # MRC mode 1: int16 pixels
            p = str(tmp_path / f'mic_{i}.mrc')
            raw = np.round(x).astype(np.int16)
            header = mrc.make_header((1,) + shape, (1, 1, 1), (0, 0, 0), dtype=np.int16, dmin=raw.min(), dmax=raw.max(),
                                     dmean=raw.mean(), rms=raw.std())
            with open(p, 'wb') as fh:
                fh.write(mrc.header_struct.pack(*list(header)))
                fh.write(raw.tobytes())
        elif i == 3:
            p = str(tmp_path / f'mic_{i}.tiff')
            Image.fromarray(x).save(p, 'tiff')
        else:
            p = str(tmp_path / f'mic_{i}.mrc')
            save_image(x, p)
        paths.append(p)
    return paths


def _tree(d):
    return {name: open(os.path.join(d, name), 'rb').read() for name in sorted(os.listdir(d))}


@pytest.mark.parametrize('scale,sample,affine', [(4, 10, False), (1, 10, False), (4, 10, True), (1, 10, True)])
def test_stream_writes_the_per_file_paths_bytes(gpu_ctx, tmp_path, scale, sample, affine):
    paths = _micrographs(tmp_path)
    formats = ['mrc', 'png']
    a, b = str(tmp_path / 'stream'), str(tmp_path / 'per_file')
    np.random.seed(7)
    tstats.normalize_images(paths, a, 0, scale, affine, 100, 900, 1, sample, True, formats)
    os.makedirs(b)
    np.random.seed(7)
    worker = tstats.Normalize(b, scale, affine, 100, 900, 1, sample, True, formats)
    for p in paths:
        worker(p)
    got, want = _tree(a), _tree(b)
    assert sorted(got) == sorted(want) and len(want) == 15
    for name in want:
        assert got[name] == want[name], name


def test_missing_file_raises_in_the_caller_and_leaves_no_thread(gpu_ctx, tmp_path):
    paths = _micrographs(tmp_path)
    paths.insert(2, str(tmp_path / 'not_there.mrc'))
    before = set(threading.enumerate())
    with pytest.raises(OSError):
        tstats.normalize_images(paths, str(tmp_path / 'out'), 0, 4, False, 100, 900, 1, 10, True, ['mrc'])
    assert [t for t in threading.enumerate() if t not in before and t.is_alive()] == []


# ---- two ranks -------------------------------------------------------------------------------------------------------
def _topaz(argv, env=None, timeout=600):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ if env is None else env)
    e['PYTHONPATH'] = root + os.pathsep + e.get('PYTHONPATH', '')
    return subprocess.run([sys.executable, '-m', 'topaz_amd'] + argv, env=e, capture_output=True, text=True, timeout=timeout,
                          cwd=root)


def test_two_ranks_share_the_gpu_preprocess_is_byte_identical(gpu_ctx, tmp_path):
    """`topaz preprocess --gpus 2`: two rank processes, both on GPU 0 (TOPAZ_AMD_SHARE_GPU=1, gloo), write disjoint files that
    equal the one-process run's byte for byte (--sample 1: no RNG draw depends on the sharding)"""
    paths = [p for p in _micrographs(tmp_path) if p.endswith('.mrc')]
    assert len(paths) == 4
    one, two = str(tmp_path / 'one'), str(tmp_path / 'two')
    args = ['preprocess', '-s', '2', '--sample', '1', '--metadata']
    r = _topaz(args + ['-o', one] + paths)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, TOPAZ_AMD_SHARE_GPU='1', TOPAZ_AMD_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0')
    r = _topaz(args + ['--gpus', '2', '-o', two] + paths, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got, want = _tree(two), _tree(one)
    assert sorted(got) == sorted(want) and len(want) == 8
    for name in want:
        assert got[name] == want[name], name
