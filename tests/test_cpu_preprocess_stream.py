"""Host side of the preprocess / normalize stream (topaz_amd/stats.py): the quantile interpolation and the sub-sample positions
against numpy itself, bit for bit, and the `--gpus` flag of the two commands.  No GPU."""
import numpy as np
import pytest

from topaz_amd import stats as tstats

Q_INIT = 1 - np.array(tstats.INIT_PIS, dtype=np.float64)            # the twelve splits of norm_fit


def _samples(n):
    rs = np.random.RandomState(n)
    yield 'randn', rs.randn(n).astype(np.float32)
    yield 'counts', rs.poisson(5000, n).astype(np.float32)                                        # heavy ties
    yield 'constant', np.full(n, 3.25, dtype=np.float32)
    x = (rs.randn(n) * 10.0 ** rs.randint(-44, 3, n)).astype(np.float32)                          # mixed signs, subnormals
    x[::3] = 0
    yield 'mixed', x
    yield 'two_values', np.where(rs.rand(n) < 0.5, -1.5, 2.5).astype(np.float32)


def _host_quantiles(x, q):
    """quantiles_device with the radix select replaced by a host sort: the brackets and the interpolation are what is tested"""
    s = np.sort(x)
    lo, hi, gamma = tstats._quantile_brackets(x.size, q)
    return tstats._lerp_quantiles(s[lo], s[hi], gamma)


@pytest.mark.parametrize('n', [1, 2, 3, 257, 100003])
def test_quantile_interpolation_equals_numpy_bit_for_bit(n):
    qs = [Q_INIT, np.array([0.0, 1.0]), np.array([0.0, 1e-9, 0.25, 0.5, 0.5 + 1e-12, 0.999999, 1.0]),
          np.random.RandomState(5).rand(16)]
    for name, x in _samples(n):
        for q in qs:
            got, want = _host_quantiles(x, q), np.quantile(x, q)
            assert got.dtype == want.dtype == np.float64, (name, got.dtype, want.dtype)
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (name, n, q, got, want)


def test_quantile_brackets_reject_out_of_range():
    with pytest.raises(ValueError):
        tstats._quantile_brackets(10, [0.5, 1.5])


@pytest.mark.parametrize('size,sample', [(36000, 10), (36000, 4), (1001, 3), (7, 2)])
def test_sample_indices_select_numpys_pixels_and_leave_the_rng_alike(size, sample):
    x = np.random.RandomState(size).randn(size).astype(np.float32)
    np.random.seed(11)
    want, weight = tstats._fit_pixels(x, sample)
    after_want = np.random.random_sample(4)
    np.random.seed(11)
    idx = tstats.sample_indices(size, sample)
    after_got = np.random.random_sample(4)
    assert idx.shape == want.shape and weight == size / len(idx)
    assert np.array_equal(x[idx].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(after_got, after_want)


@pytest.mark.parametrize('command', ['normalize', 'preprocess'])
def test_parsers_accept_gpus(command):
    """(fails without the stream: the flag table of the two commands had no --gpus)"""
    import importlib
    module = importlib.import_module('topaz_amd.commands.' + command)
    args = module.add_arguments().parse_args(['a.mrc', 'b.mrc', '-o', 'out', '--gpus', '2', '-s', '4'])
    assert args.gpus == 2 and args.scale == 4 and args.files == ['a.mrc', 'b.mrc']
    assert module.add_arguments().parse_args(['a.mrc']).gpus == 0
    from topaz_amd.main import _ranks_to_launch
    assert _ranks_to_launch(args) in (0, 2)                    # (0 inside a rank process)
