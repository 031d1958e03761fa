"""Host side of `topaz denoise --lowpass` / `--deconvolve` (topaz_amd/denoise.py): the low-pass projection
operators against a float64 restatement of the reference's lowpass (topaz/denoise.py:174-197), the tile geometry and the
unblurring-filter design against what the reference itself produced (tests/golden/denoise_prefilter.npz, written by
tools/make_denoise_prefilter_golden.py), the too-small-tile error and the CLI wiring.  No GPU needed.

The float64 restatements below are shared with tests/test_gpu_denoise_prefilter.py and the fixture tool."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

FIXTURE = os.path.join(GOLDEN, 'denoise_prefilter.npz')
WIDTH = 11


# ---- inputs (regenerated from seeds; only mic_a is a file) -------------------------------------------------------------------
def _blur(x, sigma):
    """separable Gaussian blur (radius ceil(4 sigma), normalised taps, zero padding), float64"""
    r = int(np.ceil(4 * sigma))
    t = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    t /= t.sum()
    xp = np.pad(x.astype(np.float64), r)
    rows = sum(t[k] * xp[k:k + x.shape[0], :] for k in range(2 * r + 1))
    return sum(t[k] * rows[:, k:k + x.shape[1]] for k in range(2 * r + 1))


def make_input(kind, H, W, seed):
    """float32 image: 'randn' N(0, 1), 'poisson' Poisson(5000) raw counts, 'blur' N(0, 1) blurred with sigma 0.4, 'mic_a'"""
    if kind == 'mic_a':
        from topaz_amd import mrc
        with open(os.path.join(GOLDEN, 'cli', 'mic_a.mrc'), 'rb') as f:
            return mrc.parse(f.read())[0].astype(np.float32)
    rng = np.random.RandomState(seed)
    if kind == 'randn':
        return rng.randn(H, W).astype(np.float32)
    if kind == 'poisson':
        return rng.poisson(5000, (H, W)).astype(np.float32)
    if kind == 'blur':
        return _blur(rng.randn(H, W), 0.4).astype(np.float32)
    raise ValueError(kind)


def parse_cases(z, key):
    """rows 'name|kind|H|W|seed|param' of the fixture's case table"""
    out = []
    for row in z[key]:
        name, kind, H, W, seed, param = str(row).split('|')
        out.append((name, kind, int(H), int(W), int(seed), float(param)))
    return out


# ---- float64 restatements --------------------------------------------------------------------------------------------------
def lowpass64(x, factor):
    """the reference's lowpass (denoise.py:174-197) in float64, without its final cast"""
    x = np.asarray(x, dtype=np.float64)
    f0 = np.abs(np.fft.fftfreq(x.shape[0]))[:, None]
    f1 = np.abs(np.fft.rfftfreq(x.shape[1]))[None, :]
    F = np.fft.rfft2(x)
    F[(f0 > 0.5 / factor) | (f1 > 0.5 / factor)] = 0
    return np.fft.irfft2(F, s=x.shape)


def cov64(xt, width=WIDTH):
    """spatial_covariance (denoise.py:22-49) of one halo'd tile in float64"""
    p = width // 2
    xt = np.asarray(xt, dtype=np.float64)
    ch, cw = xt.shape[0] - 2 * p, xt.shape[1] - 2 * p
    xc = xt[p:p + ch, p:p + cw]
    return np.array([[np.vdot(xt[a:a + ch, b:b + cw], xc) for b in range(width)] for a in range(width)]) / (ch * cw)


def min_ps(cov):
    """smallest real power-spectrum value over the non-DC bins (the conditioning precondition of the accuracy inputs)"""
    ps = np.fft.fft2(np.fft.ifftshift(cov)).real.ravel()
    return float(ps[1:].min())


def deconv64(x, patch, width=WIDTH):
    """correct_spatial_covariance(x, patch=P) restated: float64 covariance and filter design per tile, weights rounded to
    float32 as AffineFilter does, then a zero-padded float64 cross-correlation per tile.  Returns (y, covariances)."""
    from topaz_amd.denoise import deconv_tiles, unblur_filter
    x = np.asarray(x, dtype=np.float32)
    H, W = x.shape
    N, M, ry, rx = deconv_tiles(H, W, patch, width)
    p = width // 2
    xp = np.pad(x.astype(np.float64), p)
    y = np.zeros((H, W))
    covs = []
    r0 = 0
    for n, (ya, yl) in zip(N, ry):
        c0 = 0
        for m, (xa, xl) in zip(M, rx):
            c = cov64(x[ya:ya + yl, xa:xa + xl], width)
            covs.append(c)
            w = unblur_filter(c).astype(np.float32).astype(np.float64)
            acc = np.zeros((n, m))
            for a in range(width):
                for b in range(width):
                    acc += w[a, b] * xp[r0 + a:r0 + a + n, c0 + b:c0 + b + m]
            y[r0:r0 + n, c0:c0 + m] = acc
            c0 += m
        r0 += n
    return y, np.stack(covs)


def f32_ulp_bar(ref, scale):
    """|gpu - ref| bar of the lowpass: one fp32 spacing of |ref| plus 1e-9 max|ref| (float64 error near zero)"""
    return np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) + 1e-9 * scale


# ---- tests ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W,factor', [(97, 131, 1.5), (97, 131, 2), (97, 131, 2.5), (97, 131, 4), (96, 128, 2),
                                        (8, 8, 2), (64, 48, 2), (64, 48, 4), (40, 30, 2.5), (33, 1, 3), (3837, 64, 2.5)])
def test_operators_reproduce_the_float64_lowpass(H, W, factor):
    from topaz_amd.denoise import lowpass_operator
    x = np.random.RandomState(H * 1000 + W).poisson(5000, (H, W)).astype(np.float32)
    qh, qw = lowpass_operator(H, factor), lowpass_operator(W, factor, rfft=True)
    assert np.allclose(qh.T @ qh, np.eye(qh.shape[1]), atol=1e-12) and np.allclose(qw.T @ qw, np.eye(qw.shape[1]), atol=1e-12)
    y = qh @ (qh.T @ x.astype(np.float64) @ qw) @ qw.T
    ref = lowpass64(x, factor)
    rel = np.abs(y - ref).max() / np.abs(ref).max()
    print(f'{H}x{W} f={factor}: rank {qh.shape[1]} x {qw.shape[1]}, relative error {rel:.2e}')
    assert rel <= 1e-12


def test_boundary_frequency_is_kept_as_upstream():
    """N = 8, factor 2: frequency 0.25 is not > 0.25, so it stays (rank 1 + 2 * 2); the Nyquist bin always goes"""
    from topaz_amd.denoise import lowpass_operator
    assert lowpass_operator(8, 2.0).shape == (8, 5) and lowpass_operator(8, 2.0, rfft=True).shape == (8, 5)
    assert lowpass_operator(8, 2.0001).shape == (8, 3)
    assert lowpass_operator(9, 1.01).shape == (9, 9) and lowpass_operator(10, 1.01).shape == (10, 9)


def test_lowpass_arguments():
    from topaz_amd.denoise import lowpass
    x = np.ones((4, 5, 6), np.float32)
    with pytest.raises(NotImplementedError):
        lowpass(x, 2, dims=3)
    y = np.ones((5, 6), np.float32)
    assert lowpass(y, 1) is y and lowpass(y, 0.5) is y


def test_fixture_lowpass_matches_the_restatement():
    """the reference's float32 outputs are the float64 restatement rounded once"""
    z = np.load(FIXTURE)
    for name, kind, H, W, seed, factor in parse_cases(z, 'lp_cases'):
        x = make_input(kind, H, W, seed)
        ref64 = lowpass64(x, factor)
        assert np.array_equal(z['lp:' + name], ref64.astype(np.float32)), name


def test_tile_geometry_matches_the_reference():
    from topaz_amd.denoise import deconv_tiles
    z = np.load(FIXTURE)
    for name, kind, H, W, seed, P in parse_cases(z, 'dc_cases'):
        _, _, ry, rx = deconv_tiles(H, W, int(P))
        shapes = [(yl, xl) for (_, yl) in ry for (_, xl) in rx]
        assert np.array_equal(np.array(shapes), z[f'dc:{name}:shapes']), name


def test_unblur_filter_matches_the_reference_from_its_covariances():
    from topaz_amd.denoise import unblur_filter
    z = np.load(FIXTURE)
    n = 0
    for name, kind, H, W, seed, P in parse_cases(z, 'dc_cases'):
        for cov, w in zip(z[f'dc:{name}:cov'], z[f'dc:{name}:winv']):
            assert np.abs(unblur_filter(cov) - w).max() <= 1e-12 * np.abs(w).max(), name
            n += 1
    # the clip branch: a covariance whose spectrum has negative bins, and one with a non-positive DC
    for key in ('clip:cov_neg', 'clip:cov_dc'):
        assert np.abs(unblur_filter(z[key]) - z[key.replace('cov', 'winv')]).max() <= 1e-12 * np.abs(z[key.replace('cov', 'winv')]).max()
    assert min_ps(z['clip:cov_neg']) < 0 and n >= 10


def test_accuracy_inputs_are_well_conditioned():
    """precondition of every deconvolution accuracy input: min Re ps >= 0.25 over the non-DC bins of each tile (float64)"""
    z = np.load(FIXTURE)
    for name, kind, H, W, seed, P in parse_cases(z, 'dc_cases'):
        _, covs = deconv64(make_input(kind, H, W, seed), int(P))
        m = min(min_ps(c) for c in covs)
        print(f'{name}: min ps {m:.3f}')
        assert m >= 0.25, name


@pytest.mark.parametrize('H,W,P', [(10, 200, 1), (200, 10, 1), (40, 200, 8), (200, 16, 3), (17, 23, 3), (30, 30, 40)])
def test_too_small_tiles_are_refused(H, W, P):
    from topaz_amd.denoise import correct_spatial_covariance, deconv_tiles, denoise_image
    with pytest.raises(ValueError, match=f'--deconv-patch {P}'):
        deconv_tiles(H, W, P)
    x = np.zeros((H, W), np.float32)
    with pytest.raises(ValueError, match='smaller than the 11 x 11 filter'):
        correct_spatial_covariance(x, patch=P)          # refused before any device work
    with pytest.raises(ValueError, match='tile'):
        denoise_image(x, [], deconvolve=True, deconv_patch=P)


def test_smallest_accepted_tiles():
    from topaz_amd.denoise import deconv_tiles
    assert deconv_tiles(11, 11, 1) == ([11], [11], [(0, 11)], [(0, 11)])
    assert deconv_tiles(33, 23, 3) == ([11, 11, 11], [8, 8, 7], [(0, 16), (6, 21), (17, 16)], [(0, 13), (3, 18), (11, 12)])
    assert deconv_tiles(5000, 4000, 0)[2:] == ([(0, 5000)], [(0, 4000)])


def test_flags_reach_denoise_stream(monkeypatch, tmp_path):
    from topaz_amd.main import main
    seen = {}

    def fake_stream(micrographs, output_path, format, suffix, models, lowpass, pixel_cutoff, gaus, inv_gaus, deconvolve,
                    deconv_patch, *rest, **kw):
        seen.update(lowpass=lowpass, deconvolve=deconvolve, deconv_patch=deconv_patch, models=models)

    def fake_stack(path, output_path, models, lowpass, pixel_cutoff, gaus, inv_gaus, deconvolve, deconv_patch, *rest):
        seen.update(stack=True, lowpass=lowpass, deconvolve=deconvolve, deconv_patch=deconv_patch)

    import topaz_amd.commands.denoise as cmd
    monkeypatch.setattr(cmd, 'denoise_stream', fake_stream)
    monkeypatch.setattr(cmd, 'denoise_stack', fake_stack)
    monkeypatch.setattr(cmd, 'set_device', lambda d: False)
    mic = os.path.join(GOLDEN, 'cli', 'mic_a.mrc')
    main(['denoise', '-m', 'none', '--lowpass', '2.5', '-o', str(tmp_path), mic])
    assert seen == dict(lowpass=2.5, deconvolve=False, deconv_patch=1, models=[])
    seen.clear()
    main(['denoise', '-m', 'none', '--deconvolve', '--deconv-patch', '3', '-o', str(tmp_path), mic])
    assert seen == dict(lowpass=1, deconvolve=True, deconv_patch=3, models=[])
    seen.clear()
    main(['denoise', '-m', 'none', '--stack', '--deconvolve', '--lowpass', '2', '-o', str(tmp_path / 's.mrc'), mic])
    assert seen == dict(stack=True, lowpass=2, deconvolve=True, deconv_patch=1)


def test_python_defaults_keep_the_reference_deconvolve():
    import inspect
    from topaz_amd.denoise import denoise_image, denoise_image_device, denoise_stack, denoise_stream
    assert inspect.signature(denoise_stream).parameters['deconvolve'].default is True
    assert inspect.signature(denoise_stack).parameters['deconvolve'].default is True
    assert inspect.signature(denoise_image).parameters['deconvolve'].default is False
    p = inspect.signature(denoise_image_device).parameters
    assert (p['lowpass'].default, p['deconvolve'].default, p['deconv_patch'].default) == (1, False, 1)


def test_fixture_is_small():
    assert os.path.getsize(FIXTURE) < 1 << 20
