"""`topaz denoise --lowpass` / `--deconvolve` on the MI355X.

Bars.  Lowpass: the reference evaluates in float64 and rounds once to float32, so per pixel
|gpu - ref| <= spacing_f32(|ref|) + 1e-9 max|ref| (one fp32 ulp plus the float64 error near zero).  Deconvolve: with f64 the
float64 restatement (covariance and filter in float64, weights rounded to float32 as AffineFilter does, float64 convolution)
and e_ref the reference's own error against it (fixture), max|gpu - f64| <= max(2 e_ref, 8 * 2^-23 * max|f64|); full-size
inputs without a fixture use the 8-ulp floor alone.  Compositions with a model: 1e-4 absolute after lowpass,
max(1e-4, 2 e_ref) after deconvolve.  Every deconvolution input has min Re ps >= 0.25 over the non-DC bins of each tile."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_cpu_denoise_prefilter import (FIXTURE, deconv64, f32_ulp_bar, lowpass64, make_input, min_ps, parse_cases)

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23
MIC_A = os.path.join(GOLDEN, 'cli', 'mic_a.mrc')


def check_lowpass(gpu, ref, label):
    gpu, ref = np.asarray(gpu), np.asarray(ref, dtype=np.float32)
    assert gpu.dtype == np.float32 and gpu.shape == ref.shape
    err = np.abs(gpu.astype(np.float64) - ref)
    bar = f32_ulp_bar(ref, float(np.abs(ref).max()))
    print(f'{label}: max|gpu - ref| {err.max():.3e}, worst share of the bar {(err / bar).max():.2f}, '
          f'{int((gpu != ref).sum())} of {gpu.size} pixels differ')
    assert np.all(err <= bar), label


def check_deconv(gpu, f64, e_ref, label):
    err = float(np.abs(np.asarray(gpu, dtype=np.float64) - f64).max())
    bound = max(2 * e_ref, 8 * ULP * float(np.abs(f64).max()))
    print(f'{label}: max|gpu - f64| {err:.3e}  e_ref {e_ref:.3e}  bound {bound:.3e}  ({err / bound:.3f} of it)')
    assert err <= bound, (label, err, bound)


def test_fixture_lowpass_cases(gpu_ctx):
    from topaz_amd.denoise import lowpass
    z = np.load(FIXTURE)
    for name, kind, H, W, seed, factor in parse_cases(z, 'lp_cases'):
        check_lowpass(lowpass(make_input(kind, H, W, seed), factor), z['lp:' + name], name)


def test_fixture_deconvolve_cases(gpu_ctx):
    from topaz_amd.denoise import correct_spatial_covariance
    z = np.load(FIXTURE)
    for name, kind, H, W, seed, P in parse_cases(z, 'dc_cases'):
        x = make_input(kind, H, W, seed)
        f64, covs = deconv64(x, int(P))
        assert min(min_ps(c) for c in covs) >= 0.25, name
        gpu = correct_spatial_covariance(x, patch=int(P))
        assert gpu.dtype == np.float32 and gpu.shape == x.shape
        check_deconv(gpu, f64, float(z[f'dc:{name}:e_ref']), name)


def test_device_covariances_match_float64(gpu_ctx):
    import torch
    from topaz_amd import runtime as rt
    x = make_input('mic_a', 0, 0, 0)
    for P in (1, 2, 3, 4):
        _, covs = deconv64(x, P)
        got = rt.spatial_cov_2d(torch.from_numpy(x).cuda(), P)
        rel = np.abs(got - covs).max() / np.abs(covs).max()
        print(f'P={P}: covariance relative error {rel:.2e}')
        assert rel <= 1e-12


@pytest.mark.parametrize('H,W,factor', [(4096, 4096, 2), (4096, 4096, 4), (3837, 3709, 2.5)])
def test_full_size_lowpass_on_raw_counts(gpu_ctx, H, W, factor):
    from topaz_amd.denoise import lowpass
    x = np.random.RandomState(H + W + int(4 * factor)).poisson(5000, (H, W)).astype(np.float32)
    check_lowpass(lowpass(x, factor), lowpass64(x, factor).astype(np.float32), f'{H}x{W} f={factor}')


@pytest.mark.parametrize('P', [1, 4])
def test_full_size_deconvolve(gpu_ctx, P):
    from topaz_amd.denoise import correct_spatial_covariance
    x = np.random.RandomState(40960 + P).randn(4096, 4096).astype(np.float32)
    f64, covs = deconv64(x, P)
    assert min(min_ps(c) for c in covs) >= 0.25
    check_deconv(correct_spatial_covariance(x, patch=P), f64, 0.0, f'4096^2 P={P}')


def test_bit_identical_on_two_calls(gpu_ctx):
    import torch
    from topaz_amd.denoise import correct_spatial_covariance, lowpass
    x = torch.from_numpy(np.random.RandomState(3).randn(1500, 1300).astype(np.float32)).cuda()
    for fn in (lambda: lowpass(x, 2.5), lambda: correct_spatial_covariance(x, patch=3), lambda: correct_spatial_covariance(x)):
        a, b = fn(), fn()
        assert torch.equal(a, b)


def test_launch_counts_do_not_depend_on_the_patch_count(gpu_ctx):
    import torch
    from topaz_amd.denoise import correct_spatial_covariance, lowpass
    x = torch.from_numpy(np.random.RandomState(4).randn(700, 900).astype(np.float32)).cuda()
    counts = {}
    for key, fn in [('lp2', lambda: lowpass(x, 2)), ('lp4', lambda: lowpass(x, 4))] + \
                   [(f'dc{P}', (lambda P=P: correct_spatial_covariance(x, patch=P))) for P in (1, 2, 4, 9)]:
        gpu_ctx.prof_enable(1)
        gpu_ctx.prof_reset()
        fn()
        counts[key] = gpu_ctx.prof_get(2)[1]
        gpu_ctx.prof_enable(0)
    print(counts)
    assert counts['lp2'] == counts['lp4'] == 4
    assert counts['dc1'] == counts['dc2'] == counts['dc4'] == counts['dc9'] == 3


def _err(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max())


def test_deconvolve_then_affine_model(gpu_ctx):
    from topaz_amd.denoise import Denoise, denoise_image
    z = np.load(FIXTURE)
    x = np.load(os.path.join(GOLDEN, 'denoise2d_pretrained.npz'))['x']
    got = denoise_image(x.copy(), [Denoise('affine')], deconvolve=True)
    bar = max(1e-4, 2 * float(z['comp:deconv:affine:e_ref']))
    print(f'deconvolve + affine: {_err(got, z["comp:deconv:affine"]):.3e} (bar {bar:.1e})')
    assert _err(got, z['comp:deconv:affine']) <= bar


def _read(path):
    from topaz_amd import mrc
    with open(path, 'rb') as f:
        return mrc.parse(f.read())[0]


def _cli(args):
    r = subprocess.run([sys.executable, '-m', 'topaz_amd', 'denoise'] + args, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r


@pytest.mark.parametrize('model', ['none', 'unet-small'])
@pytest.mark.parametrize('flags,key', [(['--lowpass', '2'], 'lowpass2'), (['--deconvolve', '--deconv-patch', '3'], 'deconv_p3')])
def test_cli(gpu_ctx, tmp_path, model, flags, key):
    z = np.load(FIXTURE)
    _cli(['-m', model] + flags + ['-o', str(tmp_path), MIC_A])
    got = _read(tmp_path / 'mic_a.mrc')
    ref = z[f'cli:{key}:{model}']
    bar = 1e-4 if key == 'lowpass2' else max(1e-4, 2 * float(z[f'cli:{key}:{model}:e_ref']))
    print(f'CLI -m {model} {" ".join(flags)}: {_err(got, ref):.3e} (bar {bar:.1e})')
    assert got.shape == ref.shape and _err(got, ref) <= bar


@pytest.mark.parametrize('flags,key', [(['--lowpass', '2'], 'lowpass2'), (['--deconvolve', '--deconv-patch', '3'], 'deconv_p3')])
def test_cli_stack(gpu_ctx, tmp_path, flags, key):
    from topaz_amd import mrc
    z = np.load(FIXTURE)
    mic = _read(MIC_A)
    src = tmp_path / 'stack.mrc'
    with open(src, 'wb') as f:
        mrc.write(f, np.stack([mic, mic]))
    _cli(['-m', 'none', '--stack'] + flags + ['-o', str(tmp_path / 'out.mrc'), str(src)])
    got = _read(tmp_path / 'out.mrc')
    ref = z[f'cli:{key}:none']
    bar = 1e-4 if key == 'lowpass2' else max(1e-4, 2 * float(z[f'cli:{key}:none:e_ref']))
    assert got.shape == (2,) + ref.shape
    for k in range(2):
        print(f'stack section {k} {" ".join(flags)}: {_err(got[k], ref):.3e} (bar {bar:.1e})')
        assert _err(got[k], ref) <= bar


def test_plain_path_unchanged(gpu_ctx, tmp_path):
    """the default arguments leave denoise_image_device as it was: same bytes with the new flags absent or at their defaults,
    and the plain CLI path writes exactly what denoise_image_device returns"""
    import torch
    from topaz_amd.denoise import Denoise, denoise_image_device, denoise_stream
    d = Denoise('unet-small')
    x = torch.from_numpy(_read(MIC_A).astype(np.float32)).cuda()
    a = denoise_image_device(x, [d], 1024, 500, False)
    b = denoise_image_device(x, [d], 1024, 500, False, lowpass=1, deconvolve=False, deconv_patch=1)
    assert torch.equal(a, b)
    denoise_stream([MIC_A], str(tmp_path), models=[d], deconvolve=False, patch_size=1024, padding=500, normalize=False,
                   return_images=False)
    assert np.array_equal(_read(tmp_path / 'mic_a.mrc'), a.cpu().numpy())
