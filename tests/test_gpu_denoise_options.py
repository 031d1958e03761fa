"""`topaz denoise --pixel-cutoff / --gaussian / --inv-gaussian / --stack` with the micrograph staying on the MI355X
(DESIGN.md §14).

Bars.  tpz_normalize_cutoff: bit for bit the numpy mask applied to what tpz_normalize returns.  Images: the project's 1e-4
absolute on the returned pixels (tests/test_gpu_denoise.py), against what the reference's denoise_image returned
(tests/golden/denoise_options*.npz, tools/make_golden_denoise_options.py; no normalised pixel of those inputs lies within 1e-5
of the cutoff, so no implementation can flip one).  Integer stack: the device path and the host loop agree to 1e-4 before the
truncating cast to the stack's dtype, so the cast moves a value by at most one integer."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_cpu_denoise_options import KEYS, load_fixture

pytestmark = pytest.mark.gpu
ATOL = 1e-4
CUTOFF, SIGMA, INV_SIGMA = 2.5, 1.2, 0.8
MIC = {name: os.path.join(GOLDEN, 'cli', name + '.mrc') for name in ('mic_a', 'mic_b')}


@functools.lru_cache(maxsize=None)
def fixture():
    return load_fixture()


@functools.lru_cache(maxsize=None)
def model(name):
    from topaz_amd.denoise import Denoise
    return Denoise(name)


@functools.lru_cache(maxsize=None)
def mic(name):
    from topaz_amd import mrc
    with open(MIC[name], 'rb') as f:
        a = mrc.parse(f.read())[0].astype(np.float32)
    a.flags.writeable = False
    return a


def _filters():
    from topaz_amd.filters import GaussianDenoise, InvGaussianFilter
    return GaussianDenoise(SIGMA), InvGaussianFilter(INV_SIGMA)


def _err(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max())


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x, dtype=np.float32)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
SIZES = [1, 63, 64, 65, 1027, 160 * 200, 2 ** 20 + 7]


def _specials(c):
    c32 = np.float32(c)
    up, down = np.nextafter(c32, np.float32(np.inf)), np.nextafter(c32, np.float32(0))
    return np.array([c32, -c32, up, -up, down, -down, np.nan, np.inf, -np.inf, 0.0, -0.0], dtype=np.float32)


def _mask(v, c):
    """the reference's cutoff (denoise.py:390-391) on a float32 array with a Python-float c"""
    v = v.copy()
    with np.errstate(invalid='ignore'):
        v[(v < -c) | (v > c)] = 0
    return v


@pytest.mark.parametrize('c', [1.5, 2.5, 0.1])
def test_normalize_cutoff_is_the_numpy_mask_of_normalize(gpu_ctx, c):
    from topaz_amd import runtime as rt
    rng = np.random.RandomState(int(c * 10))
    sp = _specials(c)
    for n in SIZES:
        for mu, std in [(0.0, 1.0), (3.75, 1.9), (5000.0, 70.7), (0.5, 0.0)]:
            x = (rng.randn(n) * 2 * (std or 1) + mu).astype(np.float32)
            # planted: the values that normalise to +-c and their float32 neighbours on both sides, NaN, +-inf (identity
            # statistics plant them exactly; the others plant the pixels nearest to them)
            k = min(n, len(sp))
            with np.errstate(invalid='ignore', over='ignore'):
                x[:k] = (sp[:k] * np.float32(std or 1) + np.float32(mu)).astype(np.float32)
            base = rt.normalize(_dev(x), mu, std).cpu().numpy()
            want = _mask(base, c)
            got = rt.normalize_cutoff(_dev(x), mu, std, c).cpu().numpy()
            assert got.dtype == np.float32 and got.shape == x.shape
            assert np.array_equal(_bits(got), _bits(want)), (n, mu, std, c, int((_bits(got) != _bits(want)).sum()))
            if (mu, std) == (0.0, 1.0) and n >= len(sp):
                # exactly on the cutoff stays, one float32 beyond goes, NaN passes, inf goes
                assert np.array_equal(got[:6], np.array([sp[0], sp[1], 0, 0, sp[4], sp[5]], np.float32))
                assert np.isnan(got[6]) and got[7] == 0 and got[8] == 0
            if std == 0.0 and n > 1:
                assert np.isnan(base).any() or np.isinf(base).any()          # the reference's inf / nan ...
                assert not np.isinf(got).any()                               # ... of which the cutoff zeroes the inf


@pytest.mark.parametrize('c', [0, -1])
def test_no_cutoff_is_normalize(gpu_ctx, c):
    import torch
    from topaz_amd import runtime as rt
    x = np.random.RandomState(7).randn(2 ** 20 + 7).astype(np.float32) * 3 + 10
    x[:11] = _specials(2.5)
    for n in (1, 65, 160 * 200, x.size):
        xd = _dev(x[:n])
        assert torch.equal(rt.normalize_cutoff(xd, 10.0, 3.0, c).view(torch.int32), rt.normalize(xd, 10.0, 3.0).view(torch.int32))


def test_normalize_cutoff_is_one_counted_launch(gpu_ctx):
    from topaz_amd import runtime as rt
    x = _dev(np.random.RandomState(8).randn(1027).astype(np.float32))
    gpu_ctx.prof_enable(1)
    gpu_ctx.prof_reset()
    rt.normalize_cutoff(x, 0.0, 1.0, 2.5)
    n = gpu_ctx.prof_get(2)[1]
    gpu_ctx.prof_enable(0)
    assert n == 1


# ---- denoise_image_device against the reference ---------------------------------------------------------------------------------
def _args(key):
    """denoise_image_device's keyword arguments for a fixture key"""
    gaus, inv = _filters()
    options, name = key.split(':')[0], key.split(':')[1]
    kw = dict(normalize=key.endswith(':norm'))
    for opt in options.split('+'):
        if opt.startswith('cutoff'):
            kw['cutoff'] = float(opt[len('cutoff'):])
        elif opt.startswith('gaus'):
            kw['gaus'] = gaus
        elif opt.startswith('invgaus'):
            kw['inv_gaus'] = inv
    return name, kw


@pytest.mark.parametrize('key', KEYS)
@pytest.mark.parametrize('name', ['mic_a', 'mic_b'])
def test_image_parity_with_the_reference(gpu_ctx, name, key):
    from topaz_amd.denoise import denoise_image_device
    net, kw = _args(key)
    got = denoise_image_device(_dev(mic(name)), [model(net)], -1, 0, **kw).cpu().numpy()
    ref = fixture()[f'{name}:{key}']
    print(f'{name} {key}: max|gpu - ref| {_err(got, ref):.3e} (bar {ATOL:.0e})')
    assert got.shape == ref.shape and got.dtype == np.float32 and _err(got, ref) <= ATOL


def test_image_parity_with_the_first_golden(gpu_ctx):
    """the two option cases tests/golden/denoise2d_pretrained.npz has held since the first round (there through the host path)"""
    from topaz_amd.denoise import denoise_image_device
    z = np.load(os.path.join(GOLDEN, 'denoise2d_pretrained.npz'))
    x = _dev(z['x'])
    got = denoise_image_device(x, [model('unet-small')], -1, 0, gaus=_filters()[0]).cpu().numpy()
    print(f'gaus1.2 unet-small: {_err(got, z["image:unet-small:gaus1.2"]):.3e}')
    assert _err(got, z['image:unet-small:gaus1.2']) <= ATOL
    got = denoise_image_device(x, [model('affine')], -1, 0, cutoff=1.5).cpu().numpy()
    print(f'cutoff1.5 affine: {_err(got, z["image:affine:cutoff"]):.3e}')
    assert _err(got, z['image:affine:cutoff']) <= ATOL


def test_filter_precedence(gpu_ctx):
    import torch
    from topaz_amd.denoise import denoise_image_device
    gaus, inv = _filters()
    x, d = _dev(mic('mic_a')), [model('unet-small')]
    only_gaus = denoise_image_device(x, d, -1, 0, gaus=gaus)
    assert torch.equal(denoise_image_device(x, d, -1, 0, gaus=gaus, inv_gaus=inv, deconvolve=True), only_gaus)
    only_inv = denoise_image_device(x, d, -1, 0, inv_gaus=inv)
    assert torch.equal(denoise_image_device(x, d, -1, 0, inv_gaus=inv, deconvolve=True), only_inv)
    assert not torch.equal(only_gaus, only_inv)
    assert not torch.equal(denoise_image_device(x, d, -1, 0, deconvolve=True), denoise_image_device(x, d, -1, 0))
    # a geometry deconv_tiles refuses matters only when the deconvolution is the branch that runs
    small = x[:10].contiguous()
    with pytest.raises(ValueError, match='smaller than the 11 x 11 filter'):
        denoise_image_device(small, [], deconvolve=True)
    for kw in (dict(gaus=gaus), dict(inv_gaus=inv), dict(gaus=gaus, inv_gaus=inv)):
        y = denoise_image_device(small, [], deconvolve=True, **kw)
        assert torch.equal(y, denoise_image_device(small, [], **kw)) and tuple(y.shape) == (10, 200)


# ---- the drivers take the device path -------------------------------------------------------------------------------------------
class _HostPath(Exception):
    pass


@pytest.fixture
def no_host_path(monkeypatch):
    import topaz_amd.denoise as dn

    def refuse(*a, **kw):
        raise _HostPath('denoise_image (the host path) was called')
    monkeypatch.setattr(dn, 'denoise_image', refuse)


def _write_stack(path, sections, dtype=np.float32, extended=b''):
    """an MRC stack in the mode of `dtype` (mrc.write itself only stores float32)"""
    from topaz_amd import mrc
    data = np.ascontiguousarray(np.stack(sections).astype(dtype))
    header = mrc.make_header(data.shape, (1, 1, 1), (90, 90, 90), dtype=dtype, exthd_size=len(extended))
    with open(path, 'wb') as f:
        f.write(mrc.header_struct.pack(*list(header)) + extended + data.tobytes())
    return data


def _read(path):
    from topaz_amd import mrc
    with open(path, 'rb') as f:
        return mrc.parse(f.read())


def test_stream_with_a_cutoff_or_a_gaussian_stays_on_the_device(gpu_ctx, tmp_path, no_host_path):
    from topaz_amd.denoise import denoise_stream
    d = [model('unet-small')]
    common = dict(models=d, deconvolve=False, patch_size=1024, padding=500, normalize=False)
    z = fixture()
    out = denoise_stream([MIC['mic_a'], MIC['mic_b']], str(tmp_path / 'c'), pixel_cutoff=CUTOFF, **common)
    for name, y in zip(('mic_a', 'mic_b'), out):
        print(f'stream cutoff {name}: {_err(y, z[f"{name}:cutoff2.5:unet-small"]):.3e}')
        assert _err(y, z[f'{name}:cutoff2.5:unet-small']) <= ATOL
        assert np.array_equal(_read(tmp_path / 'c' / f'{name}.mrc')[0], y)
    out = denoise_stream([MIC['mic_b']], str(tmp_path / 'g'), gaus=_filters()[0], **common)
    assert _err(out[0], z['mic_b:gaus1.2:unet-small']) <= ATOL
    out = denoise_stream([MIC['mic_a']], str(tmp_path / 'i'), inv_gaus=_filters()[1], **common)
    assert _err(out[0], z['mic_a:invgaus0.8:unet-small']) <= ATOL


@pytest.mark.parametrize('ring_min_bytes', [0, 1 << 30], ids=['ring', 'one-by-one'])
def test_stack_stays_on_the_device(gpu_ctx, tmp_path, no_host_path, monkeypatch, ring_min_bytes):
    """both ways a section can take on the device: through the ring (sections of RING_MIN_BYTES and more) and one by one"""
    import topaz_amd.denoise as dn
    from topaz_amd.denoise import denoise_stack
    assert 4 * 160 * 200 < dn.RING_MIN_BYTES <= 4 * 512 * 512
    monkeypatch.setattr(dn, 'RING_MIN_BYTES', ring_min_bytes)
    extended = bytes(range(96))
    _write_stack(tmp_path / 's.mrc', [mic('mic_a'), mic('mic_b')], extended=extended)
    out = denoise_stack(str(tmp_path / 's.mrc'), str(tmp_path / 'o.mrc'), [model('unet-small')], pixel_cutoff=CUTOFF,
                        gaus=_filters()[0], deconvolve=False, normalize=False)
    written, header, ext = _read(tmp_path / 'o.mrc')
    assert out.shape == (2, 160, 200) and out.dtype == np.float32 and np.array_equal(written, out)
    assert header.mode == 2 and (header.nz, header.ny, header.nx) == (2, 160, 200) and ext == extended
    assert os.path.getsize(tmp_path / 'o.mrc') == 1024 + 96 + 2 * 160 * 200 * 4
    for k, name in enumerate(('mic_a', 'mic_b')):                # its own micrograph's fixture: own statistics, no mix-up
        e = _err(out[k], fixture()[f'{name}:cutoff2.5+gaus1.2:unet-small'])
        print(f'stack section {k}: {e:.3e}')
        assert e <= ATOL


def test_host_path_is_kept_where_it_belongs(gpu_ctx, tmp_path, no_host_path):
    from topaz_amd.denoise import denoise_stack, denoise_stream

    class Model3D:
        dims = 3
    _write_stack(tmp_path / 's.mrc', [mic('mic_a'), mic('mic_b')])
    with pytest.raises(_HostPath):                               # `-m none`, no filter: the pass-through
        denoise_stream([MIC['mic_a']], str(tmp_path), models=[], deconvolve=False)
    with pytest.raises(_HostPath):
        denoise_stack(str(tmp_path / 's.mrc'), str(tmp_path / 'o.mrc'), [], deconvolve=False)
    with pytest.raises(_HostPath):                               # a 3-D model, whatever the options
        denoise_stream([MIC['mic_a']], str(tmp_path), models=[Model3D()], pixel_cutoff=CUTOFF, deconvolve=False)
    with pytest.raises(_HostPath):
        denoise_stack(str(tmp_path / 's.mrc'), str(tmp_path / 'o.mrc'), [Model3D()], gaus=_filters()[0], deconvolve=False)


# ---- the command line ------------------------------------------------------------------------------------------------------------
def _cli(args):
    r = subprocess.run([sys.executable, '-m', 'topaz_amd', 'denoise'] + [str(a) for a in args], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


OPTIONS = ['-m', 'unet-small', '--pixel-cutoff', CUTOFF, '--gaussian', SIGMA]


def test_cli_micrograph(gpu_ctx, tmp_path):
    _cli(OPTIONS + ['-o', tmp_path, MIC['mic_a']])
    got = _read(tmp_path / 'mic_a.mrc')[0]
    e = _err(got, fixture()['mic_a:cutoff2.5+gaus1.2:unet-small'])
    print(f'CLI --pixel-cutoff 2.5 --gaussian 1.2: {e:.3e}')
    assert got.shape == (160, 200) and e <= ATOL


def test_cli_float_stack(gpu_ctx, tmp_path):
    _write_stack(tmp_path / 's.mrc', [mic('mic_a'), mic('mic_b')])
    r = _cli(OPTIONS + ['--stack', '-o', tmp_path / 'o.mrc', tmp_path / 's.mrc'])
    assert 'stack sections [0, 1] of 2' in r.stderr
    got, header, _ = _read(tmp_path / 'o.mrc')
    assert got.shape == (2, 160, 200) and header.mode == 2
    for k, name in enumerate(('mic_a', 'mic_b')):
        e = _err(got[k], fixture()[f'{name}:cutoff2.5+gaus1.2:unet-small'])
        print(f'CLI --stack section {k}: {e:.3e}')
        assert e <= ATOL


def test_cli_int16_stack(gpu_ctx, tmp_path):
    """an integer stack keeps today's semantics: every section truncated to the stack's dtype, then stored as float32"""
    from topaz_amd.denoise import denoise_image
    stack = _write_stack(tmp_path / 's.mrc', [np.round(mic('mic_a') * 100), np.round(mic('mic_b') * 100)], dtype=np.int16)
    assert _read(tmp_path / 's.mrc')[1].mode == 1
    for section in stack:                                        # (precondition: no pixel sits on the cutoff)
        v = (section - section.mean()) / section.std()
        assert np.abs(np.abs(v) - CUTOFF).min() > 1e-5
    _cli(OPTIONS + ['--stack', '-o', tmp_path / 'o.mrc', tmp_path / 's.mrc'])
    got, header, _ = _read(tmp_path / 'o.mrc')
    assert header.mode == 2 and got.dtype == np.float32 and got.shape == stack.shape
    assert np.array_equal(got, np.trunc(got))                    # whole numbers: the cast to int16 happened
    host = np.zeros_like(stack)                                  # today's loop (denoise_stack's host branch) on the same input
    for k, section in enumerate(stack):
        host[k] = denoise_image(section, [model('unet-small')], cutoff=CUTOFF, gaus=_filters()[0], deconvolve=False,
                                patch_size=1024, padding=500, normalize=False)
    diff = np.abs(got.astype(np.int64) - host.astype(np.int64))
    print(f'int16 stack: {int((diff != 0).sum())} of {diff.size} values differ from the host loop, largest difference {diff.max()}')
    assert diff.max() <= 1
