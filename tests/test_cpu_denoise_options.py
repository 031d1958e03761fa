"""Host side of the device-resident denoise options: the flag surface, the byte layout of a stack written
section by section, the sharding of the sections, the eligibility predicate and the new C-ABI symbol.  No GPU needed."""
import io
import os

import numpy as np
import pytest

from conftest import GOLDEN

FIXTURES = [os.path.join(GOLDEN, 'denoise_options.npz'), os.path.join(GOLDEN, 'denoise_options_mic_b.npz')]
KEYS = ['cutoff2.5:affine', 'cutoff2.5:unet-small', 'gaus1.2:unet-small', 'cutoff2.5+gaus1.2:unet-small',
        'cutoff2.5+gaus1.2:unet-small:norm', 'invgaus0.8:unet-small']


def load_fixture():
    """the two fixture files (one per micrograph: twelve float32 images exceed the size limit of one file) as one dict"""
    out = {}
    for path in FIXTURES:
        z = np.load(path, allow_pickle=False)
        out.update({k: z[k] for k in z.files if k != 'meta'})
    return out


# (option strings, default) of the inference flags of the reference's `topaz denoise` (commands/denoise.py:23-69, v0.3.18)
REFERENCE_FLAGS = [
    (('-d', '--device'), 0), (('-o', '--output'), ''), (('--suffix',), ''), (('--format',), 'mrc'), (('--normalize',), False),
    (('--stack',), False), (('--save-prefix',), None), (('--save-interval',), 10), (('-m', '--model'), ['unet']),
    (('-a', '--dir-a'), None), (('-b', '--dir-b'), None), (('--hdf',), None), (('--preload',), False), (('--holdout',), 0.1),
    (('--lowpass',), 1), (('--gaussian',), 0), (('--inv-gaussian',), 0), (('--deconvolve',), False), (('--deconv-patch',), 1),
    (('--pixel-cutoff',), 0), (('-s', '--patch-size'), 1024), (('-p', '--patch-padding'), 500), (('--method',), 'noise2noise'),
    (('--arch',), 'unet'), (('--optim',), 'adagrad'), (('--lr',), 0.001), (('--criteria',), 'L2'), (('-c', '--crop'), 800),
    (('--batch-size',), 4), (('--num-epochs',), 100), (('--num-workers',), 16), (('-j', '--num-threads'), 0),
]


def test_parser_mirrors_the_reference_flags():
    from topaz_amd.commands import denoise
    parser = denoise.add_arguments()
    actions = {tuple(a.option_strings): a for a in parser._actions if a.option_strings}
    for strings, default in REFERENCE_FLAGS:
        assert strings in actions, strings
        assert actions[strings].default == default and type(actions[strings].default) is type(default), strings
    a = parser.parse_args(['--pixel-cutoff', '2.5', '--gaussian', '1.2', '--inv-gaussian', '0.8', '--stack', 'x.mrc'])
    assert (a.pixel_cutoff, a.gaussian, a.inv_gaussian, a.stack, a.micrographs, a.format_) == (2.5, 1.2, 0.8, True, ['x.mrc'], 'mrc')
    assert isinstance(a.pixel_cutoff, float) and isinstance(a.gaussian, float) and isinstance(a.inv_gaussian, float)


def test_stack_section_offsets_are_the_layout_of_mrc_write():
    """a stack assembled with pwrite at stack_section_offset equals what mrc.write gives, with a non-empty extended header"""
    from topaz_amd import mrc
    from topaz_amd.denoise import stack_section_offset
    nz, ny, nx = 5, 7, 9
    ext = bytes(range(200)) + b'\x01' * 24
    data = np.random.RandomState(5).randn(nz, ny, nx).astype(np.float32)
    header = mrc.make_header(data.shape, (1, 1, 1), (90, 90, 90), exthd_size=len(ext), dtype=np.int16)
    want = io.BytesIO()
    mrc.write(want, data, header=header, extended_header=ext)
    want = want.getvalue()
    assert stack_section_offset(0, ny, nx, len(ext)) == 1024 + 224
    assert stack_section_offset(3, ny, nx, len(ext)) == 1024 + 224 + 3 * 7 * 9 * 4
    assert stack_section_offset(nz, ny, nx, len(ext)) == len(want)
    assert stack_section_offset(2, ny, nx, 0) == 1024 + 2 * 7 * 9 * 4
    got = bytearray(len(want))
    got[:1024 + len(ext)] = mrc.header_struct.pack(*list(header._replace(mode=2))) + ext
    for k in (4, 1, 3, 0, 2):                                                # any order: the ranks do not wait for each other
        at = stack_section_offset(k, ny, nx, len(ext))
        got[at:at + ny * nx * 4] = data[k].tobytes()
    assert bytes(got) == want
    parsed, h, e = mrc.parse(bytes(got))
    assert h.mode == 2 and e == ext and np.array_equal(parsed, data)


@pytest.mark.parametrize('nz,world', [(1, 2), (1, 8), (3, 8), (2, 2), (8, 8), (3, 2), (17, 4), (512, 8)])
def test_sections_are_dealt_once_each(nz, world):
    from topaz_amd.parallel import shard_indices
    shares = [shard_indices(nz, r, world) for r in range(world)]
    assert sorted(k for s in shares for k in s) == list(range(nz))
    assert all(s == sorted(s) and all(k % world == r for k in s) for r, s in enumerate(shares))
    assert sum(1 for s in shares if not s) == max(0, world - nz)             # nz < N: the other ranks idle
    assert max(len(s) for s in shares) - min(len(s) for s in shares) <= 1
    assert shard_indices(3, 0, 2) == [0, 2] and shard_indices(3, 1, 2) == [1]


class _Model:
    def __init__(self, dims):
        self.dims = dims


def test_eligibility_predicate():
    from topaz_amd.denoise import runs_on_device
    m2, m3, g = _Model(2), _Model(3), object()
    # something to do, every model 2-D
    assert runs_on_device([m2])
    assert runs_on_device([m2, m2], pixel_cutoff=3, gaus=g, inv_gaus=g, deconvolve=True, lowpass=2)
    assert runs_on_device([], pixel_cutoff=2.5)
    assert runs_on_device([], gaus=g)
    assert runs_on_device([], inv_gaus=g)
    assert runs_on_device([], lowpass=2)
    assert runs_on_device([], deconvolve=True)
    # `-m none` and no filter: the host pass-through
    assert not runs_on_device([])
    assert not runs_on_device([], lowpass=1, pixel_cutoff=0, gaus=None, inv_gaus=None, deconvolve=False)
    assert not runs_on_device([], pixel_cutoff=-1) and not runs_on_device([], lowpass=0.5)
    # a 3-D model keeps the host loop whatever else is asked
    assert not runs_on_device([m3]) and not runs_on_device([m2, m3], pixel_cutoff=3, gaus=g)
    assert runs_on_device([m2], pixel_cutoff=3) is True and runs_on_device([]) is False


def test_signatures_keep_their_defaults_and_gain_the_options():
    import inspect
    from topaz_amd.denoise import denoise_image_device, denoise_stack
    p = inspect.signature(denoise_image_device).parameters
    assert (p['cutoff'].default, p['gaus'].default, p['inv_gaus'].default) == (0, None, None)
    assert list(p)[:8] == ['x', 'models', 'patch_size', 'padding', 'normalize', 'lowpass', 'deconvolve', 'deconv_patch']
    s = inspect.signature(denoise_stack).parameters
    assert list(s) == ['path', 'output_path', 'models', 'lowpass', 'pixel_cutoff', 'gaus', 'inv_gaus', 'deconvolve',
                       'deconv_patch', 'patch_size', 'padding', 'normalize', 'use_cuda']


def test_new_symbol_is_declared_and_prototyped():
    from topaz_amd import _lib
    from conftest import ROOT
    assert 'tpz_normalize_cutoff' in _lib.EXPORTED_SYMBOLS
    header = open(os.path.join(ROOT, 'include', 'topaz_hip.h')).read()
    assert 'int tpz_normalize_cutoff(tpz_ctx* ctx, const float* d_x, size_t n, float mean, float std, float cutoff, float* d_y);' \
        in header
    restype, argtypes = _lib._SIGNATURES['tpz_normalize_cutoff']
    assert len(argtypes) == 7
    assert 'tpz_normalize_cutoff' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


def test_fixture_holds_every_case_with_a_safe_margin():
    z = load_fixture()
    for mic in ('mic_a', 'mic_b'):
        for key in KEYS:
            assert z[f'{mic}:{key}'].shape == (160, 200) and z[f'{mic}:{key}'].dtype == np.float32
        assert float(z[f'{mic}:margin']) > 1e-5                              # no normalised pixel sits on the cutoff
    for path in FIXTURES:
        assert os.path.getsize(path) < 1 << 20
