"""`topaz extract --preprocess` without a GPU: the flag surface, the argument checks that run before anything is loaded, the
place the callable takes in the scoring loop, and the C-ABI of the resampler behind it."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

PREPROCESS_DEFAULTS = dict(preprocess=0, preprocess_affine=False, preprocess_sample=10, preprocess_niters=100,
                           preprocess_alpha=900, preprocess_beta=1)


def test_preprocess_flags_parse_with_the_defaults_of_normalize():
    from topaz_amd.commands import extract, normalize
    a = extract.add_arguments().parse_args(['-r', '14', '-x', '8', '-o', 'out.txt', 'a.mrc', 'b.mrc'])
    # the assertions of test_cli_flag_surface_and_defaults still hold: the new flags are additive
    assert (a.model, a.threshold, a.device, a.format, a.dims, a.radius, a.up_scale, a.down_scale, a.patch_size) == \
        ('resnet16', -6, 0, 'coord', 2, 14, 8.0, 1, 0)
    assert a.paths == ['a.mrc', 'b.mrc'] and not a.per_micrograph and a.num_workers == 0
    for key, value in PREPROCESS_DEFAULTS.items():
        assert getattr(a, key) == value, key
    # ... and are the defaults `topaz normalize` / `topaz preprocess` have for the same quantities
    n = normalize.add_arguments().parse_args(['x.mrc'])
    assert (a.preprocess_affine, a.preprocess_sample, a.preprocess_niters, a.preprocess_alpha, a.preprocess_beta) == \
        (n.affine, n.sample, n.niters, n.alpha, n.beta)
    b = extract.add_arguments().parse_args(['--preprocess', '4', '--preprocess-affine', '--preprocess-sample', '1',
                                            '--preprocess-niters', '7', '--preprocess-alpha', '2.5', '--preprocess-beta', '3',
                                            '-r', '9', 'a.mrc'])
    assert (b.preprocess, b.preprocess_affine, b.preprocess_sample, b.preprocess_niters, b.preprocess_alpha, b.preprocess_beta) == \
        (4, True, 1, 7, 2.5, 3.0)
    assert 'frame of the scored' in extract.add_arguments().format_help()       # the help says where the picks live


@pytest.mark.parametrize('extra', [['--dims', '3'], ['-m', 'none']])
def test_preprocess_with_dims3_or_no_model_raises_before_anything_is_loaded(monkeypatch, extra):
    from topaz_amd import extract as ex
    from topaz_amd.commands import extract as cmd

    def boom(*a, **k):
        raise AssertionError('nothing may be loaded before the arguments are checked')

    for name in ('load_model', 'Scorer', 'ImageFeed', 'load_image'):
        monkeypatch.setattr(ex, name, boom)
    args = cmd.add_arguments().parse_args(['--preprocess', '2', '-r', '8', 'a.mrc'] + extra)
    with pytest.raises(ValueError, match='--preprocess'):
        cmd.main(args)
    # the library entry refuses the same combinations, whatever the callable
    kw = dict(paths=['a.mrc'], device=0, batch_size=1, threshold=-6, radius=8, num_workers=0, targets=None, min_radius=5,
              max_radius=100, step=5, match_radius=None, patch_size=0, only_validate=False, output=None, per_micrograph=False,
              suffix='', out_format='coord', up_scale=1, down_scale=1)
    with pytest.raises(ValueError, match='--preprocess'):
        ex.extract_particles(model='none' if extra[0] == '-m' else 'resnet8_u32', dims=3 if extra[0] == '--dims' else 2,
                             preprocess=lambda x: x, **kw)
    with pytest.raises(ValueError):
        cmd.main(cmd.add_arguments().parse_args(['--preprocess', '-1', '-r', '8', 'a.mrc']))


def test_callable_is_applied_once_per_image_in_path_order_before_scoring(monkeypatch):
    from topaz_amd import extract as ex
    events = []
    paths = [f'mic_{i}.mrc' for i in (3, 1, 2, 0)]

    class FakeFeed:
        def __init__(self, paths, ctx, headers=False):
            self.paths = list(paths)

        def __iter__(self):
            for i, p in enumerate(self.paths):
                events.append(('feed', p))
                yield p, torch.full((4, 4), float(i))

    class FakeScorer:
        ctx = object()

        def __init__(self, model, device, precision_check, verbose):
            events.append(('load', model))

        def __call__(self, image, patch_size=0):
            events.append(('score', float(image[0, 0])))
            return image * 2

    def preprocess(x):
        events.append(('preprocess', float(x[0, 0])))
        return x + 100

    monkeypatch.setattr(ex, 'ImageFeed', FakeFeed)
    monkeypatch.setattr(ex, 'Scorer', FakeScorer)
    out = list(ex.score_images('resnet8_u32', paths, preprocess=preprocess))
    assert [p for p, _ in out] == paths
    assert [float(s[0, 0]) for _, s in out] == [200.0, 202.0, 204.0, 206.0]          # scored AFTER the callable
    want = [('load', 'resnet8_u32')]
    for i, p in enumerate(paths):
        want += [('feed', p), ('preprocess', float(i)), ('score', 100.0 + i)]
    assert events == want
    # without the callable nothing changes
    events.clear()
    out = list(ex.score_images('resnet8_u32', paths[:1]))
    assert float(out[0][1][0, 0]) == 0.0 and ('preprocess', 0.0) not in events
    with pytest.raises(ValueError):
        list(ex.score_images('none', paths, preprocess=preprocess))


def test_device_preprocess_goes_through_downsample_then_normalize(monkeypatch):
    from topaz_amd import stats as tstats
    from topaz_amd.utils import image as im
    calls = []
    monkeypatch.setattr(im, 'downsample_device', lambda x, s: calls.append(('down', s)) or x[::s, ::s])
    monkeypatch.setattr(tstats, 'normalize_device', lambda x, **kw: (calls.append(('norm', tuple(x.shape), kw)) or x - 1, {'mu': 1}))
    p = tstats.DevicePreprocess(2, True, 7, 2.5, 3, 1)
    y = p(torch.ones(6, 8))
    assert tuple(y.shape) == (3, 4) and p.last_meta == {'mu': 1}
    assert calls == [('down', 2), ('norm', (3, 4), dict(alpha=2.5, beta=3, num_iters=7, sample=1, method='affine'))]
    calls.clear()
    tstats.DevicePreprocess(1)(torch.ones(6, 8))                                       # scale 1: normalise only, NORMALIZE's defaults
    assert calls == [('norm', (6, 8), dict(alpha=900, beta=1, num_iters=100, sample=10, method='gmm'))]
    with pytest.raises(ValueError):
        tstats.DevicePreprocess(0)
    with pytest.raises(NotImplementedError):
        tstats.DevicePreprocess(2)(torch.ones(2, 6, 8))


RESAMPLE_ABI = ('tpz_resample_create', 'tpz_resample_run', 'tpz_resample_free', 'tpz_resample_shape', 'tpz_resample_2d_host',
                'tpz_resample_upload_bytes')


def test_header_declares_and_library_exports_the_resampler():
    from topaz_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'topaz_hip.h')).read()
    declared = set(re.findall(r'\b(tpz_[a-z0-9_]+)\s*\(', header))
    lib = C.CDLL(_lib.LIB_PATH)                       # raw dlopen: no GPU needed
    for name in RESAMPLE_ABI:
        assert name in declared, f'{name} not declared in include/topaz_hip.h'
        assert name in _lib.EXPORTED_SYMBOLS, f'{name} has no ctypes prototype'
        assert hasattr(lib, name), f'{name} not exported by libtopaz_hip.so'
    # without a context the entry points fail cleanly (an error code and a message), they do not crash
    lib.tpz_resample_create.restype = C.c_int
    lib.tpz_last_error.restype = C.c_char_p
    out = C.c_void_p()
    one = (C.c_float * 4)(1, 0, 0, 1)
    assert lib.tpz_resample_create(None, 2, 2, 1, 1, one, one, C.byref(out)) != 0 and not out.value
    assert b'tpz_resample_create' in lib.tpz_last_error(None)
    lib.tpz_resample_run.restype = C.c_int
    assert lib.tpz_resample_run(None, None, None) != 0
    lib.tpz_resample_free(None)
    lib.tpz_resample_upload_bytes.restype = C.c_longlong
    assert lib.tpz_resample_upload_bytes(None) == 0


def test_operator_cache_and_plan_cache_are_keyed_by_shape():
    from topaz_amd.utils import image as im
    L, R = im._downsample_operators(10, 12, 5, 4)
    assert L.shape == (10, 10) and R.shape == (4, 24) and L.dtype == R.dtype == np.float32
    assert im._downsample_operators(10, 12, 5, 4)[0] is L
    assert im._PLAN_CACHE_MAX >= 2
