"""The host side of the precision check (`--precision-check`, tpz_model_calibrate): the flag on the four commands, the one
policy function, and the C-ABI declarations kept in step between the header and the ctypes table."""
import os
import re

import pytest

from conftest import ROOT

NEW_SYMBOLS = ('tpz_delta_stats', 'tpz_model_calibrate', 'tpz_model_set_exact', 'tpz_model_get_exact')


def _parsers():
    from topaz_amd.commands import denoise, denoise3d, extract, segment
    return {'extract': (extract, ['-r', '8', 'mic.mrc']), 'segment': (segment, ['mic.mrc']),
            'denoise': (denoise, ['mic.mrc']), 'denoise3d': (denoise3d, ['tomo.mrc'])}


@pytest.mark.parametrize('command', ['extract', 'segment', 'denoise', 'denoise3d'])
def test_precision_check_flag(command):
    module, argv = _parsers()[command]
    parser = module.add_arguments()
    assert parser.parse_args(argv).precision_check == 'auto'
    for mode in ('auto', 'always', 'never'):
        assert parser.parse_args(argv + ['--precision-check', mode]).precision_check == mode
    with pytest.raises(SystemExit):
        parser.parse_args(argv + ['--precision-check', 'sometimes'])


def test_should_check_policy():
    from topaz_amd.precision import should_check
    files = ('model_epoch10.sav', '/data/run3/unet_custom.sav', 'saved_models/resnet8_u32.sav')
    aliases = ('resnet8_u32', 'resnet16_u32', 'resnet16', 'resnet8', 'unet', 'unet-small', 'fcnn', 'affine', 'unet-v0.2.1',
               'unet-3d', 'unet-3d-10a', 'unet-3d-20a')
    for f in files:
        assert should_check('auto', f) and should_check('always', f) and not should_check('never', f)
    for a in aliases:
        assert not should_check('auto', a) and should_check('always', a) and not should_check('never', a)
    for mode in ('auto', 'always', 'never'):
        assert not should_check(mode, 'none') and not should_check(mode, None)
    with pytest.raises(ValueError):
        should_check('sometimes', 'model.sav')


def test_default_bar_is_the_parity_contract_in_one_place():
    from topaz_amd import precision, runtime
    assert runtime.DEFAULT_BAR == 1e-4
    assert not hasattr(precision, 'DEFAULT_BAR')          # read from runtime when a check runs, not copied at import


def test_default_tile_is_seeded_and_sized():
    import numpy as np
    from topaz_amd.precision import default_tile
    a, b = default_tile(2), default_tile(3)
    assert a.shape == (256, 256) and b.shape == (48, 48, 48) and a.dtype == b.dtype == np.float32
    assert np.array_equal(a, np.random.RandomState(0).randn(256, 256).astype(np.float32))
    assert not np.array_equal(a, default_tile(2, seed=1))


def test_header_and_ctypes_table_declare_the_new_entry_points():
    from topaz_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'topaz_hip.h')).read()
    declared = set(re.findall(r'\bint\s+(tpz_[a-z0-9_]+)\s*\(', header))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.EXPORTED_SYMBOLS, name
    assert 'typedef struct tpz_delta {' in header and 'typedef struct tpz_calibration {' in header
    # the ctypes mirrors have the header's layout: float, float, long long, double / three ints, the delta, a double
    import ctypes as C
    assert C.sizeof(_lib.TpzDelta) == 24 and _lib.TpzDelta.argmax.offset == 8 and _lib.TpzDelta.sum_sq.offset == 16
    assert C.sizeof(_lib.TpzCalibration) == 48 and _lib.TpzCalibration.d.offset == 16 and _lib.TpzCalibration.rms_delta.offset == 40


def test_calibrate_needs_the_filled_network():
    from topaz_amd.model.classifier import LinearClassifier
    from topaz_amd.model.factory import load_state_dict_from_pkg
    model = LinearClassifier('resnet8', load_state_dict_from_pkg('resnet8_u32.sav'))
    with pytest.raises(NotImplementedError):
        model.calibrate()
