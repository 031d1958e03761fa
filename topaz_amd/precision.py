"""The precision check of a loaded model: how far its 2xf16 result is from its own fp32 result, and what the commands do about it.

The default path multiplies 22-bit operands (csrc/conv_split.h); that it stays within the project's 1e-4 contract was measured on
the packaged and the seeded weights only.  A model the user trained is untested by construction, so `topaz extract`, `segment`,
`denoise` and `denoise3d` measure it once after loading (`--precision-check`): one seeded tile through the
model on both paths (DeviceModel.calibrate -> tpz_model_calibrate), and a model above the bar runs on the fp32 kernels from then on.

Nothing here runs implicitly: `cuda()`, `forward` and `Denoise.__init__` never calibrate.
"""
from __future__ import annotations

import sys
import warnings
from typing import Optional

import numpy as np

from . import runtime as rt

MODES = ('auto', 'always', 'never')
# the tile a check runs on when the caller supplies none: seeded standard-normal pixels
TILE_2D = (256, 256)
TILE_3D = (48, 48, 48)


def should_check(mode: str, model_arg) -> bool:
    """THE policy of `--precision-check`: `auto` checks a model given as a file (user-trained) and skips the pretrained aliases,
    which the project's own GPU tests pin, and 'none'; `always` checks the aliases too; `never` checks nothing."""
    if mode not in MODES:
        raise ValueError(f'--precision-check {mode!r}: expected one of {", ".join(MODES)}')
    if mode == 'never' or model_arg is None or model_arg == 'none' or not isinstance(model_arg, str):
        return False
    if mode == 'always':
        return True
    from .denoising.models import model_name_dict
    from .model.factory import _PRETRAINED
    return model_arg not in _PRETRAINED and model_arg not in model_name_dict


def default_tile(dims: int, seed: int = 0) -> np.ndarray:
    """the default calibration input: RandomState(seed).randn, 256 x 256 for 2-D programs, 48 x 48 x 48 for 3-D ones"""
    shape = TILE_3D if dims == 3 else TILE_2D
    return np.random.RandomState(seed).randn(*shape).astype(np.float32)


def calibrate(device_model: 'rt.DeviceModel', x=None, bar: Optional[float] = None, seed: int = 0) -> dict:
    """DeviceModel.calibrate on x ([H, W] / [D, H, W], or any layout forward takes) or, x None, on default_tile(dims, seed)"""
    if x is None:
        x = default_tile(device_model.dims, seed)
    if isinstance(x, np.ndarray):
        x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim == device_model.dims:
        x = x[None, None]
    return device_model.calibrate(x, bar)


def describe(r: dict) -> str:
    if not r['eligible']:
        return 'no 2xf16 path for this model: it runs on the fp32 kernels, nothing to compare'
    if r['overflow']:
        return 'the calibration tile left the f16 range (such images are re-run on the fp32 kernels): no comparison made'
    return (f'2xf16 against fp32 on the calibration tile: max |delta| {r["max_abs_delta"]:.3e} (rms {r["rms_delta"]:.3e}, '
            f'max |output| {r["max_abs_ref"]:.3e}), bar {r["bar"]:.1e}')


def check_loaded_model(model, mode: str, model_arg, verbose: bool = False, stream=None) -> Optional[dict]:
    """What a command does once per loaded model, after cuda() and before the first input: when should_check(mode, model_arg),
    model.calibrate() on the default tile, seed 0, at DEFAULT_BAR.  `verbose`: one line on stderr says what was measured.  A
    model above the bar is pinned to the fp32 kernels and a RuntimeWarning says so whatever the verbosity; a calibration tile
    that left the f16 range prints one line and changes nothing.  Under --gpus every rank checks for itself: same seed, same
    arithmetic, the same decision.  Returns the measurement (None when nothing was checked)."""
    if not should_check(mode, model_arg):
        return None
    stream = stream or sys.stderr
    r = model.calibrate(bar=rt.DEFAULT_BAR, seed=0)
    if r['eligible'] and r['overflow']:
        print(f'# precision check of {model_arg}: {describe(r)}', file=stream)
    elif verbose:
        print(f'# precision check of {model_arg}: {describe(r)}', file=stream)
    if r['tripped']:
        warnings.warn(f'topaz_amd: the 2xf16 path is {r["max_abs_delta"]:.3e} away from the fp32 result of {model_arg} on the '
                      f'calibration tile, above the bar of {r["bar"]:.1e}: this model runs on the fp32 matrix-core kernels, several '
                      f'times slower (--precision-check never skips the check)', RuntimeWarning, stacklevel=2)
    return r
