"""Stored MRC pixel types without a GPU: `mrc.read_stored_into` keeps the bytes of the file in the dtype of the file, `read_into`
decodes what it always decoded, and the two entry points behind the device decode are declared in every place a symbol of the
C ABI is declared in."""
import ctypes as C
import fnmatch
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from topaz_amd import mrc

MODES = {0: np.int8, 1: np.int16, 2: np.float32, 6: np.uint16, 12: np.float16}


def _pixels(mode, shape, seed=0):
    """values that use the whole range of the type (uint16 above 32 767, negative integers, float16 subnormals and -0.0)"""
    dt = np.dtype(MODES[mode])
    rs = np.random.RandomState(seed + mode)
    n = int(np.prod(shape))
    if dt.kind in 'iu':
        info = np.iinfo(dt)
        x = rs.randint(info.min, info.max + 1, n).astype(dt)
        x[:2] = (info.min, info.max)
    elif dt == np.float16:
        x = rs.randint(0, 1 << 16, n).astype(np.uint16)
        x[(x & 0x7c00) == 0x7c00] &= 0x83ff                       # no inf / nan here: the comparisons below are on values too
        x[:4] = (0x0001, 0x8000, 0x03ff, 0x7bff)                  # smallest subnormal, -0.0, largest subnormal, largest normal
        x = x.view(np.float16)
    else:
        x = rs.randn(n).astype(np.float32)
    return x.reshape(shape)


def write_stored(path, x, extended=b''):
    """an MRC file that holds x in x's own dtype (mrc.write always stores float32)"""
    x = np.ascontiguousarray(x)
    mode = {np.dtype(v): k for k, v in MODES.items()}[x.dtype]
    shape = x.shape if x.ndim == 3 else (1,) + x.shape
    header = mrc.make_header(shape, (1, 1, 1), (0, 0, 0), exthd_size=len(extended))._replace(mode=mode)
    with open(path, 'wb') as f:
        f.write(mrc.header_struct.pack(*list(header)))
        f.write(extended)
        f.write(x.tobytes())
    return str(path)


def _alloc(calls):
    def alloc(shape, dtype=np.float32):
        calls.append((tuple(shape), np.dtype(dtype)))
        return np.full(shape, 77, dtype=dtype)
    return alloc


@pytest.mark.parametrize('shape', [(5, 3), (2, 7, 9)])
@pytest.mark.parametrize('mode', [0, 1, 6, 12])
def test_read_stored_into_keeps_dtype_and_bytes(tmp_path, mode, shape):
    x = _pixels(mode, shape)
    path = write_stored(tmp_path / 'x.mrc', x, extended=b'abcdefgh')
    calls = []
    got, header, extended = mrc.read_stored_into(path, _alloc(calls))
    assert calls == [(shape, np.dtype(MODES[mode]))]
    assert got.dtype == np.dtype(MODES[mode]) and got.shape == shape
    assert got.tobytes() == x.tobytes()
    assert header.mode == mode and extended == b'abcdefgh'
    assert (header.nx, header.ny, header.nz) == (shape[-1], shape[-2], shape[0] if len(shape) == 3 else 1)


def test_read_stored_into_float32_is_read_into(tmp_path):
    x = _pixels(2, (6, 11))
    path = write_stored(tmp_path / 'x.mrc', x)
    a, ha, ea = mrc.read_stored_into(path, _alloc([]))
    b, hb, eb = mrc.read_into(path, lambda shape: np.empty(shape, dtype=np.float32))
    assert a.dtype == b.dtype == np.float32 and a.tobytes() == b.tobytes() == x.tobytes()
    assert ha == hb and ea == eb


@pytest.mark.parametrize('mode,dtype,per_pixel', [(3, np.int16, 2), (4, np.complex64, 1), (16, np.uint8, 3)])
def test_vector_modes_return_none(tmp_path, mode, dtype, per_pixel):
    header = mrc.make_header((1, 4, 5), (1, 1, 1), (0, 0, 0))._replace(mode=mode)
    path = tmp_path / 'v.mrc'
    with open(path, 'wb') as f:
        f.write(mrc.header_struct.pack(*list(header)))
        f.write(np.zeros(4 * 5 * per_pixel, dtype=dtype).tobytes())
    calls = []
    assert mrc.read_stored_into(str(path), _alloc(calls)) is None and calls == []
    assert mrc.read_into(str(path), _alloc(calls)) is None


@pytest.mark.parametrize('mode', [0, 1, 2, 6, 12])
def test_truncated_file_raises_value_error(tmp_path, mode):
    x = _pixels(mode, (8, 8))
    path = write_stored(tmp_path / 'x.mrc', x)
    whole = open(path, 'rb').read()
    with open(path, 'wb') as f:
        f.write(whole[:-2 * x.dtype.itemsize])
    with pytest.raises(ValueError):
        mrc.read_stored_into(path, _alloc([]))
    with pytest.raises(ValueError):
        mrc.read_into(path, lambda shape: np.empty(shape, dtype=np.float32))


@pytest.mark.parametrize('mode', [0, 1, 2, 6, 12])
def test_read_into_is_unchanged(tmp_path, mode):
    x = _pixels(mode, (9, 13))
    path = write_stored(tmp_path / 'x.mrc', x)
    got, header, extended = mrc.read_into(path, lambda shape: np.empty(shape, dtype=np.float32))
    want, hp, ep = mrc.parse(open(path, 'rb').read())
    assert got.dtype == np.float32 and got.shape == (9, 13)
    assert got.tobytes() == want.astype(np.float32).tobytes()
    assert header == hp and extended == ep == b''


def test_stored_modes_are_the_four_native_types():
    assert mrc.STORED_MODES == {np.dtype(np.int8): 0, np.dtype(np.int16): 1, np.dtype(np.uint16): 6, np.dtype(np.float16): 12}
    assert np.dtype('>i2') not in mrc.STORED_MODES and np.dtype(np.float32) not in mrc.STORED_MODES


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
PROTOTYPES = {
    'tpz_decode': 'int tpz_decode(tpz_ctx* ctx, const void* d_raw, int mrc_mode, size_t n, float* d_out);',
    'tpz_stage_h2d_decode': 'int tpz_stage_h2d_decode(tpz_stage* st, int slot, int mrc_mode, size_t n);',
    'tpz_stage_decode_bytes': 'size_t tpz_stage_decode_bytes(int mrc_mode, size_t n);',
}


@pytest.mark.parametrize('name', sorted(PROTOTYPES))
def test_symbols_are_declared_everywhere(name):
    from topaz_amd import _lib
    assert name in _lib.EXPORTED_SYMBOLS and name in _lib._SIGNATURES
    assert PROTOTYPES[name] in open(os.path.join(ROOT, 'include', 'topaz_hip.h')).read()
    restype, argtypes = _lib._SIGNATURES[name]
    assert len(argtypes) == PROTOTYPES[name].count(',') + 1
    # the version script exports by pattern: the name must match a global pattern of it
    text = open(os.path.join(ROOT, 'topaz_amd', 'csrc', 'libtopaz_hip.map')).read()
    globs = re.search(r'global:(.*?)local:', text, re.S).group(1).replace(';', ' ').split()
    assert any(fnmatch.fnmatchcase(name, g) for g in globs), globs
    assert name in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


def test_null_arguments_are_refused():
    from topaz_amd import _lib
    lib = _lib.load_library()
    buf = (C.c_char * 64)()
    assert lib.tpz_decode(None, None, 1, 8, None) != 0
    assert lib.tpz_decode(None, C.addressof(buf), 1, 8, C.addressof(buf)) != 0            # no context
    assert lib.tpz_stage_h2d_decode(None, 0, 1, 8) != 0
    # the slot layout: the fp32 image, then the stored pixels at the next multiple of 256 bytes, the whole a multiple of 256
    assert lib.tpz_stage_decode_bytes(1, 100) == 512 + 256 and lib.tpz_stage_decode_bytes(0, 64) == 256 + 256
    assert lib.tpz_stage_decode_bytes(12, 4096 * 4096) == 4096 * 4096 * 6 and lib.tpz_stage_decode_bytes(6, 0) == 0
    assert lib.tpz_stage_decode_bytes(2, 100) == 0 and lib.tpz_stage_decode_bytes(3, 100) == 0
