"""tpz_tile_cut / tpz_tile_flags / tpz_tile_paste bit for bit against numpy: windows that start before the tensor,
reach past it or miss it, tile sizes whose rows are aligned, unaligned and shorter than a 16-byte group, pointers one float off
a 16-byte boundary, sentinels around every destination, and every refused argument."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = np.uint32(0xDEADBEEF)
GUARD = 64                                             # words of sentinel on either side of a destination
SHAPES = [(7, 9), (33, 70), (5, 7, 9)]
SIZES = [1, 4, 37]
NAN, NEG_ZERO = np.uint32(0x7fc00001), np.uint32(0x80000000)


def _bits(shape, seed):
    """random fp32 bit patterns with NaNs (quiet and signalling, both signs), +-inf, -0.0, +0.0 and subnormals among them"""
    rs = np.random.RandomState(seed)
    x = rs.randint(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)
    flat = x.reshape(-1)
    special = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0xff923456, 0x7f800000, 0xff800000, 0x80000000, 0x00000000,
                        0x00000001, 0x807fffff, 0x00400000], dtype=np.uint32)
    where = rs.choice(flat.size, size=min(flat.size, 3 * len(special)), replace=False)
    flat[where] = np.resize(special, len(where))
    return x


def _dev(words, offset):
    """device copy of uint32 words behind `offset` floats of slack: (the int32 tensor that owns them, pointer to the words)"""
    words = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
    buf = np.concatenate([np.full(4 + offset, SENTINEL, np.uint32), words])        # (4 + offset: the allocation is 16-byte aligned)
    t = torch.from_numpy(buf.view(np.int32)).cuda()
    return t, t.data_ptr() + 4 * (4 + offset)


def _guarded(n_words, offset, fill=SENTINEL, itemsize=4):
    """a destination of n_words elements between GUARD words of sentinel, `offset` elements off a 16-byte boundary"""
    dt = np.uint32 if itemsize == 4 else np.uint64
    total = GUARD + 4 + offset + n_words + GUARD
    t = torch.from_numpy(np.full(total, fill, dt).view(np.int32 if itemsize == 4 else np.int64)).cuda()
    lo = GUARD + 4 + offset
    return t, t.data_ptr() + itemsize * lo, lo


def _read(t, lo, n, itemsize=4):
    a = t.cpu().numpy().view(np.uint32 if itemsize == 4 else np.uint64)
    return a[lo:lo + n], a[:lo], a[lo + n:]


def _dhw(shape):
    return (1,) + tuple(shape) if len(shape) == 2 else tuple(shape)


def _zyx(v, fill):
    return (fill,) + tuple(v) if len(v) == 2 else tuple(v)


def _window_of(x, origin, extent):
    out = np.zeros(extent, dtype=x.dtype)
    src, dst = [], []
    for o, e, n in zip(origin, extent, x.shape):
        lo, hi = max(o, 0), min(o + e, n)
        if lo >= hi:
            return out
        src.append(slice(lo, hi))
        dst.append(slice(lo - o, hi - o))
    out[tuple(dst)] = x[tuple(src)]
    return out


def _origins(shape, size):
    """per axis: -3, 0, the far edge minus 1, wholly outside"""
    return list(itertools.product(*[(-3, 0, n - 1, n + 2) for n in shape]))


def _err(ctx):
    return (ctx.lib.tpz_last_error(ctx.handle) or b'').decode()


@pytest.mark.parametrize('offset', [0, 1], ids=['aligned', 'one_float_off'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_cut_against_numpy(gpu_ctx, shape, offset):
    ctx = gpu_ctx
    x = _bits(shape, 11 + len(shape))
    keep, src = _dev(x, offset)
    D, H, W = _dhw(shape)
    checked = zero_tiles = 0
    for size in SIZES:
        extent = (size,) * len(shape)
        n = size ** len(shape)
        for origin in _origins(shape, size):
            for dst_offset in ((0, 3) if size == 4 else (offset,)):
                out, dst, lo = _guarded(n, dst_offset)
                rc = ctx.lib.tpz_tile_cut(ctx.handle, C.c_void_p(src), D, H, W, *_zyx(origin, 0), *_zyx(extent, 1), C.c_void_p(dst))
                assert rc == 0, _err(ctx)
                torch.cuda.synchronize()
                got, front, back = _read(out, lo, n)
                want = _window_of(x, origin, extent)
                assert np.array_equal(got.reshape(extent), want), (size, origin)
                assert (front == SENTINEL).all() and (back == SENTINEL).all(), (size, origin)
                checked += 1
                zero_tiles += int(not want.any())
    assert checked >= 3 * 4 ** len(shape) and zero_tiles >= len(shape)               # (windows wholly outside: all-zero tiles)
    del keep


@pytest.mark.parametrize('offset', [0, 1], ids=['aligned', 'one_float_off'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_flags_of_a_whole_grid_in_one_launch(gpu_ctx, shape, offset):
    ctx = gpu_ctx
    x = _bits(shape, 5)
    x[x == NEG_ZERO] = 0                                                             # (kept apart: the cases below)
    # zero a corner so that some windows inside the tensor are all-zero too
    x[tuple(slice(0, 3) for _ in shape)] = 0
    keep, src = _dev(x, offset)
    D, H, W = _dhw(shape)
    for size in SIZES:
        extent = (size,) * len(shape)
        origins = _origins(shape, size) + [tuple(0 for _ in shape), tuple(1 for _ in shape)]
        org = np.ascontiguousarray([_zyx(o, 0) for o in origins], dtype=np.int32)
        out, dst, lo = _guarded(len(origins), offset)
        before = ctx.launches()
        rc = ctx.lib.tpz_tile_flags(ctx.handle, C.c_void_p(src), D, H, W, org.ctypes.data_as(C.c_void_p), len(origins),
                                    *_zyx(extent, 1), C.c_void_p(dst))
        assert rc == 0, _err(ctx)
        assert ctx.launches() - before == 1
        torch.cuda.synchronize()
        got, front, back = _read(out, lo, len(origins))
        want = np.array([int(((_window_of(x, o, extent) & np.uint32(0x7fffffff)) != 0).any()) for o in origins], dtype=np.uint32)
        assert np.array_equal(got, want), size
        assert want.min() == 0 and want.max() == 1
        assert (front == SENTINEL).all() and (back == SENTINEL).all()
        for o, f in zip(origins, got):
            if any(c >= n for c, n in zip(o, shape)):
                assert f == 0                                                        # wholly outside: flag 0
    del keep


def test_flags_nan_negative_zero_and_what_lies_outside(gpu_ctx):
    """torch's ne(0): a NaN counts, -0.0 does not -- and neither does memory that is not the tensor's: the words around it, the
    start of the next row behind a window that reaches past the right edge"""
    from topaz_amd import runtime as rt
    ctx = gpu_ctx
    H, W = 9, 11
    for dims in (2, 3):
        shape = (H, W) if dims == 2 else (3, H, W)
        only_nan = np.zeros(shape, np.uint32)
        only_nan[(1,) * (dims - 2) + (4, 6)] = NAN
        only_negzero = np.full(shape, NEG_ZERO, np.uint32)
        subnormal = np.zeros(shape, np.uint32)
        subnormal[(0,) * (dims - 2) + (5, 5)] = 1                                    # the smallest subnormal: != 0
        next_row = np.zeros(shape, np.uint32)
        next_row[(0,) * (dims - 2) + (5, 0)] = 0x3f800000                            # 1.0 at the start of row 5
        size = (4,) * dims
        front = (0,) * (dims - 2)
        cases = [(only_nan, front + (3, 4), 1), (only_nan, (-3,) * (dims - 2) + (3, 4), 1 if dims == 2 else 0),
                 (only_nan, front + (5, 4), 0), (only_negzero, front + (0, 0), 0), (only_negzero, front + (-2, 9), 0),
                 (subnormal, front + (4, 4), 1),
                 (next_row, front + (4, W - 1), 0),                                  # reaches past the right edge of row 4
                 (next_row, front + (5, -3), 1)]
        for x, origin, want in cases:
            # the tensor lies in a buffer of NaN words: nothing outside it may be taken for an element
            buf = np.full(x.size + 64, NAN, np.uint32)
            buf[33:33 + x.size] = x.reshape(-1)
            dev = torch.from_numpy(buf.view(np.float32)).cuda()
            view = dev[33:33 + x.size].view(shape)
            torch_says = int(bool(torch.from_numpy(_window_of(x, origin, size).view(np.float32)).ne(0).any()))
            got = rt.tile_flags(view, [origin, tuple(n + 1 for n in shape)], size, ctx).cpu().numpy()
            assert got.dtype == np.int32 and got.tolist() == [want, 0], (dims, origin)
            assert torch_says == want
            tile = rt.tile_cut(view, origin, size, ctx).cpu().numpy().view(np.uint32)
            assert np.array_equal(tile, _window_of(x, origin, size))
    assert rt.tile_flags(torch.zeros(4, 4).cuda(), [], (2, 2), ctx).numel() == 0     # zero windows: not an error


PASTES = [  # (tile shape, crop, extent, canvas shape, at)
    ((37, 37), (3, 3), (31, 31), (33, 70), (0, 0)),
    ((37, 37), (3, 3), (31, 31), (33, 70), (10, 50)),                                # clipped at the far corner
    ((37, 37), (0, 1), (37, 36), (33, 70), (-5, -6)),                                # clipped at the near corner
    ((4, 4), (1, 1), (2, 2), (7, 9), (6, 8)),
    ((4, 4), (0, 0), (4, 4), (7, 9), (2, 4)),
    ((1, 1), (0, 0), (1, 1), (7, 9), (6, 8)),
    ((1, 1), (0, 0), (1, 1), (7, 9), (7, 9)),                                        # wholly outside: nothing written
    ((8, 40), (2, 4), (4, 32), (33, 70), (3, 4)),                                    # 16-byte groups on both sides
    ((8, 8, 8), (2, 2, 2), (4, 4, 4), (5, 7, 9), (0, 0, 0)),
    ((8, 8, 8), (2, 2, 2), (4, 4, 4), (5, 7, 9), (4, 4, 8)),                         # clipped on every axis
    ((37, 4, 5), (1, 0, 1), (36, 4, 3), (5, 7, 9), (-33, 5, 7)),
]


@pytest.mark.parametrize('offset', [0, 1], ids=['aligned', 'one_element_off'])
@pytest.mark.parametrize('f64', [False, True], ids=['fp32_canvas', 'fp64_canvas'])
def test_paste_against_numpy(gpu_ctx, f64, offset):
    ctx = gpu_ctx
    for k, (tshape, crop, extent, cshape, at) in enumerate(PASTES):
        tile = _bits(tshape, 40 + k)
        before = _bits(cshape, 80 + k)
        keep, src = _dev(tile, offset)
        n = int(np.prod(cshape))
        if f64:
            prior = before.view(np.float32).astype(np.float64)
            prior[np.isnan(prior)] = -7.25                                           # (NaN bits of a conversion are not compared)
            prior = prior.view(np.uint64)
            canvas, dst, lo = _guarded(n, offset, fill=np.uint64(0xDEADBEEFDEADBEEF), itemsize=8)
            host = canvas.cpu().numpy().view(np.uint64)
            host[lo:lo + n] = prior.reshape(-1)
            canvas.copy_(torch.from_numpy(host.view(np.int64)))
        else:
            prior = before
            canvas, dst, lo = _guarded(n, offset)
            host = canvas.cpu().numpy().view(np.uint32)
            host[lo:lo + n] = prior.reshape(-1)
            canvas.copy_(torch.from_numpy(host.view(np.int32)))
        rc = ctx.lib.tpz_tile_paste(ctx.handle, C.c_void_p(src), *_zyx(tshape, 1), *_zyx(crop, 0), *_zyx(extent, 1),
                                    C.c_void_p(dst), 1 if f64 else 0, *_dhw(cshape), *_zyx(at, 0))
        assert rc == 0, _err(ctx)
        torch.cuda.synchronize()
        got, front, back = _read(canvas, lo, n, 8 if f64 else 4)
        # numpy: the box of the tile, clipped to the canvas
        want = prior.copy().reshape(cshape)
        box = tile[tuple(slice(c, c + e) for c, e in zip(crop, extent))]
        src_sl, dst_sl, empty = [], [], False
        for a, e, m in zip(at, extent, cshape):
            lo_, hi_ = max(a, 0), min(a + e, m)
            empty |= lo_ >= hi_
            dst_sl.append(slice(lo_, hi_))
            src_sl.append(slice(lo_ - a, hi_ - a))
        if not empty:
            piece = box[tuple(src_sl)]
            if f64:
                wide = piece.view(np.float32).astype(np.float64)
                nan = np.isnan(wide)
                want_f = want.view(np.float64)
                want_f[tuple(dst_sl)] = wide
                got_f = got.view(np.float64).reshape(cshape)
                assert np.array_equal(np.isnan(got_f[tuple(dst_sl)]), nan), k
                got_f[tuple(dst_sl)][nan] = 0.0
                want_f[tuple(dst_sl)][nan] = 0.0
            else:
                want[tuple(dst_sl)] = piece
        assert np.array_equal(got.reshape(cshape), want), (k, tshape, at)            # (bits: fp32 -> fp64 is exact)
        sent = np.uint64(0xDEADBEEFDEADBEEF) if f64 else SENTINEL
        assert (front == sent).all() and (back == sent).all(), k
        del keep


def test_python_wrappers_round_trip(gpu_ctx):
    """runtime.tile_cut / tile_paste: cut every tile of a grid out of an image and paste the tiles' cores back -- the image"""
    from topaz_amd import runtime as rt
    from topaz_amd.model.utils import tile_windows
    for shape, patch, pad in (((33, 70), 16, 3), ((5, 7, 9), 6, 1)):
        x = torch.from_numpy(_bits(shape, 3).view(np.int32).astype(np.float32)).cuda()
        for dtype in (torch.float32, torch.float64):
            out = torch.full(shape, -1.0, dtype=dtype, device='cuda')
            for w in tile_windows(shape, patch, pad):
                tile = rt.tile_cut(x, w.origin, w.extent, gpu_ctx)
                assert tuple(tile.shape) == w.extent
                rt.tile_paste(tile, (pad,) * len(shape), w.pasted, out, w.paste, gpu_ctx)
            assert torch.equal(out, x.to(dtype))


def test_refused_arguments(gpu_ctx):
    ctx = gpu_ctx
    lib, h = ctx.lib, ctx.handle
    buf = torch.zeros(4096, dtype=torch.float32, device='cuda')
    p = C.c_void_p(buf.data_ptr())
    org = (C.c_int * 3)(0, 0, 0)
    big = (1 << 11, 1 << 10, 1 << 10)                                               # 2^31 elements
    refused = [
        ('tpz_tile_cut', lambda: lib.tpz_tile_cut(h, None, 1, 8, 8, 0, 0, 0, 1, 4, 4, p)),
        ('tpz_tile_cut', lambda: lib.tpz_tile_cut(h, p, 1, 8, 8, 0, 0, 0, 1, 4, 4, None)),
        ('tpz_tile_cut', lambda: lib.tpz_tile_cut(h, p, 1, 0, 8, 0, 0, 0, 1, 4, 4, p)),
        ('tpz_tile_cut', lambda: lib.tpz_tile_cut(h, p, 1, 8, 8, 0, 0, 0, 1, 4, 0, p)),
        ('tpz_tile_cut', lambda: lib.tpz_tile_cut(h, p, 1, 8, 8, 0, 0, 0, 1, -4, 4, p)),
        ('tpz_tile_cut', lambda: lib.tpz_tile_cut(h, p, 1, 8, 8, 0, 0, 0, *big, p)),
        ('tpz_tile_cut', lambda: lib.tpz_tile_cut(h, p, 1, 8, 8, 0, 1 << 30, 0, 1, 4, 4, p)),
        ('tpz_tile_flags', lambda: lib.tpz_tile_flags(h, None, 1, 8, 8, org, 1, 1, 4, 4, p)),
        ('tpz_tile_flags', lambda: lib.tpz_tile_flags(h, p, 1, 8, 8, None, 1, 1, 4, 4, p)),
        ('tpz_tile_flags', lambda: lib.tpz_tile_flags(h, p, 1, 8, 8, org, 1, 1, 4, 4, None)),
        ('tpz_tile_flags', lambda: lib.tpz_tile_flags(h, p, 1, 8, -8, org, 1, 1, 4, 4, p)),
        ('tpz_tile_flags', lambda: lib.tpz_tile_flags(h, p, 1, 8, 8, org, 1, 0, 4, 4, p)),
        ('tpz_tile_flags', lambda: lib.tpz_tile_flags(h, p, 1, 8, 8, org, 1, *big, p)),
        ('tpz_tile_flags', lambda: lib.tpz_tile_flags(h, p, 1, 8, 8, org, 1 << 31, 1, 4, 4, p)),
        ('tpz_tile_paste', lambda: lib.tpz_tile_paste(h, None, 1, 4, 4, 0, 0, 0, 1, 4, 4, p, 0, 1, 8, 8, 0, 0, 0)),
        ('tpz_tile_paste', lambda: lib.tpz_tile_paste(h, p, 1, 4, 4, 0, 0, 0, 1, 4, 4, None, 0, 1, 8, 8, 0, 0, 0)),
        ('tpz_tile_paste', lambda: lib.tpz_tile_paste(h, p, 1, 4, 4, 0, 0, 0, 1, 0, 4, p, 0, 1, 8, 8, 0, 0, 0)),
        ('tpz_tile_paste', lambda: lib.tpz_tile_paste(h, p, 1, 4, 4, 0, 0, 0, 1, 4, 4, p, 1, 1, 8, 0, 0, 0, 0)),
        ('tpz_tile_paste', lambda: lib.tpz_tile_paste(h, p, 1, 4, 4, 0, 1, 0, 1, 4, 4, p, 0, 1, 8, 8, 0, 0, 0)),     # crop + n > tile
        ('tpz_tile_paste', lambda: lib.tpz_tile_paste(h, p, 1, 4, 4, 0, 0, -1, 1, 4, 4, p, 0, 1, 8, 8, 0, 0, 0)),    # crop < 0
        ('tpz_tile_paste', lambda: lib.tpz_tile_paste(h, p, 1, 4, 4, 1, 0, 0, 1, 4, 4, p, 0, 1, 8, 8, 0, 0, 0)),     # z crop, 2-D
        ('tpz_tile_paste', lambda: lib.tpz_tile_paste(h, p, *big, 0, 0, 0, 1, 4, 4, p, 0, 1, 8, 8, 0, 0, 0)),
        ('tpz_tile_paste', lambda: lib.tpz_tile_paste(h, p, 1, 4, 4, 0, 0, 0, 1, 4, 4, p, 0, 1, 8, 8, 0, 0, -(1 << 30))),
    ]
    launches = ctx.launches()
    for name, call in refused:
        assert call() != 0, name
        assert _err(ctx).startswith(name + ':'), (name, _err(ctx))
    assert ctx.launches() == launches                                                # refused before any launch
    assert lib.tpz_tile_flags(h, p, 1, 8, 8, None, 0, 1, 4, 4, None) == 0            # zero windows is not an error
    assert ctx.launches() == launches
    torch.cuda.synchronize()
    assert not buf.any()
