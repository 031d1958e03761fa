"""Results encoded on the device on their way out: tpz_encode's float16 against numpy's astype(np.float16) bit for
bit -- around every one of the 65 536 half patterns, at the rounding midpoints, the overflow threshold, the subnormals and NaN
payloads -- with its overflow counter; its uint8 against utils.image.quantize around every rounding boundary; both over the
lengths and alignments at which the vector body and the scalar loop meet; Stage.download_encoded through a ring."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SENTINEL = 0xa5
GUARD = 64                      # bytes in front of and behind d_out (d_out stays 16-byte aligned)
LENGTHS = [0, 1, 7, 8, 9, 2047, 2048, 2049, 8 * 256 * 3 + 5]
ENC_F16, ENC_U8 = 12, 8
ITEM = {ENC_F16: 2, ENC_U8: 1}
STORED = {ENC_F16: np.uint16, ENC_U8: np.uint8}


def _encode(ctx, x: np.ndarray, enc: int, params=None, count: bool = True, in_offset: int = 0, out_offset: int = 0):
    """tpz_encode on x -> (return code, stored pixels as their unsigned bits, guard bytes in front, guard bytes behind, counter).
    in_offset (floats) moves d_in off 16 bytes, out_offset (pixels) d_out."""
    n, item = x.size, ITEM[enc]
    src = torch.zeros(n + 8, dtype=torch.float32, device='cuda')
    src[in_offset:in_offset + n] = torch.from_numpy(x.view(np.int32)).cuda().view(torch.float32)      # (bit-exact: no float pass)
    out = torch.full((2 * GUARD + (n + out_offset) * item + 16,), SENTINEL, dtype=torch.uint8, device='cuda')
    counter = torch.zeros(1, dtype=torch.int64, device='cuda')
    p = None if params is None else (C.c_float * 2)(*params)
    ctx.bind_current_stream()
    lo = GUARD + out_offset * item
    rc = ctx.lib.tpz_encode(ctx.handle, C.c_void_p(src.data_ptr() + 4 * in_offset), n, enc, p, C.c_void_p(out.data_ptr() + lo),
                            C.c_void_p(counter.data_ptr()) if count else None)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    return rc, got[lo:lo + n * item].view(STORED[enc]), got[:lo], got[lo + n * item:], int(counter.item())


def _half(x: np.ndarray) -> np.ndarray:
    with np.errstate(over='ignore', invalid='ignore'):
        return x.astype(np.float16)


@pytest.fixture(scope='module')
def around_every_half():
    """fp32 inputs around all 65 536 half patterns (see the module docstring); shared, read only"""
    h = np.arange(65536, dtype=np.uint16).view(np.float16)
    finite = h[np.isfinite(h)].astype(np.float32)
    up, down = np.float32(np.inf), np.float32(-np.inf)
    # the exact midpoint between a half and the next one up (in fp64, then to fp32: 12 significant bits, exact)
    with np.errstate(over='ignore'):                             # (65504 steps to inf)
        nxt = np.nextafter(h[np.isfinite(h)], np.float16(np.inf)).astype(np.float64)
    mid = ((finite.astype(np.float64) + np.where(np.isinf(nxt), 65536.0, nxt)) / 2).astype(np.float32)
    special = np.array([65504, 65519.996, 65520, np.finfo(np.float32).max, np.inf, -np.inf, 0.0, -0.0,
                        -65504, -65519.996, -65520, -np.finfo(np.float32).max], dtype=np.float32)
    assert special[1] < np.float32(65520) and special[1] > np.float32(65504)
    sub32 = np.array([1, 2, 0x7fffff, 0x400000, 0x80000001, 0x807fffff], dtype=np.uint32).view(np.float32)   # fp32 subnormals
    small = np.array([2.0 ** -25, 2.0 ** -24, 2.0 ** -26, 1.5 * 2.0 ** -25, 2.0 ** -14, -2.0 ** -25], dtype=np.float32)
    small = np.concatenate([small, np.nextafter(small, up), np.nextafter(small, down)])
    payloads = (np.arange(1, 9, dtype=np.uint32) * np.uint32(0x0009a7c1)) & np.uint32(0x7fffff)
    payloads[0], payloads[1] = 1, 0x1fff                      # payloads whose top ten bits are zero: the +1 of numpy's rule
    nans = np.concatenate([0x7f800000 | payloads, 0xff800000 | payloads]).astype(np.uint32)
    assert len(set(nans.tolist())) == 16 and np.isnan(nans.view(np.float32)).all()
    x = np.concatenate([finite, np.nextafter(finite, up), np.nextafter(finite, down), mid, np.nextafter(mid, up),
                        np.nextafter(mid, down), special, sub32, small, nans.view(np.float32)])
    return np.ascontiguousarray(x, dtype=np.float32)


def test_f16_bits_equal_numpy_astype_around_every_half(gpu_ctx, around_every_half):
    x = around_every_half
    want = _half(x).view(np.uint16)
    lost = int(np.sum(np.isfinite(x) & np.isinf(_half(x))))
    assert lost > 0 and ((want & 0x7c00) == 0).sum() > 4000 and np.isnan(x).sum() == 16    # the input holds what it should
    rc, got, front, back, counted = _encode(gpu_ctx, x, ENC_F16)
    assert rc == 0
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(hex(x.view(np.uint32)[i]), hex(got[i]), hex(want[i])) for i in bad[:8]]
    assert counted == lost
    assert (front == SENTINEL).all() and (back == SENTINEL).all()
    # without a counter: the same bytes
    rc, again, front, back, counted = _encode(gpu_ctx, x, ENC_F16, count=False)
    assert rc == 0 and np.array_equal(again, want) and counted == 0
    assert (front == SENTINEL).all() and (back == SENTINEL).all()


@pytest.fixture(scope='module')
def mixed_floats():
    """LENGTHS[-1] + 8 floats for the length cases: normal values, some beyond the half range, subnormal halves, a NaN"""
    rs = np.random.RandomState(7)
    x = (rs.randn(LENGTHS[-1] + 8) * 3).astype(np.float32)
    x[::97] *= np.float32(1e5)
    x[5::131] *= np.float32(1e-7)
    x[3] = np.nan
    return x


@pytest.mark.parametrize('offset', [0, 1])
@pytest.mark.parametrize('n', LENGTHS)
def test_f16_lengths_and_alignment(gpu_ctx, mixed_floats, n, offset):
    """offset 1: the source is a view one float into a buffer (4-byte aligned only): the scalar loop for every pixel"""
    x = mixed_floats[offset:offset + n]
    rc, got, front, back, counted = _encode(gpu_ctx, x, ENC_F16, in_offset=offset)
    assert rc == 0
    assert np.array_equal(got, _half(x).view(np.uint16)), (n, offset)
    assert counted == int(np.sum(np.isfinite(x) & np.isinf(_half(x))))
    assert (front == SENTINEL).all() and (back == SENTINEL).all()          # nothing past n is written
    if n == LENGTHS[-1]:
        assert counted > 0
        # and a destination that is only 2-byte aligned
        rc, got, front, back, counted = _encode(gpu_ctx, x, ENC_F16, in_offset=offset, out_offset=1)
        assert rc == 0 and np.array_equal(got, _half(x).view(np.uint16))
        assert (front == SENTINEL).all() and (back == SENTINEL).all()


@pytest.fixture(scope='module')
def around_every_byte():
    """inputs of quantize(x, -3, 3) around every rounding boundary (see the module docstring)"""
    k = np.arange(256, dtype=np.float64)
    up, down = np.float32(np.inf), np.float32(-np.inf)
    levels = (k * 6 / 255 - 3).astype(np.float32)
    halves = ((k + 0.5) * 6 / 255 - 3).astype(np.float32)
    parts = [np.linspace(-4, 4, 100001, dtype=np.float32)]
    for v in (levels, halves):
        parts += [v, np.nextafter(v, up), np.nextafter(v, down)]
    parts.append(np.array([np.inf, -np.inf], dtype=np.float32))
    return np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)


def test_u8_bytes_equal_quantize(gpu_ctx, around_every_byte):
    from topaz_amd.utils.image import quantize
    x = around_every_byte
    want = quantize(x, -3, 3)
    assert want.dtype == np.uint8 and want.min() == 0 and want.max() == 255 and len(np.unique(want)) == 256
    rc, got, front, back, _ = _encode(gpu_ctx, x, ENC_U8, params=(-3, 3))
    assert rc == 0
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(float(x[i]), int(got[i]), int(want[i])) for i in bad[:8]]
    assert (front == SENTINEL).all() and (back == SENTINEL).all()


@pytest.mark.parametrize('offset', [0, 1])
@pytest.mark.parametrize('n', LENGTHS)
def test_u8_lengths_and_alignment(gpu_ctx, around_every_byte, n, offset):
    from topaz_amd.utils.image import quantize
    x = around_every_byte[50000 - 3000 + offset:][:n]              # (the middle of the ramp: every byte value occurs)
    rc, got, front, back, _ = _encode(gpu_ctx, x, ENC_U8, params=(-3, 3), in_offset=offset)
    assert rc == 0
    assert np.array_equal(got, quantize(x, -3, 3) if n else np.zeros(0, np.uint8)), (n, offset)
    assert (front == SENTINEL).all() and (back == SENTINEL).all()
    if n == LENGTHS[-1]:
        rc, got, front, back, _ = _encode(gpu_ctx, x, ENC_U8, params=(-3, 3), in_offset=offset, out_offset=3)
        assert rc == 0 and np.array_equal(got, quantize(x, -3, 3))
        assert (front == SENTINEL).all() and (back == SENTINEL).all()


def test_u8_stores_nan_as_zero(gpu_ctx):
    x = np.array([np.nan, 0.0, -np.nan, 3.0] * 5, dtype=np.float32)
    rc, got, _, _, _ = _encode(gpu_ctx, x, ENC_U8, params=(-3, 3))
    assert rc == 0 and got.tolist() == [0, 128, 0, 255] * 5


def test_encode_refuses_what_it_cannot_do(gpu_ctx):
    x = np.zeros(16, dtype=np.float32)
    for enc in (0, 1, 2, 6, -1, 16):
        rc = gpu_ctx.lib.tpz_encode(gpu_ctx.handle, C.c_void_p(256), 16, enc, None, C.c_void_p(256), None)
        assert rc != 0 and b'TPZ_ENC' in gpu_ctx.lib.tpz_last_error(gpu_ctx.handle)
    rc, got, front, back, _ = _encode(gpu_ctx, x, ENC_U8, params=None)             # no mi, ma
    assert rc != 0 and (got == SENTINEL).all()
    assert gpu_ctx.lib.tpz_encode(gpu_ctx.handle, None, 16, ENC_F16, None, None, None) != 0
    assert gpu_ctx.lib.tpz_stage_encode_bytes(3, 100) == 0
    assert gpu_ctx.lib.tpz_stage_encode_bytes(ENC_F16, 100) == 256 + 256 and gpu_ctx.lib.tpz_stage_encode_bytes(ENC_U8, 257) == 768


def test_runtime_encode(gpu_ctx):
    from topaz_amd import runtime as rt
    x = np.random.RandomState(3).randn(37, 41).astype(np.float32) * 2
    x[4, 5], x[6, 7] = 7e4, -1e9
    half, lost = rt.encode(torch.from_numpy(x).cuda(), rt.ENC_F16, ctx=gpu_ctx)
    assert half.dtype == torch.float16 and tuple(half.shape) == x.shape and lost == 2
    assert np.array_equal(half.cpu().numpy().view(np.uint16), _half(x).view(np.uint16))
    from topaz_amd.utils.image import quantize
    u8, lost = rt.encode(torch.from_numpy(x).cuda(), rt.ENC_U8, (-3, 3), ctx=gpu_ctx)
    assert u8.dtype == torch.uint8 and lost == 0 and np.array_equal(u8.cpu().numpy(), quantize(x))


def test_download_encoded_through_a_ring_of_two_slots(gpu_ctx):
    """three tensors of growing size through two slots: each arrives as the bytes and the counter of tpz_encode; a plain
    download into a slot that carried encoded pixels still delivers float32; bad arguments queue nothing"""
    from topaz_amd import runtime as rt
    from topaz_amd._lib import TopazHipError
    from topaz_amd.utils.image import quantize
    rs = np.random.RandomState(11)
    shapes = [(5, 7), (64, 65), (130, 257)]
    xs = [(rs.randn(*s) * 3).astype(np.float32) for s in shapes]
    for i, x in enumerate(xs):
        x.reshape(-1)[:i + 1] = 1e6                                # i + 1 finite values beyond the half range
    n_max = xs[-1].size
    assert rt.Stage.encode_bytes(gpu_ctx, rt.ENC_F16, n_max) == (2 * n_max + 255) // 256 * 256 + 256
    stage = rt.Stage(gpu_ctx, max(rt.Stage.encode_bytes(gpu_ctx, rt.ENC_F16, n_max), 4 * n_max), 2)
    try:
        devs = [torch.from_numpy(x).cuda() for x in xs]
        for enc, params in ((rt.ENC_F16, None), (rt.ENC_U8, (-3, 3))):
            for i, (x, d) in enumerate(zip(xs, devs)):
                k = i % 2
                stage.download_encoded(k, d, enc, params)
                stage.wait(k)
                got = stage.host_array(k, x.shape, rt.ENC_DTYPES[enc])
                want, lost = rt.encode(d, enc, params, ctx=gpu_ctx)
                assert np.array_equal(got.view(STORED[enc]), want.cpu().numpy().view(STORED[enc])), (enc, i)
                assert stage.overflow_count(k, x.size, enc) == lost == (i + 1 if enc == rt.ENC_F16 else 0)
                if enc == rt.ENC_F16:
                    assert np.array_equal(got.view(np.uint16), _half(x).view(np.uint16))
                else:
                    assert np.array_equal(got, quantize(x))
        stage.download(0, devs[2])                                 # the slot of today's path, after encoded traffic
        stage.wait(0)
        assert np.array_equal(stage.host_array(0, xs[2].shape), xs[2])
        # refused, nothing queued: an unknown encoding, no mi / ma, a slot that is too small
        marker = stage.host_array(1, (64,), np.uint8)
        marker[:] = 0x77
        big = torch.zeros(stage.slot_bytes, dtype=torch.float32, device='cuda')
        for bad in (lambda: stage.download_encoded(1, devs[0], 5), lambda: stage.download_encoded(1, devs[0], rt.ENC_U8),
                    lambda: stage.download_encoded(1, big, rt.ENC_F16), lambda: stage.download_encoded(7, devs[0], rt.ENC_F16)):
            with pytest.raises(TopazHipError):
                bad()
        rc = gpu_ctx.lib.tpz_stage_d2h_encode(stage.handle, 1, None, 8, rt.ENC_F16, None)
        assert rc != 0
        stage.wait(1)
        torch.cuda.synchronize()
        assert (stage.host_array(1, (64,), np.uint8) == 0x77).all()
    finally:
        stage.close()


def test_result_ring_hands_over_the_stored_dtype_and_the_count(gpu_ctx):
    from topaz_amd import runtime as rt
    from topaz_amd.streaming import ResultRing
    from topaz_amd.utils.image import quantize
    rs = np.random.RandomState(13)
    xs = [(rs.randn(40 + 30 * i, 33) * 2).astype(np.float32) for i in range(4)]
    xs[2][1, 1] = xs[2][2, 2] = -7e4
    got, heard = [], []
    ring = ResultRing(gpu_ctx, lambda host, i, what: got.append((i, what, np.array(host))), 2,
                      on_overflow=lambda lost, i, what: heard.append((i, what, lost)))
    with ring:
        for i, x in enumerate(xs):
            d = torch.from_numpy(x).cuda()
            ring.put(d, i, 'f32')
            ring.put(d, i, 'f16', encode=rt.ENC_F16)
            ring.put(d, i, 'u8', encode=(rt.ENC_U8, (-3, 3)))
    ring.check()
    assert [(i, what) for i, what, _ in got] == [(i, what) for i in range(4) for what in ('f32', 'f16', 'u8')]
    for i, what, host in got:
        want = {'f32': xs[i], 'f16': _half(xs[i]), 'u8': quantize(xs[i])}[what]
        assert host.dtype == want.dtype and host.shape == want.shape and np.array_equal(host, want), (i, what)
    assert heard == [(2, 'f16', 2)]
