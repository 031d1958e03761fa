"""MRC frames staged in the type the file stores and decoded on the device: tpz_decode against numpy's
astype(np.float32) bit for bit over every value of every type and over the lengths at which its vector body and its scalar tail
meet; the feed over a mixed list of files; the commands on int16 / float16 / float32 files of the same values, byte for byte."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_cpu_stored_types import MODES, write_stored

pytestmark = pytest.mark.gpu
CLI = os.path.join(GOLDEN, 'cli')
GUARD = 32                      # floats in front of and behind d_out (128 bytes: d_out stays 16-byte aligned)
SENTINEL = 0x5ca1ab1e
LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65, 4099, (1 << 20) + 3]


def _decode(ctx, raw_bytes: np.ndarray, mode: int, n: int, out_offset: int = 0, raw_offset: int = 0):
    """tpz_decode on n pixels -> (return code, fp32 result as uint32 bits [n], the guard words in front, those behind).
    out_offset (floats) / raw_offset (bytes) move the pointers off their natural alignment."""
    raw = torch.zeros(raw_bytes.size + 64, dtype=torch.uint8, device='cuda')
    raw[raw_offset:raw_offset + raw_bytes.size] = torch.from_numpy(raw_bytes).cuda()
    out = torch.full((n + 2 * GUARD + 8,), SENTINEL, dtype=torch.int32, device='cuda')
    ctx.bind_current_stream()
    rc = ctx.lib.tpz_decode(ctx.handle, C.c_void_p(raw.data_ptr() + raw_offset), mode, n,
                            C.c_void_p(out.data_ptr() + 4 * (GUARD + out_offset)))
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    lo = GUARD + out_offset
    return rc, got[lo:lo + n], got[:lo], got[lo + n:]


def _assert_decoded(got_bits, stored: np.ndarray, what):
    want = stored.astype(np.float32)
    nan = np.isnan(want)
    assert np.array_equal(got_bits[~nan], want.view(np.uint32)[~nan]), what
    assert np.isnan(got_bits.view(np.float32)[nan]).all(), what
    return int(nan.sum())


# ---- decode: every value ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', [0, 1, 6, 12])
def test_decode_every_value(gpu_ctx, mode):
    dt = np.dtype(MODES[mode])
    count = 256 if mode == 0 else 65536
    stored = np.arange(count, dtype=np.uint8 if mode == 0 else np.uint16).view(dt)      # every bit pattern of the type
    rc, got, front, back = _decode(gpu_ctx, stored.view(np.uint8), mode, count)
    assert rc == 0
    n_nan = _assert_decoded(got, stored, mode)
    assert n_nan == (2046 if mode == 12 else 0)
    assert (front == SENTINEL).all() and (back == SENTINEL).all()
    if mode == 12:
        sub = (stored.view(np.uint16) & 0x7c00) == 0
        f = got.view(np.float32)
        assert sub.sum() == 2048 and (np.abs(f[sub & (stored != 0)]) >= np.float32(2.0 ** -24)).all()   # normal fp32 values
        assert got[0] == 0 and got[0x8000] == 0x80000000                                                # +0.0, -0.0
        assert got[0x7c00] == 0x7f800000 and got[0xfc00] == 0xff800000                                  # +inf, -inf


# ---- decode: lengths ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def random_stored():
    """(1 << 20) + 3 random pixels per mode, shared by the length cases (which only read them)"""
    out = {}
    for mode in (0, 1, 6, 12):
        rs = np.random.RandomState(100 + mode)
        if mode == 0:
            x = rs.randint(-128, 128, LENGTHS[-1]).astype(np.int8)
        else:
            x = rs.randint(0, 1 << 16, LENGTHS[-1]).astype(np.uint16).view(MODES[mode])
        out[mode] = x
    return out


@pytest.mark.parametrize('n', LENGTHS)
@pytest.mark.parametrize('mode', [0, 1, 6, 12])
def test_decode_lengths(gpu_ctx, random_stored, mode, n):
    stored = random_stored[mode][:n]
    if mode == 6 and n >= 7:
        assert (stored >= 32768).any()
    if mode in (0, 1) and n >= 7:
        assert (stored < 0).any()
    rc, got, front, back = _decode(gpu_ctx, np.ascontiguousarray(stored).view(np.uint8), mode, n)
    assert rc == 0
    _assert_decoded(got, stored, (mode, n))
    assert (front == SENTINEL).all() and (back == SENTINEL).all()


@pytest.mark.parametrize('mode', [0, 1, 6, 12])
def test_decode_into_an_output_off_16_bytes(gpu_ctx, random_stored, mode):
    """d_out need only be 4-byte aligned: off 16 bytes every pixel takes the scalar loop (more than one block of it)"""
    for off in (1, 2, 3):
        stored = random_stored[mode][:4099]
        rc, got, front, back = _decode(gpu_ctx, np.ascontiguousarray(stored).view(np.uint8), mode, 4099, out_offset=off)
        assert rc == 0
        _assert_decoded(got, stored, (mode, off))
        assert (front == SENTINEL).all() and (back == SENTINEL).all()


def test_decode_refuses_what_it_cannot_do(gpu_ctx):
    raw = np.zeros(64, dtype=np.uint8)
    for mode in (2, 3, 4, 16, 101, -1):
        rc, _, front, back = _decode(gpu_ctx, raw, mode, 8)
        assert rc != 0 and (front == SENTINEL).all() and (back == SENTINEL).all()
        assert b'mode' in gpu_ctx.lib.tpz_last_error(gpu_ctx.handle)
    rc, got, front, back = _decode(gpu_ctx, raw, 1, 8, raw_offset=2)                      # d_raw off 16 bytes
    assert rc != 0 and (got == SENTINEL).all()
    assert b'16-byte' in gpu_ctx.lib.tpz_last_error(gpu_ctx.handle)
    assert gpu_ctx.lib.tpz_decode(gpu_ctx.handle, None, 1, 8, None) != 0


def test_decode_stored_and_stage_upload(gpu_ctx):
    """the two Python forms: runtime.decode_stored on a numpy volume, Stage.upload_decode on a slot (and its size check)"""
    from topaz_amd import runtime as rt
    from topaz_amd._lib import TopazHipError
    x = np.random.RandomState(5).randint(-32768, 32768, (3, 37, 41)).astype(np.int16)
    y = rt.decode_stored(x, gpu_ctx)
    assert y.dtype == torch.float32 and tuple(y.shape) == x.shape
    assert np.array_equal(y.cpu().numpy().view(np.uint32), x.astype(np.float32).view(np.uint32))
    with pytest.raises(TopazHipError):
        rt.decode_stored(x.astype(np.int32), gpu_ctx)
    n = x.size
    need = rt.Stage.decode_bytes(gpu_ctx, 1, n)
    assert need == ((4 * n + 255) // 256 + (2 * n + 255) // 256) * 256
    stage = rt.Stage(gpu_ctx, need, 2)
    try:
        for k in (0, 1, 0):                                        # (a slot used twice: the release / ready events chain)
            stage.host_array(k, x.shape, np.int16)[...] = x + k
            stage.upload_decode(k, 1, n)
            stage.acquire(k)
            got = stage.device_tensor(k, x.shape).cpu().numpy()
            stage.release(k)
            assert np.array_equal(got.view(np.uint32), (x + k).astype(np.float32).view(np.uint32))
        with pytest.raises(TopazHipError, match='slot'):
            stage.upload_decode(0, 1, n + 256)                     # the raw region would not fit
        with pytest.raises(TopazHipError, match='mode'):
            stage.upload_decode(0, 2, n)
    finally:
        stage.close()


# ---- the feed -----------------------------------------------------------------------------------------------------------
FEED_FILES = [('a_i16', np.int16, (37, 41)), ('b_f32', np.float32, (37, 41)), ('c_f16', np.float16, (64, 64)),
              ('d_u16', np.uint16, (130, 257)), ('e_i8', np.int8, (5, 3)), ('f_f32', np.float32, (16, 16))]


def _feed_files(d):
    rs = np.random.RandomState(11)
    paths = []
    for name, dtype, shape in FEED_FILES:
        dt = np.dtype(dtype)
        if dt.kind in 'iu':
            x = rs.randint(np.iinfo(dt).min, np.iinfo(dt).max + 1, shape).astype(dt)
        else:
            x = (rs.randn(*shape) * 100).astype(dt)
        paths.append(write_stored(d / (name + '.mrc'), x))
    return paths


def test_feed_over_mixed_types(gpu_ctx, tmp_path):
    from topaz_amd import mrc
    from topaz_amd.extract import ImageFeed
    paths = _feed_files(tmp_path)
    feed = ImageFeed(paths, gpu_ctx, headers=True)
    seen = []
    for (path, x, header, extended), (name, dtype, shape) in zip(feed, FEED_FILES):
        want, want_header, _ = mrc.read_into(path, lambda s: np.empty(s, dtype=np.float32))
        assert x.dtype == torch.float32 and tuple(x.shape) == shape and header == want_header
        assert np.array_equal(x.cpu().numpy().view(np.uint32), want.view(np.uint32)), name
        seen.append(path)
    assert seen == paths
    assert feed.uploaded_bytes == sum(int(np.prod(shape)) * np.dtype(dtype).itemsize for _, dtype, shape in FEED_FILES)
    assert not feed.thread.is_alive() and feed.stage is None


def test_feed_grows_its_ring_for_a_larger_stored_image(gpu_ctx, tmp_path):
    """a second image whose fp32 + stored bytes exceed the 1 MiB the first ring was rounded to: a new ring mid-stream, of the
    size tpz_stage_h2d_decode needs (6 bytes per uint16 pixel, not 4)"""
    from topaz_amd.extract import ImageFeed
    rs = np.random.RandomState(12)
    small = rs.randint(-100, 100, (37, 41)).astype(np.int16)
    big = rs.randint(0, 65536, (450, 521)).astype(np.uint16)       # 4 n = 937 800 < 1 MiB < 6 n: grows because of the raw region
    assert 4 * big.size < (1 << 20) < 6 * big.size
    paths = [write_stored(tmp_path / 'small.mrc', small), write_stored(tmp_path / 'big.mrc', big),
             write_stored(tmp_path / 'small2.mrc', small)]
    feed = ImageFeed(paths, gpu_ctx)
    sizes = []
    for (path, x), want in zip(feed, (small, big, small)):
        sizes.append(feed.slot_bytes)
        assert np.array_equal(x.cpu().numpy().view(np.uint32), want.astype(np.float32).view(np.uint32)), path
    assert sizes[0] == 1 << 20 and sizes[1] == sizes[2] == 2 << 20
    assert feed.uploaded_bytes == 2 * (2 * small.size + big.size)


def test_feed_takes_in_memory_sections_in_their_stored_type(gpu_ctx):
    from topaz_amd.extract import ImageFeed
    rs = np.random.RandomState(13)
    stack = rs.randint(-3000, 3000, (3, 33, 47)).astype(np.int16)
    wide = rs.randint(0, 1 << 20, (9, 10)).astype(np.int32)        # not a stored type: converted on the host as before
    feed = ImageFeed([(k, stack[k], None, None) for k in range(3)] + [(3, wide, None, None)], gpu_ctx)
    for (key, x), want in zip(feed, list(stack) + [wide]):
        assert np.array_equal(x.cpu().numpy().view(np.uint32), want.astype(np.float32).view(np.uint32)), key
    assert feed.uploaded_bytes == 2 * stack.size + 4 * wide.size


@pytest.mark.timeout(120)
def test_feed_left_early_shuts_down(gpu_ctx, tmp_path):
    from topaz_amd.extract import ImageFeed
    feed = ImageFeed(_feed_files(tmp_path), gpu_ctx)
    it = iter(feed)
    next(it)
    next(it)
    it.close()                                                     # the consumer leaves after the second item
    assert not feed.thread.is_alive() and feed.stage is None
    torch.cuda.synchronize()


# ---- commands: byte-identical outputs -----------------------------------------------------------------------------------
def _run(argv):
    from topaz_amd.main import main
    main(argv)


@pytest.fixture(scope='module')
def mic_files(tmp_path_factory):
    """one integer-valued 150 x 190 crop of mic_a (pixels * 100 + 1000 rounded: 580 .. 1420, below 2048 so float16 holds them
    exactly) as int16, float16 and float32 files of the same name in three directories"""
    from topaz_amd import mrc
    mic, _, _ = mrc.parse(open(os.path.join(CLI, 'mic_a.mrc'), 'rb').read())
    v = np.round(mic[5:155, 3:193] * 100 + 1000).astype(np.int16)
    assert 0 < v.min() and v.max() < 2048 and np.array_equal(v.astype(np.float16).astype(np.float32), v.astype(np.float32))
    root = tmp_path_factory.mktemp('stored')
    files = {}
    for tag, dtype in (('f32', np.float32), ('i16', np.int16), ('f16', np.float16)):
        os.makedirs(root / tag)
        files[tag] = write_stored(root / tag / 'mic.mrc', v.astype(dtype))
    stack = np.stack([v, v[::-1], v[:, ::-1]])
    for tag, dtype in (('f32', np.float32), ('i16', np.int16)):
        files['stack_' + tag] = write_stored(root / tag / 'stack.mrc', stack.astype(dtype))
    return root, files


COMMANDS = {
    'normalize': (['normalize'], 'dir'),
    'preprocess': (['preprocess', '-s', '2', '--sample', '1'], 'dir'),
    'denoise': (['denoise', '-m', 'unet-small'], 'dir'),
    'extract': (['extract', '-m', 'resnet8_u32', '-r', '8'], 'file'),
    'extract_preprocess': (['extract', '-m', 'resnet8_u32', '-r', '8', '--preprocess', '2', '--preprocess-sample', '1'], 'file'),
}


@pytest.mark.parametrize('command', sorted(COMMANDS))
def test_commands_give_the_bytes_of_the_float32_file(gpu_ctx, mic_files, command):
    root, files = mic_files
    argv, kind = COMMANDS[command]
    outputs = {}
    for tag in ('f32', 'i16', 'f16'):
        out = root / f'{command}_{tag}'
        np.random.seed(3)                                          # (`normalize` draws its default 1-in-10 sample from this RNG)
        if kind == 'dir':
            _run(argv + ['-o', str(out), files[tag]])
            names = sorted(os.listdir(out))
            outputs[tag] = [(n, open(out / n, 'rb').read()) for n in names]
        else:
            _run(argv + ['-o', str(out) + '.txt', files[tag]])
            outputs[tag] = [('picks', open(str(out) + '.txt', 'rb').read())]
        assert outputs[tag] and all(len(b) > 0 for _, b in outputs[tag])
    if kind == 'file':
        assert outputs['f32'][0][1].count(b'\n') >= 2              # a header line and a pick at least: the tables compare something
    assert outputs['i16'] == outputs['f32']
    assert outputs['f16'] == outputs['f32']


def test_denoise_stack_int16_through_the_ring(gpu_ctx, mic_files, monkeypatch):
    """`denoise --stack` on a 3-section int16 stack with the sections going through the feed's ring IN int16 (the ring is for
    sections of 1 MiB and more: the threshold is lowered here so that 150 x 190 sections take it).  An integer stack's output is
    cast to the stack's dtype before it is written (what the reference's np.zeros_like(stack) does), a float32 stack's is not: the
    int16 run must give (a) the bytes of the same int16 stack through the one-by-one path, which converts on the host as it always
    did, and (b) the float32 stack's output put through that cast."""
    from topaz_amd import denoise, mrc
    root, files = mic_files
    outs = {}
    for tag, src, ring in (('i16_ring', 'stack_i16', True), ('i16_host', 'stack_i16', False), ('f32_ring', 'stack_f32', True)):
        monkeypatch.setattr(denoise, 'RING_MIN_BYTES', 0 if ring else 1 << 20)
        out = str(root / f'stack_{tag}.mrc')
        _run(['denoise', '-m', 'unet-small', '--stack', '-o', out, files[src]])
        outs[tag] = open(out, 'rb').read()
    assert outs['i16_ring'] == outs['i16_host']
    f32, header, _ = mrc.parse(outs['f32_ring'])
    got, _, _ = mrc.parse(outs['i16_ring'])
    assert got.shape == (3, 150, 190) and np.array_equal(got, f32.astype(np.int16).astype(np.float32))
    assert outs['i16_ring'][:1024] == outs['f32_ring'][:1024]


# ---- 3-D ----------------------------------------------------------------------------------------------------------------
def test_denoise3d_int16_volume(gpu_ctx, tmp_path):
    from topaz_amd import mrc
    from topaz_amd.commands import denoise3d
    tomo, _, _ = mrc.parse(open(os.path.join(CLI, 'tomo.mrc'), 'rb').read())
    v = np.round(tomo[2:30, 1:32, 5:34] * 100 + 1000).astype(np.int16)          # 28 x 31 x 29
    assert v.shape == (28, 31, 29) and 0 < v.min()
    results = {}
    for tag, dtype in (('f32', np.float32), ('i16', np.int16)):
        os.makedirs(tmp_path / tag)
        src = write_stored(tmp_path / tag / 'tomo.mrc', v.astype(dtype))
        args = denoise3d.add_arguments().parse_args(['-m', os.path.join(CLI, 'unet3d_nf8_state.sav'), '--base-kernel-width', '7',
                                                     '-s', '16', '-p', '8', '-d', '0', '-o', str(tmp_path / tag / 'out'), src])
        returned = denoise3d.main(args)
        results[tag] = (open(tmp_path / tag / 'out' / 'tomo.mrc', 'rb').read(), returned)
    assert results['i16'][0] == results['f32'][0]
    for tag in ('f32', 'i16'):
        returned = results[tag][1]
        assert len(returned) == 1 and isinstance(returned[0], np.ndarray)
        assert returned[0].dtype == np.float32 and np.array_equal(returned[0], v.astype(np.float32))
    den, header, _ = mrc.parse(results['i16'][0])
    assert header.mode == 2 and den.shape == v.shape and np.isfinite(den).all() and den.std() > 0
