"""float16 MRC output (`--float16`, MRC mode 12), the host side: the flag on every command that writes MRC, its
refusal with another --format, mrc.write(dtype=np.float16), and the 2-bytes-per-pixel offsets of stack sections and particles."""
import argparse
import io
import os

import numpy as np
import pytest

from conftest import ROOT


def _parsers():
    from topaz_amd.commands import denoise, denoise3d, downsample, extract, normalize, particle_stack, preprocess
    return {'preprocess': (preprocess, ['a.mrc']), 'normalize': (normalize, ['a.mrc']), 'downsample': (downsample, ['a.mrc']),
            'denoise': (denoise, ['a.mrc']), 'denoise --stack': (denoise, ['--stack', 's.mrc']),
            'denoise3d': (denoise3d, ['t.mrc']), 'particle_stack': (particle_stack, ['picks.txt', '--size', '32']),
            'extract': (extract, ['-r', '8', '--particle-stack', 'o.mrcs', '--particle-size', '32', 'a.mrc'])}


@pytest.mark.parametrize('command', sorted(_parsers()))
def test_flag_parses_on_every_command_that_writes_mrc(command):
    module, argv = _parsers()[command]
    # (as the `topaz` entry point builds them: particle_stack alone keeps the reference's flag surface)
    parser = module.add_arguments(argparse.ArgumentParser())
    assert parser.parse_args(argv).float16 is False
    assert parser.parse_args(argv + ['--float16']).float16 is True
    assert '--float16' in parser.format_help()


def test_whole_command_lines_parse_with_ranks():
    from topaz_amd.commands import denoise, extract
    a = denoise.add_arguments().parse_args(['--stack', '--gpus', '2', '--float16', '-o', 'o.mrc', 's.mrc'])
    assert (a.stack, a.gpus, a.float16) == (True, 2, True)
    b = extract.add_arguments().parse_args(['-r', '8', '--gpus', '2', '--particle-stack', 'o.mrcs', '--particle-size', '32',
                                            '--float16', 'a.mrc'])
    assert (b.gpus, b.float16, b.particle_stack) == (2, True, 'o.mrcs')


def test_float16_with_another_format_is_refused_before_anything_is_read(tmp_path, monkeypatch):
    """the inputs do not exist and no device is asked for: the refusal comes first"""
    from topaz_amd import cuda
    from topaz_amd.commands import denoise, downsample, extract, normalize
    from topaz_amd.mrc import check_float16_formats

    def no_device(*a, **k):
        raise AssertionError('a device was asked for before the refusal')
    monkeypatch.setattr(cuda, 'set_device', no_device)
    monkeypatch.setattr(denoise, 'set_device', no_device)
    missing = str(tmp_path / 'missing.mrc')
    with pytest.raises(ValueError, match='--float16.*png'):
        denoise.main(denoise.add_arguments().parse_args(['--float16', '--format', 'png', '-o', str(tmp_path), missing]))
    with pytest.raises(ValueError, match='--float16.*jpg'):
        denoise.main(denoise.add_arguments().parse_args(['--float16', '--format', 'jpg', '-o', str(tmp_path), missing]))
    for fmt in ('png', 'mrc,png', 'tiff'):
        with pytest.raises(ValueError, match='--float16'):
            normalize.main(normalize.add_arguments().parse_args(['--float16', '--format', fmt, '-o', str(tmp_path), missing]))
    with pytest.raises(ValueError, match='--float16'):
        downsample.main(downsample.add_arguments().parse_args(['--float16', '-o', str(tmp_path / 'small.png'), missing]))
    with pytest.raises(ValueError, match='--particle-stack'):
        extract.main(extract.add_arguments().parse_args(['-r', '8', '--float16', missing]))
    assert os.listdir(tmp_path) == []
    check_float16_formats(True, ['mrc'])
    check_float16_formats(False, ['png', 'tiff'])


def test_write_float16_round_trips_and_the_generated_header_describes_the_file():
    from topaz_amd import mrc
    rs = np.random.RandomState(0)
    x = (rs.randn(3, 17, 23) * 100).astype(np.float32)
    x[0, 0, :4] = [65504, 1e-7, -0.0, 3e-5]                       # the largest half, a subnormal, a signed zero
    half = x.astype(np.float16)
    f = io.BytesIO()
    mrc.write(f, half, dtype=np.float16)
    array, header, extended = mrc.parse(f.getvalue())
    assert header.mode == 12 and array.dtype == np.float16 and extended == b''
    assert np.array_equal(array.view(np.uint16), half.view(np.uint16))
    assert len(f.getvalue()) == 1024 + 2 * x.size
    up = half.astype(np.float32)
    assert (header.amin, header.amax, header.amean, header.rms) == \
        tuple(np.float32(v) for v in (up.min(), up.max(), up.mean(), up.std()))
    assert (header.nx, header.ny, header.nz) == (23, 17, 3)
    # a float32 array under dtype=np.float16 is cast: the same file
    g = io.BytesIO()
    mrc.write(g, x, dtype=np.float16)
    assert g.getvalue() == f.getvalue()
    # a supplied header keeps its statistics; only its mode follows the stored type
    supplied = mrc.make_header(x.shape, (1, 2, 3), (90, 90, 90), dmin=-7, dmax=7, dmean=0.5, rms=2, exthd_size=4)
    assert supplied.mode == 2
    h = io.BytesIO()
    mrc.write(h, half, header=supplied, extended_header=b'abcd', dtype=np.float16)
    array, header, extended = mrc.parse(h.getvalue())
    assert header == supplied._replace(mode=12) and extended == b'abcd'
    assert np.array_equal(array.view(np.uint16), half.view(np.uint16))
    with pytest.raises(ValueError):
        mrc.write(io.BytesIO(), x, dtype=np.int16)


def test_headers_accept_float16_by_name():
    from topaz_amd import mrc
    assert mrc.get_mode_for_header(np.float16) == 12 and mrc.get_mode_for_header(np.dtype('float16')) == 12
    assert mrc.get_mode_for_header(np.float32) == 2 and mrc.get_mode_for_header(np.int16) == 1
    assert mrc.make_header((2, 3, 4), (1, 1, 1), (0, 0, 0), dtype=np.float16).mode == 12
    assert mrc.make_header((2, 3, 4), (1, 1, 1), (0, 0, 0)).mode == 2


def test_default_write_is_the_bytes_of_today():
    """mode 2, the statistics of the float32 array, the array's own bytes: spelled out here, not read from mrc.write"""
    from topaz_amd import mrc
    x = (np.random.RandomState(1).randn(1, 9, 11) * 3).astype(np.float32)
    header = mrc.make_header(x.shape, (1, 1, 1), (0, 0, 0), mz=1, dmin=x.min(), dmax=x.max(), dmean=x.mean(), rms=x.std())
    assert (header.mode, header.nx, header.ny, header.nz, header.next) == (2, 11, 9, 1, 0)
    want = mrc.header_struct.pack(*list(header)) + x.tobytes()
    for kw in ({}, {'dtype': np.float32}):
        f = io.BytesIO()
        mrc.write(f, x, **kw)
        assert f.getvalue() == want
    # a float16 array without the dtype is stored as float32, as ever
    f = io.BytesIO()
    mrc.write(f, x.astype(np.float16))
    assert mrc.parse(f.getvalue())[1].mode == 2 and len(f.getvalue()) == 1024 + 4 * x.size


def test_save_image_passes_float16_and_uint8_through(tmp_path):
    from PIL import Image
    from topaz_amd import mrc
    from topaz_amd.utils.image import quantize, save_image
    x = (np.random.RandomState(2).randn(12, 14) * 2).astype(np.float32)
    header = mrc.make_header((1, 12, 14), (1, 1, 1), (0, 0, 0))
    save_image(x, str(tmp_path / 'a.mrc'), header=header)
    save_image(x.astype(np.float16), str(tmp_path / 'b.mrc'), header=header)
    a, ha, _ = mrc.parse(open(tmp_path / 'a.mrc', 'rb').read())
    b, hb, _ = mrc.parse(open(tmp_path / 'b.mrc', 'rb').read())
    assert ha.mode == 2 and hb == ha._replace(mode=12)
    assert np.array_equal(b.view(np.uint16), a.astype(np.float16).view(np.uint16))
    for fmt in ('png', 'jpg'):
        save_image(x, str(tmp_path / 'f32'), f=fmt)
        save_image(quantize(x), str(tmp_path / 'u8'), f=fmt)       # already bytes: not quantised a second time
        assert open(tmp_path / ('f32.' + fmt), 'rb').read() == open(tmp_path / ('u8.' + fmt), 'rb').read()
    assert np.array_equal(np.array(Image.open(tmp_path / 'u8.png')), quantize(x))


def test_offsets_take_two_bytes_per_pixel_under_the_flag():
    from topaz_amd.denoise import stack_section_offset
    from topaz_amd.utils import picks as pk
    assert stack_section_offset(0, 96, 128, 40) == stack_section_offset(0, 96, 128, 40, 2) == 1064
    assert stack_section_offset(3, 96, 128, 40) == 1064 + 4 * 3 * 96 * 128
    assert stack_section_offset(3, 96, 128, 40, 4) == stack_section_offset(3, 96, 128, 40)
    assert stack_section_offset(3, 96, 128, 40, 2) == 1064 + 2 * 3 * 96 * 128
    assert pk.particle_bytes(1, 32) == 4 * 32 * 32 and pk.particle_bytes(1, 32, True) == 2 * 32 * 32
    assert pk.particle_bytes(3, 9, False) == 4 * 3 * 81 and pk.particle_bytes(3, 9, True) == 2 * 3 * 81
    # one round of a sharded extract: rank 1 of counts (5, 7, 0) after 10 particles starts at particle 15, whatever the type --
    # its byte follows from the particle size
    first, base = pk.particle_offset(10, [5, 7, 0], 1)
    assert (first, base) == (15, 22)
    assert pk.particle_byte_offset(first, pk.particle_bytes(1, 32)) == 1024 + 15 * 4096
    assert pk.particle_byte_offset(first, pk.particle_bytes(1, 32, True)) == 1024 + 15 * 2048


def test_particle_stack_plan_and_seal_under_the_flag(tmp_path):
    from topaz_amd import mrc
    from topaz_amd.utils import picks as pk
    records = [pk.Record('a.mrc', np.array([[5, 6], [7, 8]]), np.array([1.0, 2.0])), pk.Record('b.mrc', np.array([[1, 2]]), np.array([3.0]))]
    out = str(tmp_path / 'stack.mrcs')
    h32, star_path, star = pk.plan_from_records(records, out, 32, 16, 1, (1, 2, 3), (90, 90, 90), None)
    h16, star_path16, star16 = pk.plan_from_records(records, out, 32, 16, 1, (1, 2, 3), (90, 90, 90), None, float16=True)
    a, b = mrc.parse_header(h32), mrc.parse_header(h16)
    assert a.mode == 2 and b == a._replace(mode=12) and (star_path, star) == (star_path16, star16)
    with open(out, 'wb') as f:
        f.write(bytes(1024 + 4 * pk.particle_bytes(1, 16, True)))       # a placeholder and four particles: one too many
    pk.seal_particle_stack(out, h16, 3, pk.particle_bytes(1, 16, True), star_path, star)
    data = open(out, 'rb').read()
    assert len(data) == 1024 + 3 * 2 * 16 * 16 and data[:1024] == h16
    array, header, _ = mrc.parse(data)
    assert array.shape == (3, 16, 16) and array.dtype == np.float16 and open(star_path).read() == star


def test_new_symbols_are_declared_prototyped_and_documented():
    from topaz_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'topaz_hip.h')).read()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name, nargs in (('tpz_encode', 7), ('tpz_stage_encode_bytes', 2), ('tpz_stage_d2h_encode', 6)):
        assert name in _lib.EXPORTED_SYMBOLS and len(_lib._SIGNATURES[name][1]) == nargs
        assert name + '(' in header and name in doc
    assert 'TPZ_ENC_F16 = %d' % _lib.TPZ_ENC_F16 in header and 'TPZ_ENC_U8 = %d' % _lib.TPZ_ENC_U8 in header
