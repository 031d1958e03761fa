"""`topaz particle_stack` without a GPU: flag surface, the planner (particle order, stack header, STAR text) against the
reference's own output (tests/golden/particle_stack/, tools/make_particle_stack_golden.py) and the explicit errors."""
import os

import numpy as np
import pandas as pd
import pytest

from conftest import GOLDEN

PS = os.path.join(GOLDEN, 'particle_stack')
CLI = os.path.join(GOLDEN, 'cli')
PICKS = os.path.join(CLI, 'extract_picks.txt')


def _plan(picks, out, size, threshold=-np.inf, resize=-1, image_root=CLI, metadata=None):
    import io
    from topaz_amd.utils.picks import plan_particle_stack
    return plan_particle_stack(picks, out, threshold, size, resize, image_root, '.mrc', metadata, log=io.StringIO())


def _read(name, mode='rb'):
    with open(os.path.join(PS, name), mode) as f:
        return f.read()


def test_flags_and_defaults_match_the_reference_parser():
    # topaz/commands/particle_stack.py:12-28: option strings, types and defaults
    from topaz_amd.commands import particle_stack
    p = particle_stack.add_arguments()
    got = {a.dest: (tuple(a.option_strings), a.type, a.default) for a in p._actions if a.dest != 'help'}
    assert got == {'file': ((), None, None), 'image_root': (('--image-root',), None, None),
                   'output': (('-o', '--output'), None, None), 'size': (('--size',), int, None),
                   'threshold': (('--threshold',), float, -np.inf), 'resize': (('--resize',), int, -1),
                   'image_ext': (('--image-ext',), None, '.mrc'), 'metadata': (('--metadata',), None, None)}
    a = p.parse_args(['picks.txt'])
    assert a.threshold == -np.inf and a.resize == -1 and a.image_ext == '.mrc' and a.size is None
    from topaz_amd.main import main
    with pytest.raises(SystemExit) as e:
        main(['particle_stack', '--help'])
    assert e.value.code == 0


@pytest.mark.parametrize('stack,size,threshold,n', [('stack32', 32, -np.inf, 88), ('stack33_t5', 33, -5.0, 44)])
def test_planner_matches_the_reference_on_the_cli_micrographs(stack, size, threshold, n):
    plan = _plan(PICKS, f'/somewhere/{stack}.mrcs', size, threshold)
    ref = _read(stack + '.mrcs')
    assert plan.n == n and plan.mz == 1
    assert len(ref) == 1024 + 4 * n * size * size
    assert plan.header == ref[:1024]
    assert plan.star == _read(stack + '.star', 'r')
    assert plan.star_path == f'/somewhere/{stack}.star'
    # particle order: grouped by sorted image name, file order within a micrograph
    star = pd.read_csv(os.path.join(PS, stack + '.star'), sep='\t', skiprows=2 + 5, header=None)
    xy = np.concatenate([m.xy for m in plan.micrographs])
    assert np.array_equal(xy, star[[1, 2]].values)
    assert [m.name for m in plan.micrographs] == ['mic_a.mrc', 'mic_b.mrc']


def test_planner_three_frames_with_metadata():
    plan = _plan(os.path.join(PS, 'picks3.txt'), 'stack9.mrcs', 9, image_root=PS, metadata=os.path.join(PS, 'meta3.star'))
    ref = _read('stack9.mrcs')
    assert plan.header == ref[:1024]
    assert plan.n == 4 and plan.mz == 3 and plan.micrographs[0].shape == (3, 96, 128)
    assert plan.star == _read('stack9.star', 'r')
    assert 'NrOfFrames' in plan.star and 'DetectorPixelSize' in plan.star and 'Voltage' in plan.star


def test_planner_resize_rescales_the_detector_pixel_size():
    plan = _plan(PICKS, 'stack32_r16.mrcs', 32, resize=16, metadata=os.path.join(PS, 'meta_ab.star'))
    assert plan.star == _read('stack32_r16_meta.star', 'r')
    from topaz_amd import mrc
    h = mrc.parse_header(plan.header)
    assert (h.nz, h.ny, h.nx, h.mz, h.mode) == (88, 16, 16, 1, 2)


def test_read_star_keeps_the_reference_types():
    from topaz_amd.utils.files import read_star
    with open(os.path.join(PS, 'stack9.star')) as f:
        t = read_star(f)
    assert list(t.columns) == ['MicrographName', 'CoordinateX', 'CoordinateY', 'AutopickFigureOfMerit', 'ImageName',
                               'NrOfFrames', 'DetectorPixelSize', 'Voltage']
    assert t['CoordinateX'].dtype.kind == 'i' and t['Voltage'].dtype.kind == 'f' and t['NrOfFrames'].dtype == object


def test_resize_operators_reproduce_the_reference_downsample():
    # the rearranged operators applied in float64 against the reference's rfft2 truncation restated in numpy
    from topaz_amd.utils.picks import resize_operators
    x = np.random.RandomState(3).randn(32, 32)
    for R in (16, 15):
        ops = resize_operators(32, R).astype(np.float64)
        cols = ops[:2 * 32 * R].reshape(2, 32, R)
        rows = ops[2 * 32 * R:].reshape(R, 64)
        y = rows @ np.concatenate([x @ cols[0], x @ cols[1]], 0)
        F = np.fft.rfft2(x)
        F = np.concatenate([F[0:R // 2, 0:R // 2 + 1], F[-R // 2:, 0:R // 2 + 1]], axis=0) * (R * R / 1024)
        assert np.abs(y - np.fft.irfft2(F, s=(R, R))).max() < 1e-5


def _tmp_picks(tmp_path, rows, score=True):
    p = tmp_path / 'picks.txt'
    with open(p, 'w') as f:
        f.write('image_name\tx_coord\ty_coord' + ('\tscore' if score else '') + '\n')
        for r in rows:
            f.write('\t'.join(str(v) for v in r) + '\n')
    return str(p)


def test_box_wholly_below_the_low_edge_is_refused(tmp_path):
    # size 32: left = x - 16, left + 32 < 0 <=> x < -16
    picks = _tmp_picks(tmp_path, [('mic_a', 40, 40, 1.0), ('mic_a', -17, 40, 1.0)])
    with pytest.raises(ValueError, match=r'\(-17, 40\)'):
        _plan(picks, str(tmp_path / 's.mrcs'), 32)
    picks = _tmp_picks(tmp_path, [('mic_b', 40, -20, 1.0)])
    with pytest.raises(ValueError, match=r'\(40, -20\)'):
        _plan(picks, str(tmp_path / 's.mrcs'), 32)
    assert not os.path.exists(tmp_path / 's.mrcs')
    # the edge case that still overlaps nothing but is accepted: left + size == 0 (all zeros, as the reference)
    assert _plan(_tmp_picks(tmp_path, [('mic_a', -16, 40, 1.0)]), str(tmp_path / 's.mrcs'), 32).n == 1


def test_non_float32_micrograph_is_refused(tmp_path):
    from topaz_amd import mrc
    x = (np.random.RandomState(0).rand(40, 50) * 100).astype(np.int16)
    h = mrc.make_header(x[None].shape, (1, 1, 1), (0, 0, 0), dtype=np.int16)
    with open(tmp_path / 'ints.mrc', 'wb') as f:
        f.write(mrc.header_struct.pack(*list(h)))
        f.write(x.tobytes())
    picks = _tmp_picks(tmp_path, [('ints', 20, 20, 0.0)])
    with pytest.raises(ValueError, match='mode 1'):
        _plan(picks, str(tmp_path / 's.mrcs'), 16, image_root=str(tmp_path))


def test_no_surviving_particles_and_missing_size_and_file(tmp_path):
    with pytest.raises(ValueError, match='no particles'):
        _plan(PICKS, str(tmp_path / 's.mrcs'), 32, threshold=100.0)
    with pytest.raises(ValueError, match='--size'):
        _plan(PICKS, str(tmp_path / 's.mrcs'), None)
    with pytest.raises(FileNotFoundError, match='nothere.mrc'):
        _plan(_tmp_picks(tmp_path, [('nothere', 5, 5)], score=False), str(tmp_path / 's.mrcs'), 8)
    # the command line reports the missing --size the same way, before touching the GPU
    from topaz_amd.main import main
    with pytest.raises(ValueError, match='--size'):
        main(['particle_stack', PICKS, '--image-root', CLI, '-o', str(tmp_path / 's.mrcs')])


def test_names_resolve_against_the_working_directory_without_image_root(tmp_path, monkeypatch):
    import shutil
    shutil.copy(os.path.join(CLI, 'mic_a.mrc'), tmp_path / 'mic_a.mrc')
    monkeypatch.chdir(tmp_path)
    plan = _plan(_tmp_picks(tmp_path, [('mic_a', 50, 50, 0.5)]), 's.mrcs', 16, image_root=None)
    assert plan.micrographs[0].path == 'mic_a.mrc'
