"""The precision check of a loaded model on the MI355X: the delta_stats kernel against numpy, tpz_model_calibrate against the two
forwards it claims to compare, the per-model exact flag on the scoring and the denoising drivers, and `--precision-check` through
the CLI.  Every equality below is exact: calibrate runs the very passes forward runs, and delta_stats reduces maxima (order-free)
in fp32 and the squares in fp64 (1e-12 relative covers any summation order of <= 2^22 non-negative float64 terms)."""
import os
import shutil
import warnings

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden_sd, load_golden

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 63, 64, 65, 255, 256, 257, 1023, 4099, 262147]
ALL_OFFSETS = [(i, j) for i in range(4) for j in range(4)]
SOME_OFFSETS = [(0, 0), (1, 1), (0, 3), (2, 1)]


# ---- delta_stats ------------------------------------------------------------------------------------------------------------
def _device_view(host: np.ndarray, offset: int) -> torch.Tensor:
    """host on the device, starting `offset` floats past a 16-byte boundary"""
    base = torch.empty(host.size + 8, dtype=torch.float32, device='cuda')
    lead = (-(base.data_ptr() // 4)) % 4 + offset
    view = base[lead:lead + host.size]
    assert view.data_ptr() % 16 == 4 * offset
    view.copy_(torch.from_numpy(host))
    return view


def _numpy_stats(a: np.ndarray, b: np.ndarray):
    with np.errstate(invalid='ignore'):
        diff = a - b                                        # float32
        d, r = np.abs(diff), np.abs(b)
    d[~np.isfinite(d)] = np.inf
    r[np.isnan(r)] = np.inf
    return d.max(), int(np.argmax(d)), r.max(), float((diff.astype(np.float64) ** 2).sum())


def _bits(stats: dict):
    """the figures as bytes (a NaN sum of squares equals itself)"""
    return {k: np.float64(v).tobytes() for k, v in stats.items()}


def _check(ctx, a, b, offsets, finite=True):
    want = _numpy_stats(a, b)
    for oa, ob in offsets:
        da, db = _device_view(a, oa), _device_view(b, ob)
        got = ctx.delta_stats(da, db)
        again = ctx.delta_stats(da, db)
        assert _bits(got) == _bits(again), (a.size, oa, ob, got, again)             # bit-identical from run to run
        assert np.float32(got['max_abs_delta']) == want[0] and got['argmax'] == want[1], (a.size, oa, ob, got, want)
        assert np.float32(got['max_abs_ref']) == want[2], (a.size, oa, ob, got, want)
        if finite:
            assert abs(got['sum_sq'] - want[3]) <= 1e-12 * want[3], (a.size, oa, ob, got['sum_sq'], want[3])


def _pair(n, seed):
    rs = np.random.RandomState(seed)
    a = rs.randn(n).astype(np.float32)
    b = (a + 1e-3 * rs.randn(n)).astype(np.float32)
    return a, b


@pytest.mark.parametrize('n', SIZES + [512 * 4096 + 4099])          # (the last: beyond the 512 workgroups the grid is capped at)
def test_delta_stats_against_numpy(gpu_ctx, n):
    a, b = _pair(n, n)
    _check(gpu_ctx, a, b, ALL_OFFSETS if n == 4099 else SOME_OFFSETS if n <= 262147 else [(0, 0), (1, 2)])


@pytest.mark.parametrize('n', [3, 257, 4099, 262147])
def test_delta_stats_argmax_is_the_first_index_of_the_maximum(gpu_ctx, n):
    for where in ([0], [n - 1], [n // 3, n - 1], [1, n // 2, n - 2]):      # index 0, index n - 1, ties across waves / workgroups
        a, b = _pair(n, 7 * n)
        for i in where:
            a[i], b[i] = 100.0, 0.0
        want = _numpy_stats(a, b)
        assert want[0] == 100.0 and want[1] == where[0]
        _check(gpu_ctx, a, b, SOME_OFFSETS)


@pytest.mark.parametrize('n', [65, 4099, 262147])
def test_delta_stats_non_finite_values(gpu_ctx, n):
    first, later = n // 5, n - 2
    # a NaN in a, a NaN in b, +inf at the same index in both (inf - inf): each is an infinite difference at the first such index
    for kind in ('nan_a', 'nan_b', 'inf_both'):
        a, b = _pair(n, 11 * n)
        for i in (later, first):
            if kind == 'nan_a':
                a[i] = np.nan
            elif kind == 'nan_b':
                b[i] = np.nan
            else:
                a[i] = b[i] = np.inf
        for oa, ob in SOME_OFFSETS:
            got = gpu_ctx.delta_stats(_device_view(a, oa), _device_view(b, ob))
            assert got['max_abs_delta'] == np.inf and got['argmax'] == first, (kind, n, oa, ob, got)
            assert (got['max_abs_ref'] == np.inf) == (kind != 'nan_a'), (kind, n, oa, ob, got)
        _check(gpu_ctx, a, b, [(0, 0), (3, 2)], finite=False)


def test_delta_stats_of_nothing_is_an_error(gpu_ctx):
    from topaz_amd._lib import TopazHipError
    e = torch.empty(0, dtype=torch.float32, device='cuda')
    with pytest.raises(TopazHipError, match='tpz_delta_stats'):
        gpu_ctx.delta_stats(e, e)
    with pytest.raises(ValueError):
        gpu_ctx.delta_stats(torch.zeros(4, device='cuda'), torch.zeros(5, device='cuda'))


# ---- calibrate: scoring networks ----------------------------------------------------------------------------------------------
def _filled(arch, sd):
    from topaz_amd.model.classifier import LinearClassifier
    m = LinearClassifier(arch, sd)
    m.eval(); m.fill(); m.cuda()
    return m


def _both_paths(ctx, model, xt):
    """(default forward, forward under ctx.set_exact(True)) of the SAME loaded model, as float32 arrays"""
    y = model(xt)[0, 0].cpu().numpy()
    ctx.set_exact(True)
    try:
        y32 = model(xt)[0, 0].cpu().numpy()
    finally:
        ctx.set_exact(False)
    return y, y32


class _Case:
    """one loaded model, one image, both forwards and the measured figure: computed once, shared, never modified"""

    def __init__(self, ctx, arch, sd, x):
        self.ctx, self.arch, self.sd, self.x = ctx, arch, sd, x
        self.xt = torch.from_numpy(x)[None, None].cuda()
        self.model = _filled(arch, sd)
        dm = self.model.device_model
        self.stats_before = dm.split_stats()
        self.r = self.model.calibrate(x, bar=0)
        self.stats_after = dm.split_stats()
        self.y, self.y32 = _both_paths(ctx, self.model, self.xt)
        self.stats_end = dm.split_stats()


@pytest.fixture(scope='module')
def case2d(gpu_ctx):
    from topaz_amd.model.factory import load_state_dict_from_pkg
    sd = {k: v.numpy() for k, v in load_state_dict_from_pkg('resnet8_u32.sav').items()}
    return _Case(gpu_ctx, 'resnet8', sd, np.random.RandomState(21).randn(96, 96).astype(np.float32))


@pytest.fixture(scope='module')
def case3d(gpu_ctx):
    from tools import synth_weights as sw
    sd = sw.calibrate_head(sw.resnet_sd_uncalibrated('resnet8', 32, 3, dims=3), (1.0, 0.0))
    sd = {k: (v.numpy() if hasattr(v, 'numpy') else np.asarray(v)) for k, v in sd.items()}
    return _Case(gpu_ctx, 'resnet8', sd, np.random.RandomState(22).randn(16, 20, 24).astype(np.float32))


def _figure_is_what_it_claims(c):
    r = c.r
    assert r['eligible'] and not r['overflow'] and not r['tripped'] and r['max_abs_delta'] > 0
    assert not c.model.device_model.exact
    diff = np.abs(c.y - c.y32)                                  # float32
    assert np.float32(r['max_abs_delta']) == diff.max(), (r, float(diff.max()))
    assert r['argmax'] == int(np.argmax(diff))
    assert np.float32(r['max_abs_ref']) == np.abs(c.y32).max()
    rms = np.sqrt(((c.y - c.y32).astype(np.float64) ** 2).sum() / diff.size)
    assert abs(r['rms_delta'] - rms) <= 1e-12 * rms
    # the counters did not move in calibrate, and the context was not left in exact mode: the default forward after it counted
    # one 2xf16 run, the forward under set_exact none
    assert c.stats_after == c.stats_before == (True, 0, 0)
    assert c.stats_end == (True, 1, 0)


def _trip_and_release(c):
    d = c.r['max_abs_delta']
    m = _filled(c.arch, c.sd)                                   # (a model of its own: the shared one is left as it is)
    dm = m.device_model
    assert np.array_equal(m(c.xt)[0, 0].cpu().numpy(), c.y)
    r = m.calibrate(c.x, bar=d / 2)
    assert r['tripped'] and dm.exact and r['max_abs_delta'] == d
    before = dm.split_stats()
    assert np.array_equal(m(c.xt)[0, 0].cpu().numpy(), c.y32)
    assert dm.split_stats() == before                           # never tried on the 2xf16 path: neither counter moved
    dm.set_exact(False)
    assert not dm.exact
    assert np.array_equal(m(c.xt)[0, 0].cpu().numpy(), c.y)
    assert dm.split_stats() == (True, before[1] + 1, before[2])
    fresh = _filled(c.arch, c.sd)
    r = fresh.calibrate(c.x, bar=2 * d)
    assert not r['tripped'] and not fresh.device_model.exact and r['max_abs_delta'] == d
    assert np.array_equal(fresh(c.xt)[0, 0].cpu().numpy(), c.y)


def test_calibrate_reports_the_distance_between_the_two_forwards(case2d):
    _figure_is_what_it_claims(case2d)


def test_calibrate_trips_above_the_bar_and_set_exact_releases(case2d):
    _trip_and_release(case2d)


def test_default_bar_is_wired(case2d):
    """The head is linear and applied in fp32, and range scaling depends on the input only: with classifier.weight / .bias times
    2^k both passes scale by an exact power of two, so the figure is 2^k * d exactly.  k: the smallest with 2^k * d above the bar."""
    from topaz_amd.runtime import DEFAULT_BAR
    d = case2d.r['max_abs_delta']
    k = 0
    while 2.0 ** k * d <= DEFAULT_BAR:
        k += 1
    assert k > 0 and 2.0 ** (k - 1) * d <= DEFAULT_BAR
    sd = dict(case2d.sd)
    for key in ('classifier.weight', 'classifier.bias'):
        sd[key] = (np.asarray(sd[key], dtype=np.float32) * np.float32(2.0 ** k))
    m = _filled('resnet8', sd)
    r = m.calibrate(case2d.x)
    print(f'd = {d:.9e}, k = {k}, 2^k d = {2.0 ** k * d:.9e}, measured {r["max_abs_delta"]:.9e}, bar {r["bar"]:.1e}')
    assert r['bar'] == DEFAULT_BAR
    assert r['tripped'] and m.device_model.exact
    assert r['max_abs_delta'] == 2.0 ** k * d


def test_calibrate_3d_reports_the_distance_between_the_two_forwards(case3d):
    _figure_is_what_it_claims(case3d)


def test_calibrate_3d_trips_above_the_bar_and_set_exact_releases(case3d):
    _trip_and_release(case3d)


def test_default_tile_and_batch_of_one(gpu_ctx, case2d):
    m = _filled(case2d.arch, case2d.sd)
    r = m.calibrate(bar=0)                                      # RandomState(0).randn(256, 256)
    from topaz_amd.precision import default_tile
    assert r == m.device_model.calibrate(torch.from_numpy(default_tile(2))[None, None], bar=0)
    assert r['eligible'] and 0 < r['max_abs_delta'] < 1e-4
    with pytest.raises(ValueError):
        m.device_model.calibrate(torch.zeros(2, 1, 96, 96), bar=0)


# ---- calibrate: denoisers honour the model flag -------------------------------------------------------------------------------
def _denoiser_honours_the_flag(ctx, d, net_input, run):
    dm = d.model.device_model
    y = run()
    ctx.set_exact(True)
    try:
        y32 = run()
    finally:
        ctx.set_exact(False)
    assert not np.array_equal(y, y32)
    own = d.model.calibrate(net_input, bar=0)
    assert own['eligible'] and not own['overflow'] and own['max_abs_delta'] > 0 and not dm.exact
    r = d.model.calibrate(net_input, bar=own['max_abs_delta'] / 2)
    assert r['tripped'] and dm.exact
    before = dm.split_stats()
    assert np.array_equal(run(), y32)
    assert dm.split_stats() == before
    dm.set_exact(False)
    assert np.array_equal(run(), y)
    assert dm.split_stats() == (True, before[1] + 1, before[2])


def test_denoise_2d_honours_the_model_flag(gpu_ctx):
    from topaz_amd.denoise import Denoise
    d = Denoise('unet-small')
    x = np.random.RandomState(23).randn(96, 80).astype(np.float32)          # odd pooled sizes; 2 x 2 patches of 48 + 2 * 16
    _denoiser_honours_the_flag(gpu_ctx, d, x, lambda: d.denoise(x, patch_size=48, padding=16))


def test_denoise_3d_honours_the_model_flag(gpu_ctx):
    from topaz_amd.denoise import Denoise3D
    from topaz_amd.denoising.models import DenoiseNet
    z = load_golden('denoise3d_unet3d_nf8')
    d = Denoise3D(DenoiseNet('unet-3d', golden_sd(z)))
    tomo = z['tomo']
    tile = np.random.RandomState(24).randn(32, 32, 32).astype(np.float32)
    _denoiser_honours_the_flag(gpu_ctx, d, tile, lambda: d.denoise(tomo, 32, 16, verbose=False))


# ---- a program without a 2xf16 path --------------------------------------------------------------------------------------------
def test_model_without_a_split_path_is_not_eligible(gpu_ctx):
    """a layer with an activation slope > 1 stays on its fp32 kernel (the 2xf16 epilogue applies max(v, slope * v)): a program
    of such layers alone has no 2xf16 path"""
    from topaz_amd.runtime import DeviceModel, LayerProgram
    rs = np.random.RandomState(25)
    prog = LayerProgram(2)
    h = prog.conv(0, rs.randn(8, 1, 3, 3).astype(np.float32) * 0.3, rs.randn(8).astype(np.float32) * 0.1, pad=1, slope=2.0)
    prog.conv(h, rs.randn(8, 8, 3, 3).astype(np.float32) * 0.1, rs.randn(8).astype(np.float32) * 0.1, pad=1, slope=1.5)
    dm = DeviceModel(prog, gpu_ctx)
    assert dm.split_stats()[0] is False
    x = torch.from_numpy(rs.randn(1, 1, 40, 40).astype(np.float32))
    r = dm.calibrate(x, bar=1e-30)
    assert r['eligible'] is False and not r['tripped'] and not r['overflow'] and not dm.exact
    assert r['max_abs_delta'] == 0 and r['sum_sq'] == 0 and r['rms_delta'] == 0
    assert dm.split_stats() == (False, 0, 0)


# ---- the CLI -----------------------------------------------------------------------------------------------------------------
USER_MODEL = os.path.join(GOLDEN, 'user_model_resnet8_bn_u16.sav')


def _extract(tmp_path, tag, *flags):
    from topaz_amd.main import main
    mic = tmp_path / 'mic_a.mrc'
    if not mic.exists():
        shutil.copy(os.path.join(GOLDEN, 'cli', 'mic_a.mrc'), mic)
    out = tmp_path / f'picks_{tag}.txt'
    main(['extract', '-m', USER_MODEL, '-r', '8', '-d', '0', '-o', str(out), *flags, str(mic)])
    return open(out, 'rb').read()


def _precision_lines(text):
    return [line for line in text.split('\n') if line.startswith('# precision check of')]


def test_cli_segment_denoise_denoise3d_check_model_files(gpu_ctx, tmp_path, capfd):
    """the other three commands: a model file is checked once under the default `auto` (one line: `segment -v`, and `denoise` /
    `denoise3d`, which always narrate on stderr), not at all under `never`, and the files written are byte-identical"""
    from topaz_amd.main import main
    cli = os.path.join(GOLDEN, 'cli')
    for name in ('mic_a.mrc', 'tomo.mrc'):
        shutil.copy(os.path.join(cli, name), tmp_path / name)
    mic, tomo = str(tmp_path / 'mic_a.mrc'), str(tmp_path / 'tomo.mrc')
    jobs = {
        'segment': (['segment', '-m', USER_MODEL, '-v', mic], '-o', 'mic_a.tiff'),
        'denoise': (['denoise', '-m', os.path.join(GOLDEN, 'user_model_unet_b11t5_nf16.sav'), '-s', '96', '-p', '24', mic], '-o',
                    'mic_a.mrc'),
        'denoise3d': (['denoise3d', '-m', os.path.join(cli, 'unet3d_nf8_state.sav'), '--base-kernel-width', '7', '-s', '32', '-p',
                       '16', '-d', '0', tomo], '-o', 'tomo.mrc'),
    }
    with warnings.catch_warnings():
        warnings.filterwarnings('error', message='topaz_amd: the 2xf16 path', category=RuntimeWarning)
        for command, (argv, out_flag, out_name) in jobs.items():
            written = {}
            for mode, n_lines in ((None, 1), ('never', 0), ('always', 1)):
                dest = tmp_path / f'{command}_{mode}'
                capfd.readouterr()
                main(argv + [out_flag, str(dest)] + (['--precision-check', mode] if mode else []))
                assert len(_precision_lines(capfd.readouterr().err)) == n_lines, (command, mode)
                written[mode] = open(dest / out_name, 'rb').read()
            assert written[None] == written['never'] == written['always'] and len(written[None]) > 1024, command


def test_cli_precision_check(gpu_ctx, tmp_path, capfd, monkeypatch):
    with warnings.catch_warnings():
        warnings.filterwarnings('error', message='topaz_amd: the 2xf16 path', category=RuntimeWarning)   # no trip at the default bar
        never = _extract(tmp_path, 'never', '--precision-check', 'never')
        default = _extract(tmp_path, 'default')
        assert never == default and len(never.split(b'\n')) > 3
        assert _precision_lines(capfd.readouterr().err) == []           # silent without -v
        assert _extract(tmp_path, 'v', '-v') == never
        lines = _precision_lines(capfd.readouterr().err)
        assert len(lines) == 1 and 'max |delta|' in lines[0] and USER_MODEL in lines[0]
        assert _extract(tmp_path, 'v_never', '-v', '--precision-check', 'never') == never
        assert _precision_lines(capfd.readouterr().err) == []
    # the same job on the fp32 kernels: the context switched to exact mode once the model is loaded, nothing checked
    import topaz_amd.extract as ex
    with monkeypatch.context() as mp:
        mp.setattr(ex, 'check_loaded_model', lambda *a, **k: gpu_ctx.set_exact(True))
        try:
            exact = _extract(tmp_path, 'exact')
        finally:
            gpu_ctx.set_exact(False)
    # a bar below this model's figure: the warning names the figure, the bar and the consequence; the picks are the fp32 ones
    import topaz_amd.runtime as rt
    monkeypatch.setattr(rt, 'DEFAULT_BAR', 1e-12)
    with pytest.warns(RuntimeWarning, match=r'above the bar of 1\.0e-12.*fp32 matrix-core kernels, several times slower'):
        tripped = _extract(tmp_path, 'tripped')
    assert tripped == exact
