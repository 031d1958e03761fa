"""Every tile walk writes every cell: the suite's A/B tests under POISONED workspace (Context.set_poison).

The workspace pools hand the same buffers to the same sequence of requests and never clear them, so the second run of a layer
finds the first run's bytes -- the right answer -- wherever it fails to store, and `torch.equal(first, second)` passes.  With the
switch on, every buffer is 0xFF bytes (f16 / f32 / f64 NaN, 64-bit keys at their maximum, ints -1) when it is taken and the
result tensors are NaN: a tile that is never computed, a cell that is never stored, or a never-written cell that reaches a result
shows as a non-finite output.  Every case also asserts, through Context.walk_stats(), that it took the walk it is there for.

Tolerances are the ones the existing tests hold the same operations to: single layers 1e-4 * (1 + |ref|) against float64
(test_gpu_split._err), networks 1e-4 absolute, fixture-backed drivers by calling the existing test's own check."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_split as tgs
from conftest import GOLDEN, golden_sd, load_golden
from oracle import denoising as oden
from oracle import nms as onms
from oracle import scoring as oscoring

pytestmark = pytest.mark.gpu
ATOL = 1e-4
MIB = 1 << 20
FORMS = ('plain', 'raster', 'persistent', 'weights_resident', 'multi')


@pytest.fixture
def poisoned(gpu_ctx):
    """poison on for the test; every switch a test here may touch is back at its default afterwards"""
    gpu_ctx.set_poison(True)
    try:
        yield gpu_ctx
    finally:
        gpu_ctx.set_poison(False)
        gpu_ctx.set_persist(1, 0)
        gpu_ctx.set_raster(True)
        gpu_ctx.set_rw(True)
        gpu_ctx.set_batch(8)
        gpu_ctx.set_roi(True)
        gpu_ctx.set_lanes(True)
        gpu_ctx.set_exact(False)
        gpu_ctx.set_tiling(40 << 20, 4096)


def _walks(ctx, fn):
    """(fn(), the conv launches it made by walk form)"""
    w0 = ctx.walk_stats()
    out = fn()
    w1 = ctx.walk_stats()
    return out, {k: w1[k] - w0[k] for k in FORMS}


def _only(form, n=1):
    return {k: (n if k == form else 0) for k in FORMS}


def _finite(t):
    return bool(torch.isfinite(t).all()) if torch.is_tensor(t) else bool(np.isfinite(t).all())


# ---- a. the switch itself ----------------------------------------------------------------------------------------------------
def test_poison_fills_the_whole_pool_buffer_and_counts_nothing_as_a_launch(gpu_ctx):
    """On a context of its own (its pool holds what one conv_split left, nothing else): with poison on a buffer taken from the
    pool is 0xFF over its whole rounded size -- a cached one as well as a new one --, the fill counters grow by exactly the
    buffers taken and their sizes, and a conv_split issues as many launches as without; with poison off nothing is filled and
    no counter moves."""
    from topaz_amd import runtime as rt
    ctx = rt.Context(0)
    try:
        g = torch.Generator().manual_seed(1)
        x = torch.randn(16, 40, 41, generator=g)
        w = (torch.randn(64, 16, 3, 3, generator=g) / 12).numpy()

        def conv():
            n0 = ctx.launches()
            y, ovf = rt.conv_split(x, w, None, pad=1, slope=1.0, ctx=ctx)
            assert not ovf
            return y, ctx.launches() - n0

        assert ctx.poison_stats() == {'on': False, 'fills': 0, 'bytes': 0}
        y_off, n_off = conv()                                   # dirties the pool: split cells of x and of y
        pool = ctx.pool_stats()
        assert pool['buffers'] >= 2 and pool['buffers_in_use'] == 0
        dirt = ctx.workspace_peek(16)
        assert dirt.size == MIB and not (dirt == 0xFF).all(), 'the pool was expected to hold the conv_split\'s cells'
        assert ctx.poison_stats() == {'on': False, 'fills': 0, 'bytes': 0}
        assert ctx.pool_stats() == pool

        ctx.set_poison(True)
        big = pool['bytes'] + MIB + 5                           # larger than anything pooled: a new buffer
        for nbytes in (16, MIB + 1, big):
            p0, s0 = ctx.pool_stats(), ctx.poison_stats()
            buf = ctx.workspace_peek(nbytes)
            p1, s1 = ctx.pool_stats(), ctx.poison_stats()
            rounded = (nbytes + MIB - 1) // MIB * MIB
            size = s1['bytes'] - s0['bytes']                    # the whole size of the buffer that was taken
            assert s1['on'] and s1['fills'] - s0['fills'] == 1
            assert size >= rounded and size % MIB == 0
            assert buf.size == rounded and (buf == 0xFF).all(), (nbytes, int((buf != 0xFF).sum()))
            assert p1['buffers_in_use'] == 0
            if p1['buffers'] == p0['buffers'] + 1:              # a new buffer: all of it was copied back
                assert size == rounded and p1['bytes'] - p0['bytes'] == rounded
            else:
                assert p1 == p0
        assert ctx.pool_stats()['bytes'] >= big                 # (the last one was new)
        s0 = ctx.poison_stats()
        y_on, n_on = conv()
        s1 = ctx.poison_stats()
        assert n_on == n_off
        assert s1['fills'] - s0['fills'] == 2 and s1['bytes'] - s0['bytes'] >= 2 * MIB      # the split copies of x and of y
        assert torch.equal(y_on, y_off) and _finite(y_on)

        ctx.set_poison(False)
        s0 = ctx.poison_stats()
        conv()
        ctx.workspace_peek(MIB + 1)
        assert ctx.poison_stats() == dict(s0, on=False)
    finally:
        ctx.lib.tpz_ctx_destroy(ctx.handle)


# ---- b. single 2xf16 layers, every walk of the same launch -------------------------------------------------------------------
# Output sizes: the smallest with >= 512 tiles of the 8-wave tile (the patch raster's threshold), a tiles_x that is no multiple
# of 8 (padding columns of the raster's 8 x 4 blocks), where the dilation allows a tiles_y that is no multiple of 4 (padding
# rows), and a last tile that overhangs in both axes.  tiles_y = ceil(Ho / (TH * dil)) * dil, tiles_x = ceil(Wo / TW).
# cin = 8 (one cell) keeps the float64 reference cheap: pick_split chooses the kernel from (k, dil, cout, epilogue) alone.
# (id, cin, cout, k, dil, Ho, Wo, epilogue, slope, (TH, TW), tiles (y, x), raster applies, persistent applies)
LAYERS = [
    ('k3_d2_c128', 8, 128, 3, 2, 470, 603, 'plain', 0.0, (16, 32), (30, 19), True, True),
    ('k3_d2_c64', 8, 64, 3, 2, 470, 905, 'plain', 0.1, (16, 48), (30, 19), True, True),
    ('k3_d4_c128_res', 8, 128, 3, 4, 500, 530, 'res', 0.0, (16, 32), (32, 17), True, True),
    # dilation 8: 370 rows are 2 bands of 128 and 114 more -- in the last band the phases 2 .. 7 have 14 rows, 0 and 1 have 15
    ('k3_d8_c128_res_post', 8, 128, 3, 8, 370, 710, 'res_post', 0.0, (16, 32), (24, 23), True, True),
    ('k5_d4_c256', 8, 256, 5, 4, 500, 530, 'plain', 0.0, (16, 32), (32, 17), True, True),          # two co-groups: grid z = 2
    ('k5_d4_c256_head', 8, 256, 5, 4, 500, 530, 'head', 0.0, (16, 32), (32, 17), True, False),     # (no persistent form)
    ('k5_d2_c32', 8, 32, 5, 2, 470, 603, 'plain', 0.1, (16, 32), (30, 19), True, True),            # four steps per stage
    ('k11_d1_c64', 8, 64, 11, 1, 490, 1060, 'plain', 0.0, (16, 64), (31, 17), True, True),
    # below the raster's threshold (40 and 100 tiles); the persistent walk over odd chunk counts and short last chunks
    ('72_to_100_k3_d4', 72, 100, 3, 4, 93, 135, 'plain', 0.0, (16, 32), (8, 5), False, True),
    # 3 cells in chunks of 2: the K loop of the short last chunk is too short to hold the whole fetch of the next tile, so the
    # library launches this layer one tile per workgroup whatever tpz_ctx_set_persist says (rt_exec.hip launch_split: next_ok)
    ('24_to_48_k3_d1', 24, 48, 3, 1, 75, 298, 'plain', 0.1, (8, 32), (10, 10), False, False),
    # ... and the same tile with whole chunks, which does walk persistently
    ('32_to_48_k3_d1', 32, 48, 3, 1, 75, 298, 'plain', 0.1, (8, 32), (10, 10), False, True),
]
FULL_REF_FLOP = 8e9         # above this the float64 reference is computed on windows


def _ref_windows(Ho, Wo, TH, TW, dil, tiles):
    """(r0, r1, c0, c1) output windows: the first tile's band of rows x its columns, the last band of rows (every row phase of
    it: the last `dil` tile rows; the last two bands without dilation) over all columns, the last two tile columns over all
    rows, and one interior tile's rows and columns"""
    ty, tx = tiles
    band, bands = TH * dil, ty // dil
    last_rows = (bands - (2 if dil == 1 else 1)) * band
    mb, mc = bands // 2, tx // 2
    return [(0, min(band, Ho), 0, min(TW, Wo)), (last_rows, Ho, 0, Wo), (0, Ho, (tx - 2) * TW, Wo),
            (mb * band, (mb + 1) * band, mc * TW, (mc + 1) * TW)]


@pytest.mark.parametrize('case', LAYERS, ids=[c[0] for c in LAYERS])
def test_every_walk_of_a_layer_writes_every_cell(poisoned, case):
    """(i) one workgroup per tile in XCD row-major order, (ii) the patch raster, (iii) persistent workgroups (8, 24 and one
    per grid slot): under poison every output element of every run is finite, (ii) and (iii) equal (i) bit for bit, (i) is
    within 1e-4 * (1 + |ref|) of float64 F.conv2d, and walk_stats names the walk each run took."""
    from topaz_amd import runtime as rt
    ctx = poisoned
    name, cin, cout, k, dil, Ho, Wo, epi, slope, (TH, TW), tiles, rasters, persists = case
    span = dil * (k - 1)
    assert tiles == ((Ho + TH * dil - 1) // (TH * dil) * dil, (Wo + TW - 1) // TW)
    assert Ho % (TH * dil) and Wo % TW, 'the last tile must overhang in both axes'
    if rasters:
        assert tiles[0] * tiles[1] >= 512 and tiles[1] % 8
    g = torch.Generator().manual_seed(1234 + cout + k * dil)
    x = torch.randn(cin, Ho + span, Wo + span, generator=g) * 2
    w = torch.randn(cout, cin, k, k, generator=g) / np.sqrt(cin * k * k)
    b = torch.randn(cout, generator=g)
    kw = dict(dil=dil, slope=slope)
    res = ps = pt = hw = None
    if epi in ('res', 'res_post'):
        res = torch.randn(cout, Ho + 4, Wo + 4, generator=g)
        kw.update(res=res.cuda(), res_crop=2)
    if epi == 'res_post':
        ps, pt = 1 + 0.1 * torch.randn(cout, generator=g), torch.randn(cout, generator=g)
        kw.update(post_scale=ps.numpy(), post_shift=pt.numpy())
    if epi == 'head':
        hw = torch.randn(cout, generator=g) / np.sqrt(cout)
        kw.update(head_w=hw.numpy(), head_b=0.7)
    xd = x.cuda()

    def run(persist, wgs, raster, form):
        ctx.set_persist(persist, wgs)
        ctx.set_raster(raster)
        (y, ovf), took = _walks(ctx, lambda: rt.conv_split(xd, w.numpy(), b.numpy(), **kw))
        label = (name, 'persist', persist, wgs, 'raster', raster)
        assert took == _only(form), (label, took)
        assert not ovf, label
        assert _finite(y), (label, int((~torch.isfinite(y)).sum()))
        return y

    y0 = run(0, 0, False, 'plain')
    assert y0.shape == (1 if epi == 'head' else cout, Ho, Wo)
    if rasters:
        y = run(0, 0, True, 'raster')
        assert torch.equal(y0, y), (name, 'raster', float((y0 - y).abs().max()))
    else:
        run(0, 0, True, 'plain')                     # (fewer than 512 tiles: the switch changes nothing)
    if epi != 'head':
        for wgs in (8, 24, 0):
            y = run(2, wgs, True, 'persistent' if persists else 'raster' if rasters else 'plain')
            assert torch.equal(y0, y), (name, 'persistent', wgs, float((y0 - y).abs().max()))
    del y

    def ref64(r0, r1, c0, c1):
        xs = x[None, :, r0:r1 + span, c0:c1 + span].double()
        y = F.conv2d(xs, w.double(), b.double(), dilation=dil)[0]
        if res is not None:
            y = y + res[:, 2 + r0:2 + r1, 2 + c0:2 + c1].double()
        if ps is not None:
            y = y * ps.double()[:, None, None] + pt.double()[:, None, None]
        y = tgs._act(y, slope)
        if hw is not None:
            y = (y * hw.double()[:, None, None]).sum(0, keepdim=True) + 0.7
        return y

    y0 = y0.cpu()
    full = 2.0 * cout * cin * k * k * Ho * Wo <= FULL_REF_FLOP
    for (r0, r1, c0, c1) in ([(0, Ho, 0, Wo)] if full else _ref_windows(Ho, Wo, TH, TW, dil, tiles)):
        e = tgs._err(y0[:, r0:r1, c0:c1], ref64(r0, r1, c0, c1))
        print(f'{name} rows {r0}:{r1} cols {c0}:{c1}: err vs float64 (scaled by 1 + |ref|) {e:.2e}')
        assert e <= 1e-4, (name, (r0, r1, c0, c1), e)


# ---- c. weights-resident kernel -------------------------------------------------------------------------------------------------
def test_weights_resident_walk_writes_every_cell(poisoned):
    """resnet16_u32 (3x3 32 -> 32 layers at dilation 1, 2 and 4, plain / residual) on a 203 x 333 image: ragged last tiles of the
    8 x 32 tile in both axes.  Finite, within the bound test_gpu_scoring holds the two kernels to -- of the oracle and of each
    other --, weights-resident launches with the switch on only, no fp32 re-run."""
    from topaz_amd.model.factory import load_model
    ctx = poisoned
    m = load_model('resnet16_u32')
    m.eval(); m.fill(); m.cuda()
    sd = {k: v.numpy() for k, v in m.state_dict().items()}
    x = np.random.RandomState(203).randn(203, 333).astype(np.float32)
    ref = oscoring.score('resnet16', sd, x)
    tol = max(ATOL, 3e-6 * float(np.abs(ref).max()))
    xt = torch.from_numpy(x)[None, None].cuda()
    st0 = m.device_model.split_stats()
    y_rw, took_rw = _walks(ctx, lambda: m(xt)[0, 0].cpu().numpy())
    ctx.set_rw(False)
    y_gen, took_gen = _walks(ctx, lambda: m(xt)[0, 0].cpu().numpy())
    st1 = m.device_model.split_stats()
    assert took_rw['weights_resident'] >= 9 and took_gen['weights_resident'] == 0, (took_rw, took_gen)
    assert sum(took_rw.values()) == sum(took_gen.values())
    assert st1[1] == st0[1] + 2 and st1[2] == st0[2], 'fp32 re-run'
    assert _finite(y_rw) and _finite(y_gen)
    e_rw, e_gen, e_ab = np.abs(y_rw - ref).max(), np.abs(y_gen - ref).max(), np.abs(y_rw - y_gen).max()
    print(f'resnet16_u32 203 x 333: |rw - oracle| {e_rw:.2e}  |general - oracle| {e_gen:.2e}  |rw - general| {e_ab:.2e}')
    assert e_rw <= tol and e_gen <= tol and e_ab <= tol


# ---- d. batched grid, lanes and ROI -------------------------------------------------------------------------------------------
def test_batched_grid_lanes_and_windows_write_every_cell(poisoned):
    """700 x 650 through the seeded 48-filter U-Net in 256 / 64 patches: patches of 320, 384 and 252 / 202 pixels in one batch
    (padding workgroups between the entries of the batched grid).  Batched against single patches, lanes on against off,
    patch windows on against off: finite and bit-identical as test_gpu_denoise asserts without poison, within 1e-4 of the
    oracle, batched-grid launches with batching on only."""
    from tools import synth_weights as sw
    from topaz_amd.denoise import Denoise
    from topaz_amd.denoising.models import DenoiseNet
    ctx = poisoned
    sd = sw.unet_sd(11)
    dn = Denoise(DenoiseNet('unet', sd))
    x = np.random.RandomState(5).randn(700, 650).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    dm = dn.model.device_model
    st0 = dm.split_stats()

    def run(batch, lanes, roi):
        ctx.set_batch(batch); ctx.set_lanes(lanes); ctx.set_roi(roi)
        y, took = _walks(ctx, lambda: dn.denoise_device(xd, 256, 64).cpu().numpy())
        assert _finite(y), ((batch, lanes, roi), int((~np.isfinite(y)).sum()))
        return y, took

    base, took_base = run(8, True, True)
    single, took_single = run(0, True, True)
    one_stream, took_one = run(8, False, True)
    whole, took_whole = run(8, True, False)
    single_whole, _ = run(0, False, False)
    st1 = dm.split_stats()
    assert took_base['multi'] > 0 and took_one['multi'] > 0 and took_whole['multi'] > 0, (took_base, took_one, took_whole)
    assert took_single['multi'] == 0 and took_single['plain'] > 0, took_single
    assert st1[1] == st0[1] + 5 and st1[2] == st0[2], 'fp32 re-run'
    for label, y in (('batch 0', single), ('lanes off', one_stream), ('roi off', whole), ('all off', single_whole)):
        assert np.array_equal(base, y), (label, float(np.abs(base - y).max()))
    ref = oden.denoise('unet', sd, x, patch_size=256, padding=64)
    assert np.abs(base - ref).max() <= ATOL


# ---- e. whole programs on a warm, poisoned pool -------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def warm_pools(gpu_ctx):
    """an unrelated network through every kind of pool first (ctx, lanes, batched passes), poison off: the buffers the programs
    below take held fp32 planes and split cells of other shapes before they are poisoned"""
    from tools import synth_weights as sw
    from topaz_amd.denoise import Denoise
    from topaz_amd.denoising.models import DenoiseNet
    from topaz_amd.model.classifier import LinearClassifier
    x = torch.from_numpy(np.random.RandomState(77).randn(300, 280).astype(np.float32)).cuda()
    dn = Denoise(DenoiseNet('unet', sw.unet_sd(12)))
    try:
        for batch in (8, 0):
            gpu_ctx.set_batch(batch)
            dn.denoise_device(x, 128, 32)
        for exact in (False, True):
            gpu_ctx.set_exact(exact)
            m = LinearClassifier('resnet8', oscoring.synthetic_resnet_sd('resnet8', 64, 7))
            m.eval(); m.fill(); m.cuda()
            m(x[None, None])
    finally:
        gpu_ctx.set_batch(8)
        gpu_ctx.set_exact(False)
    torch.cuda.synchronize()


def _scorer(model):
    model.eval(); model.fill(); model.cuda()
    return model.device_model, lambda x: model(torch.from_numpy(x)[None, None].cuda())[0, 0].cpu().numpy()


def _program(name):
    """(device model, [(label, run() -> numpy, expected)]) of a golden fixture"""
    from topaz_amd.denoise import Denoise, Denoise3D
    from topaz_amd.denoising.models import DenoiseNet
    from topaz_amd.model.classifier import LinearClassifier
    from topaz_amd.model.factory import load_model
    from topaz_amd.model.utils import predict_in_patches
    z = load_golden(name)
    if name.startswith('score_'):
        tag = name[len('score_'):]
        if tag == 'patched_resnet8_u32':
            m = load_model('resnet8_u32')
            dm, _ = _scorer(m)
            size = int(z['patch']) + 2 * (m.width // 2)
            return dm, [('patched', lambda: predict_in_patches(m, torch.from_numpy(z['x0'])[None, None], size, use_cuda=True)[0, 0],
                         z['y0'])]
        if tag == 'resnet8_u32':
            m = load_model(tag)
        elif os.path.exists(os.path.join(GOLDEN, f'user_model_{tag}.sav')) and 'pooling' in z.files:
            m = load_model(os.path.join(GOLDEN, f'user_model_{tag}.sav'))            # (conv stacks trained with --pooling)
        else:
            m = LinearClassifier(str(z['arch']), golden_sd(z))
        dm, score = _scorer(m)
        runs, k = [], 0
        while f'x{k}' in z.files:
            runs.append((f'x{k}', (lambda x: lambda: score(x))(z[f'x{k}']), z[f'y{k}']))
            k += 1
        return dm, runs
    if name == 'denoise2d_unet3':
        d = Denoise(os.path.join(GOLDEN, 'user_model_unet3.sav'))
        return d.model.device_model, [('whole', lambda: d.denoise(z['x'], -1), z['whole']),
                                      ('p96_24', lambda: d.denoise(z['x'], 96, 24), z['p96_24'])]
    if name == 'denoise2d_unet_b11t5_nf16':
        d = Denoise(DenoiseNet('unet', golden_sd(z)))
        return d.model.device_model, [('whole', lambda: d.denoise(z['x'], -1), z['whole']),
                                      ('p48_20', lambda: d.denoise(z['x'], 48, 20), z['p48_20'])]
    assert name == 'denoise3d_unet3d_nf8'
    d = Denoise3D(DenoiseNet('unet-3d', golden_sd(z)))
    return d.model.device_model, [('p32_16', lambda: d.denoise(z['tomo'], 32, 16, verbose=False), z['p32_16']),
                                  ('small', lambda: d.denoise(z['small'], -1, verbose=False), z['small_whole'])]


PROGRAMS = ['score_resnet8_u32', 'score_resnet16_u16', 'score_conv127_max_bn_u16', 'score_conv31_avg_u32',
            'score_patched_resnet8_u32', 'score_resnet8_3d_bn_u8', 'score_conv31_3d_max_bn_u8', 'denoise2d_unet3',
            'denoise2d_unet_b11t5_nf16', 'denoise3d_unet3d_nf8']


@pytest.mark.parametrize('exact', [False, True], ids=['2xf16', 'exact_fp32'])
@pytest.mark.parametrize('name', PROGRAMS)
def test_programs_on_a_warm_poisoned_pool(warm_pools, poisoned, name, exact):
    """the reference's own outputs at 1e-4, every temporary tensor NaN before its producer runs: poison in cells that are
    legitimately never read (channels past the last of a cell, rows outside a window) changes nothing -- finite, no f16-range
    flag and so no fp32 re-run"""
    ctx = poisoned
    dm, runs = _program(name)
    ctx.set_exact(exact)
    for label, run, want in runs:
        st0 = dm.split_stats()
        y = np.asarray(run())
        st1 = dm.split_stats()
        assert y.shape == want.shape and _finite(y), (name, label, int((~np.isfinite(y)).sum()))
        assert st1[2] == st0[2], (name, label, 'an activation was flagged beyond the f16 range: fp32 re-run')
        if st0[0] and not exact:
            assert st1[1] > st0[1], (name, label, 'expected the 2xf16 path')
        if exact:
            assert st1[1] == st0[1]
        err = float(np.abs(y - want).max())
        print(f'{name} {label} exact={exact}: max |gpu - reference| {err:.2e}')
        assert err <= ATOL, (name, label, err)


@pytest.mark.parametrize('exact', [False, True], ids=['2xf16', 'exact_fp32'])
def test_tiled_scoring_on_a_poisoned_pool_equals_the_whole_image(warm_pools, poisoned, exact):
    """tpz_ctx_set_tiling(1, tile), as test_gpu_scoring forces it: halo-grown tiles through per-tile workspace, stitched --
    identical bits to the whole-image pass"""
    from topaz_amd.model.factory import load_model
    ctx = poisoned
    dm, score = _scorer(load_model('resnet8_u32'))
    x = np.round(np.random.RandomState(5).randn(257, 199) * 300 + 2500).astype(np.float32)
    ctx.set_exact(exact)
    st0 = dm.split_stats()
    whole = score(x)
    ctx.set_tiling(1, 128)
    tiled = score(x)
    st1 = dm.split_stats()
    assert whole.shape == x.shape and _finite(whole) and _finite(tiled)
    assert st1[2] == st0[2] and st1[1] == st0[1] + (0 if exact else 2)
    assert np.array_equal(whole, tiled)


# ---- f. drivers outside the convs that take workspace ---------------------------------------------------------------------------
def _pow2(n):
    return n > 0 and n & (n - 1) == 0


def test_nms_under_poison(poisoned):
    """pick counts that are no power of two: the tail of the sort buffer behind the candidates is filled by fill_u64_kernel,
    and 0xFF keys left there would sort as the largest.  Bit-exact against the C restatement of the reference's loop."""
    from topaz_amd import runtime as rt
    rs = np.random.RandomState(17)
    for shape, r, thr in (((257, 300), 5, -0.3), ((33, 500), 8, 0.2), ((100, 90), 3, 1.0)):
        x = rs.randn(*shape).astype(np.float32)
        x[rs.rand(*shape) < 0.05] = 0.5
        so, co = onms.nms2d(x, r, thr)
        s, c = rt.nms(torch.from_numpy(x), r, thr)
        assert len(so) > 2 and not _pow2(len(so)) and not _pow2(int((x > thr).sum())), (shape, len(so))
        assert np.array_equal(c.cpu().numpy(), co) and np.array_equal(s.cpu().numpy(), so), shape
    for shape, r, scale, thr in (((20, 24, 28), 2, 1.0, 0.5), ((9, 40, 33), 3, 1.5, -0.2)):
        v = rs.randn(*shape).astype(np.float32)
        v[rs.rand(*shape) < 0.05] = 0.75
        so, co = onms.nms3d(v, r, scale, thr)
        s, c = rt.nms(torch.from_numpy(v), r, thr, scale=scale)
        assert len(so) > 2 and not _pow2(len(so)) and not _pow2(int((v > thr).sum())), (shape, len(so))
        assert np.array_equal(c.cpu().numpy(), co) and np.array_equal(s.cpu().numpy(), so), shape


def test_prefilters_under_poison(poisoned):
    """tpz_lowpass_2d (float64 operator and intermediate buffers) and tpz_tile_filter_2d / tpz_spatial_cov_2d (partials,
    covariances, weights) against denoise_prefilter.npz, with the existing tests' own bars"""
    import test_gpu_denoise_prefilter as tpf
    tpf.test_fixture_lowpass_cases(poisoned)
    tpf.test_fixture_deconvolve_cases(poisoned)


def test_particle_stack_resize_under_poison(poisoned, tmp_path):
    """crop / operator / product buffers of tpz_particle_stack: the 32 -> 15 resize golden"""
    import test_gpu_particle_stack as tps
    tps.test_resize_golden(poisoned, 15, tmp_path)


def test_resample_plan_under_poison(poisoned):
    """the intermediate U of a ResamplePlan run at a tile-edge shape: P one above the tile in stage 2, ragged K"""
    import test_gpu_resample as trs
    trs._check((130, 20), 1, (trs.T + 1, 9))
    trs._check((2 * trs.T, 3 * trs.T + trs.KS), 1, (trs.T + 2, trs.T + 72))


def test_order_stats_mean_std_and_gmm_under_poison(poisoned):
    """the radix-select histogram (64-bit counters) at n = 257, the reduction partials of mean / std on 37 x 41 pixels against
    float64, and the parameter / output blocks of the mixture fits on `small`"""
    import test_gpu_preprocess_stream as tpp
    from topaz_amd import runtime as rt
    tpp.test_order_stats_and_quantiles_equal_numpy(poisoned, 257)
    x = torch.from_numpy(np.random.RandomState(37).randn(37, 41).astype(np.float32)) * 3 + 100
    m, s = rt.mean_std(x, unbiased=True)
    assert abs(m - x.double().mean().item()) < 1e-4 and abs(s - x.double().std().item()) < 1e-5
    m, s = rt.mean_std(x, unbiased=False)
    assert abs(s - x.numpy().astype(np.float64).std()) < 1e-5
    tpp.test_fused_fit_equals_gmm_fit_bit_for_bit(poisoned, 'small', 100, 1)
    tpp.test_fused_fit_equals_gmm_fit_bit_for_bit(poisoned, 'small', 1, 10)
