"""Workspace buffers of the runtime drivers (csrc/rt_internal.h WorkBuf): every driver gives back what it took from the context's
pools, on its error paths too and whatever pool is current by then, and a repeated call finds its buffers cached instead of
growing the pools.  Toy shapes: what is asserted is Context.pool_stats(), not the arithmetic (the other files do that)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import golden_sd, load_golden

pytestmark = pytest.mark.gpu
BATCH_MEM = 1 << 40          # a fixed budget for the batched passes: the batch does not follow the machine's free memory


class _Env:
    """the models and inputs of the cases: loaded once, shared, never modified"""

    def __init__(self, ctx):
        from topaz_amd.denoise import Denoise, Denoise3D
        from topaz_amd.denoising.models import DenoiseNet
        from topaz_amd.model.factory import load_model
        rs = np.random.RandomState(611)
        self.ctx = ctx
        self.scorer = load_model('resnet8_u32')
        self.scorer.eval(); self.scorer.fill(); self.scorer.cuda()
        self.x64 = rs.randn(64, 64).astype(np.float32)
        self.x48 = rs.randn(48, 48).astype(np.float32)
        self.unet = Denoise('unet-small')
        self.unet_deep = Denoise('unet-v0.2.1')
        self.x96 = torch.from_numpy(rs.randn(96, 96).astype(np.float32)).cuda()
        self.x20 = rs.randn(20, 40).astype(np.float32)
        z = load_golden('denoise3d_unet3d_nf8')
        self.unet3d = Denoise3D(DenoiseNet('unet-3d', golden_sd(z)))
        self.tomo = torch.from_numpy(z['tomo']).cuda()
        self.w64 = (rs.randn(64, 64, 3, 3) / 24).astype(np.float32)
        self.x_conv = torch.from_numpy(rs.randn(64, 20, 45).astype(np.float32)).cuda()
        self.res_conv = torch.from_numpy(rs.randn(64, 22, 47).astype(np.float32)).cuda()
        self.x_pool = torch.from_numpy(rs.randn(8, 16, 16).astype(np.float32)).cuda()
        self.score = torch.from_numpy(rs.randn(64, 64).astype(np.float32)).cuda()
        px = np.where(rs.rand(4096) < 0.85, rs.randn(4096), 3.5 + 0.8 * rs.randn(4096)).astype(np.float32)
        self.pis = np.array([0.1, 0.5, 1.0])
        self.splits = np.quantile(px, 1 - self.pis).astype(np.float64)
        self.px = torch.from_numpy(px).cuda()
        self.x_lp = torch.from_numpy(rs.randn(32, 48).astype(np.float32)).cuda()
        self.x32 = torch.from_numpy(rs.randn(32, 32).astype(np.float32)).cuda()
        self.w_tile = rs.randn(4, 11, 11).astype(np.float32)
        self.xy = rs.randint(0, 64, size=(5, 2))

    def forward(self, x):
        with torch.no_grad():
            return self.scorer(torch.from_numpy(x)[None, None].cuda())


@pytest.fixture(scope='module')
def env(gpu_ctx):
    return _Env(gpu_ctx)


def _score(e):
    e.forward(e.x64)


def _score_tiled(e):
    try:
        e.ctx.set_tiling(1, 16)
        e.forward(e.x48)
    finally:
        e.ctx.set_tiling(40 << 20, 4096)


def _score_exact(e):
    try:
        e.ctx.set_exact(True)
        e.forward(e.x64)
    finally:
        e.ctx.set_exact(False)


def _calibrate(e):
    r = e.scorer.calibrate(e.x64, bar=0)
    assert r['eligible']


def _denoise_2d(e):
    e.unet.model.device_model.denoise_2d(e.x96, 32, 16)


def _denoise_2d_lanes(e):
    try:
        e.ctx.set_batch(0)
        _denoise_2d(e)
    finally:
        e.ctx.set_batch(8)


def _denoise_2d_exact(e):
    try:
        e.ctx.set_exact(True)
        _denoise_2d(e)
    finally:
        e.ctx.set_exact(False)


def _denoise_3d(e):
    e.unet3d.model.device_model.denoise_3d(e.tomo, 32, 16)


def _denoise_3d_shard(e):
    e.unet3d.model.device_model.denoise_3d(e.tomo, 32, 16, shard=1, n_shards=2)


def _denoise_too_small(e):
    """an argument error the library reports after its driver took buffers (test_gpu_denoise.py test_edge_cases)"""
    from topaz_amd._lib import TopazHipError
    with pytest.raises(TopazHipError, match='too small'):
        e.unet_deep.denoise(e.x20, -1)


def _conv_split(e):
    from topaz_amd import runtime as rt
    rt.conv_split(e.x_conv, e.w64, None, pad=1, slope=1.0, ctx=e.ctx)
    rt.conv_split(e.x_conv, e.w64, None, pad=1, slope=0.0, res=e.res_conv, res_crop=1, ctx=e.ctx)


def _pool_split(e):
    from topaz_amd import runtime as rt
    rt.pool(e.x_pool, 'max', 1, 1, split=True, ctx=e.ctx)


def _nms(e):
    from topaz_amd import runtime as rt
    s, _ = rt.nms(e.score, 4, 0.0, ctx=e.ctx)
    assert len(s) > 1


def _nms_over_capacity(e):
    """more picks than the caller's lists hold: tpz_nms_2d reports it (and the count) after the whole driver has run"""
    from topaz_amd.runtime import _ptr
    coords = torch.empty((1, 2), dtype=torch.int32, device=e.score.device)
    out = torch.empty((1,), dtype=torch.float32, device=e.score.device)
    n = C.c_int(0)
    e.ctx.bind_current_stream()
    rc = e.ctx.lib.tpz_nms_2d(e.ctx.handle, _ptr(e.score), 64, 64, 4, 0.0, _ptr(coords), _ptr(out), 1, C.byref(n))
    assert rc != 0 and n.value > 1
    assert b'exceed the output capacity' in e.ctx.lib.tpz_last_error(e.ctx.handle)


def _order_stats(e):
    from topaz_amd import runtime as rt
    rt.order_stats(e.px, [0, 2048, 4095], ctx=e.ctx)


def _gather(e):
    from topaz_amd import runtime as rt
    rt.gather(e.px, [4095, 0, 17], ctx=e.ctx)


def _gmm_fit_fused(e):
    from topaz_amd import runtime as rt
    rt.gmm_fit_fused(e.px, e.pis, e.splits, num_iters=5, ctx=e.ctx)


def _gmm_fit(e):
    from topaz_amd import runtime as rt
    rt.gmm_fit(e.px, e.pis, e.splits, num_iters=5, ctx=e.ctx)


def _lowpass(e):
    from topaz_amd import runtime as rt
    from topaz_amd.denoise import lowpass_operator
    rt.lowpass_2d(e.x_lp, lowpass_operator(32, 2.0), lowpass_operator(48, 2.0, rfft=True), ctx=e.ctx)


def _spatial_cov(e):
    from topaz_amd import runtime as rt
    rt.spatial_cov_2d(e.x32, 2, ctx=e.ctx)


def _tile_filter(e):
    from topaz_amd import runtime as rt
    rt.tile_filter_2d(e.x32, e.w_tile, 2, ctx=e.ctx)


def _particle_stack(e):
    from topaz_amd import runtime as rt
    from topaz_amd.utils.picks import resize_operators
    rt.particle_stack(e.score, e.xy, 16, 8, resize_operators(16, 8), ctx=e.ctx)


def _resample(e):
    from topaz_amd import runtime as rt
    from topaz_amd.utils.image import _downsample_operators
    plan = rt.ResamplePlan(*_downsample_operators(32, 32, 16, 16), ctx=e.ctx)
    try:
        plan.run(e.x32)
    finally:
        plan.close()


# the denoise, scoring and NMS cases: those that run the layer executor, the lanes, the batched passes and the NMS driver
REPEATED = [_score, _score_tiled, _score_exact, _calibrate, _denoise_2d, _denoise_2d_lanes, _denoise_2d_exact, _denoise_3d,
            _denoise_3d_shard, _denoise_too_small, _nms, _nms_over_capacity]
CASES = REPEATED + [_conv_split, _pool_split, _order_stats, _gather, _gmm_fit_fused, _gmm_fit, _lowpass, _spatial_cov,
                    _tile_filter, _particle_stack, _resample]


def _name(fn):
    return fn.__name__.lstrip('_')


def run_case(e, fn):
    """one case under the fixed batch budget, the context drained; -> pool_stats() after it"""
    try:
        e.ctx.set_batch_memory(BATCH_MEM)
        fn(e)
        e.ctx.sync()
    finally:
        e.ctx.set_batch_memory(0)
    return e.ctx.pool_stats()


@pytest.mark.parametrize('case', CASES, ids=_name)
def test_no_buffer_stays_in_use(env, case):
    assert run_case(env, case)['buffers_in_use'] == 0


@pytest.mark.parametrize('case', REPEATED, ids=_name)
def test_a_repeated_call_does_not_grow_the_pools(env, case):
    """a buffer left marked used is never handed out again: the next call allocates anew, and the pools grow"""
    run_case(env, case)
    second = run_case(env, case)
    third = run_case(env, case)
    assert (third['buffers'], third['bytes']) == (second['buffers'], second['bytes']) and third['buffers_in_use'] == 0
