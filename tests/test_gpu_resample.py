"""The truncated-DFT resampler with device-resident operators (tpz_resample_*, csrc/rt_resample.hip + resample_gemm.h) against
the oracle's numpy-FFT restatement of the reference downsample, and the structural facts of a plan: a run uploads nothing,
repeats bit for bit, and a plan can be freed, re-created and evicted under work already enqueued."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

ATOL = 1e-4            # the bar tests/test_gpu_ops.py holds the downsample to
T, KS = 128, 16        # RS_TILE (tile extent in P and in Q) and RS_KS (K step) of csrc/resample_gemm.h

# (M, N) -> (m, n).  The two GEMMs of a run are  stage 1: P = 2m, Q = N, K = M   and   stage 2: P = m, Q = n, K = N + N.
_EDGE_SHAPES = (
    # P one below / at / above the tile: stage 2 (P = m) and stage 1 (P = 2m, even: 126 / 128 / 130)
    [((130, 20), (m, 9)) for m in (T - 1, T, T + 1, T // 2 - 1, T // 2, T // 2 + 1)]
    # Q: stage 1 (Q = N) and stage 2 (Q = n)
    + [((20, q), (9, q)) for q in (T - 1, T, T + 1)] + [((20, T + 1), (9, T - 1))]
    # K: stage 1 (K = M) and both segments of stage 2 (K = N)
    + [((k, k), (k // 2, k // 2)) for k in (KS - 1, KS, KS + 1)]
    # the kernel has two K loops, picked per tile: float4 loads for a tile inside C when every K is a multiple of KS and the rows
    # are 16-byte aligned, clamped single loads otherwise.  All tiles on the first; interior tiles on the first and ragged ones
    # on the second in ONE launch (both stages); whole tiles on the second because K is ragged; ... because rows are unaligned
    + [((2 * T, 3 * T), (T, T)), ((2 * T, 3 * T + KS), (T + 2, T + 72)), ((2 * T - 6, 3 * T), (T, T)), ((2 * T, 3 * T + 2), (T, T))]
)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _randn(shape):
    return np.random.RandomState(shape[0] * 7919 + shape[1]).randn(*shape).astype(np.float32)


def _check(shape_in, factor=1, shape_out=None):
    from oracle.denoising import downsample as oracle_downsample
    from topaz_amd.utils.image import downsample_device
    x = _randn(shape_in)
    want = oracle_downsample(x, factor, shape_out)
    got = downsample_device(_dev(x), factor, shape_out)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == want.shape
    err = np.abs(got.cpu().numpy() - want).max()
    print(f'{shape_in} -> {want.shape}: max |delta| {err:.2e}')
    assert err <= ATOL, (shape_in, want.shape, err)


@pytest.mark.parametrize('shape_in,factor,shape_out', [((5, 7), 2, None), ((37, 53), 4, None), ((64, 64), 1, (64, 64)),
                                                      ((200, 130), 3, None)])
def test_resample_vs_oracle(gpu_ctx, shape_in, factor, shape_out):
    _check(shape_in, factor, shape_out)


@pytest.mark.parametrize('shape_in,shape_out', _EDGE_SHAPES)
def test_resample_vs_oracle_at_tile_edges(gpu_ctx, shape_in, shape_out):
    _check(shape_in, 1, shape_out)


def test_resample_vs_reference_golden(gpu_ctx):
    from topaz_amd.utils.image import downsample_device
    z = load_golden('downsample_cases')
    names = sorted({k.split(':')[0] for k in z.files if ':' in k})
    assert names
    for name in names:
        y = downsample_device(_dev(z[name + ':x']), int(z[name + ':factor'])).cpu().numpy()
        ref = z[name + ':y']
        assert y.shape == ref.shape
        assert np.abs(y - ref).max() <= ATOL, (name, np.abs(y - ref).max())


def test_raw_counts_no_worse_than_twice_torch_cpu_fp32(gpu_ctx):
    """Poisson(5000) counts, 515 x 387 / 4: against a float64 evaluation of the same (float32) operators, the kernel's error is at
    most twice that of torch-CPU's fp32 evaluation (L @ x, then the two column products)."""
    from topaz_amd.utils.image import _downsample_operators, downsample_device
    M, N = 515, 387
    m, n = M // 4, N // 4
    x = np.random.RandomState(11).poisson(5000, (M, N)).astype(np.float32)
    L, R = _downsample_operators(M, N, m, n)
    U64 = L.astype(np.float64) @ x.astype(np.float64)
    R64 = R.astype(np.float64)
    ref = U64[:m] @ R64[:, :N].T + U64[m:] @ R64[:, N:].T
    Lt, Rt, xt = torch.from_numpy(L), torch.from_numpy(R), torch.from_numpy(x)
    Ut = Lt @ xt
    cpu32 = (Ut[:m] @ Rt[:, :N].T + Ut[m:] @ Rt[:, N:].T).numpy()
    got = downsample_device(_dev(x), 4).cpu().numpy()
    e_gpu, e_cpu = np.abs(got - ref).max(), np.abs(cpu32 - ref).max()
    print(f'raw counts {M}x{N}/4 vs float64 (values up to {np.abs(ref).max():.0f}): kernel {e_gpu:.3e}, torch-CPU fp32 {e_cpu:.3e}')
    assert e_gpu <= 2 * e_cpu, (e_gpu, e_cpu)


def test_plan_reuse_uploads_nothing_and_repeats_bit_for_bit(gpu_ctx):
    from topaz_amd import runtime as rt
    from topaz_amd.utils.image import _downsample_operators
    M, N, m, n = 300, 260, 75, 65
    L, R = _downsample_operators(M, N, m, n)
    x = _dev(_randn((M, N)))
    before = rt.resample_upload_bytes(gpu_ctx)
    plan = rt.ResamplePlan(L, R, gpu_ctx)
    created = rt.resample_upload_bytes(gpu_ctx)
    assert created - before >= L.nbytes + R.nbytes                  # the operators went up once (rows padded to 16 bytes)
    y0 = plan.run(x)
    launches = gpu_ctx.launches()
    y1 = plan.run(x)
    assert gpu_ctx.launches() - launches == 2                       # two GEMM launches, nothing else
    assert rt.resample_upload_bytes(gpu_ctx) == created             # ... and no operator byte
    assert np.array_equal(_bits(y0.cpu().numpy()), _bits(y1.cpu().numpy()))
    assert np.array_equal(_bits(plan.run_host(x.cpu().numpy())), _bits(y0.cpu().numpy()))
    # free, then the same shape again
    plan.close()
    assert plan.handle is None
    with pytest.raises(rt._lib.TopazHipError):
        plan.run(x)
    again = rt.ResamplePlan(L, R, gpu_ctx)
    assert rt.resample_upload_bytes(gpu_ctx) == created + (created - before)
    assert np.array_equal(_bits(again.run(x).cpu().numpy()), _bits(y0.cpu().numpy()))
    again.close()
    with pytest.raises(ValueError):
        rt.ResamplePlan(L, R, gpu_ctx).run(x[:, :-1])


def test_bad_shapes_are_refused(gpu_ctx):
    from topaz_amd import runtime as rt
    with pytest.raises(rt._lib.TopazHipError):                      # m > M: not a reduction
        rt.ResamplePlan(np.zeros((12, 5), np.float32), np.zeros((3, 8), np.float32), gpu_ctx)


def test_cache_eviction_frees_the_plan_under_enqueued_work(gpu_ctx):
    from topaz_amd.utils import image as im
    for plan in im._PLAN_CACHE.values():
        plan.close()
    im._PLAN_CACHE.clear()
    x = _dev(_randn((512, 384)))
    want = im.downsample_device(x, 4).cpu().numpy()
    (key, first), = im._PLAN_CACHE.items()
    y = im.downsample_device(x, 4)                                  # enqueued, not waited for
    assert im._PLAN_CACHE[key] is first                             # ... on the cached plan
    for k in range(im._PLAN_CACHE_MAX):                             # as many other shapes as the cache holds: `first` goes
        im.downsample_device(x[:64 + 4 * k, :48], 2)
    assert key not in im._PLAN_CACHE and first.handle is None and len(im._PLAN_CACHE) == im._PLAN_CACHE_MAX
    assert np.array_equal(_bits(y.cpu().numpy()), _bits(want))
    assert np.array_equal(_bits(im.downsample_device(x, 4).cpu().numpy()), _bits(want))     # (a new plan for the old shape)


def test_strided_views_are_copied_not_misread(gpu_ctx):
    from topaz_amd.utils.image import downsample_device
    x = _dev(_randn((140, 96)))
    for view in (x[::2, 1::2], x.t(), x[3:131, 5:69]):
        assert not view.is_contiguous()
        want = downsample_device(view.contiguous(), 2)
        assert np.array_equal(_bits(downsample_device(view, 2).cpu().numpy()), _bits(want.cpu().numpy()))
    # the numpy entry point takes strided arrays the same way
    from topaz_amd.utils.image import downsample
    xn = x.cpu().numpy()
    assert np.array_equal(_bits(downsample(xn[::2, 1::2], 2)), _bits(downsample_device(x[::2, 1::2].contiguous(), 2).cpu().numpy()))
