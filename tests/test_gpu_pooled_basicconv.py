"""conv31 / conv63 / conv127 stacks trained with `--pooling max|avg` on the MI355X: the filled forward against what the reference
itself returned (tools/make_pooled_basicconv_golden.py), the two padded pool ops against torch on the CPU, `topaz segment` with
such a model file, and the refusal above the tiling limit.  Tolerance on logits: 1e-4 absolute."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu
ATOL = 1e-4
FIXTURES = ['conv31_max_bn_u16', 'conv31_avg_u32', 'conv31_max_drop_bn_u16', 'conv127_max_bn_u16', 'conv127_avg_bn_u16',
            'conv31_3d_max_bn_u8', 'conv63_3d_avg_bn_u8', 'conv31_max_bn_u16_us2']
DILS = [1, 2, 4, 8]


def _load(name):
    from topaz_amd.model.factory import load_model
    m = load_model(os.path.join(GOLDEN, f'user_model_{name}.sav'))
    m.eval()
    m.fill()
    m.cuda()
    return m


def _score(m, x):
    with torch.no_grad():
        return m(torch.from_numpy(x)[None, None].cuda())[0, 0].cpu().numpy()


# ---- 1. every fixture, default path and exact fp32 --------------------------------------------------------------------
@pytest.mark.parametrize('name', FIXTURES)
def test_filled_forward_vs_reference_golden(gpu_ctx, name):
    z = load_golden(f'score_{name}')
    m = _load(name)
    assert m.pooling == str(z['pooling']) and m.width == int(z['width'])
    k = 0
    while f'x{k}' in z.files:
        x, ref = z[f'x{k}'], z[f'y{k}']
        y = _score(m, x)
        assert y.shape == ref.shape
        err = float(np.abs(y - ref).max())
        gpu_ctx.set_exact(True)
        try:
            y32 = _score(m, x)
        finally:
            gpu_ctx.set_exact(False)
        err32 = float(np.abs(y32 - ref).max())
        print(f'{name} {x.shape} -> {y.shape}: |default - ref| {err:.2e}  |exact - ref| {err32:.2e}  split layers '
              f'{m.device_model.split_layers()}  split stats {m.device_model.split_stats()}')
        assert y32.shape == ref.shape
        assert err <= ATOL and err32 <= ATOL
        k += 1


# ---- 2. the ops alone ------------------------------------------------------------------------------------------------------
def _cases():
    """(dims, d, shape): 2-D shapes are C x H x W, 3-D ones C x D x H x W.  Per dilation d the smallest input with a 3^dims output
    (every class of tap: corner, edge, interior), then 5 x 23 x 31 and 17 x 9 x 40: sizes that are no multiple of a 256-thread
    block or of an 8-channel cell, more than one block, one axis barely longer than the window."""
    out = []
    for d in DILS:
        out += [(2, d, (1, 2 * d + 1, 2 * d + 1)), (2, d, (5, 23, 31)), (2, d, (17, 9, 40))]
        out += [(3, d, (3, 2 * d + 1, 2 * d + 1, 2 * d + 1)), (3, d, (3, 5, 23, 31)), (3, d, (2, 17, 9, 40))]
    return out


def _fits(d, shape):
    return min(n + 2 - 2 * d for n in shape[1:]) >= 1


def _ids(c):
    return f'{c[0]}d-d{c[1]}-' + 'x'.join(map(str, c[2]))


def _torch_max(x, dims, d):
    f = F.max_pool2d if dims == 2 else F.max_pool3d
    return f(x[None], 3, stride=1, padding=1, dilation=d)[0]


def _torch_avg(x, dims):
    f = F.avg_pool2d if dims == 2 else F.avg_pool3d
    return f(x[None], 3, stride=1, padding=1)[0]


def _split_round_trip(x):
    """the fp32 value a split cell stands for: hi = f16(x), lo = f16(x - hi) (csrc/split_fmt.h), joined as hi + lo"""
    hi = x.half()
    lo = (x - hi.float()).half()
    return hi.float() + lo.float()


def _input(dims, shape, seed, special=False):
    rs = np.random.RandomState(seed)
    x = (rs.randn(*shape) * 3).astype(np.float32)
    if special:
        flat = x.reshape(-1)
        n = flat.size
        for j, v in enumerate((np.nan, np.inf, -np.inf, np.inf, -np.inf, np.nan)):
            flat[(j * 7919 + 3) % n] = v
        flat[:: max(1, n // 5)] = -np.inf            # runs of -inf: windows where padding and data tie
    return torch.from_numpy(x)


@pytest.mark.parametrize('case', _cases(), ids=_ids)
def test_padded_max_op_is_bit_identical_to_torch(gpu_ctx, case):
    """fp32 planes: finite, and NaN / +-inf inputs (a NaN propagates, -inf never comes from the padding alone); split cells:
    bit-identical to torch on the values the cells stand for.  (NaN / inf do not exist in split cells: the conversion raises the
    overflow flag and the image is re-run on the fp32 kernels -- asserted here as the flag.)"""
    from topaz_amd import runtime as rt
    dims, d, shape = case
    if not _fits(d, shape):
        with pytest.raises(ValueError, match='too small'):
            rt.pool(torch.zeros(shape), 'max', dil=d, pad=1, ctx=gpu_ctx)
        return
    for special in (False, True):
        x = _input(dims, shape, 11 * d + len(shape), special)
        y, _ = rt.pool(x, 'max', dil=d, pad=1, split=False, ctx=gpu_ctx)
        ref = _torch_max(x, dims, d)
        assert tuple(y.shape) == tuple(ref.shape)
        assert np.array_equal(y.cpu().numpy().view(np.uint32), ref.numpy().view(np.uint32)), (case, special)
    x = _input(dims, shape, 13 * d + len(shape))
    ys, ovf = rt.pool(x, 'max', dil=d, pad=1, split=True, ctx=gpu_ctx)
    ref = _torch_max(_split_round_trip(x), dims, d)
    assert not ovf and np.array_equal(ys.cpu().numpy().view(np.uint32), ref.numpy().view(np.uint32)), case
    _, ovf = rt.pool(_input(dims, shape, 5, special=True), 'max', dil=d, pad=1, split=True, ctx=gpu_ctx)
    assert ovf


@pytest.mark.parametrize('case', [c for c in _cases() if c[1] == 1], ids=_ids)
def test_padded_mean_op(gpu_ctx, case):
    """fp32 planes within 8 * 2^-23 * max|x| of the float64 mean (the project's 8-ulp floor); NaN / +-inf where torch has them.
    Split cells against the fp32-plane kernel: the inputs are rounded to 22 bits on the way in and the mean on the way out, each
    at most 2^-23 relative, so the format's own bound is 2^-22 * max|x|; the bar is twice that."""
    from topaz_amd import runtime as rt
    dims, _, shape = case
    x = _input(dims, shape, 17 + len(shape))
    amax = float(x.abs().max())
    y, _ = rt.pool(x, 'avg', ctx=gpu_ctx)
    ref64 = _torch_avg(x.double(), dims)
    assert tuple(y.shape) == tuple(x.shape)
    err = float((y.cpu().double() - ref64).abs().max())
    ys, ovf = rt.pool(x, 'avg', split=True, ctx=gpu_ctx)
    err_s = float((ys.cpu().double() - y.cpu().double()).abs().max())
    print(f'mean {_ids(case)}: |planes - float64| / (2^-23 max|x|) = {err / (2.0 ** -23 * amax):.3f}   '
          f'|split - planes| / (2^-22 max|x|) = {err_s / (2.0 ** -22 * amax):.3f}')
    assert err <= 8 * 2.0 ** -23 * amax
    assert not ovf and err_s <= 2 * 2.0 ** -22 * amax
    xs = _input(dims, shape, 19, special=True)
    y, _ = rt.pool(xs, 'avg', ctx=gpu_ctx)
    ref = _torch_avg(xs, dims)
    y = y.cpu()
    assert torch.equal(torch.isnan(y), torch.isnan(ref))
    fin = torch.isfinite(ref)
    assert torch.equal(y[~fin & ~torch.isnan(ref)], ref[~fin & ~torch.isnan(ref)])          # +-inf where torch has them
    if bool(fin.any()):                             # (the 3^dims case has no window without a special value)
        bound = 8 * 2.0 ** -23 * float(xs[torch.isfinite(xs)].abs().max())
        assert float((y[fin].double() - _torch_avg(xs.double(), dims)[fin]).abs().max()) <= bound


@pytest.mark.parametrize('dims', [2, 3])
def test_pool_ops_through_a_two_layer_program(gpu_ctx, dims):
    """conv + pool as a layer program: the dispatch of TPZ_OP_MAXPOOL with padding and of TPZ_OP_AVGPOOL, the output shape the
    library predicts and the host-side LayerProgram.out_shape.  The pool's input is the same conv run as a one-layer program
    (exact mode: one fp32 kernel either way), so the max must come out bit for bit."""
    from topaz_amd.runtime import DeviceModel, LayerProgram
    rs = np.random.RandomState(23 + dims)
    C = 5
    w = (rs.randn(*((C, 1) + (3,) * dims)) * 0.4).astype(np.float32)
    b = (rs.randn(C) * 0.1).astype(np.float32)
    shape = (23, 31) if dims == 2 else (9, 23, 31)
    x = torch.from_numpy(rs.randn(*((1, 1) + shape)).astype(np.float32))
    gpu_ctx.set_exact(True)
    try:
        p0 = LayerProgram(dims)
        p0.conv(0, w, b, pad=1, slope=0.1)
        t = DeviceModel(p0, gpu_ctx).forward(x.cuda()).cpu()[0]
        assert tuple(t.shape) == (C,) + shape
        for d in DILS:
            for op in ('max', 'avg') if d == 1 else ('max',):
                p = LayerProgram(dims)
                s = p.conv(0, w, b, pad=1, slope=0.1)
                s = p.maxpool(s, 3, d, pad=1) if op == 'max' else p.avgpool(s)
                D, H, W = (1,) + shape if dims == 2 else shape
                want = p.out_shape(D, H, W)
                if min(want) < 1:
                    continue
                dm = DeviceModel(p, gpu_ctx)
                assert dm.out_shape(D, H, W) == want
                y = dm.forward(x.cuda()).cpu()[0]
                if op == 'max':
                    ref = _torch_max(t, dims, d)
                    assert tuple(y.shape) == tuple(ref.shape) and torch.equal(y, ref), (dims, d)
                else:
                    ref = _torch_avg(t.double(), dims)
                    assert tuple(y.shape) == tuple(ref.shape)
                    assert float((y.double() - ref).abs().max()) <= 8 * 2.0 ** -23 * float(t.abs().max())
    finally:
        gpu_ctx.set_exact(False)


def test_unpadded_resnet_pool_is_unchanged(gpu_ctx):
    """pad = 0 takes the kernel it always took: the --pooling max ResNet golden still scores to 1e-4 and a program that ends in the
    unpadded pool equals torch's unpadded max"""
    from topaz_amd.runtime import DeviceModel, LayerProgram
    rs = np.random.RandomState(31)
    w = (rs.randn(12, 1, 3, 3) * 0.3).astype(np.float32)
    x = torch.from_numpy(rs.randn(1, 1, 40, 52).astype(np.float32))
    p0 = LayerProgram(2)
    p0.conv(0, w, None, pad=1, slope=0.1)
    p = LayerProgram(2)
    p.maxpool(p.conv(0, w, None, pad=1, slope=0.1), 3, 2)
    gpu_ctx.set_exact(True)
    try:
        t = DeviceModel(p0, gpu_ctx).forward(x.cuda()).cpu()
        y = DeviceModel(p, gpu_ctx).forward(x.cuda()).cpu()
    finally:
        gpu_ctx.set_exact(False)
    assert torch.equal(y, F.max_pool2d(t, 3, stride=1, dilation=2))


# ---- 3. topaz segment ------------------------------------------------------------------------------------------------------
def test_segment_with_a_pooled_model_file(gpu_ctx, tmp_path):
    from PIL import Image
    from topaz_amd import mrc
    from topaz_amd.main import main
    z = load_golden('score_conv31_max_bn_u16')
    with open(tmp_path / 'mic.mrc', 'wb') as f:
        mrc.write(f, z['x0'][np.newaxis])
    main(['segment', '-m', os.path.join(GOLDEN, 'user_model_conv31_max_bn_u16.sav'), '-o', str(tmp_path / 'seg'),
          str(tmp_path / 'mic.mrc')])
    y = np.array(Image.open(tmp_path / 'seg' / 'mic.tiff'))
    assert y.dtype == np.float32 and y.shape == z['y0'].shape == (68, 88)          # 2 smaller than the 70 x 90 micrograph
    assert np.abs(y - z['y0']).max() <= ATOL


# ---- 4. above the tiling limit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['conv31_max_bn_u16', 'conv31_avg_u32'])
def test_frame_above_the_tiling_limit_is_refused(gpu_ctx, name):
    from topaz_amd._lib import TopazHipError
    m = _load(name)
    x = np.random.RandomState(3).randn(96, 96).astype(np.float32)
    for exact in (False, True):
        try:
            gpu_ctx.set_exact(exact)
            whole = _score(m, x)
            assert whole.shape == ((94, 94) if m.pooling == 'max' else (96, 96))
            gpu_ctx.set_tiling(96 * 96 - 1, 64)
            with pytest.raises(TopazHipError, match=r'conv31/63/127.*--pooling max\|avg.*not scored in tiles'):
                _score(m, x)
            gpu_ctx.set_tiling(96 * 96, 64)                  # at the limit: scored whole, as before
            assert np.array_equal(_score(m, x), whole)
        finally:
            gpu_ctx.set_tiling(40 << 20, 4096)
            gpu_ctx.set_exact(False)
