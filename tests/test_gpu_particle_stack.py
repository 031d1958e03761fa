"""`topaz particle_stack` on the MI355X: the golden CLI runs of tests/golden/particle_stack/ (the reference's own stacks and
STAR files), raw-count micrographs against an in-test numpy restatement of the reference loop (topaz/utils/picks.py:141-161),
the resize path, batching, chunking and a full-size micrograph.

Tolerance rule for standardised values (no resize): with f64 = (c - c.mean()) / c.std() evaluated in float64 on the float32
crop c and ref32 = the same expression in numpy float32 (the reference's arithmetic; for golden cases the fixture's data),
e_ref = max |ref32 - f64| and the GPU must satisfy max |gpu - f64| <= max(2 e_ref, 8 * 2^-23 * max |f64|).  The factor 2 allows
another summation order, the ulp floor covers cases where e_ref is tiny.  Resized values are held to 1e-4 absolute, the
project's parity bar for pixel outputs."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
PS = os.path.join(GOLDEN, 'particle_stack')
CLI = os.path.join(GOLDEN, 'cli')
PICKS = os.path.join(CLI, 'extract_picks.txt')
ULP = 2.0 ** -23


def _box(mic, x, y, S):
    """the reference's crop (picks.py:141-146) and the in-image mask of the S x S box"""
    mz, n, m = mic.shape
    left, upper = x - S // 2, y - S // 2
    right, lower = left + S, upper + S
    c = mic[:, max(0, upper):min(n, lower), max(0, left):min(m, right)]
    mask = np.zeros((S, S), bool)
    mask[max(0, -upper):max(0, min(S + n - lower, S)), max(0, -left):max(0, min(S + m - right, S))] = True
    if c.size == 0:
        mask[:] = False
    return c, mask


def restate(mic, xy, S):
    """(f64, ref32, in-image mask) of the reference loop: (c - c.mean()) / c.std() in float64 and in numpy float32, zero outside"""
    mz = mic.shape[0]
    f64 = np.zeros((len(xy), mz, S, S))
    r32 = np.zeros((len(xy), mz, S, S), np.float32)
    inb = np.zeros((len(xy), mz, S, S), bool)
    with np.errstate(invalid='ignore', divide='ignore'):
        for i, (x, y) in enumerate(xy):
            c, mask = _box(mic, int(x), int(y), S)
            if c.size == 0:
                continue
            d = c.astype(np.float64)
            f64[i][:, mask] = ((d - d.mean()) / d.std()).reshape(mz, -1)
            r32[i][:, mask] = ((c - c.mean()) / c.std()).reshape(mz, -1)
            inb[i][:, mask] = True
    return f64, r32, inb


def check_rule(gpu, f64, ref32, inb, label):
    gpu = np.asarray(gpu, dtype=np.float32).reshape(f64.shape)
    assert np.array_equal(np.isnan(gpu), np.isnan(f64)), label
    assert np.all(gpu[~inb] == 0.0), label
    ok = np.isfinite(f64)
    e_ref = float(np.abs(ref32[ok].astype(np.float64) - f64[ok]).max()) if ok.any() else 0.0
    err = float(np.abs(gpu[ok].astype(np.float64) - f64[ok]).max()) if ok.any() else 0.0
    bound = max(2 * e_ref, 8 * ULP * (float(np.abs(f64[ok]).max()) if ok.any() else 0.0))
    print(f'{label}: max|gpu - f64| {err:.3e}  e_ref {e_ref:.3e}  bound {bound:.3e}  ({err / bound if bound else 0:.2f} of it)')
    assert err <= bound, (label, err, bound)


def _read_mrc(path):
    from topaz_amd import mrc
    with open(path, 'rb') as f:
        a, h, _ = mrc.parse(f.read())
    return a, h


def _mic(name, root=CLI):
    a, _ = _read_mrc(os.path.join(root, name))
    return a[None] if a.ndim == 2 else a


def _cli(args, tmp_path):
    r = subprocess.run([sys.executable, '-m', 'topaz_amd', 'particle_stack'] + args, cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr
    return r


def _picks_by_micrograph(picks_path, threshold=-np.inf):
    import pandas as pd
    t = pd.read_csv(picks_path, sep='\t')
    if 'score' in t:
        t = t.loc[t['score'] >= threshold]
    return [(str(k), g[['x_coord', 'y_coord']].values) for k, g in t.groupby('image_name')]


@pytest.mark.parametrize('stack,size,threshold,root,picks,meta', [
    ('stack32', 32, None, CLI, PICKS, None),
    ('stack33_t5', 33, -5.0, CLI, PICKS, None),
    ('stack9', 9, None, PS, os.path.join(PS, 'picks3.txt'), os.path.join(PS, 'meta3.star')),
])
def test_golden_cli_runs(stack, size, threshold, root, picks, meta, tmp_path):
    out = tmp_path / (stack + '.mrcs')
    args = [picks, '--image-root', root, '--size', str(size), '-o', str(out)]
    if threshold is not None:
        args += ['--threshold', str(threshold)]
    if meta:
        args += ['--metadata', meta]
    r = _cli(args, tmp_path)
    assert '# Extracting' in r.stderr
    ref = open(os.path.join(PS, stack + '.mrcs'), 'rb').read()
    got = open(out, 'rb').read()
    assert len(got) == len(ref) and got[:1024] == ref[:1024]
    assert open(tmp_path / (stack + '.star')).read() == open(os.path.join(PS, stack + '.star')).read()
    gpu = np.frombuffer(got[1024:], np.float32)
    ref32 = np.frombuffer(ref[1024:], np.float32)
    f64s, masks = [], []
    for name, xy in _picks_by_micrograph(picks, -np.inf if threshold is None else threshold):
        f64, _, inb = restate(_mic(name + '.mrc', root), xy, size)
        f64s.append(f64)
        masks.append(inb)
    f64, inb = np.concatenate(f64s), np.concatenate(masks)
    ref32 = ref32.reshape(f64.shape)
    assert np.array_equal(np.isnan(ref32), np.isnan(f64))
    check_rule(gpu, f64, ref32, inb, stack)
    if stack == 'stack9':
        assert np.isnan(gpu.reshape(f64.shape)[0]).sum() == 243 and np.all(gpu.reshape(f64.shape)[3] == 0)


def _edge_picks(rng, H, W, S, n):
    """interior picks plus boxes cut by each edge and at each corner, none wholly outside the low edges"""
    h = S // 2
    xs = list(rng.randint(h, W - h, n)) + [0, W - 1, rng.randint(0, W), rng.randint(0, W), -h + 1, W + h - 2, 1, W - 2]
    ys = list(rng.randint(h, H - h, n)) + [rng.randint(0, H), rng.randint(0, H), 0, H - 1, -h + 1, H + h - 2, H - 2, 1]
    return np.stack([xs, ys], 1).astype(np.int32)


@pytest.mark.parametrize('kind', ['poisson5000', 'offset1e4'])
@pytest.mark.parametrize('S', [32, 64, 256])
def test_raw_count_micrographs_under_the_tolerance_rule(gpu_ctx, kind, S):
    import torch
    from topaz_amd import runtime as rt
    rng = np.random.RandomState(1000 + S)
    H, W = (512, 640) if S < 256 else (1024, 1152)
    mic = (rng.poisson(5000, (1, H, W)) if kind == 'poisson5000' else 1e4 + rng.randn(1, H, W)).astype(np.float32)
    xy = _edge_picks(rng, H, W, S, 48)
    gpu = rt.particle_stack(torch.from_numpy(mic[0]).cuda(), xy, S, ctx=gpu_ctx).cpu().numpy()
    f64, r32, inb = restate(mic, xy, S)
    check_rule(gpu, f64, r32, inb, f'{kind} S={S}')


def _np_resize(boxes32, R):
    """the reference's 2-D downsample (topaz/utils/image.py:38-61) per frame, then (r - r.mean()) / r.std() in float32"""
    out = []
    for box in boxes32:
        fr = []
        for x in box:
            F = np.fft.rfft2(x)
            F = np.concatenate([F[0:R // 2, 0:R // 2 + 1], F[-R // 2:, 0:R // 2 + 1]], axis=0)
            F *= (R * R) / (x.shape[-2] * x.shape[-1])
            fr.append(np.fft.irfft2(F, s=(R, R)).astype(np.float32))
        r = np.stack(fr)
        out.append((r - r.mean()) / r.std())
    return np.stack(out)


@pytest.mark.parametrize('R', [16, 15])
def test_resize_golden(gpu_ctx, R, tmp_path):
    from topaz_amd.main import main
    out = tmp_path / 'stack32_r16.mrcs'
    args = ['particle_stack', PICKS, '--image-root', CLI, '--size', '32', '--resize', str(R), '-o', str(out)]
    if R == 16:
        args += ['--metadata', os.path.join(PS, 'meta_ab.star')]
    main(args)
    got = open(out, 'rb').read()
    assert len(got) == 1024 + 4 * 88 * R * R
    a, h = _read_mrc(out)
    assert (h.nz, h.ny, h.nx, h.mz) == (88, R, R, 1)
    ref = np.load(os.path.join(PS, f'resize{R}.npy'))
    err = float(np.abs(a.reshape(ref.shape) - ref).max())
    print(f'resize 32 -> {R}: max |gpu - reference| {err:.3e}')
    assert err <= 1e-4
    if R == 16:
        assert open(tmp_path / 'stack32_r16.star').read() == open(os.path.join(PS, 'stack32_r16_meta.star')).read()


@pytest.mark.parametrize('S,R,mz', [(64, 32, 1), (64, 31, 2), (256, 128, 1)])
def test_resize_random_against_numpy(gpu_ctx, S, R, mz):
    import torch
    from topaz_amd import runtime as rt
    from topaz_amd.utils.picks import resize_operators
    rng = np.random.RandomState(7 * S + R)
    H, W = 600, 700
    mic = (rng.poisson(5000, (mz, H, W))).astype(np.float32)
    xy = _edge_picks(rng, H, W, S, 24)
    img = torch.from_numpy(mic if mz > 1 else mic[0]).cuda()
    gpu = rt.particle_stack(img, xy, S, R, resize_operators(S, R), ctx=gpu_ctx).cpu().numpy()
    _, r32, _ = restate(mic, xy, S)
    with np.errstate(invalid='ignore', divide='ignore'):
        ref = _np_resize(r32, R)
    # the corner box with a single in-image pixel (mz = 1) has zero variance: NaN in the reference, NaN after its resize too
    nan = np.isnan(ref)
    err = float(np.abs(gpu[~nan] - ref[~nan]).max())
    print(f'resize {S} -> {R} (mz {mz}): max |gpu - numpy| {err:.3e}, {nan.reshape(len(xy), -1).any(1).sum()} NaN particles')
    assert gpu.shape == (len(xy), mz, R, R) and np.array_equal(np.isnan(gpu), nan) and err <= 1e-4


def test_one_launch_per_chunk_whatever_the_particle_count(gpu_ctx):
    import torch
    from topaz_amd import runtime as rt
    from topaz_amd.utils.picks import resize_operators
    rng = np.random.RandomState(5)
    img = torch.from_numpy(rng.randn(512, 512).astype(np.float32)).cuda()
    counts = {}
    for R in (32, 16):
        ops = resize_operators(32, R) if R != 32 else None
        for n in (10, 1000):
            xy = rng.randint(0, 512, (n, 2)).astype(np.int32)
            gpu_ctx.prof_enable(1)
            gpu_ctx.prof_reset()
            rt.particle_stack(img, xy, 32, R, ops, ctx=gpu_ctx)
            counts[(R, n)] = gpu_ctx.prof_get(2)[1]
            gpu_ctx.prof_enable(0)
    print(counts)
    assert counts[(32, 10)] == counts[(32, 1000)] == 1
    assert counts[(16, 10)] == counts[(16, 1000)] == 4


@pytest.mark.parametrize('resize', [-1, 15])
def test_chunks_are_bit_identical_to_one_chunk(gpu_ctx, resize, tmp_path):
    import io
    from topaz_amd.utils.picks import plan_particle_stack, write_particle_stack
    outs = []
    R = 32 if resize < 0 else resize
    per = 4 * (R * R + (0 if resize < 0 else 32 * 32 + 2 * 32 * R))
    for budget in (1 << 30, 7 * per):              # 88 picks (48 + 40 per micrograph) in chunks of 7: ragged last chunks
        out = tmp_path / f'b{budget}' / 's.mrcs'
        out.parent.mkdir()
        plan = plan_particle_stack(PICKS, str(out), -np.inf, 32, resize, CLI, '.mrc', None, log=io.StringIO())
        write_particle_stack(plan, budget_bytes=budget, log=io.StringIO())
        outs.append(open(out, 'rb').read())
    assert len(outs[0]) == 1024 + 4 * 88 * R * R and outs[0] == outs[1]


def test_full_size_micrograph(gpu_ctx):
    import torch
    from topaz_amd import runtime as rt
    rng = np.random.RandomState(4096)
    mic = (1e4 + rng.randn(1, 4096, 4096)).astype(np.float32)
    xy = _edge_picks(rng, 4096, 4096, 256, 2000 - 8)
    assert len(xy) == 2000
    gpu = rt.particle_stack(torch.from_numpy(mic[0]).cuda(), xy, 256, ctx=gpu_ctx).cpu().numpy()
    f64, r32, inb = restate(mic, xy, 256)
    check_rule(gpu, f64, r32, inb, 'full size 4096^2, 2000 picks, S=256')
