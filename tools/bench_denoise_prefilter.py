"""Measure `topaz denoise --lowpass` / `--deconvolve` on one MI355X (profiles/denoise_prefilter.txt).

    python tools/bench_denoise_prefilter.py [--runs 5] [--cpu-runs 2] [--out profiles/denoise_prefilter.txt]

Per 4096^2 float32 micrograph (seeded N(0, 1) + 5000 for lowpass, N(0, 1) for deconvolve):
  - device ms of lowpass at f = 2 and 4 and of deconvolve at P = 1 and 4 (the library profiler: HIP events around every launch),
    median of --runs calls after one warm-up, and the fp64 rate the lowpass GEMMs reach (algorithmic FLOP / device time),
  - the wall time of one call from the host (operator upload and host filter design included),
  - the wall time of the CLI (`python -m topaz_amd denoise -m none ...`, interpreter start included) on one micrograph,
  - the same work on the host through the reference's arithmetic restated in numpy (float64 rfft2 / irfft2) and torch
    (float32 conv2d covariance and filter, as correct_spatial_covariance does): a baseline, not a target.
"""
from __future__ import annotations

import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, 'tests'))


def device_ms(ctx, fn, runs):
    fn()
    ctx.sync()
    ms, wall, fl = [], [], 0.0
    for _ in range(runs):
        ctx.prof_enable(1)
        ctx.prof_reset()
        t = time.perf_counter()
        fn()
        ctx.sync()
        wall.append(1e3 * (time.perf_counter() - t))
        m, n, fl = ctx.prof_get(2)
        ms.append(m)
        ctx.prof_enable(0)
    return float(np.median(ms)), float(np.median(wall)), fl, n


def cpu_lowpass(x, f):
    from test_cpu_denoise_prefilter import lowpass64
    return lowpass64(x, f).astype(np.float32)


def cpu_deconv(x, P):
    """correct_spatial_covariance's arithmetic in torch float32 (conv2d) with the float64 numpy filter design"""
    import torch
    import torch.nn.functional as F
    from topaz_amd.denoise import deconv_tiles, unblur_filter
    xt = torch.from_numpy(x)
    N, M, ry, rx = deconv_tiles(*x.shape, P)
    y = torch.zeros_like(xt)
    r0 = 0
    for n, (ya, yl) in zip(N, ry):
        c0 = 0
        for m, (xa, xl) in zip(M, rx):
            t = xt[ya:ya + yl, xa:xa + xl]
            c = t[5:-5, 5:-5]
            cov = F.conv2d(t[None, None], c[None, None]).squeeze() / c.numel()
            w = torch.from_numpy(unblur_filter(cov.double().numpy()).astype(np.float32))
            f = F.conv2d(t[None, None], w[None, None], padding=5).squeeze()
            y[r0:r0 + n, c0:c0 + m] = f[r0 - ya:r0 - ya + n, c0 - xa:c0 - xa + m]
            c0 += m
        r0 += n
    return y


def timed(fn, runs):
    fn()
    ts = []
    for _ in range(runs):
        t = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t))
    return float(np.median(ts)), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--cpu-runs', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'denoise_prefilter.txt'))
    a = ap.parse_args()
    import torch
    from topaz_amd import runtime as rt
    from topaz_amd.denoise import correct_spatial_covariance, lowpass, lowpass_operator
    ctx = rt.get_context(0)
    rng = np.random.RandomState(355)
    x_lp = (5000 + rng.randn(4096, 4096)).astype(np.float32)
    x_dc = rng.randn(4096, 4096).astype(np.float32)
    d_lp, d_dc = torch.from_numpy(x_lp).cuda(), torch.from_numpy(x_dc).cuda()
    lines = ['# tools/bench_denoise_prefilter.py: one MI355X, 4096^2 float32 micrograph; device ms = library profiler (HIP events',
             '# around every launch), median of %d calls; host wall = one call from Python incl. operator upload / filter design' % a.runs]
    for f in (2, 4):
        ms, wall, fl, n = device_ms(ctx, lambda: lowpass(d_lp, f), a.runs)
        r = lowpass_operator(4096, float(f)).shape[1]
        lines.append(f'lowpass f={f}: rank {r}, {n} launches, device {ms:.2f} ms, {fl / 1e9:.1f} GFLOP fp64 -> {fl / ms / 1e9:.1f} '
                     f'TFLOP/s; host wall {wall:.1f} ms')
    for P in (1, 4):
        ms, wall, fl, n = device_ms(ctx, lambda: correct_spatial_covariance(d_dc, patch=P), a.runs)
        lines.append(f'deconvolve P={P}: {n} launches, device {ms:.2f} ms; host wall {wall:.1f} ms')
    with tempfile.TemporaryDirectory(dir='/dev/shm' if os.path.isdir('/dev/shm') else None) as d:
        from topaz_amd import mrc
        src = os.path.join(d, 'mic.mrc')
        with open(src, 'wb') as fh:
            mrc.write(fh, x_lp[None])
        for flags in (['--lowpass', '2'], ['--lowpass', '4'], ['--deconvolve'], ['--deconvolve', '--deconv-patch', '4'], []):
            cmd = [sys.executable, '-m', 'topaz_amd', 'denoise', '-m', 'none'] + flags + ['-o', os.path.join(d, 'out'), src]
            if not flags:
                cmd[cmd.index('none')] = 'unet-small'
            t = time.perf_counter()
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr
            lines.append(f'CLI wall ({" ".join(cmd[4:6] + flags)}): {time.perf_counter() - t:.2f} s (one micrograph, interpreter start '
                         f'included)')
    torch.set_num_threads(16)
    for f in (2, 4):
        med, lo, hi = timed(lambda: cpu_lowpass(x_lp, f), a.cpu_runs)
        lines.append(f'CPU lowpass f={f} (numpy float64 rfft2 / irfft2): {med:.0f} ms ({lo:.0f}-{hi:.0f})')
    for P in (1, 4):
        med, lo, hi = timed(lambda: cpu_deconv(x_dc, P), a.cpu_runs)
        lines.append(f'CPU deconvolve P={P} (torch float32 conv2d, 16 threads): {med:.0f} ms ({lo:.0f}-{hi:.0f})')
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text)


if __name__ == '__main__':
    main()
