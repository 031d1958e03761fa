"""Measure `topaz particle_stack` on one MI355X (the numbers behind profiles/particle_stack.txt and DESIGN.md section 8).

    python tools/bench_particle_stack.py [--mics 8] [--picks 2000] [--size 256] [--resize 128] [--cpu-runs 3] [--tmp /dev/shm]

Workload: `--mics` synthetic 4096^2 float32 micrographs (seeded Poisson(5000) counts) with `--picks` picks each (uniform over
the image, boxes cut by the edges included), run once at --size and once at --size -> --resize.  Reports
  - device ms per micrograph of each kernel (the library profiler: HIP events around every launch), the algorithmic HBM bytes
    of those launches and the fraction of 8 TB/s they represent,
  - the wall time of the whole CLI (`python -m topaz_amd particle_stack`, interpreter start included) per micrograph, output on
    tmpfs,
  - the same workload through a numpy restatement of the reference loop (topaz/utils/picks.py:132-163, the resize as the
    per-frame 2-D truncated DFT) on the same host: 1 warm-up and --cpu-runs timed runs, median and spread.
"""
from __future__ import annotations

import argparse
import io
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM = 8e12


def make_inputs(d, n_mics, n_picks, H=4096, W=4096):
    from topaz_amd import mrc
    rng = np.random.RandomState(355)
    rows = []
    for i in range(n_mics):
        x = rng.poisson(5000, (H, W)).astype(np.float32)
        with open(os.path.join(d, f'mic{i}.mrc'), 'wb') as f:
            mrc.write(f, x[None])
        xs, ys = rng.randint(0, W, n_picks), rng.randint(0, H, n_picks)
        rows += [f'mic{i}\t{a}\t{b}\t{s:.4f}' for a, b, s in zip(xs, ys, rng.randn(n_picks))]
    picks = os.path.join(d, 'picks.txt')
    with open(picks, 'w') as f:
        f.write('image_name\tx_coord\ty_coord\tscore\n' + '\n'.join(rows) + '\n')
    return picks


def device_kernels(picks, d, S, R, n_mics):
    from topaz_amd import runtime as rt
    from topaz_amd.utils.picks import plan_particle_stack, write_particle_stack
    plan = plan_particle_stack(picks, os.path.join(d, 'dev.mrcs'), -np.inf, S, R, d, '.mrc', None, log=io.StringIO())
    write_particle_stack(plan, log=io.StringIO())                      # warm-up (pinned rings, workspaces)
    ctx = rt.get_context(0)
    ctx.prof_enable(1)
    ctx.prof_reset()
    write_particle_stack(plan, log=io.StringIO())
    ctx.sync()
    rows = ctx.prof_kernels_bytes()
    ctx.prof_enable(0)
    out = []
    for name, ms, n, fl, by in rows:
        if name.startswith('particle_'):
            out.append(f'  {name:22s} {ms / n_mics:8.3f} ms/mic  {n:4d} launches  {by / n_mics / 1e6:8.1f} MB/mic  '
                       f'{by / (ms * 1e-3) / 1e12:6.2f} TB/s = {by / (ms * 1e-3) / HBM:5.1%} of 8 TB/s' +
                       (f'  {fl / (ms * 1e-3) / 1e12:6.1f} TFLOP/s fp32' if fl else ''))
    return out


def cli_wall(picks, d, S, R, n_mics):
    out = os.path.join(d, 'cli.mrcs')
    cmd = [sys.executable, '-m', 'topaz_amd', 'particle_stack', picks, '--image-root', d, '--size', str(S), '-o', out]
    if R != S:
        cmd += ['--resize', str(R)]
    t0 = time.perf_counter()
    subprocess.run(cmd, cwd=ROOT, check=True, capture_output=True)
    return (time.perf_counter() - t0) / n_mics * 1e3


def numpy_reference(picks, d, S, R):
    """the reference loop restated in numpy: per particle slice, mean, std, allocation, write (resize per frame)"""
    import pandas as pd
    from topaz_amd import mrc
    particles = pd.read_csv(picks, sep='\t')
    with open(os.path.join(d, 'cpu.mrcs'), 'wb') as f:
        for name, coords in particles.groupby('image_name'):
            with open(os.path.join(d, str(name) + '.mrc'), 'rb') as fm:
                mic, _, _ = mrc.parse(fm.read())
            mic = mic[np.newaxis]
            _, n, m = mic.shape
            for x, y in zip(coords['x_coord'].values, coords['y_coord'].values):
                left, upper = x - S // 2, y - S // 2
                right, lower = left + S, upper + S
                c = mic[:, max(0, upper):min(n, lower), max(0, left):min(m, right)]
                c = (c - c.mean()) / c.std()
                stack = np.zeros((1, S, S), dtype=np.float32)
                stack[:, max(0, -upper):min(S + n - lower, S), max(0, -left):min(S + m - right, S)] = c
                if R != S:
                    F = np.fft.rfft2(stack)
                    F = np.concatenate([F[..., 0:R // 2, 0:R // 2 + 1], F[..., -R // 2:, 0:R // 2 + 1]], axis=-2) * (R * R / (S * S))
                    r = np.fft.irfft2(F, s=(R, R)).astype(np.float32)
                    stack = (r - r.mean()) / r.std()
                f.write(stack.tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mics', type=int, default=8)
    ap.add_argument('--picks', type=int, default=2000)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--resize', type=int, default=128)
    ap.add_argument('--cpu-runs', type=int, default=3)
    ap.add_argument('--tmp', default='/dev/shm' if os.path.isdir('/dev/shm') else None)
    a = ap.parse_args()
    d = tempfile.mkdtemp(prefix='particle_stack_', dir=a.tmp)
    try:
        picks = make_inputs(d, a.mics, a.picks)
        print(f'# {a.mics} synthetic 4096^2 float32 micrographs (Poisson 5000), {a.picks} picks each; output on {d}')
        for R in (a.size, a.resize):
            label = f'S = {a.size}' + (f' -> R = {R}' if R != a.size else '')
            print(f'\n== {label}')
            print('device kernels (library profiler):')
            for line in device_kernels(picks, d, a.size, R, a.mics):
                print(line)
            print(f'CLI wall time: {cli_wall(picks, d, a.size, R, a.mics):.1f} ms per micrograph')
            numpy_reference(picks, d, a.size, R)                         # warm-up
            ts = []
            for _ in range(a.cpu_runs):
                t0 = time.perf_counter()
                numpy_reference(picks, d, a.size, R)
                ts.append((time.perf_counter() - t0) / a.mics * 1e3)
            print(f'numpy restatement of the reference loop (CPU baseline): median {np.median(ts):.1f} ms per micrograph, '
                  f'spread {min(ts):.1f} .. {max(ts):.1f} ({a.cpu_runs} runs after 1 warm-up)')
            sys.stdout.flush()
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == '__main__':
    main()
