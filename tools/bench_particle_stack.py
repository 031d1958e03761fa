"""Measure `topaz particle_stack` on one MI355X (the numbers behind profiles/particle_stack.txt and DESIGN.md section 8).

    python tools/bench_particle_stack.py [--mics 8] [--picks 2000] [--size 256] [--resize 128] [--cpu-runs 3] [--tmp /dev/shm]
                                         [--fused | --fused-only] [--two-command-root DIR]

Workload: `--mics` synthetic 4096^2 float32 micrographs (seeded Poisson(5000) counts) with `--picks` picks each (uniform over
the image, boxes cut by the edges included), run once at --size and once at --size -> --resize.  Reports
  - device ms per micrograph of each kernel (the library profiler: HIP events around every launch), the algorithmic HBM bytes
    of those launches and the fraction of 8 TB/s they represent,
  - the wall time of the whole CLI (`python -m topaz_amd particle_stack`, interpreter start included) per micrograph, output on
    tmpfs,
  - the same workload through a numpy restatement of the reference loop (topaz/utils/picks.py:132-163, the resize as the
    per-frame 2-D truncated DFT) on the same host: 1 warm-up and --cpu-runs timed runs, median and spread.
With --fused / --fused-only also (or only) the leg behind profiles/extract_particle_stack.txt and DESIGN.md section 13:
`extract --particle-stack` against `extract` followed by `particle_stack` on the same micrographs (fused_leg); with
--two-command-root DIR the two commands run from the source tree DIR, e.g. a checkout of the parent commit with its built library.
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


# raw frames -> picks in the raw frame (--preprocess-sample 1: no RNG draw, every run writes the same table)
EXTRACT = '-m resnet8_u32 -r 8 -t -100 -d 0 --preprocess 4 --preprocess-sample 1 -x 4'


def _cli(argv, root=ROOT):
    t0 = time.perf_counter()
    subprocess.run([sys.executable, '-m', 'topaz_amd'] + argv, cwd=root, check=True, capture_output=True)
    return time.perf_counter() - t0


def _particle_kernels(ctx, n_mics):
    rows = [r for r in ctx.prof_kernels() if r[0].startswith('particle_')]
    return sum(r[1] for r in rows) / n_mics, sum(r[2] for r in rows)


def fused_leg(d, S, R, n_mics, n_picks, extract_args, two_root=ROOT, runs=3):
    """`extract --particle-stack` against `extract` followed by `particle_stack` on the same micrographs: CLI wall time per
    micrograph of both (median of `runs`, output on the same tmpfs) and the device time of the particle kernels in both (library
    profiler, in process).  The stack threshold is the score that keeps n_picks picks per micrograph of the table `extract`
    writes, so both legs cut the pick count the rest of this tool uses.  two_root: the source tree whose `python -m topaz_amd`
    runs the two-command leg (a checkout of the parent commit, to measure against the code before the fused command)."""
    EXTRACT = extract_args.split()
    import pandas as pd
    from topaz_amd import runtime as rt
    from topaz_amd.main import main as topaz
    mics = [os.path.join(d, f'mic{i}.mrc') for i in range(n_mics)]
    table = os.path.join(d, 'extract_picks.txt')
    stack_args = ['--size', str(S)] + (['--resize', str(R)] if R != S else [])
    fused_args = ['--particle-size', str(S)] + (['--particle-resize', str(R)] if R != S else [])
    _cli(['extract'] + EXTRACT + ['-o', table] + mics)                                   # warm-up (page cache, code objects)
    scores = np.sort(pd.read_csv(table, sep='\t').score.values)[::-1]
    kept = min(len(scores), n_picks * n_mics)
    T = repr(float(scores[kept - 1]))
    lines = [f'  extract {" ".join(EXTRACT)}: {len(scores)} picks in the table, {kept} with score >= {T} go into the stack']
    two, one = [], []
    for _ in range(runs):
        t = _cli(['extract'] + EXTRACT + ['-o', table] + mics, two_root)
        t += _cli(['particle_stack', table, '--image-root', d, '--threshold', T, '-o', os.path.join(d, 'two.mrcs')] + stack_args,
                  two_root)
        two.append(t / n_mics * 1e3)
        one.append(_cli(['extract'] + EXTRACT + ['-o', os.path.join(d, 'fused_picks.txt'), '--particle-stack',
                                                 os.path.join(d, 'fused.mrcs'), '--particle-threshold', T] + fused_args + mics)
                   / n_mics * 1e3)
    import filecmp
    same = filecmp.cmp(os.path.join(d, 'two.mrcs'), os.path.join(d, 'fused.mrcs'), shallow=False)
    lines.append(f'  CLI wall time, extract then particle_stack: median {np.median(two):.1f} ms per micrograph '
                 f'({min(two):.1f} .. {max(two):.1f}, {runs} runs)')
    lines.append(f'  CLI wall time, extract --particle-stack:    median {np.median(one):.1f} ms per micrograph '
                 f'({min(one):.1f} .. {max(one):.1f}, {runs} runs); stacks byte-identical: {same}')
    # device time of the particle kernels, in process: the fused command launches what particle_stack launches
    ctx = rt.get_context(0)
    for label, argv in (('particle_stack', ['particle_stack', table, '--image-root', d, '--threshold', T, '-o',
                                            os.path.join(d, 'two.mrcs')] + stack_args),
                        ('extract --particle-stack', ['extract'] + EXTRACT + ['-o', os.path.join(d, 'fused_picks.txt'),
                                                      '--particle-stack', os.path.join(d, 'fused.mrcs'), '--particle-threshold', T]
                         + fused_args + mics)):
        topaz(argv)                                                                          # warm-up
        ctx.prof_enable(1)
        ctx.prof_reset()
        topaz(argv)
        ctx.sync()
        ms, n = _particle_kernels(ctx, n_mics)
        ctx.prof_enable(0)
        lines.append(f'  particle kernels in {label}: {ms:.3f} ms per micrograph, {n} launches')
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mics', type=int, default=8)
    ap.add_argument('--picks', type=int, default=2000)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--resize', type=int, default=128)
    ap.add_argument('--cpu-runs', type=int, default=3)
    ap.add_argument('--tmp', default='/dev/shm' if os.path.isdir('/dev/shm') else None)
    ap.add_argument('--fused', action='store_true', help='also measure extract --particle-stack against extract + particle_stack')
    ap.add_argument('--fused-only', action='store_true', help='only that')
    ap.add_argument('--extract-args', default=EXTRACT, help='the extract flags of the fused leg')
    ap.add_argument('--two-command-root', default=ROOT, help='source tree that runs the two-command leg (default: this one)')
    a = ap.parse_args()
    d = tempfile.mkdtemp(prefix='particle_stack_', dir=a.tmp)
    try:
        picks = make_inputs(d, a.mics, a.picks)
        print(f'# {a.mics} synthetic 4096^2 float32 micrographs (Poisson 5000), {a.picks} picks each; output on {d}')
        for R in (a.size, a.resize):
            label = f'S = {a.size}' + (f' -> R = {R}' if R != a.size else '')
            print(f'\n== {label}')
            if a.fused or a.fused_only:
                print(f'extract --particle-stack against extract + particle_stack (two-command leg from {a.two_command_root}):'
                      if a.two_command_root != ROOT else 'extract --particle-stack against extract + particle_stack:')
                for line in fused_leg(d, a.size, R, a.mics, a.picks, a.extract_args, a.two_command_root):
                    print(line)
                sys.stdout.flush()
                if a.fused_only:
                    continue
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
