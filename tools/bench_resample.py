"""Measure the truncated-DFT downsample on one MI355X (the numbers behind profiles/resample.txt and DESIGN.md section 12).

    python tools/bench_resample.py [--parent DIR] [--reps 10] [--mics 16] [--tmp /dev/shm] [--no-split] [--no-fused]

Three parts, each printed as it finishes:

  legs    `utils.image.downsample_device` of a tree on the shapes 4096^2 -> 1024^2, 4096^2 -> 512^2, 5760x4092 -> 1440x1023 and
          3838x3710 -> 959x927 (Poisson(5000) counts resident on the device): 2 warm-up calls (operators, plans, workspaces), then
          --reps calls, each between HIP events on the stream and on the host clock; median and spread of both.  With --parent DIR
          (another checkout of this project, built) the legs run as child processes in the order parent, this tree, parent -- one
          visit of one box, the parent on both sides of the tree under test.  Without it only this tree is measured.
  split   where the time of the composite this tree replaced goes (two tpz_conv 1x1 GEMMs, two transposes, one torch.cat),
          re-stated here from entry points this tree still has, 4096^2 -> 1024^2: host time of every call, the kernels' own time
          from the in-library profiler (HIP events around each launch), and for scale a 32 MB host-to-device copy by itself.
          tpz_conv builds, packs, uploads, runs, synchronises and frees inside one call: packing, upload and free are not timed
          apart from each other -- they are the call's host time minus its kernel time.
  fused   `topaz extract --preprocess 4` against `topaz preprocess -s 4` followed by `topaz extract`, --mics synthetic 4096^2
          micrographs on --tmp, resnet16_u32, in process: 1 warm-up and 2 timed runs of each flow.
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [((4096, 4096), (1024, 1024)), ((4096, 4096), (512, 512)), ((5760, 4092), (1440, 1023)), ((3838, 3710), (959, 927))]


def _counts(shape, seed=355):
    import torch
    return torch.from_numpy(np.random.RandomState(seed).poisson(5000, shape).astype(np.float32)).cuda()


def leg(tree, reps):
    """one tree's downsample_device on every shape -> JSON on stdout (run as a child process: one package per process)"""
    sys.path.insert(0, os.path.abspath(tree))
    import torch
    import topaz_amd
    from topaz_amd.utils.image import downsample_device
    rows = []
    for shape_in, shape_out in SHAPES:
        x = _counts(shape_in)
        for _ in range(2):
            downsample_device(x, shape=shape_out)
        torch.cuda.synchronize()
        dev, host = [], []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            y = downsample_device(x, shape=shape_out)
            host.append((time.perf_counter() - t0) * 1e3)
            e1.record()
            e1.synchronize()
            dev.append(e0.elapsed_time(e1))
        assert tuple(y.shape) == shape_out
        rows.append(dict(shape_in=shape_in, shape_out=shape_out, stream_ms=dev, host_ms=host))
        del x, y
    print(json.dumps(dict(package=os.path.dirname(topaz_amd.__file__), rows=rows)))


def _fmt(v):
    return f'{np.median(v):9.3f} ({min(v):.3f} .. {max(v):.3f})'


def run_legs(parent, reps):
    order = [('this tree', ROOT)] if not parent else [('parent', parent), ('this tree', ROOT), ('parent', parent)]
    print(f'== downsample_device, {reps} calls after 2 warm-up calls; ms per call: median (min .. max)')
    medians = {}
    for label, tree in order:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--leg', os.path.abspath(tree), '--reps', str(reps)],
                           capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            print(f'{label}: leg failed ({r.returncode})\n{r.stderr[-2000:]}')
            continue
        out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
        print(f'-- {label}: {out["package"]}')
        for row in out['rows']:
            (M, N), (m, n) = row['shape_in'], row['shape_out']
            print(f'  {M}x{N} -> {m}x{n}:  on the stream {_fmt(row["stream_ms"])}   in the call (host) {_fmt(row["host_ms"])}')
            medians.setdefault((label, M, N, m, n), []).append(float(np.median(row['stream_ms'])))
        sys.stdout.flush()
    if parent:
        print('-- parent / this tree (medians on the stream; the parent as the mean of its two legs)')
        for (M, N), (m, n) in SHAPES:
            p, t = medians.get(('parent', M, N, m, n)), medians.get(('this tree', M, N, m, n))
            if p and t:
                print(f'  {M}x{N} -> {m}x{n}:  {np.mean(p):.3f} ms / {t[0]:.3f} ms = {np.mean(p) / t[0]:.1f} x')


def run_split(reps):
    sys.path.insert(0, ROOT)
    import torch
    from topaz_amd import runtime as rt
    from topaz_amd.utils.image import _downsample_operators
    (M, N), (m, n) = SHAPES[0]
    ctx = rt.get_context()
    L, R = _downsample_operators(M, N, m, n)
    x = _counts((M, N))
    Lw, Rw = L.reshape(2 * m, M, 1, 1), R.reshape(n, 2 * N, 1, 1)
    steps = ('conv 1 (L, 32 MB of weights)', 'transpose 1', 'torch.cat', 'conv 2 (R, 32 MB of weights)', 'transpose 2')
    host = {s: [] for s in steps}
    kern = {0: [], 2: []}
    total = []

    def timed(label, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        host[label].append((time.perf_counter() - t0) * 1e3)
        return out

    for rep in range(reps + 1):
        ctx.prof_enable(1)
        ctx.prof_reset()
        t0 = time.perf_counter()
        U = timed(steps[0], lambda: rt.conv(x.reshape(M, N // 64, 64), Lw).reshape(2 * m, N))
        Ut = timed(steps[1], lambda: rt.transpose(U))
        Ucat = timed(steps[2], lambda: torch.cat([Ut[:, :m], Ut[:, m:]], 0).contiguous())
        yt = timed(steps[3], lambda: rt.conv(Ucat.reshape(2 * N, m // 64, 64), Rw).reshape(n, m))
        timed(steps[4], lambda: rt.transpose(yt))
        total.append((time.perf_counter() - t0) * 1e3)
        for cls in kern:
            kern[cls].append(ctx.prof_get(cls)[0])
        ctx.prof_enable(0)
        if rep == 0:                                                  # warm-up
            for v in list(host.values()) + list(kern.values()) + [total]:
                v.clear()
    print(f'\n== the composite this tree replaced, {M}x{N} -> {m}x{n}, {reps} runs after 1 warm-up; ms: median (min .. max)')
    print('   (every step followed by a device synchronise, so the steps add up; the in-library profiler is on)')
    for s in steps:
        print(f'  host time of the call   {s:32s} {_fmt(host[s])}')
    print(f'  host time, all five steps {"":30s} {_fmt(total)}')
    print(f'  kernel time (in-library profiler)  conv_mfma launches of both convs {_fmt(kern[0])}')
    print(f'  kernel time (in-library profiler)  elementwise launches (transposes) {_fmt(kern[2])}')
    rest = [t - a - b for t, a, b in zip(total, kern[0], kern[2])]
    print(f'  all five steps minus kernel time: model build, weight packing, upload, synchronise, free, torch.cat {_fmt(rest)}')
    h = np.ascontiguousarray(L)
    d = torch.empty(L.shape, dtype=torch.float32, device='cuda')
    copy = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d.copy_(torch.from_numpy(h))
        torch.cuda.synchronize()
        copy.append((time.perf_counter() - t0) * 1e3)
    print(f'  for scale: one {h.nbytes >> 20} MB pageable host-to-device copy by itself {_fmt(copy[1:])}  (each conv uploads one packed operator)')
    # the new entry on the same input, same process
    from topaz_amd.utils.image import downsample_device
    for _ in range(2):
        downsample_device(x, shape=(m, n))
    ctx.prof_enable(1)
    ctx.prof_reset()
    new = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        downsample_device(x, shape=(m, n))
        torch.cuda.synchronize()
        new.append((time.perf_counter() - t0) * 1e3)
    ms, launches, flops = ctx.prof_get(2)
    ctx.prof_enable(0)
    print(f'  this tree, same input: call + synchronise {_fmt(new)};  kernels {ms / reps:.3f} ms per call in {launches // reps} launches, '
          f'{flops / reps / 1e9:.1f} GFLOP per call = {flops / ms / 1e9:.1f} TFLOP/s fp32 in the kernels')
    sys.stdout.flush()


def run_fused(n_mics, tmp):
    sys.path.insert(0, ROOT)
    import torch
    from tools.bench_preprocess import make_inputs
    from topaz_amd.main import main as topaz
    d = tempfile.mkdtemp(prefix='resample_', dir=tmp)
    try:
        paths = make_inputs(d, n_mics, 4096)
        extract = ['extract', '-m', 'resnet16_u32', '-r', '8', '-d', '0']
        print(f'\n== {n_mics} synthetic 4096^2 float32 MRC micrographs on {d}: picks from raw frames, resnet16_u32, -r 8, --sample 10')

        def fused():
            np.random.seed(7)
            topaz(extract + ['--preprocess', '4', '-o', os.path.join(d, 'fused.txt')] + paths)

        def two_step():
            np.random.seed(7)
            proc = os.path.join(d, 'proc')
            t0 = time.perf_counter()
            topaz(['preprocess', '-s', '4', '-o', proc] + paths)
            t1 = time.perf_counter()
            topaz(extract + ['-o', os.path.join(d, 'two.txt')] + [os.path.join(proc, os.path.basename(p)) for p in paths])
            return t1 - t0, time.perf_counter() - t1

        for label, flow in (('two commands (preprocess -s 4 -o proc/, then extract proc/*.mrc)', two_step),
                            ('fused (extract --preprocess 4)', fused)):
            flow()                                                    # warm-up: model load, plans, pinned rings
            for run in range(2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                parts = flow()
                dt = time.perf_counter() - t0
                extra = f'  (preprocess {parts[0] * 1e3 / n_mics:.1f} + extract {parts[1] * 1e3 / n_mics:.1f})' if parts else ''
                print(f'{label}: run {run + 1}: {dt:.2f} s, {dt * 1e3 / n_mics:.1f} ms per micrograph{extra}')
                sys.stdout.flush()
        same = open(os.path.join(d, 'fused.txt'), 'rb').read() == open(os.path.join(d, 'two.txt'), 'rb').read()
        print(f'pick files of the two flows byte-identical: {"yes" if same else "NO"}')
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default=None, help='built checkout of the parent commit: legs run parent, this tree, parent')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--mics', type=int, default=16)
    ap.add_argument('--tmp', default='/dev/shm' if os.path.isdir('/dev/shm') else None)
    ap.add_argument('--no-split', action='store_true')
    ap.add_argument('--no-fused', action='store_true')
    ap.add_argument('--leg', default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg, a.reps)
    run_legs(a.parent, a.reps)
    if not a.no_split:
        run_split(a.reps)
    if not a.no_fused:
        run_fused(a.mics, a.tmp)


if __name__ == '__main__':
    main()
