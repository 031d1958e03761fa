"""Measure `topaz denoise` with its options on one MI355X (the numbers behind profiles/denoise_options.txt and DESIGN.md §14).

    python tools/bench_denoise_options.py [--size 4096] [--mics 8] [--runs 5] [--model unet-v0.2.1] [--tmp /dev/shm] [--tree DIR]
                                          [--legs image,stream,filter,stack]

Workload: synthetic `--size`^2 float32 micrographs (seeded Poisson(5000) counts, one pixel in 2000 hot), the packaged `--model`,
the CLI's tiling (1024 / 500), output not normalised.  Every figure: 1 warm-up, `--runs` timed repetitions, median and spread.
  image   per micrograph in process, numpy in and numpy out: denoise_image (the host passes around the device calls) against
          denoise_image_device (upload, every pass on the device, download), for --pixel-cutoff 3, --gaussian 2 and both; the
          device function also with the micrograph already resident and the result left there
  stream  `--mics` MRC files on tmpfs through denoise_stream, MRC output on tmpfs, the same three option sets
  filter  tpz_filter_2d (conv_direct_kernel, one channel in and out) alone at `--size`^2 for k = 13, 21 and 31, between HIP events
  stack   denoise_stack with --pixel-cutoff 3 on a 16 x 2048^2 and a 512 x 128^2 float32 stack on tmpfs: time per section
--tree DIR measures the `topaz_amd` package found in DIR (another checkout, built) instead of this one; the tool only uses what
every version of the package has (the `image` leg skips the device function where it lacks the options), so a parent commit is
measured by the same program on the same box.
"""
from __future__ import annotations

import argparse
import inspect
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILING = dict(patch_size=1024, padding=500, normalize=False)


def micrograph(rng, size):
    x = rng.poisson(5000, (size, size)).astype(np.float32)
    hot = rng.randint(0, x.size, size=x.size // 2000)
    x.reshape(-1)[hot] += 4000                                   # what --pixel-cutoff is for
    return x


def timed(fn, runs, sync=None):
    """seconds of `runs` calls after one warm-up"""
    fn()
    if sync:
        sync()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        if sync:
            sync()
        ts.append(time.perf_counter() - t0)
    return ts


def line(label, ts, per=1, unit='ms'):
    ms = np.asarray(ts) * 1e3 / per
    return f'{label:58s} median {np.median(ms):9.2f} {unit}   spread {ms.min():9.2f} .. {ms.max():9.2f}   ({len(ts)} runs after 1 warm-up)'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--mics', type=int, default=8)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--model', default='unet-v0.2.1', help='a packaged model (the v0.2.2 blob behind the alias unet is not packaged)')
    ap.add_argument('--legs', default='image,stream,filter,stack')
    ap.add_argument('--tmp', default='/dev/shm' if os.path.isdir('/dev/shm') else None)
    ap.add_argument('--tree', default=ROOT, help='checkout whose topaz_amd package is measured (default: this one)')
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    import topaz_amd
    from topaz_amd import denoise as dn, mrc, runtime as rt
    from topaz_amd.filters import GaussianDenoise
    legs = a.legs.split(',')
    has_options = 'cutoff' in inspect.signature(dn.denoise_image_device).parameters
    print(f'# package: {os.path.dirname(topaz_amd.__file__)}  (denoise_image_device takes the options: {"yes" if has_options else "no"})')
    print(f'# {torch.cuda.get_device_name(0)}; model {a.model}; {a.size}^2 float32 micrographs; tiling {TILING}')
    model = [dn.Denoise(a.model)]
    gaus = GaussianDenoise(2)
    option_sets = [('--pixel-cutoff 3', dict(cutoff=3)), ('--gaussian 2', dict(gaus=gaus)),
                   ('--pixel-cutoff 3 --gaussian 2', dict(cutoff=3, gaus=gaus))]
    sync = torch.cuda.synchronize
    rng = np.random.RandomState(355)
    d = tempfile.mkdtemp(prefix='denoise_options_', dir=a.tmp)
    try:
        if 'image' in legs:
            print('\n== per micrograph, in process (ms per micrograph)')
            x = micrograph(rng, a.size)
            xd = torch.from_numpy(x).cuda()
            for label, kw in option_sets:
                print(line(f'{label}: denoise_image, numpy in / out', timed(lambda: dn.denoise_image(x, model, deconvolve=False, **kw, **TILING), a.runs)))
                if has_options:
                    print(line(f'{label}: denoise_image_device, numpy in / out',
                               timed(lambda: dn.denoise_image_device(torch.from_numpy(x).cuda(), model, **kw, **TILING).cpu().numpy(), a.runs)))
                    print(line(f'{label}: denoise_image_device, resident',
                               timed(lambda: dn.denoise_image_device(xd, model, **kw, **TILING), a.runs, sync)))
                sys.stdout.flush()
            print(line('no option: denoise_image_device, resident', timed(lambda: dn.denoise_image_device(xd, model, **TILING), a.runs, sync)))
            print(line('the network alone (Denoise.denoise_device), resident', timed(lambda: model[0].denoise_device(xd, 1024, 500), a.runs, sync)))
        if 'stream' in legs:
            print(f'\n== denoise_stream, {a.mics} MRC files on {d}, MRC output there too (ms per micrograph)')
            paths = []
            for i in range(a.mics):
                paths.append(os.path.join(d, f'mic{i:02d}.mrc'))
                with open(paths[-1], 'wb') as f:
                    mrc.write(f, micrograph(rng, a.size)[None])
            for label, kw in option_sets:
                kw = dict(kw)
                kw['pixel_cutoff'] = kw.pop('cutoff', 0)
                ts = timed(lambda: dn.denoise_stream(paths, os.path.join(d, 'out'), models=model, deconvolve=False, return_images=False,
                                                     **kw, **TILING), a.runs)
                print(line(label, ts, per=a.mics))
                sys.stdout.flush()
            for p in paths:
                os.unlink(p)
            shutil.rmtree(os.path.join(d, 'out'), ignore_errors=True)
        if 'filter' in legs:
            print(f'\n== tpz_filter_2d (conv_direct_kernel) alone on a resident {a.size}^2 image (ms per call, HIP events)')
            xd = torch.from_numpy(micrograph(rng, a.size)).cuda()
            for k in (13, 21, 31):
                w = np.random.RandomState(k).randn(k, k).astype(np.float32)
                rt.filter_2d(xd, w)
                ms = []
                for _ in range(a.runs):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    rt.filter_2d(xd, w)
                    e1.record()
                    e1.synchronize()
                    ms.append(e0.elapsed_time(e1) / 1e3)
                gflops = 2.0 * k * k * a.size * a.size / np.median(ms) / 1e9
                print(line(f'k = {k}', ms) + f'   {gflops:8.0f} GFLOP/s')
            sys.stdout.flush()
        if 'stack' in legs:
            print(f'\n== denoise_stack --pixel-cutoff 3, float32 stacks on {d} (ms per section)')
            for nz, n in ((16, 2048), (512, 128)):
                src, dst = os.path.join(d, 'stack.mrc'), os.path.join(d, 'stack_out.mrc')
                with open(src, 'wb') as f:
                    mrc.write(f, np.stack([micrograph(rng, n) for _ in range(nz)]))
                devnull = open(os.devnull, 'w')
                saved, sys.stderr = sys.stderr, devnull                   # (one progress line per section)
                try:
                    ts = timed(lambda: dn.denoise_stack(src, dst, model, pixel_cutoff=3, deconvolve=False, **TILING), a.runs)
                finally:
                    sys.stderr = saved
                    devnull.close()
                print(line(f'{nz} x {n}^2', ts, per=nz))
                sys.stdout.flush()
                os.unlink(src)
                os.unlink(dst)
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == '__main__':
    main()
