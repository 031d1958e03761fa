"""Measure `topaz preprocess` on one MI355X (the numbers behind profiles/preprocess_stream.txt and DESIGN.md section 10).

    python tools/bench_preprocess.py [--mics 16] [--size 4096] [--sample 10] [--runs 3] [--tmp /dev/shm] [--tree DIR]

Workload: `--mics` synthetic `--size`^2 float32 MRC micrographs (seeded Poisson(5000) counts with darker discs) on tmpfs, through
`stats.normalize_images` with the flags of `preprocess -s 4 --sample N` and of `-s 1 --sample N`, MRC output on tmpfs.  Reports
  - files per second of normalize_images: 1 warm-up and --runs timed runs, median and spread,
  - where a tree has the device stream, the same files through its per-file `Normalize` loop (the serial path the stream is
    tested against) in the same process,
  - one further run with every stage timed: the device-side stages between HIP events on the stream they run on, the host-side
    ones (file decode, np.random.choice, np.quantile, the numpy normalisation, the file writers) on the host clock; the sum of
    the host stages can exceed the wall time of a stream, whose reader and writer threads run under the GPU's work,
  - passes over the pixels per mixture fit, where the fit reports them.
--tree DIR measures the `topaz_amd` package found in DIR (another checkout, built) instead of this one; the tool only uses
what every version of the package has, so it runs unchanged on a tree without the stream.
"""
from __future__ import annotations

import argparse
import os
import shutil
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_inputs(d, n_mics, size):
    from topaz_amd import mrc
    rng = np.random.RandomState(355)
    yy, xx = np.mgrid[0:size, 0:size]
    paths = []
    for i in range(n_mics):
        x = rng.poisson(5000, (size, size)).astype(np.float32)
        for cy, cx in rng.randint(0, size, size=(40, 2)):
            y0, y1, x0, x1 = max(0, cy - 64), min(size, cy + 64), max(0, cx - 64), min(size, cx + 64)
            disc = ((yy[y0:y1, x0:x1] - cy) ** 2 + (xx[y0:y1, x0:x1] - cx) ** 2) <= 60 ** 2
            x[y0:y1, x0:x1] -= 150 * disc
        p = os.path.join(d, f'mic{i:02d}.mrc')
        with open(p, 'wb') as f:
            mrc.write(f, x[None])
        paths.append(p)
    return paths


class Stages:
    """wrap named functions of the package (those that exist) and time them: device stages between HIP events, host stages on
    the host clock"""

    DEVICE = [('topaz_amd.utils.image', 'downsample_device'), ('topaz_amd.utils.image', 'downsample'),
              ('topaz_amd.runtime', 'gather'), ('topaz_amd.runtime', 'order_stats'), ('topaz_amd.runtime', 'gmm_fit_fused'),
              ('topaz_amd.runtime', 'gmm_fit'), ('topaz_amd.runtime', 'normalize_f64')]
    HOST = [('topaz_amd.utils.image', 'load_image'), ('topaz_amd.mrc', 'read_into'), ('numpy.random', 'choice'),
            ('numpy', 'quantile'), ('topaz_amd.utils.image', 'save_image')]

    def __init__(self):
        import importlib
        import torch
        self.torch, self.lock = torch, threading.Lock()
        self.events, self.host, self.passes, self.saved, self.depth = {}, {}, [], [], threading.local()
        for device, table in ((True, self.DEVICE), (False, self.HOST)):
            for modname, attr in table:
                mod = importlib.import_module(modname)
                if hasattr(mod, attr):
                    self.saved.append((mod, attr, getattr(mod, attr)))
                    setattr(mod, attr, self._wrap(f'{modname.split(".")[-1]}.{attr}', getattr(mod, attr), device))

    def _wrap(self, label, fn, device):
        def timed(*a, **kw):
            # (a wrapped function called from inside a wrapped one -- downsample -> downsample_device -- is timed once, outermost)
            nested = getattr(self.depth, 'n', 0) > 0
            self.depth.n = getattr(self.depth, 'n', 0) + 1
            try:
                if nested:
                    return fn(*a, **kw)
                if device:
                    e0, e1 = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
                    e0.record()
                t0 = time.perf_counter()
                out = fn(*a, **kw)
                dt = time.perf_counter() - t0
                if device:
                    e1.record()
                    with self.lock:
                        self.events.setdefault(label, []).append((e0, e1))
                    if label.endswith('gmm_fit_fused'):
                        self.passes.append(out[-1])
                with self.lock:
                    self.host[label] = self.host.get(label, 0.0) + dt
                return out
            finally:
                self.depth.n -= 1
        return timed

    def restore(self):
        for mod, attr, fn in self.saved:
            setattr(mod, attr, fn)

    def report(self, n_mics):
        self.torch.cuda.synchronize()
        lines = []
        for label, pairs in self.events.items():
            ms = sum(a.elapsed_time(b) for a, b in pairs)
            lines.append(f'  device  {label:28s} {ms / n_mics:9.3f} ms/mic on the stream   {self.host[label] * 1e3 / n_mics:9.3f} ms/mic '
                         f'in the call (host)   {len(pairs) // max(n_mics, 1):3d} calls/mic')
        for label, s in self.host.items():
            if label not in self.events:
                lines.append(f'  host    {label:28s} {s * 1e3 / n_mics:9.3f} ms/mic')
        if self.passes:
            lines.append(f'  passes over the pixels per fit: mean {np.mean(self.passes):.1f}, min {min(self.passes)}, max {max(self.passes)}')
        else:
            lines.append('  passes over the pixels per fit: not reported by this tree (one pass per initialisation and EM iteration)')
        return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mics', type=int, default=16)
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--sample', type=int, default=10)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--scales', default='4,1')
    ap.add_argument('--tmp', default='/dev/shm' if os.path.isdir('/dev/shm') else None)
    ap.add_argument('--tree', default=ROOT, help='checkout whose topaz_amd package is measured (default: this one)')
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import topaz_amd
    from topaz_amd import stats
    has_stream = hasattr(stats, 'normalize_device')
    d = tempfile.mkdtemp(prefix='preprocess_', dir=a.tmp)
    try:
        paths = make_inputs(d, a.mics, a.size)
        print(f'# package: {os.path.dirname(topaz_amd.__file__)}  (device stream: {"yes" if has_stream else "no"})')
        print(f'# {a.mics} synthetic {a.size}^2 float32 MRC micrographs (Poisson 5000 with darker discs) on {d}; MRC output there too')

        def run_images(scale, out):
            np.random.seed(7)
            stats.normalize_images(paths, out, 0, scale, False, 100, 900, 1, a.sample, False, ['mrc'])

        def run_per_file(scale, out):
            np.random.seed(7)
            os.makedirs(out, exist_ok=True)
            worker = stats.Normalize(out, scale, False, 100, 900, 1, a.sample, False, ['mrc'])
            for p in paths:
                worker(p)

        for scale in [int(s) for s in a.scales.split(',')]:
            print(f'\n== preprocess -s {scale} --sample {a.sample}')
            legs = [('normalize_images', run_images)] + ([('per-file Normalize loop', run_per_file)] if has_stream else [])
            rates = {}
            for label, leg in legs:
                out = os.path.join(d, 'out')
                leg(scale, out)                                           # warm-up (operators, pinned rings, workspaces)
                ts = []
                for _ in range(a.runs):
                    t0 = time.perf_counter()
                    leg(scale, out)
                    ts.append(a.mics / (time.perf_counter() - t0))
                rates[label] = float(np.median(ts))
                print(f'{label}: median {np.median(ts):.2f} files/s, spread {min(ts):.2f} .. {max(ts):.2f} '
                      f'({a.runs} runs after 1 warm-up; {1e3 / np.median(ts):.1f} ms per micrograph)')
                sys.stdout.flush()
            if has_stream:
                print(f'stream / per-file: {rates["normalize_images"] / rates["per-file Normalize loop"]:.2f} x')
            st = Stages()
            try:
                t0 = time.perf_counter()
                run_images(scale, os.path.join(d, 'out'))
                wall = time.perf_counter() - t0
            finally:
                st.restore()
            print(f'stages of one more normalize_images run ({wall * 1e3 / a.mics:.1f} ms per micrograph with the timers in):')
            for line in st.report(a.mics):
                print(line)
            sys.stdout.flush()
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == '__main__':
    main()
