"""Measure `topaz segment` on one MI355X (the numbers behind profiles/segment_stream.txt and DESIGN.md section 17).

    python tools/bench_segment.py [--mics 16] [--size 4096] [--patch 1024] [--runs 3] [--tmp /dev/shm] [--tree DIR]

Workload: `--mics` synthetic `--size`^2 MRC micrographs (seeded Poisson(5000) counts with darker discs, normalised) on tmpfs, once
stored as float32 and once as int16, through `commands.segment.segment_images` with `resnet8_u32`, the maps written to tmpfs.
Legs, each 1 warm-up and --runs timed runs (files per second and ms per micrograph: median and spread; a run ends when every
map is on disk):
  - whole image, float32 inputs and int16 inputs,
  - `-p PATCH`, float32 inputs,
  - `--format mrc --float16`, float32 inputs (a tree without the flag: not measured),
  - `extract -m none` over the TIFF maps of the first leg: score_images(None, ...) into the device suppression.
--tree DIR measures the `topaz_amd` package found in DIR (another checkout, built) instead of this one; the tool only uses what
every version of the package has, so it runs unchanged on a tree whose `segment` is the per-file loop.
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


def make_inputs(d, n_mics, size):
    """(float32 paths, int16 paths) of the same micrographs: normalised pixels as float32, 1000 x those rounded as int16"""
    from topaz_amd import mrc
    rng = np.random.RandomState(355)
    yy, xx = np.mgrid[0:size, 0:size]
    f32, i16 = [], []
    os.makedirs(os.path.join(d, 'f32'))
    os.makedirs(os.path.join(d, 'i16'))
    for i in range(n_mics):
        x = rng.poisson(5000, (size, size)).astype(np.float32)
        for cy, cx in rng.randint(0, size, size=(40, 2)):
            y0, y1, x0, x1 = max(0, cy - 64), min(size, cy + 64), max(0, cx - 64), min(size, cx + 64)
            disc = ((yy[y0:y1, x0:x1] - cy) ** 2 + (xx[y0:y1, x0:x1] - cx) ** 2) <= 60 ** 2
            x[y0:y1, x0:x1] -= 150 * disc
        x = (x - x.mean()) / x.std()
        p = os.path.join(d, 'f32', f'mic{i:02d}.mrc')
        with open(p, 'wb') as f:
            mrc.write(f, x[None])
        f32.append(p)
        q = np.round(x * 1000).astype(np.int16)
        header = mrc.make_header((1, size, size), (1, 1, 1), (0, 0, 0))._replace(mode=1)
        p = os.path.join(d, 'i16', f'mic{i:02d}.mrc')
        with open(p, 'wb') as f:
            f.write(mrc.header_struct.pack(*list(header)))
            f.write(q.tobytes())
        i16.append(p)
    return f32, i16


def timed(label, leg, n_files, runs):
    leg()                                                             # warm-up (code objects, pinned rings, workspaces)
    rates = []
    for _ in range(runs):
        t0 = time.perf_counter()
        leg()
        rates.append(n_files / (time.perf_counter() - t0))
    med = float(np.median(rates))
    print(f'{label}: median {med:.2f} files/s, spread {min(rates):.2f} .. {max(rates):.2f} ({runs} runs after 1 warm-up; '
          f'{1e3 / med:.1f} ms per micrograph)')
    sys.stdout.flush()
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mics', type=int, default=16)
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--patch', type=int, default=1024)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--model', default='resnet8_u32')
    ap.add_argument('--radius', type=int, default=8)
    ap.add_argument('--tmp', default='/dev/shm' if os.path.isdir('/dev/shm') else None)
    ap.add_argument('--tree', default=ROOT, help='checkout whose topaz_amd package is measured (default: this one)')
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    import topaz_amd
    from topaz_amd.commands import segment
    from topaz_amd.extract import nms_iterator, score_images
    from topaz_amd.model.factory import load_model
    assert torch.cuda.is_available(), 'bench_segment needs the MI355X: nothing is measured without it'
    streams = 'fmt' in inspect.signature(segment.segment_images).parameters
    d = tempfile.mkdtemp(prefix='segment_', dir=a.tmp)
    try:
        f32, i16 = make_inputs(d, a.mics, a.size)
        model = load_model(a.model)
        model.eval(); model.fill(); model.cuda(0)
        print(f'# package: {os.path.dirname(topaz_amd.__file__)}  (segment streams: {"yes" if streams else "no"})')
        print(f'# {a.mics} synthetic {a.size}^2 MRC micrographs (float32 and int16) on {d}; {a.model}; maps written there too')

        def seg(paths, out, patch=None, **kw):
            def leg():
                segment.segment_images(model, paths, os.path.join(d, out), True, False, patch, **kw)
                torch.cuda.synchronize()
            return leg

        timed('whole image, float32 inputs', seg(f32, 'whole_f32'), a.mics, a.runs)
        timed('whole image, int16 inputs', seg(i16, 'whole_i16'), a.mics, a.runs)
        timed(f'-p {a.patch}, float32 inputs', seg(f32, 'patched', a.patch), a.mics, a.runs)
        if streams:
            timed('--format mrc --float16, float32 inputs', seg(f32, 'half', fmt='mrc', float16=True), a.mics, a.runs)
        else:
            print('--format mrc --float16: not measured (this tree has no such flag)')
        maps = [os.path.join(d, 'whole_f32', os.path.splitext(os.path.basename(p))[0] + '.tiff') for p in f32]

        def picks():
            n = 0
            for _, scores, _ in nms_iterator(score_images(None, maps, device=0, keep_on_device=True), a.radius, -6.0):
                n += len(scores)
            torch.cuda.synchronize()
            return n

        timed(f'extract -m none -r {a.radius} over the TIFF maps ({picks()} picks)', picks, a.mics, a.runs)
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == '__main__':
    main()
