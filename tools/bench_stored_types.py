"""Measure what the stored type of an MRC file costs the streaming commands on one MI355X (the numbers behind
profiles/stored_type_staging.txt and DESIGN.md section 15).

    python tools/bench_stored_types.py [--mics 16] [--size 4096] [--runs 3] [--tmp /dev/shm] [--parent DIR] [--out FILE]

Workload: `--mics` synthetic `--size`^2 micrographs on tmpfs -- the content of tools/bench_preprocess.py (seeded Poisson counts
with darker discs) at a mean of 1000 counts, so that every value is an integer below 2048 and float32, int16 and float16 files
hold exactly the same pixels -- written once per type.  Per type, 1 warm-up and --runs timed runs (median and spread) of
  - `topaz preprocess -s 4` (MRC output on tmpfs), ms per micrograph,
  - `topaz extract --preprocess 4 -m resnet8_u32 -r 8`, ms per micrograph,
  - the feed alone: `ImageFeed` over the files with a consumer that does nothing (read, upload, decode; no command around it),
and from one further run of `preprocess -s 4` with counters in: the time the feed's reader thread spends in the MRC reader
(mrc.read_into / mrc.read_stored_into, without the wait for a free slot inside it) and the pixel bytes queued host -> device
(the sizes handed to the staging ring's upload calls; where the feed counts them itself, `ImageFeed.uploaded_bytes`, that figure
is printed next to it).
One more leg: an int16 volume of 256 x 512 x 512 from the tomogram reader of `topaz denoise3d` to the float32 device tensor the
tiling starts from (read-to-first-tile), --runs times after a warm-up.

--parent DIR: a built checkout of another commit (its topaz_amd package).  Every leg then runs on both trees, one child process
per tree, the same files, the same box, one job; the reading compares this tree with the parent's figures, never with its own.
The tool only uses what both versions of the package have, so it runs unchanged on a tree without the device decode.
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = [('float32', np.float32, 2), ('int16', np.int16, 1), ('float16', np.float16, 12)]
VOLUME = (256, 512, 512)


def write_stored(path, x, mrc):
    mode = {np.dtype(d): m for _, d, m in TYPES}[x.dtype]
    shape = x.shape if x.ndim == 3 else (1,) + x.shape
    with open(path, 'wb') as f:
        f.write(mrc.header_struct.pack(*list(mrc.make_header(shape, (1, 1, 1), (0, 0, 0))._replace(mode=mode))))
        f.write(memoryview(np.ascontiguousarray(x).reshape(-1).view(np.uint8)))


def make_inputs(d, n_mics, size):
    """{type name: paths}; the files of a type live in a directory of their own under the same names"""
    sys.path.insert(0, ROOT)
    from topaz_amd import mrc
    rng = np.random.RandomState(355)
    yy, xx = np.mgrid[0:size, 0:size]
    for name, _, _ in TYPES:
        os.makedirs(os.path.join(d, name))
    for i in range(n_mics):
        x = rng.poisson(1000, (size, size)).astype(np.int16)
        for cy, cx in rng.randint(0, size, size=(40, 2)):
            y0, y1, x0, x1 = max(0, cy - 64), min(size, cy + 64), max(0, cx - 64), min(size, cx + 64)
            disc = ((yy[y0:y1, x0:x1] - cy) ** 2 + (xx[y0:y1, x0:x1] - cx) ** 2) <= 60 ** 2
            x[y0:y1, x0:x1] -= (67 * disc).astype(np.int16)      # (2.1 sigma, the contrast of 150 counts at a mean of 5000)
        assert 0 <= x.min() and x.max() < 2048
        for name, dtype, _ in TYPES:
            write_stored(os.path.join(d, name, f'mic{i:02d}.mrc'), x.astype(dtype), mrc)
    vol = rng.poisson(1000, VOLUME[1:]).astype(np.int16)
    write_stored(os.path.join(d, 'volume_int16.mrc'), np.broadcast_to(vol, VOLUME), mrc)
    return {name: [os.path.join(d, name, f'mic{i:02d}.mrc') for i in range(n_mics)] for name, _, _ in TYPES}


class Counters:
    """host time inside the MRC readers of the feed and the bytes handed to the ring's upload calls, on any version of the package"""

    def __init__(self):
        from topaz_amd import mrc, runtime as rt
        self.lock, self.read_s, self.bytes, self.saved = threading.Lock(), 0.0, 0, []
        for attr in ('read_into', 'read_stored_into'):
            if hasattr(mrc, attr):
                self._patch(mrc, attr, self._timed(getattr(mrc, attr)))
        upload = rt.Stage.upload

        def counted_upload(stage, slot, nbytes, src=None):
            with self.lock:
                self.bytes += int(nbytes)
            return upload(stage, slot, nbytes, src)
        self._patch(rt.Stage, 'upload', counted_upload)
        if hasattr(rt.Stage, 'upload_decode'):
            upload_decode = rt.Stage.upload_decode

            def counted_decode(stage, slot, mode, n):
                with self.lock:
                    self.bytes += int(n) * (1 if mode == 0 else 2)
                return upload_decode(stage, slot, mode, n)
            self._patch(rt.Stage, 'upload_decode', counted_decode)

    def _patch(self, owner, attr, fn):
        self.saved.append((owner, attr, getattr(owner, attr)))
        setattr(owner, attr, fn)

    def _timed(self, fn):
        """time in the reader minus the time in its `alloc` (the feed's wait for a free slot: the consumer's time, not the read's)"""
        def timed(path, alloc):
            waited = [0.0]

            def timed_alloc(*a, **kw):
                t = time.perf_counter()
                try:
                    return alloc(*a, **kw)
                finally:
                    waited[0] += time.perf_counter() - t
            t0 = time.perf_counter()
            try:
                return fn(path, timed_alloc)
            finally:
                with self.lock:
                    self.read_s += time.perf_counter() - t0 - waited[0]
        return timed

    def restore(self):
        for owner, attr, fn in self.saved:
            setattr(owner, attr, fn)


def _timed_runs(fn, runs):
    fn()                                                               # warm-up (operators, pinned rings, workspaces, the model)
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def leg(a):
    """the measurements of one tree, as one JSON line on stdout"""
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    import topaz_amd
    from topaz_amd import denoise, extract, runtime as rt
    from topaz_amd.main import main as topaz
    d = a.data
    paths = {name: sorted(os.path.join(d, name, f) for f in os.listdir(os.path.join(d, name))) for name, _, _ in TYPES}
    n = len(paths['float32'])
    out = {'package': os.path.dirname(topaz_amd.__file__), 'types': {}}
    ctx = rt.get_context()
    feeds = []
    feed_init = extract.ImageFeed.__init__

    def keep_feed(self, *args, **kw):
        feed_init(self, *args, **kw)
        feeds.append(self)
    extract.ImageFeed.__init__ = keep_feed
    with open(os.devnull, 'w') as null:
        stderr, sys.stderr = sys.stderr, null                         # (the commands' progress lines)
        try:
            for name, _, _ in TYPES:
                outdir = os.path.join(d, 'out_' + os.path.basename(os.path.abspath(a.tree)) + '_' + name)

                def preprocess():
                    np.random.seed(7)
                    topaz(['preprocess', '-s', '4', '-o', outdir] + paths[name])

                def pick():
                    np.random.seed(7)
                    topaz(['extract', '-m', 'resnet8_u32', '-r', '8', '--preprocess', '4', '-o', outdir + '.txt'] + paths[name])

                def feed_alone():
                    for _ in extract.ImageFeed(paths[name], ctx):
                        pass
                    torch.cuda.synchronize()

                res = {'feed_ms': [1e3 * t / n for t in _timed_runs(feed_alone, a.runs)],
                       'preprocess_ms': [1e3 * t / n for t in _timed_runs(preprocess, a.runs)],
                       'extract_ms': [1e3 * t / n for t in _timed_runs(pick, a.runs)]}
                counters = Counters()
                del feeds[:]
                try:
                    preprocess()
                finally:
                    counters.restore()
                res['read_ms'] = 1e3 * counters.read_s / n
                res['upload_bytes'] = counters.bytes / n
                res['feed_uploaded_bytes'] = (sum(f.uploaded_bytes for f in feeds) / n
                                              if feeds and hasattr(feeds[0], 'uploaded_bytes') else None)
                out['types'][name] = res
                shutil.rmtree(outdir, ignore_errors=True)
        finally:
            sys.stderr = stderr
    # denoise3d: from the file to the float32 device tensor the tiling starts from
    read, _ = denoise._tomogram_io()
    job = denoise._Job(0, os.path.join(d, 'volume_int16.mrc'), '')

    def first_tile():
        tomo = read(job)[0]
        if tomo.dtype != np.float32 and hasattr(rt, 'decode_stored'):
            x = rt.decode_stored(tomo, ctx)
        else:
            x = rt.as_device_f32(tomo, ctx)
        torch.cuda.synchronize()
        assert x.dtype == torch.float32 and tuple(x.shape) == VOLUME
    out['volume_ms'] = [1e3 * t for t in _timed_runs(first_tile, a.runs)]
    print('RESULT ' + json.dumps(out))


def _stat(v):
    return f'{np.median(v):8.2f} ({min(v):.2f} .. {max(v):.2f})'


def report(results, a):
    lines = [f'# {a.mics} synthetic {a.size}^2 micrographs (Poisson 1000 with darker discs, integers below 2048: the same pixels in '
             f'every type) on tmpfs; 1 warm-up + {a.runs} timed runs, median (min .. max); ms per micrograph',
             '# feed alone: ImageFeed over the files with a consumer that does nothing; preprocess: `topaz preprocess -s 4`; extract: '
             "`topaz extract --preprocess 4 -m resnet8_u32 -r 8`; read: host time of the feed's MRC reader without its wait for a free "
             "slot; H2D: pixel bytes per micrograph handed to the ring's upload calls (feed: ImageFeed.uploaded_bytes)"]
    for tag, r in results:
        lines.append(f'\n== {tag}: {r["package"]}')
        lines.append(f'{"type":8s} {"feed alone":>26s} {"preprocess -s 4":>26s} {"extract --preprocess 4":>26s} {"read":>9s} {"H2D bytes":>12s} {"feed":>12s}')
        for name, _, _ in TYPES:
            t = r['types'][name]
            fed = '-' if t['feed_uploaded_bytes'] is None else f'{t["feed_uploaded_bytes"]:.0f}'
            lines.append(f'{name:8s} {_stat(t["feed_ms"]):>26s} {_stat(t["preprocess_ms"]):>26s} {_stat(t["extract_ms"]):>26s} {t["read_ms"]:9.2f} '
                         f'{t["upload_bytes"]:12.0f} {fed:>12s}')
        lines.append(f'denoise3d, int16 {VOLUME[0]}x{VOLUME[1]}x{VOLUME[2]}, file -> float32 device tensor: {_stat(r["volume_ms"])} ms')
    if len(results) == 2:
        (_, new), (_, old) = results
        lines.append('\n== reading: this tree against the parent (faster = below the parent by more than the larger of the two spreads)')
        for name, _, _ in TYPES:
            for key, label in (('feed_ms', 'feed alone'), ('preprocess_ms', 'preprocess -s 4'), ('extract_ms', 'extract --preprocess 4')):
                x, y = new['types'][name][key], old['types'][name][key]
                spread = max(max(x) - min(x), max(y) - min(y))
                delta = float(np.median(x) - np.median(y))
                verdict = 'faster' if delta < -spread else 'slower' if delta > spread else 'inside the spread'
                lines.append(f'{name:8s} {label:24s} {np.median(x):8.2f} vs {np.median(y):8.2f} ms  ({delta:+.2f} ms, '
                             f'{np.median(y) / np.median(x):.2f} x; spread {spread:.2f} ms): {verdict}')
        x, y = new['volume_ms'], old['volume_ms']
        lines.append(f'denoise3d int16 read-to-first-tile {np.median(x):8.2f} vs {np.median(y):8.2f} ms ({np.median(y) / np.median(x):.2f} x)')
    return '\n'.join(lines) + '\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mics', type=int, default=16)
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--tmp', default='/dev/shm' if os.path.isdir('/dev/shm') else None)
    ap.add_argument('--tree', default=ROOT, help='checkout whose topaz_amd package is measured (default: this one)')
    ap.add_argument('--parent', default=None, help='a second, built checkout measured on the same files (the yardstick)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'stored_type_staging.txt'))
    ap.add_argument('--leg', action='store_true', help=argparse.SUPPRESS)      # a child: one tree, JSON on stdout
    ap.add_argument('--data', default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    d = tempfile.mkdtemp(prefix='stored_types_', dir=a.tmp)
    try:
        make_inputs(d, a.mics, a.size)
        results = []
        for tag, tree in [('this tree', a.tree)] + ([('parent', a.parent)] if a.parent else []):
            # one fresh process per tree: two versions of the package (and of the library) never share a process
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--leg', '--tree', tree, '--data', d, '--runs', str(a.runs)],
                               capture_output=True, text=True)
            line = [s for s in r.stdout.split('\n') if s.startswith('RESULT ')]
            if r.returncode != 0 or not line:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit(f'the leg on {tree} failed ({r.returncode})')
            results.append((tag, json.loads(line[0][7:])))
        text = report(results, a)
        sys.stdout.write(text)
        with open(a.out, 'w') as f:
            f.write(text)
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == '__main__':
    main()
