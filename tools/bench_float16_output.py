"""Measure what `--float16` output costs or saves the commands that write MRC, on one MI355X, and whether the default float32
path moved against the parent commit (the numbers behind profiles/float16_output.txt and DESIGN.md section 16).

    python tools/bench_float16_output.py [--mics 8] [--size 4096] [--runs 3] [--tmp /dev/shm] [--parent DIR] [--out FILE]

Workload: `--mics` synthetic `--size`^2 float32 micrographs on tmpfs (seeded Poisson counts with darker discs, as
tools/bench_stored_types.py makes them) and a pick table of 400 picks per micrograph.  Per command -- `topaz denoise -m unet-v0.2.1` (the full U-Net whose weights are packaged),
`topaz preprocess -s 4`, `topaz particle_stack --size 256` -- without and with `--float16`: 1 warm-up and --runs timed runs, wall
ms per micrograph (median, min .. max), and from one further run with counters in: the bytes the result ring copied device ->
host (the sizes handed to tpz_stage_d2h / tpz_stage_d2h_encode) and the bytes of the files written, both per micrograph.

--parent DIR: a built checkout of the parent commit.  The float32 legs then run on both trees, one child process per tree, the
same files, the same box, one job.  The verdict on the default path compares the medians against the run-to-run spread (the
larger max - min of the two): "no slower" means the median is not above the parent's by more than that spread.
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
COMMANDS = ('denoise -m unet-v0.2.1', 'preprocess -s 4', 'particle_stack --size 256')
PICKS = 400


def make_inputs(d, n_mics, size):
    sys.path.insert(0, ROOT)
    from topaz_amd import mrc
    rng = np.random.RandomState(355)
    yy, xx = np.mgrid[0:size, 0:size]
    os.makedirs(os.path.join(d, 'mics'))
    rows = ['image_name\tx_coord\ty_coord\tscore']
    for i in range(n_mics):
        x = rng.poisson(1000, (size, size)).astype(np.float32)
        for cy, cx in rng.randint(0, size, size=(40, 2)):
            y0, y1, x0, x1 = max(0, cy - 64), min(size, cy + 64), max(0, cx - 64), min(size, cx + 64)
            disc = ((yy[y0:y1, x0:x1] - cy) ** 2 + (xx[y0:y1, x0:x1] - cx) ** 2) <= 60 ** 2
            x[y0:y1, x0:x1] -= (67 * disc).astype(np.float32)
        with open(os.path.join(d, 'mics', f'mic{i:02d}.mrc'), 'wb') as f:
            f.write(mrc.header_struct.pack(*list(mrc.make_header((1, size, size), (1, 1, 1), (0, 0, 0)))))
            f.write(memoryview(x.reshape(-1).view(np.uint8)))
        for px, py in rng.randint(0, size, size=(PICKS, 2)):
            rows.append(f'mic{i:02d}\t{px}\t{py}\t{rng.rand():.4f}')
    with open(os.path.join(d, 'picks.txt'), 'w') as f:
        f.write('\n'.join(rows) + '\n')


class Counters:
    """bytes handed to the ring's device -> host calls, on either version of the package"""

    def __init__(self):
        from topaz_amd import runtime as rt
        self.lock, self.bytes, self.saved = threading.Lock(), 0, []
        download = rt.Stage.download

        def counted(stage, slot, src):
            with self.lock:
                self.bytes += src.numel() * src.element_size()
            return download(stage, slot, src)
        self._patch(rt.Stage, 'download', counted)
        if hasattr(rt.Stage, 'download_encoded'):
            encoded = rt.Stage.download_encoded

            def counted_encoded(stage, slot, src, enc, params=None):
                with self.lock:
                    self.bytes += src.numel() * rt.ENC_DTYPES[enc].itemsize + 8      # (and the overflow counter)
                return encoded(stage, slot, src, enc, params)
            self._patch(rt.Stage, 'download_encoded', counted_encoded)

    def _patch(self, owner, attr, fn):
        self.saved.append((owner, attr, getattr(owner, attr)))
        setattr(owner, attr, fn)

    def restore(self):
        for owner, attr, fn in self.saved:
            setattr(owner, attr, fn)


def _tree_bytes(path):
    if os.path.isfile(path):
        return os.path.getsize(path)
    return sum(os.path.getsize(os.path.join(r, f)) for r, _, fs in os.walk(path) for f in fs if f.endswith(('.mrc', '.mrcs')))


def leg(a):
    """the measurements of one tree, as one JSON line on stdout"""
    sys.path.insert(0, os.path.abspath(a.tree))
    import topaz_amd
    from topaz_amd.main import main as topaz
    d = a.data
    mics = sorted(os.path.join(d, 'mics', f) for f in os.listdir(os.path.join(d, 'mics')))
    n = len(mics)
    tag = os.path.basename(os.path.abspath(a.tree))
    out = {'package': os.path.dirname(topaz_amd.__file__), 'legs': {}}
    has_flag = os.path.exists(os.path.join(os.path.dirname(topaz_amd.__file__), 'commands', '_spec.py')) and \
        '--float16' in open(os.path.join(os.path.dirname(topaz_amd.__file__), 'commands', '_spec.py')).read()
    with open(os.devnull, 'w') as null:
        stderr, sys.stderr = sys.stderr, null                         # (the commands' progress lines)
        try:
            for command in COMMANDS:
                for flag in ([], ['--float16']) if has_flag and not a.float32_only else ([],):
                    target = os.path.join(d, f'out_{tag}_{command.split()[0]}_{"f16" if flag else "f32"}')

                    def run():
                        np.random.seed(7)
                        if command.startswith('denoise'):
                            topaz(['denoise', '-m', 'unet-v0.2.1', '-o', target] + flag + mics)
                        elif command.startswith('preprocess'):
                            topaz(['preprocess', '-s', '4', '-o', target] + flag + mics)
                        else:
                            topaz(['particle_stack', os.path.join(d, 'picks.txt'), '--image-root', os.path.join(d, 'mics'),
                                   '--size', '256', '-o', target + '.mrcs'] + flag)

                    run()                                              # warm-up (the model, operators, pinned rings)
                    ts = []
                    for _ in range(a.runs):
                        t0 = time.perf_counter()
                        run()
                        ts.append(time.perf_counter() - t0)
                    counters = Counters()
                    try:
                        run()
                    finally:
                        counters.restore()
                    written = _tree_bytes(target) if os.path.isdir(target) else _tree_bytes(target + '.mrcs')
                    out['legs'][command + (' --float16' if flag else '')] = {
                        'ms': [1e3 * t / n for t in ts], 'd2h_bytes': counters.bytes / n, 'written_bytes': written / n}
                    shutil.rmtree(target, ignore_errors=True)
                    for ext in ('.mrcs', '.star'):
                        if os.path.exists(target + ext):
                            os.unlink(target + ext)
        finally:
            sys.stderr = stderr
    print('RESULT ' + json.dumps(out))


def _stat(v):
    return f'{np.median(v):8.2f} ({min(v):.2f} .. {max(v):.2f})'


def report(results, a):
    lines = [f'# {a.mics} synthetic {a.size}^2 float32 micrographs (Poisson 1000 with darker discs) on tmpfs, {PICKS} picks each; 1 '
             f'warm-up + {a.runs} timed runs, wall ms per micrograph: median (min .. max)',
             '# D2H: bytes per micrograph handed to the result ring\'s device -> host calls; written: bytes of the MRC files per micrograph']
    for tag, r in results:
        lines.append(f'\n== {tag}')
        lines.append(f'{"command":40s} {"ms per micrograph":>28s} {"D2H bytes":>14s} {"written bytes":>14s}')
        for name, t in r['legs'].items():
            lines.append(f'{name:40s} {_stat(t["ms"]):>28s} {t["d2h_bytes"]:14.0f} {t["written_bytes"]:14.0f}')
    new = results[0][1]['legs']
    lines.append('\n== reading: --float16 against the default, this tree (spread: the larger max - min of the two)')
    for command in COMMANDS:
        if command + ' --float16' not in new:
            continue
        x, y = new[command + ' --float16'], new[command]
        spread = max(max(x['ms']) - min(x['ms']), max(y['ms']) - min(y['ms']))
        delta = float(np.median(x['ms']) - np.median(y['ms']))
        verdict = 'faster' if delta < -spread else 'slower' if delta > spread else 'inside the spread'
        lines.append(f'{command:28s} {np.median(x["ms"]):8.2f} vs {np.median(y["ms"]):8.2f} ms ({delta:+.2f} ms; spread {spread:.2f} ms): '
                     f'{verdict}; D2H x{x["d2h_bytes"] / max(y["d2h_bytes"], 1):.3f}, written x{x["written_bytes"] / y["written_bytes"]:.3f}')
    if len(results) == 2:
        old = results[1][1]['legs']
        lines.append('\n== verdict: the default float32 path, this tree against the parent (no slower = not above the parent by more than the '
                     'spread)')
        for command in COMMANDS:
            x, y = new[command]['ms'], old[command]['ms']
            spread = max(max(x) - min(x), max(y) - min(y))
            delta = float(np.median(x) - np.median(y))
            verdict = 'SLOWER' if delta > spread else 'no slower'
            lines.append(f'{command:28s} {np.median(x):8.2f} vs {np.median(y):8.2f} ms ({delta:+.2f} ms; spread {spread:.2f} ms): {verdict}')
    return '\n'.join(lines) + '\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mics', type=int, default=8)
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--tmp', default='/dev/shm' if os.path.isdir('/dev/shm') else None)
    ap.add_argument('--tree', default=ROOT, help='checkout whose topaz_amd package is measured (default: this one)')
    ap.add_argument('--parent', default=None, help='a built checkout of the parent commit, measured on the same files')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'float16_output.txt'))
    ap.add_argument('--leg', action='store_true', help=argparse.SUPPRESS)      # a child: one tree, JSON on stdout
    ap.add_argument('--float32-only', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--data', default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    d = tempfile.mkdtemp(prefix='float16_output_', dir=a.tmp)
    try:
        make_inputs(d, a.mics, a.size)
        results = []
        for tag, tree in [('this tree', a.tree)] + ([('parent', a.parent)] if a.parent else []):
            # one fresh process per tree: two versions of the package (and of the library) never share a process
            cmd = [sys.executable, os.path.abspath(__file__), '--leg', '--tree', tree, '--data', d, '--runs', str(a.runs)]
            r = subprocess.run(cmd + (['--float32-only'] if tag == 'parent' else []), capture_output=True, text=True)
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
