"""Measure the precision check on one MI355X (the table of profiles/precision_check.txt and DESIGN.md section 11).

    python tools/precision_table.py [--out profiles/precision_check.txt] [--limit 300]

Calibrates a fixed set of models on the default tile (RandomState(0).randn, 256 x 256 or 48^3) at the default bar, measuring only
(bar = 0 in the call, the verdict against runtime.DEFAULT_BAR taken here), and records per model max_abs_delta, max_abs_ref,
rms_delta and the wall time of the calibrate call (a second call: the first one also builds the K-loop schedules of the model's
layers, which any first forward pays).  The models: every packaged detector and denoiser, the benchmark's seeded networks
(tools/synth_weights.py), a seeded conv127 with 32 units and a seeded 3-D resnet8 with 32 units.

Every model is measured in a child process of its own under a time limit of --limit seconds; the run stops at the first child
that fails or runs out of time and writes what it has.  This process never opens the GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MODELS = ['resnet8_u32', 'resnet16_u32', 'unet-v0.2.1', 'unet-small', 'fcnn', 'affine', 'resnet8-u64 seed 7',
          'resnet16-u64 seed 7', 'unet nf48 seed 11', 'unet-3d nf48 seed 13', 'conv127-u32 seed 7', 'resnet8-3d-u32 seed 3']


def load(name):
    """the loaded model (filled where it is a classifier) named by a row of MODELS"""
    from tools import synth_weights as sw
    from topaz_amd.denoising.models import DenoiseNet, load_model as load_denoiser
    from topaz_amd.model.classifier import LinearClassifier
    from topaz_amd.model.factory import load_model as load_detector

    def filled(m):
        m.eval(); m.fill(); m.cuda()
        return m

    if name in ('resnet8_u32', 'resnet16_u32'):
        return filled(load_detector(name))
    if name in ('unet-v0.2.1', 'unet-small', 'fcnn', 'affine'):
        return load_denoiser(name).cuda()
    if name == 'resnet8-u64 seed 7':
        return sw.hip_resnet('resnet8', 64, seed=7)[0]
    if name == 'resnet16-u64 seed 7':
        return sw.hip_resnet('resnet16', 64, seed=7)[0]
    if name == 'unet nf48 seed 11':
        return DenoiseNet('unet', sw.unet_sd(11, nf=48, base_width=11, top_width=5)).cuda()
    if name == 'unet-3d nf48 seed 13':
        return DenoiseNet('unet-3d', sw.unet_sd(13, nf=48, base_width=7, top_width=3, dims=3)).cuda()
    if name == 'conv127-u32 seed 7':
        return filled(LinearClassifier('conv127', sw.basic_sd((7, 5, 5, 5, 5), 32, 7)))
    if name == 'resnet8-3d-u32 seed 3':
        return filled(LinearClassifier('resnet8', sw.calibrate_head(sw.resnet_sd_uncalibrated('resnet8', 32, 3, dims=3), (1.0, 0.0))))
    raise ValueError(name)


def measure(name) -> dict:
    import torch
    model = load(name)
    r = model.calibrate(bar=0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    again = model.calibrate(bar=0)
    torch.cuda.synchronize()
    r['wall_ms'] = (time.perf_counter() - t0) * 1e3
    r['repeatable'] = all(again[k] == r[k] for k in ('max_abs_delta', 'max_abs_ref', 'argmax', 'sum_sq'))
    r['dims'] = model.dims
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'precision_check.txt'))
    ap.add_argument('--limit', type=int, default=300, help='seconds a model may take (load + two calibrations)')
    ap.add_argument('--one', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        print('RESULT ' + json.dumps(measure(args.one)))
        return 0
    from topaz_amd.runtime import DEFAULT_BAR
    lines = ['precision check: 2xf16 against fp32 of the same loaded model, default tile (RandomState(0).randn; 256 x 256, 3-D: 48^3),',
             f'bar {DEFAULT_BAR:.1e} absolute (tools/precision_table.py; wall = the second calibrate call of the process)', '',
             f'{"model":<24}{"tile":<10}{"max_abs_delta":>14}{"max_abs_ref":>13}{"rms_delta":>12}{"wall ms":>10}  verdict']
    rc = 0
    for name in MODELS:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--one', name], capture_output=True, text=True,
                               timeout=args.limit, cwd=ROOT)
        except subprocess.TimeoutExpired:
            lines.append(f'{name:<24}STOPPED: no result within {args.limit} s; the models after it were not measured')
            rc = 1
            break
        got = [line for line in p.stdout.split('\n') if line.startswith('RESULT ')]
        if p.returncode != 0 or not got:
            lines.append(f'{name:<24}STOPPED: exit status {p.returncode}; the models after it were not measured')
            sys.stderr.write(p.stderr[-4000:])
            rc = 1
            break
        r = json.loads(got[-1][len('RESULT '):])
        tile = '48^3' if r['dims'] == 3 else '256^2'
        if not r['eligible']:
            verdict = 'no 2xf16 path (fp32 kernels): nothing to compare'
        elif r['overflow']:
            verdict = 'tile left the f16 range: no comparison'
        else:
            verdict = ('TRIPS' if not r['max_abs_delta'] <= DEFAULT_BAR else 'passes') + ('' if r['repeatable'] else ', NOT repeatable')
        lines.append(f'{name:<24}{tile:<10}{r["max_abs_delta"]:>14.3e}{r["max_abs_ref"]:>13.3e}{r["rms_delta"]:>12.3e}'
                     f'{r["wall_ms"]:>10.2f}  {verdict}')
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return rc


if __name__ == '__main__':
    sys.exit(main())
