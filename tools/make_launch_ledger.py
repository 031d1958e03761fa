"""Record the launch ledger of a PARENT revision: tests/golden/launch_ledger_parent.json.

Test infrastructure, run by hand on the MI355X before a change to the layer executor (csrc/rt_exec.hip and the drivers around it)
is made; no test runs it.  Recipe:

    PYTHONDONTWRITEBYTECODE=1 python tools/make_launch_ledger.py --parent REV [--build-only]

The sources of revision REV (git archive of topaz_amd/ and include/) are unpacked and built under tools/_run/launch_ledger_parent/
-- `--build-only` stops there, so a machine without a GPU can prepare the tree -- and a child process that imports THAT build
replays the legs of LEGS below.  Where there is no git history beside the tool, a tree prepared earlier is used as it is.

Per run of a leg, with prof_enable(1) and after prof_reset(), the ledger holds
  digest    sha256 of the output array's bytes
  shape     its shape
  launches  the ctx.launches() delta
  classes   prof_get(c)'s launch count and FLOP for c in 0..3
  kernels   the rows of prof_kernels_bytes() as [name, launches, FLOP, bytes], sorted by name (milliseconds left out)
  stats     the deltas of split_stats()'s (finished on the 2xf16 path, re-run on the fp32 kernels) where the run is a scoring pass
Everything is host arithmetic or a bit pattern, so the ledger is deterministic; the tool still runs every leg twice and refuses to
write the file if the two disagree.  tests/test_gpu_launch_ledger.py replays the same legs (record() below) on the code under
test: the bit-identity tests compare windowed against unwindowed runs of one build and cannot see a window that became too large;
the FLOP and bytes of every launch can.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import shutil
import subprocess
import sys

sys.dont_write_bytecode = True
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
if ROOT not in sys.path:
    sys.path.append(ROOT)                 # (behind PYTHONPATH: the child imports the parent's topaz_amd, the rest from here)
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
LEDGER = os.path.join(GOLDEN, 'launch_ledger_parent.json')
TREE = os.path.join(ROOT, 'tools', '_run', 'launch_ledger_parent')


# ---- the legs --------------------------------------------------------------------------------------------------------------
def _image(seed, shape):
    import numpy as np
    return (np.random.RandomState(seed).randn(*shape) * 3 + 1).astype(np.float32)


def _switches(ctx, batch=8, lanes=True, exact=False):
    ctx.set_batch(batch)
    ctx.set_lanes(lanes)
    ctx.set_exact(exact)


def _restore(ctx):
    ctx.set_batch(8)
    ctx.set_lanes(True)
    ctx.set_exact(False)
    ctx.set_range(True)
    ctx.set_tiling(40 << 20, 4096)
    ctx.prof_enable(False)


def _denoise_2d_runs(ctx, d, x, patch, pad, variants):
    for tag, kw in variants:
        def run(kw=kw):
            _switches(ctx, **kw)
            return d.denoise(x, patch, pad)
        yield tag, run, None


def leg_a(ctx):
    """patched 2-D denoise, pretrained unet-small: stem, fused pool, per-parity decoder, stencil last conv; in exact mode the fp32
    per-parity form and the direct kernel.  Patches clipped at all four borders, more patches than one batch of 8."""
    from topaz_amd.denoise import Denoise
    d = Denoise('unet-small')
    x = _image(101, (300, 420))
    variants = [('batched', {}), ('lanes', dict(batch=0)), ('one_stream', dict(batch=0, lanes=False)), ('exact', dict(exact=True))]
    yield from _denoise_2d_runs(ctx, d, x, 96, 64, variants)


def leg_b(ctx):
    """patched 2-D denoise, the 48-filter U-Net with an 11 x 11 base and a 5 x 5 top kernel: the 5 x 5 sub-pixel decoder and the
    96- and 128-channel tiles.  (Its 5 x 5 last conv has 32 input channels, 800 taps, and takes the stencil like leg A's; the
    column-kernel last conv and its shift-sum are leg E.)"""
    from oracle import denoising as oden
    from topaz_amd.denoise import Denoise
    from topaz_amd.denoising.models import DenoiseNet
    d = Denoise(DenoiseNet('unet', oden.synthetic_unet_sd(11, nf=48, base_width=11, top_width=5)))
    x = _image(102, (260, 300))
    yield from _denoise_2d_runs(ctx, d, x, 128, 60, [('default', {}), ('exact', dict(exact=True))])


def leg_c(ctx):
    """tiled 3-D denoise: z windows in both argument structs, the z-pair pool branch"""
    import numpy as np
    import torch
    from topaz_amd.denoise import Denoise3D
    from topaz_amd.denoising.models import DenoiseNet
    z = np.load(os.path.join(GOLDEN, 'denoise3d_unet3d_nf8.npz'), allow_pickle=False)
    d = Denoise3D(DenoiseNet('unet-3d', {k[3:]: z[k] for k in z.files if k.startswith('sd:')}))
    dm = d.model.device_model
    t = torch.from_numpy(z['tomo']).cuda()
    for tag, kw in (('default', {}), ('exact', dict(exact=True))):
        def run(kw=kw):
            _switches(ctx, **kw)
            return dm.denoise_3d(t, 32, 16).cpu().numpy()
        yield tag, run, None


FOLD_MODEL = 'resnet16_u32'       # a pretrained detector whose load folds a 1 x 1 projection (record() checks that it does)


def leg_d(ctx):
    """scoring: the weights-resident kernel, a folded 1 x 1 projection, the padded pool branch in 2-D and 3-D, run_image's tiles,
    and an overflow of the 2xf16 pass that is re-run on the fp32 kernels"""
    import numpy as np
    import torch
    from topaz_amd.model.factory import load_model

    def load(name):
        m = load_model(name if '.' not in name else os.path.join(GOLDEN, name))
        m.eval()
        m.fill()
        m.cuda()
        return m

    def score(m, x, exact=False):
        def run():
            _switches(ctx, exact=exact)
            with torch.no_grad():
                return m(torch.from_numpy(x)[None, None].cuda())[0, 0].cpu().numpy()
        return run
    r8, fold = load('resnet8_u32'), load(FOLD_MODEL)
    rs = np.random.RandomState(103)
    yield 'resnet8_u32', score(r8, rs.randn(200, 260).astype(np.float32)), r8.device_model
    xf = rs.randn(200, 260).astype(np.float32)
    yield 'folded_projection', score(fold, xf), fold.device_model
    yield 'conv31_max_2d', score(load('user_model_conv31_max_bn_u16.sav'), rs.randn(70, 90).astype(np.float32)), None
    yield 'conv31_max_3d', score(load('user_model_conv31_3d_max_bn_u8.sav'), rs.randn(20, 22, 27).astype(np.float32)), None
    xt = rs.randn(150, 170).astype(np.float32)

    def tiled():
        ctx.set_tiling(10000, 64)
        try:
            return score(r8, xt)()
        finally:
            ctx.set_tiling(40 << 20, 4096)
    yield 'tiled', tiled, r8.device_model
    xo = (rs.randn(200, 260) * 1e6).astype(np.float32)

    def overflow():
        ctx.set_range(False)
        try:
            return score(r8, xo)()
        finally:
            ctx.set_range(True)
    yield 'overflow_rerun', overflow, r8.device_model
    # (not part of the ledger: on the fp32 kernels nothing is folded, so every conv layer of FOLD_MODEL launches once)
    yield '_unfolded', score(fold, xf, exact=True), None


def leg_e(ctx):
    """patched 2-D denoise, pretrained fcnn: its 64 -> 1 channel 11 x 11 last conv is too large for the stencil (which the last
    convs of legs A - C take), so it runs as the column kernel over 2 * pad extra columns followed by the shift-sum"""
    from topaz_amd.denoise import Denoise
    d = Denoise('fcnn')
    x = _image(104, (300, 420))
    yield from _denoise_2d_runs(ctx, d, x, 96, 64, [('default', {}), ('exact', dict(exact=True))])


LEGS = {'A': leg_a, 'B': leg_b, 'C': leg_c, 'D': leg_d, 'E': leg_e}
RUNS = {'A': ['batched', 'lanes', 'one_stream', 'exact'], 'B': ['default', 'exact'], 'C': ['default', 'exact'],
        'D': ['resnet8_u32', 'folded_projection', 'conv31_max_2d', 'conv31_max_3d', 'tiled', 'overflow_rerun'],
        'E': ['default', 'exact']}


def _measure(ctx, run, dm):
    import numpy as np
    ctx.prof_enable(1)
    ctx.prof_reset()
    n0 = ctx.launches()
    before = dm.split_stats() if dm is not None else None
    y = run()
    row = {'digest': hashlib.sha256(np.ascontiguousarray(y).tobytes()).hexdigest(), 'shape': list(y.shape),
           'launches': ctx.launches() - n0,
           'classes': [list(ctx.prof_get(c)[1:]) for c in range(4)],
           'kernels': sorted([k[0], k[2], k[3], k[4]] for k in ctx.prof_kernels_bytes())}
    if dm is not None:
        after = dm.split_stats()
        row['stats'] = [after[1] - before[1], after[2] - before[2]]
    return row


def record(ctx, legs=None):
    """{leg: {run: row}} of the code that is imported; every switch is pinned first and restored afterwards"""
    out = {}
    try:
        for leg in legs or sorted(LEGS):
            out[leg] = {}
            for tag, run, dm in LEGS[leg](ctx):
                run()                   # (first use: anything issued once per model stays out of the counts)
                out[leg][tag] = _measure(ctx, run, dm)
            assert [t for t in out[leg] if t[0] != '_'] == RUNS[leg], (leg, list(out[leg]))
    finally:
        _restore(ctx)
    if 'E' in out:
        assert any(k[0].startswith('shiftsum') for k in out['E']['default']['kernels']), 'the fcnn leg must take the shift-sum'
    if 'D' in out:
        d = out['D']
        assert d['overflow_rerun']['stats'] == [0, 1], 'the scaled image must be re-run on the fp32 kernels: %r' % d['overflow_rerun']
        assert d['resnet8_u32']['stats'] == [1, 0]
        assert any('weights resident' in k[0] for k in d['resnet8_u32']['kernels'])
        convs = lambda row: row['classes'][0][0] + row['classes'][1][0]          # (classes 0 and 1: the convolutions)
        assert convs(d['folded_projection']) < convs(d.pop('_unfolded')), f'{FOLD_MODEL} folds no projection'
    return out


# ---- the parent's tree -----------------------------------------------------------------------------------------------------
def prepare(rev):
    """unpack and build revision `rev` under TREE; returns the full revision"""
    have_git = subprocess.run(['git', '-C', ROOT, 'rev-parse', '--git-dir'], capture_output=True).returncode == 0
    mark = os.path.join(TREE, 'REVISION')
    if not have_git:
        if not os.path.exists(mark):
            raise SystemExit(f'no git history here and no prepared tree under {TREE}: run with --build-only where there is one')
        return open(mark).read().strip()
    full = subprocess.run(['git', '-C', ROOT, 'rev-parse', rev], check=True, capture_output=True, text=True).stdout.strip()
    if not (os.path.exists(mark) and open(mark).read().strip() == full):
        shutil.rmtree(TREE, ignore_errors=True)
        os.makedirs(TREE)
        tar = subprocess.run(['git', '-C', ROOT, 'archive', full, 'topaz_amd', 'include'], check=True, capture_output=True).stdout
        subprocess.run(['tar', '-x', '-C', TREE], input=tar, check=True)
    env = dict(os.environ, PYTHONPATH=TREE, PYTHONDONTWRITEBYTECODE='1')
    subprocess.run([sys.executable, '-m', 'topaz_amd.build'], env=env, cwd=TREE, check=True)
    with open(mark, 'w') as f:
        f.write(full + '\n')
    return full


def _child(path):
    import topaz_amd
    assert os.path.dirname(os.path.abspath(topaz_amd.__file__)).startswith(TREE), topaz_amd.__file__
    from topaz_amd.runtime import get_context
    ctx = get_context(0)
    first, second = record(ctx), record(ctx)
    if first != second:
        for leg in first:
            for tag in first[leg]:
                if first[leg][tag] != second[leg][tag]:
                    print(f'leg {leg} run {tag} differs between two runs:\n  {first[leg][tag]}\n  {second[leg][tag]}', file=sys.stderr)
        raise SystemExit('the ledger is not deterministic: nothing written')
    with open(path, 'w') as f:
        json.dump(first, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default='HEAD', help='revision whose build the ledger is recorded from')
    ap.add_argument('--build-only', action='store_true', help='unpack and build the revision, record nothing (needs no GPU)')
    ap.add_argument('--child', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return _child(a.child)
    full = prepare(a.parent)
    if a.build_only:
        print(f'{full} built under {TREE}')
        return
    tmp = LEDGER + '.tmp'
    env = dict(os.environ, PYTHONPATH=TREE + os.pathsep + ROOT, PYTHONDONTWRITEBYTECODE='1')
    try:
        subprocess.run([sys.executable, os.path.abspath(__file__), '--child', tmp], env=env, cwd=ROOT, check=True)
        legs = json.load(open(tmp))
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    with open(LEDGER, 'w') as f:
        json.dump({'revision': full, 'fold_model': FOLD_MODEL, 'legs': legs}, f, indent=1, sort_keys=True)
        f.write('\n')
    n = sum(len(v) for v in legs.values())
    print(f'{LEDGER}: {n} runs of {len(legs)} legs at {full}, {os.path.getsize(LEDGER) / 1024:.0f} KiB')


if __name__ == '__main__':
    main()
