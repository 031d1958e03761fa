"""Device time of the padded pool kernels (csrc/pool_pad.hip) at 32 channels x 4096 x 4096, fp32 planes and split cells.

    python tools/bench_pool_pad.py [--reps 20]                      host view: HIP events around tpz_pool on fp32 planes
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_pool_pad.py --reps 20      kernel times, all four kernels

tpz_pool on split cells runs three kernels (fp32 -> cells, the pool, cells -> fp32), so the split-cell pools are timed from the
kernel trace only.  The algorithmic bytes of one launch -- the input read once, the output written once -- are printed per case:
bytes / kernel time against the 8 TB/s of HBM3E is the figure profiles/pooled_basicconv.txt records.
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import torch  # noqa: E402

CASES = [('max', 1), ('max', 8), ('avg', 1)]         # (op, dilation): a max at dilation d writes 2 (d - 1) fewer rows and columns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--channels', type=int, default=32)
    ap.add_argument('--size', type=int, default=4096)
    a = ap.parse_args()
    from topaz_amd import runtime as rt
    ctx = rt.get_context(0)
    C, n = a.channels, a.size
    x = torch.randn((C, n, n), dtype=torch.float32, device=ctx.torch_device())
    for op, d in CASES:
        no = n + 2 - 2 * d
        nbytes = 4.0 * C * (n * n + no * no)          # split cells: 2 + 2 bytes per element, C a multiple of 8 -- the same
        for split in (False, True):
            for _ in range(3):
                rt.pool(x, op, dil=d, pad=1, split=split, ctx=ctx)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                rt.pool(x, op, dil=d, pad=1, split=split, ctx=ctx)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / a.reps
            what = 'call incl. both format conversions' if split else 'call (one kernel + synchronise)'
            print(f'{op} d={d} {"split cells" if split else "fp32 planes"} {C}x{n}x{n} -> {no}x{no}: {nbytes / 1e9:.3f} GB algorithmic, '
                  f'{ms:.3f} ms per {what}' + ('' if split else f' = {nbytes / ms / 1e9:.2f} TB/s'))


if __name__ == '__main__':
    main()
