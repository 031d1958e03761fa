"""`topaz particle_stack` (topaz/utils/picks.py:71-197 create_particle_stack): one standardised box per pick, written as an MRC
stack with a RELION STAR file next to it.

The work is split in two.  plan_particle_stack reads the pick table, the micrograph headers and the optional metadata STAR on
the host and fixes everything that does not depend on pixel values -- the particle order, the stack header and the STAR text --
and refuses bad input before a byte is written.  write_particle_stack then streams the micrographs through the MI355X
(extract.ImageFeed: micrograph i+1 is decoded and uploaded while micrograph i is cropped), cuts the boxes in chunks that fit a
device byte budget (tpz_particle_stack: one launch per chunk, four with --resize) and hands each chunk through a pinned staging
slot to a writer thread, so the stack is written once, in order, and never held whole on the host.

Divergences from the reference, all deliberate:
  - --resize: the reference hands the 3-D (mz, S, S) box to its 2-D `downsample`, whose concatenation then joins frames instead
    of frequency rows (an even resize writes 2*mz frames per particle under a header that declares mz, an odd one raises).
    Here every frame goes through the 2-D truncated DFT of utils/image.py and the particle is standardised again.
  - a box that misses the image on the high side is all zeros wherever it lies (the reference raises for W < left < W + size).
  - explicit errors where the reference crashes obscurely: no --size, no particle left after thresholding, a missing micrograph,
    a micrograph that is not float32 (MRC mode 2: out of scope), a box wholly outside the low edge, resize > size.
  - without --image-root the names are resolved against the working directory.
"""
from __future__ import annotations

import io
import os
import sys
from typing import List, NamedTuple, Optional

import numpy as np
import pandas as pd

from .. import mrc
from .files import read_star, write_star

DEFAULT_BUDGET = 256 << 20      # device bytes of one chunk of particles (output plus the resize intermediates)


class Micrograph(NamedTuple):
    label: str                  # the table's image name
    name: str                   # MicrographName: label + image_ext
    path: str
    xy: np.ndarray              # [n, 2] int32 (x, y), in file order
    shape: tuple                # (H, W) or (mz, H, W), as ImageFeed yields it


class Plan(NamedTuple):
    output: str
    star_path: str
    size: int
    resize: int
    mz: int
    n: int
    micrographs: List[Micrograph]
    header: bytes               # the 1024-byte MRC header of the stack
    star: str                   # the STAR file's text


def _header_of(path: str):
    with open(path, 'rb') as f:
        return mrc.parse_header(f.read(1024))


def plan_particle_stack(input_file: str, output_file: str, threshold: float, size: Optional[int], resize: int,
                        image_root: Optional[str], image_ext: str, metadata_file: Optional[str], log=sys.stderr) -> Plan:
    """everything of create_particle_stack but the pixels; raises ValueError / FileNotFoundError on bad input"""
    if size is None:
        raise ValueError('particle_stack: --size is required')
    if size < 1:
        raise ValueError(f'particle_stack: --size must be positive, got {size}')
    if not output_file:
        raise ValueError('particle_stack: -o/--output is required')
    particles = pd.read_csv(input_file, sep='\t')
    print('#', 'Loaded', len(particles), 'particles', file=log)
    if 'score' in particles:
        particles = particles.loc[particles['score'] >= threshold]
        print('#', 'Thresholding at', threshold, file=log)
    print('#', 'Extracting', len(particles), 'particles', file=log)
    N = len(particles)
    if N == 0:
        raise ValueError('particle_stack: no particles left to extract' + (f' at threshold {threshold}' if 'score' in particles else ''))
    if resize < 0:
        resize = size
    if resize == 0 or resize > size:
        raise ValueError(f'particle_stack: --resize must lie in 1..{size} (only downsampling), got {resize}')
    for col in ('x_coord', 'y_coord'):
        if not np.issubdtype(particles[col].dtype, np.integer):
            raise ValueError(f'particle_stack: {col} must hold integer pixel coordinates')

    micrographs, names, xs, ys, scores = [], [], [], [], []
    mz = cella = cellb = None
    for image_name, coords in particles.groupby('image_name'):
        name = str(image_name) + image_ext
        path = os.path.join(image_root or '', name)
        if not os.path.isfile(path):
            raise FileNotFoundError(f'particle_stack: micrograph {path} not found')
        h = _header_of(path)
        if h.mode != 2:
            raise ValueError(f'particle_stack: {path} has MRC mode {h.mode}; only float32 micrographs (mode 2) are supported')
        z = h.nz
        if mz is None:
            mz = z
            cella, cellb = (h.xlen, h.ylen, h.zlen), (h.alpha, h.beta, h.gamma)
        elif z != mz:
            raise ValueError(f'particle_stack: {path} has {z} frames, the first micrograph {mz}')
        x = coords['x_coord'].values
        y = coords['y_coord'].values
        bad = np.flatnonzero((x - size // 2 + size < 0) | (y - size // 2 + size < 0))
        if bad.size:
            j = int(bad[0])
            raise ValueError(f'particle_stack: pick ({x[j]}, {y[j]}) of {name}: its {size}-pixel box lies wholly outside the '
                             'low edge of the micrograph')
        micrographs.append(Micrograph(str(image_name), name, path, np.stack([x, y], 1).astype(np.int32),
                                      (h.ny, h.nx) if z == 1 else (z, h.ny, h.nx)))
        names += [name] * len(coords)
        xs.append(x)
        ys.append(y)
        if 'score' in coords:
            scores.append(coords['score'].values)

    header = mrc.header_struct.pack(*list(mrc.make_header((N * mz, resize, resize), cella, cellb, mz=mz, dtype=np.float32)))

    stack_name = os.path.basename(output_file)
    star_path = os.path.splitext(output_file)[0] + '.star'
    table = {'MicrographName': names, 'CoordinateX': np.concatenate(xs), 'CoordinateY': np.concatenate(ys)}
    if 'score' in particles:
        table['AutopickFigureOfMerit'] = np.concatenate(scores)
    metadata = pd.DataFrame(table)
    metadata['ImageName'] = [str(i + 1) + '@' + stack_name for i in range(len(metadata))]
    if mz > 1:
        metadata['NrOfFrames'] = mz
    if metadata_file is not None:
        with open(metadata_file, 'r') as f:
            metadata = pd.merge(metadata, read_star(f), on='MicrographName', how='left')
    if resize != size and 'DetectorPixelSize' in metadata:
        metadata['DetectorPixelSize'] = metadata['DetectorPixelSize'].values.astype(float) * (size / resize)
    buf = io.StringIO()
    write_star(metadata, buf)
    return Plan(output_file, star_path, size, resize, mz, N, micrographs, header, buf.getvalue())


def resize_operators(size: int, resize: int) -> np.ndarray:
    """the fp32 operators tpz_particle_stack resizes a size^2 frame with: [2][size][resize] column operators [R1, R2] followed by
    the [resize][2 size] row operator [Re Lc | Im Lc], rearranged from utils/image._downsample_operators (numpy's own FFT applied
    to identity matrices in float64: y = Re(Lc x) R1 + Im(Lc x) R2)"""
    from .image import _downsample_operators
    S, R = size, resize
    L, Rm = _downsample_operators(S, S, R, R)            # L: [Re Lc; Im Lc] (2R x S), Rm: [R1; R2]^T (R x 2S)
    cols = np.stack([Rm[:, :S].T, Rm[:, S:].T])          # 2 x S x R
    rows = np.concatenate([L[:R], L[R:]], axis=1)        # R x 2S
    return np.ascontiguousarray(np.concatenate([cols.ravel(), rows.ravel()]).astype(np.float32))


def write_particle_stack(plan: Plan, device: int = 0, budget_bytes: int = DEFAULT_BUDGET, log=sys.stderr) -> None:
    """cut, standardise (and resize) the planned particles on the MI355X and write the stack and the STAR file"""
    import queue
    import threading

    import torch

    from .. import runtime as rt
    from ..extract import ImageFeed
    torch.cuda.set_device(device)
    ctx = rt.get_context(device)
    S, R, mz = plan.size, plan.resize, plan.mz
    ops = resize_operators(S, R) if R != S else None
    out_bytes = 4 * mz * R * R
    dev_bytes = out_bytes + (4 * mz * (S * S + 2 * S * R) if R != S else 0)
    per_chunk = max(1, min(int(budget_bytes) // dev_bytes, max(len(m.xy) for m in plan.micrographs)))
    DEPTH = 2
    stage = rt.Stage(ctx, per_chunk * out_bytes, DEPTH)
    free_slots: 'queue.Queue' = queue.Queue()
    for k in range(DEPTH):
        free_slots.put(k)
    todo: 'queue.Queue' = queue.Queue()
    failed: list = []

    with open(plan.output, 'wb') as f:
        f.write(plan.header)

        def writer():
            while True:
                item = todo.get()
                if item is None:
                    return
                k, n_floats, _device_chunk = item               # (the tensor lives until its copy has landed)
                try:
                    if not failed:
                        stage.wait(k)
                        f.write(memoryview(stage.host_array(k, (n_floats,))).cast('B'))
                except BaseException as e:                      # surfaces in the main thread
                    failed.append(e)
                finally:
                    free_slots.put(k)

        th = threading.Thread(target=writer, daemon=True)
        th.start()
        try:
            for m, (path, img) in zip(plan.micrographs, ImageFeed([m.path for m in plan.micrographs], ctx)):
                if tuple(img.shape) != tuple(m.shape):
                    raise ValueError(f'particle_stack: {path} holds {tuple(img.shape)} pixels, its header says {m.shape}')
                print('#', m.label, len(m.xy), 'particles', file=log)
                for c0 in range(0, len(m.xy), per_chunk):
                    xy = m.xy[c0:c0 + per_chunk]
                    out = rt.particle_stack(img, xy, S, R, ops, ctx=ctx)
                    k = free_slots.get()
                    if failed:
                        raise failed[0]
                    stage.download(k, out)
                    todo.put((k, out.numel(), out))
        finally:
            todo.put(None)
            th.join()
            stage.close()
        if failed:
            raise failed[0]
    with open(plan.star_path, 'w') as f:
        f.write(plan.star)


def create_particle_stack(input_file: str, output_file: str, threshold: float, size: Optional[int], resize: int,
                          image_root: Optional[str], image_ext: str, metadata_file: Optional[str], device: int = 0,
                          budget_bytes: int = DEFAULT_BUDGET) -> Plan:
    """topaz/utils/picks.py:71-197 on the MI355X; budget_bytes: device bytes of one chunk of particles"""
    plan = plan_particle_stack(input_file, output_file, threshold, size, resize, image_root, image_ext, metadata_file)
    write_particle_stack(plan, device=device, budget_bytes=budget_bytes)
    return plan
