"""`topaz particle_stack` (topaz/utils/picks.py:71-197 create_particle_stack): one standardised box per pick, written as an MRC
stack with a RELION STAR file next to it.

The work is split in two.  plan_particle_stack reads the pick table, the micrograph headers and the optional metadata STAR on
the host and fixes everything that does not depend on pixel values -- the particle order, the stack header and the STAR text --
and refuses bad input before a byte is written.  write_particle_stack then streams the micrographs through the MI355X
(streaming.ImageFeed: micrograph i+1 is decoded and uploaded while micrograph i is cropped), cuts the boxes in chunks that fit a
device byte budget (tpz_particle_stack: one launch per chunk, four with --resize) and hands each chunk through a pinned staging
slot to a writer thread (streaming.ResultRing), so the stack is written once and never held whole on the host.

Both halves are shared with `topaz extract --particle-stack` (ExtractStack), which cuts the boxes of a micrograph while it is
resident for picking: plan_from_records builds the header and the STAR text from picks held in memory, StackWriter is the
streaming half.  A chunk goes to the byte its first particle's index fixes (os.pwrite) and the header is written last, so the
ranks of `--gpus N` write one file -- each its share of the plan's micrographs here, each its share of the input list there --
and a stack whose length is only known after the last micrograph needs no second pass.  Output is byte-identical to one process.

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
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import pandas as pd

from .. import mrc
from .. import streaming
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
    float16: bool = False       # the stack stores float16 (MRC mode 12) instead of float32


class Record(NamedTuple):
    """the kept picks of one micrograph, in memory: what the stack header and the STAR text are built from"""
    name: str                   # MicrographName
    xy: np.ndarray              # [n, 2] integer (x, y), in table order
    scores: Optional[np.ndarray]  # float64 [n], or None for a table without a score column


def _header_of(path: str):
    with open(path, 'rb') as f:
        return mrc.parse_header(f.read(1024))


def check_boxes(name: str, xy: np.ndarray, size: int) -> None:
    """a box wholly outside the low edge of the micrograph has no crop (the reference crashes there): ValueError"""
    x, y = xy[:, 0], xy[:, 1]
    bad = np.flatnonzero((x - size // 2 + size < 0) | (y - size // 2 + size < 0))
    if bad.size:
        j = int(bad[0])
        raise ValueError(f'particle_stack: pick ({x[j]}, {y[j]}) of {name}: its {size}-pixel box lies wholly outside the '
                         'low edge of the micrograph')


def particle_bytes(mz: int, resize: int, float16: bool = False) -> int:
    """bytes of one particle in the stack: mz frames of resize^2 pixels, 4 bytes each, or 2 under --float16"""
    return (2 if float16 else 4) * mz * resize * resize


def particle_byte_offset(index: int, out_bytes: int) -> int:
    """byte of particle `index` in the stack file: behind the 1024-byte header (the stack has no extended header)"""
    return 1024 + out_bytes * int(index)


def plan_from_records(records: Sequence[Record], output_file: str, size: int, resize: int, mz: int, cella, cellb,
                      metadata_file: Optional[str], float16: bool = False):
    """(stack header bytes, STAR path, STAR text) of the particles in `records`, in that order -- the half of the planner that
    does not care where the picks came from: `particle_stack` reads them from a table, `extract --particle-stack` has them in
    memory.  resize: the written box size (== size when off); cella / cellb: of the first micrograph's header; float16: the
    header says mode 12."""
    N = int(sum(len(r.xy) for r in records))
    header = mrc.header_struct.pack(*list(mrc.make_header((N * mz, resize, resize), cella, cellb, mz=mz,
                                                          dtype=np.float16 if float16 else np.float32)))

    stack_name = os.path.basename(output_file)
    star_path = os.path.splitext(output_file)[0] + '.star'
    names = [r.name for r in records for _ in range(len(r.xy))]
    table = {'MicrographName': names, 'CoordinateX': np.concatenate([np.asarray(r.xy)[:, 0] for r in records]),
             'CoordinateY': np.concatenate([np.asarray(r.xy)[:, 1] for r in records])}
    if records[0].scores is not None:
        table['AutopickFigureOfMerit'] = np.concatenate([np.asarray(r.scores, dtype=np.float64) for r in records])
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
    return header, star_path, buf.getvalue()


def plan_particle_stack(input_file: str, output_file: str, threshold: float, size: Optional[int], resize: int,
                        image_root: Optional[str], image_ext: str, metadata_file: Optional[str], log=None,
                        float16: bool = False) -> Plan:
    """everything of create_particle_stack but the pixels; raises ValueError / FileNotFoundError on bad input.
    log: where the progress lines go (default: sys.stderr as it is at the call, not at import)"""
    log = sys.stderr if log is None else log
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

    micrographs, records = [], []
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
        xy = np.stack([coords['x_coord'].values, coords['y_coord'].values], 1)
        check_boxes(name, xy, size)
        micrographs.append(Micrograph(str(image_name), name, path, xy.astype(np.int32),
                                      (h.ny, h.nx) if z == 1 else (z, h.ny, h.nx)))
        records.append(Record(name, xy, coords['score'].values if 'score' in coords else None))

    header, star_path, star = plan_from_records(records, output_file, size, resize, mz, cella, cellb, metadata_file, float16)
    return Plan(output_file, star_path, size, resize, mz, N, micrographs, header, star, float16)


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


def particle_offset(base: int, counts: Sequence[int], rank: int) -> Tuple[int, int]:
    """One round of a sharded `extract --particle-stack`: the ranks hold the micrographs round * world + r and `counts[r]` is the
    number of particles rank r keeps of its one (0: none kept, or no micrograph left in a ragged last round).  Input order is
    rank order within the round, so with `base` particles in the rounds before, rank `rank` writes from particle
    base + sum(counts[:rank]) on.  Returns (that index, the base of the next round)."""
    counts = [int(c) for c in counts]
    return base + sum(counts[:rank]), base + sum(counts)


class StackWriter:
    """The streaming half of a particle stack, shared by `particle_stack` and `extract --particle-stack`.  cut() crops,
    standardises (and resizes) the picks of one resident micrograph in chunks of the device byte budget and hands every chunk
    to a streaming.ResultRing, whose writer thread puts the chunk at the byte the global index of its first particle fixes
    (os.pwrite): the ranks of a sharded job write one file, and a stack whose length is only known after the last micrograph
    gets its header last (seal_particle_stack).  Every rank opens the same file and none truncates it."""

    DEPTH = 2

    def __init__(self, ctx, path: str, size: int, resize: int, mz: int, budget_bytes: int = DEFAULT_BUDGET, capacity: int = 0,
                 placeholder: bool = True, float16: bool = False):
        """capacity: particles per ring slot to start with (it grows to the largest chunk seen); placeholder: write the 1024
        bytes the header will replace (rank 0); float16: a chunk is encoded to float16 on the device on its way to the pinned
        slot (ResultRing.put's `encode`) and a particle takes half the bytes of the file"""
        from .. import runtime as rt
        self.ctx, self.path, self.S, self.R, self.mz = ctx, path, size, resize, mz
        self.ops = resize_operators(size, resize) if resize != size else None
        self.encode = rt.ENC_F16 if float16 else None
        self.out_bytes = particle_bytes(mz, resize, float16)
        # (the chunk size follows the float32 the device holds, whatever the file stores: the same chunks either way)
        dev_bytes = 4 * mz * resize * resize + (4 * mz * (size * size + 2 * size * resize) if resize != size else 0)
        self.per_chunk = max(1, int(budget_bytes) // dev_bytes)
        self.fd = os.open(path, os.O_WRONLY | os.O_CREAT, 0o666)
        if placeholder:
            os.pwrite(self.fd, bytes(1024), 0)
        self.ring = streaming.ResultRing(ctx, lambda chunk, at: streaming.pwrite_all(self.fd, chunk, at), self.DEPTH,
                                         on_overflow=self._overflowed)
        if capacity:
            self.ring.reserve(self._slot_bytes(min(self.per_chunk, capacity)))

    def _slot_bytes(self, particles: int) -> int:
        """ring slot bytes for a chunk of that many particles"""
        from .. import runtime as rt
        pixels = particles * self.mz * self.R * self.R
        return 4 * pixels if self.encode is None else rt.Stage.encode_bytes(self.ctx, self.encode, pixels)

    def _overflowed(self, lost: int, at: int) -> None:
        first = (at - 1024) // self.out_bytes
        streaming.warn_overflow(f'{self.path} (the chunk of particles from {first + 1} on)', lost)

    def check(self) -> None:
        self.ring.check()

    def cut(self, img, xy: np.ndarray, first: int) -> None:
        """the particles at xy ([n, 2] int32) of the resident micrograph img are particles first .. first + n - 1 of the stack"""
        from .. import runtime as rt
        for c0 in range(0, len(xy), self.per_chunk):
            part = xy[c0:c0 + self.per_chunk]
            self.ring.reserve(self._slot_bytes(len(part)))      # (a growth drains the ring: before the launch, not after it)
            out = rt.particle_stack(img, part, self.S, self.R, self.ops, ctx=self.ctx)
            self.ring.put(out, particle_byte_offset(first + c0, self.out_bytes), encode=self.encode)

    def close(self) -> None:
        """wait for the last write, free the ring, close the file (idempotent; a writer failure stays available to check())"""
        if self.fd is None:
            return
        self.ring.close()
        os.close(self.fd)
        self.fd = None


def seal_particle_stack(path: str, header: bytes, n: int, out_bytes: int, star_path: str, star: str) -> None:
    """what rank 0 does last: the header over the placeholder, the file cut to its n particles, the STAR file"""
    fd = os.open(path, os.O_WRONLY)
    try:
        os.pwrite(fd, header, 0)
        os.ftruncate(fd, 1024 + n * out_bytes)
    finally:
        os.close(fd)
    with open(star_path, 'w') as f:
        f.write(star)


def write_particle_stack(plan: Plan, device: int = 0, budget_bytes: int = DEFAULT_BUDGET, log=None,
                         ranks: Tuple[int, int, int] = (0, 0, 1)) -> None:
    """cut, standardise (and resize) the planned particles on the MI355X and write the stack and the STAR file.
    ranks: (rank, local_rank, world) of a sharded job -- this rank takes the plan's micrographs i = rank (mod world); the plan
    holds every count, so each micrograph's place in the file is known up front."""
    import torch

    from .. import parallel
    from .. import runtime as rt
    log = sys.stderr if log is None else log
    rank, local_rank, world = ranks
    torch.cuda.set_device(device)
    ctx = rt.get_context(device)
    firsts = np.concatenate([[0], np.cumsum([len(m.xy) for m in plan.micrographs])])
    mine = parallel.shard_indices(len(plan.micrographs), rank, world)
    mics = [plan.micrographs[i] for i in mine]
    writer = StackWriter(ctx, plan.output, plan.size, plan.resize, plan.mz, budget_bytes,
                         capacity=max([len(m.xy) for m in mics] or [0]), placeholder=(rank == 0), float16=plan.float16)
    try:
        for j, (path, img) in enumerate(streaming.ImageFeed([m.path for m in mics], ctx)):
            m = mics[j]
            if tuple(img.shape) != tuple(m.shape):
                raise ValueError(f'particle_stack: {path} holds {tuple(img.shape)} pixels, its header says {m.shape}')
            print('#', m.label, len(m.xy), 'particles', file=log)
            writer.cut(img, m.xy, int(firsts[mine[j]]))
    finally:
        writer.close()
    writer.check()
    if world > 1:
        parallel.barrier(parallel.collective_device(local_rank))       # every rank's particles are in the file
    if rank == 0:
        seal_particle_stack(plan.output, plan.header, plan.n, writer.out_bytes, plan.star_path, plan.star)


def create_particle_stack(input_file: str, output_file: str, threshold: float, size: Optional[int], resize: int,
                          image_root: Optional[str], image_ext: str, metadata_file: Optional[str], device: int = 0,
                          budget_bytes: int = DEFAULT_BUDGET, float16: bool = False) -> Plan:
    """topaz/utils/picks.py:71-197 on the MI355X; budget_bytes: device bytes of one chunk of particles.  Under `--gpus N`
    (WORLD_SIZE > 1) every rank plans the whole table and cuts its share of the micrographs into the one output file."""
    from .. import parallel
    under_ranks = int(os.environ.get('WORLD_SIZE', '1')) > 1
    quiet = under_ranks and int(os.environ.get('RANK', '0')) != 0
    plan = plan_particle_stack(input_file, output_file, threshold, size, resize, image_root, image_ext, metadata_file,
                               float16=float16, **({'log': io.StringIO()} if quiet else {}))
    ranks = parallel.init_from_env() if under_ranks else (0, 0, 1)      # (after the plan: bad input fails before the rendezvous)
    if ranks[2] > 1:
        device = parallel.rank_device(ranks[1])
    write_particle_stack(plan, device=device, budget_bytes=budget_bytes, ranks=ranks,
                         **({'log': io.StringIO()} if quiet else {}))
    return plan


# ---------------------------------------------------------------------------------------------------------------------
# `extract --particle-stack`: the stack written while the micrographs are resident for picking
# ---------------------------------------------------------------------------------------------------------------------
def check_particle_stack_args(output, size, resize, model, dims, targets, only_validate) -> None:
    """`extract --particle-stack` cuts 2-D boxes from the micrograph a network has just scored: refused without a box size, for
    tomograms, for inputs that already are score maps and for the `--targets` modes (they keep score maps resident, not images).
    Raises ValueError; touches neither the GPU nor a model file."""
    if not output:
        return
    if size is None:
        raise ValueError('--particle-stack needs --particle-size (the box size in pixels)')
    if size < 1:
        raise ValueError(f'--particle-stack: --particle-size must be positive, got {size}')
    if resize == 0 or resize > size:
        raise ValueError(f'--particle-stack: --particle-resize must lie in 1..{size} (only downsampling), got {resize}')
    if dims != 2:
        raise ValueError('--particle-stack works on micrographs (--dims 2): a particle is a 2-D box')
    if model is None or model == 'none':
        raise ValueError('--particle-stack needs a model (-m): with -m none the inputs are score maps, not micrographs')
    if targets is not None or only_validate:
        raise ValueError('--particle-stack does not go with --targets / --only-validate: they keep every score map resident, '
                         'not the micrographs')


def check_particle_stack_inputs(paths: Sequence[str]) -> None:
    """`particle_stack` orders the particles by sorted micrograph name; `extract` processes its inputs as given.  Rather than
    reorder the extraction, a list whose names (basename without extension) are not strictly increasing in plain string order
    is refused -- which refuses duplicate names too; a shell glob always passes.  The inputs must be MRC files."""
    last = None
    for p in paths:
        name, ext = os.path.splitext(os.path.basename(p))
        if ext != '.mrc':
            raise ValueError(f'--particle-stack cuts boxes from MRC micrographs (.mrc); got {p}')
        if last is not None and not last < name:
            raise ValueError(f'--particle-stack: pass the micrographs sorted by name, each once ({name!r} comes after {last!r}): '
                             'the stack holds the particles in the order `topaz particle_stack` writes them, by sorted name')
        last = name


def scores_as_read_back(xy: np.ndarray, scores: np.ndarray) -> np.ndarray:
    """float64 [n]: the scores `particle_stack` reads back from the rows `extract` writes for these picks.  The table holds a
    float32 score with the digits of its float64 value (tpz_format_picks), but pandas' default float parser is not correctly
    rounded -- about one score in eight comes back one unit in the last place off, and prints as other digits in the STAR file.
    So the value is made the way the two-command flow makes it: the same text through the same parser."""
    from .files import format_pick_rows
    scores = np.asarray(scores, dtype=np.float32).reshape(-1)
    if len(scores) == 0:
        return np.zeros(0, np.float64)
    text = format_pick_rows('m', np.asarray(xy).reshape(len(scores), -1)[:, :2], scores, 2)
    return pd.read_csv(io.BytesIO(text), sep='\t', header=None, usecols=[3])[3].values.astype(np.float64)


class ExtractStack:
    """The particle stack of `topaz extract --particle-stack`: add() is called once per micrograph, in processing order, while
    the image the feed decoded is still resident -- its kept picks are cut there and then (StackWriter) -- and finish() writes
    the header and the STAR file once the number of particles is known.

    With WORLD_SIZE > 1 the ranks advance in rounds of `world` micrographs: every add() (skip_round() for a rank the ragged last
    round leaves without an image) is one tiny all_gather of the kept counts, from which each rank derives where its particles
    go (particle_offset); finish() gathers the kept picks to rank 0 (parallel.gather_pick_tables), which writes the STAR."""

    def __init__(self, output: str, size: int, resize: int, threshold: float, metadata_file: Optional[str],
                 ranks: Tuple[int, int, int] = (0, 0, 1), budget_bytes: int = DEFAULT_BUDGET, float16: bool = False):
        self.output, self.size, self.threshold, self.metadata_file = output, int(size), float(threshold), metadata_file
        self.float16 = bool(float16)
        self.resize = self.size if resize < 0 else int(resize)
        self.rank, self.local_rank, self.world = ranks
        self.budget_bytes = budget_bytes
        self.writer: Optional[StackWriter] = None
        self.base = 0                                           # particles in the rounds so far
        self.rows: list = []                                    # (input index, kept scores fp32, kept xy int32)
        self.cell = None                                        # (cella, cellb) of the first micrograph
        # a stack from an earlier run must not survive a run that fails
        if self.rank == 0:
            for p in (output, os.path.splitext(output)[0] + '.star'):
                if os.path.exists(p):
                    os.unlink(p)

    def claim(self, n: int) -> int:
        """the stack index of the first of the n particles this rank keeps of its micrograph of the current round"""
        counts = [n]
        if self.world > 1:
            from .. import parallel
            counts = parallel.gather_scalars(float(n), parallel.collective_device(self.local_rank))
        first, self.base = particle_offset(self.base, counts, self.rank)
        return first

    def skip_round(self) -> None:
        self.claim(0)

    def add(self, index: int, path: str, image, header, scores, coords) -> int:
        """micrograph `index` of the input list: image is the device tensor the feed decoded from `path`, header its MRC header,
        (scores, coords) its pick table as written (coordinates after -x/-s).  Returns the number of particles cut."""
        from .. import runtime as rt
        if image.dim() != 2:
            raise ValueError(f'--particle-stack: {path} holds {tuple(image.shape)} pixels; a micrograph is one 2-D image')
        s32 = np.asarray(scores, dtype=np.float32).reshape(-1)
        xy = np.zeros((0, 2), np.int32)
        if len(s32):
            xy = np.ascontiguousarray(np.asarray(coords).reshape(len(s32), -1)[:, :2], dtype=np.int32)
        keep = scores_as_read_back(xy, s32) >= self.threshold
        xy = np.ascontiguousarray(xy[keep])
        check_boxes(os.path.basename(path), xy, self.size)
        if index == 0:
            self.cell = ((header.xlen, header.ylen, header.zlen), (header.alpha, header.beta, header.gamma))
        first = self.claim(len(xy))
        if self.writer is None:
            self.writer = StackWriter(rt.get_context(image.device.index), self.output, self.size, self.resize, 1,
                                      self.budget_bytes, placeholder=(self.rank == 0), float16=self.float16)
        self.writer.cut(image, xy, first)
        self.rows.append((index, s32[keep], xy))
        return len(xy)

    def close(self) -> None:
        if self.writer is not None:
            self.writer.close()

    def discard(self) -> None:
        """after a failure: no half-written stack stays behind"""
        self.close()
        if self.rank == 0 and os.path.exists(self.output):
            os.unlink(self.output)

    def finish(self, paths: Sequence[str]) -> int:
        """every micrograph has been added: wait for the writes, then (rank 0) header and STAR.  Returns the stack length."""
        import torch
        self.close()
        if self.writer is not None:
            self.writer.check()
        tables = {i: (s, xy) for i, s, xy in self.rows}
        if self.world > 1:
            from .. import parallel
            # (a collective: every rank has closed its writer, so the gathered picks are all in the file)
            got = parallel.gather_pick_tables([r[0] for r in self.rows], [torch.from_numpy(r[1]) for r in self.rows],
                                              [torch.from_numpy(r[2]) for r in self.rows],
                                              parallel.collective_device(self.local_rank))
            if self.rank == 0:
                tables = {i: (s.numpy(), c.numpy()) for i, (s, c) in got.items()}
        n = self.base
        if n == 0:
            self.discard()
            raise ValueError(f'--particle-stack: no particles left to extract at threshold {self.threshold}')
        if self.rank == 0:
            records = [Record(os.path.basename(paths[i]), tables[i][1], scores_as_read_back(tables[i][1], tables[i][0]))
                       for i in sorted(tables) if len(tables[i][0])]
            header, star_path, star = plan_from_records(records, self.output, self.size, self.resize, 1, self.cell[0],
                                                        self.cell[1], self.metadata_file, self.float16)
            seal_particle_stack(self.output, header, n, particle_bytes(1, self.resize, self.float16), star_path, star)
        return n


