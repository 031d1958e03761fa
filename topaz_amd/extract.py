"""`topaz extract` on the MI355X: score micrographs, suppress non-maxima, write pick tables.

Drop-in surface of topaz/extract.py -- the names callers import keep their arguments and return values
(NonMaximumSuppression / nms_iterator :26-104, extract_auprc / find_opt_radius :135-204, score_images :224-256,
stream_inputs :259-263, extract_particles :266-367) -- over a different engine:

  ImageFeed      (streaming.py, imported here: `score_images` looks it up as a global of this module) a reader thread decodes
                 micrograph i+1 straight into a pinned staging slot (tpz_stage) and queues its H2D copy while the GPU scores
                 micrograph i; the host never waits for a copy.
  Scorer         the filled network as one HIP model (load once, one forward per image); score maps stay in HBM.
  suppression    tpz_nms_2d / _3d on the device map; only the pick table crosses PCIe.
  RadiusSearch   `--targets`: score maps cached on the device once, one device NMS + one Hungarian matching per radius.
  PickSink       the three output shapes (one TSV, per-micrograph tables, stdout).
  ExtractStack   `--particle-stack` (utils/picks.py): the boxes around a micrograph's picks, cut from the image the feed decoded
                 while it is still resident and streamed into the MRC stack `topaz particle_stack` would write.

Differences from the reference, all deliberate: there is no CPU path (`device` < 0 raises); worker pools are accepted and
ignored (the suppression is on the GPU); with WORLD_SIZE > 1 the micrographs are dealt round-robin to the ranks and the
pick tables gathered to rank 0 over RCCL (topaz_amd/parallel.py), as are the per-image records of the `--targets` radius
search, which rank 0 pools in single-process order; an existing directory given as `-o` receives
`extracted_particles.txt` (upstream: `sys.path.join` typo, extract.py:318) and `COORDS/` is created (upstream forgets).
The patched suppression branch of NonMaximumSuppression cannot run upstream (extract.py:55 unpacks three values from a
two-tuple; the default 64/32 tiling has step 0): it is implemented here as written-to-be, tile by tile on the device.
"""
from __future__ import annotations

import os
import sys
from typing import Dict, Iterable, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import pandas as pd
import torch

from . import parallel
from .algorithms import match_coordinates, non_maximum_suppression, non_maximum_suppression_3d
from .metrics import average_precision
from .model.factory import load_model
from .model.utils import predict_in_patches_device
from .precision import check_loaded_model
from .streaming import ImageFeed
from .utils import files as file_utils
from .utils.image import load_image
from .utils.printing import report

__all__ = ['NonMaximumSuppression', 'crop_translate_coords_scores', 'nms_iterator', 'extract_auprc', 'find_opt_radius',
           'score_images', 'stream_inputs', 'extract_particles', 'match_coordinates']


# ---------------------------------------------------------------------------------------------------------------------
# suppression
# ---------------------------------------------------------------------------------------------------------------------
def _suppress(score, radius: int, threshold: float, dims: int) -> Tuple[np.ndarray, np.ndarray]:
    if dims == 3:
        return non_maximum_suppression_3d(score, radius, threshold=threshold)
    return non_maximum_suppression(score, radius, threshold=threshold)


def crop_translate_coords_scores(scores, coords, patch_size, patch_overlap, x, y, z=None):
    """keep the picks of a tile that lie in its core [overlap, overlap + patch_size) on every axis and move them to
    image coordinates (tile origin x, y[, z]); coords columns are (x, y[, z])"""
    coords = np.asarray(coords)
    core = ((coords >= patch_overlap) & (coords < patch_size + patch_overlap)).all(axis=-1)
    moved = coords[core].copy()
    for column, origin in enumerate((x, y) if z is None else (x, y, z)):
        moved[:, column] += origin
    return np.asarray(scores)[core], moved


class NonMaximumSuppression:
    """callable (name, score map) -> (name, scores, coords); whole image when `patch_size` is falsy (what the CLI uses)"""

    def __init__(self, radius: int, threshold: float, dims: int = 2, patch_size=64, patch_overlap=32, verbose: bool = False):
        self.radius, self.threshold, self.dims = radius, threshold, dims
        self.patch_size, self.patch_overlap, self.verbose = patch_size, patch_overlap, verbose

    def __call__(self, item):
        name, score = item
        if self.verbose:
            report(f'Scoring {name}')
        if not self.patch_size:
            s, c = _suppress(score, self.radius, self.threshold, self.dims)
            return name, s, c
        step = self.patch_size - 2 * self.patch_overlap
        if step <= 0:
            raise ValueError(f'patch_size {self.patch_size} leaves no core after removing 2 x {self.patch_overlap} overlap')
        t = (score if torch.is_tensor(score) else torch.as_tensor(np.asarray(score))).float()
        ov, size = self.patch_overlap, self.patch_size
        # halo of -inf: the padding must neither be picked nor suppress picks next to the border
        padded = torch.nn.functional.pad(t[None], (ov, ov) * self.dims, value=float('-inf'))[0]
        shape = tuple(t.shape)
        kept_s, kept_c = [], []
        for i in range(0, shape[-2], step):
            for j in range(0, shape[-1], step):
                for k in (range(0, shape[-3], step) if self.dims == 3 else (None,)):
                    tile = padded[i:i + size, j:j + size] if k is None else padded[k:k + size, i:i + size, j:j + size]
                    s, c = _suppress(tile.contiguous(), self.radius, self.threshold, self.dims)
                    s, c = crop_translate_coords_scores(s, c, step, ov, j - ov, i - ov, None if k is None else k - ov)
                    kept_s.append(s)
                    kept_c.append(c)
        if not kept_s:
            return name, np.array([]), np.array([])
        return name, np.concatenate(kept_s, axis=0), np.concatenate(kept_c, axis=0)


def nms_iterator(paths_scores, radius, threshold, pool=None, dims=2, patch_size=0, patch_overlap=0, verbose=False):
    """(name, score map) pairs -> (name, scores, coords); `pool` is accepted and ignored (the GPU is the pool)"""
    suppress = NonMaximumSuppression(radius, threshold, dims=dims, patch_size=patch_size, patch_overlap=patch_overlap,
                                     verbose=verbose)
    return (suppress(item) for item in paths_scores)


# ---------------------------------------------------------------------------------------------------------------------
# `--targets`: validation and radius search
# ---------------------------------------------------------------------------------------------------------------------
class RadiusSearch:
    """Score maps (kept wherever they are -- device tensors stay in HBM) against a table of labelled coordinates.
    evaluate(r) = one suppression per micrograph at radius r (doubled for tomograms, like ExtractMatches :125),
    Hungarian matching of picks to targets within `match_radius` (default r), pooled average precision."""

    def __init__(self, targets: pd.DataFrame, scores: Dict[str, object], threshold: float, match_radius=None, dims: int = 2):
        self.threshold, self.match_radius, self.dims = threshold, match_radius, dims
        self.pairs = [(score, targets.loc[targets.image_name == name, ['x_coord', 'y_coord']].values)
                      for name, score in scores.items()]

    def evaluate_local(self, radius) -> List[Tuple[np.ndarray, np.ndarray, float, int]]:
        """one record per map of this object, in the order of `self.pairs`: (hit flag of every pick fp32[n], its score
        fp32[n], summed squared distance of the hits to their targets, number of targets).  What a rank of a sharded job
        computes; `reduce` pools the records of every rank."""
        records = []
        for score, target in self.pairs:
            s, coords = _suppress(score, radius * 2 if self.dims == 3 else radius, self.threshold, self.dims)
            matched, dist = match_coordinates(target, coords, radius if self.match_radius is None else self.match_radius)
            records.append((matched, s, float(np.sum(dist[matched == 1] ** 2)), len(target)))
        return records

    @staticmethod
    def reduce(records) -> Tuple[float, float, int, int]:
        """(auprc, rmse, hits, targets) of records given IN SINGLE-PROCESS IMAGE ORDER: the average precision sorts by score
        with ties kept in input order and the squared error is a float sum, so both depend on it"""
        sq_err, n_targets, hit_flags, hit_scores = 0.0, 0, [], []
        for matched, s, err, n in records:
            sq_err += err
            hit_flags.append(matched)
            hit_scores.append(s)
            n_targets += n
        hits, preds = np.concatenate(hit_flags), np.concatenate(hit_scores)
        n_hit = hits.sum()
        return average_precision(hits, preds, N=n_targets), np.sqrt(sq_err / n_hit), int(n_hit), n_targets

    def evaluate(self, radius) -> Tuple[float, float, int, int]:
        return self.reduce(self.evaluate_local(radius))

    @staticmethod
    def line(radius, result) -> str:
        au, rmse, recall, n = result
        return '# radius={}, auprc={}, rmse={}, recall={}, targets={}'.format(radius, au, rmse, recall, n)

    def best(self, lo: int, hi: int, step: int) -> Tuple[int, float]:
        curve = np.full(hi + 1, -1.0)
        for r in range(lo, hi + 1, step):
            res = self.evaluate(r)
            curve[r] = res[0]
            print(self.line(r, res))
        r = int(np.argmax(curve))
        return r, curve[r]


def _radius_over_ranks(search: RadiusSearch, image_ids: Sequence[int], radius: int, lo: int, hi: int, step: int, rank: int,
                       local_rank: int) -> int:
    """`--targets` with WORLD_SIZE > 1.  Every rank evaluates the maps it holds (`image_ids`: their positions in the
    single-process image order; none is fine) at every radius of the sweep, or at the one given radius; ONE exchange moves all
    records to rank 0 (parallel.gather_radius_records), which pools them per radius in that order -- the arithmetic of one
    process, bit for bit --, prints what one process prints and broadcasts the radius every rank then extracts at."""
    dev = parallel.collective_device(local_rank)
    searching = radius < 0
    radii = list(range(lo, hi + 1, step)) if searching else [radius]
    if searching and rank == 0:
        report('Finding optimal radius for extraction')
    gathered = parallel.gather_radius_records([search.evaluate_local(r) for r in radii], image_ids, dev)
    if rank == 0:
        curve = np.full(hi + 1, -1.0)
        for r, records in zip(radii, gathered):
            res = RadiusSearch.reduce(records)
            print(RadiusSearch.line(r, res))
            if searching:
                curve[r] = res[0]
        if searching:
            radius = int(np.argmax(curve))
            report(f'Optimal radius found: {radius} with AUPRC: {curve[radius]}')
    return parallel.broadcast_int(radius, 0, dev)


def extract_auprc(targets, scores, radius, threshold, match_radius=None, pool=None, dims=2):
    return RadiusSearch(targets, scores, threshold, match_radius, dims).evaluate(radius)


def find_opt_radius(targets, target_scores, threshold, lo=0, hi=200, step=10, match_radius=None, pool=None, dims=2):
    return RadiusSearch(targets, target_scores, threshold, match_radius, dims).best(lo, hi, step)


# ---------------------------------------------------------------------------------------------------------------------
# scoring
# ---------------------------------------------------------------------------------------------------------------------
class Scorer:
    """the filled scoring network on one MI355X"""

    def __init__(self, model, device: int = 0, precision_check: str = 'never', verbose: bool = False):
        """precision_check: the `--precision-check` mode (precision.check_loaded_model: once, here, before the first image)"""
        if device is not None and device < 0:
            raise RuntimeError('topaz_amd has no CPU path: use -d >= 0 (an MI355X)')
        torch.cuda.set_device(device)
        self.device = device
        self.model = load_model(model)
        self.model.eval()
        self.model.fill()
        self.model.cuda(device)
        self.ctx = self.model.device_model.ctx
        self.precision = check_loaded_model(self.model, precision_check, model, verbose)

    def __call__(self, image: torch.Tensor, patch_size: int = 0):
        """[H, W] / [D, H, W] device tensor -> logits of the same shape, a float32 device tensor; patched: the map
        predict_in_patches stitches, left where the suppression reads it (its float64 values are these float32 numbers)"""
        if patch_size:
            halo = self.model.width // 2
            return predict_in_patches_device(self.model, image, patch_size + 2 * halo, is_3d=(image.dim() == 3))
        with torch.no_grad():
            return self.model(image[None, None])[0, 0]


def score_images(model, paths: Iterable[str], device: int = 0, patch_size: int = 0, batch_size: int = 1,
                 keep_on_device: bool = False, precision_check: str = 'never',
                 verbose: bool = False, preprocess=None, with_image: bool = False) -> Iterator[Tuple[str, np.ndarray]]:
    """generator of (path, score map).  `model` None / 'none': the inputs already are score maps (what `segment` wrote: TIFF,
    MRC, .npy volumes) and pass through -- under keep_on_device through the ImageFeed, as device tensors of their own.
    keep_on_device=True yields device tensors (no PCIe round trip before the suppression).  precision_check / verbose: the
    `--precision-check` mode of the loaded model (Scorer).  preprocess: a callable device tensor -> device tensor (e.g.
    stats.DevicePreprocess) applied to every image the feed yields before it is scored -- here, in the consuming thread and in
    path order, so whatever it draws from the NumPy RNG is drawn in the order `topaz preprocess` draws it.
    with_image=True: items are (path, score map, image, MRC header or None) -- image is the device tensor the feed decoded from
    the file, BEFORE `preprocess`; it aliases a staging slot and is valid until the consumer asks for the next item."""
    paths = list(paths)
    if model is None or model == 'none':
        if preprocess is not None:
            raise ValueError('preprocess needs a model: score maps are not micrographs')
        if with_image:
            raise ValueError('with_image needs a model: score maps are not micrographs')
        if not keep_on_device:
            for path in paths:
                yield path, _load_map(path)
            return
        # the maps take the road micrographs take: the feed's reader thread reads map i+1 (an MRC file in the type it stores,
        # decoded on the device; TIFF through PIL; a .npy volume as an item in memory) under the suppression of map i.  Each is
        # copied out of its staging slot, which the feed re-uses: the caller may keep every map (`--targets`)
        from . import runtime as rt
        if device is not None and device < 0:
            raise RuntimeError('topaz_amd has no CPU path: use -d >= 0 (an MI355X)')
        torch.cuda.set_device(device)
        items = [(p, np.load(p, mmap_mode='r'), None, None) if os.path.splitext(p)[1] == '.npy' else p for p in paths]
        for path, scores in ImageFeed(items, rt.get_context(device)):
            yield path, scores.clone()
        return
    scorer = Scorer(model, device, precision_check, verbose)
    for item in (ImageFeed(paths, scorer.ctx, headers=True) if with_image else ImageFeed(paths, scorer.ctx)):
        path, raw = item[0], item[1]
        image = raw if preprocess is None else preprocess(raw)
        scores = scorer(image, patch_size)
        if torch.is_tensor(scores) and not keep_on_device:
            scores = scores.cpu().numpy()
            if patch_size:
                scores = scores.astype(np.float64)               # (what predict_in_patches returns, upstream and here)
        if with_image:
            yield path, scores, raw, item[2]
        else:
            yield path, scores


def _load_map(path: str) -> np.ndarray:
    """a score map on the host: an image file, or the .npy volume `segment` writes of a tomogram"""
    if os.path.splitext(path)[1] == '.npy':
        return np.load(path)
    return load_image(path, make_image=False, return_header=False)


def _keep_resident(items, resident: list):
    """(path, score map) of score_images(with_image=True) items, for the suppression; the image and the header of the item being
    worked on are left in `resident` -- replaced, not collected: the tensor is only valid until the next item is asked for"""
    for path, scores, image, header in items:
        resident[:] = [image, header]
        yield path, scores
    resident[:] = []


def check_preprocess_args(preprocess, model, dims) -> None:
    """`--preprocess` is the 2-D `topaz preprocess` in front of a scoring network: refused for tomograms and for inputs that
    already are score maps.  Raises ValueError; touches neither the GPU nor a model file."""
    if not preprocess:
        return
    if dims != 2:
        raise ValueError('--preprocess works on micrographs (--dims 2): `topaz preprocess` has no 3-D form')
    if model is None or model == 'none':
        raise ValueError('--preprocess needs a model (-m): with -m none the inputs already are score maps')


def stream_inputs(f) -> Iterator[str]:
    return (line.strip() for line in f if line.strip())


# ---------------------------------------------------------------------------------------------------------------------
# output
# ---------------------------------------------------------------------------------------------------------------------
class PickSink:
    """where pick tables go: one TSV (file or stdout, rank 0 writes it after the gather) or one table per micrograph
    (each rank writes its own files)"""

    def __init__(self, output: Optional[str], per_micrograph: bool, suffix: str, out_format: str, dims: int):
        self.per_micrograph, self.suffix, self.format, self.dims = per_micrograph, suffix, out_format, dims
        self.rows: List[Tuple[int, str, np.ndarray, np.ndarray]] = []
        if per_micrograph:
            if os.path.isdir(output):
                self.dir = output
            else:
                parent = os.path.dirname(output)
                self.dir = os.path.join(parent, 'COORDS')
                os.makedirs(self.dir, exist_ok=True)
            self.path = None
        else:
            self.dir = None
            self.path = os.path.join(output, 'extracted_particles.txt') if (output is not None and os.path.isdir(output)) \
                else output

    def add(self, index: int, path: str, scores: np.ndarray, coords: np.ndarray) -> None:
        name, ext = os.path.splitext(os.path.basename(path))
        if not self.per_micrograph:
            self.rows.append((index, name, scores, coords))
            return
        cols = {'image_name': name, 'x_coord': coords[:, 0], 'y_coord': coords[:, 1]}
        if self.dims == 3:
            cols['z_coord'] = coords[:, 2]
        cols['score'] = scores
        with open(os.path.join(self.dir, name + self.suffix + '.' + self.format), 'w') as f:
            file_utils.write_table(f, pd.DataFrame(cols), format=self.format, image_ext=ext)

    def finish(self, paths: Sequence[str], rank: int, world: int, local_rank: int) -> None:
        if self.per_micrograph:
            return
        tables = {i: (name, s, c) for i, name, s, c in self.rows}
        if world > 1:
            dev = parallel.collective_device(local_rank)
            got = parallel.gather_pick_tables([r[0] for r in self.rows],
                                              [torch.from_numpy(np.asarray(r[2], dtype=np.float32)) for r in self.rows],
                                              [torch.from_numpy(np.asarray(r[3], dtype=np.int32)) for r in self.rows], dev)
            if rank == 0:
                tables = {i: (os.path.splitext(os.path.basename(paths[i]))[0], s.numpy(), c.numpy()) for i, (s, c) in got.items()}
        if rank != 0:
            return
        # rows formatted by the library's host-side writer (tpz_format_picks: the f-string's text -- a float32 score with the
        # digits of its float64 value -- byte for byte; tests/test_cpu_host.py), not by a Python loop over the picks
        out = sys.stdout if self.path is None else open(self.path, 'w')
        try:
            print('image_name\tx_coord\ty_coord' + ('\tz_coord' if self.dims == 3 else '') + '\tscore', file=out)
            for i in sorted(tables):
                name, scores, coords = tables[i]
                out.write(file_utils.format_pick_rows(name, coords, scores, self.dims).decode())
        finally:
            if out is not sys.stdout:
                out.close()


# ---------------------------------------------------------------------------------------------------------------------
# the command
# ---------------------------------------------------------------------------------------------------------------------
def extract_particles(paths: List[str], model, device: int, batch_size: int, threshold: float, radius: int,
                      num_workers: int, targets: str, min_radius: int, max_radius: int, step: int, match_radius: int,
                      patch_size, only_validate: bool, output: str, per_micrograph: bool, suffix: str, out_format: str,
                      up_scale: float, down_scale: float, dims=2, verbose: bool = False, precision_check: str = 'never',
                      preprocess=None, particle_stack: Optional[str] = None, particle_size: Optional[int] = None,
                      particle_resize: int = -1, particle_threshold: float = -np.inf, particle_metadata: Optional[str] = None,
                      particle_float16: bool = False):
    """preprocess: None, or a callable device tensor -> device tensor (stats.DevicePreprocess) every micrograph goes through
    before it is scored (`--preprocess`).  Everything downstream -- patches, the radius search, the ranks, the outputs -- sees
    the smaller, normalised image only: picks are in ITS frame, as they are when `topaz preprocess` wrote it to a file first;
    up_scale / down_scale move them, as ever.
    particle_stack: also write the MRC particle stack (and its STAR file) `topaz particle_stack` would make of the pick table:
    particle_size boxes (particle_resize: down-sampled to that size) around the picks with score >= particle_threshold, cut at
    the coordinates the table holds from the image the feed decoded -- under `preprocess` the raw frame -- while it is resident
    (utils.picks.ExtractStack); particle_float16: stored as float16 (MRC mode 12).  The pick table itself is what it is without
    the stack."""
    from .utils import picks as pk
    check_preprocess_args(preprocess, model, dims)               # (before anything is loaded)
    pk.check_particle_stack_args(particle_stack, particle_size, particle_resize, model, dims, targets, only_validate)
    report('Beginning extraction')
    rank, local_rank, world = parallel.init_from_env()
    if world > 1:
        device = parallel.rank_device(local_rank)
    if len(paths):
        paths = list(paths)
    elif parallel.under_launcher() and os.environ.get('TOPAZ_AMD_INPUT_LIST'):
        # a rank of `topaz extract --gpus N < list`: the launcher read stdin once for all ranks (main.py).  Only a rank process
        # honours the variable, and only once: a stale / exported copy must not silently replace stdin elsewhere
        with open(os.environ.pop('TOPAZ_AMD_INPUT_LIST')) as f:
            paths = list(stream_inputs(f))
    else:
        paths = list(stream_inputs(sys.stdin))
    stack = None
    if particle_stack:
        pk.check_particle_stack_inputs(paths)                    # (still nothing loaded)
        stack = pk.ExtractStack(particle_stack, particle_size, particle_resize, particle_threshold, particle_metadata,
                                (rank, local_rank, world), float16=particle_float16)
    mine = parallel.shard_indices(len(paths), rank, world)
    maps = score_images(model, [paths[i] for i in mine], device=device, patch_size=patch_size, batch_size=batch_size,
                        keep_on_device=True, precision_check=precision_check, verbose=verbose, preprocess=preprocess,
                        with_image=stack is not None)
    resident: list = []                                          # the image (and header) behind the score map being suppressed
    if stack is not None:
        maps = _keep_resident(maps, resident)
    radius = -1 if radius is None else radius

    if targets is not None:
        # every score map is needed at once (they stay in HBM); the table is keyed by the paths as given (extract.py:284-290)
        maps = dict(maps)
        table = pd.read_csv(targets, sep='\t')
        # the images of the table in single-process order; each is evaluated by the rank that scored it (the last one, had the
        # list named it twice) and carries its position in that order through the exchange
        owner = {p: i for i, p in enumerate(paths)}
        named = [n for n in table.image_name.unique() if n in owner]
        held = [g for g, n in enumerate(named) if owner[n] % world == rank]
        search = RadiusSearch(table, {named[g]: maps[named[g]] for g in held}, threshold, match_radius, dims)
        if world > 1:
            radius = _radius_over_ranks(search, held, radius, min_radius, max_radius, step, rank, local_rank)
        elif radius < 0:
            report('Finding optimal radius for extraction')
            radius, auprc = search.best(min_radius, max_radius, step)
            report(f'Optimal radius found: {radius} with AUPRC: {auprc}')
        else:
            print(search.line(radius, search.evaluate(radius)))
        maps = maps.items()
    elif radius < 0:
        raise Exception('Must specify targets for choosing the extraction radius if extraction radius is not provided')

    if not only_validate:
        sink = PickSink(output, per_micrograph, suffix, out_format, dims)
        scale = up_scale / down_scale
        for k, (path, scores, coords) in enumerate(nms_iterator(maps, radius, threshold, dims=dims, verbose=verbose)):
            if verbose:
                report(f'Extracted {len(scores)} particles from {os.path.splitext(os.path.basename(path))[0]}')
            if scale != 1:
                coords = np.round(coords * scale).astype(int)
            sink.add(mine[k], path, scores, coords)
            if stack is not None:
                try:
                    stack.add(mine[k], path, resident[0], resident[1], scores, coords)
                except BaseException:
                    stack.discard()
                    raise
        if stack is not None:
            for _ in range(len(mine), -(-len(paths) // world)):   # a ragged last round: the ranks without an image take part
                stack.skip_round()
        sink.finish(paths, rank, world, local_rank)
        if stack is not None:
            n = stack.finish(paths)
            if verbose and rank == 0:
                report(f'Wrote {n} particles to {particle_stack}')
    report('Extraction complete')
