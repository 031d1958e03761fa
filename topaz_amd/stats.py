"""GMM / affine image normalisation on the MI355X: the host side of topaz/stats.py:17-84,277-352
(`pixels_given_radius`, `calculate_pi`, `normalize`, `norm_fit`, `Normalize`, `normalize_images`).

The mixture fit itself (`gmm_fit`, stats.py:120-203: twelve initialisations x up to `num_iters` EM iterations over
the sampled pixels) runs on the device through `tpz_gmm_fit` -- one fused E-step pass per iteration, statistics in
fp64; the quantile splits and the optional random sub-sample are taken on the host exactly as the reference takes
them (`np.quantile`, `np.random.choice` on the global NumPy RNG), so a seeded run fits the same pixels.

That is the per-file path (`Normalize`, `normalize`, `norm_fit`).  `normalize_images`, behind the two commands, streams the files
through the device instead (second half of this file): the same results byte for byte, with the sub-sample
gathered, the quantiles selected, all initialisations fitted per pass and the image normalised without leaving the GPU; the feed
that brings the files in, the pinned ring that carries the results out and the loop between them are streaming.py's."""
from __future__ import annotations

import json
import os
import sys
from typing import List, NamedTuple, Optional

import numpy as np

from . import streaming

INIT_PIS = (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.98, 1.0)     # stats.py:91
_FIT_ARRAYS = ('mus', 'stds', 'pis', 'logps')                                    # per-initialisation results (metadata)


def _lattice_points(radius: int, dims: int) -> int:
    """integer offsets within `radius` of the origin: a disc (dims 2) or a ball (dims 3)"""
    k = np.arange(-int(radius), int(radius) + 1, dtype=np.int64) ** 2
    d2 = k[:, None] + k[None, :]
    if dims == 3:
        d2 = d2[:, :, None] + k[None, None, :]
    return int(np.count_nonzero(d2 <= int(radius) ** 2))


def pixels_given_radius(radius, dims=2):
    """Pixels the reference attributes to a particle of that radius (stats.py:17-26).  Its mask always lives on a CUBE of side
    2r + 1 whatever `dims` is; in 2-D the z axis simply does not enter the distance, so the disc is counted once per z plane --
    2r + 1 times.  `calculate_pi` feeds that number on, so it is kept."""
    if dims == 3:
        return _lattice_points(radius, 3)
    return _lattice_points(radius, 2) * (2 * int(radius) + 1)


def calculate_pi(expected_num_particles, radius, total_pixels, dims=2):
    """prior fraction of particle pixels (stats.py:29-34)"""
    return pixels_given_radius(radius, dims=dims) * expected_num_particles / total_pixels


def norm_fit(x, alpha=900, beta=1, scale=1, num_iters=100, use_cuda=True, verbose=False, tol=1e-3):
    """stats.py:87-117: fit every initialisation, keep the one with the largest log-probability.
    Returns (mu, std, pi, logp, mus, stds, pis, logps)."""
    from . import runtime as rt
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float32).ravel())
    pis = np.array(INIT_PIS, dtype=np.float64)
    splits = np.quantile(x, 1 - pis).astype(np.float64)
    mus, stds, pis_fit, logps = rt.gmm_fit(x, pis, splits, alpha=alpha, beta=beta, scale=scale, num_iters=num_iters,
                                           tol=tol)
    i = int(np.argmax(logps))
    return mus[i], stds[i], pis_fit[i], logps[i], mus, stds, pis_fit, logps


def _fit_pixels(x: np.ndarray, sample: int):
    """the pixels the mixture is fitted on and the weight each one carries: all of them, or every `sample`-th of them drawn
    without replacement from the GLOBAL NumPy RNG -- the reference's contract (stats.py:55-60): a run seeded with
    np.random.seed fits the same pixels here and there"""
    if sample <= 1:
        return x, 1
    n = int(np.round(x.size / sample))
    return np.random.choice(x.ravel(), size=n, replace=False), x.size / n


def normalize(x, alpha=900, beta=1, num_iters=100, sample=1, method='gmm', use_cuda=True, verbose=False):
    """(x - mu) / std as float32 plus the metadata dict of stats.py:37-84; mu, std = the image's own mean and standard
    deviation (`affine`) or the background component of the fitted two-component mixture (`gmm`)."""
    if method == 'affine':
        meta = {'mu': float(x.mean()), 'std': float(x.std()), 'pi': 1}
    else:
        pixels, weight = _fit_pixels(x, sample)
        fit = norm_fit(pixels, alpha=alpha, beta=beta, scale=weight, num_iters=num_iters, verbose=verbose)
        meta = dict(zip(('mu', 'std', 'pi', 'logp') + _FIT_ARRAYS, fit))
        meta.update(alpha=alpha, beta=beta, sample=sample)
    return ((x - meta['mu']) / meta['std']).astype(np.float32), meta


def _jsonable(meta: dict) -> dict:
    """the metadata with NumPy arrays and scalars as plain lists and floats"""
    out = {}
    for k, v in meta.items():
        if k in _FIT_ARRAYS:
            out[k] = np.asarray(v).tolist()
        elif isinstance(v, np.generic):
            out[k] = v.item()
        else:
            out[k] = v
    return out


class Normalize:
    """per-file worker of `topaz normalize` / `topaz preprocess` (stats.py:277-331): load, optional Fourier down-sampling,
    normalisation, one output file per requested format, optional `<name>.metadata.json`."""

    def __init__(self, dest, scale, affine, num_iters, alpha, beta, sample, metadata, formats, use_cuda=True):
        self.dest, self.scale, self.formats, self.metadata = dest, scale, formats, metadata
        self.fit_args = dict(alpha=alpha, beta=beta, num_iters=num_iters, sample=sample, method='affine' if affine else 'gmm')

    def _load(self, path):
        """(float32 pixels, MRC header or None, extended header or None), down-sampled by `scale` with the header's size
        fields following"""
        from .utils.image import downsample, load_image
        loaded = load_image(path, make_image=False)
        pixels, header, extended = loaded if isinstance(loaded, tuple) else (loaded, None, None)
        pixels = pixels.astype(np.float32)
        if self.scale > 1:
            pixels = downsample(pixels, self.scale)
            if header:
                header = header._replace(ny=pixels.shape[0], nx=pixels.shape[1])
        return pixels, header, extended

    def __call__(self, path):
        from .utils.image import save_image
        pixels, header, extended = self._load(path)
        pixels, meta = normalize(pixels, **self.fit_args)
        name = os.path.splitext(os.path.basename(path))[0]
        stem = os.path.join(self.dest, name)
        for fmt in self.formats:
            save_image(pixels, stem, f=fmt, header=header, extended_header=extended)
        if self.metadata:
            with open(stem + '.metadata.json', 'w') as fh:
                json.dump(_jsonable(meta), fh, indent=4)
        return name




# ---- the device-resident stream behind `topaz normalize` / `topaz preprocess` -------------------------------------------------
# Every pass over the pixels of `Normalize` above, on the device, image after image (streaming.stream_images): the feed decodes the
# next file into pinned memory while this one is down-sampled, sub-sampled (gather), split at its quantiles (radix select), fitted
# (all initialisations per pass) and normalised; the result leaves through the pinned result ring that a writer thread drains.  `Normalize`, `normalize` and
# `norm_fit` stay as the per-file path the stream is tested against: same files, byte for byte.

def _quantile_brackets(n: int, q):
    """np.quantile's `linear` method for n sorted values: the positions of the two bracketing order statistics and the weight
    gamma of each quantile, formed as numpy forms them (virtual index (n - 1) q; at the upper end both positions are the last
    element).  q: float64 in [0, 1]."""
    q = np.asarray(q, dtype=np.float64)
    if q.size and not (np.all(q >= 0) and np.all(q <= 1)):
        raise ValueError('Quantiles must be in the range [0, 1]')
    virtual = (n - 1) * q
    previous = np.floor(virtual)
    following = previous + 1
    above = virtual >= n - 1
    previous[above] = -1
    following[above] = -1
    gamma = virtual - previous
    return previous.astype(np.intp) % n, following.astype(np.intp) % n, gamma


def _lerp_quantiles(a, b, gamma):
    """numpy's interpolation between the bracketing values a <= b (float32) with float64 weights: a + (b - a) t below t = 0.5,
    b - (b - a)(1 - t) from there on, hence a where a == b; b - a is formed in the dtype of the values, as numpy forms it."""
    a, b = np.asarray(a), np.asarray(b)
    diff = np.subtract(b, a)
    out = np.asarray(np.add(a, diff * gamma), dtype=np.float64)
    np.subtract(b, diff * (1 - gamma), out=out, where=gamma >= 0.5)
    return out


def quantiles_device(x_dev, q):
    """np.quantile(x, q) (default `linear` method, float64 result) of a device tensor without sorting or downloading it: the
    bracketing order statistics of all quantiles come from one radix select (runtime.order_stats), the interpolation is numpy's,
    on the host.  NaN everywhere when x holds a NaN."""
    from . import runtime as rt
    q = np.asarray(q, dtype=np.float64)
    lo, hi, gamma = _quantile_brackets(int(x_dev.numel()), q.ravel())
    values = rt.order_stats(x_dev, np.concatenate([lo, hi]))
    return _lerp_quantiles(values[:lo.size], values[lo.size:], gamma).reshape(q.shape)


def sample_indices(size: int, sample: int):
    """positions of the pixels `_fit_pixels` draws from an image of `size` pixels: np.random.choice on the GLOBAL NumPy RNG picks
    values through a permutation of the positions, so drawing the positions themselves consumes the RNG identically and names the
    same pixels"""
    n = int(np.round(size / sample))
    return np.random.choice(size, size=n, replace=False)


def normalize_device(x_dev, alpha=900, beta=1, num_iters=100, sample=1, method='gmm'):
    """`normalize` of a device tensor: (normalised float32 tensor on the device, the same metadata dict)"""
    from . import runtime as rt
    if method == 'affine':
        # numpy's float32 pairwise mean / std are not what a device reduction gives bit for bit: the statistics stay numpy's
        x = x_dev.cpu().numpy()
        meta = {'mu': float(x.mean()), 'std': float(x.std()), 'pi': 1}
        return rt.normalize(x_dev, meta['mu'], meta['std']), meta
    size = int(x_dev.numel())
    pixels, weight = x_dev.reshape(-1), 1
    if sample > 1:
        idx = sample_indices(size, sample)
        pixels, weight = rt.gather(x_dev, idx), size / len(idx)
    pis = np.array(INIT_PIS, dtype=np.float64)
    splits = quantiles_device(pixels, 1 - pis)
    mus, stds, pis_fit, logps, _ = rt.gmm_fit_fused(pixels, pis, splits, alpha=alpha, beta=beta, scale=weight,
                                                    num_iters=num_iters, tol=1e-3)
    i = int(np.argmax(logps))
    meta = dict(zip(('mu', 'std', 'pi', 'logp') + _FIT_ARRAYS, (mus[i], stds[i], pis_fit[i], logps[i], mus, stds, pis_fit, logps)))
    meta.update(alpha=alpha, beta=beta, sample=sample)
    return rt.normalize_f64(x_dev, meta['mu'], meta['std']), meta


class DevicePreprocess:
    """What `topaz preprocess -s scale` does to one micrograph, on a device tensor: Fourier down-sampling by `scale` (when > 1), then
    the mixture-fit (or `affine`) normalisation -- the two steps of `_normalize_stream` below, through the same functions, so the
    result equals the file `topaz preprocess` writes bit for bit.  `topaz extract --preprocess` applies it to every image before
    scoring.  With sample > 1 each call draws from the global NumPy RNG: call it in path order.  `last_meta` keeps the metadata
    of the latest call (what --metadata would have written)."""

    def __init__(self, scale=1, affine=False, niters=100, alpha=900, beta=1, sample=10):
        self.scale = int(scale)
        if self.scale < 1:
            raise ValueError(f'preprocess scale must be >= 1, got {scale}')
        self.fit_args = dict(alpha=alpha, beta=beta, num_iters=niters, sample=sample, method='affine' if affine else 'gmm')
        self.last_meta = None

    def __call__(self, x_dev):
        from .utils.image import downsample_device
        if x_dev.dim() != 2:
            raise NotImplementedError('preprocess: 2-D micrographs only')
        if self.scale > 1:
            x_dev = downsample_device(x_dev, self.scale)
        y, self.last_meta = normalize_device(x_dev, **self.fit_args)
        return y


EIGHT_BIT_FORMATS = ('png', 'jpg', 'jpeg')     # save_image quantises these with mi, ma = -3, 3


class _Output(NamedTuple):
    """what the writer of _normalize_stream needs besides the pixels of one put"""
    path: str
    header: object
    extended: object
    meta: Optional[dict]
    formats: List[str]          # the formats written from these pixels
    last: bool                  # the image's last put: the metadata file and the progress line follow it


def _normalize_stream(paths: List[str], dest: str, scale: int, fit_args: dict, metadata: bool, formats: List[str],
                      verbose: bool, float16: bool = False) -> None:
    """the loop of `normalize_images` over this process's files: streaming.stream_images around the two halves below.  The
    result leaves the device in the type each format stores: float32 (or float16, encoded there: `float16`) for mrc / tiff, and
    the uint8 of save_image's quantize, made there as well, for png / jpg -- one put per stored type."""
    from . import runtime as rt
    from .utils.image import downsample_device, save_image
    if not paths:
        return
    affine = fit_args['method'] == 'affine'
    # (--affine normalises on the host, in the writer: the image comes down as float32 and is converted there)
    as_float = [f for f in formats if affine or f not in EIGHT_BIT_FORMATS]
    as_bytes = [f for f in formats if f not in as_float]

    def process(path, x, header, extended):
        if scale > 1:
            x = downsample_device(x, scale)
            if header:
                header = header._replace(ny=x.shape[0], nx=x.shape[1])
        if affine:
            # (a copy when x is still the feed's own slot, which the feed re-uses once the next image is asked for)
            y, meta = (x if scale > 1 else x.clone()), None
        else:
            y, meta = normalize_device(x, **fit_args)        # every RNG draw happens here, in path order
        # one put per stored type; the last one of an image also writes its metadata
        puts = []
        if as_float or not as_bytes:
            puts.append((as_float, rt.ENC_F16 if float16 and not affine else None))
        if as_bytes:
            puts.append((as_bytes, (rt.ENC_U8, (-3, 3))))
        return [streaming.Put(y, (_Output(path, header, extended, meta, fmts, k == len(puts) - 1),), encode)
                for k, (fmts, encode) in enumerate(puts)]

    def write(pixels, job):
        path, header, extended, meta, fmts, last = job
        name = os.path.splitext(os.path.basename(path))[0]
        stem = os.path.join(dest, name)
        if affine:
            # --affine keeps numpy's own statistics: the (down-sampled) image came down, the per-file expressions run here,
            # under the GPU's work on the next image
            pixels, meta = normalize(pixels, **fit_args)
            if float16:
                pixels = streaming.as_float16(pixels, stem + '.mrc')
        for fmt in fmts:
            save_image(pixels, stem, f=fmt, header=header, extended_header=extended)
        if not last:
            return
        if metadata:
            with open(stem + '.metadata.json', 'w') as fh:
                json.dump(_jsonable(meta), fh, indent=4)
        if verbose:
            print('# processed:', name, file=sys.stderr)

    def overflowed(lost, job):
        streaming.warn_overflow(os.path.join(dest, os.path.splitext(os.path.basename(job.path))[0]) + '.mrc', lost)

    streaming.stream_images(paths, rt.get_context(), process, write, on_overflow=overflowed)


def normalize_images(paths: List[str], dest: str, num_workers: int, scale: int, affine: bool, niters: int, alpha: float,
                     beta: float, sample: int, metadata: bool, formats: List[str], use_cuda: bool = True,
                     verbose: bool = False, float16: bool = False):
    """stats.py:334-352 as a device-resident stream.  Rank r of a multi-process launch takes files r, r + world, ...; the ranks
    write disjoint files and exchange nothing.  With sample > 1 each rank draws the sub-samples of ITS files from its own RNG, so
    the fitted subsets depend on the number of ranks (sample = 1: the same files for any number).  `num_workers` is accepted and
    unused: the parallelism is the reader / GPU / writer pipeline and the ranks.  float16: the MRC files are stored as float16
    (mode 12), encoded on the device; only with formats == ['mrc']."""
    from . import mrc, parallel
    mrc.check_float16_formats(float16, formats)
    rank, _, world = parallel.init_from_env()
    os.makedirs(dest, exist_ok=True)
    mine = [paths[i] for i in parallel.shard_indices(len(paths), rank, world)]
    fit_args = dict(alpha=alpha, beta=beta, num_iters=niters, sample=sample, method='affine' if affine else 'gmm')
    _normalize_stream(mine, dest, scale, fit_args, metadata, formats, verbose, float16)
