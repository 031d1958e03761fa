"""Mirror of the inference side of topaz/denoise.py: Denoise (:245-332), Denoise3D (:336-377),
denoise_image (:382-416), denoise_stack (:419-447), denoise_stream (:450-490), denoise_tomogram
(:495-530) and denoise_tomogram_stream (:533-557).

Patching, per-patch normalisation (torch mean / unbiased std), the network and the stitching all
run on the device inside tpz_denoise_2d / tpz_denoise_3d; only the image goes in and the denoised
image comes out.

The pre-filters of denoise_image mirror spatial_covariance (:22-49), estimate_unblur_filter (:52-75),
correct_spatial_covariance (:129-172) and the 2-D lowpass (:174-197).  Both flags crash in v0.3.18 (SURVEY.md P6:
`lowpass` is shadowed by the parameter, the deconvolution is handed an ndarray); they run here as evidently intended
(DESIGN.md §9): lowpass as fp64 GEMMs with the projections onto the kept frequencies (tpz_lowpass_2d), the deconvolution
as per-tile lag covariances (tpz_spatial_cov_2d), the host's float64 filter design and one per-tile filter over the
whole image (tpz_tile_filter_2d).

The device-resident drivers of 2-D images (`denoise`, `denoise --stack`) are streaming.stream_images around
denoise_image_device: the feed, the pinned result ring and its writer thread live in streaming.py, not here.
"""
from __future__ import annotations

import functools
import itertools
import os
import sys
from typing import List, Optional, Union

import numpy as np
import torch

from . import runtime as rt
from . import streaming
from .denoising.models import DenoiseNet, load_model
from .filters import AffineFilter, GaussianDenoise, InvGaussianFilter


class Denoise:
    """Object for micrograph denoising utilities (denoise.py:245-332)."""

    def __init__(self, model: Union[DenoiseNet, str], use_cuda: bool = True, dims: int = 2):
        if isinstance(model, DenoiseNet):
            self.model = model
        elif isinstance(model, str):
            try:
                self.model = load_model(model)
            except Exception as e:
                raise ValueError('Unable to load model: ' + model) from e
        else:
            raise TypeError('Unrecognized model:' + str(model))
        self.model.cuda()                       # the MI355X path has no CPU mode
        self.device = self.model.device_model.ctx.torch_device()
        self.dims = dims
        self.use_cuda = True

    def __call__(self, input):
        return self._denoise(input)

    def _to_device(self, x) -> torch.Tensor:
        return rt.as_device_f32(x, self.model.device_model.ctx)

    def _denoise(self, input) -> np.ndarray:
        """normalise by the array's own mean / unbiased std, model, un-normalise (denoise.py:274-296)"""
        x = self._to_device(input)
        if x.dim() == self.dims + 1 and x.shape[0] == 1:
            x = x[0]
        if x.dim() != self.dims:
            raise ValueError(f'expected a {self.dims}-D array, got shape {tuple(x.shape)}')
        dm = self.model.device_model
        y = dm.denoise_3d(x, -1, 0) if self.dims == 3 else dm.denoise_2d(x, -1, 0)
        return y.cpu().numpy()

    def denoise_patches(self, x, patch_size: int, padding: int = 128) -> np.ndarray:
        return self._run2d(x, patch_size, padding, force_patches=True)

    def denoise(self, x, patch_size: int = -1, padding: int = 128) -> np.ndarray:
        return self._run2d(x, patch_size, padding)

    def denoise_device(self, x: torch.Tensor, patch_size: int = -1, padding: int = 128) -> torch.Tensor:
        """same as denoise() but device tensor in, device tensor out (no PCIe traffic)"""
        if self.dims == 3:
            return self.model.device_model.denoise_3d(x, -1, 0)
        return self.model.device_model.denoise_2d(x, patch_size, padding)

    def _run2d(self, x, patch_size, padding, force_patches=False) -> np.ndarray:
        if self.dims == 3:
            return self._denoise(x)
        xd = self._to_device(x)
        if force_patches and not (patch_size > 0 and (patch_size + padding < xd.shape[0] or patch_size + padding < xd.shape[1])):
            # denoise_patches called directly on a small image still tiles it (denoise.py:307-322)
            out = np.zeros(tuple(xd.shape), dtype=np.float32)
            H, W = xd.shape
            for i in range(0, H, patch_size):
                for j in range(0, W, patch_size):
                    si, ei = max(0, i - padding), min(H, i + patch_size + padding)
                    sj, ej = max(0, j - padding), min(W, j + patch_size + padding)
                    yij = self.model.device_model.denoise_2d(xd[si:ei, sj:ej].contiguous(), -1, 0).cpu().numpy()
                    oi, oj = i - si, j - sj
                    out[i:i + patch_size, j:j + patch_size] = yij[oi:oi + patch_size, oj:oj + patch_size]
            return out
        return self.model.device_model.denoise_2d(xd, patch_size, padding).cpu().numpy()


class Denoise3D(Denoise):
    """Object for denoising tomograms (denoise.py:336-377)."""

    def __init__(self, model, use_cuda: bool = True, dims: int = 3):
        super().__init__(model, use_cuda, dims=3)

    def denoise(self, tomo: np.ndarray, patch_size: int = 96, padding: int = 48, batch_size: int = 1,
                volume_num: int = 1, total_volumes: int = 1, verbose: bool = True, across_ranks: bool = False,
                stored: Optional[dict] = None) -> np.ndarray:
        """across_ranks=True (multi-process launch, every rank holding the same tomogram): the ceil(n / patch)^3 tiles are
        dealt round-robin to the ranks -- they are independent (datasets.py:412-468), the global mean / std every rank
        computes over the whole volume is the same deterministic reduction -- and the ranks' partial volumes are summed onto
        rank 0 with one RCCL reduce; the other ranks return None.  stored: a dict that receives the float16 form of the result,
        encoded on the resident volume before the download (tpz_encode) -- 'half', and 'lost', the finite voxels stored as inf."""
        x = self._to_device(tomo)
        dm = self.model.device_model
        if across_ranks and patch_size >= 1:
            from . import parallel
            rank, _, world = parallel.init_from_env()
            part = dm.denoise_3d(x, patch_size, padding, shard=rank, n_shards=world)
            if parallel.collective_device(0).type == 'cpu':       # gloo rehearsal (ranks sharing a GPU): reduce host tensors
                part = part.cpu()
            y = parallel.sum_to_root(part)
            if y is None:
                return None
        else:
            y = dm.denoise_3d(x, patch_size, padding)
        if verbose:
            print(f'# [{volume_num}/{total_volumes}] 100%', file=sys.stderr, end='\r')
            print(' ' * 100, file=sys.stderr, end='\r')
        if stored is not None:
            half, stored['lost'] = rt.encode(y, rt.ENC_F16, ctx=dm.ctx)
            stored['half'] = half.cpu().numpy()
        if torch.is_tensor(tomo) and tomo.is_cuda:                # (a volume decoded on the device: _tomogram_io)
            return y.cpu().numpy()
        return y.cpu().numpy().astype(np.asarray(tomo).dtype, copy=False)


# ---- pre-filters (denoise.py:22-75, 129-197) ------------------------------------------------------------------------------
DECONV_WIDTH = 11


@functools.lru_cache(maxsize=16)
def lowpass_operator(n: int, factor: float, rfft: bool = False) -> np.ndarray:
    """Q [n, r] float64 with Q Q^T the projection of lowpass(x, factor) along one axis of length n: orthonormal columns
    1/sqrt(n), sqrt(2/n) cos(2 pi k j / n), sqrt(2/n) sin(2 pi k j / n) for every kept frequency k >= 1.  The kept set comes from
    the reference's own expressions (denoise.py:178-189): fftfreq along the rows, rfftfreq along the last axis, a bin is zeroed
    when |freq| > 0.5 / factor.  For factor > 1 the set is symmetric and misses the Nyquist bin, so the filter is real and
    separable, y = P_H x P_W.  Cached (read-only): the device upload reads it asynchronously."""
    if not factor > 1:
        raise ValueError(f'lowpass factor {factor}: only factors > 1 filter (denoise.py:386)')
    freq = np.fft.rfftfreq(n) if rfft else np.fft.fftfreq(n)
    keep = ~(np.abs(freq) > 0.5 / factor)
    half = (n - 1) // 2                                    # positive frequencies below Nyquist
    ks = [k for k in range(1, half + 1) if keep[k]]
    assert keep[0] and (n % 2 or not keep[n // 2])
    assert rfft or all(keep[n - k] == keep[k] for k in range(1, half + 1))
    j = np.arange(n, dtype=np.int64)
    q = np.empty((n, 1 + 2 * len(ks)), dtype=np.float64)
    q[:, 0] = 1.0 / np.sqrt(n)
    if ks:
        t = (2 * np.pi / n) * (np.outer(j, np.asarray(ks, dtype=np.int64)) % n)   # exact phase reduction
        q[:, 1::2] = np.sqrt(2.0 / n) * np.cos(t)
        q[:, 2::2] = np.sqrt(2.0 / n) * np.sin(t)
    q.flags.writeable = False
    return q


def _device_ctx():
    return rt.get_context()


def _like(y: torch.Tensor, x):
    """the device result in the form the input came in: numpy (x's dtype), a host tensor, or the device tensor itself"""
    if isinstance(x, np.ndarray):
        return y.cpu().numpy().astype(x.dtype, copy=False)
    if isinstance(x, torch.Tensor) and x.device.type == 'cpu':
        return y.cpu()
    return y


def lowpass(x, factor=1, dims=2):
    """hard low-pass of a 2-D image (denoise.py:174-197): every rfftn bin with |fftfreq| > 0.5 / factor along the rows or
    |rfftfreq| > 0.5 / factor along the columns is zeroed, evaluated as the exact fp64 projection P_H x P_W on the device and
    rounded to float32 once.  numpy or tensor in, the same form out.  factor <= 1 returns x unchanged (the caller's
    `lowpass > 1` test, denoise.py:386)."""
    if dims != 2 or np.ndim(x) != 2:
        raise NotImplementedError('lowpass: only the 2-D filter is implemented (nothing calls the 3-D form)')
    if not factor > 1:
        return x
    H, W = x.shape
    y = rt.lowpass_2d(rt.as_device_f32(x, _device_ctx()), lowpass_operator(H, float(factor)),
                      lowpass_operator(W, float(factor), rfft=True))
    return _like(y, x)


_lowpass = lowpass          # denoise_image's parameter of the same name shadows the function (the reference's crash)


def deconv_tiles(H: int, W: int, patch: int = 1, width: int = DECONV_WIDTH):
    """(N, M, halo'd tile rows, halo'd tile columns) of correct_spatial_covariance (denoise.py:135-158): N / M the tile
    heights / widths (the first H % patch / W % patch one longer), each halo'd span (start, length) clipped at the image.
    patch <= 1 is the whole image.  Raises ValueError when a halo'd tile is smaller than the filter (the reference fails inside
    conv2d)."""
    P = max(1, int(patch))
    p = width // 2
    spans = []
    for n in (H, W):
        q, r = divmod(n, P)
        sizes = [q + (1 if t < r else 0) for t in range(P)]
        starts = [sum(sizes[:t]) for t in range(P)]
        spans.append((sizes, [(max(0, a - p), min(n, a + m + p) - max(0, a - p)) for a, m in zip(starts, sizes)]))
    (N, ry), (M, rx) = spans
    h, w = min(s[1] for s in ry), min(s[1] for s in rx)
    if h < width or w < width:
        raise ValueError(f'--deconvolve: a {H} x {W} image in {P} x {P} patches (--deconv-patch {P}) has a {h} x {w} tile '
                         f'(halo included), smaller than the {width} x {width} filter')
    return N, M, ry, rx


def unblur_filter(cov: np.ndarray) -> np.ndarray:
    """w_inv of estimate_unblur_filter (denoise.py:61-73) in float64 from the lag covariances cov [width, width]: the power
    spectrum Re fft2(ifftshift(cov)), non-positive bins and the DC bin set to 1, then fftshift(ifft2(ps^-1/2)).real"""
    ps = np.fft.fft2(np.fft.ifftshift(np.asarray(cov, dtype=np.float64))).real
    ps = np.where(ps <= 0, 1.0, ps)
    ps[0, 0] = 1.0
    return np.fft.fftshift(np.fft.ifft2(1.0 / np.sqrt(ps))).real


def spatial_covariance(x, n=DECONV_WIDTH, s=11) -> np.ndarray:
    """the n x n lag covariances of a 2-D image (denoise.py:22-49), float64 from fp64 sums on the device"""
    return rt.spatial_cov_2d(rt.as_device_f32(x, _device_ctx()), 1, n)[0]


def estimate_unblur_filter(x, width=DECONV_WIDTH, s=11):
    """(AffineFilter(w_inv), cov) of denoise.py:52-75; cov float64"""
    cov = spatial_covariance(x, n=width, s=s)
    return AffineFilter(unblur_filter(cov)), cov


def correct_spatial_covariance(x, width=DECONV_WIDTH, s=11, patch=1):
    """denoise.py:129-172 called as intended (on a tensor): each of the patch x patch tiles (halo width // 2) is filtered with
    the fp32-rounded unblurring filter of its own covariances.  Three launches whatever the patch count: the covariances of
    all tiles, then one zero-padded filter over the whole image with each pixel's tile weights (equal to filtering each halo'd
    tile and keeping its centre).  numpy or tensor in, the same form out (float32)."""
    if np.ndim(x) != 2:
        raise NotImplementedError('correct_spatial_covariance: only 2-D images')
    H, W = x.shape
    P = max(1, int(patch))
    deconv_tiles(H, W, P, width)
    xd = rt.as_device_f32(x, _device_ctx())
    cov = rt.spatial_cov_2d(xd, P, width)
    w = np.stack([unblur_filter(c) for c in cov]).astype(np.float32)
    y = rt.tile_filter_2d(xd, w, P)
    return y.cpu().numpy() if isinstance(x, np.ndarray) else _like(y, x)


def denoise_image(mic: np.ndarray, models: List[Denoise], lowpass=1, cutoff=0, gaus: GaussianDenoise = None,
                  inv_gaus: InvGaussianFilter = None, deconvolve=False, deconv_patch=1, patch_size=-1, padding=0,
                  normalize=False, use_cuda=True) -> np.ndarray:
    """denoise_image (denoise.py:382-416).  numpy mean / POPULATION std here (unlike _denoise).  The pre-filters run as
    evidently intended: lowpass on the raw micrograph, deconvolution on the normalised one."""
    mic = np.asarray(mic)
    if deconvolve and gaus is None and inv_gaus is None:
        deconv_tiles(*mic.shape, deconv_patch)              # refused before anything runs
    if lowpass > 1:
        mic = _lowpass(mic, lowpass)
    mu, std = mic.mean(), mic.std()
    x = (mic - mu) / std
    if cutoff > 0:
        x[(x < -cutoff) | (x > cutoff)] = 0
    if gaus is not None:
        x = gaus.apply(x)
    elif inv_gaus is not None:
        x = inv_gaus.apply(x)
    elif deconvolve:
        x = correct_spatial_covariance(x, patch=deconv_patch)
    if len(models) == 0:
        # `-m none` (commands/denoise.py:100-106 still builds a Denoise around no model): the pre-filtered image passes through
        out = np.asarray(x, dtype=np.float32)
    else:
        out = sum(model.denoise(x, patch_size=patch_size, padding=padding) for model in models) / len(models)
    if normalize:
        out = (out - out.mean()) / out.std()
    else:
        out = std * out + mu
    return out


def denoise_image_device(x: torch.Tensor, models: List[Denoise], patch_size: int = -1, padding: int = 0,
                         normalize: bool = False, lowpass: float = 1, deconvolve: bool = False,
                         deconv_patch: int = 1, cutoff: float = 0, gaus: GaussianDenoise = None,
                         inv_gaus: InvGaussianFilter = None) -> torch.Tensor:
    """denoise_image (denoise.py:382-416) with the micrograph staying on the device: population mean / std (the reference's
    numpy statistics, here a deterministic fp64 reduction on the GPU), (x - mu) / std, the networks' average, then either
    re-normalisation or std * y + mu.  The CLI path spends no host pass over the 16.7 M pixels this way (the host passes of the
    numpy version measured in DESIGN.md §14).  The options in the reference's order (:386-414): lowpass > 1 filters the raw
    micrograph; cutoff > 0 zeroes the normalised pixels beyond +-cutoff in the normalisation launch itself
    (tpz_normalize_cutoff); then exactly one filter of the normalised image -- gaus before inv_gaus before deconvolve, the
    reference's if / elif / elif -- on the device tensor; with no model the pre-filtered image passes through (`-m none`)."""
    from . import runtime as rt
    deconvolve = bool(deconvolve) and gaus is None and inv_gaus is None       # (the branch that runs)
    if deconvolve:
        deconv_tiles(*x.shape, deconv_patch)                # refused before anything runs
    if lowpass > 1:
        x = _lowpass(x, lowpass)
    mu, std = rt.mean_std(x, unbiased=False)
    # (x - mu) / std as numpy rounds it; std == 0 -> inf / nan like upstream
    xn = rt.normalize_cutoff(x, mu, std, cutoff) if cutoff > 0 else rt.normalize(x, mu, std)
    if gaus is not None:
        xn = gaus(xn)
    elif inv_gaus is not None:
        xn = inv_gaus(xn)
    elif deconvolve:
        xn = correct_spatial_covariance(xn, patch=deconv_patch)
    out = None if models else xn
    for model in models:
        y = model.denoise_device(xn, patch_size, padding)
        out = y if out is None else out + y
    if len(models) > 1:
        out = out / len(models)
    if normalize:
        m2, s2 = rt.mean_std(out, unbiased=False)
        return rt.normalize(out, m2, s2)
    return rt.affine(out, std, mu)


# ---- file-level drivers -----------------------------------------------------------------------------------------------
# Counterparts of denoise_stack (denoise.py:419-447), denoise_stream (:450-490), denoise_tomogram (:495-530) and
# denoise_tomogram_stream (:533-557): same arguments, same files on disk.  Structure here: a Job names one input and its
# output path; `_run_jobs` overlaps the disk read of job i+1 and the write of job i-1 with the GPU work of job i (one
# reader and one writer thread around the device loop) and shards the jobs over the ranks when launched multi-process.
class _Job:
    __slots__ = ('index', 'src', 'dst')

    def __init__(self, index: int, src: str, dst: str):
        self.index, self.src, self.dst = index, src, dst


def _output_path(src: str, outdir: Optional[str], suffix: str, ext: str) -> str:
    """<outdir>/<name><suffix><ext>, or next to the input with '.denoised' when no directory is given
    (denoise.py:476-483, 512-520)"""
    stem, _ = os.path.splitext(src)
    if not outdir:
        return stem + (suffix or '.denoised') + ext
    return os.path.join(outdir, os.path.basename(stem) + suffix + ext)


def _run_jobs(jobs: List[_Job], read, process, write, progress) -> list:
    """read(job) -> item; process(job, item) -> result; write(job, item, result).  Reads run one job ahead and writes one
    job behind the processing, each on its own thread; exceptions of either surface here."""
    from concurrent.futures import ThreadPoolExecutor
    results = []
    if not jobs:
        return results
    with ThreadPoolExecutor(1, 'tpz-read') as reader, ThreadPoolExecutor(1, 'tpz-write') as writer:
        nxt = reader.submit(read, jobs[0])
        pending = None
        for n, job in enumerate(jobs):
            item = nxt.result()
            if n + 1 < len(jobs):
                nxt = reader.submit(read, jobs[n + 1])
            result = process(job, item)
            if pending is not None:
                pending.result()
            pending = writer.submit(write, job, item, result)
            results.append(result)
            progress(n + 1)
        if pending is not None:
            pending.result()
    return results


def denoise_stack(path: str, output_path: str, models: List[Denoise], lowpass: float = 1, pixel_cutoff: float = 0,
                  gaus=None, inv_gaus=None, deconvolve: bool = True, deconv_patch: int = 1, patch_size: int = 1024,
                  padding: int = 500, normalize: bool = True, use_cuda: bool = True):
    """the reference's signature (denoise.py:419-447) around denoise_stack_stored: a float32 output stack"""
    return denoise_stack_stored(path, output_path, models, lowpass, pixel_cutoff, gaus, inv_gaus, deconvolve, deconv_patch,
                                patch_size, padding, normalize, use_cuda, float16=False)


def denoise_stack_stored(path: str, output_path: str, models: List[Denoise], lowpass: float = 1, pixel_cutoff: float = 0,
                         gaus=None, inv_gaus=None, deconvolve: bool = True, deconv_patch: int = 1, patch_size: int = 1024,
                         padding: int = 500, normalize: bool = True, use_cuda: bool = True, *, float16: bool = False):
    """every section of one MRC stack, written back as one stack with the input's header.  On the device (runs_on_device) the
    sections go through the ring of denoise_stream, each with its own statistics, and rank r of a multi-process launch takes
    sections r, r + world, ... -- all ranks write the one output file (_denoise_stack_device); otherwise the host loop.
    float16: the output stack is stored as float16 (MRC mode 12)."""
    from . import mrc
    with open(path, 'rb') as f:
        stack, header, extended_header = mrc.parse(f.read())
    print('# denoising stack with shape:', stack.shape, file=sys.stderr)
    models = models or []
    if stack.dtype.kind in 'iuf' and runs_on_device(models, lowpass, pixel_cutoff, gaus, inv_gaus, deconvolve):
        return _denoise_stack_device(stack, header, extended_header, output_path, models, patch_size, padding, normalize,
                                     float16=float16, lowpass=lowpass, deconvolve=deconvolve, deconv_patch=deconv_patch,
                                     cutoff=pixel_cutoff, gaus=gaus, inv_gaus=inv_gaus)
    out = np.zeros_like(stack)
    for k, section in enumerate(stack):
        out[k] = denoise_image(section, models, lowpass=lowpass, cutoff=pixel_cutoff, gaus=gaus, inv_gaus=inv_gaus,
                               deconvolve=deconvolve, deconv_patch=deconv_patch, patch_size=patch_size, padding=padding,
                               normalize=normalize, use_cuda=use_cuda)
        print(f'# {k + 1} of {len(stack)} completed.', file=sys.stderr, end='\r')
    print('', file=sys.stderr)
    print('# writing to', output_path, file=sys.stderr)
    with open(output_path, 'wb') as f:
        if float16:
            mrc.write(f, streaming.as_float16(out, output_path), header=header, extended_header=extended_header, dtype=np.float16)
        else:
            mrc.write(f, out, header=header, extended_header=extended_header)
    return out


def denoise_stream(micrographs: List[str], output_path: str, format: str = 'mrc', suffix: str = '',
                   models: List[Denoise] = None, lowpass: float = 1, pixel_cutoff: float = 0, gaus=None, inv_gaus=None,
                   deconvolve: bool = True, deconv_patch: int = 1, patch_size: int = 1024, padding: int = 500,
                   normalize: bool = True, use_cuda: bool = True, return_images: bool = True, float16: bool = False):
    """one output image per micrograph; rank r of a multi-process launch takes micrographs r, r + world, ...
    float16 (format 'mrc' only): the files are stored as float16 (MRC mode 12), encoded on the device.
    Returns the denoised micrographs like the reference (denoise.py:450-490 keeps every one of them in memory);
    return_images=False (the CLI, which ignores them) returns the output paths instead."""
    from . import mrc, parallel
    from .utils.image import load_image, save_image
    mrc.check_float16_formats(float16, [format])
    rank, _, world = parallel.init_from_env()
    if output_path:
        os.makedirs(output_path, exist_ok=True)
    jobs = [_Job(i, micrographs[i], _output_path(micrographs[i], output_path, suffix, '.' + format))
            for i in parallel.shard_indices(len(micrographs), rank, world)]

    models = models or []
    # every pass over the pixels on the device, whatever the options; a 3-D model, or `-m none` without a pre-filter (a
    # pass-through), keeps the host loop
    if runs_on_device(models, lowpass, pixel_cutoff, gaus, inv_gaus, deconvolve):
        return _denoise_stream_device(jobs, models, patch_size, padding, normalize, len(micrographs), return_images,
                                      float16=float16, lowpass=lowpass, deconvolve=deconvolve, deconv_patch=deconv_patch, cutoff=pixel_cutoff,
                                      gaus=gaus, inv_gaus=inv_gaus)

    def read(job):
        loaded = load_image(job.src, make_image=False)
        return loaded if isinstance(loaded, tuple) else (loaded, None, None)

    def process(job, item):
        return denoise_image(item[0], models, lowpass=lowpass, cutoff=pixel_cutoff, gaus=gaus, inv_gaus=inv_gaus,
                             deconvolve=deconvolve, deconv_patch=deconv_patch, patch_size=patch_size, padding=padding,
                             normalize=normalize, use_cuda=use_cuda)

    def write(job, item, mic):
        save_image(streaming.as_float16(mic, job.dst) if float16 else mic, job.dst, header=item[1], extended_header=item[2])

    total = len(micrographs)
    out = _run_jobs(jobs, read, process, write, lambda n: print(f'# {n} of {total} completed.', file=sys.stderr, end='\r'))
    print('', file=sys.stderr)
    return out


def runs_on_device(models, lowpass: float = 1, pixel_cutoff: float = 0, gaus=None, inv_gaus=None,
                   deconvolve: bool = False) -> bool:
    """whether denoise_stream / denoise_stack keep the images on the device: every model is 2-D and there is something to do --
    a model, or any pre-filter.  A 3-D model, or `-m none` with no filter (a pass-through), takes the host loop."""
    return all(m.dims == 2 for m in models) and bool(len(models) > 0 or lowpass > 1 or deconvolve or pixel_cutoff > 0 or
                                                     gaus is not None or inv_gaus is not None)


# sections of a stack below this many bytes run one by one on the calling thread instead of through the ring
RING_MIN_BYTES = 1 << 20


def stack_section_offset(k: int, ny: int, nx: int, extended_bytes: int, itemsize: int = 4) -> int:
    """byte of section k in an MRC stack as mrc.write lays it out: the 1024-byte header, the extended header, sections of float32
    pixels (itemsize 4) or, under --float16, of float16 pixels (itemsize 2)"""
    return 1024 + extended_bytes + itemsize * k * ny * nx


def _denoise_stream_device(jobs: List[_Job], models: List[Denoise], patch_size: int, padding: int, normalize: bool, total: int,
                           return_images: bool = False, float16: bool = False, **options) -> list:
    """the `topaz denoise` loop with every pass over the pixels on the device (_device_ring); options: the keyword arguments of
    denoise_image_device (lowpass, deconvolve, deconv_patch, cutoff, gaus, inv_gaus).  The result leaves the device in the type
    its file stores: float16 under `float16`, the uint8 of save_image's quantize for a PNG / JPEG file nobody asked back as an
    image, float32 otherwise."""
    from .stats import EIGHT_BIT_FORMATS
    from .utils.image import save_image
    results = [job.dst for job in jobs]
    eight_bit = bool(jobs) and os.path.splitext(jobs[0].dst)[1][1:] in EIGHT_BIT_FORMATS and not return_images
    encode = rt.ENC_F16 if float16 else (rt.ENC_U8, (-3, 3)) if eight_bit else None

    def emit(host, n, path, header, extended):
        save_image(host, jobs[n].dst, header=header, extended_header=extended)
        if return_images:
            results[n] = np.array(host, dtype=np.float32)

    _device_ring([job.src for job in jobs], models, lambda x: denoise_image_device(x, models, patch_size, padding, normalize,
                                                                                   **options), emit, total, encode,
                 lambda lost, n, *_: streaming.warn_overflow(jobs[n].dst, lost))
    return results


def _denoise_stack_device(stack: np.ndarray, header, extended_header, output_path: str, models: List[Denoise], patch_size: int,
                          padding: int, normalize: bool, float16: bool = False, **options) -> np.ndarray:
    """`topaz denoise --stack` through the ring of the stream: section k+1 uploads and section k-1 leaves under the kernels of
    section k, each section with its own statistics (sections below RING_MIN_BYTES run one by one on the calling thread
    instead, through the same functions).  The writer thread casts a section to the stack's dtype (what the host
    loop's np.zeros_like(stack) does to an integer stack) and puts its float32 form at its byte of the output file (os.pwrite).
    Rank r of a multi-process launch takes sections r, r + world, ...; rank 0 lays down the header, and a barrier makes the file
    whole before any rank returns.  Returns the full stack (one process) or this rank's sections in a zero array.
    float16: the header says mode 12 and a section takes 2 bytes per pixel; a section of a float stack is encoded on the device
    (an integer stack's is truncated on the host first, as ever, and converted there)."""
    from . import mrc, parallel
    rank, local_rank, world = parallel.init_from_env()
    extended_header = extended_header or b''
    sections = stack if stack.ndim == 3 else stack[None]          # (mrc.parse squeezes a one-section stack)
    nz, ny, nx = sections.shape
    mine = parallel.shard_indices(nz, rank, world)
    out = np.zeros_like(sections)
    itemsize, stored = (2, np.float16) if float16 else (4, np.float32)
    encode = rt.ENC_F16 if float16 and stack.dtype.kind == 'f' else None
    print(f'# rank {rank} of {world}: stack sections {mine} of {nz}, writing to {output_path}', file=sys.stderr, flush=True)
    fd = os.open(output_path, os.O_WRONLY | os.O_CREAT, 0o666)     # every rank opens the one file, none empties it
    try:
        if rank == 0:
            # (the header mrc.write gives a stack written with the input's header; the length fixed up front cuts off what a
            # longer file of an earlier run would leave behind)
            os.pwrite(fd, mrc.header_struct.pack(*list(header._replace(mode=mrc.get_mode_for_header(stored)))) + extended_header, 0)
            os.ftruncate(fd, stack_section_offset(nz, ny, nx, len(extended_header), itemsize))

        def overflowed(lost, n, k, *_):
            streaming.warn_overflow(f'{output_path} section {k}', lost)

        def emit(host, n, k, _header, _extended):
            out[k] = host                                       # the cast to the stack's dtype (truncation for integers)
            if encode is None:                                  # (an encoded section is written as it came down)
                host = streaming.as_float16(out[k], f'{output_path} section {k}') if float16 else \
                    np.ascontiguousarray(out[k], dtype=np.float32)
            streaming.pwrite_all(fd, host, stack_section_offset(k, ny, nx, len(extended_header), itemsize))

        def process(x):
            return denoise_image_device(x, models, patch_size, padding, normalize, **options)

        if 4 * ny * nx >= RING_MIN_BYTES:
            _device_ring([(k, sections[k], None, None) for k in mine], models, process, emit, nz, encode, overflowed)
        else:
            # small sections: the copies the ring would hide are shorter than its hand-offs between threads
            ctx = models[0].model.device_model.ctx if models else rt.get_context()
            for n, k in enumerate(mine):
                y = process(rt.as_device_f32(np.array(sections[k], dtype=np.float32), ctx))
                if encode is not None:
                    y, lost = rt.encode(y, encode, ctx=ctx)
                    if lost:
                        overflowed(lost, n, k)
                emit(y.cpu().numpy(), n, k, None, None)
                print(f'# {n + 1} of {nz} completed.', file=sys.stderr, end='\r')
            print('', file=sys.stderr)
    finally:
        os.close(fd)
    if world > 1:
        parallel.barrier(parallel.collective_device(local_rank))   # every rank's sections are in the file
    return out.reshape(stack.shape)


def _device_ring(items: list, models: List[Denoise], process, emit, total: int, encode=None, on_overflow=None) -> None:
    """The device-resident loop shared by the stream and the stack (streaming.stream_images).  items: file paths, or (key, array,
    header, extended header) for images already in memory.  The GPU runs process(device tensor) -> device tensor on image i
    while image i+1 is decoded and uploaded, and a writer thread calls emit(pinned host array, i, path or key, header, extended
    header) for image i-1.  encode: the type the results leave the device in (streaming.ResultRing.put), on_overflow(count, i,
    path or key, header, extended header): the ring's hook."""
    if not items:
        return
    ctx = models[0].model.device_model.ctx if models else rt.get_context()
    count = itertools.count()

    def step(key, x, header, extended):
        n, y = next(count), process(x)
        print(f'# {n + 1} of {total} completed.', file=sys.stderr, end='\r')
        return streaming.Put(y, (n, key, header, extended), encode)

    streaming.stream_images(items, ctx, step, emit, on_overflow=on_overflow)
    print('', file=sys.stderr)


def _tomogram_io(float16: bool = False):
    from . import mrc

    def read(job):
        # an int8 / int16 / uint16 / float16 volume stays in its stored type (one read INTO the array, no host pass over the
        # voxels): _tomogram_device sends it up as stored and tpz_decode makes the float32 volume there
        got = mrc.read_stored_into(job.src, lambda shape, dtype: np.empty(shape, dtype=dtype))
        if got is not None:
            return got
        with open(job.src, 'rb') as f:
            tomo, header, extended = mrc.parse(f.read())
        return tomo.astype(np.float32), header, extended

    def write(job, item, denoised, stored=None):
        # 3-D denoise refreshes the density statistics of the header (denoise.py:523-526); under float16 they stay those of the
        # float32 volume, whose float16 form (Denoise3D.denoise's `stored`) is what the file holds
        header = item[1]._replace(mode=2, amin=denoised.min(), amax=denoised.max(), amean=denoised.mean())
        with open(job.dst, 'wb') as f:
            if float16:
                if stored['lost']:
                    streaming.warn_overflow(job.dst, stored['lost'])
                mrc.write(f, stored['half'], header=header, extended_header=item[2], dtype=np.float16)
            else:
                mrc.write(f, denoised, header=header, extended_header=item[2])
    return read, write


def _tomogram_device(model: 'Denoise3D', tomo: np.ndarray, pool) -> tuple:
    """(what Denoise3D.denoise takes, the float32 volume the drivers return) for a volume as _tomogram_io read it.  A stored
    type is decoded on the device (runtime.decode_stored); the float32 host copy callers of the drivers have always been handed
    is made by a thread of `pool` under the denoising -- a future, resolved when the driver returns."""
    from . import mrc
    if tomo.dtype not in mrc.STORED_MODES:
        return tomo, tomo
    return rt.decode_stored(tomo, model.model.device_model.ctx), pool.submit(tomo.astype, np.float32)


def _resolved(volume):
    return volume if isinstance(volume, np.ndarray) else volume.result()


def denoise_tomogram(path: str, model: Denoise3D, outdir: str = None, suffix: str = '', patch_size: int = 96,
                     padding: int = 48, volume_num: int = 1, total_volumes: int = 1, gaus=None, verbose: bool = True,
                     float16: bool = False):
    """one tomogram; returns the INPUT volume, Gaussian-filtered when `gaus` is given -- what the reference returns
    (it filters `tomo`, writes `denoised`: denoise.py:509,528-530)"""
    read, write = _tomogram_io(float16)
    stored = {} if float16 else None
    job = _Job(0, path, _output_path(path, outdir, suffix, os.path.splitext(path)[1]))
    from concurrent.futures import ThreadPoolExecutor
    item = read(job)
    with ThreadPoolExecutor(1, 'tpz-f32') as pool:
        x, volume = _tomogram_device(model, item[0], pool)
        denoised = model.denoise(x, patch_size=patch_size, padding=padding, batch_size=1, volume_num=volume_num,
                                 total_volumes=total_volumes, verbose=verbose, stored=stored)
        del x
        write(job, item, denoised, stored)
        volume = _resolved(volume)
    return gaus.apply(volume) if gaus is not None else volume


def denoise_tomogram_stream(volumes: List[str], model: Denoise3D, output_path: str, suffix: str = '', gaus: float = None,
                            patch_size: int = 96, padding: int = 48, verbose: bool = True, use_cuda: bool = True,
                            float16: bool = False):
    """tomograms (or, when there are fewer tomograms than ranks, their tiles) sharded over the ranks of a multi-process
    launch; the next volume is read while this one is denoised"""
    from . import parallel
    if gaus is not None and gaus > 0:
        # upstream builds a TWO-dimensional GaussianDenoise here (denoise.py:546, dims defaults to 2) and applies it to
        # the input volume before anything is written (:509): Conv2d rejects the 5-D tensor, so `--gaussian` > 0 has
        # only ever raised.  Same outcome, said plainly.  (denoise_tomogram(gaus=GaussianDenoise(s, dims=3)) works.)
        raise RuntimeError('denoise3d --gaussian: the 2-D Gaussian module cannot filter a volume (upstream fails in '
                           'Conv2d at this point); use 0')
    rank, _, world = parallel.init_from_env()
    if output_path:
        os.makedirs(output_path, exist_ok=True)
    read, write_volume = _tomogram_io(float16)
    total = len(volumes)
    # fewer tomograms than ranks: split each tomogram's TILES over all ranks instead of leaving ranks idle (a 512x512x256
    # volume is 108 independent 192^3 tiles); otherwise whole tomograms are dealt to the ranks
    by_tiles = world > 1 and total < world and patch_size >= 1
    mine = range(total) if by_tiles else parallel.shard_indices(total, rank, world)
    jobs = [_Job(i, volumes[i], _output_path(volumes[i], output_path, suffix, os.path.splitext(volumes[i])[1])) for i in mine]
    inputs = []          # upstream returns the list of (unfiltered) input volumes; kept for the same return value

    from concurrent.futures import ThreadPoolExecutor
    pool = ThreadPoolExecutor(1, 'tpz-f32')

    def process(job, item):
        x, volume = _tomogram_device(model, item[0], pool)
        inputs.append(volume)
        stored = {} if float16 else None
        return model.denoise(x, patch_size=patch_size, padding=padding, batch_size=1, volume_num=job.index + 1,
                             total_volumes=total, verbose=verbose and rank == 0, across_ranks=by_tiles, stored=stored), stored

    def write(job, item, result):                  # (sharded by tiles, only rank 0 holds the assembled volume)
        if result[0] is not None:
            write_volume(job, item, *result)

    try:
        _run_jobs(jobs, read, process, write, lambda n: print(f'# {n} of {total} tomograms denoised.', file=sys.stderr, end='\r'))
        inputs = [_resolved(v) for v in inputs]
    finally:
        pool.shutdown()
    print('', file=sys.stderr)
    return inputs
