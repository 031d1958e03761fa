"""`topaz segment` -- topaz/commands/segment.py:16-56 + segment_images (model/utils.py:71-105), as a device-resident stream
(DESIGN.md §17): the feed reads file i+1 in the type it stores while file i is scored, the map of file i-1 leaves through the
pinned result ring under a writer thread, and with `--gpus N` rank r takes files r, r + N, ..."""
import os

import numpy as np
import torch

from .. import parallel, streaming

name = 'segment'
help = 'write per-pixel score maps of a trained classifier'

FORMATS = ('tiff', 'mrc', 'npy')


def add_arguments(parser=None):
    from ._spec import SEGMENT, build_parser
    return build_parser(SEGMENT, help, parser)


class MapSink:
    """where score maps go: <destdir>/<micrograph name>.tiff (float32, 2-D) or .npy (volumes) -- model/utils.py:96-105 -- unless
    `fmt` names one of FORMATS for all of them; an .mrc map carries the header handed to write()"""

    def __init__(self, destdir: str, verbose: bool, fmt=None):
        if fmt is not None and fmt not in FORMATS:
            raise ValueError(f'score maps are written as {", ".join(FORMATS)}, not {fmt}')
        os.makedirs(destdir, exist_ok=True)
        self.destdir, self.verbose, self.fmt = destdir, verbose, fmt

    def path_of(self, source_path: str, ndim: int) -> str:
        stem = os.path.join(self.destdir, os.path.splitext(os.path.basename(source_path))[0])
        return stem + '.' + (self.fmt or ('npy' if ndim == 3 else 'tiff'))

    def write(self, source_path: str, scores: np.ndarray, header=None, extended=None) -> str:
        """scores: float32 -- or, for an .mrc map, float16, stored as it is (mode 12)"""
        path = self.path_of(source_path, scores.ndim)
        if self.verbose:
            print('# saving:', os.path.splitext(path)[0])
        if path.endswith('.npy'):
            np.save(path, scores)
        elif path.endswith('.mrc'):
            from .. import mrc
            if header is not None:
                nz, ny, nx = scores.shape if scores.ndim == 3 else (1,) + scores.shape
                header = header._replace(nz=nz, ny=ny, nx=nx)
            with open(path, 'wb') as f:
                mrc.write(f, scores if scores.ndim == 3 else scores[np.newaxis], header=header,
                          extended_header=(extended or b'') if header is not None else b'',
                          dtype=np.float16 if scores.dtype == np.float16 else np.float32)
        elif scores.ndim == 3:
            raise ValueError(f'{source_path}: a volume is written as npy or mrc, not tiff')
        else:
            from PIL import Image
            Image.fromarray(np.ascontiguousarray(scores, dtype=np.float32)).save(path, 'tiff')
        return path


def score_map_device(model, x: torch.Tensor, patch_size=None) -> torch.Tensor:
    """per-pixel (per-voxel) logits of one micrograph / tomogram on the device, float32: the filled model over the whole tensor or,
    with `patch_size`, over tiles of twice that size that overlap by the receptive field (the evident intent of
    model/utils.py:88-90, which passes predict_in_patches a keyword it does not take and crashes upstream -- SURVEY 3.1)"""
    if patch_size is not None:
        from ..model.utils import predict_in_patches_device
        return predict_in_patches_device(model, x, 2 * patch_size, is_3d=(x.dim() == 3))
    with torch.no_grad():
        return model(x[None, None])[0, 0]


def score_map(model, pixels: np.ndarray, patch_size=None) -> np.ndarray:
    """score_map_device of a host array, back on the host: float32, or the float64 of predict_in_patches with `patch_size`"""
    if patch_size is not None:
        from ..model.utils import predict_in_patches
        x = torch.as_tensor(np.ascontiguousarray(pixels), dtype=torch.float32)[None, None]
        return predict_in_patches(model, x, patch_size=2 * patch_size, is_3d=(pixels.ndim == 3), use_cuda=True)[0, 0]
    x = torch.as_tensor(np.ascontiguousarray(pixels), dtype=torch.float32)
    return score_map_device(model, x.cuda()).cpu().numpy()


def is_volume(path: str) -> bool:
    """an MRC file of more than one section, by its header (nothing else of the file is read)"""
    if os.path.splitext(path)[1] != '.mrc':
        return False
    from .. import mrc
    with open(path, 'rb') as f:
        return mrc.parse_header(f.read(1024)).nz > 1


def check_segment_args(paths, preprocess=0, fmt=None, float16=False, model='resnet16') -> None:
    """what `segment` refuses, before a GPU, a model or an image is touched: an unknown --format, --float16 with anything but
    --format mrc, a negative --preprocess, --preprocess on a volume (ValueError)"""
    from ..extract import check_preprocess_args
    from ..mrc import check_float16_formats
    if fmt is not None and fmt not in FORMATS:
        raise ValueError(f'--format is one of {", ".join(FORMATS)}, not {fmt}')
    if float16:
        check_float16_formats(True, [fmt or 'the default (tiff / npy)'])
    if preprocess < 0:
        raise ValueError(f'--preprocess {preprocess}: a reduction factor >= 1, or 0 for off')
    if preprocess:
        for path in paths:
            check_preprocess_args(preprocess, model, 3 if is_volume(path) else 2)


def segment_images(model, paths, output_dir, use_cuda, verbose, patch_size=None, preprocess=None, fmt=None, float16=False):
    """topaz.model.utils.segment_images (model/utils.py:71-105): one score map file per input, streamed.  The rank of a
    multi-process launch (parallel.init_from_env) takes files rank, rank + world, ... and writes only those; the ranks exchange
    nothing.  preprocess: None, or a callable device tensor -> device tensor (stats.DevicePreprocess) every micrograph goes
    through before it is scored, here, in path order.  fmt: MapSink's; float16: an .mrc map is encoded to float16 on the copy
    stream on its way out."""
    if float16 and fmt != 'mrc':
        raise ValueError('--float16 stores MRC mode 12 and goes with --format mrc only')
    rank, _, world = parallel.init_from_env()
    mine = [paths[i] for i in parallel.shard_indices(len(paths), rank, world)]
    sink = MapSink(output_dir, verbose, fmt)
    if not mine:
        return

    def process(path, x, header, extended):
        if preprocess is not None:
            x = preprocess(x)
        return streaming.Put(score_map_device(model, x, patch_size), (path, header, extended),
                             streaming.rt.ENC_F16 if float16 else None)

    def write(scores, path, header, extended):
        sink.write(path, scores, header, extended)

    def overflowed(lost, path, header, extended):
        streaming.warn_overflow(sink.path_of(path, 2 if header is None or header.nz == 1 else 3), lost)

    streaming.stream_images(mine, model.device_model.ctx, process, write, on_overflow=overflowed)


def main(args):
    from ..cuda import set_device
    from ..model.factory import load_model
    from ..torch import set_num_threads
    scale = getattr(args, 'preprocess', 0)
    fmt, float16 = getattr(args, 'format', None), getattr(args, 'float16', False)
    check_segment_args(args.paths, scale, fmt, float16, args.model)          # (before a model or an image is read)
    if (args.patch_size is not None) and (args.patch_size <= 0):
        raise ValueError('patch size must be positive')
    set_num_threads(args.num_threads)
    _, local_rank, world = parallel.init_from_env()
    device = parallel.rank_device(local_rank) if world > 1 else args.device
    use_cuda = set_device(device)
    model = load_model(args.model)
    model.eval()
    model.fill()
    model.cuda(device)
    from ..precision import check_loaded_model
    check_loaded_model(model, getattr(args, 'precision_check', 'auto'), args.model, args.verbose)
    preprocess = None
    if scale:
        from ..stats import DevicePreprocess
        preprocess = DevicePreprocess(scale, args.preprocess_affine, args.preprocess_niters, args.preprocess_alpha,
                                      args.preprocess_beta, args.preprocess_sample)
    segment_images(model, args.paths, args.destdir, use_cuda, args.verbose, args.patch_size, preprocess, fmt, float16)


if __name__ == '__main__':
    main(add_arguments().parse_args())
