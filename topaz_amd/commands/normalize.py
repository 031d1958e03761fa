"""`topaz normalize`: 2-component Gaussian-mixture (or affine) normalisation of a set of images, the mixture fit
on the MI355X (flag surface: _spec.NORMALIZE, mirroring topaz/commands/normalize.py:16-45).  The files stream through the device
(stats.normalize_images); `--gpus N` shards them over N rank processes, rank r taking files r, r + N, ..."""

name = 'normalize'
help = 'scale images to zero mean / unit variance of the background component of a 2-Gaussian pixel mixture'


def add_arguments(parser=None):
    from ._spec import NORMALIZE, build_parser
    return build_parser(NORMALIZE, help, parser)


def main(args):
    from .. import parallel
    from ..cuda import set_device
    from ..stats import normalize_images
    from ..mrc import check_float16_formats
    float16 = getattr(args, 'float16', False)
    check_float16_formats(float16, args.format_.split(','))         # (before a device is touched or a file read)
    _, local_rank, world = parallel.init_from_env()
    set_device(parallel.rank_device(local_rank) if world > 1 else args.device)
    normalize_images(args.files, args.destdir, 0, args.scale, args.affine, args.niters, args.alpha, args.beta,
                     args.sample, args.metadata, args.format_.split(','), True, args.verbose, float16=float16)


if __name__ == '__main__':
    main(add_arguments().parse_args())
