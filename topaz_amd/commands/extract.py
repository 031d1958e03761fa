"""`topaz extract`: score micrographs, suppress non-maxima, write pick tables (flag surface: _spec.EXTRACT,
mirroring topaz/commands/extract.py:12-67)."""

from ..extract import extract_particles

name = 'extract'
help = 'score micrographs with a trained classifier and pick particles by non-maximum suppression'


def add_arguments(parser=None):
    from ._spec import EXTRACT, build_parser
    return build_parser(EXTRACT, help, parser)


def main(args):
    from ..extract import check_preprocess_args
    from ..torch import set_num_threads
    scale = getattr(args, 'preprocess', 0)
    if scale < 0:
        raise ValueError(f'--preprocess {scale}: a reduction factor >= 1, or 0 for off')
    check_preprocess_args(scale, args.model, args.dims)
    from ..utils.picks import check_particle_stack_args
    stack = dict(particle_stack=getattr(args, 'particle_stack', None), particle_size=getattr(args, 'particle_size', None),
                 particle_resize=getattr(args, 'particle_resize', -1),
                 particle_threshold=getattr(args, 'particle_threshold', -float('inf')),
                 particle_metadata=getattr(args, 'particle_metadata', None),
                 particle_float16=getattr(args, 'float16', False))
    if stack['particle_float16'] and not stack['particle_stack']:
        raise ValueError('--float16 is the stored type of the --particle-stack file: it needs --particle-stack')
    check_particle_stack_args(stack['particle_stack'], stack['particle_size'], stack['particle_resize'], args.model, args.dims,
                              args.targets, args.only_validate)
    preprocess = None
    if scale:
        from ..stats import DevicePreprocess
        preprocess = DevicePreprocess(scale, args.preprocess_affine, args.preprocess_niters, args.preprocess_alpha,
                                      args.preprocess_beta, args.preprocess_sample)
    set_num_threads(args.num_threads)
    extract_particles(args.paths, args.model, args.device, args.batch_size, args.threshold, args.radius, args.num_workers,
                      args.targets, args.min_radius, args.max_radius, args.step_radius, args.assignment_radius,
                      args.patch_size, args.only_validate, args.output, args.per_micrograph, args.suffix, args.format,
                      args.up_scale, args.down_scale, dims=args.dims, verbose=args.verbose,
                      precision_check=getattr(args, 'precision_check', 'auto'), preprocess=preprocess, **stack)


if __name__ == '__main__':
    main(add_arguments().parse_args())
