"""`topaz particle_stack`: an MRC particle stack and a RELION STAR file from a pick table, the boxes cut, standardised and
resized on the MI355X (flag surface: _spec.PARTICLE_STACK, mirroring topaz/commands/particle_stack.py:12-28)."""

name = 'particle_stack'
help = 'extract mrc particle stack given coordinates table'


def add_arguments(parser=None):
    from ._spec import PARTICLE_STACK, PARTICLE_STACK_RANKS, build_parser
    # the parser of the command alone is the reference's flag surface; under the `topaz` entry point, whose launcher starts the
    # rank processes, it also takes --gpus and --float16
    return build_parser(PARTICLE_STACK + (PARTICLE_STACK_RANKS if parser is not None else []), help, parser)


def main(args):
    from ..utils.picks import create_particle_stack
    create_particle_stack(args.file, args.output, args.threshold, args.size, args.resize, args.image_root, args.image_ext,
                          args.metadata, float16=getattr(args, 'float16', False))


if __name__ == '__main__':
    main(add_arguments().parse_args())
