"""Flag tables of the hot-path commands.

The flag names, short options, types, defaults and choices are the drop-in surface of the reference CLI
(topaz/commands/{extract,denoise,denoise3d,segment,downsample,normalize,particle_stack}.py); they are kept as data here and the
parsers are generated from them.  Help texts are this project's own wording.  Flags that only make sense
for training are accepted (so existing command lines keep parsing) and rejected at run time.
"""
from __future__ import annotations

import argparse
from typing import Any, Dict, List, Sequence, Tuple

# (option strings, keyword arguments for add_argument)
Flag = Tuple[Sequence[str], Dict[str, Any]]

_GPUS: Flag = (('--gpus',), dict(type=int, default=0, help='start this many rank processes, one per MI355X, and shard the '
                                   'inputs over them (0: a single process, or all GPUs with -d -2)'))
_PRECISION: Flag = (('--precision-check',), dict(choices=['auto', 'always', 'never'], default='auto',
                                                help='measure the 2xf16 path of each loaded model against its fp32 result on one seeded '
                                                     'tile and run a model above 1e-4 on the fp32 kernels: auto checks model files '
                                                     '(user-trained), always the pretrained aliases too, never nothing'))
_FLOAT16: Flag = (('--float16',), dict(action='store_true',
                                      help='store the MRC output as float16 (MRC mode 12, what RELION writes with --float16): half '
                                           'the bytes, encoded on the GPU with the rounding of numpy\'s astype(float16); values '
                                           'beyond +-65504 become inf and are reported on stderr.  MRC output only'))
_THREADS: Flag = (('-j', '--num-threads'), dict(type=int, default=0, help='host threads for torch (0: library default, <0: all cores)'))

# the fit of `--preprocess` (extract, segment): the flags of `topaz preprocess` under a prefix
_PREPROCESS_FIT: List[Flag] = [
    (('--preprocess-affine',), dict(action='store_true', help='--preprocess: plain (x - mean) / std instead of the mixture fit '
                                                              '(`topaz preprocess --affine`)')),
    (('--preprocess-sample',), dict(type=int, default=10, help='--preprocess: fit the mixture on every n-th pixel '
                                                               '(`topaz preprocess --sample`)')),
    (('--preprocess-niters',), dict(type=int, default=100, help='--preprocess: cap on the EM iterations of one fit (`--niters`)')),
    (('--preprocess-alpha',), dict(type=float, default=900, help='--preprocess: alpha of the Beta prior on the mixing proportion '
                                                                 '(`--alpha`)')),
    (('--preprocess-beta',), dict(type=float, default=1, help='--preprocess: beta of the Beta prior on the mixing proportion '
                                                              '(`--beta`)')),
]

EXTRACT: List[Flag] = [
    (('paths',), dict(nargs='*', help='micrographs to pick from; read from stdin when empty')),
    (('-m', '--model'), dict(default='resnet16', help='pretrained alias, model file, or "none" when the inputs already are score maps')),
    (('-r', '--radius'), dict(type=int, help='suppression radius in pixels')),
    (('-t', '--threshold'), dict(type=float, default=-6, help='keep picks with a log-odds score above this')),
    (('-s', '--down-scale'), dict(type=float, default=1, help='divide output coordinates by this')),
    (('-x', '--up-scale'), dict(type=float, default=1, help='multiply output coordinates by this')),
    (('--num-workers',), dict(type=int, default=0, help='ignored: suppression runs on the GPU')),
    _THREADS,
    (('-p', '--patch-size'), dict(type=int, default=0, help='score the image in tiles of this size (0: whole image)')),
    (('--batch-size',), dict(type=int, default=1, help='accepted for compatibility')),
    (('--assignment-radius',), dict(type=int, help='match radius between picks and --targets (default: the extraction radius)')),
    (('--min-radius',), dict(type=int, default=5, help='radius search: lower bound')),
    (('--max-radius',), dict(type=int, default=100, help='radius search: upper bound')),
    (('--step-radius',), dict(type=int, default=5, help='radius search: step')),
    (('--targets',), dict(help='labelled coordinates; enables the radius search / validation report')),
    (('--only-validate',), dict(action='store_true', help='print validation metrics, write no picks')),
    (('-d', '--device'), dict(type=int, default=0, help='MI355X index (no CPU mode); LOCAL_RANK under torchrun')),
    (('-o', '--output'), dict(help='pick file, or directory with --per-micrograph')),
    (('--per-micrograph',), dict(action='store_true', help='one pick file per micrograph')),
    (('--suffix',), dict(default='', help='suffix of the per-micrograph file names')),
    (('--format',), dict(choices=['coord', 'csv', 'star', 'json', 'box'], default='coord', help='pick file format')),
    (('--dims',), dict(type=int, default=2, choices=[2, 3], help='2: micrographs, 3: tomograms')),
    (('-v', '--verbose'), dict(action='store_true', help='progress on stderr')),
    _GPUS,
    _PRECISION,
    (('--preprocess',), dict(type=int, default=0, metavar='S',
                             help='pick from raw micrographs: put every input through what `topaz preprocess -s S` does -- Fourier '
                                  'down-sampling by S (when S > 1), then normalisation -- in device memory before it is scored '
                                  '(0: off; 1: normalise only).  Picks are in the frame of the scored, S times smaller image, '
                                  'exactly as when `topaz preprocess` wrote it to a file first: -x S scales them back to the raw '
                                  'frame.  Needs --dims 2 and a model')),
    *_PREPROCESS_FIT,
    (('--particle-stack',), dict(metavar='PATH',
                                 help='also write the MRC particle stack `topaz particle_stack` would make of the pick table, and '
                                      'its STAR file next to it, cut while each micrograph is resident for picking (under '
                                      '--preprocess S -x S: from the raw frame).  The micrographs must be MRC files given sorted '
                                      'by name; needs --particle-size, --dims 2 and a model, not with --targets')),
    (('--particle-size',), dict(type=int, help='--particle-stack: box size in pixels (`particle_stack --size`)')),
    (('--particle-resize',), dict(type=int, default=-1, help='--particle-stack: downsample every box to this size '
                                                             '(`particle_stack --resize`; default: off)')),
    (('--particle-threshold',), dict(type=float, default=-float('inf'),
                                     help='--particle-stack: keep picks with score >= this in the stack (`particle_stack '
                                          '--threshold`; default: -inf).  The pick table is not filtered by it')),
    (('--particle-metadata',), dict(metavar='STAR', help='--particle-stack: per-micrograph metadata merged into the output STAR '
                                                         '(`particle_stack --metadata`)')),
    (('--float16',), dict(action='store_true', help='--particle-stack: store the stack as float16 (MRC mode 12)')),
]

_TRAINING_ONLY = 'training option (not supported on this path)'

DENOISE: List[Flag] = [
    (('-d', '--device'), dict(type=int, default=0, help='MI355X index; LOCAL_RANK under torchrun')),
    (('micrographs',), dict(nargs='*', help='images to denoise')),
    (('-o', '--output'), dict(default='', help='output directory (default: next to the input, suffix .denoised)')),
    (('--suffix',), dict(default='', help='suffix of the output names')),
    (('--format',), dict(dest='format_', default='mrc', help='mrc, tiff, png or jpg')),
    (('--normalize',), dict(action='store_true', help='standardise the output instead of restoring mean and scale')),
    (('--stack',), dict(action='store_true', help='the input is one MRC stack: every section is denoised on its own statistics and -o names '
                                                    'the one output stack; --gpus shards the sections, all ranks writing that one file')),
    (('--save-prefix',), dict(help=_TRAINING_ONLY)),
    (('--save-interval',), dict(type=int, default=10, help=_TRAINING_ONLY)),
    (('-m', '--model'), dict(nargs='+', default=['unet'], help='one or more models (outputs averaged): unet, unet-small, fcnn, affine, unet-v0.2.1, or a file')),
    (('-a', '--dir-a'), dict(help=_TRAINING_ONLY)),
    (('-b', '--dir-b'), dict(help=_TRAINING_ONLY)),
    (('--hdf',), dict(help=_TRAINING_ONLY)),
    (('--preload',), dict(action='store_true', help=_TRAINING_ONLY)),
    (('--holdout',), dict(type=float, default=0.1, help=_TRAINING_ONLY)),
    (('--lowpass',), dict(type=float, default=1, help='hard low-pass of the raw micrograph before denoising: keep frequencies up to 0.5 / F (F > 1)')),
    (('--gaussian',), dict(type=float, default=0, help='sigma of a Gaussian pre-filter')),
    (('--inv-gaussian',), dict(type=float, default=0, help='sigma of an inverse-Gaussian pre-filter')),
    (('--deconvolve',), dict(action='store_true', help='flatten the spatial covariance of the normalised micrograph before denoising')),
    (('--deconv-patch',), dict(type=int, default=1, help='estimate the --deconvolve filter per tile of an N x N grid (default: 1, the whole micrograph)')),
    (('--pixel-cutoff',), dict(type=float, default=0, help='zero pixels further than this many sigma from the mean before filtering and denoising '
                                                                   '(0: keep every pixel)')),
    (('-s', '--patch-size'), dict(type=int, default=1024, help='tile size (<1: whole image)')),
    (('-p', '--patch-padding'), dict(type=int, default=500, help='halo around each tile')),
    (('--method',), dict(choices=['noise2noise', 'masked'], default='noise2noise', help=_TRAINING_ONLY)),
    (('--arch',), dict(choices=['unet', 'unet-small', 'unet2', 'unet3', 'fcnet', 'fcnet2', 'affine'], default='unet', help=_TRAINING_ONLY)),
    (('--optim',), dict(choices=['adam', 'adagrad', 'sgd'], default='adagrad', help=_TRAINING_ONLY)),
    (('--lr',), dict(type=float, default=0.001, help=_TRAINING_ONLY)),
    (('--criteria',), dict(default='L2', choices=['L0', 'L1', 'L2'], help=_TRAINING_ONLY)),
    (('-c', '--crop'), dict(type=int, default=800, help=_TRAINING_ONLY)),
    (('--batch-size',), dict(type=int, default=4, help=_TRAINING_ONLY)),
    (('--num-epochs',), dict(type=int, default=100, help=_TRAINING_ONLY)),
    (('--num-workers',), dict(type=int, default=16, help=_TRAINING_ONLY)),
    _THREADS,
    _GPUS,
    _PRECISION,
    _FLOAT16,
]

DENOISE3D: List[Flag] = [
    (('volumes',), dict(nargs='*', help='tomograms to denoise')),
    (('-o', '--output'), dict(default='', help='output directory (default: next to the input, suffix .denoised)')),
    (('--suffix',), dict(default='', help='suffix of the output names')),
    (('-m', '--model'), dict(default='unet-3d', help='unet-3d, unet-3d-10a, unet-3d-20a, or a saved model / state_dict file')),
    (('-a', '--even-train-path'), dict(help=_TRAINING_ONLY)),
    (('-b', '--odd-train-path'), dict(help=_TRAINING_ONLY)),
    (('--N-train',), dict(type=int, default=1000, help=_TRAINING_ONLY)),
    (('--N-test',), dict(type=int, default=200, help=_TRAINING_ONLY)),
    (('-c', '--crop'), dict(type=int, default=96, help=_TRAINING_ONLY)),
    (('--base-kernel-width',), dict(type=int, default=11, help='first-layer kernel width of a state_dict model')),
    (('--optim',), dict(choices=['adam', 'adagrad', 'sgd'], default='adagrad', help=_TRAINING_ONLY)),
    (('--lr',), dict(type=float, default=0.001, help=_TRAINING_ONLY)),
    (('--criteria',), dict(default='L2', choices=['L1', 'L2'], help=_TRAINING_ONLY)),
    (('--momentum',), dict(type=float, default=0.8, help=_TRAINING_ONLY)),
    (('--batch-size',), dict(type=int, default=10, help=_TRAINING_ONLY)),
    (('--num-epochs',), dict(type=int, default=500, help=_TRAINING_ONLY)),
    (('-w', '--weight_decay'), dict(type=float, default=0, help=_TRAINING_ONLY)),
    (('--save-interval',), dict(type=int, default=10, help=_TRAINING_ONLY)),
    (('--save-prefix',), dict(help=_TRAINING_ONLY)),
    (('--num-workers',), dict(type=int, default=1, help=_TRAINING_ONLY)),
    _THREADS,
    (('-g', '--gaussian'), dict(type=float, default=0, help='sigma of a Gaussian post-filter (raises: a no-op upstream)')),
    (('-s', '--patch-size'), dict(type=int, default=96, help='tile size (<1: whole volume)')),
    (('-p', '--patch-padding'), dict(type=int, default=48, help='halo around each tile')),
    (('-d', '--device'), dict(type=int, default=-2, help='-2: every visible MI355X (one rank process each; LOCAL_RANK when already under a launcher); >=0: that GPU; -1 is an error')),
    _GPUS,
    _PRECISION,
    _FLOAT16,
]

SEGMENT: List[Flag] = [
    (('paths',), dict(nargs='+', help='images to score')),
    (('-m', '--model'), dict(default='resnet16', help='pretrained alias or model file')),
    (('-o', '--destdir'), dict(help='directory for the score maps')),
    (('-d', '--device'), dict(type=int, default=0, help='MI355X index')),
    _THREADS,
    (('-p', '--patch-size'), dict(type=int, default=None, help='score in tiles of twice this size (default: whole image)')),
    (('-v', '--verbose'), dict(action='store_true', help='progress on stdout')),
    _GPUS,
    _PRECISION,
    (('--preprocess',), dict(type=int, default=0, metavar='S',
                             help='score raw micrographs: put every input through what `topaz preprocess -s S` does -- Fourier '
                                  'down-sampling by S (when S > 1), then normalisation -- in device memory before it is scored '
                                  '(0: off; 1: normalise only).  The map has the size of the S times smaller image.  Micrographs '
                                  'only, not volumes')),
    *_PREPROCESS_FIT,
    (('--format',), dict(choices=['tiff', 'mrc', 'npy'], default=None,
                         help='file type of the score maps (default: tiff for micrographs, npy for volumes); mrc carries the '
                              'header of an MRC input with its mode and size updated')),
    _FLOAT16,
]

DOWNSAMPLE: List[Flag] = [
    (('file',), dict()),
    (('-s', '--scale'), dict(type=int, default=4, help='integer reduction factor')),
    (('-o', '--output'), dict(help='file to write')),
    (('-v', '--verbose'), dict(action='store_true', help='report the shapes')),
    _FLOAT16,
]


NORMALIZE: List[Flag] = [
    (('files',), dict(nargs='+')),
    (('-s', '--scale'), dict(default=1, type=int, help='shrink the images by this factor first')),
    (('--affine',), dict(action='store_true', help='plain (x - mean) / std of the whole image instead of the mixture fit')),
    (('--sample',), dict(default=10, type=int, help='fit the mixture on every n-th pixel (random subset drawn from the NumPy RNG in '
                                                    'file order; with --gpus each rank draws for its own files only, so the '
                                                    'subsets depend on the number of ranks -- --sample 1 does not)')),
    (('--niters',), dict(default=100, type=int, help='cap on the EM iterations of one fit')),
    (('-a', '--alpha'), dict(default=900, type=float, help='alpha of the Beta prior on the mixing proportion')),
    (('-b', '--beta'), dict(default=1, type=float, help='beta of the Beta prior on the mixing proportion')),
    (('--metadata',), dict(action='store_true', help='also write <name>.metadata.json with the fitted parameters')),
    (('-d', '--device'), dict(default=0, type=int, help='GPU to use')),
    (('-t', '--num-workers'), dict(type=int, default=0, help='accepted for compatibility (the fit runs on the GPU; --gpus shards the files)')),
    (('-j', '--num-threads'), dict(type=int, default=0, help='accepted for compatibility')),
    (('-o', '--destdir'), dict(help='directory to write into')),
    (('--format',), dict(dest='format_', default='mrc', help='comma separated list of mrc, tiff, png')),
    (('-v', '--verbose'), dict(action='store_true', help='name every processed file')),
    _GPUS,
    _FLOAT16,
]


PARTICLE_STACK: List[Flag] = [
    (('file',), dict(help='pick table (tab separated: image_name, x_coord, y_coord[, score])')),
    (('--image-root',), dict(help='directory of the micrographs (default: the working directory)')),
    (('-o', '--output'), dict(help='particle stack to write (the STAR file goes next to it)')),
    (('--size',), dict(type=int, help='box size in pixels (required)')),
    (('--threshold',), dict(type=float, default=-float('inf'), help='keep picks with score >= this (default: -inf)')),
    (('--resize',), dict(type=int, default=-1, help='downsample every box to this size (default: off)')),
    (('--image-ext',), dict(default='.mrc', help='extension appended to the image names (default: .mrc)')),
    (('--metadata',), dict(help='STAR file of per-micrograph metadata merged into the output STAR on MicrographName')),
]
# kept apart from the table above, which mirrors the reference's parser flag for flag (tests/test_cpu_particle_stack.py): the
# ranks cut the plan's micrographs i = rank (mod N) into the one output file; --float16 stores the stack as MRC mode 12
PARTICLE_STACK_RANKS: List[Flag] = [_GPUS, _FLOAT16]


def build_parser(flags: List[Flag], description: str, parser: argparse.ArgumentParser = None) -> argparse.ArgumentParser:
    parser = parser or argparse.ArgumentParser(description=description)
    for names, kw in flags:
        parser.add_argument(*names, **kw)
    return parser
