"""Generate tests/golden/denoise_options.npz (mic_a) and denoise_options_mic_b.npz (mic_b) by running the REFERENCE's own denoise_image with a pixel cutoff, a Gaussian and an
inverse-Gaussian pre-filter.

Test infrastructure, run by hand on the CPU where the reference (tbepler/topaz 0.3.18) is available, as
make_denoise_prefilter_golden.py is; no test runs it.  Recipe:

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_denoise_options.py <reference checkout>

The inputs are tests/golden/cli/mic_a.mrc and mic_b.mrc (160 x 200 float32); every array is what the reference's denoise_image
returns in process with its packaged models, whole image (patch_size -1).  The reference's InvGaussianFilter cannot be
constructed (filters.py:85 calls GaussianDenoise.__init__ without a sigma), so the inverse filter is assembled from its working
parts as inv_gaussian.npz was: a reference GaussianDenoise(0.8) whose weights are overwritten with inverse_filter of the
normalised kernel.  Keys, <mic> in (mic_a, mic_b):
  <mic>:cutoff2.5:affine            cutoff=2.5, Denoise('affine')
  <mic>:cutoff2.5:unet-small        cutoff=2.5, Denoise('unet-small')
  <mic>:gaus1.2:unet-small          gaus=GaussianDenoise(1.2)
  <mic>:cutoff2.5+gaus1.2:unet-small        both
  <mic>:cutoff2.5+gaus1.2:unet-small:norm   both, normalize=True
  <mic>:invgaus0.8:unet-small       inv_gaus as above
  <mic>:margin                      min over pixels of | |(mic - mu) / std| - 2.5 | in the reference's float32 arithmetic

A normalised pixel on the cutoff would flip between implementations and move the result by 2.5: the tool refuses to write a
fixture unless every margin is above 1e-5 (hundreds of float32 ulps of 2.5).
"""
from __future__ import annotations

import os
import sys
import types

sys.dont_write_bytecode = True
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
# twelve float32 images do not fit one file under the repository's 1 MiB limit: one file per micrograph
OUT = {'mic_a': os.path.join(ROOT, 'tests', 'golden', 'denoise_options.npz'),
       'mic_b': os.path.join(ROOT, 'tests', 'golden', 'denoise_options_mic_b.npz')}
CUTOFF, SIGMA, INV_SIGMA, MARGIN = 2.5, 1.2, 0.8, 1e-5


def main(argv):
    if len(argv) != 2:
        sys.exit(__doc__)
    sys.path.insert(0, argv[1])
    h5 = types.ModuleType('h5py')            # imported at module top by topaz/denoising/datasets.py, unused on this path
    h5.File = object
    sys.modules['h5py'] = h5
    import numpy as np
    import torch
    from topaz import mrc
    from topaz.denoise import Denoise, denoise_image
    from topaz.filters import GaussianDenoise, gaussian_filter, inverse_filter
    torch.set_num_threads(8)

    width = 1 + 2 * int(np.ceil(INV_SIGMA * 5))
    f = gaussian_filter(INV_SIGMA, s=width)
    f /= f.sum()
    inv = GaussianDenoise(INV_SIGMA)
    inv.filter.weight.data[:] = torch.from_numpy(inverse_filter(f)).float()
    gaus = GaussianDenoise(SIGMA)
    small, affine = Denoise('unet-small', use_cuda=False), Denoise('affine', use_cuda=False)

    meta = np.asarray(repr(dict(reference='tbepler/topaz 0.3.18', torch=torch.__version__, numpy=np.__version__,
                                cutoff=CUTOFF, gaus=SIGMA, inv_gaus=INV_SIGMA)))
    for name, path in OUT.items():
        out = {'meta': meta}
        with open(os.path.join(ROOT, 'tests', 'golden', 'cli', name + '.mrc'), 'rb') as fh:
            mic = np.array(mrc.parse(fh.read())[0], dtype=np.float32)
        xn = (mic - mic.mean()) / mic.std()                   # denoise.py:388-389, float32 like the reference's
        assert xn.dtype == np.float32
        margin = float(np.abs(np.abs(xn.astype(np.float64)) - CUTOFF).min())
        assert margin > MARGIN, f'{name}: a normalised pixel lies {margin:.2e} from the cutoff'
        out[f'{name}:margin'] = np.float64(margin)
        cases = {
            'cutoff2.5:affine': dict(models=[affine], cutoff=CUTOFF),
            'cutoff2.5:unet-small': dict(models=[small], cutoff=CUTOFF),
            'gaus1.2:unet-small': dict(models=[small], gaus=gaus),
            'cutoff2.5+gaus1.2:unet-small': dict(models=[small], cutoff=CUTOFF, gaus=gaus),
            'cutoff2.5+gaus1.2:unet-small:norm': dict(models=[small], cutoff=CUTOFF, gaus=gaus, normalize=True),
            'invgaus0.8:unet-small': dict(models=[small], inv_gaus=inv),
        }
        for key, kw in cases.items():
            with torch.no_grad():
                y = denoise_image(mic.copy(), kw.pop('models'), **kw)
            out[f'{name}:{key}'] = np.asarray(y, dtype=np.float32)
            assert out[f'{name}:{key}'].shape == mic.shape and np.isfinite(out[f'{name}:{key}']).all()
        print(f'{name}: margin {margin:.2e}, {int((np.abs(xn) > CUTOFF).sum())} pixels beyond the cutoff')
        np.savez_compressed(path, **out)
        print(f'{path}: {os.path.getsize(path) / 1024:.0f} KiB')
        assert os.path.getsize(path) < 1 << 20


if __name__ == '__main__':
    main(sys.argv)
