"""Generate the particle_stack fixtures under tests/golden/particle_stack/ by running the REFERENCE itself.

Test infrastructure, run by hand where the reference (tbepler/topaz 0.3.18) is available, as oracle/make_golden.py is; no test
runs it.  Recipe:

    PYTHONDONTWRITEBYTECODE=1 TOPAZ_REFERENCE=<reference checkout> python tools/make_particle_stack_golden.py

Fixtures (tests/test_cpu_particle_stack.py and tests/test_gpu_particle_stack.py read them):
  1. stack32.mrcs / .star   the reference CLI on tests/golden/cli/extract_picks.txt over mic_a / mic_b at --size 32
  2. stack33_t5.mrcs / .star   the same at --size 33 --threshold -5 (odd size, 44 of the 88 picks)
  3. frames3.mrc (3 x 96 x 128, seeded N(0, 1) with a constant 20 x 20 patch), picks3.txt, meta3.star and the reference's
     stack9.mrcs / .star at --size 9 --metadata meta3.star: a box inside the patch (NaN), boxes cut by the corners' edges and
     one past the high x edge (all zeros)
  4. resize16.npy / resize15.npy: the reference's 2-D downsample applied to each frame of fixture 1's boxes, then
     (r - r.mean()) / r.std() in float32 -- the reference CLI's own --resize output is unusable (its 2-D downsample receives the
     3-D box); stack32_r16_meta.star: the reference CLI's STAR at --resize 16 --metadata meta_ab.star (valid: only its stack
     bytes are wrong)
"""
from __future__ import annotations

import contextlib
import io
import os
import shutil
import sys
import tempfile
import types

sys.dont_write_bytecode = True
REF = os.environ.get('TOPAZ_REFERENCE', '/root/reference')
sys.path.insert(0, REF)
_h5 = types.ModuleType('h5py')
_h5.File = object
sys.modules['h5py'] = _h5

import numpy as np  # noqa: E402

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
CLI = os.path.join(ROOT, 'tests', 'golden', 'cli')
OUT = os.path.join(ROOT, 'tests', 'golden', 'particle_stack')


def run(picks, out_name, size, threshold=-np.inf, resize=-1, image_root=CLI, metadata=None, keep_stack=True):
    from topaz.utils.picks import create_particle_stack
    tmp = tempfile.mkdtemp()
    try:
        out = os.path.join(tmp, out_name)
        with contextlib.redirect_stderr(io.StringIO()):
            create_particle_stack(picks, out, threshold, size, resize, image_root, '.mrc', metadata)
        star = os.path.splitext(out_name)[0] + '.star'
        if keep_stack:
            shutil.copy(out, os.path.join(OUT, out_name))
        shutil.copy(os.path.join(tmp, star), os.path.join(OUT, star if keep_stack else os.path.splitext(out_name)[0] + '_meta.star'))
    finally:
        shutil.rmtree(tmp)


def frames3():
    """3-frame float32 micrograph with a constant patch, its pick table and metadata STAR"""
    import topaz.mrc as mrc
    x = np.random.RandomState(20251016).randn(3, 96, 128).astype(np.float32)
    x[:, 40:60, 60:80] = 1.25
    with open(os.path.join(OUT, 'frames3.mrc'), 'wb') as f:
        mrc.write(f, x)
    rows = [('frames3', 70, 50, 3.5),     # the 9^2 box lies inside the constant patch: zero variance
            ('frames3', 2, 1, 1.25),      # cut by the left and the top edge
            ('frames3', 126, 94, -0.5),   # cut by the right and the bottom edge
            ('frames3', 145, 30, 0.75)]   # left = 141 >= 128 + 9: past the high x edge, all zeros
    with open(os.path.join(OUT, 'picks3.txt'), 'w') as f:
        f.write('image_name\tx_coord\ty_coord\tscore\n')
        for r in rows:
            f.write('%s\t%d\t%d\t%s\n' % r)
    with open(os.path.join(OUT, 'meta3.star'), 'w') as f:
        f.write('data_images\nloop_\n_rlnMicrographName #1\n_rlnDetectorPixelSize #2\n_rlnVoltage #3\n'
                'frames3.mrc\t5.0\t300.0\n')


def meta_ab():
    with open(os.path.join(OUT, 'meta_ab.star'), 'w') as f:
        f.write('data_images\nloop_\n_rlnMicrographName #1\n_rlnDetectorPixelSize #2\n_rlnVoltage #3\n'
                'mic_a.mrc\t5.0\t300.0\nmic_b.mrc\t6.5\t200.0\n')


def resized(R):
    from topaz.utils.image import downsample
    with open(os.path.join(OUT, 'stack32.mrcs'), 'rb') as f:
        f.seek(1024)
        boxes = np.frombuffer(f.read(), dtype=np.float32).reshape(-1, 1, 32, 32)
    out = []
    for box in boxes:
        r = np.stack([downsample(frame, 0, shape=(R, R)) for frame in box])
        out.append((r - r.mean()) / r.std())
    np.save(os.path.join(OUT, f'resize{R}.npy'), np.stack(out).astype(np.float32))


def main():
    os.makedirs(OUT, exist_ok=True)
    picks = os.path.join(CLI, 'extract_picks.txt')
    run(picks, 'stack32.mrcs', 32)
    run(picks, 'stack33_t5.mrcs', 33, threshold=-5.0)
    frames3()
    run(os.path.join(OUT, 'picks3.txt'), 'stack9.mrcs', 9, image_root=OUT, metadata=os.path.join(OUT, 'meta3.star'))
    meta_ab()
    run(picks, 'stack32_r16.mrcs', 32, resize=16, metadata=os.path.join(OUT, 'meta_ab.star'), keep_stack=False)
    resized(16)
    resized(15)
    for name in sorted(os.listdir(OUT)):
        print(f'{name}: {os.path.getsize(os.path.join(OUT, name)) / 1024:.0f} KiB')


if __name__ == '__main__':
    main()
