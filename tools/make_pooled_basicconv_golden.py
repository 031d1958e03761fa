"""Generate the pooled-BasicConv fixtures under tests/golden/ by running the REFERENCE itself.

Test infrastructure, run by hand where the reference (tbepler/topaz 0.3.18) is available, as oracle/make_golden.py is; no test
runs it.  Recipe:

    PYTHONDONTWRITEBYTECODE=1 TOPAZ_REFERENCE=<reference checkout> python tools/make_pooled_basicconv_golden.py [--parent REV]

Fixtures (tests/test_cpu_pooled_basicconv.py and tests/test_gpu_pooled_basicconv.py read them), one pair per model of CASES:
  user_model_<name>.sav   torch.save(model) of a seeded LinearClassifier(BasicConv(..., pooling='max'|'avg')), saved unfilled as
                          `topaz train -m conv31|conv63|conv127 --pooling max|avg` does (training.py:601)
  score_<name>.npz        inputs x0 (, x1), the reference's filled eval-mode outputs y0 (, y1), width, the stride fill() returned,
                          and what fill() left on the modules: kind / dilation / padding of every conv and pool, in order
and pooled_basicconv_parent.npz: for a few UNPOOLED goldens, the sha256 of the layer program (program_digest below) that the
packer of revision --parent builds (default HEAD: run the tool before the change under test is committed) -- the generalised
packer must keep producing those bytes.
"""
from __future__ import annotations

import argparse
import hashlib
import os
import subprocess
import sys
import tempfile
import types

sys.dont_write_bytecode = True
REF = os.environ.get('TOPAZ_REFERENCE')
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
OUT = os.path.join(ROOT, 'tests', 'golden')

# name, sizes, units, unit_scaling, bn, dropout, pooling, dims, input shapes
CASES = [
    ('conv31_max_bn_u16', [7, 5, 5], 16, 1, True, 0.0, 'max', 2, [(70, 90), (37, 53)]),
    ('conv31_avg_u32', [7, 5, 5], 32, 1, False, 0.0, 'avg', 2, [(70, 90), (37, 53)]),
    ('conv31_max_drop_bn_u16', [7, 5, 5], 16, 1, True, 0.3, 'max', 2, [(70, 90), (37, 53)]),
    ('conv127_max_bn_u16', [7, 5, 5, 5, 5], 16, 1, True, 0.0, 'max', 2, [(64, 75)]),
    ('conv127_avg_bn_u16', [7, 5, 5, 5, 5], 16, 1, True, 0.0, 'avg', 2, [(64, 75)]),
    ('conv31_3d_max_bn_u8', [7, 5, 5], 8, 1, True, 0.0, 'max', 3, [(20, 22, 27)]),
    ('conv63_3d_avg_bn_u8', [7, 5, 5, 5], 8, 1, True, 0.0, 'avg', 3, [(20, 22, 27)]),
    ('conv31_max_bn_u16_us2', [7, 5, 5], 16, 2, True, 0.0, 'max', 2, [(70, 90), (37, 53)]),      # `topaz train`'s default unit_scaling
]
# unpooled goldens whose packed program must not change: file, sizes key, dims
UNPOOLED = [('user_model_conv31_drop_bn_u16.sav', 'conv31', 2), ('user_model_conv127_bn_u16.sav', 'conv127', 2),
            ('user_model_conv31_3d_bn_u8.sav', 'conv31', 3)]

_DIGEST_SNIPPET = '''
import hashlib, sys
from topaz_amd.model import pack
from topaz_amd.model.unpickle import load_module_pickle
path, arch, dims = sys.argv[1], sys.argv[2], int(sys.argv[3])
a, sd, traits = load_module_pickle(path, with_traits=True)
assert a == arch and not traits['pooling']
P, width = pack.pack_basicconv(pack.BASIC_SIZES[arch], sd, traits['dropout'], dims)
h = hashlib.sha256()
for L in P.layers:
    h.update(bytes(L))
h.update(P.flat_blob().tobytes())
print(h.hexdigest())
'''


def program_digest(program) -> str:
    """sha256 over the tpz_layer structs and the weight blob of a LayerProgram: the bytes tpz_model_load receives"""
    h = hashlib.sha256()
    for L in program.layers:
        h.update(bytes(L))
    h.update(program.flat_blob().tobytes())
    return h.hexdigest()


def parent_digests(rev):
    """pack the unpooled goldens with the Python sources of revision `rev` (git archive into a scratch directory)"""
    import numpy as np
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(['git', '-C', ROOT, 'archive', rev, 'topaz_amd/__init__.py', 'topaz_amd/_lib.py', 'topaz_amd/runtime.py',
                              'topaz_amd/model'], check=True, capture_output=True).stdout
        subprocess.run(['tar', '-x', '-C', tmp], input=tar, check=True)
        env = dict(os.environ, PYTHONPATH=tmp, PYTHONDONTWRITEBYTECODE='1')
        for fn, arch, dims in UNPOOLED:
            r = subprocess.run([sys.executable, '-c', _DIGEST_SNIPPET, os.path.join(OUT, fn), arch, str(dims)], env=env, cwd=tmp,
                               check=True, capture_output=True, text=True)
            out[fn] = np.asarray(r.stdout.strip())
            print(f'{fn}: {r.stdout.strip()}')
    full = subprocess.run(['git', '-C', ROOT, 'rev-parse', rev], check=True, capture_output=True, text=True).stdout.strip()
    np.savez_compressed(os.path.join(OUT, 'pooled_basicconv_parent.npz'), revision=np.asarray(full), **out)


def _first(v):
    return v[0] if isinstance(v, (tuple, list)) else v


def models():
    if not REF or not os.path.isdir(os.path.join(REF, 'topaz')):
        raise SystemExit('set TOPAZ_REFERENCE to a checkout of tbepler/topaz 0.3.18')
    sys.path.insert(0, REF)
    h5 = types.ModuleType('h5py')         # imported at module top by topaz/denoising/datasets.py, unused on this path
    h5.File = object
    sys.modules['h5py'] = h5
    import numpy as np
    import torch
    from topaz.model.classifier import LinearClassifier
    from topaz.model.features.basic import BasicConv

    meta = dict(reference='tbepler/topaz 0.3.18', torch=torch.__version__, numpy=np.__version__)
    for ci, (name, sizes, units, us, bn, drop, pooling, dims, shapes) in enumerate(CASES):
        torch.manual_seed(300 + ci)
        m = LinearClassifier(BasicConv(list(sizes), units, unit_scaling=us, dropout=drop, bn=bn, pooling=pooling, dims=dims),
                             dims=dims)
        g = torch.Generator().manual_seed(400 + ci)
        for mod in m.modules():
            if isinstance(mod, (torch.nn.BatchNorm2d, torch.nn.BatchNorm3d)):
                mod.weight.data = 1.0 + 0.1 * torch.randn(mod.weight.shape, generator=g)
                mod.bias.data = 0.1 * torch.randn(mod.bias.shape, generator=g)
                mod.running_mean.data = 0.1 * torch.randn(mod.running_mean.shape, generator=g)
                mod.running_var.data = 1.0 + 0.2 * torch.rand(mod.running_var.shape, generator=g)
            if isinstance(mod, torch.nn.PReLU):
                mod.weight.data.uniform_(0.1, 0.4, generator=g)
        path = os.path.join(OUT, f'user_model_{name}.sav')
        torch.save(m, path)                                   # unfilled, as training does
        m.eval()
        width = m.width
        stride = m.fill()                                     # once, as extract.py:230 does
        kinds, dils, pads = [], [], []
        for mod in m.features.features.children():
            kind = type(mod).__name__
            if kind.startswith(('Conv', 'MaxPool', 'AvgPool')):
                assert _first(mod.stride) == 1, (name, kind, mod.stride)
                kinds.append(kind)
                dils.append(_first(getattr(mod, 'dilation', 1)))
                pads.append(_first(mod.padding))
        rs = np.random.RandomState(500 + ci)
        arrays = {}
        for k, shape in enumerate(shapes):
            x = rs.randn(*shape).astype(np.float32)
            with torch.no_grad():
                y = m(torch.from_numpy(x)[None, None])[0, 0].numpy()
            arrays[f'x{k}'], arrays[f'y{k}'] = x, y
            print(f'{name}: {shape} -> {y.shape}, |y| <= {np.abs(y).max():.3f}')
        npz = os.path.join(OUT, f'score_{name}.npz')
        np.savez_compressed(npz, meta=np.asarray(repr(meta)), arch=np.asarray({3: 'conv31', 4: 'conv63', 5: 'conv127'}[len(sizes)]),
                            pooling=np.asarray(pooling), dims=np.asarray(dims), dropout=np.asarray(drop > 0), bn=np.asarray(bn),
                            units=np.asarray(units), unit_scaling=np.asarray(us), width=np.asarray(width), stride=np.asarray(stride),
                            kinds=np.asarray(kinds), dilations=np.asarray(dils), paddings=np.asarray(pads), **arrays)
        print(f'  {os.path.getsize(path) / 1024:.0f} KiB .sav, {os.path.getsize(npz) / 1024:.0f} KiB .npz')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default='HEAD', help='revision whose packer the unpooled digests are taken from')
    a = ap.parse_args()
    parent_digests(a.parent)
    models()


if __name__ == '__main__':
    main()
