"""conv31 / conv63 / conv127 stacks trained with `--pooling max|avg` (topaz/model/features/basic.py:33-39,54-56,81-89), host side:
the loader, the traits, width / fill() and the packed layer program against what the reference's own filled modules recorded
(tools/make_pooled_basicconv_golden.py).  No GPU."""
import hashlib
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from topaz_amd import _lib
from topaz_amd.model import pack
from topaz_amd.model.factory import load_model
from topaz_amd.model.unpickle import load_module_pickle

FIXTURES = ['conv31_max_bn_u16', 'conv31_avg_u32', 'conv31_max_drop_bn_u16', 'conv127_max_bn_u16', 'conv127_avg_bn_u16',
            'conv31_3d_max_bn_u8', 'conv63_3d_avg_bn_u8', 'conv31_max_bn_u16_us2']


def program_digest(program) -> str:
    """sha256 over the tpz_layer structs and the weight blob: the bytes tpz_model_load receives (as the generator computes it)"""
    h = hashlib.sha256()
    for L in program.layers:
        h.update(bytes(L))
    h.update(program.flat_blob().tobytes())
    return h.hexdigest()


@pytest.mark.parametrize('name', FIXTURES)
def test_pooled_pickle_loads_and_packs_like_the_reference_fills(name):
    z = load_golden(f'score_{name}')
    path = os.path.join(GOLDEN, f'user_model_{name}.sav')
    arch, sd, traits = load_module_pickle(path, with_traits=True)
    pooling, dims = str(z['pooling']), int(z['dims'])
    assert arch == str(z['arch'])
    assert traits == {'pooling': pooling, 'dropout': bool(z['dropout'])}
    idx = sorted({int(k.split('.')[2]) for k in sd if k.startswith('features.features.')})
    n_convs = len(pack.BASIC_SIZES[arch])
    # numbered without the Dropouts; every pool keeps an index of its own, which holds no tensor
    per_block = 2 + int(bool(z['bn']))
    want_idx = [b * (per_block + 1) + j for b in range(n_convs) for j in range(per_block)]
    assert idx == want_idx

    m = load_model(path)
    assert m.arch == arch and m.pooling == pooling and m.dropout == bool(z['dropout']) and m.dims == dims
    assert m.width == int(z['width']) == {'conv31': 31, 'conv63': 63, 'conv127': 127}[arch]
    assert m.fill() == int(z['stride']) == 2 ** (n_convs - 1)
    assert m.features.units == int(z['units']) and m.latent_dim == int(z['units']) * int(z['unit_scaling']) ** (n_convs - 1)

    # the program: convs and pools in the reference's order, with the dilation and padding fill() left on each module
    P = m._program
    ops = [L for L in P.layers]
    kinds = [str(k) for k in z['kinds']]
    assert len(ops) == len(kinds) == 2 * n_convs - 1
    first = True
    for L, kind, dil, pad in zip(ops, kinds, z['dilations'], z['paddings']):
        assert L.dims == dims
        if kind.startswith('Conv'):
            assert L.op == _lib.TPZ_OP_CONV
            # the reference pads the image once by width // 2 and runs unpadded convs: the first conv carries that padding
            assert L.pad == (m.width // 2 if first else 0) and int(pad) == 0
            first = False
        elif kind.startswith('MaxPool'):
            assert L.op == _lib.TPZ_OP_MAXPOOL and L.k == 3 and L.pad == int(pad) == 1
        else:
            assert kind.startswith('AvgPool') and L.op == _lib.TPZ_OP_AVGPOOL and L.k == 3 and L.pad == int(pad) == 1
        assert L.dil == int(dil), (kind, L.dil, int(dil))
    assert ops[-1].head == 1
    k = 0
    while f'x{k}' in z.files:
        shape = z[f'x{k}'].shape
        D, H, W = (1,) + tuple(shape) if dims == 2 else tuple(shape)
        got = P.out_shape(D, H, W)
        assert (got[1:] if dims == 2 else got) == z[f'y{k}'].shape
        k += 1


def test_shrink_of_the_max_pooled_score_map():
    """a filled max pool at dilation d loses 2 (d - 1) per axis: conv31 2, conv63 8, conv127 22; the mean preserves the size"""
    for arch, loss in (('conv31', 2), ('conv63', 8), ('conv127', 22)):
        n = len(pack.BASIC_SIZES[arch])
        dils, pool_dils, stride = pack.basic_fill(n, True, False, 'max')
        assert dils == [2 ** i for i in range(n)] and pool_dils == [2 ** i for i in range(n - 1)] and stride == 2 ** (n - 1)
        assert sum(2 * (d - 1) for d in pool_dils) == loss
        assert pack.basic_fill(n, False, False, 'avg')[1] == [1] * (n - 1)
        assert pack.basic_width(pack.BASIC_SIZES[arch], 'max') == pack.basic_width(pack.BASIC_SIZES[arch]) == 2 ** (n + 2) - 1
    # with --dropout the zip of fill() slips (basic.py:57-58): conv31 + BN pools at 1 and 4
    assert pack.basic_fill(3, True, True, 'max') == ([1, 2, 4], [1, 4], 4)
    # a pool that fill() never reaches would stay strided: refused, not approximated
    with pytest.raises(NotImplementedError, match='strided'):
        pack.basic_fill(5, False, True, 'max')


def _repickle(tmp_path, name, edit):
    """the module pickle of a fixture with its layer list edited: loaded with the loader's own inert stand-ins, saved again with
    classes of the same qualified names registered under a scratch `topaz` package (nothing of the reference is imported)"""
    import sys
    import types
    from topaz_amd.model.unpickle import _PickleModule
    obj = torch.load(os.path.join(GOLDEN, f'user_model_{name}.sav'), map_location='cpu', weights_only=False,
                     pickle_module=_PickleModule)
    seq = obj.__dict__['_modules']['features'].__dict__['_modules']['features']
    edit(seq.__dict__['_modules'])
    added = []
    try:
        for o in (obj, obj.__dict__['_modules']['features']):
            modname, _, cls = type(o)._tpz_qualname.rpartition('.')
            parts = modname.split('.')
            for i in range(1, len(parts) + 1):
                pkg = '.'.join(parts[:i])
                if pkg not in sys.modules:
                    sys.modules[pkg] = types.ModuleType(pkg)
                    added.append(pkg)
            type(o).__module__, type(o).__qualname__ = modname, cls
            setattr(sys.modules[modname], cls, type(o))
        out = tmp_path / f'{name}_edited.sav'
        torch.save(obj, str(out))
    finally:
        for pkg in added:
            sys.modules.pop(pkg, None)
    return str(out)


def test_unknown_layer_kind_is_still_refused(tmp_path):
    def swap_activation(mods):
        key = next(k for k, v in mods.items() if type(v).__name__ == 'PReLU')
        mods[key] = torch.nn.Tanh()
    with pytest.raises(NotImplementedError, match='Tanh'):
        load_module_pickle(_repickle(tmp_path, 'conv31_max_bn_u16', swap_activation))

    def other_pool(mods):
        key = next(k for k, v in mods.items() if type(v).__name__ == 'MaxPool2d')
        mods[key] = torch.nn.MaxPool2d(2, stride=2)
    with pytest.raises(NotImplementedError, match='kernel_size'):
        load_module_pickle(_repickle(tmp_path, 'conv31_max_bn_u16', other_pool))

    def lp_pool(mods):
        key = next(k for k, v in mods.items() if type(v).__name__ == 'AvgPool2d')
        mods[key] = torch.nn.LPPool2d(2, 3, stride=2)
    with pytest.raises(NotImplementedError, match='LPPool2d'):
        load_module_pickle(_repickle(tmp_path, 'conv31_avg_u32', lp_pool))
    # the unedited round trip loads: the refusals above are about the edits
    arch, sd, traits = load_module_pickle(_repickle(tmp_path, 'conv31_avg_u32', lambda mods: None), with_traits=True)
    assert arch == 'conv31' and traits['pooling'] == 'avg'


def test_avg_pooling_is_for_the_conv_stacks_only():
    from topaz_amd.model.classifier import LinearClassifier
    with pytest.raises(ValueError, match='avg'):
        LinearClassifier('resnet8', {'classifier.weight': np.zeros((1, 4, 1, 1), np.float32)}, pooling='avg')


@pytest.mark.parametrize('fn,arch,dims', [('user_model_conv31_drop_bn_u16.sav', 'conv31', 2),
                                          ('user_model_conv127_bn_u16.sav', 'conv127', 2),
                                          ('user_model_conv31_3d_bn_u8.sav', 'conv31', 3)])
def test_unpooled_programs_keep_their_bytes(fn, arch, dims):
    """the generalised packer builds, for an unpooled stack, the very bytes the packer before it built (digests taken by the
    generator from that revision's sources)"""
    z = load_golden('pooled_basicconv_parent')
    a, sd, traits = load_module_pickle(os.path.join(GOLDEN, fn), with_traits=True)
    assert a == arch and not traits['pooling']
    P, width = pack.pack_basicconv(pack.BASIC_SIZES[arch], sd, traits['dropout'], dims)
    assert program_digest(P) == str(z[fn])
    m = load_model(os.path.join(GOLDEN, fn))
    assert program_digest(m._program) == str(z[fn]) and not m.pooling
