"""Mirror of the patching helpers of topaz/model/utils.py: insize_from_outsize (:39-68),
predict_in_patches (:110-130), get_patches (:133-169), reconstruct_from_patches (:172-193).

Patch geometry is host logic (tile_origins, tile_windows); predict_in_patches_device keeps the image, the tiles and the
stitched map on the device -- tiles cut, tested for the all-zero rule and pasted by the library's tile kernels (tpz_tile_cut /
_flags / _paste), no padded copy, one readback of the flags -- and predict_in_patches is that plus one download.  Quirk kept from the reference: all-zero tiles are skipped by get_patches (:159,165)
while reconstruct_from_patches (:181-191) does not know about it, so an image with an all-zero tile ends in
IndexError exactly as upstream does.
"""
from __future__ import annotations

from typing import List, NamedTuple, Tuple

import numpy as np
import torch


def insize_from_outsize(layers, outsize):
    """layers: objects (or dicts) with kernel_size / stride / padding / dilation"""
    for layer in layers[::-1]:
        get = (lambda k, d: layer.get(k, d)) if isinstance(layer, dict) else (lambda k, d: getattr(layer, k, d))
        first = lambda v: v[0] if isinstance(v, tuple) else v
        k, s = first(get('kernel_size', 1)), first(get('stride', 1))
        p, d = first(get('padding', 0)), first(get('dilation', 1))
        outsize = (outsize - 1) * s + 1 + (k - 1) * d - 2 * p
    return outsize


def tile_origins(shape, step: int):
    """origins of the tile grid over an image / volume of `shape` = ([D,] H, W): rows outermost, then columns, then -- for a
    volume -- planes, which is the order both the cutting and the stitching side walk (model/utils.py:151-166, 181-191)"""
    if len(shape) == 2:
        return [(None, i, j) for i in range(0, shape[0], step) for j in range(0, shape[1], step)]
    return [(k, i, j) for i in range(0, shape[1], step) for j in range(0, shape[2], step) for k in range(0, shape[0], step)]


def _window(t, origin, size):
    """the (at most) size^dims window of tensor / array `t` at `origin`, clipped by slicing at the far edges"""
    k, i, j = origin
    if k is None:
        return t[..., i:i + size, j:j + size]
    return t[..., k:k + size, i:i + size, j:j + size]


def get_patches(X: torch.Tensor, patch_size: int, patch_padding: int = 0, is_3d: bool = False) -> List[torch.Tensor]:
    """tiles of `patch_size` cut from X zero-padded by `patch_padding` on every side, at stride patch_size - 2 * padding
    over the UNPADDED extent (model/utils.py:133-169).  Tiles that hold nothing but zeros are left out, as upstream."""
    dims = 3 if is_3d else 2
    padded = torch.nn.functional.pad(X, (patch_padding,) * (2 * dims))
    tiles = (_window(padded, o, patch_size) for o in tile_origins(tuple(X.shape[-dims:]), patch_size - 2 * patch_padding))
    return [t for t in tiles if bool(t.ne(0).any())]


def reconstruct_from_patches(patches, original_shape, patch_size, patch_padding=0, is_3d=False) -> np.ndarray:
    """float64 array of `original_shape` with patch n pasted at the n-th origin of the same grid (model/utils.py:172-193);
    a patch list shortened by get_patches' zero-tile rule runs out here (IndexError), as upstream."""
    dims = 3 if is_3d else 2
    canvas = np.zeros(original_shape)
    for n, origin in enumerate(tile_origins(tuple(original_shape[-dims:]), patch_size - 2 * patch_padding)):
        piece = patches[n]
        k, i, j = origin
        if k is None:
            canvas[..., i:i + piece.shape[-2], j:j + piece.shape[-1]] = piece
        else:
            canvas[..., k:k + piece.shape[-3], i:i + piece.shape[-2], j:j + piece.shape[-1]] = piece
    return canvas


class TileWindow(NamedTuple):
    """one tile of the grid; every field has one entry per axis, ([z,] y, x)"""
    origin: Tuple[int, ...]      # of the cut window, in the UNPADDED tensor: negative at the near faces
    extent: Tuple[int, ...]      # of the cut window: patch_size, less where slicing the padded array clips it at a far face
    paste: Tuple[int, ...]       # where the tile's scores go in the stitched map
    pasted: Tuple[int, ...]      # how much of them: the extent less the halo on both sides


def tile_windows(shape, patch_size: int, pad: int) -> List[TileWindow]:
    """the tiles of get_patches / reconstruct_from_patches (model/utils.py:133-193) over a tensor of `shape` = ([D,] H, W), without
    the padded array: tile n is the window of `patch_size` at tile_origins()[n] of the tensor zero-padded by `pad` -- in the
    coordinates of the tensor itself it starts at origin - pad and, like a slice of the padded array, ends no later than the far
    face + pad --, and its scores less a halo of `pad` go to the grid origin.  In the order of tile_origins.  Host geometry only."""
    step = patch_size - 2 * pad
    if step <= 0:
        raise ValueError(f'patch_size {patch_size} does not exceed twice the halo {pad}')
    shape = tuple(int(n) for n in shape)
    out = []
    for origin in tile_origins(shape, step):
        grid = tuple(o for o in origin if o is not None)
        extent = tuple(min(patch_size, n + 2 * pad - o) for o, n in zip(grid, shape))
        out.append(TileWindow(tuple(o - pad for o in grid), extent, grid, tuple(e - 2 * pad for e in extent)))
    return out


def predict_in_patches_device(model, x_dev: torch.Tensor, patch_size: int, is_3d: bool = False,
                              out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """predict_in_patches with everything left on the device: x_dev, [(D,)H,W] with any number of leading axes of length 1, ->
    the stitched scores as a device tensor of the same shape and `out_dtype` (float32: the values of the reference's float64
    map, which are float32 numbers; float64: that map itself).
    The image is neither padded nor copied: tpz_tile_flags tests every tile of the grid for get_patches' all-zero rule in one
    launch and the flags come back in ONE readback, before any tile is scored; then, per tile, tpz_tile_cut makes the
    zero-padded window, the filled model scores it and tpz_tile_paste puts the scores less their halo into the map -- no
    synchronisation, no ATen copy.  The all-zero-tile quirk is kept: get_patches skips such tiles (:159,165) while
    reconstruct_from_patches does not know about it and runs out of tiles -- the same IndexError here."""
    from .. import runtime as rt
    pad = model.width // 2
    dims = 3 if is_3d else 2
    if patch_size - 2 * pad <= 0:
        raise ValueError(f'patch_size {patch_size} does not exceed the receptive field {model.width}')
    if out_dtype not in (torch.float32, torch.float64):
        raise ValueError(f'the stitched map is float32 or float64, not {out_dtype}')
    shape = tuple(x_dev.shape[-dims:])
    if x_dev.dim() < dims or tuple(x_dev.shape[:-dims]) != (1,) * (x_dev.dim() - dims):
        raise ValueError(f'one {"volume" if is_3d else "image"} is needed, got {tuple(x_dev.shape)}')
    ctx = model.device_model.ctx
    x = rt.as_device_f32(x_dev, ctx).reshape(shape)
    windows = tile_windows(shape, patch_size, pad)
    flags = rt.tile_flags(x, [w.origin for w in windows], (patch_size,) * dims, ctx).cpu()
    if not bool(flags.all()):
        # upstream stitches patches[idx] for every slot of the grid and runs past the end of the kept tiles
        raise IndexError('list index out of range (an all-zero tile was skipped: topaz/model/utils.py:159,181-191)')
    out = torch.zeros(shape, dtype=out_dtype, device=ctx.torch_device())
    for w in windows:
        tile = rt.tile_cut(x, w.origin, w.extent, ctx)
        with torch.no_grad():
            s = model(tile[None, None])[0, 0]
        rt.tile_paste(s, (pad,) * dims, w.pasted, out, w.paste, ctx)
    return out.reshape(tuple(x_dev.shape))


def predict_in_patches(model, X: torch.Tensor, patch_size: int, is_3d: bool = False, use_cuda: bool = True) -> np.ndarray:
    """X: [1,1,(D,)H,W] host or device tensor -> float64 array of the same shape (model/utils.py:110-130): tiles of
    `patch_size` cut from the image padded by width // 2 at stride patch_size - 2 * (width // 2); the filled model pads each
    tile again, its scores are cropped by width // 2 and stitched.
    The image goes to the device ONCE; predict_in_patches_device does the rest there into a float64 map, which comes back in
    one copy (upstream moves every tile on and off the GPU)."""
    dev = model.device_model.ctx.torch_device()
    return predict_in_patches_device(model, X.to(device=dev, dtype=torch.float32), patch_size, is_3d, torch.float64).cpu().numpy()
