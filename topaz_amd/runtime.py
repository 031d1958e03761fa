"""Thin Python objects over the C-ABI: one Context per GPU, DeviceModel = a loaded layer program.

PyTorch is used only as plumbing: device memory (tensors), the current HIP stream and
torch.distributed.  All arithmetic of the hot path happens inside libtopaz_hip.so.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import TpzLayer, check, load_library

_contexts = {}

# The bar of the precision check (DeviceModel.calibrate, `--precision-check`): the project's parity contract -- scores and
# denoised pixels within 1e-4 absolute of the reference -- applied to the distance between a model's 2xf16 and fp32 results.
# This is the one place it lives; it is read when a check runs.
DEFAULT_BAR = 1e-4

# The encodings a float32 result can leave the device in (tpz_encode, Stage.download_encoded) and the dtype each is stored as
ENC_F16, ENC_U8 = _lib.TPZ_ENC_F16, _lib.TPZ_ENC_U8
ENC_DTYPES = {ENC_F16: np.dtype(np.float16), ENC_U8: np.dtype(np.uint8)}
# The tile walks Context.walk_stats() counts 2xf16 conv launches by, in the order of tpz_ctx_walk_stats
WALKS = ('plain', 'raster', 'persistent', 'weights_resident', 'multi')


class Context:
    """tpz_ctx for one device.  Use get_context(device) rather than constructing directly."""

    def __init__(self, device: int = 0):
        if not torch.cuda.is_available():
            raise _lib.TopazHipError('no HIP device visible: topaz_amd needs an MI355X (gfx950); there is no CPU path')
        self.lib = load_library()
        self.device = int(device)
        h = C.c_void_p()
        check(self.lib.tpz_ctx_create(self.device, C.byref(h)))
        self.handle = h
        self._bound_stream = None
        self._poison = self.poison_stats()['on']        # (TPZ_DEBUG=1 TPZ_POISON=1: on from the start)

    def bind_current_stream(self) -> None:
        """run subsequent calls on torch's current stream for this device"""
        s = torch.cuda.current_stream(self.device).cuda_stream
        if s != self._bound_stream:
            check(self.lib.tpz_ctx_set_stream(self.handle, C.c_void_p(s)), self.handle)
            self._bound_stream = s

    def sync(self) -> None:
        check(self.lib.tpz_ctx_sync(self.handle), self.handle)

    def torch_device(self) -> torch.device:
        return torch.device('cuda', self.device)

    # ---- profiling counters (HIP events around every launch of a kernel class)
    def prof_enable(self, on=True) -> None:
        """True / 1: time every launch; 2: only convolution launches of >= 20 GFLOP; False / 0: off"""
        check(self.lib.tpz_prof_enable(self.handle, int(on)), self.handle)

    def prof_reset(self) -> None:
        check(self.lib.tpz_prof_reset(self.handle), self.handle)

    def set_exact(self, on: bool = True) -> None:
        """pin the fp32 MFMA kernels (no 2xf16 path) for models run on this context"""
        check(self.lib.tpz_ctx_set_exact(self.handle, 1 if on else 0), self.handle)

    def set_lanes(self, on=True) -> None:
        """patch lanes of tpz_denoise_2d / _3d (two auxiliary streams; an int 2 .. 4: that many); off: every launch on the ctx stream"""
        check(self.lib.tpz_ctx_set_lanes(self.handle, int(on)), self.handle)

    def set_tiling(self, limit_px: int = 40 << 20, tile: int = 4096) -> None:
        """internal tiling of the scoring pass: images above `limit_px` pixels are scored in tile^2 tiles with a receptive-field halo"""
        check(self.lib.tpz_ctx_set_tiling(self.handle, int(limit_px), int(tile)), self.handle)

    def set_raster(self, on: bool = True) -> None:
        """patch raster of the large 8-wave conv launches: each XCD walks 8 x 4 blocks of neighbouring tiles (default on)"""
        check(self.lib.tpz_ctx_set_raster(self.handle, 1 if on else 0), self.handle)

    def set_range(self, on: bool = True) -> None:
        """range scaling of the scoring pass: run on x * 2^-s with the biases scaled alike when max|x| > 32 (default on)"""
        check(self.lib.tpz_ctx_set_range(self.handle, 1 if on else 0), self.handle)

    def set_batch(self, n: int = 8) -> None:
        """patches / tiles per batched launch of tpz_denoise_2d / _3d on the 2xf16 path (0: off, the patch lanes instead)"""
        check(self.lib.tpz_ctx_set_batch(self.handle, int(n)), self.handle)

    def set_batch_memory(self, nbytes: int = 0) -> None:
        """device bytes a batched denoise pass may take for its per-image workspaces (0: 90 % of the free memory)"""
        check(self.lib.tpz_ctx_set_batch_memory(self.handle, int(nbytes)), self.handle)

    def launches(self) -> int:
        """kernel launches issued on this context so far (convolutions and elementwise)"""
        return int(self.lib.tpz_prof_launches(self.handle))

    def pool_stats(self) -> dict:
        """workspace buffers cached by all pools of this context (ctx, lane and batched-pass pools), their bytes, and how many
        are marked in use -- 0 between calls"""
        n, b, u = C.c_longlong(), C.c_longlong(), C.c_longlong()
        check(self.lib.tpz_ctx_pool_stats(self.handle, C.byref(n), C.byref(b), C.byref(u)), self.handle)
        return {'buffers': n.value, 'bytes': b.value, 'buffers_in_use': u.value}

    def set_poison(self, on: bool = True) -> None:
        """poisoned workspace, for tests: every temporary buffer the library takes is filled whole with 0xFF bytes first, and the
        result tensors this module allocates with NaN (_result), so that a cell nothing writes shows in the result (default off)"""
        check(self.lib.tpz_ctx_set_poison(self.handle, 1 if on else 0), self.handle)
        self._poison = bool(on)

    def poison_stats(self) -> dict:
        """whether the poison switch is on, the workspace fills made and the bytes filled since the context was created"""
        on, n, b = C.c_int(), C.c_longlong(), C.c_longlong()
        check(self.lib.tpz_ctx_poison_stats(self.handle, C.byref(on), C.byref(n), C.byref(b)), self.handle)
        return {'on': bool(on.value), 'fills': n.value, 'bytes': b.value}

    def walk_stats(self) -> dict:
        """2xf16 conv launches since the context was created, by tile walk (tpz_ctx_walk_stats)"""
        out = (C.c_longlong * 5)()
        check(self.lib.tpz_ctx_walk_stats(self.handle, out), self.handle)
        return dict(zip(WALKS, (int(v) for v in out)))

    def workspace_peek(self, nbytes: int) -> np.ndarray:
        """what a driver taking `nbytes` of workspace from the ctx pool would find: the buffer's first nbytes, rounded up to a
        whole MiB, as uint8 (tpz_debug_workspace_peek)"""
        self.bind_current_stream()
        out = np.empty((max(int(nbytes), 1) + (1 << 20) - 1) >> 20 << 20, dtype=np.uint8)
        check(self.lib.tpz_debug_workspace_peek(self.handle, int(nbytes), out.ctypes.data_as(C.c_void_p)), self.handle)
        return out

    def set_roi(self, on: bool = True) -> None:
        """patch windows of tpz_denoise_2d: each layer of a patch computes only what the kept centre depends on (default on)"""
        check(self.lib.tpz_ctx_set_roi(self.handle, 1 if on else 0), self.handle)

    def set_rw(self, on: bool = True) -> None:
        """the weights-resident kernel for the 3x3 32 -> 32 layers of the 32-unit detectors (csrc/conv_rw.h; default on)"""
        check(self.lib.tpz_ctx_set_rw(self.handle, 1 if on else 0), self.handle)

    def set_persist(self, mode: int = 1, workgroups: int = 0) -> None:
        """persistent workgroups of the 2xf16 convolutions: 0 never, 1 large launches (default), 2 every eligible launch with
        `workgroups` workgroups (0: one per grid slot)"""
        check(self.lib.tpz_ctx_set_persist(self.handle, int(mode), int(workgroups)), self.handle)

    def delta_stats(self, a: torch.Tensor, b: torch.Tensor) -> dict:
        """tpz_delta_stats of two fp32 device tensors of the same size: max |a - b| (a non-finite difference counts as inf), the
        first flat index that attains it, max |b| and the float64 sum of (a - b)^2; deterministic"""
        self.bind_current_stream()
        a, b = as_device_f32(a, self).reshape(-1), as_device_f32(b, self).reshape(-1)
        if a.numel() != b.numel():
            raise ValueError(f'delta_stats: {a.numel()} against {b.numel()} elements')
        out = _lib.TpzDelta()
        check(self.lib.tpz_delta_stats(self.handle, _ptr(a), _ptr(b), a.numel(), C.byref(out)), self.handle)
        return _delta_dict(out)

    def prof_get(self, cls: int) -> Tuple[float, int, float]:
        ms, n, fl = C.c_double(), C.c_longlong(), C.c_double()
        check(self.lib.tpz_prof_get(self.handle, cls, C.byref(ms), C.byref(n), C.byref(fl)), self.handle)
        return ms.value, n.value, fl.value


def _delta_dict(d: '_lib.TpzDelta') -> dict:
    return {'max_abs_delta': float(d.max_abs_delta), 'max_abs_ref': float(d.max_abs_ref), 'argmax': int(d.argmax),
            'sum_sq': float(d.sum_sq)}


def _prof_get_dominant(self):
    """(name, total ms, launches, algorithmic FLOP) of the conv_mfma instantiation with the most time"""
    ms, n, fl = C.c_double(), C.c_longlong(), C.c_double()
    buf = C.create_string_buffer(256)
    check(self.lib.tpz_prof_get_dominant(self.handle, C.byref(ms), C.byref(n), C.byref(fl), buf, 256), self.handle)
    return buf.value.decode(), ms.value, n.value, fl.value


def _prof_kernels(self):
    """[(name, total ms, launches, FLOP)] of every conv_mfma instantiation launched since the last reset,
    by accumulated time"""
    out = []
    while True:
        ms, n, fl = C.c_double(), C.c_longlong(), C.c_double()
        buf = C.create_string_buffer(256)
        check(self.lib.tpz_prof_get_kernel(self.handle, len(out), C.byref(ms), C.byref(n), C.byref(fl), buf, 256),
              self.handle)
        if not buf.value:
            return out
        out.append((buf.value.decode(), ms.value, n.value, fl.value))


def _prof_kernels_bytes(self):
    """[(name, total ms, launches, FLOP, algorithmic HBM bytes)]: prof_kernels() plus the bytes each instantiation's launches
    read and wrote once (inputs with halo, weights, outputs) -- the bandwidth of the HBM-bound kernels"""
    out = []
    for rank, (name, ms, n, fl) in enumerate(self.prof_kernels()):
        b = C.c_double()
        check(self.lib.tpz_prof_get_kernel_bytes(self.handle, rank, C.byref(b)), self.handle)
        out.append((name, ms, n, fl, b.value))
    return out


def _mfma_sustained(self, ms: int = 300, zero_operands: bool = False):
    """(dense f16 TFLOP/s, s_memtime / s_memrealtime tick ratio) of a register-resident v_mfma_f32_16x16x32_f16 loop on every SIMD"""
    tf, ratio = C.c_double(), C.c_double()
    check(self.lib.tpz_prof_mfma_sustained(self.handle, int(ms), int(bool(zero_operands)), C.byref(tf), C.byref(ratio)), self.handle)
    return tf.value, ratio.value


Context.mfma_sustained = _mfma_sustained
Context.prof_get_dominant = _prof_get_dominant
Context.prof_kernels = _prof_kernels
Context.prof_kernels_bytes = _prof_kernels_bytes


def get_context(device: Optional[int] = None) -> Context:
    if device is None or device < 0:
        device = torch.cuda.current_device() if torch.cuda.is_available() else 0
    key = device
    ctx = _contexts.get(key)
    if ctx is None:
        ctx = Context(device)
        _contexts[key] = ctx
    ctx.bind_current_stream()
    return ctx


def _ptr(t: torch.Tensor) -> C.c_void_p:
    return C.c_void_p(t.data_ptr())


def _result(ctx: Context, shape, dtype=torch.float32) -> torch.Tensor:
    """an uninitialised tensor on the ctx device for a result the library stores straight into; under Context.set_poison it is
    filled with NaN (integers: all ones) on the current stream first, as the library's own workspace is"""
    y = torch.empty(tuple(shape), dtype=dtype, device=ctx.torch_device())
    if ctx._poison:
        y.fill_(float('nan') if dtype.is_floating_point else (255 if dtype == torch.uint8 else -1))
    return y


def as_device_f32(x, ctx: Context) -> torch.Tensor:
    """numpy / tensor -> contiguous fp32 tensor on the ctx device"""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    return x.to(device=ctx.torch_device(), dtype=torch.float32).contiguous()


class Stage:
    """tpz_stage: ring of (pinned host buffer, device buffer) slots with a copy stream of its own.  The H2D copy of the
    next image and the D2H copy of the previous result run under the current image's kernels (include/topaz_hip.h)."""

    def __init__(self, ctx: Context, slot_bytes: int, depth: int = 2):
        self.ctx, self.slot_bytes, self.depth = ctx, int(slot_bytes), int(depth)
        h = C.c_void_p()
        check(ctx.lib.tpz_stage_create(ctx.handle, self.slot_bytes, self.depth, C.byref(h)), ctx.handle)
        self.handle = h

    def close(self) -> None:
        if self.handle:
            self.ctx.lib.tpz_stage_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def host_array(self, slot: int, shape, dtype=np.float32) -> np.ndarray:
        """numpy view of slot's pinned buffer (fill it, then upload())"""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        assert n <= self.slot_bytes
        p = self.ctx.lib.tpz_stage_host_ptr(self.handle, slot)
        buf = (C.c_char * n).from_address(p)
        return np.frombuffer(buf, dtype=dtype).reshape(shape)

    def device_tensor(self, slot: int, shape) -> torch.Tensor:
        """fp32 tensor aliasing slot's device buffer (valid between acquire() and release())"""
        n = int(np.prod(shape))
        assert 4 * n <= self.slot_bytes
        p = self.ctx.lib.tpz_stage_device_ptr(self.handle, slot)
        holder = _DevPtr(p, 4 * n)
        return torch.as_tensor(holder, device=self.ctx.torch_device()).view(torch.float32).reshape(shape)

    def upload(self, slot: int, nbytes: int, src: Optional[np.ndarray] = None) -> None:
        ptr = None if src is None else np.ascontiguousarray(src).ctypes.data_as(C.c_void_p)
        check(self.ctx.lib.tpz_stage_h2d(self.handle, slot, ptr, int(nbytes)), self.ctx.handle)

    @staticmethod
    def decode_bytes(ctx: Context, mode: int, n: int) -> int:
        """bytes a slot needs for upload_decode of n pixels of MRC mode `mode`: the fp32 image plus, behind it, the stored pixels"""
        need = int(ctx.lib.tpz_stage_decode_bytes(int(mode), int(n)))
        if need == 0 and n:
            raise _lib.TopazHipError(f'MRC mode {mode} is not a stored type the device decodes (0, 1, 6, 12)')
        return need

    def upload_decode(self, slot: int, mode: int, n: int) -> None:
        """upload() for n pixels that lie in the slot's pinned buffer in their stored type (host_array(slot, shape, dtype) filled
        them): n * itemsize bytes cross to the device and are decoded to fp32 at the start of the slot on the copy stream
        (tpz_stage_h2d_decode); acquire() / device_tensor() as after upload()"""
        check(self.ctx.lib.tpz_stage_h2d_decode(self.handle, slot, int(mode), int(n)), self.ctx.handle)

    def acquire(self, slot: int) -> None:
        self.ctx.bind_current_stream()
        check(self.ctx.lib.tpz_stage_acquire(self.handle, slot), self.ctx.handle)

    def release(self, slot: int) -> None:
        check(self.ctx.lib.tpz_stage_release(self.handle, slot), self.ctx.handle)

    def download(self, slot: int, src: torch.Tensor) -> None:
        check(self.ctx.lib.tpz_stage_d2h(self.handle, slot, _ptr(src), src.numel() * src.element_size()), self.ctx.handle)

    @staticmethod
    def encode_bytes(ctx: Context, enc: int, n: int) -> int:
        """bytes a slot needs for download_encoded of n pixels: the encoded pixels and, behind them, the overflow counter"""
        need = int(ctx.lib.tpz_stage_encode_bytes(int(enc), int(n)))
        if need == 0:
            raise _lib.TopazHipError(f'encoding {enc} is neither ENC_F16 nor ENC_U8')
        return need

    def download_encoded(self, slot: int, src: torch.Tensor, enc: int, params=None) -> None:
        """download() of a float32 tensor in the type a file stores it in (tpz_stage_d2h_encode): ENC_F16, the float16 of numpy's
        astype, or ENC_U8 with params = (mi, ma), the uint8 of utils.image.quantize.  The pixels are encoded on the copy stream
        and 2 or 1 bytes per pixel cross to the pinned slot; after wait(), host_array(slot, shape, ENC_DTYPES[enc]) holds them
        and overflow_count(slot, n, enc) the number of finite values float16 stored as +-inf."""
        if src.dtype != torch.float32 or not src.is_contiguous():
            raise _lib.TopazHipError('download_encoded: a contiguous float32 tensor is needed')
        p = None if params is None else (C.c_float * 2)(float(params[0]), float(params[1]))
        check(self.ctx.lib.tpz_stage_d2h_encode(self.handle, slot, _ptr(src), src.numel(), int(enc), p), self.ctx.handle)

    def overflow_count(self, slot: int, n: int, enc: int) -> int:
        """the counter download_encoded left behind the n encoded pixels of the slot (read it after wait())"""
        off = self.encode_bytes(self.ctx, enc, n) - 256
        p = self.ctx.lib.tpz_stage_host_ptr(self.handle, slot)
        return int(C.c_ulonglong.from_address(p + off).value)

    def wait(self, slot: int) -> None:
        check(self.ctx.lib.tpz_stage_wait(self.handle, slot), self.ctx.handle)


class _DevPtr:
    """__cuda_array_interface__ holder for a raw device pointer owned by the library"""

    def __init__(self, ptr: int, nbytes: int):
        self.__cuda_array_interface__ = {'shape': (nbytes,), 'typestr': '|u1', 'data': (int(ptr), False), 'version': 3}


def score_host(model: 'DeviceModel', x: np.ndarray) -> np.ndarray:
    """tpz_score_2d_host: numpy image in, numpy logits out (synchronous; staging inside the library)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    H, W = x.shape
    model.ctx.bind_current_stream()
    Do, Ho, Wo = model.out_shape(1, H, W)
    y = np.empty((Ho, Wo), dtype=np.float32)
    check(model.ctx.lib.tpz_score_2d_host(model.handle, x.ctypes.data_as(C.c_void_p), H, W, y.ctypes.data_as(C.c_void_p)),
          model.ctx.handle)
    return y


def denoise_host(model: 'DeviceModel', x: np.ndarray, patch: int, pad: int) -> np.ndarray:
    x = np.ascontiguousarray(x, dtype=np.float32)
    H, W = x.shape
    model.ctx.bind_current_stream()
    y = np.empty_like(x)
    check(model.ctx.lib.tpz_denoise_2d_host(model.handle, x.ctypes.data_as(C.c_void_p), H, W, int(patch), int(pad),
                                            y.ctypes.data_as(C.c_void_p)), model.ctx.handle)
    return y


def nms_host(x: np.ndarray, r: int, threshold: float, ctx: Optional[Context] = None):
    """tpz_nms_2d_host: numpy score map in, (scores, coords) numpy arrays out"""
    ctx = ctx or get_context()
    ctx.bind_current_stream()
    x = np.ascontiguousarray(x, dtype=np.float32)
    H, W = x.shape
    cap = x.size if r < 1 else max(1024, min(x.size, (4 * x.size) // max(1, r * r) + 1024))
    thr = float(threshold)
    if thr == float('-inf'):
        thr = -3.4028234663852886e38 * 2
    while True:
        coords = np.empty((cap, 2), dtype=np.int32)
        scores = np.empty((cap,), dtype=np.float32)
        n = C.c_int(0)
        rc = ctx.lib.tpz_nms_2d_host(ctx.handle, x.ctypes.data_as(C.c_void_p), H, W, int(r), thr,
                                     coords.ctypes.data_as(C.c_void_p), scores.ctypes.data_as(C.c_void_p), cap, C.byref(n))
        if rc != 0 and n.value > cap:
            cap = n.value
            continue
        check(rc, ctx.handle)
        return scores[:n.value].copy(), coords[:n.value].copy()


class LayerProgram:
    """Host-side builder of the tpz_layer list + weight blob (the model manifest)."""

    def __init__(self, dims: int = 2):
        self.dims = dims
        self.layers: List[TpzLayer] = []
        self.blob: List[np.ndarray] = []
        self.n_floats = 0
        self.n_slots = 1          # slot 0 = input

    def new_slot(self) -> int:
        s = self.n_slots
        self.n_slots += 1
        return s

    def _push(self, a) -> int:
        a = np.ascontiguousarray(np.asarray(a, dtype=np.float32).ravel())
        off = self.n_floats
        self.blob.append(a)
        self.n_floats += a.size
        return off

    def conv(self, src: int, weight, bias=None, dil: int = 1, pad: int = 0, slope: float = 1.0, src2: int = -1,
             res: int = -1, res_crop: int = 0, post_scale=None, post_shift=None, head_w=None, head_b=None,
             dst: Optional[int] = None) -> int:
        w = np.asarray(weight, dtype=np.float32)
        cout, cin, k = w.shape[0], w.shape[1], w.shape[-1]
        L = TpzLayer()
        L.op = _lib.TPZ_OP_CONV
        L.dims = self.dims
        L.src, L.src2 = src, src2
        L.dst = self.new_slot() if dst is None else dst
        L.cin, L.cout, L.k, L.dil, L.pad = cin, cout, k, dil, pad
        L.slope = float(slope)
        L.w_off = self._push(w)
        L.b_off = self._push(bias) if bias is not None else -1
        L.res, L.res_crop = res, res_crop
        if post_scale is not None:
            L.post_scale_off = self._push(post_scale)
            L.post_shift_off = self._push(post_shift)
        else:
            L.post_scale_off = L.post_shift_off = -1
        if head_w is not None:
            L.head = 1
            L.head_w_off = self._push(head_w)
            L.head_b_off = self._push(np.asarray([head_b], dtype=np.float32))
        else:
            L.head = 0
            L.head_w_off = L.head_b_off = -1
        self.layers.append(L)
        return L.dst

    def maxpool2(self, src: int) -> int:
        L = TpzLayer()
        L.op = _lib.TPZ_OP_MAXPOOL2
        L.dims = self.dims
        L.src, L.src2, L.res = src, -1, -1
        L.dst = self.new_slot()
        L.w_off = L.b_off = L.post_scale_off = L.post_shift_off = L.head_w_off = L.head_b_off = -1
        L.slope = 1.0
        self.layers.append(L)
        return L.dst

    def maxpool(self, src: int, k: int = 3, dil: int = 1, pad: int = 0) -> int:
        """k^dims max over a window dilated by `dil`, stride 1, `pad` elements of -inf padding (TPZ_OP_MAXPOOL: a filled
        MaxPool(k, stride); pad = 1 needs k = 3 and is the pool of a conv31/63/127 stack trained with --pooling max)"""
        return self._pool(_lib.TPZ_OP_MAXPOOL, src, k, dil, pad)

    def avgpool(self, src: int) -> int:
        """3^dims mean, stride 1, one element of zero padding, divisor 3^dims (TPZ_OP_AVGPOOL: the filled AvgPool(3, stride 2,
        padding 1) of a conv31/63/127 stack trained with --pooling avg)"""
        return self._pool(_lib.TPZ_OP_AVGPOOL, src, 3, 1, 1)

    def _pool(self, op: int, src: int, k: int, dil: int, pad: int) -> int:
        L = TpzLayer()
        L.op = op
        L.dims = self.dims
        L.src, L.src2, L.res = src, -1, -1
        L.dst = self.new_slot()
        L.k, L.dil, L.pad = k, dil, pad
        L.w_off = L.b_off = L.post_scale_off = L.post_shift_off = L.head_w_off = L.head_b_off = -1
        L.slope = 1.0
        self.layers.append(L)
        return L.dst

    def out_shape(self, D: int, H: int, W: int) -> Tuple[int, int, int]:
        """size of the program's output for a D x H x W input (D = 1 in 2-D), as tpz_model_out_shape computes it on the device
        side: a conv or pool with window k, dilation dil and padding pad maps n to n + 2 * pad - dil * (k - 1), MAXPOOL2 to n // 2"""
        shapes = {0: (D, H, W)}
        for L in self.layers:
            d, h, w = shapes[L.src2 if L.op == _lib.TPZ_OP_CONV and L.src2 >= 0 else L.src]
            if L.op == _lib.TPZ_OP_MAXPOOL2:
                o = (d // 2 if L.dims == 3 else 1, h // 2, w // 2)
            else:
                grow = 2 * L.pad - L.dil * (L.k - 1)
                o = (d + grow if L.dims == 3 else 1, h + grow, w + grow)
            shapes[L.dst] = o
        return shapes[self.layers[-1].dst]

    def flat_blob(self) -> np.ndarray:
        if not self.blob:
            return np.zeros(1, dtype=np.float32)
        return np.concatenate(self.blob).astype(np.float32, copy=False)


class DeviceModel:
    """tpz_model: weights packed into MFMA fragment order and resident in HBM."""

    def __init__(self, program: LayerProgram, ctx: Optional[Context] = None):
        self.ctx = ctx or get_context()
        self.dims = program.dims
        lib = self.ctx.lib
        n = len(program.layers)
        arr = (TpzLayer * n)(*program.layers)
        blob = program.flat_blob()
        h = C.c_void_p()
        check(lib.tpz_model_load(self.ctx.handle, arr, n, blob.ctypes.data_as(C.c_void_p), blob.size, C.byref(h)),
              self.ctx.handle)
        self.handle = h
        n_conv, n_split, off = self.split_layers()
        if 0 < n_split < n_conv:
            import warnings
            warnings.warn(f'topaz_amd: {n_conv - n_split} of {n_conv} convolution layers of this model have no 2xf16 kernel and run '
                          f'on the fp32 matrix-core kernels (correct, several times slower): {off}', RuntimeWarning, stacklevel=3)

    def split_layers(self) -> Tuple[int, int, str]:
        """(convolution layers, those on the 2xf16 path, description of the others)"""
        a, b = C.c_int(), C.c_int()
        buf = C.create_string_buffer(512)
        check(self.ctx.lib.tpz_model_split_layers(self.handle, C.byref(a), C.byref(b), buf, 512), self.ctx.handle)
        return a.value, b.value, buf.value.decode()

    def __del__(self):
        try:
            if getattr(self, 'handle', None):
                self.ctx.lib.tpz_model_free(self.handle)
                self.handle = None
        except Exception:
            pass

    def out_shape(self, D: int, H: int, W: int) -> Tuple[int, int, int]:
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        check(self.ctx.lib.tpz_model_out_shape(self.handle, D, H, W, C.byref(a), C.byref(b), C.byref(c)),
              self.ctx.handle)
        return a.value, b.value, c.value

    def split_stats(self) -> Tuple[bool, int, int]:
        """(eligible for the 2xf16 path, images finished on it, images re-run on the fp32 kernels)"""
        e, a, b = C.c_int(), C.c_longlong(), C.c_longlong()
        check(self.ctx.lib.tpz_model_split_stats(self.handle, C.byref(e), C.byref(a), C.byref(b)), self.ctx.handle)
        return bool(e.value), a.value, b.value

    def _batch_input(self, x) -> Tuple[torch.Tensor, int, int, int, int, Tuple[int, int, int]]:
        """x: [N,1,(D,)H,W] (or without the channel axis) -> (fp32 tensor on the ctx device, N, D, H, W, output size)"""
        nd = self.dims
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x))
        if x.dim() == nd + 1:
            x = x.unsqueeze(1)
        if x.dim() != nd + 2 or x.shape[1] != 1:
            raise ValueError(f'expected [N,1,{"D,H,W" if nd == 3 else "H,W"}] input, got {tuple(x.shape)}')
        x = as_device_f32(x, self.ctx)
        N = x.shape[0]
        D = x.shape[2] if nd == 3 else 1
        H, W = x.shape[-2], x.shape[-1]
        Do, Ho, Wo = self.out_shape(D, H, W)
        if min(Do, Ho, Wo) < 1:
            raise ValueError(f'input {tuple(x.shape)} is too small for this model')
        return x, N, D, H, W, (Do, Ho, Wo)

    def calibrate(self, x, bar: Optional[float] = None) -> dict:
        """tpz_model_calibrate: the 2xf16 error of this model on the image x (any layout forward takes, N = 1) against its own
        fp32 result.  Returns eligible / overflow / tripped (bools), max_abs_delta, max_abs_ref, argmax (flat index into the
        output), sum_sq, rms_delta and the bar.  bar None: DEFAULT_BAR; a max_abs_delta above a bar > 0 pins this model to the
        fp32 kernels (`exact`, tripped = True); bar <= 0 only measures.  No counter of split_stats() moves."""
        self.ctx.bind_current_stream()
        x, N, D, H, W, _ = self._batch_input(x)
        if N != 1:
            raise ValueError(f'calibrate takes one image, got a batch of {N}')
        bar = DEFAULT_BAR if bar is None else float(bar)
        out = _lib.TpzCalibration()
        check(self.ctx.lib.tpz_model_calibrate(self.handle, _ptr(x), D, H, W, bar, C.byref(out)), self.ctx.handle)
        r = _delta_dict(out.d)
        r.update(eligible=bool(out.eligible), overflow=bool(out.overflow), tripped=bool(out.tripped),
                 rms_delta=float(out.rms_delta), bar=bar)
        return r

    def set_exact(self, on: bool = True) -> None:
        """pin this model to the fp32 MFMA kernels (tpz_model_set_exact), whatever its context runs otherwise"""
        check(self.ctx.lib.tpz_model_set_exact(self.handle, 1 if on else 0), self.ctx.handle)

    @property
    def exact(self) -> bool:
        on = C.c_int(0)
        check(self.ctx.lib.tpz_model_get_exact(self.handle, C.byref(on)), self.ctx.handle)
        return bool(on.value)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x: [N,1,(D,)H,W] (or without the channel axis) on the ctx device -> [N,1,(Do,)Ho,Wo]"""
        self.ctx.bind_current_stream()
        nd = self.dims
        x, N, D, H, W, (Do, Ho, Wo) = self._batch_input(x)
        co = C.c_int(1)
        check(self.ctx.lib.tpz_model_out_channels(self.handle, C.byref(co)), self.ctx.handle)
        shape = (N, co.value, Do, Ho, Wo) if nd == 3 else (N, co.value, Ho, Wo)
        y = _result(self.ctx, shape)
        check(self.ctx.lib.tpz_model_forward(self.handle, _ptr(x), N, D, H, W, _ptr(y)), self.ctx.handle)
        return y

    def denoise_2d(self, x: torch.Tensor, patch: int, pad: int) -> torch.Tensor:
        self.ctx.bind_current_stream()
        x = as_device_f32(x, self.ctx)
        H, W = x.shape
        y = _result(self.ctx, x.shape)
        check(self.ctx.lib.tpz_denoise_2d(self.handle, _ptr(x), H, W, int(patch), int(pad), _ptr(y)), self.ctx.handle)
        return y

    def denoise_3d(self, x: torch.Tensor, patch: int, pad: int, shard: int = 0, n_shards: int = 1) -> torch.Tensor:
        """n_shards > 1: only this shard's tiles are denoised; the rest of the returned volume is zero (sum the shards)"""
        self.ctx.bind_current_stream()
        x = as_device_f32(x, self.ctx)
        D, H, W = x.shape
        y = _result(self.ctx, x.shape) if n_shards == 1 else torch.zeros_like(x)
        check(self.ctx.lib.tpz_denoise_3d_shard(self.handle, _ptr(x), D, H, W, int(patch), int(pad), int(shard), int(n_shards),
                                                _ptr(y)), self.ctx.handle)
        return y


# ---- single ops ------------------------------------------------------------------------------------
def conv(x: torch.Tensor, weight, bias=None, dil: int = 1, pad: int = 0, slope: float = 1.0,
         x2: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None, res_crop: int = 0,
         post_scale=None, post_shift=None, head_w=None, head_b: float = 0.0,
         ctx: Optional[Context] = None) -> torch.Tensor:
    """One fused convolution through tpz_conv.  x: [C1,(D1,)H1,W1]; x2 (optional, concatenated after the
    nearest-upsampled x): [C2,(D,)H,W].  Returns [Cout,(Do,)Ho,Wo] (or [1,...] with a fused head)."""
    ctx = ctx or get_context()
    ctx.bind_current_stream()
    w = np.ascontiguousarray(np.asarray(weight, dtype=np.float32))
    dims = w.ndim - 2
    x = as_device_f32(x, ctx)
    c1 = x.shape[0]
    D1 = x.shape[1] if dims == 3 else 1
    H1, W1 = x.shape[-2], x.shape[-1]
    if x2 is not None:
        x2 = as_device_f32(x2, ctx)
        D = x2.shape[1] if dims == 3 else 1
        H, W = x2.shape[-2], x2.shape[-1]
        cin = c1 + x2.shape[0]
    else:
        D, H, W, cin = D1, H1, W1, c1
    cout, k = w.shape[0], w.shape[-1]
    assert w.shape[1] == cin, (w.shape, cin)
    span = dil * (k - 1)
    Do = D + 2 * pad - span if dims == 3 else 1
    Ho, Wo = H + 2 * pad - span, W + 2 * pad - span
    co = 1 if head_w is not None else cout
    shape = (co, Do, Ho, Wo) if dims == 3 else (co, Ho, Wo)
    y = _result(ctx, shape)

    def hp(a):
        if a is None:
            return None, C.c_void_p(None)
        a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
        return a, a.ctypes.data_as(C.c_void_p)

    kb, pb = hp(bias)
    ks, ps_ = hp(post_scale)
    kt, pt = hp(post_shift)
    kh, ph = hp(head_w)
    if res is not None:
        res = as_device_f32(res, ctx)
    check(ctx.lib.tpz_conv(ctx.handle, dims, _ptr(x), c1, D1, H1, W1, _ptr(x2) if x2 is not None else C.c_void_p(None),
                           cin, D, H, W, w.ctypes.data_as(C.c_void_p), pb, cout, k, dil, pad, float(slope),
                           _ptr(res) if res is not None else C.c_void_p(None), res_crop, ps_, pt, ph, float(head_b),
                           _ptr(y)), ctx.handle)
    return y


def conv_split(x: torch.Tensor, weight, bias=None, dil: int = 1, pad: int = 0, slope: float = 1.0,
               res: Optional[torch.Tensor] = None, res_crop: int = 0, post_scale=None, post_shift=None,
               head_w=None, head_b: float = 0.0, ctx: Optional[Context] = None) -> Tuple[torch.Tensor, bool]:
    """The same 2-D convolution on the 2xf16 kernels (tpz_conv_split_2d): fp32 tensors in and out, converted
    to split f16 cells on the device.  Returns (y, overflow) -- overflow: a result left the f16 range."""
    ctx = ctx or get_context()
    ctx.bind_current_stream()
    w = np.ascontiguousarray(np.asarray(weight, dtype=np.float32))
    x = as_device_f32(x, ctx)
    cin, H, W = x.shape
    cout, k = w.shape[0], w.shape[-1]
    assert w.ndim == 4 and w.shape[1] == cin, (w.shape, cin)
    span = dil * (k - 1)
    Ho, Wo = H + 2 * pad - span, W + 2 * pad - span
    y = _result(ctx, (1 if head_w is not None else cout, Ho, Wo))

    def hp(a):
        if a is None:
            return None, C.c_void_p(None)
        a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
        return a, a.ctypes.data_as(C.c_void_p)

    kb, pb = hp(bias)
    ks, ps_ = hp(post_scale)
    kt, pt = hp(post_shift)
    kh, ph = hp(head_w)
    if res is not None:
        res = as_device_f32(res, ctx)
    ovf = C.c_int(0)
    check(ctx.lib.tpz_conv_split_2d(ctx.handle, _ptr(x), cin, H, W, w.ctypes.data_as(C.c_void_p), pb, cout, k, dil,
                                    pad, float(slope), _ptr(res) if res is not None else C.c_void_p(None), res_crop,
                                    ps_, pt, ph, float(head_b), _ptr(y), C.byref(ovf)), ctx.handle)
    return y, bool(ovf.value)


def gmm_fit(x, pis, splits, alpha: float = 900.0, beta: float = 1.0, scale: float = 1.0, num_iters: int = 100,
            tol: float = 1e-3, ctx: Optional[Context] = None):
    """tpz_gmm_fit: EM fits of the 2-component pixel mixture for every initialisation (topaz/stats.py:87-203).
    x: pixel values (any array / device tensor); returns (mus, stds, pis, logps) as float64 arrays."""
    ctx = ctx or get_context()
    ctx.bind_current_stream()
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32)))
    x = as_device_f32(x.reshape(-1), ctx)
    pis = np.ascontiguousarray(np.asarray(pis, dtype=np.float64))
    splits = np.ascontiguousarray(np.asarray(splits, dtype=np.float64))
    n = len(pis)
    outs = [np.zeros(n, dtype=np.float64) for _ in range(4)]
    check(ctx.lib.tpz_gmm_fit(ctx.handle, _ptr(x), x.numel(), pis.ctypes.data_as(C.c_void_p),
                              splits.ctypes.data_as(C.c_void_p), n, float(alpha), float(beta), float(scale),
                              int(num_iters), float(tol), *[o.ctypes.data_as(C.c_void_p) for o in outs]), ctx.handle)
    return tuple(outs)


def gmm_fit_fused(x, pis, splits, alpha: float = 900.0, beta: float = 1.0, scale: float = 1.0, num_iters: int = 100,
                  tol: float = 1e-3, ctx: Optional[Context] = None):
    """tpz_gmm_fit_fused: gmm_fit with every initialisation advanced by one pass over the pixels per EM iteration; the same four
    arrays bit for bit, plus the number of passes over x: (mus, stds, pis, logps, n_passes)."""
    ctx = ctx or get_context()
    ctx.bind_current_stream()
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32)))
    x = as_device_f32(x.reshape(-1), ctx)
    pis = np.ascontiguousarray(np.asarray(pis, dtype=np.float64))
    splits = np.ascontiguousarray(np.asarray(splits, dtype=np.float64))
    n = len(pis)
    outs = [np.zeros(n, dtype=np.float64) for _ in range(4)]
    n_passes = C.c_int(0)
    check(ctx.lib.tpz_gmm_fit_fused(ctx.handle, _ptr(x), x.numel(), pis.ctypes.data_as(C.c_void_p),
                                    splits.ctypes.data_as(C.c_void_p), n, float(alpha), float(beta), float(scale),
                                    int(num_iters), float(tol), *[o.ctypes.data_as(C.c_void_p) for o in outs],
                                    C.byref(n_passes)), ctx.handle)
    return tuple(outs) + (int(n_passes.value),)


def order_stats(x: torch.Tensor, ranks, ctx: Optional[Context] = None) -> np.ndarray:
    """tpz_order_stats: the ranks[j]-th smallest (0-based) elements of x, exactly, as a float32 array; at most 32 ranks per call.
    All NaN when x holds a NaN (np.quantile)."""
    ctx = ctx or get_context()
    ctx.bind_current_stream()
    x = as_device_f32(x.reshape(-1), ctx)
    ranks = np.ascontiguousarray(np.asarray(ranks, dtype=np.int64).ravel())
    out = np.zeros(len(ranks), dtype=np.float32)
    check(ctx.lib.tpz_order_stats(ctx.handle, _ptr(x), x.numel(), ranks.ctypes.data_as(C.c_void_p), len(ranks),
                                  out.ctypes.data_as(C.c_void_p)), ctx.handle)
    return out


def gather(x: torch.Tensor, idx, ctx: Optional[Context] = None) -> torch.Tensor:
    """tpz_gather_f32: x.ravel()[idx] on the device; idx: host integers, checked against the size of x before the launch"""
    ctx = ctx or get_context()
    ctx.bind_current_stream()
    x = as_device_f32(x.reshape(-1), ctx)
    idx = np.ascontiguousarray(np.asarray(idx, dtype=np.int64).ravel())
    y = _result(ctx, (len(idx),))
    check(ctx.lib.tpz_gather_f32(ctx.handle, _ptr(x), x.numel(), idx.ctypes.data_as(C.c_void_p), len(idx), _ptr(y)),
          ctx.handle)
    return y


def normalize_f64(x: torch.Tensor, mean: float, std: float, ctx: Optional[Context] = None) -> torch.Tensor:
    """(x - mean) / std as numpy evaluates it for a float32 x and np.float64 scalars (tpz_normalize_f64): in float64, rounded to
    float32 once; std == 0 -> inf / nan"""
    ctx = ctx or get_context()
    ctx.bind_current_stream()
    x = as_device_f32(x, ctx)
    y = _result(ctx, x.shape)
    check(ctx.lib.tpz_normalize_f64(ctx.handle, _ptr(x), x.numel(), float(mean), float(std), _ptr(y)), ctx.handle)
    return y


def maxpool2(x: torch.Tensor, ctx: Optional[Context] = None) -> torch.Tensor:
    ctx = ctx or get_context()
    ctx.bind_current_stream()
    x = as_device_f32(x, ctx)
    dims = x.dim() - 1
    Cc = x.shape[0]
    D = x.shape[1] if dims == 3 else 1
    H, W = x.shape[-2], x.shape[-1]
    shape = (Cc, D // 2, H // 2, W // 2) if dims == 3 else (Cc, H // 2, W // 2)
    y = _result(ctx, shape)
    check(ctx.lib.tpz_maxpool2(ctx.handle, dims, _ptr(x), Cc, D, H, W, _ptr(y)), ctx.handle)
    return y


def pool(x: torch.Tensor, op: str = 'max', dil: int = 1, pad: int = 1, split: bool = False,
         ctx: Optional[Context] = None) -> Tuple[torch.Tensor, bool]:
    """One padded 3^dims pool through tpz_pool.  x: [C,(D,)H,W]; op 'max' (window dilated by dil, -inf padding) or 'avg' (dil = 1,
    pad = 1, zero padding, divisor 3^dims).  split: on split f16 cells (converted on the device either side) instead of fp32 planes.
    Returns ([C,(Do,)Ho,Wo], overflow) -- overflow: split cells could not hold an input value (beyond the f16 range, inf or NaN)."""
    ctx = ctx or get_context()
    ctx.bind_current_stream()
    x = as_device_f32(x, ctx)
    dims = x.dim() - 1
    Cc = x.shape[0]
    D = x.shape[1] if dims == 3 else 1
    H, W = x.shape[-2], x.shape[-1]
    grow = 2 * pad - 2 * dil
    shape = (Cc, D + grow, H + grow, W + grow) if dims == 3 else (Cc, H + grow, W + grow)
    if min(shape) < 1:
        raise ValueError(f'input {tuple(x.shape)} is too small for a 3-tap pool at dilation {dil}, padding {pad}')
    y = _result(ctx, shape)
    ovf = C.c_int(0)
    code = {'max': _lib.TPZ_OP_MAXPOOL, 'avg': _lib.TPZ_OP_AVGPOOL}[op]
    check(ctx.lib.tpz_pool(ctx.handle, code, dims, _ptr(x), Cc, D, H, W, int(dil), int(pad), 1 if split else 0, _ptr(y),
                           C.byref(ovf)), ctx.handle)
    return y, bool(ovf.value)


def mean_std(x: torch.Tensor, unbiased: bool, ctx: Optional[Context] = None) -> Tuple[float, float]:
    ctx = ctx or get_context()
    ctx.bind_current_stream()
    x = as_device_f32(x, ctx)
    out = (C.c_float * 2)()
    check(ctx.lib.tpz_mean_std(ctx.handle, _ptr(x), x.numel(), 1 if unbiased else 0, out), ctx.handle)
    return float(out[0]), float(out[1])


def affine(x: torch.Tensor, scale: float, shift: float, ctx: Optional[Context] = None) -> torch.Tensor:
    ctx = ctx or get_context()
    ctx.bind_current_stream()
    x = as_device_f32(x, ctx)
    y = _result(ctx, x.shape)
    check(ctx.lib.tpz_affine(ctx.handle, _ptr(x), x.numel(), float(scale), float(shift), _ptr(y)), ctx.handle)
    return y


def normalize(x: torch.Tensor, mean: float, std: float, ctx: Optional[Context] = None) -> torch.Tensor:
    """(x - mean) / std as numpy evaluates it in fp32 (tpz_normalize): subtraction first, IEEE division; std == 0 -> inf / nan"""
    ctx = ctx or get_context()
    ctx.bind_current_stream()
    x = as_device_f32(x, ctx)
    y = _result(ctx, x.shape)
    check(ctx.lib.tpz_normalize(ctx.handle, _ptr(x), x.numel(), float(mean), float(std), _ptr(y)), ctx.handle)
    return y


def decode_stored(x: np.ndarray, ctx: Optional[Context] = None) -> torch.Tensor:
    """a numpy array of int8 / int16 / uint16 / float16 pixels -> the fp32 device tensor numpy's astype(np.float32) would give,
    bit for bit (tpz_decode).  The array goes up in its stored type: a quarter or half of the float32 bytes cross the bus and
    the host converts nothing."""
    from .mrc import STORED_MODES
    ctx = ctx or get_context()
    ctx.bind_current_stream()
    x = np.ascontiguousarray(x)
    mode = STORED_MODES.get(x.dtype)
    if mode is None:
        raise _lib.TopazHipError(f'decode_stored: {x.dtype} is not a stored type the device decodes (int8, int16, uint16, '
                                 'float16)')
    raw = torch.from_numpy(x.reshape(-1).view(np.uint8)).to(ctx.torch_device())
    y = _result(ctx, x.shape)
    if x.size:
        check(ctx.lib.tpz_decode(ctx.handle, _ptr(raw), mode, x.size, _ptr(y)), ctx.handle)
    return y


def encode(x: torch.Tensor, enc: int, params=None, ctx: Optional[Context] = None, count: bool = True,
           out: Optional[torch.Tensor] = None):
    """a float32 device tensor -> (the tensor a file stores, overflow count) on the device (tpz_encode): ENC_F16 gives the
    float16 tensor of numpy's astype(np.float16), bit for bit, and the number of finite values stored as +-inf; ENC_U8 with
    params = (mi, ma) the uint8 tensor of utils.image.quantize and 0.  count=False passes no counter (the count returned is
    None); out: a tensor of the stored dtype to write into (its first x.numel() elements; views that are only 2- or 4-byte
    aligned are fine).  x may be any contiguous float32 view."""
    ctx = ctx or get_context()
    ctx.bind_current_stream()
    if enc not in ENC_DTYPES:
        raise _lib.TopazHipError(f'encode: encoding {enc} is neither ENC_F16 nor ENC_U8')
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()):
        x = as_device_f32(x, ctx)
    dtype = torch.float16 if enc == ENC_F16 else torch.uint8
    if out is None:
        out = _result(ctx, x.shape, dtype)
    elif out.dtype != dtype or out.numel() < x.numel() or not out.is_contiguous():
        raise _lib.TopazHipError('encode: `out` must be a contiguous tensor of the stored dtype with room for every pixel')
    counter = torch.zeros(1, dtype=torch.int64, device=x.device) if count and enc == ENC_F16 else None
    p = None if params is None else (C.c_float * 2)(float(params[0]), float(params[1]))
    if x.numel():
        check(ctx.lib.tpz_encode(ctx.handle, _ptr(x), x.numel(), int(enc), p, _ptr(out), None if counter is None else _ptr(counter)),
              ctx.handle)
    return out, (int(counter.item()) if counter is not None else (0 if count else None))


def _dense_f32(x: torch.Tensor, ctx: Context, what: str) -> Tuple[torch.Tensor, int, int, int]:
    """a 2-D or 3-D tensor as the dense fp32 device tensor the tile entry points read (a contiguous view stays the view it is),
    with its (D, H, W)"""
    if x.dim() not in (2, 3):
        raise ValueError(f'{what}: a [H, W] or [D, H, W] tensor is needed, got {tuple(x.shape)}')
    x = as_device_f32(x, ctx)
    return (x, 1) + tuple(x.shape) if x.dim() == 2 else (x,) + tuple(x.shape)


def _zyx(v, dims: int, z: int) -> Tuple[int, int, int]:
    """(z, y, x) of a per-axis triple or pair given in the order of the tensor's axes; the given z for an image"""
    v = tuple(int(a) for a in v)
    if len(v) != dims:
        raise ValueError(f'{dims} coordinates are needed, got {v}')
    return v if dims == 3 else (z,) + v


def tile_cut(x: torch.Tensor, origin, size, ctx: Optional[Context] = None) -> torch.Tensor:
    """tpz_tile_cut: the window of `size` = ([td,] th, tw) of the [D,] H, W tensor x at `origin` = ([z0,] y0, x0) as a dense
    tensor of its own, zero where the window leaves x (the origin may be negative, the window may reach past x or miss it).
    One launch, asynchronous."""
    ctx = ctx or get_context()
    ctx.bind_current_stream()
    x, D, H, W = _dense_f32(x, ctx, 'tile_cut')
    dims = x.dim()
    z0, y0, x0 = _zyx(origin, dims, 0)
    td, th, tw = _zyx(size, dims, 1)
    if min(td, th, tw) < 1:
        raise ValueError(f'tile_cut: size {tuple(size)} must be positive')
    y = _result(ctx, (td, th, tw)[3 - dims:])
    check(ctx.lib.tpz_tile_cut(ctx.handle, _ptr(x), D, H, W, z0, y0, x0, td, th, tw, _ptr(y)), ctx.handle)
    return y


def tile_flags(x: torch.Tensor, origins, size, ctx: Optional[Context] = None) -> torch.Tensor:
    """tpz_tile_flags: int32 device tensor [n], 1 where the window of `size` at origins[t] holds an element of x that is != 0
    (torch's ne(0): NaN counts, -0.0 and what lies outside x do not), for all n windows in ONE launch.  Asynchronous: the
    caller reads the flags back (one .cpu()) when it needs them."""
    ctx = ctx or get_context()
    ctx.bind_current_stream()
    x, D, H, W = _dense_f32(x, ctx, 'tile_flags')
    dims = x.dim()
    td, th, tw = _zyx(size, dims, 1)
    org = np.ascontiguousarray([_zyx(o, dims, 0) for o in origins], dtype=np.int32).reshape(-1, 3)
    flags = _result(ctx, (len(org),), torch.int32)
    check(ctx.lib.tpz_tile_flags(ctx.handle, _ptr(x), D, H, W, org.ctypes.data_as(C.c_void_p), len(org), td, th, tw, _ptr(flags)),
          ctx.handle)
    return flags


def tile_paste(tile: torch.Tensor, crop, extent, canvas: torch.Tensor, at, ctx: Optional[Context] = None) -> None:
    """tpz_tile_paste: the box [crop, crop + extent) per axis of the fp32 tile goes into `canvas` (a contiguous float32 or float64
    device tensor of the tile's dimensionality) at `at`, clipped to the canvas; nothing else of the canvas is written.
    One launch, asynchronous."""
    ctx = ctx or get_context()
    ctx.bind_current_stream()
    tile, td, th, tw = _dense_f32(tile, ctx, 'tile_paste')
    dims = tile.dim()
    if not (canvas.is_cuda and canvas.is_contiguous() and canvas.dim() == dims and canvas.dtype in (torch.float32, torch.float64)):
        raise _lib.TopazHipError('tile_paste: the canvas must be a contiguous float32 / float64 device tensor of the tile\'s rank')
    D, H, W = tuple(canvas.shape) if dims == 3 else (1,) + tuple(canvas.shape)
    cz, cy, cx = _zyx(crop, dims, 0)
    nz, ny, nx = _zyx(extent, dims, 1)
    z, y, x = _zyx(at, dims, 0)
    check(ctx.lib.tpz_tile_paste(ctx.handle, _ptr(tile), td, th, tw, cz, cy, cx, nz, ny, nx, _ptr(canvas),
                                 1 if canvas.dtype == torch.float64 else 0, D, H, W, z, y, x), ctx.handle)


def normalize_cutoff(x: torch.Tensor, mean: float, std: float, cutoff: float, ctx: Optional[Context] = None) -> torch.Tensor:
    """normalize() with denoise_image's pixel cutoff fused (tpz_normalize_cutoff): v = (x - mean) / std, then 0 where
    v < -cutoff or v > cutoff, compared in fp32; NaN passes, +-inf is zeroed; cutoff <= 0 is normalize()"""
    ctx = ctx or get_context()
    ctx.bind_current_stream()
    x = as_device_f32(x, ctx)
    y = _result(ctx, x.shape)
    check(ctx.lib.tpz_normalize_cutoff(ctx.handle, _ptr(x), x.numel(), float(mean), float(std), float(cutoff), _ptr(y)),
          ctx.handle)
    return y


def filter_2d(x: torch.Tensor, w, bias: float = 0.0, ctx: Optional[Context] = None) -> torch.Tensor:
    ctx = ctx or get_context()
    ctx.bind_current_stream()
    x = as_device_f32(x, ctx)
    w = np.ascontiguousarray(np.asarray(w, dtype=np.float32))
    H, W = x.shape
    y = _result(ctx, x.shape)
    check(ctx.lib.tpz_filter_2d(ctx.handle, _ptr(x), H, W, w.ctypes.data_as(C.c_void_p), w.shape[-1], float(bias),
                                _ptr(y)), ctx.handle)
    return y


def lowpass_2d(x: torch.Tensor, qh: np.ndarray, qw: np.ndarray, ctx: Optional[Context] = None) -> torch.Tensor:
    """tpz_lowpass_2d: y = qh (qh^T x qw) qw^T in fp64, rounded to fp32 once.  x [H, W]; qh [H, rh] and qw [W, rw] float64 host
    operators (denoise.lowpass_operator).  The caller keeps qh / qw alive (the operator cache does).  Asynchronous."""
    ctx = ctx or get_context()
    ctx.bind_current_stream()
    x = as_device_f32(x, ctx)
    H, W = x.shape
    assert qh.dtype == np.float64 and qw.dtype == np.float64 and qh.flags.c_contiguous and qw.flags.c_contiguous
    assert qh.shape[0] == H and qw.shape[0] == W
    y = _result(ctx, x.shape)
    check(ctx.lib.tpz_lowpass_2d(ctx.handle, _ptr(x), H, W, qh.ctypes.data_as(C.c_void_p), qh.shape[1],
                                 qw.ctypes.data_as(C.c_void_p), qw.shape[1], _ptr(y)), ctx.handle)
    return y


def spatial_cov_2d(x: torch.Tensor, patch: int = 1, width: int = 11, ctx: Optional[Context] = None) -> np.ndarray:
    """tpz_spatial_cov_2d: the lag covariances of the patch x patch tiles of x -> [patch * patch, width, width] float64 (host)"""
    ctx = ctx or get_context()
    ctx.bind_current_stream()
    x = as_device_f32(x, ctx)
    H, W = x.shape
    cov = np.empty((patch * patch, width, width), dtype=np.float64)
    check(ctx.lib.tpz_spatial_cov_2d(ctx.handle, _ptr(x), H, W, int(patch), int(width), cov.ctypes.data_as(C.c_void_p)),
          ctx.handle)
    return cov


def tile_filter_2d(x: torch.Tensor, w: np.ndarray, patch: int = 1, ctx: Optional[Context] = None) -> torch.Tensor:
    """tpz_tile_filter_2d: zero-padded cross-correlation of x with the fp32 weights w [patch * patch, k, k] of each pixel's tile"""
    ctx = ctx or get_context()
    ctx.bind_current_stream()
    x = as_device_f32(x, ctx)
    H, W = x.shape
    w = np.ascontiguousarray(w, dtype=np.float32)
    assert w.shape == (patch * patch, w.shape[-1], w.shape[-1])
    y = _result(ctx, x.shape)
    check(ctx.lib.tpz_tile_filter_2d(ctx.handle, _ptr(x), H, W, int(patch), w.shape[-1], w.ctypes.data_as(C.c_void_p), _ptr(y)),
          ctx.handle)
    return y


def particle_stack(img: torch.Tensor, xy, size: int, resize: int = -1, ops: Optional[np.ndarray] = None,
                   out: Optional[torch.Tensor] = None, ctx: Optional[Context] = None) -> torch.Tensor:
    """tpz_particle_stack: the standardised size^2 boxes around the picks xy ([n, 2] int (x, y)) of one micrograph img ([H, W] or
    [mz, H, W] on the device) -> [n, mz, R, R] fp32 on the device, R = resize (resize <= 0: size).  ops: the host operators of
    utils.picks.resize_operators(size, resize), needed when R < size.  Asynchronous on the ctx stream."""
    ctx = ctx or get_context()
    ctx.bind_current_stream()
    img = as_device_f32(img, ctx)
    mz, H, W = (1,) + tuple(img.shape) if img.dim() == 2 else tuple(img.shape)
    xy = np.ascontiguousarray(np.asarray(xy, dtype=np.int32).reshape(-1, 2))
    n = xy.shape[0]
    R = int(resize) if resize > 0 else int(size)
    if out is None:
        out = _result(ctx, (n, mz, R, R))
    assert out.is_contiguous() and out.numel() == n * mz * R * R
    if ops is not None:
        ops = np.ascontiguousarray(ops, dtype=np.float32)
    check(ctx.lib.tpz_particle_stack(ctx.handle, _ptr(img), mz, H, W, xy.ctypes.data_as(C.c_void_p), n, int(size), R,
                                     ops.ctypes.data_as(C.c_void_p) if ops is not None else C.c_void_p(None), _ptr(out)),
          ctx.handle)
    return out


def nms(score: torch.Tensor, r: int, threshold: float, scale: float = 1.0, ctx: Optional[Context] = None,
        cap: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """device NMS.  score [H,W] or [D,H,W]; returns (scores[n] fp32, coords[n,dims] int32 (x,y[,z])) on device"""
    ctx = ctx or get_context()
    ctx.bind_current_stream()
    score = as_device_f32(score, ctx)
    dims = score.dim()
    n_el = score.numel()
    if cap is None:
        # a pick suppresses at least itself; with r >= 1 picks are > r apart, so this bound is generous
        cap = n_el if r < 1 else max(1024, min(n_el, (4 * n_el) // max(1, r * r) + 1024))
    while True:
        coords = _result(ctx, (cap, dims), torch.int32)
        out = _result(ctx, (cap,))
        n = C.c_int(0)
        thr = float(threshold)
        if thr == float('-inf'):
            thr = -3.4028234663852886e38 * 2   # passes through c_float as -inf
        if dims == 2:
            H, W = score.shape
            rc = ctx.lib.tpz_nms_2d(ctx.handle, _ptr(score), H, W, int(r), thr, _ptr(coords), _ptr(out), cap,
                                    C.byref(n))
        else:
            D, H, W = score.shape
            rc = ctx.lib.tpz_nms_3d(ctx.handle, _ptr(score), D, H, W, int(r), float(scale), thr, _ptr(coords),
                                    _ptr(out), cap, C.byref(n))
        if rc != 0 and n.value > cap:
            cap = n.value          # capacity guess too small: rerun with the exact size
            continue
        check(rc, ctx.handle)
        return out[:n.value], coords[:n.value]


class ResamplePlan:
    """tpz_resample: the two operators of one truncated-DFT reduction (M, N) -> (m, n), packed and resident in HBM.  L [2m, M] and
    R [n, 2N] are the float32 host operators of utils.image._downsample_operators; they are uploaded here, once.  run() only
    enqueues on the ctx stream.  close() (or the last reference going away) waits for that stream and frees the operators."""

    def __init__(self, L: np.ndarray, R: np.ndarray, ctx: Optional[Context] = None):
        self.ctx = ctx or get_context()
        L = np.ascontiguousarray(L, dtype=np.float32)
        R = np.ascontiguousarray(R, dtype=np.float32)
        if L.ndim != 2 or R.ndim != 2 or L.shape[0] % 2 or R.shape[1] % 2:
            raise ValueError(f'resample operators [2m, M] and [n, 2N] expected, got {L.shape} and {R.shape}')
        self.shape_in = (L.shape[1], R.shape[1] // 2)
        self.shape_out = (L.shape[0] // 2, R.shape[0])
        h = C.c_void_p()
        check(self.ctx.lib.tpz_resample_create(self.ctx.handle, self.shape_in[0], self.shape_in[1], self.shape_out[0],
                                               self.shape_out[1], L.ctypes.data_as(C.c_void_p), R.ctypes.data_as(C.c_void_p),
                                               C.byref(h)), self.ctx.handle)
        self.handle = h

    def run(self, x: torch.Tensor) -> torch.Tensor:
        """x: fp32 [M, N] on the ctx device -> fp32 [m, n] on the device.  A non-contiguous view (or another dtype / device) is
        copied into a dense fp32 device tensor first (as_device_f32); the kernel only ever reads dense rows."""
        if not self.handle:
            raise _lib.TopazHipError('resample plan used after close()')
        if tuple(x.shape) != self.shape_in:
            raise ValueError(f'resample plan for {self.shape_in} images, got {tuple(x.shape)}')
        self.ctx.bind_current_stream()
        x = as_device_f32(x, self.ctx)
        y = _result(self.ctx, self.shape_out)
        check(self.ctx.lib.tpz_resample_run(self.handle, _ptr(x), _ptr(y)), self.ctx.handle)
        return y

    def run_host(self, x: np.ndarray) -> np.ndarray:
        """tpz_resample_2d_host: numpy image in, numpy image out (synchronous; staged inside the library)"""
        if not self.handle:
            raise _lib.TopazHipError('resample plan used after close()')
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.shape != self.shape_in:
            raise ValueError(f'resample plan for {self.shape_in} images, got {x.shape}')
        self.ctx.bind_current_stream()
        y = np.empty(self.shape_out, dtype=np.float32)
        check(self.ctx.lib.tpz_resample_2d_host(self.handle, x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p)),
              self.ctx.handle)
        return y

    def close(self) -> None:
        if getattr(self, 'handle', None):
            self.ctx.lib.tpz_resample_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def resample_upload_bytes(ctx: Optional[Context] = None) -> int:
    """operator bytes the context has uploaded for resample plans so far (tpz_resample_upload_bytes): grows when a plan is
    created, never when one runs"""
    ctx = ctx or get_context()
    return int(ctx.lib.tpz_resample_upload_bytes(ctx.handle))


def transpose(x: torch.Tensor, ctx: Optional[Context] = None) -> torch.Tensor:
    ctx = ctx or get_context()
    ctx.bind_current_stream()
    x = as_device_f32(x, ctx)
    R, Cc = x.shape
    y = _result(ctx, (Cc, R))
    check(ctx.lib.tpz_transpose_2d(ctx.handle, _ptr(x), R, Cc, _ptr(y)), ctx.handle)
    return y
