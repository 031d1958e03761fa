"""The two pinned rings every device-resident file loop is built from, and the loop itself.

  ImageFeed      the way in: a reader thread decodes image i+1 straight into a pinned staging slot (tpz_stage) and queues its H2D
                 copy while the GPU works on image i; the host never waits for a copy.
  ResultRing     the way out: the result of image i is copied into a pinned slot on the copy stream and a writer thread hands
                 it to a callback once it has landed, under the GPU's work on image i+1.
  stream_images  ImageFeed -> process (calling thread, in order) -> ResultRing: the loop of `preprocess` / `normalize` (stats.py)
                 and of `denoise` [`--stack`] (denoise.py).  utils/picks.py cuts several chunks per image and drives a
                 ResultRing itself.

The only module of the package that builds an rt.Stage, a queue or a thread (the host-path pools of denoise.py aside)."""
from __future__ import annotations

import contextlib
import os
import queue
import sys
import threading
from typing import Iterator, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import mrc
from . import runtime as rt
from .utils.image import load_image


def slot_bytes_for(nbytes: int) -> int:
    """the slot size of a ring that has to hold nbytes: rounded up to 1 MiB, so that images of about one size share a ring"""
    return (int(nbytes) + (1 << 20) - 1) & ~((1 << 20) - 1)


def pwrite_all(fd: int, view, at: int) -> None:
    """the whole of a C-contiguous buffer (a numpy array, a memoryview) at byte `at` of fd; os.pwrite may write less than asked"""
    view = memoryview(view).cast('B')
    done = 0
    while done < len(view):
        done += os.pwrite(fd, view[done:], at + done)


def warn_overflow(what, count: int) -> None:
    """the one line a command prints when float16 output stored finite values as +-inf: `what` names the file or the section"""
    print(f'# warning: {what}: {int(count)} finite value(s) beyond the float16 range (|x| >= 65520) stored as inf',
          file=sys.stderr, flush=True)


def as_float16(x: np.ndarray, what) -> np.ndarray:
    """the float16 form of a result that is on the host already (the paths that do not go through a ring), with the warning"""
    x = np.asarray(x)
    with np.errstate(over='ignore'):
        half = np.ascontiguousarray(x, dtype=np.float16)
    lost = int(np.count_nonzero(np.isinf(half) & np.isfinite(x)))
    if lost:
        warn_overflow(what, lost)
    return half


class ImageFeed:
    """Iterate (path, device tensor [H, W] or [D, H, W]) with the NEXT micrograph's disk read, H2D copy and fp32 conversion
    running under the consumer's work on the current one.  A reader thread reads into the pinned buffer of a free staging
    slot and queues the copy; the consumer acquires the slot on its stream, uses the tensor, and the slot is released (for
    re-use two images later) when the consumer asks for the next item.  Pixels stored as int8, int16, uint16 or float16 cross
    to the device as stored and become fp32 there, on the copy stream; the tensor yielded is fp32 either way."""

    DEPTH = 3

    def __init__(self, paths: Sequence[str], ctx: 'rt.Context', headers: bool = False):
        """headers=True: items are (path, tensor, MRC header or None, extended header or None).  An entry of `paths` that is not
        a string is an image already in memory, (key, array, header, extended header): it takes the same ring, its key in the
        place of the path."""
        self.paths, self.ctx, self.headers = list(paths), ctx, headers
        self.stage: Optional[rt.Stage] = None
        self.slot_bytes = 0
        self.ready: 'queue.Queue' = queue.Queue(maxsize=self.DEPTH - 1)
        self.free: 'queue.Queue' = queue.Queue()
        self.thread = threading.Thread(target=self._reader, daemon=True)
        self._retired: List['rt.Stage'] = []      # outgrown rings: closed by the consumer when the feed ends
        self._stop = threading.Event()           # the consumer left (done, or an exception): the reader must not block
        self.uploaded_bytes = 0                  # pixel bytes queued host -> device so far (the reader thread counts them)

    def _ensure_stage(self, nbytes: int) -> None:
        # (called from the reader thread before any slot of a new, larger ring is handed out)
        if self.stage is None or nbytes > self.slot_bytes:
            old = self.stage
            self.slot_bytes = slot_bytes_for(nbytes)
            self.stage = rt.Stage(self.ctx, self.slot_bytes, self.DEPTH)
            while not self.free.empty():
                self.free.get_nowait()
            for k in range(self.DEPTH):
                self.free.put((self.stage, k))
            if old is not None:
                self._retired.append(old)  # closed by the consumer when the feed ends (never from this thread: tpz_stage_free
                                           # synchronises the ctx stream the consumer is enqueuing on)

    def _get_free(self):
        """a free slot, or None once the consumer has left"""
        while not self._stop.is_set():
            try:
                return self.free.get(timeout=0.1)
            except queue.Empty:
                pass
        return None

    def _put_ready(self, item) -> bool:
        while not self._stop.is_set():
            try:
                self.ready.put(item, timeout=0.1)
                return True
            except queue.Full:
                pass
        return False

    def _reader(self) -> None:
        try:
            torch.cuda.set_device(self.ctx.device)
            class _Left(Exception):
                pass

            held = []

            def pinned(shape, dtype=np.float32):
                """the pinned buffer of a free staging slot for an image of that shape (the ring grows when it must).  A dtype
                the device decodes (mrc.STORED_MODES): the slot holds the fp32 image and, behind it, the stored pixels"""
                n = int(np.prod(shape))
                mode = mrc.STORED_MODES.get(np.dtype(dtype))
                nbytes = n * 4 if mode is None else rt.Stage.decode_bytes(self.ctx, mode, n)
                if self.stage is None or nbytes > self.slot_bytes:
                    # wait until every slot of the old ring came back, then grow
                    if self.stage is not None:
                        for _ in range(self.DEPTH):
                            if self._get_free() is None:
                                raise _Left()
                    self._ensure_stage(nbytes)
                slot = self._get_free()
                if slot is None:
                    raise _Left()
                # the slot's previous upload may still be queued (a consumer that only enqueues runs ahead of the copy
                # stream): the pinned buffer is refilled only after that copy has read it
                slot[0].wait(slot[1])
                held[:] = [slot, n, mode]
                return slot[0].host_array(slot[1], shape, np.float32 if mode is None else dtype)

            for path in self.paths:
                header = extended = None
                try:
                    # an MRC file is read straight into pinned memory IN THE TYPE IT STORES (float32, or int8 / int16 / uint16 /
                    # float16, which the device decodes: Stage.upload_decode); anything else is loaded and converted into it; so
                    # is an image the caller already holds (a section of a stack), which keeps a stored type of those four too
                    in_memory = not isinstance(path, str)
                    if in_memory:
                        path, image, header, extended = path
                    got = mrc.read_stored_into(path, pinned) if not in_memory and os.path.splitext(path)[1] == '.mrc' else None
                    if got is not None:
                        host, header, extended = got
                    else:
                        if not in_memory:
                            loaded = load_image(path, make_image=False)
                            image, header, extended = loaded if isinstance(loaded, tuple) else (loaded, None, None)
                        image = np.asarray(image)
                        host = pinned(image.shape, image.dtype if image.dtype in mrc.STORED_MODES else np.float32)
                        np.copyto(host, image, casting='unsafe')
                except _Left:
                    return
                (stage, k), n, mode = held
                if mode is None:
                    stage.upload(k, 4 * n)
                else:
                    stage.upload_decode(k, mode, n)
                self.uploaded_bytes += n * host.dtype.itemsize
                if not self._put_ready((path, stage, k, host.shape, header, extended)):
                    return
            self._put_ready(None)
        except BaseException as e:                                            # surface reader failures in the consumer
            self._put_ready(e)

    def __iter__(self) -> Iterator[Tuple[str, torch.Tensor]]:
        self.thread.start()
        held = None
        try:
            while True:
                if held is not None:            # the consumer came back for more: it is done with the previous tensor
                    held[0].release(held[1])
                    self.free.put(held)
                    held = None
                item = self.ready.get()
                if item is None:
                    return
                if isinstance(item, BaseException):
                    raise item
                path, stage, k, shape, header, extended = item
                stage.acquire(k)
                held = (stage, k)
                if self.headers:
                    yield path, stage.device_tensor(k, shape), header, extended
                else:
                    yield path, stage.device_tensor(k, shape)
        finally:
            if held is not None:
                held[0].release(held[1])
            # the consumer is leaving (exhausted, early exit or exception): unblock and join the reader, then close the rings
            # from THIS thread (the one that enqueues on the ctx stream)
            self._stop.set()
            if self.thread.is_alive():
                self.thread.join(timeout=30)
            if not self.thread.is_alive():
                for st in self._retired:
                    st.close()
                self._retired = []
                if self.stage is not None:
                    self.stage.close()
                    self.stage = None


class ResultRing:
    """Carry float32 results off the device -- as they are, or encoded there to float16 / uint8 (put's `encode`) -- without the
    calling thread waiting for a copy.  put(tensor, *payload) queues the D2H
    copy of a device tensor into a free pinned slot of an rt.Stage ring of `depth` slots; a writer thread waits for the copy and
    calls write(host_array, *payload) -- host_array: the slot's pinned buffer as a numpy view of the tensor's shape, valid for
    the call.  The tensor is referenced here until its copy has landed.
    After a failure of `write` (or of the wait) the thread skips every later item, still returning their slots, and the FIRST
    failure is raised in the calling thread by the next put() and by check().
    Growth: a tensor larger than a slot, or a larger reserve(), waits until all slots are back (everything queued so far has
    been written), closes the outgrown rt.Stage at once from the calling thread, then creates the larger one: never two rings
    of pinned memory at a time, however often the sizes rise.  tpz_stage_free synchronises the context's stream, so each growth
    costs the caller one stream synchronisation -- only when a result is larger than every result before it."""

    def __init__(self, ctx: 'rt.Context', write, depth: int = 2, on_overflow=None):
        self.ctx, self.write, self.depth, self.on_overflow = ctx, write, depth, on_overflow
        self.stage: Optional[rt.Stage] = None
        self.slot_bytes = 0
        self.free: 'queue.Queue' = queue.Queue()
        self.todo: 'queue.Queue' = queue.Queue()
        self.failed: list = []
        self.thread = threading.Thread(target=self._writer, daemon=True)
        self.thread.start()

    def _writer(self) -> None:
        while True:
            item = self.todo.get()
            if item is None:
                return
            k, shape, payload, enc = item[:4]                   # (item[4], the tensor, lives until its copy is done)
            try:
                if not self.failed:
                    self.stage.wait(k)                          # the D2H of this slot has landed
                    if enc is None:
                        self.write(self.stage.host_array(k, shape), *payload)
                    else:
                        lost = self.stage.overflow_count(k, int(np.prod(shape)), enc)
                        if lost and self.on_overflow is not None:
                            self.on_overflow(lost, *payload)
                        self.write(self.stage.host_array(k, shape, rt.ENC_DTYPES[enc]), *payload)
            except BaseException as e:                          # surfaces in the calling thread
                self.failed.append(e)
            finally:
                del item
                self.free.put(k)

    def check(self) -> None:
        if self.failed:
            raise self.failed[0]

    def reserve(self, nbytes: int) -> None:
        """make every slot hold nbytes (see Growth above); nothing happens when it already does"""
        if self.stage is not None and nbytes <= self.slot_bytes:
            return
        if self.stage is not None:
            for _ in range(self.depth):
                self.free.get()
            self.stage.close()
            self.stage = None
        self.slot_bytes = slot_bytes_for(nbytes)
        self.stage = rt.Stage(self.ctx, self.slot_bytes, self.depth)
        for k in range(self.depth):
            self.free.put(k)

    def put(self, tensor: torch.Tensor, *payload, encode=None) -> None:
        """encode: None (the float32 bytes), rt.ENC_F16, or (rt.ENC_U8, (mi, ma)) -- the tensor is encoded on the copy stream
        (Stage.download_encoded), `write` gets the pinned view in the stored dtype (np.float16 / np.uint8) and, before it, the
        ring's on_overflow(count, *payload) hears of finite values float16 stored as +-inf, when there are any"""
        enc, params = encode if isinstance(encode, tuple) else (encode, None)
        if enc is None:
            self.reserve(tensor.numel() * tensor.element_size())
        else:
            self.reserve(rt.Stage.encode_bytes(self.ctx, enc, tensor.numel()))
        k = self.free.get()
        if self.failed:
            self.free.put(k)
            raise self.failed[0]
        if enc is None:
            self.stage.download(k, tensor)
        else:
            self.stage.download_encoded(k, tensor, enc, params)
        self.todo.put((k, tuple(tensor.shape), payload, enc, tensor))

    def close(self) -> None:
        """wait for the last write, end the thread, free the ring (idempotent; a failure stays available to check())"""
        if self.thread.is_alive():
            self.todo.put(None)
            self.thread.join()
        if self.stage is not None:
            self.stage.close()
            self.stage = None

    def __enter__(self) -> 'ResultRing':
        return self

    def __exit__(self, *exc) -> None:
        self.close()


class Put(NamedTuple):
    """one result of stream_images' `process`: what ResultRing.put takes"""
    tensor: torch.Tensor
    payload: tuple
    encode: object = None       # None (float32), rt.ENC_F16, or (rt.ENC_U8, (mi, ma))


def stream_images(items: Sequence, ctx: 'rt.Context', process, write, on_overflow=None) -> None:
    """The device-resident loop over files (or over images already in memory: ImageFeed).  The feed's reader thread decodes and
    uploads image i+1, process(key, device tensor, header, extended header) -> (device tensor, payload tuple) runs on image i in
    the calling thread and in order (whatever it draws from the NumPy RNG is drawn in path order), and the ring's writer thread
    calls write(pinned host array, *payload) for image i-1.  process returns that pair, or a Put (the pair and the encoding the
    result leaves the device in; on_overflow: the ring's hook), or a list of Puts: one put each.  On the way out, also by an
    exception: the feed is closed (its reader joined), then the ring (everything queued is written, unless a write failed), then
    a writer's failure is raised."""
    feed = iter(ImageFeed(items, ctx, headers=True))
    with ResultRing(ctx, write, on_overflow=on_overflow) as ring, contextlib.closing(feed):   # (left in reverse: the feed first)
        for key, x, header, extended in feed:
            results = process(key, x, header, extended)
            for put in (results if isinstance(results, list) else [Put(*results)]):
                ring.put(put.tensor, *put.payload, encode=put.encode)
    ring.check()
