"""streaming.ResultRing, stream_images and pwrite_all without a GPU: `runtime.Stage` is replaced by a host fake with one numpy
buffer per slot that records what is done to it, so the order of writes, the growth rule, the failure rule and the lifetime of
a queued tensor are checked on the threads the commands use."""
import gc
import os
import threading
import weakref

import numpy as np
import pytest
import torch

from topaz_amd import runtime as rt
from topaz_amd import streaming


class Boom(Exception):
    pass


@pytest.fixture
def stages(monkeypatch):
    """the fake in the place of rt.Stage; yields the namespace its instances report to: `events` (('create' | 'close', stage) and
    whatever a test appends), `made`, and `gate`, the event every wait() blocks on (set unless a test clears it)"""
    class Stage:
        events, made, gate = [], [], threading.Event()

        def __init__(self, ctx, slot_bytes, depth=2):
            self.slot_bytes, self.depth, self.closed, self.waits = slot_bytes, depth, False, []
            self.slots = [np.zeros(slot_bytes, dtype=np.uint8) for _ in range(depth)]
            self.made.append(self)
            self.events.append(('create', self))

        def download(self, slot, src):
            assert not self.closed and not src.is_cuda
            raw = src.contiguous().numpy().reshape(-1).view(np.uint8)
            assert raw.size <= self.slot_bytes
            self.slots[slot][:raw.size] = raw

        def wait(self, slot):
            assert not self.closed
            assert self.gate.wait(timeout=30)
            self.waits.append(slot)

        def host_array(self, slot, shape, dtype=np.float32):
            assert not self.closed
            n = int(np.prod(shape)) * np.dtype(dtype).itemsize
            return self.slots[slot][:n].view(dtype).reshape(shape)

        def close(self):
            if not self.closed:
                self.closed = True
                self.events.append(('close', self))

    Stage.gate.set()
    monkeypatch.setattr(rt, 'Stage', Stage)
    yield Stage
    Stage.gate.set()


def _tensor(n, seed):
    return torch.from_numpy(np.random.RandomState(seed).randn(n).astype(np.float32))


def test_slot_bytes_round_up_to_one_mib():
    assert [streaming.slot_bytes_for(n) for n in (1, 40, 1 << 20, (1 << 20) + 1, 3 << 20)] == \
        [1 << 20, 1 << 20, 1 << 20, 2 << 20, 3 << 20]


def test_items_are_written_in_order_with_their_payloads(stages):
    seen = []
    tensors = [_tensor(12, i).reshape(3, 4) for i in range(5)]
    with streaming.ResultRing(object(), lambda host, i, name: seen.append((host.copy(), i, name))) as ring:
        for i, t in enumerate(tensors):
            ring.put(t, i, f'image-{i}')
    ring.check()
    assert [(i, name) for _, i, name in seen] == [(i, f'image-{i}') for i in range(5)]
    for (host, _, _), t in zip(seen, tensors):
        assert host.shape == (3, 4) and host.dtype == np.float32 and np.array_equal(host, t.numpy())
    assert len(stages.made) == 1 and stages.made[0].depth == 2 and stages.made[0].closed
    assert sorted(stages.made[0].waits) == [0, 0, 0, 1, 1]                  # every write waited for its slot's copy


def test_a_larger_item_closes_the_ring_and_makes_one_larger(stages):
    sizes = [10, (1 << 18) + 1, 10]                                         # 40 bytes, one float over 1 MiB, 40 bytes
    tensors = [_tensor(n, n) for n in sizes]

    def write(host, i):
        assert np.array_equal(host, tensors[i].numpy())
        stages.events.append(('written', i))

    with streaming.ResultRing(object(), write) as ring:
        for i, t in enumerate(tensors):
            ring.put(t, i)
            assert sum(not s.closed for s in stages.made) == 1              # never two rings open
    first, second = stages.made                                             # exactly two
    assert (first.slot_bytes, second.slot_bytes) == (1 << 20, 2 << 20)
    assert stages.events == [('create', first), ('written', 0), ('close', first), ('create', second), ('written', 1),
                             ('written', 2), ('close', second)]


def test_a_reservation_that_covers_the_items_means_no_growth(stages):
    seen = []
    with streaming.ResultRing(object(), lambda host: seen.append(host.size)) as ring:
        ring.reserve((1 << 20) + 4)
        ring.reserve(100)                                                   # (smaller: nothing happens)
        for n in (10, (1 << 18) + 1, 10):
            ring.put(_tensor(n, 0))
    assert seen == [10, (1 << 18) + 1, 10]
    assert len(stages.made) == 1 and stages.made[0].slot_bytes == 2 << 20


def _failing_write(written):
    def write(host, i):
        if i == 1:
            raise Boom(f'item {i}')
        written.append(i)
    return write


def test_a_failed_write_is_raised_by_a_later_put_and_skips_the_rest(stages):
    written = []
    ring = streaming.ResultRing(object(), _failing_write(written))
    # two slots: the fourth put at the latest takes the slot the failed item gave back
    with pytest.raises(Boom, match='item 1'):
        for i in range(4):
            ring.put(_tensor(10, i), i)
    thread = ring.thread
    ring.close()
    assert written == [0]
    assert stages.made[0].closed and not thread.is_alive()
    with pytest.raises(Boom, match='item 1'):
        ring.check()


def test_a_failed_write_is_raised_by_check_after_close(stages):
    written = []
    stages.gate.clear()                                                     # no copy lands before all four are queued
    ring = streaming.ResultRing(object(), _failing_write(written), depth=4)
    for i in range(4):
        ring.put(_tensor(10, i), i)
    stages.gate.set()
    ring.close()
    assert written == [0]                                                   # items three and four were skipped
    assert stages.made[0].closed and not ring.thread.is_alive()
    with pytest.raises(Boom, match='item 1'):
        ring.check()


def test_closing_twice_is_harmless(stages):
    seen = []
    ring = streaming.ResultRing(object(), lambda host: seen.append(host[0]))
    ring.put(torch.full((4,), 3.0))
    ring.close()
    ring.close()
    ring.check()
    assert seen == [3.0] and stages.events == [('create', stages.made[0]), ('close', stages.made[0])]
    never_used = streaming.ResultRing(object(), seen.append)
    never_used.close()
    never_used.close()
    assert len(stages.made) == 1 and not never_used.thread.is_alive()


def test_a_queued_tensor_lives_until_its_copy_has_landed(stages):
    stages.gate.clear()
    ring = streaming.ResultRing(object(), lambda host: None)
    t = _tensor(10, 0)
    ref = weakref.ref(t)
    ring.put(t)
    del t
    gc.collect()
    assert ref() is not None                                                # the copy is still in flight: the ring holds it
    stages.gate.set()
    ring.close()
    gc.collect()
    assert ref() is None


def test_stream_images_closes_the_feed_then_the_ring_then_raises(stages, monkeypatch):
    order = []

    class Feed:
        def __init__(self, items, ctx, headers=False):
            assert headers
            self.items = items

        def __iter__(self):
            try:
                for key in self.items:
                    yield key, torch.full((2, 3), float(key)), {'of': key}, None
            finally:
                order.append('feed closed')

    monkeypatch.setattr(streaming, 'ImageFeed', Feed)
    real_close = stages.close
    monkeypatch.setattr(stages, 'close', lambda self: (order.append('ring closed'), real_close(self)))
    calls = []

    def process(key, x, header, extended):
        calls.append((key, threading.current_thread()))
        return x + 1, (key, header)

    def write(host, key, header):
        if key == 2:
            raise Boom('write')
        order.append(('written', key, float(host[0, 0]), header))

    with pytest.raises(Boom, match='write'):
        streaming.stream_images([1, 2], object(), process, write)
    assert calls == [(1, threading.current_thread()), (2, threading.current_thread())]
    assert [o for o in order if isinstance(o, str)] == ['feed closed', 'ring closed']
    assert order.index(('written', 1, 2.0, {'of': 1})) < order.index('ring closed') and len(order) == 3

    # a failure of the loop itself leaves the same way, and nothing is running afterwards
    del order[:]
    before = set(threading.enumerate())
    with pytest.raises(Boom, match='process'):
        streaming.stream_images([1], object(), lambda *a: (_ for _ in ()).throw(Boom('process')), write)
    assert order == ['feed closed']                                         # (no result: no ring was ever made)
    assert [t for t in threading.enumerate() if t not in before and t.is_alive()] == []


def test_pwrite_all_finishes_short_writes(tmp_path, monkeypatch):
    real = os.pwrite
    monkeypatch.setattr(os, 'pwrite', lambda fd, data, at: real(fd, bytes(data[:7]), at))
    x = np.arange(30, dtype=np.float32).reshape(5, 6)
    fd = os.open(str(tmp_path / 'f'), os.O_WRONLY | os.O_CREAT, 0o666)
    try:
        streaming.pwrite_all(fd, x, 16)
    finally:
        os.close(fd)
    assert open(str(tmp_path / 'f'), 'rb').read() == bytes(16) + x.tobytes()
