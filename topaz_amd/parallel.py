"""Multi-GPU layer: micrographs shard embarrassingly (one image per rank at a time, rank r takes
images i = r (mod world)); the exchange steps are the gather of the per-image pick tables to
rank 0 for the single-TSV output mode of `topaz extract` (topaz/extract.py:321-354) and, with
`--targets`, one gather of every rank's per-image hit / score records of the whole radius sweep.

One process per GPU; torch.distributed backend 'nccl' (= RCCL over xGMI on ROCm) on the GPU box,
'gloo' in the CPU tests.  The reference has no distributed code; this is new.
"""
from __future__ import annotations

import os
import sys
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.distributed as dist


def init_from_env(backend: Optional[str] = None) -> Tuple[int, int, int]:
    """(rank, local_rank, world).  Single process when WORLD_SIZE is unset or 1."""
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    if world > 1:
        pin_this_rank(local_rank, int(os.environ.get('LOCAL_WORLD_SIZE', world)))
    if (world > 1 or os.environ.get('TOPAZ_AMD_FORCE_DIST') == '1') and not dist.is_initialized():
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29500')
        if backend is None:
            backend = os.environ.get('TOPAZ_AMD_DIST_BACKEND') or ('nccl' if torch.cuda.is_available() else 'gloo')
        if backend == 'nccl':
            if world > 1:
                preflight(rank, local_rank, world)        # one line per rank on stderr; fails fast on a rank without a GPU
            torch.cuda.set_device(local_rank)
            dist.init_process_group(backend, rank=rank, world_size=world, device_id=torch.device('cuda', local_rank))
        else:
            with _stdout_to_stderr():
                dist.init_process_group(backend, rank=rank, world_size=world)
    return rank, local_rank, world


class _stdout_to_stderr:
    """File descriptor 1 points at stderr inside the block.  The gloo library announces every rank's connections on stdout
    ("[Gloo] Rank r is connected to ...") while the process group is built, in several writes per line: the ranks of one job
    share the launcher's stdout, their banners interleave there, and fragments of them ended up between the lines of a command
    whose stdout is its result (`extract --targets`).  Diagnostics belong on stderr; stdout is back when the block ends."""

    def __enter__(self):
        self.saved = None
        try:
            sys.stdout.flush()
            self.saved = os.dup(1)
            os.dup2(2, 1)
        except (OSError, ValueError):
            if self.saved is not None:
                os.close(self.saved)
                self.saved = None
        return self

    def __exit__(self, *exc):
        if self.saved is not None:
            try:
                os.dup2(self.saved, 1)
            finally:
                os.close(self.saved)
        return False


def rank_device(local_rank: int) -> int:
    """HIP device of a rank process: its local rank -- or, with TOPAZ_AMD_SHARE_GPU=1 (a rehearsal of the multi-rank job on a
    box with fewer GPUs than ranks: RCCL refuses two ranks on one device, so this goes with TOPAZ_AMD_DIST_BACKEND=gloo),
    local_rank modulo the visible devices."""
    if os.environ.get('TOPAZ_AMD_SHARE_GPU') == '1' and torch.cuda.is_available():
        return local_rank % max(1, torch.cuda.device_count())
    return local_rank


def collective_device(local_rank: int) -> torch.device:
    """where the tensors of the exchange step live: the rank's GPU under RCCL, host memory under gloo"""
    if dist.is_available() and dist.is_initialized() and dist.get_backend() == 'gloo':
        return torch.device('cpu')
    return torch.device('cuda', rank_device(local_rank))


def preflight(rank: int, local_rank: int, world: int, stream=None) -> dict:
    """First-contact report of a rank of a multi-GPU job, before anything is timed: which device it drives (name, PCI address,
    NUMA node), the CPUs it is pinned to, the rendezvous it uses -- one line per rank on stderr, so that a hang or a crash in the
    first collective can be attributed -- and a fail-fast check that the device exists (a rank without a GPU would otherwise
    die inside RCCL's init with the other ranks waiting on it)."""
    import sys
    info = {'rank': rank, 'local_rank': local_rank, 'world': world, 'pid': os.getpid(),
            'master': f"{os.environ.get('MASTER_ADDR', '?')}:{os.environ.get('MASTER_PORT', '?')}",
            'cpus': os.environ.get('TOPAZ_AMD_RANK_CPUS') or 'unpinned',
            'visible': {v: os.environ[v] for v in _VISIBLE_VARS if os.environ.get(v)},
            'ipc_legacy': os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY')}
    n_dev = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if local_rank >= n_dev:
        raise RuntimeError(f'rank {rank}: local rank {local_rank} has no GPU ({n_dev} visible; {info["visible"] or "no *_VISIBLE_DEVICES set"})')
    pr = torch.cuda.get_device_properties(local_rank)
    info['device'] = pr.name
    try:
        info['pci'] = f'{int(getattr(pr, "pci_domain_id", 0)):04x}:{int(pr.pci_bus_id):02x}:{int(pr.pci_device_id):02x}.0'
        info['numa_node'] = int(open(f'/sys/bus/pci/devices/{info["pci"]}/numa_node').read())
    except (AttributeError, OSError, ValueError):
        pass
    print('[topaz_amd rank] ' + ' '.join(f'{k}={v}' for k, v in info.items()), file=stream or sys.stderr, flush=True)
    return info


def under_launcher() -> bool:
    """True inside a rank process (torchrun or launch_local_ranks set WORLD_SIZE)"""
    return 'WORLD_SIZE' in os.environ


def free_port() -> int:
    import socket
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _parse_cpulist(text: str) -> List[int]:
    out: List[int] = []
    for part in text.strip().split(','):
        if not part:
            continue
        lo, _, hi = part.partition('-')
        out.extend(range(int(lo), int(hi or lo) + 1))
    return out


_VISIBLE_VARS = ('HIP_VISIBLE_DEVICES', 'ROCR_VISIBLE_DEVICES', 'CUDA_VISIBLE_DEVICES', 'GPU_DEVICE_ORDINAL')


def gpu_numa_nodes(n: int, sysfs: str = '/sys') -> Optional[List[int]]:
    """NUMA node of HIP device 0 .. n-1 as HIP itself enumerates them: the device's PCI address (torch's device properties) ->
    /sys/bus/pci/devices/<domain:bus:device.0>/numa_node.  Unlike the DRM card order this holds under *_VISIBLE_DEVICES
    subsets and partition modes.  None when it cannot be resolved (no GPU runtime in this process, properties without a PCI
    address, no sysfs entry) -- the caller then falls back.  Only called in rank processes, which initialise HIP anyway."""
    try:
        if not torch.cuda.is_available() or torch.cuda.device_count() < n:
            return None
        nodes = []
        for r in range(n):
            pr = torch.cuda.get_device_properties(r)
            bdf = f'{int(getattr(pr, "pci_domain_id", 0)):04x}:{int(pr.pci_bus_id):02x}:{int(pr.pci_device_id):02x}.0'
            nodes.append(int(open(os.path.join(sysfs, 'bus/pci/devices', bdf, 'numa_node')).read().strip()))
        return nodes
    except (AttributeError, OSError, ValueError, RuntimeError):
        return None


def cpu_sets_for_ranks(n: int, sysfs: str = '/sys', allowed: Optional[Sequence[int]] = None,
                       nodes: Optional[Sequence[int]] = None) -> List[List[int]]:
    """Host placement of n rank processes on one node: rank r gets CPUs of the NUMA node GPU r hangs off (the amdgpu render
    devices of /sys/class/drm in card order, their device/numa_node, that node's cpulist), the GPUs of one node sharing its CPUs
    in equal contiguous slices -- each rank's launch thread (~700 kernel launches per micrograph) and reader thread then stay
    next to their GPU's PCIe root and off the other ranks' cores.  Fallback when the topology cannot be read (no sysfs entry,
    numa_node -1, fewer GPUs listed than ranks): the allowed CPUs cut into n equal contiguous slices.  Pure function of the
    sysfs tree (tests feed it a fake one)."""
    import glob
    if allowed is None:
        try:
            allowed = sorted(os.sched_getaffinity(0))
        except (AttributeError, OSError):
            allowed = list(range(os.cpu_count() or 1))
    allowed = list(allowed)

    def even_slices(cpus: Sequence[int], k: int) -> List[List[int]]:
        cpus = list(cpus)
        if len(cpus) < k:
            return [cpus for _ in range(k)]
        return [cpus[i * len(cpus) // k:(i + 1) * len(cpus) // k] for i in range(k)]

    if nodes is not None:
        nodes = list(nodes)
    elif any(os.environ.get(v) for v in _VISIBLE_VARS):
        # HIP device r is not DRM card r under a visible-devices subset: do not guess (gpu_numa_nodes resolves it in the rank)
        return even_slices(allowed, n)
    else:
        nodes = _drm_numa_nodes(sysfs)
    if len(nodes) < n or any(v < 0 for v in nodes[:n]):
        return even_slices(allowed, n)
    nodes = nodes[:n]
    out: List[List[int]] = [[] for _ in range(n)]
    for node in sorted(set(nodes)):
        try:
            cpus = [c for c in _parse_cpulist(open(os.path.join(sysfs, f'devices/system/node/node{node}/cpulist')).read())
                    if c in set(allowed)]
        except (OSError, ValueError):
            return even_slices(allowed, n)
        ranks = [r for r in range(n) if nodes[r] == node]
        if not cpus:
            return even_slices(allowed, n)
        for r, sl in zip(ranks, even_slices(cpus, len(ranks))):
            out[r] = sl
    return out


def _drm_numa_nodes(sysfs: str) -> List[int]:
    """NUMA nodes of the amdgpu devices in DRM card order (only meaningful when every GPU is visible, in that order)"""
    import glob
    nodes: List[int] = []
    try:
        cards = sorted(glob.glob(os.path.join(sysfs, 'class/drm/card[0-9]*')),
                       key=lambda p: int(''.join(ch for ch in os.path.basename(p) if ch.isdigit())))
        for c in cards:
            if '-' in os.path.basename(c):                       # connectors (card0-DP-1), not devices
                continue
            drv = os.path.join(c, 'device/driver')
            if os.path.exists(drv) and os.path.basename(os.path.realpath(drv)) != 'amdgpu':
                continue
            nodes.append(int(open(os.path.join(c, 'device/numa_node')).read().strip()))
    except (OSError, ValueError):
        nodes = []
    return nodes


def _set_affinity_all_threads(cpus: Sequence[int]) -> None:
    """sched_setaffinity(0, .) moves the calling thread only: threads that exist already (an OpenMP pool, torch's workers)
    are moved one by one through /proc/self/task"""
    cpus = set(cpus)
    os.sched_setaffinity(0, cpus)
    try:
        for tid in os.listdir('/proc/self/task'):
            try:
                os.sched_setaffinity(int(tid), cpus)
            except (OSError, ValueError):
                pass                                    # (a thread that ended meanwhile)
    except OSError:
        pass


_PINNED: Optional[List[int]] = None


def pin_this_rank(local_rank: int, local_world: int) -> Optional[List[int]]:
    """Host placement of this rank process, applied by the rank itself (never in a fork hook of the launcher): the CPU set
    launch_local_ranks handed over in TOPAZ_AMD_RANK_CPUS, else -- torchrun, or a *_VISIBLE_DEVICES subset the launcher would
    not guess about -- the CPUs next to ITS GPU, resolved through HIP's own PCI address of the device (gpu_numa_nodes), else the
    DRM card order when every GPU is visible.  Every existing thread is moved.  No-op with TOPAZ_AMD_NO_AFFINITY=1 or where
    affinity cannot be set; a failure leaves the rank unpinned rather than failing the job."""
    global _PINNED
    if os.environ.get('TOPAZ_AMD_NO_AFFINITY') == '1' or not hasattr(os, 'sched_setaffinity'):
        return None
    if _PINNED is not None:                   # init_from_env is called by every layer that shards (command, stream, sink): pin once
        return list(_PINNED)
    try:
        given = os.environ.get('TOPAZ_AMD_RANK_CPUS')
        if given:
            cpus = [int(c) for c in given.split(',') if c.strip()]
        else:
            nodes = gpu_numa_nodes(local_world) if any(os.environ.get(v) for v in _VISIBLE_VARS) else None
            sets = cpu_sets_for_ranks(local_world, nodes=nodes)
            cpus = sets[local_rank] if 0 <= local_rank < len(sets) else []
        if not cpus:
            return None
        _set_affinity_all_threads(cpus)
        os.environ['TOPAZ_AMD_RANK_CPUS'] = ','.join(map(str, cpus))
        _PINNED = list(cpus)
        return list(cpus)
    except (OSError, ValueError):
        return None


def launch_local_ranks(n: int, argv: Sequence[str], env: Optional[dict] = None, timeout: Optional[float] = None) -> int:
    """One process per GPU without an external launcher: start `n` copies of `argv` (a full command line, e.g.
    [sys.executable, 'bench.py', '--gpus', '8']) with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT set,
    rank r on GPU r, all on 127.0.0.1.  stdout / stderr are inherited, so rank 0's output is the job's output.
    Returns the largest exit code; when a rank fails the others are terminated (a hung collective would otherwise
    wait for its peer forever).  The counterpart of the reference's `-d -2` "use every GPU" (commands/denoise3d.py:
    102-103,117-118 -- DataParallel threads there, processes over RCCL here)."""
    import subprocess
    import time
    base = dict(os.environ if env is None else env)
    base.update(WORLD_SIZE=str(n), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(free_port()))
    base.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    procs = []
    # host placement: rank r on the CPUs next to GPU r (cpu_sets_for_ranks; TOPAZ_AMD_NO_AFFINITY=1 leaves the ranks unpinned)
    cpu_sets = None if base.get('TOPAZ_AMD_NO_AFFINITY') == '1' else cpu_sets_for_ranks(n)
    for r in range(n):
        e = dict(base, RANK=str(r), LOCAL_RANK=str(r), LOCAL_WORLD_SIZE=str(n))
        # the rank pins ITSELF to these CPUs first thing in init_from_env (pin_this_rank): no preexec_fn -- this process has
        # imported torch and is multi-threaded, where a fork hook may deadlock, and a failure to pin must not fail the launch
        if cpu_sets and cpu_sets[r] and not any(base.get(v) for v in _VISIBLE_VARS):
            e['TOPAZ_AMD_RANK_CPUS'] = ','.join(map(str, cpu_sets[r]))
        # (stdin is not shared: N readers of one pipe would each see a part of it -- the launcher resolves stdin input itself)
        procs.append(subprocess.Popen(list(argv), env=e, stdin=subprocess.DEVNULL))
    t0 = time.time()
    codes: List[Optional[int]] = [None] * n
    try:
        while any(c is None for c in codes):
            for r, p in enumerate(procs):
                if codes[r] is None:
                    codes[r] = p.poll()
            failed = [c for c in codes if c not in (None, 0)]
            if failed or (timeout is not None and time.time() - t0 > timeout):
                for r, p in enumerate(procs):
                    if codes[r] is None:
                        p.terminate()
                for r, p in enumerate(procs):
                    if codes[r] is None:
                        try:
                            codes[r] = p.wait(10)
                        except subprocess.TimeoutExpired:
                            p.kill()
                            codes[r] = p.wait()
                return max([abs(c) for c in failed] or [124])
            time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return max(abs(c) for c in codes)


def shard_indices(n_items: int, rank: int, world: int) -> List[int]:
    """items processed by `rank`: i = rank (mod world), in input order"""
    return list(range(rank, n_items, world))


def barrier(device: Optional[torch.device] = None) -> None:
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        if device is not None and device.type == 'cuda':
            dist.barrier(device_ids=[device.index])
        else:
            dist.barrier()


def max_over_ranks(value: float, device: torch.device) -> float:
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return value
    t = torch.tensor([value], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def sum_over_ranks(value: float, device: torch.device) -> float:
    """all_reduce(SUM) of one number; `value` itself without a process group"""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return value
    t = torch.tensor([value], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return float(t.item())


def gather_scalars(value: float, device: torch.device) -> List[float]:
    """every rank's number, on every rank (one all_gather)"""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return [value]
    t = torch.tensor([value], dtype=torch.float64, device=device)
    out = [torch.zeros_like(t) for _ in range(dist.get_world_size())]
    dist.all_gather(out, t)
    return [float(o.item()) for o in out]


def sum_to_root(t: torch.Tensor, dst: int = 0) -> Optional[torch.Tensor]:
    """element-wise sum of every rank's tensor onto rank `dst` (one reduce; RCCL on device tensors, gloo on host ones).
    Used to assemble a tomogram whose tiles were denoised by different ranks: each voxel is non-zero on exactly one rank, so
    the sum is exact.  Returns the tensor on dst, None elsewhere; a single process returns its tensor unchanged."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return t
    dist.reduce(t, dst=dst, op=dist.ReduceOp.SUM)
    return t if dist.get_rank() == dst else None


def gather_pick_tables(image_ids: Sequence[int], scores: Sequence[torch.Tensor], coords: Sequence[torch.Tensor],
                       device: torch.device, dst: int = 0):
    """Gather per-image pick tables to rank `dst`.

    Every rank passes the images it owns: ids, scores[i] (fp32 [n_i]) and coords[i] (int32 [n_i, d]).
    Exchange: the table sizes are data (the picks of an image), so one small all_gather of (images, rows, d) per rank fixes the
    stride -- read back with ONE device-to-host copy -- and then ONE gather moves every rank's table as a single int32 buffer
    packed on the device: `max_img` (id, n) header pairs followed by `max_rows` rows of (x, y[, z], score bits), padded to the
    largest rank.  A few hundred KB per micrograph: latency-bound, each peer writes to the root over its own xGMI link.
    Returns on dst a dict id -> (scores, coords) (CPU tensors), on the other ranks None.
    """
    d = coords[0].shape[1] if len(coords) else 2
    if not (dist.is_available() and dist.is_initialized()):
        return {int(i): (s.cpu(), c.cpu()) for i, s, c in zip(image_ids, scores, coords)}
    world, rank = dist.get_world_size(), dist.get_rank()      # (a 1-rank group takes the collective path too)
    trace = os.environ.get('TOPAZ_AMD_TRACE_GATHER') == '1'   # per-phase host clock of this rank on stderr
    import time as _time
    marks = [('start', _time.perf_counter())]
    n_img = len(image_ids)
    counts = [int(s.numel()) for s in scores]                  # (shapes: host-side knowledge, no device read)
    n_rows = int(sum(counts))
    meta = torch.tensor([n_img, n_rows, d], dtype=torch.int64, device=device)
    metas_t = torch.zeros(world * 3, dtype=torch.int64, device=device)
    dist.all_gather_into_tensor(metas_t, meta)
    metas = metas_t.view(world, 3).cpu().tolist()              # the one host read
    marks.append(('sizes all_gather', _time.perf_counter()))
    max_img = max(1, max(m[0] for m in metas))
    max_rows = max(1, max(m[1] for m in metas))
    d = max(m[2] for m in metas)
    w = d + 1
    # one buffer per rank: [max_img x (id, n)] ++ [max_rows x (coords..., score bits)], int32 -- packed WHERE THE TABLES LIVE
    # (the rank's GPU) and moved to the collective's device in one piece: under gloo (host tensors) that is one device-to-host
    # copy per rank instead of two per image
    pdev = scores[0].device if n_img else device
    buf = torch.zeros(2 * max_img + w * max_rows, dtype=torch.int32, device=pdev)
    if n_img:
        head = torch.tensor([[int(i), c] for i, c in zip(image_ids, counts)], dtype=torch.int32)
        buf[:2 * n_img] = head.reshape(-1).to(pdev, non_blocking=True)
    if n_rows:
        rows = buf[2 * max_img:2 * max_img + w * n_rows].view(n_rows, w)
        rows[:, :d] = torch.cat([c.to(device=pdev, dtype=torch.int32).reshape(-1, d) for c in coords], 0)
        rows[:, d] = torch.cat([s.to(device=pdev, dtype=torch.float32).reshape(-1) for s in scores], 0).view(torch.int32)
    if buf.device != device:
        buf = buf.to(device)
    marks.append(('pack', _time.perf_counter()))
    bufs = [torch.zeros_like(buf) for _ in range(world)] if rank == dst else None
    dist.gather(buf, bufs, dst=dst)
    marks.append(('gather', _time.perf_counter()))
    if trace:
        sys.stderr.write(f'[topaz_amd gather] rank {rank}: ' + ', '.join(f'{b[0]} {1e3 * (b[1] - a[1]):.1f} ms' for a, b in zip(marks, marks[1:]))
                         + f' ({n_rows} rows of {n_img} images, buffer {buf.numel() * 4} B)\n')
    if rank != dst:
        return None
    out = {}
    allb = torch.stack(bufs, 0).cpu()                          # one copy of everything gathered
    for r in range(world):
        h = allb[r, :2 * max_img].view(max_img, 2)
        rw = allb[r, 2 * max_img:].view(max_rows, w)
        off = 0
        for k in range(metas[r][0]):
            iid, n = int(h[k, 0]), int(h[k, 1])
            blk = rw[off:off + n]
            out[iid] = (blk[:, d].contiguous().view(torch.float32).clone(), blk[:, :d].clone())
            off += n
    return out


def gather_radius_records(per_radius_records: Sequence[Sequence[tuple]], image_ids: Sequence[int], device: torch.device,
                          dst: int = 0) -> Optional[list]:
    """Gather the `--targets` records of a whole radius sweep to rank `dst`.

    per_radius_records[k][j] is RadiusSearch.evaluate_local's record of this rank's j-th map at the k-th radius -- (hit flags
    fp32 [n], scores fp32 [n], squared error, number of targets) -- and image_ids[j] that map's position in the single-process
    image order.  A rank without maps passes empty lists and takes part all the same.
    Exchange, as in gather_pick_tables: one all_gather of (radii, records, picks) per rank fixes the stride, then ONE gather
    moves every rank's sweep as a single int64 buffer, padded to the largest rank: `max_rec` index rows of (radius slot, image
    id, n_picks, n_targets), `max_rec` squared errors (float64 bits), and per record its n flags followed by its n scores
    (float32 bits, two to a word) -- 8 n + 40 bytes per image and radius.  Every bit pattern travels unchanged.
    Returns on dst, per radius, the records sorted by image id; None on the other ranks."""
    n_slots = len(per_radius_records)
    flat = [(k, int(i), rec) for k, records in enumerate(per_radius_records) for i, rec in zip(image_ids, records)]
    if not (dist.is_available() and dist.is_initialized()):
        return [[rec for _, _, rec in sorted((f for f in flat if f[0] == k), key=lambda f: f[1])] for k in range(n_slots)]
    world, rank = dist.get_world_size(), dist.get_rank()
    n_rec = len(flat)
    n_picks = int(sum(len(rec[0]) for _, _, rec in flat))
    metas_t = torch.zeros(world * 3, dtype=torch.int64, device=device)
    dist.all_gather_into_tensor(metas_t, torch.tensor([n_slots, n_rec, n_picks], dtype=torch.int64, device=device))
    metas = metas_t.view(world, 3).cpu().tolist()
    if any(m[0] != n_slots for m in metas):
        raise RuntimeError(f'the ranks disagree on the number of radii: {[m[0] for m in metas]}')
    max_rec = max(1, max(m[1] for m in metas))
    max_picks = max(1, max(m[2] for m in metas))
    # packed on the host, where the records are (the Hungarian matching produced them there): one copy to the collective's device
    buf = np.zeros(5 * max_rec + max_picks, dtype=np.int64)
    index = buf[:4 * max_rec].reshape(max_rec, 4)
    sq_err = buf[4 * max_rec:5 * max_rec].view(np.float64)
    values = buf[5 * max_rec:].view(np.float32)
    off = 0
    for j, (k, i, (flags, scores, err, n_targets)) in enumerate(flat):
        n = len(flags)
        index[j] = (k, i, n, n_targets)
        sq_err[j] = err
        values[off:off + n] = flags
        values[off + n:off + 2 * n] = scores
        off += 2 * n
    t = torch.from_numpy(buf).to(device)
    bufs = [torch.zeros_like(t) for _ in range(world)] if rank == dst else None
    dist.gather(t, bufs, dst=dst)
    if rank != dst:
        return None
    allb = torch.stack(bufs, 0).cpu().numpy()                  # one copy of everything gathered
    slots: List[list] = [[] for _ in range(n_slots)]
    for r in range(world):
        index = allb[r, :4 * max_rec].reshape(max_rec, 4)
        sq_err = allb[r, 4 * max_rec:5 * max_rec].view(np.float64)
        values = allb[r, 5 * max_rec:].view(np.float32)
        off = 0
        for j in range(metas[r][1]):
            k, i, n, n_targets = (int(v) for v in index[j])
            slots[k].append((i, (values[off:off + n].copy(), values[off + n:off + 2 * n].copy(), float(sq_err[j]), n_targets)))
            off += 2 * n
    return [[rec for _, rec in sorted(s, key=lambda e: e[0])] for s in slots]


def broadcast_int(value: int, src: int = 0, device: Optional[torch.device] = None) -> int:
    """rank `src`'s integer on every rank (one broadcast); `value` itself without a process group"""
    if not (dist.is_available() and dist.is_initialized()):      # (a 1-rank group takes the collective path too)
        return int(value)
    t = torch.tensor([int(value)], dtype=torch.int64, device=device)
    dist.broadcast(t, src=src)
    return int(t.item())
