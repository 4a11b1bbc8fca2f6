"""Host-array pipeline: a ring of staging slots that puts the host's float32 narrowing, the upload and the download of
predict / evaluate / fit on host arrays UNDER the kernels of the neighbouring chunks.

A slot holds pinned float32 staging and a device tensor per input, a device buffer and pinned staging per result, and three
events.  Chunk k lives in slot k mod S:

    host      collect(k - S): wait out[s], copy the pinned result into its rows of the ONE result array
    host      stage(k):       narrow the chunk's rows straight into the pinned inputs
    upload    wait done[s] (the slot's device inputs were read by chunk k - S); pinned -> device; record up[s]
    compute   acquire(k):     wait up[s]; the caller's run(...) on the slot's device inputs, in chunk order
    compute   release(k):     result -> the slot's device buffer; record done[s]
    download  wait done[s]; device buffer -> pinned result; record out[s]

The compute stream is the caller's current one; the ring owns the upload and the download stream and no other.  The result
is copied into the slot's buffer ON the compute stream, so no tensor of the caching allocator is ever read on a foreign
stream (no record_stream).  The host blocks in event waits only: one per chunk (out[s] in predict, which implies up[s]; up[s]
where nothing comes back) and the drain at the end.

The ring talks to its buffers through a backend: TorchBackend (pinned memory, streams, events) on the GPU, NumpyBackend
(plain arrays, copies done at once, every operation logged) so that the plan, the narrowing, the budget and the error path
run on a machine without one.
"""
import os
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np

# What `model.host_pipeline = None` without FOV_HOST_PIPELINE means.  Decided by tools/host_pipeline_time.py: on
# only if the slowest pipelined round beats the fastest round of the serial loop at EVERY timed shape.
DEFAULT_ON = False
DEFAULT_BYTES = 1 << 30      # FOV_HOST_PIPELINE_BYTES: pinned bytes one ring may hold
MAX_THREADS = 16             # the narrowing never runs on more, whatever the machine has
_PER_THREAD = 1 << 20        # source bytes a thread must have to be worth starting
_OUT_ITEM = 8                # a result's dtype is known once chunk 0 has run: it is budgeted as the widest real type

_pool = None
_pool_lock = threading.Lock()


def enabled(attribute):
    """model.host_pipeline (True / False) wins; None: FOV_HOST_PIPELINE=0|1; neither: DEFAULT_ON."""
    if attribute is not None:
        return bool(attribute)
    env = os.environ.get("FOV_HOST_PIPELINE", "")
    return DEFAULT_ON if env == "" else env != "0"


def budget_bytes():
    return int(os.environ.get("FOV_HOST_PIPELINE_BYTES", str(DEFAULT_BYTES)))


def chunk_plan(n, batch_size):
    """[(lo, hi)] of the serial loop: `batch_size` rows at a time, None / 0: all rows in one chunk; no rows, no chunk."""
    bs = n if not batch_size else int(batch_size)
    return [(lo, min(lo + bs, n)) for lo in range(0, n, max(bs, 1))]


def is_host_array(a):
    """What the ring narrows itself: a NumPy array of a real dtype, whatever its strides."""
    return isinstance(a, np.ndarray) and a.dtype.kind in "biuf"


def slot_bytes(in_row_shapes, out_row_shapes, rows):
    """Pinned bytes of one slot: float32 inputs, results at _OUT_ITEM bytes an element."""
    count = lambda shapes: sum(int(np.prod(s, dtype=np.int64)) for s in shapes)
    return rows * (4 * count(in_row_shapes) + _OUT_ITEM * count(out_row_shapes))


def slots_for(per_slot, budget):
    """3 slots (upload k+1, compute k, download k-1) where they fit the budget, else 2, else 0: the serial loop."""
    for s in (3, 2):
        if s * per_slot <= budget:
            return s
    return 0


def _threads():
    global _pool
    with _pool_lock:
        if _pool is None:
            _pool = ThreadPoolExecutor(max_workers=MAX_THREADS, thread_name_prefix="fov-narrow")
        return _pool


def narrow(dst, src):
    """dst[...] = src as float32, bit for bit what np.ascontiguousarray(src, dtype=np.float32) holds (the same cast loop:
    round to nearest even, overflow to inf), for any real dtype and any strides, written straight into dst (pinned).  Rows
    are split over at most MAX_THREADS threads (NumPy casts outside the GIL), one per _PER_THREAD bytes of source."""
    n = src.shape[0] if src.ndim else 1
    parts = int(min(MAX_THREADS, n, src.nbytes // _PER_THREAD))
    with np.errstate(over="ignore", invalid="ignore"):
        if parts < 2:
            np.copyto(dst, src, casting="unsafe")
            return
        cut = [n * i // parts for i in range(parts + 1)]

        def part(a, b):
            with np.errstate(over="ignore", invalid="ignore"):      # (errstate is per thread)
                np.copyto(dst[a:b], src[a:b], casting="unsafe")
        for f in [_threads().submit(part, a, b) for a, b in zip(cut[:-1], cut[1:])]:
            f.result()


def gather(dst, src, rows):
    """dst[...] = src[rows] without the temporary of a fancy index: rows an index array (every entry in range) or a slice."""
    if isinstance(rows, slice):
        np.copyto(dst, src[rows])
    else:
        np.take(src, rows, axis=0, out=dst, mode="clip")


class TorchBackend:
    """Pinned host memory, device tensors, the two streams the ring owns and the caller's current one."""

    def __init__(self, device):
        import torch
        self.torch, self.device = torch, torch.device(device)
        self.streams = {"up": torch.cuda.Stream(device=self.device), "down": torch.cuda.Stream(device=self.device)}

    def _stream(self, name):
        return self.torch.cuda.current_stream(self.device) if name == "compute" else self.streams[name]

    def host(self, shape, like=None):
        return self.torch.empty(tuple(shape), dtype=self.torch.float32 if like is None else like.dtype, pin_memory=True)

    def dev(self, shape, like=None):
        return self.torch.empty(tuple(shape), dtype=self.torch.float32 if like is None else like.dtype, device=self.device)

    def array(self, buf):
        return buf.numpy()

    def event(self):
        return self.torch.cuda.Event()

    def copy(self, dst, src, stream):
        with self.torch.cuda.stream(self._stream(stream)):
            dst.copy_(src, non_blocking=True)

    def record(self, event, stream):
        event.record(self._stream(stream))

    def wait(self, stream, event):
        self._stream(stream).wait_event(event)

    def host_wait(self, event):
        event.synchronize()

    def drain(self):
        for name in ("up", "compute", "down"):
            self._stream(name).synchronize()


class NumpyBackend:
    """Plain arrays and no streams: every copy is done where it is queued, every operation is logged as
    (what, stream or None) - the ring's plan and ordering on a machine without a GPU."""

    def __init__(self):
        self.log = []
        self.bytes = 0

    def host(self, shape, like=None):
        a = np.empty(tuple(shape), np.float32 if like is None else like.dtype)
        self.bytes += a.nbytes
        return a

    def dev(self, shape, like=None):
        return np.empty(tuple(shape), np.float32 if like is None else like.dtype)

    def array(self, buf):
        return buf

    def event(self):
        return [0]       # how often it was recorded

    def copy(self, dst, src, stream):
        self.log.append(("copy", stream))
        np.copyto(dst, src)

    def record(self, event, stream):
        event[0] += 1
        self.log.append(("record", stream))

    def wait(self, stream, event):
        self.log.append(("wait", stream))

    def host_wait(self, event):
        assert event[0] > 0, "the host waits for an event nobody recorded"
        self.log.append(("host_wait", None))

    def drain(self):
        self.log.append(("drain", None))


class _Slot:
    def __init__(self, b, row_shapes, rows):
        self.host_in = [b.host((rows,) + tuple(s)) for s in row_shapes]
        self.view_in = [b.array(h) for h in self.host_in]
        self.dev_in = [b.dev((rows,) + tuple(s)) for s in row_shapes]
        self.dev_out = self.host_out = self.view_out = None      # made to fit the first result
        self.up, self.done, self.out = b.event(), b.event(), b.event()
        self.n = 0
        self.up_pending = False      # up recorded and the host has not waited past it: the pinned inputs are not free
        self.read = False            # done recorded at least once: the device inputs have had a reader


class Ring:
    """S slots of `rows` rows for inputs of `row_shapes` (float32).  One user at a time; chunks in order."""

    def __init__(self, backend, row_shapes, rows, slots):
        self.b, self.rows, self.S = backend, int(rows), int(slots)
        self.slots = [_Slot(backend, row_shapes, self.rows) for _ in range(self.S)]
        self.held = None

    def stage(self, k, fill, n):
        """fill(views) writes the chunk's n rows into the slot's pinned inputs (views of n rows); then the upload is queued."""
        s, b = self.slots[k % self.S], self.b
        if s is self.held:
            raise RuntimeError("slot %d is staged while its chunk is still held" % (k % self.S))
        if s.up_pending:
            b.host_wait(s.up)
            s.up_pending = False
        fill([v[:n] for v in s.view_in])
        s.n = n
        if s.read:
            b.wait("up", s.done)
        for d, h in zip(s.dev_in, s.host_in):
            b.copy(d[:n], h[:n], "up")
        b.record(s.up, "up")
        s.up_pending = True

    def acquire(self, k):
        """The chunk's device inputs, valid on the compute stream from here; an earlier chunk still held is released."""
        if self.held is not None:
            self.release()
        s = self.slots[k % self.S]
        self.b.wait("compute", s.up)
        self.held = s
        return [d[:s.n] for d in s.dev_in]

    def release(self, results=None):
        """Everything queued on the compute stream so far is what reads the held chunk's inputs.  results: device tensors
        of the chunk's rows, sent on their way to the host."""
        s, b = self.held, self.b
        self.held = None
        if results is not None:
            if s.dev_out is None:
                s.dev_out = [b.dev((self.rows,) + tuple(r.shape[1:]), like=r) for r in results]
                s.host_out = [b.host((self.rows,) + tuple(r.shape[1:]), like=r) for r in results]
                s.view_out = [b.array(h) for h in s.host_out]
            for d, r in zip(s.dev_out, results):
                if r.shape[0] != s.n or tuple(r.shape[1:]) != tuple(d.shape[1:]) or r.dtype != d.dtype:
                    raise ValueError("a chunk of %d rows returned %s %s where %s was expected" % (
                        s.n, tuple(r.shape), r.dtype, (s.n,) + tuple(d.shape[1:])))
                b.copy(d[:s.n], r, "compute")
        b.record(s.done, "compute")
        s.read = True
        if results is not None:
            b.wait("down", s.done)
            for h, d in zip(s.host_out, s.dev_out):
                b.copy(h[:s.n], d[:s.n], "down")
            b.record(s.out, "down")

    def collect(self, k):
        """The chunk's results as views of the slot's pinned staging, once they are there."""
        s = self.slots[k % self.S]
        self.b.host_wait(s.out)
        s.up_pending = False          # out follows done follows up
        return [v[:s.n] for v in s.view_out]

    def finish(self):
        if self.held is not None:
            self.release()

    def abort(self):
        """After an exception: nothing of the ring is in flight when this returns."""
        self.held = None
        self.b.drain()


def make_ring(backend_factory, in_row_shapes, out_row_shapes, rows, budget=None):
    """A ring for chunks of `rows` rows, or None where not even two slots fit the budget.  The backend is built only then."""
    slots = slots_for(slot_bytes(in_row_shapes, out_row_shapes, rows), budget_bytes() if budget is None else budget)
    return Ring(backend_factory(), in_row_shapes, rows, slots) if slots else None


def predict(ring, arrays, plan, call, several):
    """call(lo, hi, device inputs) over the chunks of `plan`, in order, through the ring; arrays: the host arrays the device
    inputs are the float32 of.  -> one preallocated result array (a list of them when `several`), filled chunk by chunk."""
    res = None

    def collect(j):
        nonlocal res
        parts = ring.collect(j)
        if res is None:
            res = [np.empty((plan[-1][1],) + p.shape[1:], p.dtype) for p in parts]
        lo, hi = plan[j]
        for r, p in zip(res, parts):
            r[lo:hi] = p

    for k, (lo, hi) in enumerate(plan):
        if k >= ring.S:
            collect(k - ring.S)
        ring.stage(k, lambda views: [narrow(v, a[lo:hi]) for v, a in zip(views, arrays)], hi - lo)
        o = call(lo, hi, ring.acquire(k))
        ring.release(list(o) if several else [o])
    for j in range(max(0, len(plan) - ring.S), len(plan)):
        collect(j)
    return res if several else res[0]


class Uploader:
    """Batches that only go up (evaluate, fit), in order.  next(fill, n) hands out the next batch's device tensors, staging it
    first if nobody has; ahead(fill, n) stages the batch next() will hand out, while the kernels of the one handed out
    before still run (it sits in another slot: S >= 2)."""

    def __init__(self, ring):
        self.ring, self.k, self.staged = ring, 0, 0      # batches handed out, batches staged

    def ahead(self, fill, n):
        if self.staged == self.k:
            self.ring.stage(self.k, fill, n)
            self.staged += 1

    def next(self, fill, n):
        self.ahead(fill, n)
        dev = self.ring.acquire(self.k)
        self.k += 1
        return dev
