"""The host-worker pipeline behind `--workers N` of the inference and evaluation CLIs (lwsnet_amd/inference.py,
lwsnet_amd/evaluate.py).

N spawned host worker PROCESSES decode and encode images in shared-memory slots; the parent uploads what they decoded, runs the
forwards through lws_pool (ForwardPool) and hands results back to them.  Python threads would do the workers' PNG work at most
~16-wide (the interpreter lock); processes scale with the host's cores.  The workers are fresh interpreters (`spawn`: a forked
child of a process that holds HIP state is not safe) that import numpy and PIL only and never touch the GPU, which is why this
module imports nothing else at its top; torch is imported inside what runs in the parent.

* `Slot`: one shared-memory block cut into regions by a layout, registered with HIP as pinned memory where the runtime allows
  (otherwise staged through pinned tensors).
* `HostWorkers`: the processes, their task and message queues, start-up, failure detection and teardown.
* `schedule`: the GPU side, on the calling thread only.  Each CLI supplies what a message does (upload and submit a full slot,
  or free it) and what retiring a job does.
"""
import collections
import multiprocessing as mp
import os
import queue
import time
from multiprocessing import shared_memory

import numpy as np

ALIGN = 256                                         # every region starts on a 256-byte boundary


def _offsets(layout):
    """Byte offset of each region of `layout` (a list of (shape, numpy dtype)) and the block's size."""
    offsets, end = [], 0
    for shape, dtype in layout:
        off = (end + ALIGN - 1) // ALIGN * ALIGN
        offsets.append(off)
        end = off + int(np.prod(shape)) * np.dtype(dtype).itemsize
    return offsets, end


def views(buf, layout):
    """numpy arrays over the regions of a block (any object with the buffer protocol)."""
    return [np.ndarray(shape, dtype, buffer=buf, offset=off) for (shape, dtype), off in zip(layout, _offsets(layout)[0])]


class Slot:
    """One shared-memory block that the host workers fill and read, with its regions as host tensors (`host[i]`).

    With a `device`, the block is registered with HIP as pinned memory where the runtime allows (`LWS_CLI_NO_HOST_REGISTER=1`
    refuses it), and otherwise staged through pinned tensors: copies between region i and the device go through `pinned(i)`,
    after `stage(i)` on the way up and followed by `unstage(i)` on the way down.  Without one the slot is plain shared memory
    (`views`: numpy arrays, as the workers see them)."""

    def __init__(self, layout, device=None):
        self.layout, self.device = layout, device
        self.shm = shared_memory.SharedMemory(create=True, size=_offsets(layout)[1])
        self.name = self.shm.name
        self.registered = False
        self.host = self._staging = None
        if device is None:
            self.views = views(self.shm.buf, layout)
            return
        import torch
        block = torch.frombuffer(self.shm.buf, dtype=torch.uint8)      # holds the buffer: close() cannot unmap it under a view
        if os.environ.get("LWS_CLI_NO_HOST_REGISTER") != "1":          # (tests force the staging path with it)
            try:
                rc = torch.cuda.cudart().cudaHostRegister(block.data_ptr(), block.numel(), 0)
                self.registered = int(rc) == 0 and block.is_pinned()
            except Exception:                                           # noqa: BLE001 (fall back to staging copies)
                self.registered = False
        self._ptr = block.data_ptr()
        self.host = [torch.from_numpy(v) for v in views(block.numpy(), layout)]
        if not self.registered:
            self._staging = [torch.empty(h.shape, dtype=h.dtype, pin_memory=True) for h in self.host]

    def pinned(self, i):
        """Region i in pinned memory, for an asynchronous copy to or from the device."""
        return self.host[i] if self.registered else self._staging[i]

    def stage(self, i):
        """Before an upload from pinned(i): the region's bytes into its staging copy (nothing to do when registered)."""
        if not self.registered:
            self._staging[i].copy_(self.host[i])

    def unstage(self, i):
        """After a download into pinned(i) has completed: the staging copy into the region (nothing to do when registered)."""
        if not self.registered:
            self.host[i].copy_(self._staging[i])

    def close(self):
        """Waits for the device (a copy may still use the block), unregisters, closes and unlinks."""
        self.host = self._staging = self.views = None
        if self.device is not None:
            import torch
            torch.cuda.synchronize(self.device)
            if self.registered:
                try:
                    torch.cuda.cudart().cudaHostUnregister(self._ptr)
                except Exception:                                       # noqa: BLE001
                    pass
        try:
            self.shm.close()
        except BufferError:                                             # a view is still alive somewhere: unlink anyway
            pass
        self.shm.unlink()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _worker(tasks, done, handler, blocks):
    """Body of a host worker process.  blocks[sid] = (name, layout) of slot sid, attached on first use.  A task is (sid, label,
    args): `handler(views of slot sid, *args)` returns (kind, value), posted as (kind, sid, value); an exception is posted as
    ("error", sid, "<label>: <type>: <message>").  None ends the loop."""
    shms, slot_views = {}, {}
    done.put(("ready", -1, None))                                       # interpreter up, numpy and PIL imported
    while True:
        task = tasks.get()
        if task is None:
            break
        sid, label, args = task
        try:
            if sid not in shms:
                name, layout = blocks[sid]
                shms[sid] = shared_memory.SharedMemory(name=name)
                slot_views[sid] = views(shms[sid].buf, layout)
            kind, value = handler(slot_views[sid], *args)
            done.put((kind, sid, value))
        except Exception as e:                                          # noqa: BLE001 (reported to the parent, which raises)
            done.put(("error", sid, f"{label}: {type(e).__name__}: {e}"))
    slot_views.clear()
    for shm in shms.values():
        shm.close()


class HostWorkers:
    """`n` host worker processes that run `handler` (a picklable callable of the worker side: numpy and PIL only) on tasks over
    `slots`.  Entering starts them; `wait_ready()` waits until all have started, so that the caller can warm the GPU up in the
    meantime.  `pending` counts the tasks put and not yet answered.  Exiting sends one None per worker, joins each for 10 s
    and terminates the ones still alive (only the children started here)."""

    def __init__(self, n, handler, slots):
        self.n, self._handler = n, handler
        self._blocks = [(sl.name, sl.layout) for sl in slots]
        self.procs, self.pending = [], 0

    def __enter__(self):
        ctx = mp.get_context("spawn")
        self._tasks, self._done = ctx.Queue(), ctx.Queue()
        try:
            for _ in range(self.n):
                pr = ctx.Process(target=_worker, args=(self._tasks, self._done, self._handler, self._blocks), daemon=True)
                pr.start()
                self.procs.append(pr)
        except BaseException:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        for _ in self.procs:
            self._tasks.put(None)
        for pr in self.procs:
            pr.join(timeout=10.0)
            if pr.is_alive():                  # e.g. blocked on the task queue's lock, which a killed worker held
                pr.terminate()
                pr.join(timeout=10.0)

    def _alive(self):
        return all(pr.is_alive() for pr in self.procs)

    def wait_ready(self):
        """Returns once every worker has started (spawn + imports: ~1 s, once); gives up after 120 s or when one has died."""
        ready, t0 = 0, time.perf_counter()
        while ready < self.n:
            try:
                msg = self._done.get(timeout=5.0)
            except queue.Empty:
                if not self._alive() or time.perf_counter() - t0 > 120.0:
                    raise RuntimeError("the host worker processes did not start")
                continue
            if msg[0] != "ready":
                raise RuntimeError(f"unexpected message from a host worker before its start-up: {msg}")
            ready += 1

    def put(self, sid, label, *args):
        """Queues handler(views of slot sid, *args); `label` names the task in an error."""
        self._tasks.put((sid, label, args))
        self.pending += 1

    def get(self):
        """The next (kind, sid, value) message.  Raises RuntimeError with the worker's text for an error message, or when a
        worker has died (checked every 5 s while no message comes)."""
        while True:
            try:
                msg = self._done.get(timeout=5.0)
            except queue.Empty:
                if not self._alive():
                    raise RuntimeError("a host worker process died")
                continue
            if msg[0] == "error":
                raise RuntimeError(msg[2])
            self.pending -= 1
            return msg


def schedule(host, depth, handle, retire, decoding):
    """The GPU side of the pipeline, on the calling thread only (ForwardPool is not to be shared between threads).  Jobs in
    flight wait in a FIFO; the oldest is retired when `depth` of them are in flight or no decode is pending (`decoding()` is
    false); otherwise the next message of the host workers is served.
    handle(kind, sid, value) -> a job to put in flight, or None;  retire(job) -> a value, yielded.
    Ends when no job is in flight and no task is pending."""
    inflight = collections.deque()
    while inflight or host.pending:
        if inflight and (len(inflight) >= depth or not decoding()):
            yield retire(inflight.popleft())
            continue
        job = handle(*host.get())
        if job is not None:
            inflight.append(job)
