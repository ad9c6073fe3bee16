"""LLC4320 time slices streamed from disk into the training loop.

``srmi.llc.LLCSource.load_region_data`` + ``get_tiles`` read every wet-value file
whole, upload it from pageable memory and stop the host for the keep list, all
of it serial with training.  ``TimesliceFeed`` produces the same tiles (bit for
bit: the same three kernels, srmi_llc_gather, srmi_tiles_nonfinite and the tile
gather, run on the same values) without any of the three:

* reader threads fetch only the file blocks the ROI touches
  (``LLCSource.read_plan``) into pinned staging memory -- file I/O only;
* the device work of a slice (H2D copies, srmi_llc_gather per variable,
  srmi_tiles_nonfinite, srmi_tiles_keep, srmi_tiles_gather_dev, the D2H copy of
  the tile count) is enqueued by the CONSUMING thread on the feed's own stream,
  from ``poll()``, as soon as the slice's bytes are in pinned memory; the keep
  list never visits the host;
* ``timeslice(i)`` makes the consumer's stream wait for the slice (a stream wait;
  the host waits only for the two-int tile count), then starts the prefetch of
  slice ``(i + 1) % len(paths)``.  ``poll()`` runs on every ``timeslice()`` and,
  through ``prepare()``, on every batch, so slice i + 1's device stage starts
  during slice i's steps.

Ordering rules.  The feed has ``depth`` slots; a slot is pinned staging per
variable plus the device buffers of one slice (compact words, region, flags,
keep list, count, tiles).

1. A slot's device buffers are overwritten only after the feed stream has waited
   on ``released[slot]``.  That event is recorded on the consumer's current stream
   when the consumer asks for a later slice (any later ``timeslice()`` call): the
   tiles ``timeslice(i)`` returned are views of the slot and stay valid until then.
2. A slot's pinned staging is refilled only after the slot's H2D event has
   completed.  The reader synchronises on that event before it reads a file (a
   host-side wait, its only call into the runtime).  Pinned staging and device
   buffers are separate resources: with ``depth=1`` the next slice's file reads
   still overlap training, its device stage does not.
3. Everything the consumer enqueues on a slice's tiles goes on the stream that was
   current when it called ``timeslice()`` (or on streams that stream waits for, as
   FusedTrainer.step's do).

An exception in a reader thread is kept and raised from the next ``timeslice()``
call.
"""
from __future__ import annotations

import queue
import threading
import time
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import call, ptr
from .llc import LLCSource, min_wet_pixels

MAX_READERS = 4
_IDLE, _READING, _LOADED, _ENQUEUED = range(4)


class _Slot:
    def __init__(self, nvars: int, n_words: int, ys: int, xs: int, ncells: int, ty: int, tx: int, dev):
        i32 = dict(dtype=torch.int32, device=dev)
        nw = max(1, n_words)
        self.pinned = [torch.empty(nw, dtype=torch.int32).pin_memory() for _ in range(nvars)]
        self.words = [torch.empty(nw, **i32) for _ in range(nvars)]
        self.region = torch.empty(nvars, ys, xs, dtype=torch.float32, device=dev)
        self.bad = torch.empty(nvars * ncells, **i32)
        self.src = torch.empty(nvars * ncells, **i32)
        self.count = torch.zeros(2, **i32)
        self.tiles = torch.empty(ncells, nvars, ty, tx, dtype=torch.float32, device=dev)
        self.count_host = torch.zeros(2, dtype=torch.int32).pin_memory()
        self.src_host = torch.zeros(nvars * ncells, dtype=torch.int32).pin_memory()
        self.h2d, self.ready, self.counted, self.released = (torch.cuda.Event() for _ in range(4))
        self.stage = _IDLE
        self.slice: Optional[int] = None      # the slice being read / staged
        self.held: Optional[int] = None       # the slice whose tiles the consumer holds
        self.wait_release = False             # `released` is recorded and not yet waited on
        self.pending = 0
        self.error: Optional[BaseException] = None
        self.t_submit = 0.0


class TimesliceFeed:
    """source: an LLCSource; paths[i]: the per-variable files of time slice i; tile:
    the (square) tile size.  depth slots, readers threads (at most MAX_READERS; never
    sized from the machine's CPU count), block_words / max_gap_blocks: the read plan
    (LLCSource.read_plan).  land / min_wet (a fraction of the tile plane): keep the
    coastal tiles, as srmi.llc.get_tiles(min_wet=); land=False is the reference's rule.
    Use as a context manager, or close()."""

    def __init__(self, source: LLCSource, paths: Sequence[Sequence[str]], tile: int, depth: int = 2,
                 readers: int = 2, block_words: int = 1024, max_gap_blocks: int = 0,
                 device: Optional[torch.device] = None, land: bool = False, min_wet: float = 0.25):
        if depth < 1 or readers < 1:
            raise ValueError("TimesliceFeed: depth and readers must be at least 1")
        # land: coastal tiles are kept (srmi_tiles_dry in place of srmi_tiles_nonfinite) when
        # every channel has min_wet of the tile plane wet, and prepare() normalises them over
        # their wet pixels (prep_batch(land=True)); train them with FusedTrainer(land=True)
        self.land = bool(land)
        self.min_wet = min_wet_pixels(min_wet, int(tile), int(tile)) if self.land else None
        if not paths or any(len(p) != len(paths[0]) or not len(p) for p in paths):
            raise ValueError("TimesliceFeed: every time slice needs the same, non-empty list of variable files")
        self.source = source
        self.device = device or source.device
        if self.device != source.device:
            raise ValueError(f"TimesliceFeed: device {self.device} but the source's index map is on {source.device}")
        self.paths = [list(p) for p in paths]
        self.nvars = len(self.paths[0])
        self.ty = self.tx = int(tile)
        self.ys, self.xs = source.ys, source.xs
        self.gy, self.gx = self.ys // self.ty, self.xs // self.tx
        self.ncells = self.gy * self.gx
        if self.ncells < 1:
            raise ValueError(f"TimesliceFeed: no {tile}-tile fits the {self.ys} x {self.xs} ROI")
        with torch.cuda.device(self.device):
            self.plan = source.read_plan(block_words, max_gap_blocks)
            self.stream = torch.cuda.Stream(device=self.device)
            self.slots = [_Slot(self.nvars, self.plan.n_words, self.ys, self.xs, self.ncells, self.ty, self.tx,
                                self.device) for _ in range(depth)]
            self.stream.wait_stream(torch.cuda.current_stream(self.device))  # the plan's index map is complete
        self._hr: Optional[torch.Tensor] = None
        self._cv = threading.Condition()
        self._jobs: "queue.Queue" = queue.Queue()
        self._stats: Dict[str, list] = {"read_s": [], "read_bytes": [], "read_wait_s": [], "enqueue_s": [],
                                        "count_wait_s": []}
        self._closed = False
        self._threads = [threading.Thread(target=self._reader, name=f"srmi-feed-reader-{k}", daemon=True)
                         for k in range(min(int(readers), MAX_READERS))]
        for t in self._threads:
            t.start()

    # ------------------------------------------------------------ reader side
    def _reader(self) -> None:
        """File I/O only: no kernel, copy or allocation is issued from here."""
        while True:
            job = self._jobs.get()
            if job is None:
                return
            slot, v, path = job
            err = None
            try:
                slot.h2d.synchronize()  # rule 2: the staging's last upload is complete
                self.plan.read_into(path, slot.pinned[v])
            except BaseException as e:  # kept for the consumer (timeslice() raises it)
                err = e
            with self._cv:
                if err is not None and slot.error is None:
                    slot.error = err
                slot.pending -= 1
                if slot.pending == 0:
                    self._stats["read_s"].append(time.perf_counter() - slot.t_submit)
                    self._stats["read_bytes"].append(self.plan.nbytes * self.nvars)
                self._cv.notify_all()

    def _submit(self, slot: _Slot, i: int) -> None:
        with self._cv:
            slot.stage, slot.slice, slot.error = _READING, i, None
            slot.pending = self.nvars
            slot.t_submit = time.perf_counter()
        for v, path in enumerate(self.paths[i]):
            self._jobs.put((slot, v, path))

    # ---------------------------------------------------------- consumer side
    def _enqueue(self, slot: _Slot) -> None:
        """The device stage of the slice in slot's staging, on the feed stream."""
        t0 = time.perf_counter()
        st, plan = self.stream, self.plan
        C, npix = self.nvars, self.ys * self.xs
        if slot.wait_release:
            st.wait_event(slot.released)  # rule 1
            slot.wait_release = False
        h = st.cuda_stream
        with torch.cuda.stream(st):
            for v in range(C):
                slot.words[v].copy_(slot.pinned[v], non_blocking=True)
            slot.h2d.record(st)
            for v in range(C):
                call("srmi_llc_gather", ptr(slot.words[v]), plan.n_words, ptr(plan.idx), npix, ptr(slot.region[v]), h)
            if self.land:
                call("srmi_tiles_dry", ptr(slot.region), C, self.ys, self.xs, self.ty, self.tx, self.min_wet,
                     ptr(slot.bad), None, h)
            else:
                call("srmi_tiles_nonfinite", ptr(slot.region), C, self.ys, self.xs, self.ty, self.tx, ptr(slot.bad), h)
            call("srmi_tiles_keep", ptr(slot.bad), C, self.ncells, ptr(slot.src), ptr(slot.count), h)
            call("srmi_tiles_gather_dev", ptr(slot.region), C, self.ys, self.xs, self.ty, self.tx, ptr(slot.src),
                 ptr(slot.count), C * self.ncells, ptr(slot.tiles), h)
            slot.src_host.copy_(slot.src, non_blocking=True)
            slot.count_host.copy_(slot.count, non_blocking=True)
            slot.counted.record(st)
            slot.ready.record(st)
        slot.stage = _ENQUEUED
        self._stats["enqueue_s"].append(time.perf_counter() - t0)

    def poll(self) -> None:
        """Enqueue the device stage of every slot whose bytes have arrived and whose
        device buffers the consumer no longer holds.  Cheap; never blocks or raises."""
        for slot in self.slots:
            if slot.stage == _READING:
                with self._cv:
                    if slot.pending == 0 and slot.error is None:
                        slot.stage = _LOADED
            if slot.stage == _LOADED and slot.held is None:
                self._enqueue(slot)

    def _wait_read(self, slot: _Slot) -> None:
        with self._cv:
            while slot.pending:
                self._cv.wait()
            err, slot.error = slot.error, None
        if err is not None:
            slot.stage, slot.slice = _IDLE, None
            raise err
        if slot.stage == _READING:
            slot.stage = _LOADED

    def _free_slot(self) -> _Slot:
        idle = [s for s in self.slots if s.stage == _IDLE]
        if idle:  # one the consumer does not hold first: its device stage can start at once
            return min(idle, key=lambda s: s.held is not None)
        slot = self.slots[0]  # every slot stages some other slice (random access): drop one
        self._wait_read(slot)
        slot.stage, slot.slice = _IDLE, None
        return slot

    def _start(self, i: int) -> _Slot:
        for s in self.slots:
            if s.stage != _IDLE and s.slice == i:
                return s
        slot = self._free_slot()
        self._submit(slot, i)
        return slot

    def timeslice(self, i: int) -> Tuple[torch.Tensor, np.ndarray, Tuple[int, int]]:
        """-> (raw tiles [n, C, tile, tile] on the device, tile ids, (gy, gx)): what
        get_tiles(load_region_data(paths[i]), tile, tile) returns.  The tiles are views
        of a slot and stay valid until the next timeslice() call."""
        if self._closed:
            raise RuntimeError("TimesliceFeed is closed")
        if not 0 <= i < len(self.paths):
            raise IndexError(f"time slice {i} of {len(self.paths)}")
        cur = torch.cuda.current_stream(self.device)
        for s in self.slots:  # the consumer is past every slice it held
            if s.held is not None:
                s.released.record(cur)
                s.held, s.wait_release = None, True
        for s in self.slots:  # a reader's failure, whichever slice it was for
            if s.stage == _READING:
                with self._cv:
                    failed = s.pending == 0 and s.error is not None
                if failed:
                    self._wait_read(s)
        slot = self._start(i)
        t0 = time.perf_counter()
        self._wait_read(slot)
        self._stats["read_wait_s"].append(time.perf_counter() - t0)
        self.poll()  # enqueues this slot's stage unless poll() already did
        t0 = time.perf_counter()
        slot.counted.synchronize()
        self._stats["count_wait_s"].append(time.perf_counter() - t0)
        cur.wait_event(slot.ready)
        n = int(slot.count_host[0])
        ids = slot.src_host[:n].numpy().astype(np.int64)  # keep[:n], as get_tiles
        slot.stage, slot.slice, slot.held = _IDLE, None, i
        if len(self.paths) > 1:
            self._start((i + 1) % len(self.paths))
        return slot.tiles[:n], ids, (self.gy, self.gx)

    def timeslices(self) -> List[Callable[[], torch.Tensor]]:
        """The callables harness.train_timeslices takes (raw tiles: train with prepare())."""
        return [lambda i=i: self.timeslice(i)[0] for i in range(len(self.paths))]

    def norm_stats(self):
        """One pass over the slices -> the finalised srmi.norm.NormStats the dataset
        norm modes (gnorm, gscale, tnorm, tscale) need.  A land feed raises: its tiles
        hold NaN, and srmi_tile_stats over them is NaN."""
        from .norm import NormStats
        if self.land:
            raise ValueError("norm_stats: the tiles of a land=True feed hold NaN; compute the statistics with a "
                             "land=False TimesliceFeed over the same files and pass them as stats= (the gnorm / "
                             "gscale constants do not depend on the tile)")
        return NormStats.compute(self.timeslices())

    def prepare(self, norm: str = "lnorm", stats=None, scale: Optional[int] = None
                ) -> Callable[[torch.Tensor, int, int, int], torch.Tensor]:
        """The `prepare` of harness.train_timeslices: norm + xyflip of a raw batch
        (srmi.batch.prep_batch, no LR: the step forms its own) into one reused HR
        buffer, then poll().  The buffer is rewritten by the next call: the step that
        read it was enqueued before, on the same stream."""
        from .batch import prep_batch
        from .norm import DATASET_NORMS, check_norm
        if check_norm(norm) in DATASET_NORMS and stats is None:
            raise ValueError(f"prepare: norm {norm!r} needs the dataset statistics (stats=feed.norm_stats())")

        def prep(raw: torch.Tensor, start: int, gb: int, flip_index: int) -> torch.Tensor:
            b = raw.shape[0]
            if self._hr is None or self._hr.shape[0] < b or self._hr.shape[1:] != raw.shape[1:]:
                self._hr = torch.empty((max(b, gb),) + tuple(raw.shape[1:]), dtype=torch.float32, device=raw.device)
            hr = self._hr[:b]
            if b:
                prep_batch(raw, flip_index, 4 if scale is None else int(scale), with_lr=False, hr=hr, norm=norm,
                           stats=stats, tile_range=(start, start + b), land=self.land)
            self.poll()
            return hr
        return prep

    def stats(self) -> Dict[str, list]:
        """Host timers, one entry per slice staged so far: read_s (submission to the
        last byte, wall, in the reader threads) and read_bytes; on the consuming thread
        read_wait_s (its wait in timeslice() for the slice's bytes), enqueue_s (its time
        in the device stage's launches) and count_wait_s (its wait for the tile count)."""
        with self._cv:
            return {k: list(v) for k, v in self._stats.items()}

    def close(self) -> None:
        if self._closed:
            return
        self._closed = True
        for _ in self._threads:
            self._jobs.put(None)
        for t in self._threads:
            t.join()
        self.stream.synchronize()

    def __enter__(self) -> "TimesliceFeed":
        return self

    def __exit__(self, *exc) -> None:
        self.close()
