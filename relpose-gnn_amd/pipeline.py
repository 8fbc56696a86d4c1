"""The micro-batch pipeline under ``evaluate.evaluate_stream``, ``evaluate.relocalize`` and ``lookahead.Lookahead``: host ->
device staging of the node images through pinned double buffers (``_InputPipeline``), one forward per micro-batch with the
asynchronous read-back of its results (``_MicroBatchRunner``), the three-stage loop that overlaps them with the host's
post-processing (``drive``) and the cut of a micro-batch's edges into its graphs (``cut_per_graph``).  The clients supply what
differs between them -- how a chunk becomes the forward's input, which forward runs, what comes back -- and nothing else."""
from __future__ import annotations

import os
import time
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as _L
from .graph import Batch, Data


def staging_workers(fp32_staging: bool, local_world: int = 1, available: Optional[int] = None, override: Optional[str] = None) -> int:
    """Staging threads of one rank's input pipeline.  One rank alone: 8 threads reach the ~40 GB/s a single fp32 stream needs, 16
    the bf16 stream's ~55 GB/s (memcpy for fp32 staging, rpg_host_f32_to_bf16 for bf16 staging).  But the host's copy rate PEAKS
    at ~16 threads IN ALL and collapses beyond (2 x EPYC 9575F, profiles/r5_stage_scale_*.jsonl: numpy copies 273 GB/s with 16
    threads, 81 with 64, 49 with 128; eight ranks' pipelines together stage 55 GB/s with 16 threads each, 73 with 8, 136 with 4,
    200 with TWO), so the ranks of one host share that budget: 16 // local_world threads per rank, at least 2 -- never more than
    the CPUs the process may run on.  RPG_STAGE_WORKERS (``override``) fixes the count."""
    own = 8 if fp32_staging else 16
    share = max(2, 16 // max(1, int(local_world)))
    if available is None:
        available = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 2) // 2
    forced = int((os.environ.get("RPG_STAGE_WORKERS", "0") if override is None else override) or 0)
    return max(1, min(forced or min(own, share), max(1, int(available))))


def staging_dtype(uint8: bool, pinned_fp32: bool, accepts_bf16: bool, bf16_input: Optional[bool] = None, local_world: int = 1,
                  workers: Optional[int] = None) -> torch.dtype:
    """The dtype in which a micro-batch of host images crosses the link.  uint8 frames go as they are.  Otherwise bf16 for a
    model that takes host-rounded bf16 images (``accepts_bf16``; ``bf16_input`` overrides it), fp32 for the rest: the bf16
    encoder rounds its fp32 input first thing, so the forward is bit-identical and the copy half the size.  With
    ``bf16_input=None`` a micro-batch whose fp32 images ALL sit in pinned host memory -- what the reference's
    DataLoader(pin_memory=True) delivers, testing/test.py:193 -- depends on what the rank can spend: the rounding pass halves
    the H2D bytes, and a Gen5 x16 link carries 51 GB/s = 6.1 k graphs/s of fp32 256 x 341 images where the bf16 forward does
    8 k; with the staging overlapped with the post-processing (round 6) 16 rounding threads deliver 7.8 k graphs/s, so a rank
    with >= 8 staging threads (``workers``, default ``staging_workers(False, local_world)``: one or two ranks per host) rounds,
    and a rank with its 2-4 threads of an 8-rank host (2 threads round ~27 ms per micro-batch) sends the loader's tensors as
    they are, with no host pass at all.  ``pinned_fp32``: a bool, or a function asked only where the answer decides."""
    if uint8:
        return torch.uint8
    if not (bf16_input if bf16_input is not None else accepts_bf16):
        return torch.float32
    if workers is None:
        workers = staging_workers(False, local_world)
    if bf16_input is None and workers < 8 and (pinned_fp32() if callable(pinned_fp32) else pinned_fp32):
        return torch.float32
    return torch.bfloat16


class _InputPipeline:
    """Host -> device staging of the node images of an evaluation stream, double buffered.

    The reference's loader hands over one graph at a time from pinned memory (``DataLoader(..., pin_memory=True)``,
    testing/test.py:193) and copies it with ``data.to(device)`` (:211).  Here a micro-batch of graphs is collated straight
    into one of TWO pinned host buffers (a ``copy_`` per graph: no ``torch.cat`` temporary, no pageable H2D), sent to one of
    two device buffers on a dedicated copy stream, and the forward of micro-batch i runs while micro-batch i+1 is being
    collated and copied.  Events order the three parties: ``sent[k]`` (copy stream: buffer k is on the device; the host may
    refill the pinned half, the compute stream may read the device half) and ``used[k]`` (compute stream: the forward that
    read device buffer k is done; the copy stream may overwrite it).  Graphs whose ``x`` is already pinned skip the staging
    copy; graphs already on the device skip the pipeline altogether (``_MicroBatchRunner`` collates them on the device)."""

    def __init__(self, device, rows: int, row_floats: int, dtype=torch.float32, local_world: int = 1):
        # dtype = torch.bfloat16: the images are ROUNDED TO bf16 WHILE THEY ARE STAGED (the bf16 encoder rounds its fp32 input
        # first thing, so the forward is bit-identical) and the H2D copy is half the size -- at 256x341 the fp32 copy of a
        # 64-graph micro-batch (537 MB, ~13.7 ms at the 39 GB/s this host reaches) outlasts the bf16 forward (9 ms)
        self.device = device
        self.dtype = dtype
        self.copy_stream = torch.cuda.Stream(device=device)
        self.host = [torch.empty((rows, row_floats), dtype=dtype, pin_memory=True) for _ in range(2)]
        # dtype = torch.uint8: camera frames (the model's frame_transform runs the image transform on the device), copied as they are
        self.host_np = [t.numpy() for t in self.host] if dtype != torch.bfloat16 else None
        self.workers = staging_workers(dtype != torch.bfloat16, local_world)
        self.pool = ThreadPoolExecutor(max_workers=self.workers) if self.workers > 1 else None
        self.dev = [torch.empty((rows, row_floats), dtype=dtype, device=device) for _ in range(2)]
        self.sent = [torch.cuda.Event() for _ in range(2)]
        self.used = [torch.cuda.Event() for _ in range(2)]
        self.n_sent = [0, 0]
        self.staged_bytes = 0       # pageable -> pinned through the staging threads
        self.direct_bytes = 0       # sent straight out of the caller's own pinned tensors (no staging copy)

    def fits(self, rows: int, row_floats: int, dtype=torch.float32) -> bool:
        return rows <= self.host[0].shape[0] and row_floats == self.host[0].shape[1] and dtype == self.dtype

    def stage(self, k: int, chunk) -> torch.Tensor:
        """Collate the chunk's node images into pinned buffer k and enqueue the H2D copy; returns the device view."""
        return self.stage_end(self.stage_begin(k, chunk))

    def stage_begin(self, k: int, chunk):
        """First half of ``stage``: hand the chunk's pageable -> pinned copies (or bf16 roundings) to the staging threads and
        return at once; ``stage_end`` waits for them and enqueues the H2D copy.  Between the two the caller may do other host
        work (round 6: the streams post-process the previous micro-batch there -- the copies release the GIL)."""
        if self.n_sent[k]:
            self.sent[k].synchronize()                 # the previous copy out of pinned buffer k has left the host
        host, dev, off = self.host[k], self.dev[k], 0
        direct = []                                    # graphs whose x is already pinned: copied from where they are
        jobs = []
        for g in chunk:
            n = g.x.shape[0]
            if g.x.is_pinned() and g.x.dtype == self.dtype and (g.x.dim() == 2 or g.x.is_contiguous()):
                direct.append((off, n, g.x if g.x.dim() == 2 else g.x.view(n, -1)))
                self.direct_bytes += g.x.numel() * g.x.element_size()
            else:
                jobs.append((off, n, g.x))
                self.staged_bytes += g.x.numel() * host.element_size()
            off += n
        if jobs:
            # pageable -> pinned by a few worker threads (numpy releases the GIL; one memcpy stream moves ~5 GB/s on the GPU
            # host, measured r3: 649 graphs/s single-threaded against 1808 with resident images at 256x341)
            host_np = self.host_np[k] if self.host_np is not None else None
            cvt = _L.lib().rpg_host_f32_to_bf16 if host_np is None else None

            def copy_some(part):
                for o, n, src in part:
                    if host_np is not None:
                        np.copyto(host_np[o:o + n], src.detach().reshape(n, -1).numpy())
                    else:
                        # fp32 -> bf16 (round to nearest even) on the way, in the library's host helper (ctypes releases the GIL)
                        t = src.detach()
                        if t.dtype != torch.float32 or not t.is_contiguous():
                            host[o:o + n].copy_(t)
                        else:
                            _L.check(cvt(t.data_ptr(), host[o:o + n].data_ptr(), t.numel()), "host_f32_to_bf16")
            w = min(len(jobs), self.workers)
            if w <= 1:
                copy_some(jobs)
                futs = []
            else:
                futs = [self.pool.submit(copy_some, jobs[i::w]) for i in range(w)]
        else:
            futs = []
        return k, off, direct, futs

    def stage_end(self, handle) -> torch.Tensor:
        k, off, direct, futs = handle
        host, dev = self.host[k], self.dev[k]
        for f in futs:
            f.result()
        with torch.cuda.stream(self.copy_stream):
            if self.n_sent[k]:
                self.copy_stream.wait_event(self.used[k])      # the forward that read device buffer k has finished
            if direct:
                lo = 0
                for o, n, src in direct:
                    if o > lo:
                        dev[lo:o].copy_(host[lo:o], non_blocking=True)
                    dev[o:o + n].copy_(src, non_blocking=True)
                    lo = o + n
                if off > lo:
                    dev[lo:off].copy_(host[lo:off], non_blocking=True)
            else:
                dev[:off].copy_(host[:off], non_blocking=True)
            self.sent[k].record(self.copy_stream)
        self.n_sent[k] += 1
        return dev[:off]

    def acquire(self, k: int) -> None:
        torch.cuda.current_stream().wait_event(self.sent[k])

    def release(self, k: int) -> None:
        self.used[k].record(torch.cuda.current_stream())


def _frame_shape(chunk: Sequence[Data]):
    """(H, W, 3) if the chunk's node images are uint8 frames [n, H, W, 3] (all of one size), None for processed images."""
    if not any(g.x.dtype == torch.uint8 for g in chunk):
        return None
    shapes = {tuple(g.x.shape[1:]) if g.x.dtype == torch.uint8 and g.x.dim() == 4 else None for g in chunk}
    if len(shapes) != 1 or None in shapes or next(iter(shapes))[-1] != 3:
        raise ValueError("a micro-batch with uint8 frames must hold frames [n, H, W, 3] of one size only, got "
                         f"{sorted(str(s) for s in shapes)}")
    return next(iter(shapes))


def _collate_on_device(chunk: Sequence[Data], x_dev: torch.Tensor, device) -> Batch:
    """The PyG collation of ``chunk`` (graph.Batch.from_data_list) with the node images already on the device in ``x_dev``:
    only the index tensors are built on the host (a few KB) and copied."""
    eis, bs, off = [], [], 0
    for gi, g in enumerate(chunk):
        n = g.x.shape[0]
        eis.append(g.edge_index + off)
        bs.append(torch.full((n,), gi, dtype=torch.int64))
        off += n
    out = Batch(x=x_dev, edge_index=torch.cat(eis, 1).to(device, non_blocking=True), y=None, edge_attr=None,
                batch=torch.cat(bs, 0).to(device, non_blocking=True))
    out.graph_sizes = ([g.x.shape[0] for g in chunk], [int(g.edge_index.shape[1]) for g in chunk])
    return out


# what ``_MicroBatchRunner.launch`` hands back: the chunk, the forward's input (``batch.x``: the chunk's images on the device,
# rows in chunk order), the results by name in (pinned) host memory and the event that marks their arrival (None on the CPU)
_Launched = namedtuple("_Launched", "chunk batch host ev")


class _MicroBatchRunner:
    """Launch side of the pipeline: bring a chunk of ``Data`` objects to the device (through the pinned double buffers of
    ``_InputPipeline`` when the images live on the host and the model on the GPU), run ONE forward over it and start the
    asynchronous copy of its results into pinned host memory.  ``launch`` returns without waiting.

    The three steps a client may replace, each with the graph stream's as its default: ``collate(chunk, x_dev)`` -> the
    forward's input (``x_dev``: the staged images, None for a chunk that was not staged); ``forward(chunk, batch)`` -> whatever
    the model returns, run between the staging buffer's acquire and release; ``outputs(chunk, batch, fwd)`` -> {name: device
    tensor or None}, read back in that order behind ONE event.  Without a GPU there is no staging, no copy and no event: the
    forward's own tensors are handed on."""

    def __init__(self, model, device, micro_batch: int, bf16_input: Optional[bool] = None, local_world: int = 1,
                 want_abs: bool = False, pose=None, collate=None, forward=None, outputs=None, capacity: Optional[int] = None,
                 want_var: bool = False):
        self.model, self.device, self.micro_batch = model, device, int(micro_batch)
        # pose (query_pose.QueryPose, GPU only): the pose rule of test.py:213-267 runs on the device behind the forward, and what
        # comes back is its [G, 16] block (pred, targ, errors) INSTEAD of the relative poses and a model-built edge list
        self.pose = pose
        self.bf16_input, self.local_world, self.want_abs = bf16_input, local_world, want_abs
        # want_var: the variances model.mc_dropout leaves behind the forward come back with the relative poses (a weighted host rule)
        self.want_var = want_var
        self.rounding_workers = staging_workers(False, local_world)      # what staging_dtype weighs for pinned fp32 sources
        self.collate, self.forward, self.outputs = collate or self._collate, forward or self._forward, outputs or self._outputs
        # rows of a staging buffer: what the client says its largest micro-batch holds, else the chunk's largest graph x micro_batch
        self.capacity = capacity
        self.on_gpu = torch.device(device).type == "cuda"
        self.pipes = {}                    # staging dtype -> _InputPipeline (at most two: the configured dtype, fp32 for pinned sources)
        self.n_batches = 0
        self.nodes_seen = 0                # nodes of the micro-batches forwarded so far: model.mc_dropout's node_base of the next one
        self.mc_draw = None                # model.mc_dropout's draw counter when the stream began (held until end_draw)
        self.h2d_bytes = 0
        self.d2h_bytes = 0                 # payload copied back per micro-batch (poses / edge list / pose rows; not the status words)
        self._prefetched = None            # (chunk, pipe, stage_begin handle) of the chunk the next launch() is expected to get

    def _staging_dtype(self, xs) -> torch.dtype:
        return staging_dtype(any(x.dtype == torch.uint8 for x in xs), lambda: all(x.dtype == torch.float32 and x.is_pinned() for x in xs),
                             getattr(self.model, "accepts_bf16_input", False), self.bf16_input, self.local_world, self.rounding_workers)

    def pieces(self, x: torch.Tensor, first: int) -> Sequence[Data]:
        """Rows ``first ...`` of a client's image tensor as a chunk: cut in one piece per staging thread when they are going to
        be staged (a pinned source still goes out as one copy per piece), whole otherwise."""
        if not self.on_gpu or x.is_cuda:
            return [Data(x=x, first=first)]
        w = max(1, min(staging_workers(self._staging_dtype([x]) != torch.bfloat16, self.local_world), x.shape[0]))
        step = -(-x.shape[0] // w)
        return [Data(x=x[j:j + step], first=first + j) for j in range(0, x.shape[0], step)]

    def _begin_staging(self, k: int, chunk):
        """Pick (or build) the chunk's pipeline and start its staging copies: -> (pipe, handle of _InputPipeline.stage_begin)."""
        rows = sum(g.x.shape[0] for g in chunk)
        dtype = self._staging_dtype([g.x for g in chunk])
        fshape = _frame_shape(chunk)                                # uint8 frames: sent as they are, whatever the model takes
        width = int(np.prod(fshape if fshape is not None else chunk[0].x.shape[1:]))
        pipe = self.pipes.get(dtype)
        if pipe is None or not pipe.fits(rows, width, dtype):
            if pipe is not None:
                torch.cuda.synchronize(self.device)                 # a larger buffer pair replaces one that is in flight
            cap = self.capacity or max(rows, max(g.x.shape[0] for g in chunk) * self.micro_batch)
            pipe = self.pipes[dtype] = _InputPipeline(torch.device(self.device), cap, width, dtype, self.local_world)
        return pipe, pipe.stage_begin(k, chunk)

    def prefetch(self, chunk: Sequence[Data]) -> None:
        """Start staging the chunk the NEXT ``launch`` call will get (its pageable -> pinned copies / bf16 roundings run on the
        staging threads while the caller does other host work); ``launch`` picks the result up if it is handed the same chunk."""
        if self._prefetched is not None or not chunk or not self.on_gpu or any(g.x.is_cuda for g in chunk):
            return
        pipe, handle = self._begin_staging(self.n_batches & 1, chunk)
        self._prefetched = (chunk, pipe, handle)

    def _pose_inputs(self, chunk: Sequence[Data]):
        """What the device pose rule reads besides the forward's output, sent from pinned memory on the current stream:
        -> (node_first [G + 1], edge_first [G + 1] of the STORED edge lists, y [N, 6] fp32 = the chunk's collated targets)."""
        device, n_g = self.device, len(chunk)
        if any(g.y is None for g in chunk):
            raise ValueError("postprocess='device': every graph needs its targets y [n, 6]")
        ns = [int(g.x.shape[0]) for g in chunk]
        idx = torch.empty(2 * (n_g + 1), dtype=torch.int64, pin_memory=True)
        idx_np = idx.numpy()
        idx_np[0] = idx_np[n_g + 1] = 0
        np.cumsum(ns, out=idx_np[1:n_g + 1])
        np.cumsum([int(g.edge_index.shape[1]) for g in chunk], out=idx_np[n_g + 2:])
        if any(g.y.is_cuda for g in chunk):
            y_dev = torch.cat([g.y.to(device=device, dtype=torch.float32).reshape(-1, 6) for g in chunk])
        else:
            y = torch.empty((sum(ns), 6), dtype=torch.float32, pin_memory=True)
            off = 0
            for g, n in zip(chunk, ns):
                y[off:off + n].copy_(g.y.reshape(n, 6))
                off += n
            y_dev = y.to(device, non_blocking=True)
        idx_dev = idx.to(device, non_blocking=True)
        return idx_dev[:n_g + 1], idx_dev[n_g + 1:], y_dev

    def _collate(self, chunk, x_dev):
        device = self.device
        if x_dev is not None:
            return _collate_on_device(chunk, x_dev, device)
        if self.on_gpu and not all(g.x.is_cuda for g in chunk):
            # a chunk that mixes device- and host-resident graphs: the host ones go over one by one, the
            # collation then happens on the device (torch.cat would refuse mixed devices)
            return Batch.from_data_list([g.to(device, non_blocking=True) for g in chunk])
        return Batch.from_data_list(chunk).to(device, non_blocking=True)

    def _forward(self, chunk, batch):
        pose_in = self._pose_inputs(chunk) if self.pose is not None else None
        mc = getattr(self.model, "mc_dropout", None)
        if mc is not None:
            # global node ids and ONE draw for the whole stream: a graph's dropout masks do not depend on how the stream was cut
            if self.mc_draw is None:
                self.mc_draw = mc.draw
            mc.place(self.mc_draw, self.nodes_seen)
        self.nodes_seen += int(batch.x.shape[0])
        return (pose_in,) + tuple(self.model(batch))

    def end_draw(self) -> None:
        """The stream is over: model.mc_dropout's next forward draws the next masks (one draw per stream, not per micro-batch)."""
        mc = getattr(self.model, "mc_dropout", None)
        if mc is not None and self.mc_draw is not None:
            mc.reset(self.mc_draw + 1)
        self.mc_draw, self.nodes_seen = None, 0

    def _outputs(self, chunk, batch, fwd):
        pose_in, ab, rel, edge_index = fwd
        # a model-built edge list (kNN graph: the reference's default --knn 4, test.py:308, posenet.py:1047-1048) comes
        # back instead of the stored one: it travels to the host with the poses and is cut per graph by the consumer
        model_built = edge_index is not batch.edge_index
        if self.pose is not None:
            # everything the rule writes travels back in one tensor, one copy (QueryPose.output_block)
            out, ints, back, spread = self.pose.output_block(len(chunk), rel.device)
            # a rule with a spread reads the variances the forward has just left, row for row with rel (mc_dropout.McSpread)
            var = None if spread is None else self.model.mc_dropout.last.rel_var
            # a stored list is cut contiguously per graph; a model-built one is cut by its targets (edges_per_graph) in the kernel
            self.pose.from_targets(rel, edge_index, pose_in[0], pose_in[2], edge_first=None if model_built else pose_in[1],
                                   out=out, inliers=ints, rel_var=var, spread=spread)
            rel, model_built = back, False
        return {"rel": rel, "abs": ab if self.want_abs else None, "ei": edge_index if model_built else None,
                "var": self.model.mc_dropout.last.rel_var if self.want_var else None}

    def read_back(self, t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        """Device tensor -> pinned host tensor by a non-blocking copy on the current stream, its bytes counted; the event
        ``launch`` records behind the micro-batch's copies marks the arrival.  A tensor that is not on the device (the CPU path,
        one a client has read back itself) and None are handed on as they are."""
        if t is None or not t.is_cuda:
            return t
        host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        host.copy_(t, non_blocking=True)
        self.d2h_bytes += host.numel() * host.element_size()
        return host

    def launch(self, chunk: Sequence[Data]) -> _Launched:
        """Stage (or pick up the prefetched) chunk, run the forward, start the read-back.  With ``pose`` host["rel"] is the
        device pose rule's output block (``QueryPose.output_block``; ``cut_block`` cuts it) and host["ei"] is None."""
        k = self.n_batches & 1
        self.n_batches += 1
        staged = self.on_gpu and not any(g.x.is_cuda for g in chunk)
        pre, self._prefetched = self._prefetched, None
        if pre is not None and (not staged or len(pre[0]) != len(chunk) or any(a is not b for a, b in zip(pre[0], chunk))):
            pre[1].stage_end(pre[2])                                # a prefetch for another chunk: complete it (keeps the buffers' events in order), then drop it
            pre = None
        x_dev = None
        if staged:
            pipe, handle = (pre[1], pre[2]) if pre is not None else self._begin_staging(k, chunk)
            x_dev = pipe.stage_end(handle)
            self.h2d_bytes += x_dev.numel() * x_dev.element_size()
            fshape = _frame_shape(chunk)
            if fshape is not None:
                x_dev = x_dev.view(-1, *fshape)
        batch = self.collate(chunk, x_dev)
        if staged:
            pipe.acquire(k)
        fwd = self.forward(chunk, batch)
        if staged:
            pipe.release(k)
        # enqueued on the forward's stream, behind it and ahead of whatever the next launch() enqueues there: a client whose
        # forward replays a captured graph (relocalize(capture=True)) hands over that graph's static outputs, which the next
        # replay overwrites -- only after these copies have read them, by stream order
        host = {name: self.read_back(t) for name, t in self.outputs(chunk, batch, fwd).items()}
        ev = None
        if self.on_gpu:
            ev = torch.cuda.Event()
            ev.record()
        return _Launched(chunk, batch, host, ev)

    def arrived(self, item: _Launched) -> None:
        """Wait for a micro-batch's results and look at the deferred checks they came with: its bad-edge counters and the pose
        rule's count of graphs without a reference edge were copied before ``ev`` -- look, do not wait for the NEXT batch."""
        if item.ev is not None:
            item.ev.synchronize()
        check = getattr(self.model, "check_edge_index", None)
        if check is not None:
            check(wait=False)
        if self.pose is not None:
            self.pose.check(wait=False)

    def run(self, n: int, chunk_at, finish, stats: Optional[dict] = None, postprocess: str = "host") -> None:
        """The whole stream: ``drive`` micro-batches ``chunk_at(0 .. n - 1)`` with ``finish(item)`` called on every arrived
        one, wait for the last deferred reports and fill ``stats``."""
        t0 = time.perf_counter()

        def done(item):
            self.arrived(item)
            finish(item)
        drive(n, chunk_at, self.launch, self.prefetch, done)
        self.end_draw()
        check = getattr(self.model, "check_edge_index", None)
        if check is not None:
            check()                                    # everything has been issued: wait for the last report
        if self.pose is not None:
            self.pose.check()
        if stats is not None:
            ps = list(self.pipes.values())
            # staged / direct: bytes that went pageable -> pinned through the staging threads / straight out of the caller's own pinned tensors
            stats.update(local_seconds=time.perf_counter() - t0, h2d_bytes=self.h2d_bytes, postprocess=postprocess,
                         d2h_bytes=self.d2h_bytes, micro_batches=self.n_batches, staged_bytes=sum(p.staged_bytes for p in ps),
                         direct_bytes=sum(p.direct_bytes for p in ps), staging_workers=max((p.workers for p in ps), default=0))


def drive(n: int, chunk_at, launch, prefetch, finish) -> None:
    """The three-stage software pipeline over ``n`` micro-batches: while the GPU runs the forward of micro-batch i
    (``launch``), the staging threads already copy / round micro-batch i + 1 into its pinned buffer (``prefetch``: they release
    the GIL) and the calling thread post-processes micro-batch i - 1 (``finish``); the H2D copy of i + 1 is then enqueued first
    thing by its ``launch``, under the forward of i.  Round 6: before, staging, launch and post-processing took turns on the main
    thread and the bf16 stream at 256 x 341 was bound by that loop (9.5 ms per micro-batch against 7.8 ms of GPU work)."""
    pending = None
    nxt = chunk_at(0) if n > 0 else None
    for i in range(n):
        item = launch(nxt)
        nxt = chunk_at(i + 1) if i + 1 < n else None
        if nxt is not None:
            prefetch(nxt)
        if pending is not None:
            finish(pending)
        pending = item
    if pending is not None:
        finish(pending)


def edges_per_graph(ei: np.ndarray, sizes: Sequence[int]):
    """Cut a model-built edge list [2, E] of a collated micro-batch at graph boundaries: -> (first node of every graph,
    [column indices of graph k]); the batch order of the columns is kept (test.py:227 takes the FIRST edge into the node)."""
    first = np.concatenate([[0], np.cumsum(np.asarray(sizes))])
    gid = np.searchsorted(first, ei[1], side="right") - 1              # graph of every edge (by its target node)
    return first, [np.flatnonzero(gid == k) for k in range(len(sizes))]


def cut_per_graph(sizes: Sequence[int], built_ei: Optional[np.ndarray], stored):
    """One micro-batch cut into its graphs: yields (columns of the relative poses, the graph's edge list with local node ids)
    per graph.  A model-built list ``built_ei`` [2, E] is cut by its targets (``edges_per_graph``); otherwise the columns follow
    ``stored``, one edge list per graph (the graphs' own, or the fixed FC list of the map path again and again), contiguously,
    and each list is handed back as it came."""
    if built_ei is not None:
        first, per_graph = edges_per_graph(built_ei, sizes)
        for k, cols in enumerate(per_graph):
            yield cols, built_ei[:, cols] - first[k]
        return
    e0 = 0
    for edges in stored:
        e = int(edges.shape[1])
        yield slice(e0, e0 + e), edges
        e0 += e
