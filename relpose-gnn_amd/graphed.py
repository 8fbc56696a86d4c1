"""Replay of the whole forward from a captured HIP graph (``torch.cuda.CUDAGraph``; a hipGraph underneath).

The forward is ~130 kernel launches per stream issued from Python through ctypes.  All kernels of the path are
capturable after a warm-up call (no allocation, no synchronisation, fixed workspaces; the two worker streams of
``PoseNetX_R2`` join the capture through events), so a fixed-shape batch can be replayed with one ``hipGraphLaunch``.
Measured on an otherwise idle MI355X host the replay is within 2 % of eager (1.72 vs 1.73 ms for one 8-node graph,
3.20 vs 3.27 ms for 4, 12.98 vs 13.0 ms for 32): the GPU is the bottleneck, the launches are already hidden.  The
graph is for hosts whose CPU is busy (8 ranks, data loading) and as the fixed-shape serving entry point.

    runner = GraphedForward(model, example_batch)        # captures once for this batch shape / edge structure
    abs_pose, rel_pose, edge_index = runner(batch)       # copies batch.x into the static input, replays, returns views

The returned tensors are the graph's static outputs: they are overwritten by the next call (clone them to keep them).
"""
from __future__ import annotations

import torch


class GraphedForward:
    def __init__(self, model, example, warmup: int = 2):
        if not example.x.is_cuda:
            raise RuntimeError("GraphedForward needs a batch on the GPU")
        if example.x.dtype == torch.uint8:
            raise TypeError("GraphedForward does not take uint8 frames: capture the model on its fp32 / bf16 input "
                            "(frame_transform.apply(frames) outside the graph)")
        if getattr(model, "droprate", 0) > 0 or getattr(model, "knn", -1) > 0:
            raise NotImplementedError("graph capture covers the deterministic fully-connected path (droprate=0, knn<=0)")
        self.model = model
        self.static = example                     # its tensors are the graph's input buffers
        self.graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(device=example.x.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(max(1, warmup)):       # packs weights, sizes workspaces
                model(self.static)
            if hasattr(model, "check_edge_index"):
                model.check_edge_index()          # validates the example's edge_index (one sync, before the capture)
            with torch.cuda.graph(self.graph, stream=side):
                self.out = model(self.static)
        torch.cuda.current_stream().wait_stream(side)

    @torch.no_grad()
    def __call__(self, data):
        if data is not self.static:
            if data.x.shape != self.static.x.shape or data.edge_index.shape != self.static.edge_index.shape:
                raise ValueError("GraphedForward was captured for a different batch shape")
            self.static.x.copy_(data.x, non_blocking=True)
            if data.edge_index.data_ptr() != self.static.edge_index.data_ptr():
                self.static.edge_index.copy_(data.edge_index, non_blocking=True)
        self.graph.replay()
        if hasattr(self.model, "publish_status"):
            self.model.publish_status()           # bad-edge counters of the replayed kernels -> model.check_edge_index()
        return self.out
