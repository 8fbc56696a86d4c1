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

``GraphedForwardMap`` is the same for the map path (``PoseNetX_R2.forward_map``, optionally followed by the device pose rule
``QueryPose.from_map``).  That step is the opposite case: one encoder image per graph, ~137 launches of 5-50 us per 64 queries,
bound by launch issue from Python -- the case a replay is for -- and, captured for one query, the serving entry point of a
camera that sends one frame at a time.

    step = GraphedForwardMap(model, fmap, example_queries, k=7, pose=QueryPose(...), pose_kwargs={"query_targets": t0})
    out = step(queries, neighbours, query_targets=t)     # out.rows: float64 [G, 16]; out.abs_pose, out.rel_pose, ...
"""
from __future__ import annotations

import contextlib
import gc
from collections import namedtuple
from typing import Optional

import numpy as np
import torch


@contextlib.contextmanager
def _capturing(graph, stream):
    """``torch.cuda.graph(graph, stream=stream)`` with Python's cycle collector held off.  A dead reference cycle may hold
    captured graphs -- a model and the steps in its ``_map_captures``, which hold the model, are one -- and the collector runs
    whenever enough objects have been allocated: in the middle of a capture, too.  On ROCm the destructor of a
    ``torch.cuda.CUDAGraph`` synchronises the device, which is not permitted while a stream is capturing and, raised from a
    destructor, ends the process.  So such cycles are collected here, ahead of the capture (``torch.cuda.graph`` no longer does
    that itself), and the collector stays off until the capture has ended."""
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph, stream=stream):
            yield
    finally:
        if was_enabled:
            gc.enable()


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
            with _capturing(self.graph, side):
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


# what a GraphedForwardMap call returns: forward_map's outputs, the neighbours the graphs were built from (the static input, or
# the rows the retrieval chose) and the pose rule's rows float64 [G, 16] (None without a pose rule) -- all static
MapStep = namedtuple("MapStep", "abs_pose rel_pose edge_index neighbours rows")

_FC_ONLY = "graph capture covers the deterministic fully-connected path (droprate=0, knn<=0)"


def _storage(t: Optional[torch.Tensor]):
    return None if t is None else (t.data_ptr(), int(t.shape[0]))


class GraphedForwardMap:
    """``model.forward_map(...)`` -- and ``pose.from_map(...)`` behind it when a ``QueryPose`` is given -- for ONE shape, captured
    once and replayed with one launch.

    ``example_queries`` [G, ...] fp32 (bf16 for the bf16 encoder) on the map's GPU give the shape; ``k`` is the number of
    database images per query (with a ``rule``, ``rule.k``; it may be None then).  Without a rule the neighbours are an input,
    int64 [G, K].  With a rule (``retrieval.RetrievalRule``) they are retrieved inside the graph from the static ``ranks`` int32
    [G, K] and query groups int64 [G]: everything the host draws per call (the rule's half-drop mask and start) stays on the host
    and is only copied in, so a seeded random rule gives other neighbours on every replay, as it does eagerly.  The forward's
    own explicit-``k`` kNN graph is not offered at all (there is no argument for it).
    ``query_descriptors`` fp32 [G, Dd]: an example, for a map that holds its own retrieval descriptors.
    ``pose_kwargs``: ``query_targets`` (an example fp32 [G, 6]; absent: the rows' target part is zeros) and ``edge_first`` (int64
    [G + 1]; absent: the cut of forward_map's own fully-connected list, K (K + 1) columns per graph -- K per graph with
    ``outputs="query"``).
    The rule's outputs are static too (``QueryPose.output_block``): the rows, ``self.inliers`` -- int32 [G, 2] = (inliers, used) per
    query for the one rule that has them, valid after a replay like the rows (``MapStep`` keeps its five fields), None for every
    other --, ``self.sigma`` -- float64 [G, 2] = (sigma_t, sigma_q) per query for a weighted rule, None for every other -- and
    ``self.packed``, the one tensor a stream copies back (the rows themselves, or the buffer that rows, spread and integers
    share).  A weighted rule reads the variances of the step's own forward (``self.spread.rel_var``, static), so it needs
    ``model.mc_dropout``.  The thresholds, the weighting and its floor are the ``QueryPose``'s: a step is captured with one rule
    and never replayed for another.
    ``outputs``: ``forward_map``'s -- ``"query"`` captures the query-only step, whose outputs are abs_pose [G, 6], rel_pose
    [G K, 6] and the G K edges into the query nodes; what that mode does not serve raises as it does there.

    ``gate`` (retrieval.PoseGate; with a rule without random draws and a map with poses): the retrieval inside the graph is
    restricted to the map rows near a prior pose (``forward_map(prior=, gate=)``).  ``self.prior`` -- float64 [G, 7], static -- is
    filled with NaN at the capture, so the warm-up and the capture rank the whole map, valid for any map; ``prior=`` of a call is
    copied into it, and a call WITHOUT ``prior`` leaves it as it is: whatever wrote it on the device since -- the update launch of
    ``tracking.Tracker``, captured with this step -- gates the next replay.  ``self.gate_info`` int32 [G, 2] = (state, rows
    inside), static, valid after a replay like the outputs.

    ``scenes`` [G] (with a rule on a ``featmap.SceneAtlas``, where it is required): each query's scene at the capture.
    ``self.scenes`` -- int32 [G], static -- is what the retrieval inside the graph scopes every query by (``forward_map(scenes=)``):
    ``scenes=`` of a call is copied into it and a call without leaves it as it is, so replays follow its current contents with no
    new capture (a tracking loop writes a camera's scene there when it moves to another room).  uint8 frames stay outside the
    graph, so a per-scene frame transform runs ahead of the call.
    A ``retrieval.SceneVote`` in its place: the election is part of the graph (``forward_map(scenes=SceneVote)``).  ``self.scenes``
    is then what the election writes and ``self.scene_info`` -- int32 [G, 2] = (elected scene, its votes), static -- is valid after
    a replay like the outputs.  ``lost_only=False``: every replay elects every query (``scenes=`` of a call is refused).
    ``lost_only=True`` (a gate is required): ``self.scenes`` starts at -1 = "elect"; a query elects when its entry is -1 or its
    static prior is not finite, and otherwise stays in the scene an earlier replay elected; ``scenes=`` of a call still copies
    explicit indices in, -1 among them.

    A model with ``droprate > 0`` is captured only with ``model.mc_dropout`` set (mc_dropout.McDropout): the step then returns the
    means over its dropout samples, the one-thread kernel that advances the draw counter is part of the graph, so every replay
    draws the next masks, and ``node_base`` is read from the device state a caller sets ahead of the replay.  ``self.spread``
    holds the variances (static, like the outputs).

    A model with ``knn > 0`` is captured only with ``model.static_knn`` set (``PoseNetX_R2.forward_map``): the kNN graph is then
    built at fixed positions inside the graph, from every replay's own features, k' = min(knn, K) edges into every node -- the
    default ``edge_first`` is the cut of that list, K + 1 times k' columns per graph (k' with ``outputs="query"``).  ``self.irregular``
    (int32 [1], static, valid after a replay like the outputs; None for every other model) is the number of nodes of the replayed
    step whose reference list is irregular: the step counts them there and not in the model's counters, so nothing raises, a
    caller that needs the reference's graph looks at it, and the step stays usable.

    The graph reads the packed weights, the workspaces, the map's tensors and the counters in place.  All of them are held
    here, so nothing it reads is freed under it, and every call compares them with what the model and the map hold NOW:
    after ``refresh_packed()`` / ``load_state_dict`` / ``.to()`` / a dtype switch / ``FeatureMap.extend`` the call raises
    ``RuntimeError`` instead of replaying over storage that is no longer the model's or the map's."""

    def __init__(self, model, fmap, example_queries: torch.Tensor, k: Optional[int] = None, *, rule=None, query_descriptors=None,
                 pose=None, pose_kwargs: Optional[dict] = None, warmup: int = 2, outputs: str = "all", gate=None, _after=None,
                 scenes=None):
        self.refuse(model, example_queries)
        model._check_outputs(outputs, None)
        q = example_queries
        if not q.is_cuda or q.device != fmap.device:
            raise RuntimeError("GraphedForwardMap needs the queries and the feature map on the same GPU")
        g = int(q.shape[0])
        if rule is not None:
            if k is not None and int(k) != rule.k:
                raise ValueError(f"GraphedForwardMap: k = {k}, but the rule picks {rule.k} rows")
            k = rule.k
        if k is None or int(k) < 1 or g < 1:
            raise ValueError("GraphedForwardMap: needs G >= 1 queries and K >= 1 database images per query")
        k = int(k)
        if rule is not None and k > len(fmap):
            raise ValueError(f"GraphedForwardMap: the rule picks {k} rows, the map has {len(fmap)}")
        if rule is None and query_descriptors is not None:
            raise ValueError("GraphedForwardMap: query_descriptors belong to retrieval: pass a rule")
        if rule is not None and (fmap.descriptors is None) != (query_descriptors is None):
            raise ValueError("GraphedForwardMap: query_descriptors must be given exactly when the map holds its own descriptors")
        if gate is not None:
            if rule is None:
                raise ValueError("GraphedForwardMap: a pose gate restricts retrieval: pass a rule")
            fmap.check_gate("GraphedForwardMap", rule, True, gate)          # (the prior is the step's own static buffer)
        pose_kwargs = dict(pose_kwargs or {})
        if pose is None and pose_kwargs:
            raise ValueError("GraphedForwardMap: pose_kwargs without a pose rule")
        if pose is not None and fmap.poses is None:
            raise ValueError("GraphedForwardMap: the pose rule needs a feature map with poses")
        unknown = set(pose_kwargs) - {"query_targets", "edge_first"}
        if unknown:
            raise ValueError(f"GraphedForwardMap: pose_kwargs takes query_targets and edge_first, got {sorted(unknown)}")
        dev = q.device
        self.model, self.fmap, self.rule, self.pose = model, fmap, rule, pose
        self.g, self.k, self.outputs = g, k, outputs
        # _after (tracking.Tracker): called with this object and every step's MapStep behind its launches -- in the warm-up and in the capture, so
        # what it launches is part of the graph
        self.gate, self._after = gate, _after
        self.scenes = self.vote = self.scene_info = None
        if rule is not None:
            # None for one scene's map (which takes no scenes); the warm-up and the capture draw nothing (see the ranks below)
            scope = fmap._scope(scenes, g, rule, "GraphedForwardMap", ranks_given=True, lost_ok=gate is not None)
            if scope is not None and len(scope) == 3:         # a SceneVote: the election writes the static scenes
                self.vote = scope[2]
                self.scenes = torch.full((g,), -1, dtype=torch.int32, device=dev)
                self.scene_info = torch.zeros((g, 2), dtype=torch.int32, device=dev)
            elif scope is not None:
                self.scenes = scope[1].clone()
        elif scenes is not None:
            raise ValueError("GraphedForwardMap: scenes scope retrieval: pass a rule (frames are transformed outside the graph)")
        self.prior = self.gate_info = None
        if gate is not None:
            fmap.gate_rows(gate)                  # cached on the map: made here, outside the capture, and held below
            self.prior = torch.full((g, 7), float("nan"), dtype=torch.float64, device=dev)
            self.gate_info = torch.zeros((g, 2), dtype=torch.int32, device=dev)
        # model.static_knn: k' = min(knn, K) columns per node, rebuilt from every replay's features inside the graph; the nodes whose
        # reference list is irregular are counted into self.irregular (int32 [1], static, zeroed by the step itself: valid after a
        # replay like the outputs), not into the model's counters -- a caller looks at it, the step stays usable
        self.kp = model._static_columns(None, k) if getattr(model, "knn", -1) > 0 else 0
        self.irregular = torch.zeros(1, dtype=torch.int32, device=dev) if self.kp else None

        # ---- the static inputs --------------------------------------------------------------------------------------------------
        self.queries = q.detach().clone(memory_format=torch.contiguous_format)
        self.neighbours = self.ranks = self.query_groups = self.query_descriptors = self.query_targets = self.edge_first = None
        self.inliers = self.sigma = self.packed = self._rows_out = None
        if rule is None:
            self.neighbours = torch.zeros((g, k), dtype=torch.int64, device=dev)          # row 0: valid for any map
        else:
            # A rule without random draws picks the same positions for every query that no group restricts: they are made once,
            # here, and stay in the static buffer.  A random rule's draws are made per call, on the host, in query order; the
            # warm-up and the capture run on positions 0..K-1 (K <= M rows and no group set: valid) so that they do not advance
            # a seeded rule's generator.
            self._fixed_ranks = None if rule.random else torch.from_numpy(rule.ranks(fmap.n_allowed(None, g))).pin_memory()
            self._ranks_fixed = not rule.random
            self.ranks = (torch.arange(k, dtype=torch.int32).repeat(g, 1) if rule.random else self._fixed_ranks).to(dev)
            if fmap.groups is not None:
                self.query_groups = torch.full((g,), -1, dtype=torch.int64, device=dev)   # -1: nothing left out
            if query_descriptors is not None:
                qd = query_descriptors
                if not torch.is_tensor(qd) or qd.dtype != torch.float32 or tuple(qd.shape) != (g, fmap.descriptors.shape[1]):
                    raise ValueError(f"GraphedForwardMap: query_descriptors must be fp32 [{g}, {fmap.descriptors.shape[1]}]")
                self.query_descriptors = qd.detach().to(dev).contiguous().clone()
            fmap.inv_norms()                      # cached on the map: made here, outside the capture, and held below
        if pose is not None:
            self._rows_out, self.inliers, self.packed, self.sigma = pose.output_block(g, dev)
            if self.sigma is not None and getattr(model, "mc_dropout", None) is None:
                raise ValueError("GraphedForwardMap: a weighted pose rule reads the Monte-Carlo variances: set model.mc_dropout")
            qt = pose_kwargs.get("query_targets")
            if qt is not None:
                if not torch.is_tensor(qt) or qt.dtype != torch.float32 or tuple(qt.shape) != (g, 6):
                    raise ValueError(f"GraphedForwardMap: pose_kwargs['query_targets'] must be fp32 [{g}, 6]")
                self.query_targets = qt.detach().to(dev).contiguous().clone()
            if "edge_first" in pose_kwargs:
                ef = pose_kwargs["edge_first"]
                self.edge_first = None if ef is None else ef.detach().to(device=dev, dtype=torch.int64).contiguous().clone()
            else:
                per_node = self.kp or k           # incoming edges of every node: k' of the fixed-position kNN list, K of the FC one
                self.edge_first = torch.arange(g + 1, dtype=torch.int64, device=dev) * (per_node if outputs == "query" else per_node * (k + 1))

        # ---- warm-up, validation, capture (the pattern of GraphedForward) ---------------------------------------------------------
        self.graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        mc = getattr(model, "mc_dropout", None)
        with torch.cuda.stream(side):
            # model.mc_dropout: every warm-up forward advances the draw counter on the device; it is put back behind them, so that
            # capturing a step draws nothing and the first replay has the masks the next eager forward would have had
            mc_saved = None if mc is None else mc.state(dev).clone()
            mc_draw = None if mc is None else mc.draw
            for _ in range(max(1, warmup)):       # packs weights, sizes the workspace pool, builds the _map_graph edge list
                self._step()
                if self.prior is not None:        # (an _after that accepted the warm-up's pose: the capture starts without a prior)
                    self.prior.fill_(float("nan"))
                if self.vote is not None:         # (... and without the scenes the warm-up elected)
                    self.scenes.fill_(-1)
            if mc_saved is not None:
                mc.state(dev).copy_(mc_saved)
            model.check_edge_index()              # one sync, before the capture: the warm-up's inputs were valid
            if pose is not None:
                pose.check()
            with _capturing(self.graph, side):
                self.out = self._step()
            if mc is not None:
                mc._init[0] = mc._word(mc_draw)   # the host's count of the draws, which the warm-up forwards moved on as well
        # the variances of a replay (mc_dropout.McSpread): static like the outputs, handed to model.mc_dropout.last by every call
        self.spread = None if mc is None else mc.last
        torch.cuda.current_stream().wait_stream(side)
        # everything the graph reads besides its static inputs, held so that it outlives the graph, and what a call compares
        self._held = self._reads()
        self._signature = self._sign(self._held)

    @staticmethod
    def refuse(model, queries) -> None:
        """Raise for what a captured map step does not cover -- before anything is queued."""
        if not torch.is_tensor(queries):
            raise TypeError("GraphedForwardMap: queries must be a tensor [G, ...]")
        if queries.dtype == torch.uint8:
            raise TypeError("GraphedForwardMap does not take uint8 frames: capture the model on its fp32 / bf16 input "
                            "(frame_transform.apply(frames) outside the graph)")
        # the always-on dropout is captured only as model.mc_dropout samples it: its masks are made on the device from a counter
        # the captured step itself advances (rpg_mc_advance), where torch's generator would replay one mask for ever
        # a model-built kNN graph is captured only at fixed positions (model.static_knn: rpg_knn_graph_uniform_f32 writes no edge
        # count for the host), where the general build waits for one
        if ((getattr(model, "droprate", 0) > 0 and getattr(model, "mc_dropout", None) is None)
                or (getattr(model, "knn", -1) > 0 and not getattr(model, "static_knn", False))):
            raise NotImplementedError(_FC_ONLY)
        if getattr(model, "use_attention", False) or not getattr(model, "use_AP", True):
            raise NotImplementedError(_FC_ONLY + "; use_attention and use_AP=False take the one-stream path, which allocates and "
                                      "publishes between its launches")

    def _step(self) -> MapStep:
        m = self.model
        kw = {}
        if self.irregular is not None:
            self.irregular.zero_()
            kw["_irregular"] = self.irregular
        if self.rule is None:
            ab, rel, ei = m.forward_map(self.queries, self.neighbours, self.fmap, outputs=self.outputs, **kw)
            nb = self.neighbours
        else:
            if self.gate is not None:
                kw.update(gate=self.gate, _static=(self.ranks, self.query_groups, self.prior, self.gate_info))
            else:
                kw["_static"] = (self.ranks, self.query_groups)
            if self.vote is not None:
                kw.update(scenes=self.vote, _vote=(self.scenes, self.scene_info))
            elif self.scenes is not None:
                kw["scenes"] = self.scenes
            ab, rel, ei, nb = m.forward_map(self.queries, None, self.fmap, rule=self.rule, query_descriptors=self.query_descriptors,
                                            outputs=self.outputs, **kw)
        if self.gate is not None:
            m.gate_info = self.gate_info
        if self.vote is not None:
            m.scene_info = self.scene_info
        rows = None
        if self.pose is not None:
            # (a weighted rule: the variances this forward has just left -- in the capture, the step's static spread.rel_var)
            var = None if self.sigma is None else m.mc_dropout.last.rel_var
            rows = self.pose.from_map(rel, ei, self.fmap, nb, query_targets=self.query_targets, edge_first=self.edge_first,
                                      out=self._rows_out, inliers=self.inliers, rel_var=var, spread=self.sigma)
        out = MapStep(ab, rel, ei, nb, rows)
        if self._after is not None:
            self._after(self, out)
        return out

    # ---- validity ------------------------------------------------------------------------------------------------------------------
    def _reads(self) -> dict:
        from . import _lib as L
        m, f = self.model, self.fmap
        return {"library": L.lib(), "encoder": m._enc._packed, "gnn": m._gnn_packed, "gnn_bf16": m._gnn_bf16,
                "dtypes": (m.encoder_dtype, m.gnn_dtype, bool(getattr(m, "static_knn", False))), "workspaces": list(m._ws_pool._buf.values()),
                "fc_graph": m._map_graphs.get((self.g, self.k + 1, str(self.queries.device))),
                "query_sel": (m._map_queries.get((self.g, self.k + 1, str(self.queries.device)))
                              if self.outputs == "query" else None),
                "knn_sel": (m._map_queries.get(("knn", self.g, self.k + 1, self.kp, str(self.queries.device)))
                            if self.outputs == "query" and self.kp else None),
                "mc_state": None if getattr(m, "mc_dropout", None) is None else m.mc_dropout._state,
                "counters": m._counters.counters, "pose_counters": None if self.pose is None else self.pose._bad.counters,
                "features": f.features, "poses": f.poses, "descriptors": f.descriptors, "groups": f.groups,
                "inv_norms": f._inv_norms if self.rule is not None else None,
                "scene_first": getattr(f, "scene_first", None) if self.scenes is not None else None,
                "gate_rows": None if self.gate is None else f._gate_rows.get((tuple(self.gate.pose_m), tuple(self.gate.pose_s)))}

    @staticmethod
    def _sign(r: dict) -> tuple:
        """Objects by identity, the map's storage by (address, rows): what must be unchanged for the graph to be replayed."""
        return (id(r["library"]), id(r["encoder"]), id(r["gnn"]), id(r["gnn_bf16"]), r["dtypes"], id(r["counters"]),
                id(r["pose_counters"]), _storage(r["features"]), _storage(r["poses"]), _storage(r["descriptors"]),
                _storage(r["groups"]), _storage(r["inv_norms"]), id(r["mc_state"]), _storage(r["scene_first"]),
                _storage(r["gate_rows"]))

    def stale(self) -> bool:
        """True once the model or the map no longer hold what the graph was captured over."""
        now = self._reads()
        if now["encoder"] is None or now["gnn"] is None:
            return True
        if self.rule is not None and now["inv_norms"] is None:
            return True
        if self.gate is not None and now["gate_rows"] is None:
            return True
        return self._sign(now) != self._signature

    # ---- replay ------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _copy_in(static: torch.Tensor, given: torch.Tensor) -> None:
        if given.data_ptr() != static.data_ptr():             # the static buffer itself: nothing to copy
            static.copy_(given, non_blocking=True)

    @torch.no_grad()
    def __call__(self, queries: torch.Tensor, neighbours: Optional[torch.Tensor] = None, ranks=None, query_descriptors=None,
                 query_groups=None, query_targets=None, prior=None, scenes=None) -> MapStep:
        """Copy the given inputs into the static buffers (non-blocking, on the current stream; a tensor that IS the static buffer
        -- ``self.queries`` filled by the caller -- is not copied), replay, publish the deferred counters.  ``ranks``: int32 [G, K]
        (tensor or array) in place of the rule's own, which are otherwise drawn here, on the host, as ``forward_map`` draws them;
        ``query_groups`` [G]: host integers, as ``forward_map`` takes them.  ``prior`` [G, 7] (a gated step only): copied into the
        static prior; None leaves that buffer as it is.  ``scenes`` [G] (a step captured on a SceneAtlas only; host integers or an
        int32 device tensor): copied into the static scenes; None leaves them as they are.  A rule with random draws, and
        ``query_groups``, size the ranks by each query's allowed rows inside its scene: such a call needs ``scenes`` as host
        integers every time (or the caller's own ``ranks``), ValueError otherwise.  A step captured with a ``SceneVote``: with
        ``lost_only`` the indices may hold -1 (elect); without, every replay elects and ``scenes`` is refused."""
        if self.stale():
            raise RuntimeError("GraphedForwardMap is stale: the model's packed weights / precision or the feature map's storage "
                               "have changed since the capture (refresh_packed, load_state_dict, .to(), FeatureMap.extend): "
                               "capture again")
        # every check before the first copy: a refused call leaves the static inputs as they were
        for static, given, name in ((self.queries, queries, "queries"), (self.neighbours, neighbours, "neighbours"),
                                    (self.query_descriptors, query_descriptors, "query_descriptors"),
                                    (self.query_targets, query_targets, "query_targets")):
            if static is None and given is not None:
                raise ValueError(f"GraphedForwardMap: {name} given, but the graph was captured without")
            if static is not None and given is None:
                raise ValueError(f"GraphedForwardMap: the graph was captured with {name}: give them")
            if static is not None and not torch.is_tensor(given):
                raise TypeError(f"GraphedForwardMap: {name} must be a tensor")
            if static is not None and (given.shape != static.shape or given.dtype != static.dtype):
                raise ValueError(f"GraphedForwardMap was captured for {name} {static.dtype} {tuple(static.shape)}, got "
                                 f"{given.dtype} {tuple(given.shape)}")
        if self.rule is None and (ranks is not None or query_groups is not None):
            raise ValueError("GraphedForwardMap: ranks / query_groups belong to retrieval: the graph was captured without a rule")
        prior_dev = None
        if prior is not None:
            if self.gate is None:
                raise ValueError("GraphedForwardMap: prior given, but the graph was captured without a gate")
            prior_dev = self.fmap.prior_tensor(prior, self.g, "GraphedForwardMap")
        sc_host = sc_dev = None
        if scenes is not None:
            if self.scenes is None:
                raise ValueError("GraphedForwardMap: scenes given, but the graph was captured without (no rule on a SceneAtlas)")
            if self.vote is None:
                sc_host, sc_dev = self.fmap._scope(scenes, self.g, self.rule, "GraphedForwardMap", ranks_given=ranks is not None)
            elif not self.vote.lost_only:
                raise ValueError("GraphedForwardMap: the step was captured with a SceneVote that every query elects by: scenes "
                                 "of a call would be overwritten (capture with lost_only=True to hold given scenes)")
            else:
                from .frames import scenes_to_device
                sc_host, sc_dev = scenes_to_device(scenes, self.g, self.fmap.device, "GraphedForwardMap")
                if sc_host is not None and sc_host.size and (sc_host.min() < -1 or sc_host.max() >= self.fmap.n_scenes):
                    raise IndexError(f"GraphedForwardMap: scenes has entries outside [-1, {self.fmap.n_scenes}) (-1: elect)")
        self.model._counters.poll()               # as the eager call starts: the report of the previous call, if it has landed
        host_ranks, qg_dev, fixed = None, None, False
        if self.rule is not None:
            qg_host, qg_dev = self.fmap._query_groups(query_groups, self.g)
            if ranks is None:
                if self.rule.random or (qg_host is not None and self.vote is None):    # (a vote: the smallest scene, fixed)
                    if self.scenes is not None and sc_host is None:
                        # the draws are sized by each query's allowed rows inside ITS scene, and the static scenes are on the
                        # device (where a tracker may have rewritten them): the host cannot size them
                        raise ValueError("GraphedForwardMap: a rule with random draws, or query_groups, on a SceneAtlas needs this "
                                         "call's scenes as host integers (scenes=), or ranks= of the caller's own")
                    ranks = self.rule.ranks(self.fmap.n_allowed(qg_host, self.g, *(() if self.scenes is None else (sc_host,))))
                elif not self._ranks_fixed:       # an earlier call left its own ranks in the static buffer
                    ranks = self._fixed_ranks
            fixed = ranks is self._fixed_ranks and ranks is not None
            if ranks is not None:
                host_ranks = ranks if torch.is_tensor(ranks) else torch.from_numpy(np.ascontiguousarray(ranks, dtype=np.int32))
                if host_ranks.dtype != torch.int32 or tuple(host_ranks.shape) != (self.g, self.k):
                    raise ValueError(f"GraphedForwardMap: ranks must be int32 [{self.g}, {self.k}], got {host_ranks.dtype} "
                                     f"{tuple(host_ranks.shape)}")
                if not host_ranks.is_cuda and not host_ranks.is_pinned():
                    host_ranks = host_ranks.pin_memory()
        for static, given in ((self.queries, queries), (self.neighbours, neighbours),
                              (self.query_descriptors, query_descriptors), (self.query_targets, query_targets)):
            if static is not None:
                self._copy_in(static, given)
        if prior_dev is not None:
            self._copy_in(self.prior, prior_dev)
        if sc_dev is not None:
            self._copy_in(self.scenes, sc_dev)
        if host_ranks is not None:
            self.ranks.copy_(host_ranks, non_blocking=True)
            self._ranks_fixed = fixed
        if self.query_groups is not None:
            if qg_dev is None:
                self.query_groups.fill_(-1)
            else:
                self.query_groups.copy_(qg_dev, non_blocking=True)
        self.graph.replay()
        if self.gate is not None:
            self.model.gate_info = self.gate_info
        self.model.scene_info = self.scene_info
        if self.spread is not None:               # the replayed step advanced the draw counter on the device
            self.model.mc_dropout.last = self.spread
            self.model.mc_dropout.advanced()
        self.model.publish_status()               # bad neighbours / ranks / edges counted by the replayed kernels
        if self.pose is not None:
            self.pose.publish()                   # ... and graphs without a usable reference edge
        return self.out
