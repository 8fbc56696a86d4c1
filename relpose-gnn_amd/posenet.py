"""``PoseNetX_R2``: host-side mirror of the reference model's nn.Module contract over the HIP hot path.

Same constructor keywords, ``forward(data, k=None) -> (abs_pose[N,6], rel_pose[E,6], edge_index[2,E])`` signature,
``data.x / data.edge_index`` input contract and state-dict key names as
/root/reference/python/niantic/modules/posenet.py:920-1091, so it drops into the evaluation scripts
(testing/test.py:157-167,211) and loads their checkpoints.  The sub-modules below (``nn.Linear`` holders named like the
reference's ``simpleConvEdge_upt`` / ``simpleEdgeModel`` / ``AttentionBlock`` children, my_gnn_layer.py:280-291,
att.py:9-14) only own parameters; the arithmetic is two C calls, ``rpg_resnet_forward_f32`` and ``rpg_gnn_forward_f32``.

``use_gnn=True`` is required (the reference's ``use_gnn=False`` branch is unreachable: posenet.py:987-989 touches an
undefined attribute).  The fast path is ``use_AP=True, use_attention=False, knn<=0, k=None`` (two C calls); the other
constructor / forward flags of the reference -- ``use_attention`` (posenet.py:1040-1041), ``use_AP=False``
(:1080-1083), kNN graphs through ``knn>0`` or ``forward(data, k)`` (:1043-1050, ``rpg_knn_graph_f32``), ``L>1``
(extra ``gnn2..`` parameter sets that the reference creates but never uses, :950-953, :1061-1069) -- run through the
same kernels with a few more fine-grained calls.  The reference's always-on dropout (``F.dropout`` without ``training=``, posenet.py:1073-1075) is honoured: with
``droprate>0`` the node/edge features come back from the GNN call, ``F.dropout`` is applied, and the heads kernel runs on
the result; parity tests use ``droprate=0``.  ``model.mc_dropout = McDropout(samples, seed)`` (mc_dropout.py; default None) samples
that dropout instead of drawing it once: every forward then returns the MEAN of the heads over ``samples`` masks in place of
abs_pose / rel_pose (same shapes) and leaves the variances in ``mc_dropout.last``; the masks are made on the device from (seed,
draw, node ids, column, sample) by one kernel per head (``rpg_pose_heads_mc_f32``), so they do not depend on stream slots,
micro-batches or the ``outputs`` mode, and the captured map step takes such a model.  Everything runs on the GPU; CPU tensors
raise (no fallback).

Index validation.  The reference's aten indexing raises ``IndexError`` for a node id outside ``[0, N)``.  Here every call
is validated on the device (``rpg_graph_prepare`` counts the offending edges, clamps them and leaves them out of the
aggregation, so nothing reads out of bounds) and the count travels to pinned host memory with an asynchronous copy
behind the kernels (``status.DeferredCounters``, which ``QueryPose`` uses too).  ``index_check = "deferred"`` (default) never blocks inside ``forward``: the count of call i is looked
at when call i+1 starts (by then a reference-style caller has already synchronised through ``.cpu()``), in
``check_edge_index()`` and by ``evaluate_stream`` right after its own device-to-host event; ``index_check = "sync"``
reads it back before returning, like the reference, at the price of one device synchronisation per call.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as _L
from . import ops
from .params import pack_gnn, pack_gnn_bf16, pack_gnn_mean_first
from .resnet import EncoderRunner, WorkspacePool
from .mc_dropout import McSpread
from .status import DeferredCounters


class AttentionBlock(nn.Module):
    """Parameter holder with the reference's child names (att.py:9-14)."""

    def __init__(self, in_channels: int):
        super().__init__()
        self.g = nn.Linear(in_channels, in_channels // 8)
        self.theta = nn.Linear(in_channels, in_channels // 8)
        self.phi = nn.Linear(in_channels, in_channels // 8)
        self.W = nn.Linear(in_channels // 8, in_channels)


class simpleEdgeModel(nn.Module):  # noqa: N801 - reference spelling (my_gnn_layer.py:224)
    def __init__(self, in_channels: int, edge_channels: int, out_channels: int):
        super().__init__()
        self.edge_mlp = nn.Sequential(nn.Linear(2 * in_channels + edge_channels, out_channels), nn.ReLU(),
                                      nn.Linear(out_channels, out_channels))


class simpleConvEdge_upt(nn.Module):  # noqa: N801 - reference spelling (my_gnn_layer.py:277)
    def __init__(self, in_channels: int, edge_channels: int, out_channels: int):
        super().__init__()
        self.mlp = nn.Sequential(nn.Linear(in_channels + edge_channels, out_channels), nn.ReLU(),
                                 nn.Linear(out_channels, out_channels))
        self.mlp_updating = nn.Sequential(nn.Linear(2 * in_channels, out_channels), nn.ReLU(),
                                          nn.Linear(out_channels, out_channels))
        self.edge_model = simpleEdgeModel(in_channels, edge_channels, edge_channels)
        self.att = AttentionBlock(in_channels)


# forward_map with static_knn and the bf16 GNN is cut into stream slots only when every slot gets at least this many graphs.
# Measured (profiles/knn_map_bench.json, "schedule"; K = 7, D = 2048): at 32 graphs of 224 x 224 two slots of 16 run at 0.95x of
# one stream -- the fully-connected bf16 step shows the same 0.95x there, so it is the schedule, not the kNN build -- at 64 graphs
# two slots of 32 are 1.01x of one stream, at 256 graphs 1.05-1.10x of the general one-stream path.
_STATIC_BF16_SLOT_GRAPHS = 32


class IrregularKnnGraph(ValueError):
    """``static_knn``: a graph of the map step has a node whose reference kNN list keeps one edge more than the fixed layout holds
    (k + 1 or more lower-numbered nodes of its graph with a bit-identical feature row, or non-finite rows)."""


def _bad_index_error(counts: torch.Tensor) -> Exception:
    """``counts``: host int32 [24], the bad-edge counters (slots 0..7), forward_map's bad-neighbour counters (8..15) and the
    ``static_knn`` map step's irregular-node counters (16..23)."""
    edges, nbrs, irregular = int(counts[:8].sum()), int(counts[8:16].sum()), int(counts[16:].sum())
    if irregular and not edges and not nbrs:
        return IrregularKnnGraph(f"forward_map with static_knn: {irregular} node(s) whose reference kNN list has k + 1 edges (duplicate "
                                 "or non-finite feature rows), so the edge list returned for that call is not the reference's: set "
                                 "model.static_knn = False for such inputs (the waiting path reproduces the extra edges) "
                                 "(detected on the device; with index_check='deferred' this refers to an EARLIER forward_map call)")
    what = []
    if irregular:
        what.append(f"static_knn: {irregular} node(s) whose reference kNN list has k + 1 edges (set model.static_knn = False)")
    if edges:
        what.append(f"edge_index has {edges} edge(s) with a node id outside its graph group / [0, N)")
    if nbrs:
        what.append(f"neighbours has {nbrs} index(es) outside the feature map's rows [0, M)")
    return IndexError("; ".join(what) + " (detected on the device; with index_check='deferred' this refers to an EARLIER "
                      "forward call)")


class PoseNetX_R2(nn.Module):  # noqa: N801 - reference spelling
    def __init__(self, feature_extractor, droprate=0.5, pretrained=True,
                 feat_dim=1024, edge_feat_dim=1024, node_dim=1024,
                 filter_nans=False, input_img_height=256, use_gnn=False, use_attention=False,
                 knn=-1, use_AP=True, gnn_recursion=2, device: int = 0, L: int = 1):
        super().__init__()
        if not use_gnn:
            raise NotImplementedError("use_gnn=False is outside the accelerated path (and unreachable in the reference: "
                                      "posenet.py:987-989 touches an undefined self.mlp)")
        if not (feat_dim == node_dim == edge_feat_dim):
            # Not a restriction of this implementation: the reference constructs such a model (posenet.py:948-953) but its
            # forward cannot run it -- fc_xyz_R = Linear(node_dim, 3) is applied to edge_feat [E, edge_feat_dim] (:974-975,
            # :1085-1086) and gnn1 = simpleConvEdge_upt(node_dim, ...) to x [N, feat_dim] (proj_node is commented out, :946):
            # every unequal combination raises "mat1 and mat2 shapes cannot be multiplied" (checked by running the reference,
            # INTEGRATION.md).  Refused at construction here, where the reference fails at the first forward.
            raise ValueError("feat_dim, edge_feat_dim and node_dim must be equal: the reference's forward (posenet.py:1053-1086) "
                             f"raises a shape error for any other combination (got {feat_dim}, {edge_feat_dim}, {node_dim})")
        if feat_dim % 32:
            raise NotImplementedError("the HIP kernels need feat_dim to be a multiple of 32")
        self.droprate = droprate
        self.input_img_height = input_img_height
        self.use_gnn, self.n_layers, self.use_attention = use_gnn, L, use_attention
        self.knn, self.use_AP, self.gnn_recursion, self.device = knn, use_AP, gnn_recursion, device

        # replace the encoder's pooling and last FC exactly as the reference does (posenet.py:942-945)
        self.feature_extractor = feature_extractor
        self.feature_extractor.avgpool = nn.AdaptiveAvgPool2d(1)
        fe_out_planes = self.feature_extractor.fc.in_features
        self.feature_extractor.fc = nn.Linear(fe_out_planes, feat_dim)
        self.proj_edge = nn.Linear(feat_dim * 2, edge_feat_dim)
        for layer in range(L):                         # only gnn1 is ever used by forward (posenet.py:1061-1069)
            setattr(self, f"gnn{layer + 1}", simpleConvEdge_upt(node_dim, edge_feat_dim, node_dim))
        if self.use_attention:
            self.att = AttentionBlock(feat_dim)
        self.fc_xyz = nn.Linear(node_dim if use_AP else node_dim * 2, 3)
        self.fc_wpqr = nn.Linear(node_dim if use_AP else node_dim * 2, 3)
        self.fc_xyz_R = nn.Linear(node_dim, 3)
        self.fc_wpqr_R = nn.Linear(node_dim, 3)

        # initialisation rule of posenet.py:981-997
        if pretrained:
            init_modules = [self.feature_extractor.fc, self.proj_edge, self.fc_xyz, self.fc_wpqr, self.fc_xyz_R,
                            self.fc_wpqr_R, self.gnn1]
        else:
            init_modules = self.modules()
        for m in init_modules:
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                nn.init.kaiming_normal_(m.weight.data)
                if m.bias is not None:
                    nn.init.constant_(m.bias.data, 0)

        # Number of HIP streams a batch is spread over (graphs are independent: the batch is cut at graph boundaries
        # and the parts run concurrently, which fills the tile-quantisation tails of one part's kernels with the other
        # part's work).  Needs the host-side slice table of relpose_gnn_amd.graph.Batch; other inputs use one stream.
        self.hip_streams = 2
        # streams the IMAGES of a batch too small to be cut at graph boundaries are spread over (see _encode_small)
        self.small_batch_streams = 1
        # optional explicit schedule (experiments / tuning): [(first graph, last graph + 1, stream slot), ...] in issue order;
        # groups on the same slot run one after the other.  None = `hip_streams` equal contiguous groups, one per stream.
        self.stream_schedule: Optional[List[Tuple[int, int, int]]] = None
        self._streams: List[torch.cuda.Stream] = []
        self._ws_pool = WorkspacePool()            # one buffer per stream slot, shared by the encoder and the GNN call
        self._enc = EncoderRunner(self._ws_pool)
        self._gnn_packed: Optional[List[torch.Tensor]] = None
        self._gnn_ptrs = None
        self._gnn_bf16: Optional[List[torch.Tensor]] = None
        self._gnn_bf16_ptrs = None
        self._gnn_dtype = "f32"
        self._extra: Dict[str, torch.Tensor] = {}
        self.index_check = "deferred"            # "deferred" | "sync" (see the module docstring)
        # device int32 [24]: bad-edge counters, one per stream slot, then the map path's bad-neighbour counters, one per slot, then
        # the static_knn map step's irregular-node counters, one per slot
        self._counters = DeferredCounters(24, _bad_index_error)
        # optional frames.FrameTransform: with it forward() also takes uint8 frames data.x [n, H, W, 3] (RGB, HWC) on the GPU and
        # runs the reference's image transform there (a plain attribute: not a module, parameter or buffer -- state_dict unchanged)
        self.frame_transform = None
        # optional mc_dropout.McDropout: with it (and droprate > 0) every forward returns the MEAN of the heads over its dropout
        # samples in place of abs_pose / rel_pose and leaves their variances in mc_dropout.last (a plain attribute as well)
        self.mc_dropout = None
        # what the last forward_map's pose gate did, int32 [G, 2] = (state, rows inside) on the device; None without a gate
        self.gate_info = None
        self.scene_info = None
        # with knn > 0: forward_map builds the kNN graph of its equal-sized graphs at fixed positions (rpg_knn_graph_uniform_f32):
        # no edge count for the host to wait for, so the two-stream schedule, outputs="query" and the captured step serve the
        # model; a graph whose reference list is irregular raises IrregularKnnGraph by the index_check contract (a plain
        # attribute as well; False: every path and refusal as without it)
        self.static_knn = False
        self._enc_digest: Optional[str] = None        # encoder_digest() cache (cleared wherever the packed weights are)
        self._map_graphs: Dict[tuple, Tuple[torch.Tensor, torch.Tensor]] = {}   # forward_map: (G, K+1, device) -> (edges, batch)
        # forward_map(outputs="query"): same key -> (selected columns [G K], query nodes [G], the selected edges [2, G K])
        self._map_queries: Dict[tuple, Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = {}
        # relocalize(capture=True): its captured micro-batch steps (graphed.GraphedForwardMap) and the pose rules they were
        # captured with, by shape / configuration; dropped with the packed weights, which every captured step reads
        self._map_captures: Dict[tuple, object] = {}

    @property
    def encoder_dtype(self) -> str:
        """'f32' (default; the 1e-4 parity path) or 'bf16' (BASELINE configs[2]: bf16 activations + bf16 MFMA convs)."""
        return self._enc.dtype

    @property
    def accepts_bf16_input(self) -> bool:
        """True if ``data.x`` may be bf16: the bf16 encoder rounds its fp32 input to bf16 first thing (the fused 64-channel stem
        and the three-kernel stem alike, round 4: ``RPG_TUNE_FUSED_STEM=0`` no longer turns bf16 staging into an error), so
        images rounded on the host (``evaluate_stream``: half the H2D bytes) give bit-identical results."""
        return self.encoder_dtype == "bf16"

    @encoder_dtype.setter
    def encoder_dtype(self, dtype: str) -> None:
        self._enc.set_dtype(dtype)
        self._enc_digest = None

    @property
    def gnn_dtype(self) -> str:
        """'f32' (default; the 1e-4 parity path) or 'bf16': the GNN's Linears on the bf16 matrix pipe (inputs rounded to
        bf16 per Linear, fp32 accumulation / bias / residual / output; attention rows, scatter-mean and heads stay fp32).
        Meant to go with encoder_dtype = 'bf16' (BASELINE configs[2]/[4]); needs the default flags (use_AP, no
        use_attention, knn <= 0) and D % 64 == 0.  With knn > 0 it runs on one stream, except in ``forward_map`` with
        ``static_knn``, which serves it per stream slot (the bf16 forward takes any edge list, and that step's poses are held
        to the one-stream path's in tests/test_hip_knn_map.py; why the waiting kNN build was kept off the slots with the bf16
        GNN is not recorded, so that path stays as it is)."""
        return self._gnn_dtype

    @gnn_dtype.setter
    def gnn_dtype(self, dtype: str) -> None:
        if dtype not in ("f32", "bf16"):
            raise ValueError("gnn_dtype must be 'f32' or 'bf16'")
        self._gnn_dtype = dtype

    # ---- packed-weight cache ------------------------------------------------------------------------------------
    def refresh_packed(self) -> None:
        """Drop the packed device copies of the weights (call after mutating parameters in place)."""
        self._enc.invalidate()
        self._gnn_packed, self._gnn_ptrs = None, None
        self._gnn_bf16, self._gnn_bf16_ptrs = None, None
        self._extra = {}
        self._ws_pool.clear()
        self._enc_digest = None
        self._map_captures = {}

    def _apply(self, fn, *a, **k):
        if hasattr(self, "_enc"):
            self.refresh_packed()
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self.refresh_packed()
        return super().load_state_dict(*a, **k)

    # ---- reference API ------------------------------------------------------------------------------------------
    def compute_RP(self, p, edge_index):
        """Relative pose targets p[src] - p[dst] (posenet.py:1021-1031; training-side helper, plain indexing)."""
        return p[edge_index[0]] - p[edge_index[1]]

    def _pack_gnn(self):
        if self._gnn_packed is None:
            sd = {kk: v.detach() for kk, v in self.state_dict().items() if not kk.startswith("feature_extractor.")}
            if not self.use_AP:        # the node heads take pair features: pack them separately, keep slots 18/19 valid
                self._extra["heads_pair_w"] = torch.cat([sd["fc_xyz.weight"], sd["fc_wpqr.weight"]], 0).float().contiguous()
                self._extra["heads_pair_b"] = torch.cat([sd["fc_xyz.bias"], sd["fc_wpqr.bias"]], 0).float().contiguous()
                d = sd["proj_edge.weight"].shape[0]
                sd["fc_xyz.weight"], sd["fc_wpqr.weight"] = sd["fc_xyz.weight"][:, :d], sd["fc_wpqr.weight"][:, :d]
            if self.use_attention:
                self._extra["att_gtp_w"] = torch.cat([sd["att.g.weight"], sd["att.theta.weight"], sd["att.phi.weight"]], 0).float().contiguous()
                self._extra["att_gtp_b"] = torch.cat([sd["att.g.bias"], sd["att.theta.bias"], sd["att.phi.bias"]], 0).float().contiguous()
                self._extra["att_w"], self._extra["att_b"] = sd["att.W.weight"].float().contiguous(), sd["att.W.bias"].float().contiguous()
            self._gnn_packed = pack_gnn(sd)
            if len(self._gnn_packed) == 26:            # the split table: the fp32 forward can take the mean before mlp.2
                self._gnn_packed += pack_gnn_mean_first(self._gnn_packed)
            self._gnn_ptrs = _L.ptr_array([t.data_ptr() for t in self._gnn_packed])
        if self._gnn_dtype == "bf16" and self._gnn_bf16 is None:
            self._gnn_bf16 = pack_gnn_bf16(self._gnn_packed)
            self._gnn_bf16_ptrs = _L.ptr_array([t.data_ptr() for t in self._gnn_bf16])

    # ---- edge_index validation without a host synchronisation (status.DeferredCounters) ------------------------------
    def publish_status(self) -> None:
        """Enqueue the counters' copy to pinned memory behind the kernels issued so far (current stream); with
        ``index_check = "sync"`` read them back instead.  Every forward ends with it.  Also for callers that replay a captured
        forward (graphed.GraphedForward): the replayed kernels keep counting bad edges on the device; this enqueues the copy
        of the counters behind the replay."""
        self._counters.publish(sync=self.index_check == "sync")

    def check_edge_index(self, wait: bool = True) -> None:
        """Raise IndexError if a forward issued so far had an edge with a node id out of range (the error the reference's
        indexing raises at the call itself).  ``wait=True`` blocks until EVERY forward issued so far has reported.
        ``wait=False`` only looks at what has already arrived in the pinned mirror: for a caller that has just synchronised
        on a later event of the same stream (``evaluate_stream`` after its device-to-host copy of batch i, with batch i+1
        already enqueued) that covers batch i without waiting for batch i+1; the counters accumulate on the device, so a
        report that is not in yet is seen by the next look."""
        self._counters.check(wait)

    def _prepare(self, x: torch.Tensor, what: str, scenes=None):
        """The start of every forward: images as the encoder takes them, the bad-edge report of the previous call if it has
        landed, packed weights.  -> (x [n, 3, H, W], the library, the device counters int32 [16]).  ``scenes``: as ``encode``'s."""
        x = self._encoder_input(x, what, scenes)                                  # posenet.py:1035
        lib = _L.lib()
        self._counters.poll()                     # bad-edge report of the previous call, if it has landed
        # all weight packing happens here, on the caller's stream, BEFORE any side stream is forked off it
        self._pack_gnn()
        self._enc.ensure_packed(self.feature_extractor.state_dict, "", x.device)
        return x, lib, self._counters.tensor(x.device)

    def _fast(self, k, knn_ok: bool = True) -> bool:
        """Whether the multi-stream schedule (_forward_streams) applies.  ``knn_ok``: the caller's batch vector can serve the
        per-slot kNN build."""
        return bool(self.use_AP and not self.use_attention and k is None and knn_ok
                    and not (self.knn > 0 and self._gnn_dtype == "bf16"))

    def _gnn_call(self, lib, feat, esrc_ptr, edst_ptr, node_off, n, e, abs_pose, rel_pose, node_f, edge_f, status, slot, query=None):
        """``query``: None, or (sel int64 [e_sel], qnodes int64 [q]) -- the query-only output mode (rpg_gnn_forward_query_*):
        the outputs then have q / e_sel rows."""
        d = feat.shape[1]
        # the slot's workspace (resnet.WorkspacePool): the SAME buffer the encoder call of this slot used a moment ago on
        # this stream -- stream order makes the reuse safe, and the split-K scratch slice exists once per slot
        bf16 = self._gnn_dtype == "bf16"
        weights = (self._gnn_ptrs, len(self._gnn_packed))
        if bf16:
            weights += (self._gnn_bf16_ptrs, len(self._gnn_bf16))
        if query is None:
            ws = self._ws_pool.get(slot, lib.rpg_gnn_workspace_bytes(n, e, d), feat.device)
            fn, name = (lib.rpg_gnn_forward_bf16, "gnn_forward_bf16") if bf16 else (lib.rpg_gnn_forward_f32, "gnn_forward")
            sel_args = ()
        else:
            sel, qn = query
            ws = self._ws_pool.get(slot, lib.rpg_gnn_query_workspace_bytes(n, e, d, sel.numel(), qn.numel()), feat.device)
            fn, name = ((lib.rpg_gnn_forward_query_bf16, "gnn_forward_query_bf16") if bf16
                        else (lib.rpg_gnn_forward_query_f32, "gnn_forward_query"))
            sel_args = (sel.data_ptr(), sel.numel(), qn.data_ptr(), qn.numel())
        rc = fn(*weights, feat.data_ptr(), esrc_ptr, edst_ptr, node_off, n, e, d, int(self.gnn_recursion), *sel_args, abs_pose.data_ptr(),
                rel_pose.data_ptr(), None if node_f is None else node_f.data_ptr(),
                None if edge_f is None else edge_f.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(),
                torch.cuda.current_stream().cuda_stream)
        _L.check(rc, name)

    def _mc(self):
        """``mc_dropout`` if set -- after the checks every forward makes before it queues anything."""
        mc = self.mc_dropout
        if mc is None:
            return None
        if not self.droprate > 0:
            raise ValueError("mc_dropout samples the always-on dropout: it needs droprate > 0 (set model.mc_dropout = None for a "
                             "model without dropout)")
        if not self.use_AP:
            raise NotImplementedError("mc_dropout does not serve use_AP=False (its absolute poses are a Linear over pairs of "
                                      "dropped node features, not the six-wide heads)")
        return mc

    def _pool_rows(self, key, rows: int, d: int, dev) -> torch.Tensor:
        """fp32 [rows, d] in the workspace pool under ``key``: the feature buffers of the Monte-Carlo heads, which a captured
        step must not allocate."""
        nbytes = max(rows, 1) * d * 4
        return self._ws_pool.get(key, nbytes, dev)[:nbytes].view(torch.float32).view(max(rows, 1), d)[:rows]

    def _drop_heads(self, node_f, edge_f, abs_out, rel_out, mc=None):
        """The reference's always-on dropout (posenet.py:1073-1075), then the heads kernel on the dropped features, which
        overwrites the poses the GNN call made from the undropped ones (the node heads only with ``use_AP``: without it the
        caller makes abs_pose from the returned, dropped node features).  ``mc`` (with ``mc_dropout``): (node ids or None, their
        offset, (edge sources, edge targets), their offset, abs_var, rel_var) -- the sample means go to abs_out / rel_out, the
        variances to the last two, and the masks follow the ids (ops.pose_heads_mc), not torch's generator."""
        t = self._gnn_packed
        if mc is not None:
            node_ids, node_off, edge_ids, edge_off, abs_var, rel_var = mc
            md = self.mc_dropout
            state = md.state(node_f.device)
            ops.pose_heads_mc(node_f, t[18], t[19], self.droprate, md.samples, md.seed, state, node_ids, node_off,
                              out=(abs_out, abs_var))
            if edge_f.shape[0]:
                ops.pose_heads_mc(edge_f, t[20], t[21], self.droprate, md.samples, md.seed, state, edge_ids, edge_off,
                                  out=(rel_out, rel_var))
            return node_f
        node_f = F.dropout(node_f, p=self.droprate)
        if self.use_AP:
            ops.pose_heads(node_f, t[18], t[19], out=abs_out)
        ops.pose_heads(F.dropout(edge_f, p=self.droprate), t[20], t[21], out=rel_out)
        return node_f

    @staticmethod
    def _graph_sizes(data, n_total: int, e_total: Optional[int]):
        """(nodes per graph, edges per graph) as host lists, or None.  Sources, cheapest first: this package's
        ``Batch.graph_sizes``; the host-side slice tables a ``torch_geometric`` ``Batch`` keeps from collation
        (``_slice_dict`` in PyG 2.x, ``__slices__`` in 1.x: cumulative offsets, never moved to the GPU -- this is what the
        reference's DataLoader hands over, testing/test.py:193); ``data.ptr`` / ``data.batch`` (device tensors: one small
        device-to-host copy BEFORE any kernel of this call is enqueued)."""
        nodes_only = e_total is None          # kNN path: data.edge_index is replaced, only the node ranges are needed
        gs = getattr(data, "graph_sizes", None)
        if gs is not None:
            if nodes_only:
                return (gs[0], [0] * len(gs[0])) if sum(gs[0]) == n_total else None
            return gs if sum(gs[0]) == n_total and sum(gs[1]) == e_total else None
        for attr in ("_slice_dict", "__slices__"):
            sl = getattr(data, attr, None)
            if isinstance(sl, dict) and "x" in sl and (nodes_only or "edge_index" in sl):
                cn = [int(v) for v in torch.as_tensor(sl["x"]).tolist()]
                if nodes_only:
                    ok = len(cn) >= 2 and cn[0] == 0 and cn[-1] == n_total
                    return ([b - a for a, b in zip(cn, cn[1:])], [0] * (len(cn) - 1)) if ok else None
                ce = [int(v) for v in torch.as_tensor(sl["edge_index"]).tolist()]
                if len(cn) == len(ce) >= 2 and cn[0] == 0 and ce[0] == 0 and cn[-1] == n_total and ce[-1] == e_total:
                    return ([b - a for a, b in zip(cn, cn[1:])], [b - a for a, b in zip(ce, ce[1:])])
                return None
        ptr, batch = getattr(data, "ptr", None), getattr(data, "batch", None)
        if torch.is_tensor(ptr) and ptr.dim() == 1 and ptr.numel() >= 2:
            cn = [int(v) for v in ptr.tolist()]
            nodes = [b - a for a, b in zip(cn, cn[1:])]
        elif torch.is_tensor(batch) and batch.dim() == 1 and batch.numel() == n_total and n_total > 0:
            nodes = [int(v) for v in torch.bincount(batch).tolist()]
        else:
            return None
        if sum(nodes) != n_total or len(nodes) < 2 or not torch.is_tensor(batch) or batch.numel() != n_total:
            return None
        if nodes_only:
            return (nodes, [0] * len(nodes))
        ei = data.edge_index
        gid = batch[ei[0]]                                     # graph of every edge (PyG keeps a graph's edges together)
        if e_total > 1 and bool((gid[1:] < gid[:-1]).any()):
            return None                                        # edges not grouped by graph: no contiguous cut exists
        edges = [int(v) for v in torch.bincount(gid, minlength=len(nodes)).tolist()]
        return (nodes, edges) if sum(edges) == e_total else None

    def _partition(self, data, n_total: int, e_total: Optional[int]):
        """Contiguous groups of whole graphs, one per stream: [(n0, n1, e0, e1, slot), ...] or None (single stream).
        ``e_total=None``: the caller replaces ``data.edge_index`` (kNN graph) -- only the node ranges matter then."""
        parts = min(int(self.hip_streams), 8)                  # one bad-edge counter per slot (self._counters)
        if parts < 2:
            return None
        ng = getattr(data, "num_graphs", None)
        if isinstance(ng, int) and ng < 2 * parts:             # e.g. the reference's batch_size=1 loop: nothing to cut
            return None
        gs = self._graph_sizes(data, n_total, e_total)
        if gs is None or len(gs[0]) < 2 * parts:
            return None
        nodes, edges = gs
        if self.stream_schedule:
            cn, ce = [0], [0]
            for a, b in zip(nodes, edges):
                cn.append(cn[-1] + a)
                ce.append(ce[-1] + b)
            out = []
            for g0, g1, slot in self.stream_schedule:
                if not (0 <= g0 < g1 <= len(nodes)) or not (0 <= slot < 8):
                    raise ValueError("stream_schedule: groups must be non-empty ranges of graphs, slots 0..7")
                out.append((cn[g0], cn[g1], ce[g0], ce[g1], slot))
            # exact-once coverage: sorted by first graph, every group starts where the previous one ended (equal lengths
            # alone would let (0,2),(1,3) through: rows 0..0 computed twice on racing streams, row 3 never written)
            nxt = 0
            for g0, g1, _ in sorted(self.stream_schedule):
                if g0 != nxt:
                    raise ValueError("stream_schedule must cover every graph of the batch exactly once "
                                     f"(gap or overlap at graph {min(g0, nxt)})")
                nxt = g1
            if nxt != len(nodes):
                raise ValueError("stream_schedule must cover every graph of the batch exactly once")
            return out
        out, g0, n0, e0 = [], 0, 0, 0
        for p in range(parts):
            g1 = len(nodes) * (p + 1) // parts
            n1, e1 = n0 + sum(nodes[g0:g1]), e0 + sum(edges[g0:g1])
            out.append((n0, n1, e0, e1, p))
            g0, n0, e0 = g1, n1, e1
        return out

    @torch.no_grad()
    def forward(self, data, k=None):
        x, edge_index = data.x, data.edge_index
        if not x.is_cuda:
            raise RuntimeError("PoseNetX_R2 (HIP) needs its inputs on the GPU: call data.to(device) first "
                               "(there is no CPU fallback)")
        if not torch.is_tensor(edge_index) or edge_index.device != x.device:
            raise RuntimeError("data.edge_index must be a tensor on the same GPU as data.x")
        self._mc()
        x, lib, _ = self._prepare(x, "data.x")
        # The multi-stream schedule serves the reference's default CLI flags too (round 5; testing/test.py:308-309: --knn 4
        # --droprate 0.5): the kNN graph is built per stream slot from that slot's encoder output, dropout + heads run per slot.
        batch_t = getattr(data, "batch", None)
        knn_ok = self.knn <= 0 or (torch.is_tensor(batch_t) and batch_t.dtype == torch.int64 and batch_t.device == x.device
                                   and batch_t.dim() == 1 and batch_t.numel() == x.size(0))
        parts = self._partition(data, x.size(0), edge_index.size(1) if self.knn <= 0 else None) if self._fast(k, knn_ok) else None
        if parts is not None and edge_index.dtype == torch.int64 and edge_index.dim() == 2 and edge_index.is_contiguous():
            enc_sd = self.feature_extractor.state_dict
            return self._forward_streams(lib, lambda n0, n1, wkey: self._enc.run(enc_sd, "", x[n0:n1], slot=wkey), x.size(0),
                                         x.device, edge_index, parts, batch_t)
        feat = self._encode_small(x)                                              # posenet.py:1037
        return self._forward_tail(lib, feat, edge_index, getattr(data, "batch", None), k)

    def _forward_tail(self, lib, feat, edge_index, batch, k, query=None, uniform=None):
        """Everything after the encoder on one stream (posenet.py:1040-1091): feat [N, d] are the node features.  ``query``: None,
        or forward_map's (selected columns, query nodes, selected edges) -- the outputs then cover those rows only.  ``uniform``
        (forward_map with static_knn): (graphs, nodes per graph, the caller's irregular counter or None) -- the kNN graph is built
        at fixed positions, and ``query`` comes without its edges, which are made here."""
        n, d = feat.shape
        if uniform is not None:
            irr = uniform[2] if uniform[2] is not None else self._counters.counters[16:17]
            edge_index, q_edges, _ = ops.knn_graph_uniform(feat, uniform[0], uniform[1], int(self.knn), 0,
                                                           q_out=None if query is None else True, irregular=irr)
            if query is not None:
                query = (query[0], query[1], q_edges)
        if self.use_attention:                                                    # posenet.py:1040-1041
            ex = self._extra
            y = ops.attention_rows(ops.linear_gather([(feat, None)], ex["att_gtp_w"], ex["att_gtp_b"], n))
            feat = ops.linear_gather([(y, None)], ex["att_w"], ex["att_b"], n, residual=feat)

        edge_index_knn = None                                                     # posenet.py:1043-1050
        if k is not None:
            edge_index_knn = ops.knn_graph(feat, int(k), batch)
        if self.knn > 0 and uniform is None:
            edge_index = ops.knn_graph(feat, int(self.knn), batch)
        elif k is not None:
            edge_index = edge_index_knn

        if edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.size(0) != 2:
            raise ValueError("edge_index must be an int64 tensor of shape [2, E]")
        ei = edge_index.contiguous()
        e = ei.size(1)
        dev = feat.device
        n_out, e_out = (n, e) if query is None else (query[1].numel(), query[0].numel())
        abs_pose = torch.empty((n_out, 6), dtype=torch.float32, device=dev)
        rel_pose = torch.empty((e_out, 6), dtype=torch.float32, device=dev)
        status = self._counters.counters[0:1]
        drop = self.droprate > 0
        want_feats = drop or not self.use_AP
        md = self._mc()
        if md is not None:
            node_f, edge_f = self._pool_rows((600, 99), n_out, d, dev), self._pool_rows((700, 99), e_out, d, dev)
        else:
            node_f = torch.empty((n_out, d), dtype=torch.float32, device=dev) if want_feats else None
            edge_f = torch.empty((e_out, d), dtype=torch.float32, device=dev) if drop else None
        self._gnn_call(lib, feat, ei.data_ptr(), ei.data_ptr() + 8 * e, 0, n, e, abs_pose, rel_pose, node_f, edge_f, status, 0,
                       None if query is None else query[:2])

        self.publish_status()                     # every call is validated; nothing blocks in "deferred" mode

        if md is not None:
            # node rows are numbered by their row (the query rows by their node id), edge rows by their end points
            md.last = McSpread(torch.empty_like(abs_pose), torch.empty_like(rel_pose))
            ids = (None, ei) if query is None else (query[1], query[2])
            self._drop_heads(node_f, edge_f, abs_pose, rel_pose, (ids[0], 0, (ids[1][0], ids[1][1]), 0, *md.last))
            md.advance(dev)
        elif drop:
            node_f = self._drop_heads(node_f, edge_f, abs_pose, rel_pose)
        if query is not None:                     # use_AP, no general kNN graph: refused by forward_map otherwise
            return abs_pose, rel_pose, (query[2] if uniform is not None else query[2].clone())
        if not self.use_AP:                                                       # posenet.py:1080-1083
            # index plumbing (compute_edge_features).  Clamped like the GNN's own copy of the end points (rpg_graph_prepare):
            # with index_check="deferred" an out-of-range node id is REPORTED by the device-side counter (IndexError at the
            # next look), and must not become an out-of-bounds row read of this gather in the meantime
            lo = torch.minimum(ei[0], ei[1]).clamp_(0, n - 1)
            hi = torch.maximum(ei[0], ei[1]).clamp_(0, n - 1)
            abs_pose = ops.linear_gather([(node_f, lo), (node_f, hi)], self._extra["heads_pair_w"],
                                         self._extra["heads_pair_b"], e)
        return abs_pose, rel_pose, (edge_index_knn if k is not None else edge_index)

    # ---- the map path: database images encoded once (featmap.FeatureMap), queries encoded per call ---------------------
    def encoder_digest(self) -> str:
        """SHA-256 of the encoder's state dict (names, dtypes, shapes, bytes): what a FeatureMap is bound to.  Computed once (one
        copy of the weights to the host) and cached; cleared wherever the packed weights are (load_state_dict, refresh_packed,
        _apply, the encoder_dtype setter)."""
        if self._enc_digest is None:
            import hashlib
            h = hashlib.sha256()
            for name, v in self.feature_extractor.state_dict().items():
                t = v.detach().cpu().contiguous()
                h.update(f"{name}|{t.dtype}|{tuple(t.shape)}|".encode())
                h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())
            self._enc_digest = h.hexdigest()
        return self._enc_digest

    @torch.no_grad()
    def encode(self, x: torch.Tensor, scenes=None) -> torch.Tensor:
        """Encoder features [n, feat_dim] fp32 of images ``x`` (what ``forward`` runs at posenet.py:1037, before the optional
        model-level attention): fp32 processed images [n, 3*H*W] / [n, 3, H, W], bf16 ones for the bf16 encoder, or uint8 frames
        [n, H, W, 3] through ``frame_transform``; on the GPU.  ``scenes`` [n] (host integers or an int32 tensor on the GPU): the
        scene of every frame, required for uint8 frames when ``frame_transform`` is a ``frames.SceneFrameTransform`` (ValueError
        without) and not read otherwise."""
        if not torch.is_tensor(x) or not x.is_cuda:
            raise RuntimeError("encode: the images must be a tensor on the GPU (there is no CPU fallback)")
        if x.size(0) == 0:
            raise ValueError("encode: no images")
        x = self._encoder_input(x, "images", scenes)
        self._enc.ensure_packed(self.feature_extractor.state_dict, "", x.device)
        return self._encode_small(x)

    def _map_graph(self, g: int, n_per: int, dev) -> Tuple[torch.Tensor, torch.Tensor]:
        """(edge_index [2, G * n(n-1)], batch [G * n]) of G fully-connected n-node graphs on ``dev``: fc_batch's order."""
        key = (g, n_per, str(dev))
        hit = self._map_graphs.get(key)
        if hit is None:
            from .graph import fc_batch
            b = fc_batch(torch.empty((g * n_per, 0)), n_per)
            hit = (b.edge_index.to(dev), b.batch.to(dev))
            if len(self._map_graphs) >= 16:
                self._map_graphs.clear()
            self._map_graphs[key] = hit
        return hit

    def _map_query(self, g: int, n_per: int, dev) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(sel int64 [G K], qnodes int64 [G], edges [2, G K]) of ``_map_graph``'s list on ``dev``: the columns whose target is a
        query node g n, ascending (graph.query_edge_columns), the query nodes, and those columns of the list.  Graph after graph
        the list repeats one pattern, so the first j K entries of ``sel`` are the selection of any j consecutive graphs."""
        key = (g, n_per, str(dev))
        hit = self._map_queries.get(key)
        if hit is None:
            from .graph import query_edge_columns
            edges = self._map_graph(g, n_per, dev)[0]
            qn = torch.arange(g, dtype=torch.int64) * n_per
            sel = query_edge_columns(edges.cpu(), qn).to(dev)
            hit = (sel, qn.to(dev), edges[:, sel].contiguous())
            if len(self._map_queries) >= 16:
                self._map_queries.clear()
            self._map_queries[key] = hit
        return hit

    def _static_columns(self, k, kk: int) -> int:
        """k' = min(knn, K), the incoming edges of every node of a K + 1-node graph, if ``forward_map`` builds its kNN graph at
        fixed positions (``static_knn``, on the flags the multi-stream schedule serves); 0 otherwise."""
        if self.static_knn and self.knn > 0 and k is None and self.use_AP and not self.use_attention:
            return min(int(self.knn), int(kk))
        return 0

    def _map_query_knn(self, g: int, n_per: int, kp: int, dev) -> Tuple[torch.Tensor, torch.Tensor]:
        """(sel int64 [G k'], qnodes int64 [G]) of the fixed-position kNN list of G graphs of ``n_per`` nodes on ``dev``: node v's
        columns are v k' + [0, k'), so query g's (node g n_per) are g n_per k' + [0, k') whatever the features are.  As for
        ``_map_query`` the first j k' entries of ``sel`` are the selection of any j consecutive graphs."""
        key = ("knn", g, n_per, kp, str(dev))
        hit = self._map_queries.get(key)
        if hit is None:
            qn = torch.arange(g, dtype=torch.int64) * n_per
            sel = ((qn * kp)[:, None] + torch.arange(kp, dtype=torch.int64)[None, :]).reshape(-1)
            hit = (sel.to(dev), qn.to(dev))
            if len(self._map_queries) >= 16:
                self._map_queries.clear()
            self._map_queries[key] = hit
        return hit

    def _check_outputs(self, outputs, k) -> None:
        """``forward_map``'s ``outputs``: an unknown value and what the query-only mode does not serve raise here, before anything
        is queued."""
        if outputs not in ("all", "query"):
            raise ValueError(f"forward_map: outputs must be 'all' or 'query', got {outputs!r}")
        if outputs == "all":
            return
        why = "the selected columns would depend on the features"
        if self.knn > 0 and not self.static_knn:
            raise NotImplementedError(f"forward_map(outputs='query') does not serve knn > 0 (a model-built kNN graph: {why})")
        if k is not None:
            raise NotImplementedError(f"forward_map(outputs='query') does not serve an explicit k (a kNN graph: {why})")
        if self.use_attention:
            raise NotImplementedError("forward_map(outputs='query') does not serve use_attention (the one-stream path, which "
                                      "allocates between its launches)")
        if not self.use_AP:
            raise NotImplementedError("forward_map(outputs='query') does not serve use_AP=False (its absolute poses are per edge, "
                                      "from pair features of all nodes)")

    @torch.no_grad()
    def forward_map(self, queries: torch.Tensor, neighbours: Optional[torch.Tensor], fmap, k=None, *, rule=None,
                    query_descriptors: Optional[torch.Tensor] = None, query_groups=None, outputs: str = "all", _static=None,
                    _irregular: Optional[torch.Tensor] = None, prior=None, gate=None, scenes=None, _vote=None):
        """The forward of G graphs, each query g followed by the K database images ``neighbours[g]`` of the feature map ``fmap``
        (dataset_7Scenes_multi.py:340-345) -- with only the G queries through the encoder.  Returns what
        ``forward(fc_batch(assembled, K + 1), k)`` returns for the assembled images: (abs_pose [G*(K+1), 6], rel_pose [E, 6],
        edge_index [2, E]), fully-connected edges per graph in fc_edge_index order, or the kNN graph over the assembled node
        features with ``knn > 0`` / ``k``.  ``queries``: images as ``encode`` takes them; ``neighbours``: int64 [G, K] on the
        same GPU, K >= 1, rows of ``fmap`` (an index outside [0, M) raises IndexError under ``index_check``, as a bad edge does).
        Every flag of ``forward`` applies; ``fmap.check(self)`` refuses a map of other encoder weights or precision.

        ``neighbours=None`` with a ``rule`` (retrieval.RetrievalRule) retrieves them on the GPU (dataset_7Scenes_multi.py:238-264)
        and returns them as a FOURTH element, int64 [G, rule.k]: without ``query_descriptors`` the query's own encoder feature,
        which this call has just computed, is matched against ``fmap.features``; a map that holds ``descriptors`` needs
        ``query_descriptors`` fp32 [G, Dd] on the same GPU.  ``query_groups`` [G] (host integers): rows of ``fmap.groups`` equal
        to a query's group are left out; -1 leaves nothing out.  Nothing blocks: the ranks are made on the host before the
        launch, and a rank the map cannot serve is reported like a bad neighbour.

        ``outputs="query"`` (default ``"all"``) returns only what the pose rule of the map path reads (test.py:227-232): (abs_pose
        [G, 6] of the queries, rel_pose [G*K, 6], edge_index [2, G*K]) -- the columns of the full list whose target is a query node,
        in the full list's order (graph g's sources are g(K+1)+1 .. g(K+1)+K, in that order), node ids unchanged, and with a
        ``rule`` the neighbours as the fourth element, as before.  The last recursion of the GNN then runs its edge rows on those
        K of K(K+1) columns per graph and its node rows on the queries only (rpg_gnn_forward_query_*): every value is the one
        ``outputs="all"`` gives at the same row, up to the summation order of differently tiled GEMMs.  Same two-stream schedule,
        same workspace pool.  ``droprate > 0`` is served as for ``"all"``, but ``F.dropout`` is drawn over [G, D] and [G*K, D], so a
        seeded run draws OTHER masks than the full forward does -- unless ``model.mc_dropout`` is set: its masks follow the node
        ids (a query row's id is its node's, an edge row's the pair of its end points), so both modes draw the same ones.
        ``knn > 0`` without ``static_knn``, an explicit ``k``, ``use_attention`` and ``use_AP=False`` raise NotImplementedError (the
        selected columns of a general kNN list depend on the features, or the path allocates between its launches); an unknown
        value raises ValueError.

        ``model.static_knn = True`` with ``knn > 0`` (no explicit ``k``, ``use_AP``, no ``use_attention``; otherwise it is ignored):
        all graphs of this call have K + 1 nodes, so every node has exactly k' = min(knn, K) incoming edges, the list has G (K + 1)
        k' columns, node v's are v k' + [0, k') and only the SOURCE ids depend on the features.  The graph is then built at those
        positions on the device (``rpg_knn_graph_uniform_f32``: the general kernel's neighbours in its order) with nothing for the
        host to wait for: the multi-stream schedule runs without an event per slot, the bf16 GNN is served on it (from 32 graphs per
        slot on; below, one stream, as on the general path, measured faster), and
        ``outputs="query"`` is accepted -- abs_pose [G, 6], rel_pose [G k', 6], edge_index [2, G k'], the columns g (K + 1) k' + [0, k')
        of the full list.  The one exception: a node whose self match is not among its knn + 1 nearest by (distance, index) -- knn + 1
        or more lower-numbered nodes of its graph with a bit-identical feature row (the same map row named again and again), or
        non-finite rows; only with K > knn -- keeps k' + 1 edges in the reference.  Such a call is reported by the ``index_check``
        contract as ``IrregularKnnGraph`` (a ValueError: at the call under ``"sync"``, at the next look under ``"deferred"``); its
        outputs are a valid graph's, not the reference's, and ``static_knn = False`` reproduces the reference's.

        ``gate`` (retrieval.PoseGate) with ``prior`` float64 [G, 7] = (t[3], q[4]) per query, a device tensor or a host array
        (staged through pinned memory), with a ``rule`` only (``neighbours=`` given: ValueError; a rule with random draws:
        ValueError): retrieval is restricted to the map rows near each query's prior pose (``ops.retrieve_gated``: a NaN prior
        row ranks the whole map; a gate that holds fewer allowed rows than the rule's largest rank needs falls back to the whole
        map).  Both ``outputs`` modes and ``static_knn``.  The states are left on the model as ``self.gate_info`` -- int32 [G, 2]
        = (state, rows inside) on the device, valid behind this call's launches like ``mc_dropout.last`` -- and None by every
        call without a gate.

        ``scenes`` [G] (host integers, or an int32 tensor on the GPU): each query's scene.  With a ``rule`` on a
        ``featmap.SceneAtlas`` it is required (ValueError without: ranking across scenes is never what was meant) and every query
        is ranked against its own scene's rows only (``ops.retrieve_scoped``: both ``outputs`` modes, ``static_knn``,
        ``mc_dropout`` and the gate, whose "rows inside" are then the scene's); a rule with random draws needs the host form, and a
        rule whose ``k`` exceeds the smallest scene is refused.  With given ``neighbours``, or on one scene's map, it is read by the frame transform only:
        uint8 queries of a model whose ``frame_transform`` is a ``frames.SceneFrameTransform`` need it.  A scene index outside
        the atlas / the statistics is reported like a bad neighbour.
        A ``retrieval.SceneVote`` in its place (a ``rule`` on a ``SceneAtlas`` only): the queries are not told their scene, each
        elects it from its most similar rows of the whole atlas and is ranked there (``ops.retrieve_elect``) -- the same poses
        and neighbours, bit for bit, as with the elected scenes given.  Both ``outputs`` modes, ``static_knn``, ``mc_dropout`` and
        the gate are served; the result is left on the model as ``self.scene_info`` -- int32 [G, 2] = (elected scene, its votes)
        on the device, like ``gate_info`` -- and None by every call without a vote.  Refused (ValueError): a rule with random draws
        (their sizes follow the scene, on the host), given ``neighbours``, uint8 queries of a ``frames.SceneFrameTransform`` (the
        statistics are needed before the encoder, the scene is known behind it; a plain ``FrameTransform`` is served), ``top``
        above the atlas's rows, and ``lost_only`` (a step with static scenes only).

        ``_static`` (graphed.GraphedForwardMap only): ``(ranks int32 [G, K], query groups int64 [G] or None)`` already on the
        device, read in place of the two per-call host products above, so that nothing of the call depends on host data; with a
        gate two more elements, ``(..., prior float64 [G, 7], gate_info int32 [G, 2])``: the step's static prior (which a
        tracking loop updates on the device) and where the states go.
        ``_vote`` (GraphedForwardMap, tracking.Tracker; with ``scenes=SceneVote``): ``(q_scene int32 [G], scene_info int32 [G, 2])``,
        the caller's static tensors that the election reads (``lost_only``: -1 elects) and writes.
        ``_irregular`` (relocalize, GraphedForwardMap): an int32 [1] device counter of the caller's that the irregular nodes are
        added to INSTEAD of the model's own counters -- the caller looks at it and nothing raises."""
        self._check_outputs(outputs, k)
        if neighbours is not None and rule is not None:
            raise ValueError("forward_map: give neighbours or a retrieval rule, not both")
        if rule is None and (query_descriptors is not None or query_groups is not None):
            raise ValueError("forward_map: query_descriptors / query_groups belong to retrieval: pass a rule (and neighbours=None)")
        if gate is not None and rule is None:
            raise ValueError("forward_map: a pose gate restricts retrieval: pass a rule and neighbours=None (given neighbours are "
                             "used as they are)")
        if _static is not None and len(_static) > 2:
            prior = _static[2]
        if prior is not None or gate is not None:
            fmap.check_gate("forward_map", rule, prior, gate)
        self.gate_info = None
        self.scene_info = None
        from .retrieval import SceneVote
        if isinstance(scenes, SceneVote):
            from .frames import SceneFrameTransform
            if rule is None:
                raise ValueError("forward_map: a SceneVote finds the scene retrieval ranks in: pass a rule and neighbours=None "
                                 "(given neighbours are used as they are)")
            if (torch.is_tensor(queries) and queries.dtype == torch.uint8
                    and isinstance(self.frame_transform, SceneFrameTransform)):
                raise ValueError("forward_map: uint8 queries of a SceneFrameTransform need their scene's statistics before the "
                                 "encoder, and a SceneVote knows the scene only behind it: pass processed queries (or use a plain "
                                 "FrameTransform)")
        elif _vote is not None:
            raise ValueError("forward_map: _vote goes with scenes=SceneVote(...)")
        elif scenes is not None and torch.is_tensor(queries):
            from .frames import scenes_to_device
            scenes = scenes_to_device(scenes, queries.size(0), queries.device, "forward_map")      # (host or None, device)
        if rule is not None:
            return self._forward_map_retrieve(queries, fmap, k, rule, query_descriptors, query_groups, _static, outputs, _irregular,
                                              prior, gate, scenes, _vote)
        if not torch.is_tensor(queries) or not torch.is_tensor(neighbours):
            raise TypeError("forward_map: queries and neighbours must be tensors")
        if neighbours.dtype != torch.int64 or neighbours.dim() != 2:
            raise TypeError(f"forward_map: neighbours must be an int64 tensor [G, K] (rows of the feature map per query), got "
                            f"{neighbours.dtype} {tuple(neighbours.shape)}")
        g, kk = neighbours.shape
        if kk < 1:
            raise ValueError("forward_map: neighbours needs K >= 1 database images per query")
        if g < 1 or queries.size(0) != g:
            raise ValueError(f"forward_map: {queries.size(0)} queries but neighbours has {g} rows")
        self._map_devices(queries, fmap, "neighbours", neighbours)
        nb = neighbours.contiguous()
        return self._forward_map_run(queries, fmap, k, g, kk, lambda qf, g0, g1, st, wkey: nb[g0:g1], outputs, _irregular, scenes)

    @staticmethod
    def _map_devices(queries, fmap, name: str, t: Optional[torch.Tensor]) -> None:
        """``forward_map``'s device rules: the queries on a GPU, the feature map and the tensor ``t`` (if given) on the same one."""
        if not queries.is_cuda:
            raise RuntimeError("forward_map: queries must be on the GPU (there is no CPU fallback)")
        if fmap.device != queries.device or (t is not None and t.device != queries.device):
            where = "" if t is None else f" ({t.device})"
            raise RuntimeError(f"forward_map: queries ({queries.device}), {name}{where} and the feature map ({fmap.device}) "
                               f"must be on the same GPU")

    def _forward_map_retrieve(self, queries, fmap, k, rule, query_descriptors, query_groups, static=None, outputs="all",
                              irregular=None, prior=None, gate=None, scenes=None, vote_out=None):
        """``forward_map`` with the neighbours retrieved per stream slot from that slot's query features (or descriptors).
        ``static``: see ``forward_map``'s ``_static``; ``vote_out``: its ``_vote``."""
        if not torch.is_tensor(queries):
            raise TypeError("forward_map: queries must be a tensor")
        if fmap.descriptors is not None and query_descriptors is None:
            raise ValueError("forward_map: the map holds its own retrieval descriptors, so the queries' descriptors must be given "
                             "(query_descriptors [G, Dd]); only a map without descriptors is matched by encoder features")
        if fmap.descriptors is None and query_descriptors is not None:
            raise ValueError("forward_map: query_descriptors given, but the map holds no descriptors to match them against")
        g, kk = queries.size(0), rule.k
        if g < 1:
            raise ValueError("forward_map: no queries")
        if kk > len(fmap):
            raise ValueError(f"forward_map: the rule picks {kk} rows, the map has {len(fmap)}")
        qd = None
        if query_descriptors is not None:
            qd = query_descriptors
            if not torch.is_tensor(qd) or qd.dtype != torch.float32 or qd.dim() != 2 or qd.shape != (g, fmap.descriptors.shape[1]):
                raise ValueError(f"forward_map: query_descriptors must be fp32 [{g}, {fmap.descriptors.shape[1]}]")
        self._map_devices(queries, fmap, "query_descriptors", qd)
        dev = queries.device
        # everything the slots share is made here, on the caller's stream, before any side stream is forked off it
        qd = None if qd is None else qd.contiguous()
        # a SceneAtlas: (host scenes or None, q_scene int32 [G] on the device); None for one scene's map -- which takes no scenes,
        # except those that only the per-scene frame transform of uint8 queries reads
        from .featmap import SceneAtlas
        from .frames import SceneFrameTransform
        for_frames = queries.dtype == torch.uint8 and isinstance(self.frame_transform, SceneFrameTransform)
        scope = fmap._scope(scenes if isinstance(fmap, SceneAtlas) or not for_frames else None, g, rule, "forward_map",
                            ranks_given=static is not None, lost_ok=vote_out is not None)
        # a SceneVote: (None, None, the vote) -- the election writes q_scene, which the slots slice like the ranks
        vote = scope[2] if scope is not None and len(scope) == 3 else None
        q_scene = None
        if vote is not None:
            q_scene, scene_info = vote_out if vote_out is not None else (
                torch.empty(g, dtype=torch.int32, device=dev), torch.empty((g, 2), dtype=torch.int32, device=dev))
            self.scene_info = scene_info
            scenes = None                         # (nothing for the frame transform to read)
        if static is None:
            qg_host, qg_dev = fmap._query_groups(query_groups, g)
            ranks = rule.device_ranks(fmap.n_allowed(qg_host, g) if scope is None else fmap.n_allowed(qg_host, g, scope[0]), dev)
        else:                                     # the host's per-call products, already in the caller's device buffers
            ranks, qg_dev = static[:2]
        gate_rows = prior_dev = info = None
        if gate is not None:
            gate_rows = fmap.gate_rows(gate)
            if static is not None and len(static) > 2:
                prior_dev, info = static[2], static[3]
            else:
                prior_dev = fmap.prior_tensor(prior, g, "forward_map")
                info = torch.empty((g, 2), dtype=torch.int32, device=dev)
            self.gate_info = info
        inv, db = fmap.inv_norms(), fmap.descriptor_matrix
        db_groups = None if qg_dev is None else fmap.groups
        nb_out = torch.empty((g, kk), dtype=torch.int64, device=dev)
        ws_bytes = _L.lib().rpg_retrieve_workspace_bytes if vote is None else _L.lib().rpg_retrieve_elect_workspace_bytes

        def neighbours_of(qf, g0, g1, st, wkey):
            ws = self._ws_pool.get((400 + wkey[0], wkey[1]), int(ws_bytes(g1 - g0, db.shape[0], db.shape[1])), dev)
            if vote is not None:
                return ops.retrieve_elect(qf if qd is None else qd[g0:g1], db, ranks[g0:g1], fmap.scene_first, vote.top,
                                          q_scene=q_scene[g0:g1], lost_only=vote.lost_only, db_gate=gate_rows,
                                          prior=None if gate is None else prior_dev[g0:g1], r2=0.0 if gate is None else gate.r2,
                                          cos_half=0.0 if gate is None else gate.cos_half, rot_gate=gate is not None and gate.rot,
                                          db_inv_norm=inv, q_group=None if qg_dev is None else qg_dev[g0:g1], db_group=db_groups,
                                          status=st, workspace=ws, out=nb_out[g0:g1],
                                          gate_info=None if gate is None else info[g0:g1], scene_info=scene_info[g0:g1])[0]
            if scope is not None:
                res = ops.retrieve_scoped(qf if qd is None else qd[g0:g1], db, ranks[g0:g1], fmap.scene_first, scope[1][g0:g1],
                                          gate_rows, None if gate is None else prior_dev[g0:g1], 0.0 if gate is None else gate.r2,
                                          0.0 if gate is None else gate.cos_half, gate is not None and gate.rot, db_inv_norm=inv,
                                          q_group=None if qg_dev is None else qg_dev[g0:g1], db_group=db_groups, status=st,
                                          workspace=ws, out=nb_out[g0:g1], gate_info=None if gate is None else info[g0:g1])
                return res if gate is None else res[0]
            if gate is not None:
                return ops.retrieve_gated(qf if qd is None else qd[g0:g1], db, ranks[g0:g1], gate_rows, prior_dev[g0:g1], gate.r2,
                                          gate.cos_half, gate.rot, db_inv_norm=inv, q_group=None if qg_dev is None else qg_dev[g0:g1],
                                          db_group=db_groups, status=st, workspace=ws, out=nb_out[g0:g1], gate_info=info[g0:g1])[0]
            return ops.retrieve(qf if qd is None else qd[g0:g1], db, ranks[g0:g1], db_inv_norm=inv,
                                q_group=None if qg_dev is None else qg_dev[g0:g1], db_group=db_groups, status=st, workspace=ws,
                                out=nb_out[g0:g1])
        return (*self._forward_map_run(queries, fmap, k, g, kk, neighbours_of, outputs, irregular, scenes), nb_out)

    def _forward_map_run(self, queries, fmap, k, g, kk, neighbours_of, outputs="all", irregular=None, scenes=None):
        """``neighbours_of(qf, g0, g1, status, wkey)``: the map rows int64 [g1 - g0, K] of queries g0..g1, whose encoder features
        are ``qf``, made on the current (slot) stream.  ``irregular``: ``forward_map``'s ``_irregular``."""
        fmap.check(self)
        self._mc()
        x, lib, status = self._prepare(queries, "queries", scenes)
        dev = x.device
        n_per = kk + 1
        kp = self._static_columns(k, kk)          # > 0: the kNN graph at fixed positions (static_knn)
        uniform = None
        if kp:
            edge_index, batch = None, None        # built per slot, on the device
            query = self._map_query_knn(g, n_per, kp, dev) if outputs == "query" else None
            uniform = (g, n_per, irregular)
        else:
            edge_index, batch = self._map_graph(g, n_per, dev)
            query = self._map_query(g, n_per, dev) if outputs == "query" else None
            if query is None:
                edge_index = edge_index.clone()   # the caller's to keep (the cached copy serves the next call)
        enc_sd = self.feature_extractor.state_dict

        parts = None
        if kp or self._fast(k):
            from .graph import Data
            spec = Data()
            spec.graph_sizes = ([n_per] * g, [n_per * kk] * g)
            parts = self._partition(spec, g * n_per, edge_index.size(1) if self.knn <= 0 else None)
            # static_knn with the bf16 GNN: the general path it stands in for runs on ONE stream, and stream slots of fewer than
            # _STATIC_BF16_SLOT_GRAPHS graphs measured slower than that (see the constant).  Below it the step keeps the general
            # path's schedule -- the same launches without the wait -- unless the caller set a schedule of their own.
            if (kp and self._gnn_dtype == "bf16" and parts is not None and not self.stream_schedule
                    and g < _STATIC_BF16_SLOT_GRAPHS * len(parts)):
                parts = None
        if parts is not None:
            def features(n0, n1, wkey):           # the slot's queries through the encoder, then its graphs' nodes
                g0, g1 = n0 // n_per, n1 // n_per
                qf = self._enc.run(enc_sd, "", x[g0:g1], slot=wkey)
                st = status[8 + wkey[0]:9 + wkey[0]]
                return ops.gather_graph_nodes(qf, fmap.features, neighbours_of(qf, g0, g1, st, wkey), status=st)
            return self._forward_streams(lib, features, g * n_per, dev, edge_index, parts, batch, query=query,
                                         per_graph=(n_per, kp or kk), uniform=uniform)
        qf = self._encode_small(x)
        feat = ops.gather_graph_nodes(qf, fmap.features, neighbours_of(qf, 0, g, status[8:9], (-1, 0)), status=status[8:9])
        return self._forward_tail(lib, feat, edge_index, batch, k, query, uniform)

    def _encoder_input(self, x: torch.Tensor, what: str, scenes=None) -> torch.Tensor:
        """Images as the encoder takes them: uint8 frames through ``frame_transform``, dtype checked, viewed as [n, 3, H, W]."""
        if x.dtype == torch.uint8 and self.frame_transform is not None:
            x = self._transform_frames(x, scenes)
        if x.dtype != torch.float32 and not (x.dtype == torch.bfloat16 and self.accepts_bf16_input):
            raise TypeError(f"{what} must be float32 (the reference's input dtype; bf16 images are taken by the bf16 encoder "
                            f"only), got {x.dtype}")
        return x.view(x.size(0), 3, self.input_img_height, -1)                    # posenet.py:1035

    def _transform_frames(self, frames: torch.Tensor, scenes=None) -> torch.Tensor:
        """uint8 frames [n, H, W, 3] -> the encoder's input [n, 3, input_img_height, W'] through ``frame_transform``, in bf16 for
        the bf16 encoder (it rounds fp32 input to bf16 first thing: same poses) and fp32 otherwise.  Written into a pooled buffer
        on the caller's stream, before any side stream is forked off it; the buffer is reused by the next call, which the
        stream order of this call's readers (all joined back to the caller's stream) makes safe."""
        if frames.dim() != 4 or frames.shape[3] != 3:
            raise ValueError(f"uint8 data.x must be frames [n, H, W, 3] (RGB, HWC), got {tuple(frames.shape)}")
        ft = self.frame_transform
        oh, ow = ft.output_size(frames.shape[1], frames.shape[2])
        if oh != self.input_img_height:
            raise ValueError(f"frame_transform turns {frames.shape[1]}x{frames.shape[2]} frames into {oh}x{ow} images, but the "
                             f"model's input_img_height is {self.input_img_height}")
        dtype = torch.bfloat16 if self.accepts_bf16_input else torch.float32
        n = frames.shape[0]
        nbytes = n * 3 * oh * ow * (2 if dtype == torch.bfloat16 else 4)
        buf = self._ws_pool.get((200, 0), max(nbytes, 16), frames.device)[:nbytes].view(dtype).view(n, 3, oh, ow)
        from .frames import SceneFrameTransform
        if isinstance(ft, SceneFrameTransform):   # the statistics follow every frame's scene
            if scenes is None:
                raise ValueError("frame_transform holds per-scene statistics (SceneFrameTransform): uint8 frames need scenes [n], "
                                 "one scene index per frame")
            if isinstance(scenes, tuple):         # (host, device), already staged by forward_map: checked here as apply checks
                if scenes[0] is not None and scenes[0].size and (scenes[0].min() < 0 or scenes[0].max() >= len(ft)):
                    raise IndexError(f"scenes has entries outside the frame transform's scenes [0, {len(ft)})")
                scenes = scenes[1]
            # a device tensor's entries cannot be checked here: a scene outside the statistics is counted like a bad neighbour
            return ft.apply(frames, scenes, dtype, out=buf, status=self._counters.tensor(frames.device)[8:9])
        return ft.apply(frames, dtype, out=buf)

    def _encode_small(self, x: torch.Tensor) -> torch.Tensor:
        """The encoder for a batch that cannot be cut at graph boundaries (one graph: the reference's batch_size=1 loop,
        testing/test.py:192).  Images are independent, so the 8 images of a graph are spread over ``small_batch_streams`` HIP
        streams: at this size every kernel is a few hundred workgroups of a few microseconds and the forward is a chain of
        ~130 launch latencies (measured r3: 29 Winograd launches of 28 us + 29 fix-ups of 6 us for 8 images) -- two or four
        such chains side by side share the chip.  One stream for larger batches (they fill the chip by themselves)."""
        n = x.size(0)
        k = min(int(self.small_batch_streams), n)
        if k < 2 or n > 32:
            return self._enc.run(self.feature_extractor.state_dict, "", x)
        feat = torch.empty((n, self.feature_extractor.fc.out_features), dtype=torch.float32, device=x.device)
        cur, streams = self._fork(k, x.device)
        for p, st in enumerate(streams):
            i0, i1 = n * p // k, n * (p + 1) // k
            with torch.cuda.stream(st):
                self._enc.run(self.feature_extractor.state_dict, "", x[i0:i1], slot=(100, p), out=feat[i0:i1])
        self._join(cur, streams)
        return feat

    def _fork(self, n: int, dev) -> Tuple[torch.cuda.Stream, List[torch.cuda.Stream]]:
        """(the caller's stream, the first ``n`` side streams): every side stream waits for what the caller's stream has been
        given so far (inputs, packed weights, the outputs allocated on it) before it runs anything issued from here on."""
        while len(self._streams) < n:
            self._streams.append(torch.cuda.Stream(device=dev))
        cur = torch.cuda.current_stream()
        ready = torch.cuda.Event()
        ready.record(cur)
        for st in self._streams[:n]:
            st.wait_event(ready)
        return cur, self._streams[:n]

    @staticmethod
    def _join(cur: torch.cuda.Stream, streams: List[torch.cuda.Stream]) -> None:
        """The caller's stream waits for everything issued to the side streams so far."""
        for st in streams:
            cur.wait_stream(st)

    def _forward_streams(self, lib, features, n_total, dev, edge_index, parts, batch=None, query=None, per_graph=None, uniform=None):
        """use_AP / no extra attention / no explicit k, on ``len(parts)`` concurrent streams.  ``features(n0, n1, wkey)`` makes the
        node features [n1 - n0, d] of nodes n0..n1 on the current (slot) stream: the encoder over those images for ``forward``,
        the queries' encoder + node assembly from a feature map for ``forward_map``.  With ``knn > 0`` (the reference's
        default CLI, testing/test.py:308) every slot builds the kNN graph of ITS graphs from its own encoder output
        (posenet.py:1047-1048; graphs are independent, so the per-slot edge lists concatenate to the whole-batch list) and the
        host learns each slot's edge count behind an event on that slot's stream -- the other slots' encoders keep the GPU
        busy meanwhile -- before it enqueues the slot's GNN.  With ``droprate > 0`` the always-on dropout and the heads
        (posenet.py:1073-1086) run per slot on the slot's stream.  ``query`` (forward_map's query-only mode; ``per_graph`` =
        (nodes, selected columns) of every graph): the outputs cover the query nodes and the selected columns, and every slot
        computes the rows of its own graphs.  ``uniform`` (forward_map with static_knn; ``per_graph`` = (nodes, k') then): see
        ``_forward_tail`` -- every slot builds its kNN graph at fixed positions (ops.knn_graph_uniform) straight into its column
        range of the outputs, and its GNN is enqueued behind it with the edge count known: no pinned copy, no event, no wait."""
        knn = int(self.knn) if self.knn > 0 else 0
        drop = self.droprate > 0
        abs_pose = torch.empty((n_total if query is None else query[1].numel(), 6), dtype=torch.float32, device=dev)
        status = self._counters.counters
        cur, streams = self._fork(1 + max(p[4] for p in parts), dev)
        d = self.feature_extractor.fc.out_features
        md = self._mc()
        abs_var = None if md is None else torch.empty_like(abs_pose)

        def heads(feat, n0, n1, ei_ptrs, node_off, e, rel_out, slot, wkey, q_slot=None, mc_edges=None):
            """``mc_edges`` (with mc_dropout): (edge sources, edge targets, the offset that makes them ids of the whole batch, the
            slot's rows of rel_var)."""
            abs_out, n_out, e_out = abs_pose[n0:n1], n1 - n0, e
            if q_slot is not None:                # (first graph, selected columns, query nodes) of this slot
                n_out, e_out = q_slot[2].numel(), q_slot[1].numel()
                abs_out = abs_pose[q_slot[0]:q_slot[0] + n_out]
            if md is not None:
                # from the pool (a captured step allocates nothing); the slot's stream orders the reuse by the next call
                node_f = self._pool_rows((600 + wkey[0], wkey[1]), n_out, d, dev)
                edge_f = self._pool_rows((700 + wkey[0], wkey[1]), e_out, d, dev)
            else:
                node_f = torch.empty((n_out, d), dtype=torch.float32, device=dev) if drop else None
                edge_f = torch.empty((e_out, d), dtype=torch.float32, device=dev) if drop else None
            self._gnn_call(lib, feat, ei_ptrs[0], ei_ptrs[1], node_off, n1 - n0, e, abs_out, rel_out, node_f, edge_f,
                           status[slot:slot + 1], wkey, None if q_slot is None else q_slot[1:])
            if md is not None:
                # the slot's node rows are rows n0 .. of the batch; its query rows carry their node ids themselves
                var_out = abs_var[n0:n1] if q_slot is None else abs_var[q_slot[0]:q_slot[0] + n_out]
                node_ids, node_id_off = (None, n0) if q_slot is None else (q_slot[2], 0)
                self._drop_heads(node_f, edge_f, abs_out, rel_out,
                                 (node_ids, node_id_off, mc_edges[:2], mc_edges[2], var_out, mc_edges[3]))
            elif drop:
                self._drop_heads(node_f, edge_f, abs_out, rel_out)
                for buf in (node_f, edge_f):
                    buf.record_stream(torch.cuda.current_stream())

        if not knn:
            e_total = edge_index.size(1)
            rel_pose = torch.empty((e_total if query is None else query[0].numel(), 6), dtype=torch.float32, device=dev)
            rel_var = None if md is None else torch.empty_like(rel_pose)
            base = edge_index.data_ptr()
            for gi, (n0, n1, e0, e1, slot) in enumerate(parts):
                st = streams[slot]
                with torch.cuda.stream(st):
                    # workspaces are per (slot, position in the slot's queue): groups of a slot run in order, so they could share,
                    # but a different shape would re-allocate every call
                    wkey = (slot, gi)
                    feat = features(n0, n1, wkey)
                    rel_out, q_slot, c0, c1 = rel_pose[e0:e1], None, e0, e1
                    if query is not None:
                        # the slot's graphs g0 .. g1: their query nodes (ids of the whole batch, like the slot's edges) and, the
                        # list being one pattern per graph, the first (g1 - g0) K entries of the selection as its local columns
                        n_per, k_sel = per_graph
                        g0, g1 = n0 // n_per, n1 // n_per
                        q_slot = (g0, query[0][:(g1 - g0) * k_sel], query[1][g0:g1])
                        c0, c1 = g0 * k_sel, g1 * k_sel
                        rel_out = rel_pose[c0:c1]
                    mc_edges = None
                    if md is not None:            # the rows' end points, ids of the whole batch: the list's (or the selection's) columns
                        ends = edge_index if query is None else query[2]
                        mc_edges = (ends[0, c0:c1], ends[1, c0:c1], 0, rel_var[c0:c1])
                    heads(feat, n0, n1, (base + 8 * e0, base + 8 * (e_total + e0)), n0, e1 - e0, rel_out, slot, wkey, q_slot, mc_edges)
                    feat.record_stream(st)
            self._join(cur, streams)
            if md is not None:                    # once per forward, behind every slot's heads: the next call draws new masks
                md.last = McSpread(abs_var, rel_var)
                md.advance(dev)
            self.publish_status()
            return abs_pose, rel_pose, (edge_index if query is None else query[2].clone())

        if uniform is not None:
            # ---- knn > 0 at fixed positions (static_knn): every graph has n_per nodes, so slot and column ranges are known here
            n_per, kp = per_graph
            e_per = n_per * kp
            g_total = n_total // n_per
            edge_index = torch.empty((2, g_total * e_per), dtype=torch.int64, device=dev)
            q_edges = None if query is None else torch.empty((2, g_total * kp), dtype=torch.int64, device=dev)
            ends = edge_index if query is None else q_edges
            rel_pose = torch.empty((ends.size(1), 6), dtype=torch.float32, device=dev)
            rel_var = None if md is None else torch.empty_like(rel_pose)
            for gi, (n0, n1, _, _, slot) in enumerate(parts):
                st = streams[slot]
                with torch.cuda.stream(st):
                    wkey = (slot, gi)
                    feat = features(n0, n1, wkey)
                    g0, g1 = n0 // n_per, n1 // n_per
                    e0, e1 = g0 * e_per, g1 * e_per
                    src, dst = edge_index[0, e0:e1], edge_index[1, e0:e1]
                    q_slot, c0, c1 = None, e0, e1
                    if query is not None:
                        c0, c1 = g0 * kp, g1 * kp
                        q_slot = (g0, query[0][:c1 - c0], query[1][g0:g1])
                    ops.knn_graph_uniform(feat, g1 - g0, n_per, knn, n0, out=(src, dst),
                                          q_out=None if query is None else (q_edges[0, c0:c1], q_edges[1, c0:c1]),
                                          irregular=uniform[2] if uniform[2] is not None else status[16 + slot:17 + slot])
                    # the rows' end points, ids of the whole batch, read from the device list the kernel has just written
                    mc_edges = None if md is None else (ends[0, c0:c1], ends[1, c0:c1], 0, rel_var[c0:c1])
                    heads(feat, n0, n1, (src.data_ptr(), dst.data_ptr()), n0, e1 - e0, rel_pose[c0:c1], slot, wkey, q_slot, mc_edges)
                    feat.record_stream(st)
            self._join(cur, streams)
            if md is not None:
                md.last = McSpread(abs_var, rel_var)
                md.advance(dev)
            self.publish_status()
            return abs_pose, rel_pose, ends

        # ---- knn > 0: phase 1 = encoder + kNN build per slot (no host wait), phase 2 = GNN per slot once its edge count is in
        pend = []
        for gi, (n0, n1, _, _, slot) in enumerate(parts):
            st = streams[slot]
            with torch.cuda.stream(st):
                wkey = (slot, gi)
                feat = features(n0, n1, wkey)
                ei_buf, meta = ops.knn_graph_launch(feat, knn, batch[n0:n1])
                meta_h = torch.empty(2, dtype=torch.int32).pin_memory()
                meta_h.copy_(meta, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(st)
                pend.append((feat, ei_buf, meta, meta_h, ev, wkey))
        rels, eis, rel_vars = [], [], []
        for (n0, n1, _, _, slot), (feat, ei_buf, meta, meta_h, ev, wkey) in zip(parts, pend):
            ev.synchronize()
            total, bad = int(meta_h[0]), int(meta_h[1])
            if bad:
                # every slot's encoder + kNN work is already enqueued on the side streams and reads the caller's x (e.g. a
                # staging buffer the caller refills once this call returns OR raises): join them before leaving
                self._join(cur, streams)
                raise ValueError("knn_graph: a graph has more than 2048 nodes (unsupported)")
            st = streams[slot]
            with torch.cuda.stream(st):
                cap = ei_buf.size(1)
                rel = torch.empty((total, 6), dtype=torch.float32, device=dev)
                mc_edges = None
                if md is not None:                # the kNN edges' end points are ids of the slot: n0 makes them the batch's
                    rel_vars.append(torch.empty_like(rel))
                    rel_vars[-1].record_stream(cur)
                    mc_edges = (ei_buf[0, :total], ei_buf[1, :total], n0, rel_vars[-1])
                heads(feat, n0, n1, (ei_buf.data_ptr(), ei_buf.data_ptr() + 8 * cap), 0, total, rel, slot, wkey, None, mc_edges)
                ei_g = ei_buf[:, :total] + n0                                     # node ids of the whole batch (posenet.py:1048)
                eis.append(ei_g)
                rels.append(rel)
                for buf in (feat, ei_buf, meta):
                    buf.record_stream(st)
                for buf in (rel, ei_g):                # allocated on the slot's stream, concatenated on the caller's below
                    buf.record_stream(cur)
        self._join(cur, streams)
        if md is not None:
            md.last = McSpread(abs_var, torch.cat(rel_vars))
            md.advance(dev)
        self.publish_status()
        return abs_pose, torch.cat(rels), torch.cat(eis, dim=1)
