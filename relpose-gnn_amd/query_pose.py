"""``QueryPose``: the pose rule of the reference's evaluation (testing/test.py:213-267) on the device.

``evaluate.query_pose`` / ``evaluate.errors`` do this on the host, graph by graph, from a copy of every relative pose.  A
``QueryPose`` runs it as one kernel launch over all graphs of a forward's output (``ops.query_pose``, rpg_query_pose_f64) and
returns a device tensor float64 [G, 16] per call: pred (t, q) [7], targ (t, q) [7], translation error, rotation error in degrees
-- so a caller whose images, map poses and neighbours already live on the GPU gets the evaluation's products without a host
round trip, and an evaluation stream copies 128 bytes per graph back instead of the [E, 6] relative poses.

A graph that has no ``ref_node``-th edge into its query node (or whose reference edge starts outside the graph) cannot be
evaluated: its row is NaN and it is counted in a status word this object owns.  ``check`` turns a non-zero count into the
``ValueError`` of ``evaluate.reference_edge``.  The status word is a ``status.DeferredCounters`` with one counter, the class
behind ``PoseNetX_R2.check_edge_index`` too: the count travels to pinned host memory with an asynchronous copy behind every
call, so nothing blocks unless the caller asks it to.

``QueryPose(fuse="mean" | "median")`` keeps none of the edges into the query node to itself: every one of them (whose source is
not the query) is an estimate of the query's pose, and the row holds their combination (``ops.query_pose_fused``,
rpg_query_pose_fused_f64; ``evaluate.fused_query_pose`` is the rule in numpy).  Same row layout, same status word, same
``publish`` / ``check`` contract; a bad graph is then one without a usable edge or with a used edge from outside the graph.

``QueryPose(fuse="consensus", inlier_t=..., inlier_deg=...)`` is the mode that says whether the pose can be believed: the
candidates vote (two support each other when their translations lie within ``inlier_t`` and their rotations within
``inlier_deg`` degrees), the best-supported one wins and the row is the mean of its supporters alone
(rpg_query_pose_consensus_f64, the same kernel's third mode; ``evaluate.consensus_query_row`` is the rule in numpy).  With
``inliers=`` (int32 [G, 2]) every graph also gets (supporters of the winner, candidates used): their ratio is the accept /
reject signal that goes with the pose.  A non-finite candidate is an outlier there, it does not void the pose.

``QueryPose(fuse="mean" | "consensus", weights="variance", var_floor=...)`` weights the mean of those two rules by the inverse of
every edge's Monte-Carlo variance (``rel_var=``, fp32 [E, 6]: ``model.mc_dropout.last.rel_var`` of the forward whose ``rel_pose``
it reads) and, with ``spread=`` (float64 [G, 2]), gives every graph the predicted standard deviation of its fused translation and
rotation (rpg_query_pose_weighted_f64, a further mode of the same kernel; ``evaluate.weighted_query_row`` is the rule in numpy).

Whatever the rule, a stream asks the object for its output block (``output_block``: the rows, the integers if the rule has them,
the one tensor to copy back, and the spread if the rule has one -- ``rel_var`` is handed over exactly then) and cuts the host copy
with ``cut_block``; it never asks which rule runs.
"""
from __future__ import annotations

import torch

from . import ops
from .status import DeferredCounters


ROW_BYTES, INT_BYTES = 16 * 8, 2 * 4       # per graph: the row of 16 doubles, and the consensus rule's (inliers, used)
SPREAD_BYTES = 2 * 8                       # per graph: a weighted rule's (sigma_t, sigma_q)


def packed_block(g: int, device, spread: bool, ints: bool):
    """The outputs of ``g`` graphs in ONE allocation, section after section: the rows (128 B per graph), then -- if the rule has
    them -- the spread (16 B per graph), then the integers (8 B per graph).  -> (buf uint8, rows float64 [g, 16], spread float64
    [g, 2] | None, inliers int32 [g, 2] | None), views of ``buf``; every section starts 16-byte aligned wherever ``buf`` does.
    ``unpack_block`` cuts the host copy the same way."""
    buf = torch.empty(g * (ROW_BYTES + (SPREAD_BYTES if spread else 0) + (INT_BYTES if ints else 0)), dtype=torch.uint8,
                      device=device)
    return (buf,) + unpack_block(buf, spread, ints)


def unpack_block(buf, spread: bool, ints: bool):
    """A buffer of ``packed_block`` (a tensor or a numpy array) -> (rows [g, 16], spread [g, 2] | None, inliers [g, 2] | None)."""
    g = buf.shape[0] // (ROW_BYTES + (SPREAD_BYTES if spread else 0) + (INT_BYTES if ints else 0))
    r, s = g * ROW_BYTES, g * (ROW_BYTES + (SPREAD_BYTES if spread else 0))
    if torch.is_tensor(buf):
        return (buf[:r].view(torch.float64).view(g, 16), buf[r:s].view(torch.float64).view(g, 2) if spread else None,
                buf[s:].view(torch.int32).view(g, 2) if ints else None)
    return (buf[:r].view("<f8").reshape(g, 16), buf[r:s].view("<f8").reshape(g, 2) if spread else None,
            buf[s:].view("<i4").reshape(g, 2) if ints else None)


class QueryPose:
    def __init__(self, pose_m=(0.0, 0.0, 0.0), pose_s=(1.0, 1.0, 1.0), ref_node: int = 0, fuse=None, max_edges: int = 64,
                 inlier_t: float = ops.INLIER_T, inlier_deg: float = ops.INLIER_DEG, weights=None,
                 var_floor: float = ops.VAR_FLOOR):
        """``pose_m`` / ``pose_s``: translation mean / std (test.py:126-130, 248-251); ``ref_node``: which of the edges into the
        query node is the reference edge (test.py:227-229).  ``fuse``: None (that one edge), or ``"mean"`` / ``"median"`` /
        ``"consensus"``: the first ``max_edges`` (1..64) edges into the query node combined -- there is no reference edge then,
        so ``ref_node`` must stay 0.  ``inlier_t`` / ``inlier_deg``: the thresholds of ``"consensus"`` (checked always, used by
        that mode only).  Their defaults 0.25 / 5.0 are API defaults, not measured optima: they belong to the scene's scale, and
        ``inlier_t`` is compared after ``* pose_s + pose_m``, i.e. in the unit of the un-normalised translation.  Both finite,
        ``inlier_t >= 0``, ``0 <= inlier_deg <= 360`` (ValueError).  ``weights``: None, or ``"variance"`` with ``fuse="mean"`` /
        ``"consensus"`` (ValueError with the other rules): the mean weighs every candidate by ``1 / (variance + var_floor)``
        (``ops.query_pose_fused``).  ``var_floor``: finite and >= 1e-30 (checked always); 1e-12 is an API default, not a tuned
        value."""
        self.pose_m, self.pose_s = ops._qp_triple(pose_m, "pose_m"), ops._qp_triple(pose_s, "pose_s")
        self.ref_node = ops._qp_ref_node(ref_node)
        self.fuse, self.max_edges = fuse, max_edges
        self.inlier_t, self.inlier_deg = ops._qp_thresholds(inlier_t, inlier_deg, "QueryPose")
        self.weights, self.var_floor = ops._qp_weights(weights, fuse, var_floor, "QueryPose")
        if fuse is not None:
            ops._qp_fuse(fuse, max_edges, "QueryPose")
            if self.ref_node != 0:
                raise ValueError(f"QueryPose: fuse={fuse!r} combines every edge into the query node, ref_node={ref_node} selects "
                                 "one: give one of the two")
        self._bad = DeferredCounters(1, self._error)          # graphs that could not be evaluated

    # ---- the output block: what a stream allocates per micro-batch and copies back in one piece ----------------------------
    def output_block(self, g: int, device):
        """The outputs of ``g`` graphs on ``device``: -> (rows float64 [g, 16] for ``out=``, inliers int32 [g, 2] for ``inliers=``
        or None, the ONE tensor a stream copies back, spread float64 [g, 2] for ``spread=`` or None).  That tensor is the rows
        themselves, 128 bytes per graph -- except where the rule writes more: a weighted rule's spread (16 bytes per graph) and
        the two integers of ``fuse="consensus"`` (8 bytes) travel behind the rows in one buffer (``packed_block``: 136 bytes per
        graph for ``"consensus"``, 144 for weighted ``"mean"``, 152 for weighted ``"consensus"``).  A caller hands ``rel_var=``
        to ``from_targets`` / ``from_map`` exactly when the spread is not None."""
        spread, ints = self.weights is not None, self.fuse == "consensus"
        if not spread and not ints:
            rows = torch.empty((g, 16), dtype=torch.float64, device=device)
            return rows, None, rows, None
        buf, rows, sp, ints = packed_block(g, device, spread, ints)
        return rows, ints, buf, sp

    def cut_block(self, host):
        """A host copy (tensor or numpy array) of the tensor ``output_block`` says to copy back -> (rows [g, 16], inliers [g, 2]
        or None, spread [g, 2] or None), views of it."""
        spread, ints = self.weights is not None, self.fuse == "consensus"
        if not spread and not ints:
            return host, None, None
        rows, sp, ints = unpack_block(host, spread, ints)
        return rows, ints, sp

    # ---- the two forms ---------------------------------------------------------------------------------------------------
    def from_targets(self, rel_pose, edge_index, node_first, node_targets, edge_first=None, out=None, candidates=None,
                     counts=None, inliers=None, rel_var=None, spread=None) -> torch.Tensor:
        """Graphs with collated targets (``evaluate_stream``): ``node_first`` int64 [G + 1], ``node_targets`` fp32 [N, 6] =
        the batch's ``data.y``.  -> float64 [G, 16] on the device.  With ``fuse``, optional outputs: ``candidates`` float64
        [G, max_edges, 16] (every used candidate as a row) and ``counts`` int32 [G] (usable edges before the cut); with
        ``fuse="consensus"`` also ``inliers`` int32 [G, 2] = (supporters of the winning candidate, candidates used).  With
        ``weights``: ``rel_var`` fp32 [E, 6], the variances of ``rel_pose``'s rows (required), and the optional output ``spread``
        float64 [G, 2] = (sigma_t, sigma_q) of the fused pose."""
        return self._run(rel_pose, dict(edge_index=edge_index, node_first=node_first, node_targets=node_targets,
                                        edge_first=edge_first, out=out), candidates, counts, inliers, rel_var, spread)

    def from_map(self, rel_pose, edge_index, fmap, neighbours, query_targets=None, edge_first=None, out=None, candidates=None,
                 counts=None, inliers=None, rel_var=None, spread=None) -> torch.Tensor:
        """Graphs of the map path (``forward_map`` / ``relocalize``): graph g is query g followed by the rows ``neighbours[g]``
        of ``fmap``, whose ``poses`` are the database images' targets; ``query_targets`` fp32 [G, 6] are the queries' own (None:
        zeros, the rows' ``targ`` part and errors then mean nothing).  -> float64 [G, 16] on the device.  ``candidates`` /
        ``counts`` / ``inliers`` / ``rel_var`` / ``spread``: as in ``from_targets``."""
        poses = getattr(fmap, "poses", None)
        if poses is None:
            raise ValueError("QueryPose.from_map: the feature map holds no poses (build it with poses=...): a query's pose is "
                             "its database image's pose minus the predicted relative pose")
        return self._run(rel_pose, dict(edge_index=edge_index, map_poses=poses, neighbours=neighbours,
                                        query_targets=query_targets, edge_first=edge_first, out=out), candidates, counts, inliers,
                         rel_var, spread)

    def _run(self, rel_pose, kw, candidates=None, counts=None, inliers=None, rel_var=None, spread=None) -> torch.Tensor:
        if self.fuse is None and (candidates is not None or counts is not None):
            raise ValueError("QueryPose: candidates / counts are outputs of the fused rule (fuse='mean', 'median' or "
                             "'consensus')")
        if self.fuse != "consensus" and inliers is not None:
            raise ValueError(f"QueryPose: inliers is an output of fuse='consensus', this rule has fuse={self.fuse!r}")
        if self.weights is None and (rel_var is not None or spread is not None):
            raise ValueError("QueryPose: rel_var / spread belong to a weighted rule (weights='variance'), this rule has "
                             "weights=None")
        if torch.is_tensor(rel_pose) and rel_pose.is_cuda:      # (anything else is refused by ops.query_pose below)
            status = self._bad.tensor(rel_pose.device)
        else:
            status = self._bad.counters
        if status is None:
            status = torch.zeros(1, dtype=torch.int32)          # placeholder for the host-side checks, which refuse the call
        if self.fuse is None:
            rows = ops.query_pose(rel_pose, pose_m=self.pose_m, pose_s=self.pose_s, ref_node=self.ref_node, status=status, **kw)
        else:
            rows = ops.query_pose_fused(rel_pose, fuse=self.fuse, max_edges=self.max_edges, pose_m=self.pose_m, pose_s=self.pose_s,
                                        status=status, candidates=candidates, counts=counts, inlier_t=self.inlier_t,
                                        inlier_deg=self.inlier_deg, inliers=inliers, weights=self.weights, rel_var=rel_var,
                                        var_floor=self.var_floor, spread=spread, **kw)
        self._bad.publish()                       # the counter's copy to pinned memory, behind this call's kernel
        return rows

    # ---- bad graphs, without a host synchronisation (status.DeferredCounters) ----------------------------------------------
    def _error(self, counts: torch.Tensor) -> ValueError:
        if self.fuse is not None:
            return ValueError(f"graph has no edge into node 0: cannot derive the query pose ({int(counts[0])} graph(s) have no "
                              "usable edge into their query node, or a used edge's source lies outside the graph; detected on "
                              "the device, their rows are NaN)")
        return ValueError(f"graph has no edge into node 0: cannot derive the query pose ({int(counts[0])} graph(s) lack edge "
                          f"number {self.ref_node} into their query node, or its source lies outside the graph; detected on the "
                          "device, their rows are NaN)")

    def publish(self) -> None:
        """For callers that replay a captured launch (a replayed launch keeps counting on the device): enqueue the counter's
        copy behind the replay."""
        self._bad.publish()

    def check(self, wait: bool = True) -> None:
        """Raise the ValueError of ``evaluate.reference_edge`` if a call issued so far met a graph it could not evaluate.
        ``wait=True`` blocks until every call issued so far has reported, ``wait=False`` only looks at what has already arrived
        in the pinned mirror (``status.DeferredCounters.check``; the contract of ``PoseNetX_R2.check_edge_index``)."""
        self._bad.check(wait)
