"""Evaluation harness: the caller side of the hot path.

Restates what ``MultiModelTrainer.eval_RP`` does with the model outputs
(/root/reference/python/niantic/testing/test.py:180-286) so that the HIP module can be evaluated without the reference's
CLI: pick the reference edge of every graph, turn the predicted relative pose into the query's absolute pose, map the
log-quaternion back with ``qexp``, un-normalise the translation, accumulate translation / rotation errors, report
median and mean, and write the ``.npz`` the reference writes.  Differences by design: graphs are evaluated in
micro-batches (the reference uses batch_size=1, test.py:192; results per graph are independent of the batching), and the
stream can be sharded over ranks (``relpose_gnn_amd.shard``).  Host-side numpy in float64 like the reference.  The two
streams, ``evaluate_stream`` and ``relocalize``, are clients of the micro-batch pipeline in ``relpose_gnn_amd.pipeline``.
"""
from __future__ import annotations

import os
from collections import namedtuple
from dataclasses import dataclass
from typing import Iterable, List, Optional, Sequence

import numpy as np
import torch

from .graph import Data, fc_edge_index
# the fused rules' names, the consensus rule's default thresholds (which see there) and their check: one home for host and device
from .ops import FUSE_MODES, INLIER_DEG, INLIER_T, VAR_FLOOR, _qp_thresholds, _qp_weights  # noqa: F401  (re-exported)
from .pipeline import (_collate_on_device, _InputPipeline, _MicroBatchRunner, cut_per_graph,  # noqa: F401  (re-exported)
                       edges_per_graph, staging_workers)


def qexp(v: np.ndarray) -> np.ndarray:
    """Exponential map R^3 -> unit quaternion (w, x, y, z): [cos|v|, sin|v|/|v| * v]   (pose_utils.py:340-348)."""
    v = np.asarray(v, dtype=np.float64)
    n = np.linalg.norm(v)
    return np.hstack((np.cos(n), np.sinc(n / np.pi) * v))


def quaternion_angular_error(q1: np.ndarray, q2: np.ndarray) -> float:
    """Angle in degrees between two unit quaternions: 2 acos(|<q1,q2>|)   (pose_utils.py:420-431)."""
    d = abs(float(np.dot(np.asarray(q2, dtype=np.float64), np.asarray(q1, dtype=np.float64))))
    d = min(1.0, max(-1.0, d))
    return 2.0 * np.arccos(d) * 180.0 / np.pi


def reference_edge(edges: np.ndarray, ref_node: int = 0) -> int:
    """Index of the ``ref_node``-th edge whose target is node 0, the query (test.py:227-229).  For the stored 8-node
    fully-connected graphs this is column 28, the edge 1 -> 0."""
    hits = np.argwhere(np.asarray(edges)[1] == 0)
    if hits.shape[0] <= ref_node:
        raise ValueError("graph has no edge into node 0: cannot derive the query pose")
    return int(hits[ref_node, 0])


def query_pose(rel_pose: np.ndarray, target: np.ndarray, edges: np.ndarray, pose_m, pose_s, ref_node: int = 0):
    """(pred[7], targ[7]) = (t, q) of the query node of ONE graph (test.py:227-251): absolute = ground truth of the
    reference edge's source node minus the predicted relative pose; rotation through qexp; translation * std + mean."""
    rel_pose, target = np.asarray(rel_pose, dtype=np.float64), np.asarray(target, dtype=np.float64)
    ref = reference_edge(edges, ref_node)
    out = target[np.asarray(edges)[0, ref]] - rel_pose[ref]
    pred = np.hstack((out[:3] * pose_s + pose_m, qexp(out[3:])))
    targ = np.hstack((target[0, :3] * pose_s + pose_m, qexp(target[0, 3:])))
    return pred, targ


_NO_EDGE = "graph has no edge into node 0: cannot derive the query pose"       # reference_edge's message


def pose_candidates(rel_pose: np.ndarray, target: np.ndarray, edges: np.ndarray, pose_m, pose_s, max_edges: int = 64):
    """Every usable edge into node 0 of ONE graph as an estimate of the query's pose: -> (cands [C, 7], targ [7], count).  Usable:
    target 0 and a source that is not node 0 (a self-edge would carry the query's own target into its estimate); used: the first
    ``max_edges`` of them in column order; ``count``: how many there were before that cut.  Row c is ``query_pose`` over used
    edge c -- on a graph without self-edges ``query_pose(..., ref_node=c)``, bit for bit.  ValueError (``reference_edge``'s) for a
    graph without a usable edge or with a used edge whose source is not one of its nodes."""
    rel_pose, target, edges = np.asarray(rel_pose, dtype=np.float64), np.asarray(target, dtype=np.float64), np.asarray(edges)
    hits = np.flatnonzero((edges[1] == 0) & (edges[0] != 0))
    if hits.size == 0:
        raise ValueError(_NO_EDGE)
    used = hits[:max_edges]
    src = edges[0, used]
    if ((src < 0) | (src >= target.shape[0])).any():
        raise ValueError(_NO_EDGE + " (a used edge's source lies outside the graph)")
    cands = []
    for c, s in zip(used, src):
        out = target[s] - rel_pose[c]
        cands.append(np.hstack((out[:3] * pose_s + pose_m, qexp(out[3:]))))
    targ = np.hstack((target[0, :3] * pose_s + pose_m, qexp(target[0, 3:])))
    return np.stack(cands), targ, int(hits.size)


def medoid_angle_sums(q: np.ndarray) -> np.ndarray:
    """[C]: for every quaternion of q [C, 4] the sum of its angular errors to the others, added up in row order."""
    c = q.shape[0]
    sums = np.zeros(c)
    for i in range(c):
        acc = 0.0                                       # (an explicit loop: the order of the additions is part of the rule)
        for d in range(c):
            if d != i:
                acc = acc + quaternion_angular_error(q[i], q[d])
        sums[i] = acc
    return sums


def consensus_support(cands: np.ndarray, inlier_t: float = INLIER_T, inlier_deg: float = INLIER_DEG) -> np.ndarray:
    """bool [C, C]: whether candidates c and d of cands [C, 7] = (t, q) support each other.  A candidate with a non-finite
    component supports nothing and is supported by nothing; a finite one supports itself (by c == d, not by an angle test); two
    finite ones c != d support each other when ``sqrt((dx*dx + dy*dy) + dz*dz) <= inlier_t`` with d* = t_c - t_d, in that order
    of operations, and ``quaternion_angular_error(q_c, q_d) <= inlier_deg``.  Symmetric bit for bit: the squares and the
    products of the dot are the same numbers either way round."""
    inlier_t, inlier_deg = _qp_thresholds(inlier_t, inlier_deg, "consensus_support")
    cands = np.asarray(cands, dtype=np.float64)
    c = cands.shape[0]
    finite = np.isfinite(cands).all(axis=1)
    sup = np.zeros((c, c), dtype=bool)
    for i in range(c):
        if not finite[i]:
            continue
        for d in range(c):
            if d == i:
                sup[i, d] = True
            elif finite[d]:
                with np.errstate(over="ignore", invalid="ignore"):       # (finite translations can still be 1e308 apart)
                    dx, dy, dz = (float(v) for v in cands[i, :3] - cands[d, :3])
                    dist = np.sqrt((dx * dx + dy * dy) + dz * dz)
                sup[i, d] = bool(dist <= inlier_t) and quaternion_angular_error(cands[i, 3:], cands[d, 3:]) <= inlier_deg
    return sup


def consensus_inliers(cands: np.ndarray, inlier_t: float = INLIER_T, inlier_deg: float = INLIER_DEG):
    """-> (I, support [C]): ``support[c]`` = how many candidates support c (``consensus_support``; 0 for a non-finite one), the
    winner c* = the lowest c among those of largest support, and I = the slots of the candidates that support c*, ascending --
    empty when every support is 0, i.e. when every candidate is non-finite."""
    sup = consensus_support(cands, inlier_t, inlier_deg)
    support = sup.sum(axis=1).astype(np.int64)
    best = int(np.argmax(support))                          # argmax: the first of equals
    if support[best] == 0:
        return np.zeros(0, dtype=np.int64), support
    return np.flatnonzero(sup[best]), support


def fuse_poses(cands: np.ndarray, fuse: str, *, inlier_t: float = INLIER_T, inlier_deg: float = INLIER_DEG) -> np.ndarray:
    """cands [C, 7] = (t, q) -> the one pose [7] (float64; every sum in row order).
    ``"mean"``: t = (t_0 + .. + t_{C-1}) / C; q = S / |S| with S the sum of q_c where <q_c, q_0> >= 0 and of -q_c elsewhere (q and
    -q are one rotation), q_0 where |S| = 0.  ``"median"``: the component-wise median of t (``np.median``: the mean of the two
    middle values for even C) and the medoid q_c*, c* the lowest c that minimises ``medoid_angle_sums``.
    One candidate is returned as it is.  Two or more of which one has a non-finite component give NaN in every component, so
    that neither mode depends on how NaN orders.
    ``"consensus"``: ``fuse_poses(cands[I], "mean")`` with I the inliers of ``consensus_inliers`` under the two thresholds
    (``inlier_t`` in the unit of the un-normalised translation -- it is compared after ``* pose_s + pose_m`` --, ``inlier_deg`` in
    degrees; the defaults 0.25 / 5.0 are API defaults that belong to the scene's scale, not measured optima).  Here a non-finite
    candidate is an outlier and voids nothing, a lone candidate has no rule of its own, and NaN in every component means that
    every candidate was non-finite.  The thresholds are checked for every mode and read by this one."""
    return _fuse(cands, fuse, inlier_t, inlier_deg)[0]


def has_inlier_counts(fuse) -> bool:
    """Whether a rule reports, per graph, how many candidates it averaged and how many voted: the consensus rule alone."""
    return fuse == "consensus"


def _fuse(cands, fuse, inlier_t, inlier_deg, who: str = "fuse_poses"):
    """``fuse_poses`` with what it averaged: -> (pose [7], the slots I of ``consensus_inliers`` -- None for a rule without them)."""
    if fuse not in FUSE_MODES:
        raise ValueError(f"fuse must be 'mean', 'median' or 'consensus', got {fuse!r}")
    inlier_t, inlier_deg = _qp_thresholds(inlier_t, inlier_deg, who)
    cands = np.asarray(cands, dtype=np.float64)
    inl = None
    if has_inlier_counts(fuse):                             # the mean of the inliers, which are finite
        inl, _ = consensus_inliers(cands, inlier_t, inlier_deg)
        if not inl.size:
            return np.full(7, np.nan), inl
        cands, fuse = cands[inl], "mean"
    c = cands.shape[0]
    if c == 1:
        return cands[0].copy(), inl
    if not np.isfinite(cands).all():
        return np.full(7, np.nan), inl
    t, q = cands[:, :3], cands[:, 3:]
    if fuse == "median":
        return np.hstack((np.median(t, axis=0), q[int(np.argmin(medoid_angle_sums(q)))])), inl     # argmin: the first of equals
    st, sq = np.zeros(3), np.zeros(4)
    for d in range(c):
        st = st + t[d]
        dot = q[d, 0] * q[0, 0] + q[d, 1] * q[0, 1] + q[d, 2] * q[0, 2] + q[d, 3] * q[0, 3]
        sq = sq + q[d] if dot >= 0.0 else sq - q[d]
    norm = np.sqrt(sq[0] * sq[0] + sq[1] * sq[1] + sq[2] * sq[2] + sq[3] * sq[3])
    return np.hstack((st / c, q[0] if norm == 0.0 else sq / norm)), inl


def fused_query_pose(rel_pose: np.ndarray, target: np.ndarray, edges: np.ndarray, pose_m, pose_s, fuse: str, max_edges: int = 64, *,
                     inlier_t: float = INLIER_T, inlier_deg: float = INLIER_DEG):
    """(pred[7], targ[7]) of the query node of ONE graph from ALL its usable reference edges (``pose_candidates``) combined by
    ``fuse_poses``: ``query_pose`` keeps one of these estimates, this is the rule that uses them all.  The host path of
    ``fuse=`` in the two streams and the statement the device kernel (rpg_query_pose_fused_f64, and for ``"consensus"`` with
    its thresholds rpg_query_pose_consensus_f64) is held to."""
    cands, targ, _ = pose_candidates(rel_pose, target, edges, pose_m, pose_s, max_edges)
    return fuse_poses(cands, fuse, inlier_t=inlier_t, inlier_deg=inlier_deg), targ


def fused_query_row(rel_pose, target, edges, pose_m, pose_s, fuse: str, max_edges: int = 64, *, inlier_t: float = INLIER_T,
                    inlier_deg: float = INLIER_DEG) -> np.ndarray:
    """The device rule's row of 16 = pred[7], targ[7], translation error, rotation error for ONE graph.  The errors are
    ``errors`` of the fused pose, except that a pose voided by a non-finite candidate (two or more candidates; with
    ``"consensus"``: a pose without a single finite candidate behind it) has NaN for both -- the rotation error of a NaN
    quaternion would be 360 by the reference's clamp."""
    return _fused_row(rel_pose, target, edges, pose_m, pose_s, fuse, max_edges, inlier_t, inlier_deg)[0]


def consensus_query_row(rel_pose, target, edges, pose_m, pose_s, max_edges: int = 64, *, inlier_t: float = INLIER_T,
                        inlier_deg: float = INLIER_DEG):
    """``fused_query_row(..., fuse="consensus")`` with the two integers that say how far the pose can be believed: -> (row [16],
    inliers, used).  ``used`` = min(usable edges, max_edges) candidates voted, ``inliers`` of them support the winner and are
    averaged into the pose; ``inliers / used`` is the caller's confidence, ``inliers == 0`` a row whose pose and errors are NaN
    because every used candidate was non-finite.  (A graph without a usable edge raises, as in ``pose_candidates``.)"""
    return _fused_row(rel_pose, target, edges, pose_m, pose_s, "consensus", max_edges, inlier_t, inlier_deg, "consensus_support")


def _fused_row(rel_pose, target, edges, pose_m, pose_s, fuse, max_edges, inlier_t, inlier_deg, who: str = "fuse_poses"):
    """ONE graph under a fused rule, its candidates made once and its inliers found at most once: -> (row [16], inliers, used),
    ``inliers`` None for a rule without them (``has_inlier_counts``)."""
    cands, targ, _ = pose_candidates(rel_pose, target, edges, pose_m, pose_s, max_edges)
    pred, inl = _fuse(cands, fuse, inlier_t, inlier_deg, who)
    with np.errstate(invalid="ignore"):
        r = errors(pred[None], targ[None])
    t_err, q_err = r.t_loss[0], r.q_loss[0]
    if (cands.shape[0] > 1 or inl is not None) and np.isnan(pred).any():
        t_err = q_err = np.nan
    return np.hstack((pred, targ, t_err, q_err)), None if inl is None else int(inl.size), int(cands.shape[0])


# ---- the fused rules weighted by the edges' Monte-Carlo variance -------------------------------------------------------------
def used_columns(edges: np.ndarray, max_edges: int = 64) -> np.ndarray:
    """The columns ``pose_candidates`` makes its candidates from, in its order: target 0, source not 0, the first ``max_edges``."""
    edges = np.asarray(edges)
    return np.flatnonzero((edges[1] == 0) & (edges[0] != 0))[:max_edges]


def variance_weights(var: np.ndarray, var_floor: float = VAR_FLOOR):
    """var [C, 6] (the candidates' rows of ``rel_var``, read as float64) -> (w [C, 3], wq [C], usable bool [C]): the translation
    weights ``w_cj = 1.0 / (v_c[j] + var_floor)`` per component, the rotation weight ``wq_c = 1.0 / (((v_c[3] + v_c[4]) + v_c[5]) +
    var_floor)`` in that order of additions, and whether the variance can be used: none of its six values NaN, negative or +inf
    (the weights of an unusable one are never read)."""
    var = np.asarray(var, dtype=np.float64).reshape(-1, 6)
    with np.errstate(all="ignore"):
        usable = ~(np.isnan(var) | (var < 0.0) | (var == np.inf)).any(axis=1)
        w = 1.0 / (var[:, :3] + var_floor)
        wq = 1.0 / (((var[:, 3] + var[:, 4]) + var[:, 5]) + var_floor)
    return w, wq, usable


def pose_spread(sw, swq, pose_s) -> np.ndarray:
    """(sigma_t, sigma_q) of a pose fused with the weight sums W [3] and Wq: ``sqrt((s_0 s_0 / W_0 + s_1 s_1 / W_1) + s_2 s_2 /
    W_2)`` with s = ``pose_s``, the predicted standard deviation of the translation in the un-normalised unit, and ``sqrt(1.0 /
    Wq)``, that of the rotation in log-quaternion units."""
    s = np.asarray(pose_s, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.array([np.sqrt((s[0] * s[0] / sw[0] + s[1] * s[1] / sw[1]) + s[2] * s[2] / sw[2]), np.sqrt(1.0 / swq)])


def weighted_mean(cands: np.ndarray, w: np.ndarray, wq: np.ndarray):
    """The weighted form of ``fuse_poses(cands, "mean")`` over two or more finite candidates: -> (pose [7], W [3], Wq).  Every sum
    sequential in row order: ``t_j = (sum_c w_cj t_cj) / W_j`` with ``W_j = sum_c w_cj``; ``q = S / |S|`` with S the sum of ``wq_c
    q_c`` where <q_c, q_0> >= 0 and of ``-wq_c q_c`` elsewhere, ``q_0`` where |S| = 0; ``Wq = sum_c wq_c``."""
    t, q = cands[:, :3], cands[:, 3:]
    st, sw, sq, swq = np.zeros(3), np.zeros(3), np.zeros(4), 0.0
    with np.errstate(all="ignore"):
        for d in range(cands.shape[0]):
            st = st + w[d] * t[d]
            sw = sw + w[d]
            dot = q[d, 0] * q[0, 0] + q[d, 1] * q[0, 1] + q[d, 2] * q[0, 2] + q[d, 3] * q[0, 3]
            sq = sq + wq[d] * q[d] if dot >= 0.0 else sq - wq[d] * q[d]
            swq = swq + wq[d]
        norm = np.sqrt(sq[0] * sq[0] + sq[1] * sq[1] + sq[2] * sq[2] + sq[3] * sq[3])
        return np.hstack((st / sw, q[0] if norm == 0.0 else sq / norm)), sw, swq


def fuse_poses_weighted(cands: np.ndarray, var: np.ndarray, fuse: str, pose_s=(1.0, 1.0, 1.0), *, inlier_t: float = INLIER_T,
                        inlier_deg: float = INLIER_DEG, var_floor: float = VAR_FLOOR):
    """``fuse_poses`` for ``fuse="mean"`` / ``"consensus"`` with every candidate weighted by the inverse of its variance: cands
    [C, 7], var [C, 6] (candidate c's row of ``rel_var``: the variance of ONE dropout sample of its relative pose) -> (pose [7],
    spread [2] = ``pose_spread`` over the same candidates, the inlier slots -- None for ``"mean"``).

    The weights are ``variance_weights``; the slot set I is all C candidates for ``"mean"`` and ``consensus_inliers`` for
    ``"consensus"``, whose voting is unchanged and unweighted -- except that a candidate with an unusable variance is treated
    like a non-finite one there: it supports nothing and is supported by nothing.  Over two or more slots the pose is
    ``weighted_mean``; one slot is returned as it is, with its own weights as W and Wq.  ``"mean"`` with C >= 2 and a non-finite
    candidate or an unusable variance gives NaN in every component, as today's ``"mean"`` does for the former.  The spread is
    NaN wherever a component of the pose is, and for C = 1 under ``"mean"`` with an unusable variance.  When every ``v +
    var_floor`` is the same power of two the pose is ``fuse_poses(cands, fuse)`` bit for bit: scaling by a power of two commutes
    with every operation here.  ``var_floor``: finite, >= 1e-30; 1e-12 is an API default, not a tuned value."""
    _, var_floor = _qp_weights("variance", fuse, var_floor, "fuse_poses_weighted")
    inlier_t, inlier_deg = _qp_thresholds(inlier_t, inlier_deg, "fuse_poses_weighted")
    cands = np.asarray(cands, dtype=np.float64)
    w, wq, usable = variance_weights(var, var_floor)
    nan7, nan2 = np.full(7, np.nan), np.full(2, np.nan)
    inl = None
    if has_inlier_counts(fuse):
        voters = cands.copy()
        voters[~usable] = np.nan
        inl, _ = consensus_inliers(voters, inlier_t, inlier_deg)
        if not inl.size:
            return nan7, nan2, inl
        cands, w, wq, usable = cands[inl], w[inl], wq[inl], usable[inl]
    if cands.shape[0] == 1:
        pose, spread = cands[0].copy(), pose_spread(w[0], wq[0], pose_s) if usable[0] else nan2
    elif not (np.isfinite(cands).all() and usable.all()):
        pose, spread = nan7, nan2
    else:
        pose, sw, swq = weighted_mean(cands, w, wq)
        spread = pose_spread(sw, swq, pose_s)
    return pose, nan2 if np.isnan(pose).any() else spread, inl


def weighted_query_row(rel_pose, rel_var, target, edges, pose_m, pose_s, fuse: str, max_edges: int = 64, *,
                       inlier_t: float = INLIER_T, inlier_deg: float = INLIER_DEG, var_floor: float = VAR_FLOOR):
    """ONE graph under a weighted rule: -> (row [16], spread [2], inliers -- None for ``"mean"`` --, used).  The candidates, the
    cut at ``max_edges``, the row layout, the errors and the two integers are those of ``fused_query_row`` /
    ``consensus_query_row``; ``rel_var`` [E, 6] is read at the candidates' columns (``used_columns``) and the pose and the spread
    are ``fuse_poses_weighted``.  The statement the device kernel (rpg_query_pose_weighted_f64) is held to, and the host path
    of ``weights="variance"`` in the two streams."""
    cands, targ, _ = pose_candidates(rel_pose, target, edges, pose_m, pose_s, max_edges)
    var = np.asarray(rel_var, dtype=np.float64)[used_columns(edges, max_edges)]
    pred, spread, inl = fuse_poses_weighted(cands, var, fuse, pose_s, inlier_t=inlier_t, inlier_deg=inlier_deg, var_floor=var_floor)
    with np.errstate(invalid="ignore"):
        r = errors(pred[None], targ[None])
    t_err, q_err = r.t_loss[0], r.q_loss[0]
    if (cands.shape[0] > 1 or inl is not None) and np.isnan(pred).any():
        t_err = q_err = np.nan
    return np.hstack((pred, targ, t_err, q_err)), spread, None if inl is None else int(inl.size), int(cands.shape[0])


@dataclass
class EvalResult:
    pred_poses: np.ndarray      # [G, 7]
    targ_poses: np.ndarray      # [G, 7]
    t_loss: np.ndarray          # [G] metres
    q_loss: np.ndarray          # [G] degrees
    inliers: Optional[np.ndarray] = None     # [G] int, fuse="consensus" only: the candidates averaged into the pose
    used: Optional[np.ndarray] = None        # [G] int, fuse="consensus" only: the candidates that voted; inliers / used = confidence
    sigma_t: Optional[np.ndarray] = None     # [G] float, weights="variance" only: predicted deviation of the fused translation
    sigma_q: Optional[np.ndarray] = None     # [G] float, weights="variance" only: that of the rotation, in log-quaternion units
    gate_state: Optional[np.ndarray] = None  # [G] int, relocalize(priors=, gate=) only: 0 gated, 1 no prior, 2 fell back to the whole map
    scene: Optional[np.ndarray] = None       # [G] int, relocalize(scenes=SceneVote) only: the scene every query elected (-1: none)
    scene_votes: Optional[np.ndarray] = None # [G] int, ... and the votes it was elected with

    @property
    def median_t(self) -> float:
        return float(np.median(self.t_loss))

    @property
    def median_q(self) -> float:
        return float(np.median(self.q_loss))

    def summary(self):
        """(median_t, mean_t, median_q, mean_q): the tuple eval_RP returns (test.py:286)."""
        return self.median_t, float(np.mean(self.t_loss)), self.median_q, float(np.mean(self.q_loss))


def errors(pred_poses: np.ndarray, targ_poses: np.ndarray) -> EvalResult:
    t_loss = np.asarray([np.linalg.norm(p - t) for p, t in zip(pred_poses[:, :3], targ_poses[:, :3])])
    q_loss = np.asarray([quaternion_angular_error(p, t) for p, t in zip(pred_poses[:, 3:], targ_poses[:, 3:])])
    return EvalResult(pred_poses, targ_poses, t_loss, q_loss)


class _PoseRows:
    """What a stream collects micro-batch by micro-batch, and the result made of it: the [G, 16] blocks of the device pose
    rule (``pose``, the stream's ``QueryPose``), or the (pred, targ) rows of the host rule of test.py:213-251.  With ``fuse`` the
    host rule is ``_fused_row`` and collects the same [G, 16] blocks as the device.  A rule with inlier counts
    (``has_inlier_counts``) adds an int [G, 2] block of (inliers, used) to every block (``ints``), a weighted rule a float [G, 2]
    block of (sigma_t, sigma_q) (``spreads``), on either path."""

    def __init__(self, pose_m, pose_s, ref_node: int, pose=None, fuse=None, max_edges: int = 64,
                 inlier_t: float = INLIER_T, inlier_deg: float = INLIER_DEG, weights=None, var_floor: float = VAR_FLOOR):
        self.pose_m, self.pose_s = np.asarray(pose_m, dtype=np.float64), np.asarray(pose_s, dtype=np.float64)
        self.ref_node, self.pose = ref_node, pose
        self.fuse, self.max_edges = fuse, max_edges
        self.inlier_t, self.inlier_deg = inlier_t, inlier_deg
        self.weights, self.var_floor = weights, var_floor
        self.ints: Optional[List[np.ndarray]] = [] if has_inlier_counts(fuse) else None
        self.spreads: Optional[List[np.ndarray]] = [] if weights is not None else None
        self.rows: Optional[List[np.ndarray]] = [] if pose is not None or fuse is not None else None
        self.preds: List[np.ndarray] = []
        self.targs: List[np.ndarray] = []

    def add_device(self, block: np.ndarray) -> None:
        """One micro-batch as the device rule sent it: the host copy of its output block (``QueryPose.output_block``)."""
        rows, ints, spread = self.pose.cut_block(block)
        if ints is not None:
            self.ints.append(ints)
        if spread is not None:
            self.spreads.append(spread)
        self.rows.append(rows)

    def add(self, rel: np.ndarray, targets: Iterable, cut: Iterable, var: Optional[np.ndarray] = None) -> None:
        """The host rule over one micro-batch: per graph its targets [n, 6] and its (columns of ``rel``, local edge list); a
        weighted rule also reads ``var``, the variances of ``rel``'s rows."""
        if self.weights is not None:
            got = [weighted_query_row(rel[cols], var[cols], target, edges, self.pose_m, self.pose_s, self.fuse, self.max_edges,
                                      inlier_t=self.inlier_t, inlier_deg=self.inlier_deg, var_floor=self.var_floor)
                   for target, (cols, edges) in zip(targets, cut)]
            if got:
                self.rows.append(np.stack([row for row, _, _, _ in got]))
                self.spreads.append(np.stack([spread for _, spread, _, _ in got]))
                if self.ints is not None:
                    self.ints.append(np.asarray([[inl, used] for _, _, inl, used in got], dtype=np.int64))
            return
        if self.fuse is not None:
            got = [_fused_row(rel[cols], target, edges, self.pose_m, self.pose_s, self.fuse, self.max_edges, self.inlier_t,
                              self.inlier_deg) for target, (cols, edges) in zip(targets, cut)]
            if got:
                self.rows.append(np.stack([row for row, _, _ in got]))
                if self.ints is not None:
                    self.ints.append(np.asarray([[inl, used] for _, inl, used in got], dtype=np.int64))
            return
        for target, (cols, edges) in zip(targets, cut):
            p, t = query_pose(rel[cols], target, edges, self.pose_m, self.pose_s, self.ref_node)
            self.preds.append(p)
            self.targs.append(t)

    def result(self, gather=None, with_targets: bool = True):
        """EvalResult of everything collected (``gather(pred, targ, ints, spread)``: all ranks' rows in place of this rank's);
        without targets only the predicted poses [G, 7].  ``ints`` is None or, with ``fuse="consensus"``, the int64 [G, 2] block of
        (inliers, used): it fills the result's two arrays, and without targets it is what ``self.integers()`` hands out.
        ``spread`` likewise: None or a weighted rule's float64 [G, 2] block of (sigma_t, sigma_q), ``self.spread()``."""
        all_rows = None
        if self.rows is not None:
            all_rows = np.concatenate(self.rows) if self.rows else np.zeros((0, 16))
            pred, targ = all_rows[:, :7], all_rows[:, 7:14]
        else:
            pred = np.stack(self.preds) if self.preds else np.zeros((0, 7))
            targ = np.stack(self.targs) if self.targs else np.zeros((0, 7))
        if not with_targets:
            return np.ascontiguousarray(pred)
        ints, spread = self.integers(), self.spread()
        if gather is not None:
            pred, targ, ints, spread = gather(pred, targ, ints, spread)
            res = errors(pred, targ)
        else:
            res = _result_from_rows(all_rows) if all_rows is not None else errors(pred, targ)
        if ints is not None:
            res.inliers, res.used = ints[:, 0].copy(), ints[:, 1].copy()
        if spread is not None:
            res.sigma_t, res.sigma_q = spread[:, 0].copy(), spread[:, 1].copy()
        return res

    def spread(self) -> Optional[np.ndarray]:
        """float64 [G, 2] = (sigma_t, sigma_q) of everything collected; None unless the rule is weighted."""
        if self.spreads is None:
            return None
        return np.concatenate(self.spreads).astype(np.float64) if self.spreads else np.zeros((0, 2))

    def integers(self) -> Optional[np.ndarray]:
        """int64 [G, 2] = (inliers, used) of everything collected; None unless ``fuse="consensus"``."""
        if self.ints is None:
            return None
        return np.concatenate(self.ints).astype(np.int64) if self.ints else np.zeros((0, 2), dtype=np.int64)


@torch.no_grad()
def evaluate_stream(model, graphs: Sequence[Data], device, micro_batch: int = 64, pose_m=(0.0, 0.0, 0.0),
                    pose_s=(1.0, 1.0, 1.0), ref_node: int = 0, rank: int = 0, world: int = 1,
                    stats: Optional[dict] = None, bf16_input: Optional[bool] = None, postprocess: str = "host",
                    fuse: Optional[str] = None, max_edges: int = 64, inlier_t: float = INLIER_T,
                    inlier_deg: float = INLIER_DEG, weights: Optional[str] = None, var_floor: float = VAR_FLOOR) -> EvalResult:
    """Run ``model`` over a stream of single-graph ``Data`` objects (x, edge_index, y) and post-process like test.py.
    With world > 1 every rank evaluates its contiguous block (shard_range) and the [G,7] rows are all-gathered.

    The loop is a three-stage software pipeline: while the GPU runs the forward of micro-batch i, the host collates
    micro-batch i+1 into pinned memory and the copy stream sends it (``pipeline._InputPipeline``; graphs that already live on
    the device are collated there instead), and once both are enqueued the host post-processes micro-batch i-1, whose relative
    poses have come back through an asynchronous copy -- so neither the H2D transfer of the images (537 MB per 64 graphs
    at 256x341), nor the D2H of the poses, nor the numpy work of test.py:213-251 leaves the GPU idle.
    ``stats`` (optional dict) receives ``h2d_bytes`` (bytes sent through the input pipeline), ``staged_bytes`` (of those: copied pageable -> pinned
    by the staging threads), ``direct_bytes`` (sent straight out of the caller's pinned tensors), ``staging_workers``, ``micro_batches`` and
    ``local_seconds`` (this rank's block, before the all-gather).  ``bf16_input`` (default: whatever the model
    accepts, i.e. True for the bf16 encoder with its fused stem): host-resident images are rounded to bf16 while they are staged --
    except, by default, micro-batches whose fp32 images all sit in PINNED memory (the reference's loader, test.py:193): those are sent
    as they are, with no host pass at all (``bf16_input=True`` forces the rounding pass for them too).  Same poses either way:
    the bf16 encoder rounds fp32 input first thing.
    Graphs whose ``x`` is uint8 camera frames ``[n, H, W, 3]`` (one size per micro-batch) are sent as uint8 -- pinned sources
    straight from where they are, pageable ones through the staging threads as a plain copy -- and the model's
    ``frame_transform`` (frames.FrameTransform) runs the reference's image transform on the device; the byte counts in ``stats``
    are then uint8 bytes.

    ``postprocess``: ``"host"`` (default) copies every micro-batch's relative poses [E, 6] (and a model-built edge list) back and
    applies the pose rule of test.py:213-267 in numpy, graph by graph.  ``"device"`` (GPU only) runs it as one kernel behind the
    forward (``query_pose.QueryPose``: float64 on the fp32 outputs, the targets ``y`` taken as fp32) and copies 16 doubles per
    graph back; the ``EvalResult`` is filled from those rows (under ``world > 1`` the gathered poses go through ``errors`` as
    before).  ``stats`` also receives ``postprocess`` and ``d2h_bytes`` (the payload copied back).

    ``fuse``: None (default) derives the query's pose from the ``ref_node``-th edge into it, as the reference does.  ``"mean"``
    / ``"median"`` combine the estimates of ALL the edges into it (the first ``max_edges`` <= 64 in column order, self-edges
    skipped; ``fused_query_pose``): with ``postprocess="host"`` in numpy, with ``"device"`` in the fused kernel
    (``QueryPose(fuse=...)``), still 16 doubles per graph back.  ``ref_node`` must stay 0 then.

    ``fuse="consensus"`` lets those estimates vote (``consensus_inliers``): two support each other when their translations lie
    within ``inlier_t`` and their rotations within ``inlier_deg`` degrees, the best-supported one wins and the pose is the
    ``"mean"`` of its supporters alone -- a wrong edge is outvoted instead of averaged in.  The result's ``inliers`` and ``used``
    (int [G]; None for every other mode) say how many estimates were averaged and how many voted: ``inliers / used`` is the
    accept / reject signal that goes with the pose.  On the device path the two integers travel with the rows, 8 more bytes per
    graph (``stats["d2h_bytes"]`` counts them); under ``world > 1`` they are gathered in graph order like the poses.  The
    defaults 0.25 / 5.0 are API defaults, not measured optima: both belong to the scene's scale, and ``inlier_t`` is compared
    after ``* pose_s + pose_m``, i.e. in the unit of the un-normalised translation.  Both must be finite, ``inlier_t >= 0``
    and ``0 <= inlier_deg <= 360`` (ValueError).

    ``weights="variance"`` (default None; with ``fuse="mean"`` or ``"consensus"``, ValueError otherwise): the mean of those
    rules weighs every estimate by the inverse of its Monte-Carlo variance, ``1 / (v + var_floor)`` (``fuse_poses_weighted``),
    so an edge the network is unsure of pulls less, and every graph gets the predicted standard deviation of its fused pose: the
    result's ``sigma_t`` (un-normalised unit of the translation) and ``sigma_q`` (log-quaternion units; ``2 * sigma_q`` radians
    is approximately the rotation angle's deviation), float [G], None for every other mode.  It needs ``model.mc_dropout`` with
    ``samples >= 2`` (ValueError before anything is queued): the variances are ``model.mc_dropout.last.rel_var``, those of ONE
    dropout sample, so the spread is the predictive deviation, not that of the S-sample mean.  The host path reads them back
    with the relative poses; the device path hands them to the kernel and 16 more bytes per graph come back
    (``stats["d2h_bytes"]``: 144 per graph for ``"mean"``, 152 for ``"consensus"``); under ``world > 1`` the two ride in the
    gathered rows like the integers.  ``var_floor`` (finite, >= 1e-30, checked always): 1e-12 is an API default, not a tuned
    value.  Whether ``sigma_t`` orders right and wrong poses on a dataset has not been measured."""
    from .shard import rank_host_slice
    _check_postprocess("evaluate_stream", postprocess, device)
    _check_fuse("evaluate_stream", fuse, max_edges, ref_node, inlier_t, inlier_deg)
    weights, var_floor = _check_weights("evaluate_stream", model, weights, fuse, var_floor)
    if world > 1 and torch.device(device).type == "cuda":
        # one process per GPU on a shared host: this rank's staging threads and pinned buffers stay on its share of the
        # cores / its GPU's NUMA node for the duration of the call (shard.rank_host_slice puts the caller's mask back on
        # return; a process its entry script has bound already is left as it is; RPG_BIND_RANKS=0 switches it off).  LOCAL_*
        # from the launcher when it set them (ranks of other nodes do not share this host)
        local_world = int(os.environ.get("LOCAL_WORLD_SIZE", world))
        with rank_host_slice(int(os.environ.get("LOCAL_RANK", rank)), local_world, torch.device(device).index):
            return _evaluate_stream(model, graphs, device, micro_batch, pose_m, pose_s, ref_node, rank, world, stats, bf16_input, local_world,
                                    postprocess, fuse, max_edges, inlier_t, inlier_deg, weights, var_floor)
    return _evaluate_stream(model, graphs, device, micro_batch, pose_m, pose_s, ref_node, rank, world, stats, bf16_input, 1, postprocess,
                            fuse, max_edges, inlier_t, inlier_deg, weights, var_floor)


def _check_postprocess(who: str, postprocess, device) -> None:
    if postprocess not in ("host", "device"):
        raise ValueError(f"{who}: postprocess must be 'host' or 'device', got {postprocess!r}")
    if postprocess == "device" and torch.device(device).type != "cuda":
        raise ValueError(f"{who}: postprocess='device' runs the pose rule on the GPU, the stream's device is {device}")


def _check_fuse(who: str, fuse, max_edges, ref_node, inlier_t=INLIER_T, inlier_deg=INLIER_DEG) -> None:
    _qp_thresholds(inlier_t, inlier_deg, who)
    if fuse is None:
        return
    if fuse not in FUSE_MODES:
        raise ValueError(f"{who}: fuse must be None, 'mean', 'median' or 'consensus', got {fuse!r}")
    if isinstance(max_edges, bool) or not isinstance(max_edges, (int, np.integer)) or not 1 <= max_edges <= 64:
        raise ValueError(f"{who}: max_edges must be an int in 1..64, got {max_edges!r}")
    if ref_node != 0:
        raise ValueError(f"{who}: fuse={fuse!r} combines every edge into the query node, ref_node={ref_node} selects one: give "
                         "one of the two")


def _check_weights(who: str, model, weights, fuse, var_floor):
    """``weights`` / ``var_floor`` of a stream, checked before anything is queued: -> (weights, var_floor as a float)."""
    weights, var_floor = _qp_weights(weights, fuse, var_floor, who)
    if weights is not None:
        mc = getattr(model, "mc_dropout", None)
        if mc is None or mc.samples < 2:
            raise ValueError(f"{who}: weights={weights!r} reads the Monte-Carlo variances of the relative poses: set "
                             "model.mc_dropout = McDropout(samples >= 2) (one sample has no variance)")
    return weights, var_floor


# what relocalize's forward hands to its read-back: forward_map's outputs, the neighbours on the device, the retrieved ones on
# their way to the host (None: they were given), and the pose rule's output block where a captured step has already filled it
_Forward = namedtuple("_Forward", "abs_pose rel_pose edge_index neighbours host_neighbours back gate_info scene_info",
                      defaults=(None, None, None, None))


def _result_from_rows(rows: np.ndarray) -> EvalResult:
    """EvalResult of the device pose rule's rows [G, 16] = pred[7], targ[7], t_err, q_err."""
    return EvalResult(np.ascontiguousarray(rows[:, :7]), np.ascontiguousarray(rows[:, 7:14]), rows[:, 14].copy(), rows[:, 15].copy())


def _evaluate_stream(model, graphs, device, micro_batch, pose_m, pose_s, ref_node, rank, world, stats, bf16_input, local_world,
                     postprocess="host", fuse=None, max_edges=64, inlier_t=INLIER_T, inlier_deg=INLIER_DEG, weights=None,
                     var_floor=VAR_FLOOR):
    from .shard import gather_rows, shard_counts, shard_range
    qp = None
    if postprocess == "device":
        from .query_pose import QueryPose
        qp = QueryPose(pose_m, pose_s, ref_node, fuse=fuse, max_edges=max_edges, inlier_t=inlier_t, inlier_deg=inlier_deg,
                       weights=weights, var_floor=var_floor)
    lo, hi = shard_range(len(graphs), rank, world)
    acc = _PoseRows(pose_m, pose_s, ref_node, pose=qp, fuse=fuse, max_edges=max_edges, inlier_t=inlier_t,
                    inlier_deg=inlier_deg, weights=weights, var_floor=var_floor)
    # the host rule of a weighted stream reads the variances too: they come back with the relative poses
    runner = _MicroBatchRunner(model, device, micro_batch, bf16_input, local_world, pose=qp,
                               want_var=weights is not None and qp is None)

    def finish(item):
        chunk, host = item.chunk, item.host
        if qp is not None:
            return acc.add_device(host["rel"].numpy())
        ei = None if host["ei"] is None else host["ei"].numpy()              # a model-built (kNN) edge list
        acc.add(host["rel"].numpy(), (g.y.cpu().numpy() for g in chunk),
                cut_per_graph([g.num_nodes for g in chunk], ei, (g.edge_index.cpu().numpy() for g in chunk)),
                None if host.get("var") is None else host["var"].numpy())

    def chunk_at(i):
        return [graphs[j] for j in range(lo + i * micro_batch, min(hi, lo + (i + 1) * micro_batch))]

    runner.run(len(range(lo, hi, micro_batch)), chunk_at, finish, stats, postprocess)   # local_seconds: this rank's own block, before the all-gather
    import torch.distributed as dist
    grouped = dist.is_available() and dist.is_initialized() and dist.get_world_size() == world
    if grouped and world == 1:
        # world size 1: only where the group's backend can take this device's tensors (an NCCL group cannot all-gather the CPU
        # tensors of a device="cpu" run -- ADVICE r5; before round 5 world = 1 never reached a collective)
        grouped = torch.device(device).type == "cuda" or dist.get_backend() != "nccl"

    def gather(pred, targ, ints=None, spread=None):
        # under a process group the collective runs at ANY world size, 1 included: a one-GPU box then executes the same RCCL
        # all-gather the 4- / 8-GPU stream does (tools/eval_stream.py under torch.distributed.run).  The consensus rule's two
        # integers ride in the same rows as two more float64 columns (small integers: exact), so they arrive in graph order too;
        # a weighted rule's two deviations ride behind them in the same way
        parts = [pred, targ] + ([] if ints is None else [ints.astype(np.float64)]) + ([] if spread is None else [spread])
        both = torch.from_numpy(np.concatenate(parts, 1)).to(device)
        both = gather_rows(both, shard_counts(len(graphs), world), always=True).cpu().numpy()
        at = 14 if ints is None else 16
        return (both[:, :7], both[:, 7:14], None if ints is None else both[:, 14:16].astype(np.int64),
                None if spread is None else both[:, at:at + 2])
    return acc.result(gather if world > 1 or grouped else None)


def seven_scenes_rel_paths(file_list: Sequence, dataset_filenames: Sequence, dataset_dir) -> List[str]:
    """The ``rel_path`` column eval_RP records for 7-Scenes (test.py:255-260): graph file ``data_<linear id>.pt`` ->
    ``dataset_filenames[linear id]`` (the colour frames of the TestSplit sequences in order, test.py:103-114) relative to
    the dataset directory."""
    out = []
    for fname in file_list:
        stem = os.path.splitext(os.path.basename(str(fname)))[0]
        linear_id = int(stem.split("_")[-1])
        out.append(os.path.relpath(str(dataset_filenames[linear_id]), str(dataset_dir)))
    return out


def save_poses(path, result: EvalResult, rel_paths: Iterable) -> None:
    """The .npz of test.py:38-42 (same field names, same length assertion).  ``rel_paths``: one entry per graph, for
    7-Scenes ``seven_scenes_rel_paths(...)``."""
    rel_paths = [str(p) for p in rel_paths]
    assert len(rel_paths) == len(result.pred_poses), \
        f"len(rel_paths): {len(rel_paths)} != {len(result.pred_poses)} len(pred_poses)"
    np.savez(path, rel_path=rel_paths, abs_t=result.pred_poses[:, :3], abs_q=result.pred_poses[:, 3:],
             targ_t=result.targ_poses[:, :3], targ_q=result.targ_poses[:, 3:])


def load_pose_stats(path):
    """Cambridge translation mean / std file, two rows of three numbers (test.py:126-130)."""
    m, s = np.loadtxt(path)
    return m, s


@torch.no_grad()
def relocalize(model, fmap, queries: torch.Tensor, neighbours=None, micro_batch: int = 64, pose_m=(0.0, 0.0, 0.0),
               pose_s=(1.0, 1.0, 1.0), ref_node: int = 0, stats: Optional[dict] = None, targets=None,
               bf16_input: Optional[bool] = None, *, rule=None, query_descriptors=None, query_groups=None,
               postprocess: str = "host", fuse: Optional[str] = None, max_edges: int = 64, capture: bool = False,
               outputs: str = "all", inlier_t: float = INLIER_T, inlier_deg: float = INLIER_DEG,
               weights: Optional[str] = None, var_floor: float = VAR_FLOOR, priors=None, gate=None, scenes=None):
    """The evaluation stream of the map path (``PoseNetX_R2.forward_map``): query g's graph is the query followed by the map
    rows ``neighbours[g]`` (its retrieved database images, dataset_7Scenes_multi.py:340-345).  Single process.

    ``queries``: [G, ...] images as ``forward_map`` takes them (processed fp32 / bf16, or uint8 frames), on the host or on the
    map's GPU; ``neighbours``: int64 [G, K].  Only the queries cross the host link, through the pipeline of
    ``evaluate_stream`` (pinned sources go out directly, pageable ones are staged, bf16 rounding by the same rules), micro-batch
    i + 1 staged while micro-batch i runs and micro-batch i - 1 is post-processed.  A map that is not on a GPU takes that
    pipeline's synchronous path without staging, as ``evaluate_stream`` on ``device="cpu"`` does.

    Returns, per query, the predicted pose [G, 7] by the rule of test.py:227-251 (``query_pose``), the "target" of the
    reference edge's source node being ``fmap.poses[neighbours[g][src - 1]]``; with ``targets`` ([G, 6], the queries' own
    ``[t, log q]``) an ``EvalResult`` instead (its ``pred_poses`` are those poses).  A map without poses gives the raw
    ``(abs_pose [G*(K+1), 6], rel_pose [E, 6])`` host tensors.  ``stats`` as in ``evaluate_stream``.

    ``neighbours=None`` with a ``rule`` (retrieval.RetrievalRule) retrieves them on the GPU inside ``forward_map`` (which see
    for ``query_descriptors`` [G, Dd] -- host or device, staged per micro-batch -- and ``query_groups`` [G], host integers): the
    neighbours of micro-batch i come back to the host with its poses, by the same pinned non-blocking copy behind the same
    event.  The chosen rows, int64 [G, K], are left in ``stats["neighbours"]`` and on an ``EvalResult`` as ``.neighbours``.

    ``gate`` (retrieval.PoseGate) with ``priors`` [G, 7] = (t[3], q[4]) per query, in the coordinates of the returned poses (host
    or device; a row of NaN: no prior), with a ``rule`` without random draws only: every query's retrieval is restricted to the
    map rows near its prior pose (``forward_map(prior=, gate=)``, which see).  The priors are staged per micro-batch next to the
    descriptors; what the gate did comes back with each micro-batch's results: ``stats["gate_state"]`` (0 = gated, 1 = no prior,
    2 = too few rows inside, ranked against the whole map) and ``stats["gate_rows"]`` (allowed rows inside), int [G], and
    ``.gate_state`` on an ``EvalResult``.  A captured step is keyed by the gate's parameters too.

    ``scenes`` [G] (host integers): each query's scene, for a ``featmap.SceneAtlas`` -- the maps of several scenes in one --
    and for a model whose ``frame_transform`` holds per-scene statistics (``forward_map(scenes=)``, which see).  One call then
    serves the queries of all scenes, where the reference loops over its sequences (dataset_7Scenes_multi.py:273-345), each
    query ranked inside its own scene; the scenes are sliced per micro-batch and staged like the priors, a captured step holds
    them in a static tensor, and the re-run of an irregular kNN micro-batch carries them along.  With a ``rule`` on an atlas
    they are required (ValueError without).
    A ``retrieval.SceneVote`` in their place (a ``rule`` without random draws on an atlas): the queries are not told their
    scene; every query elects it on the GPU from its most similar rows of the whole atlas and is ranked there
    (``forward_map(scenes=SceneVote)``, which see for what is refused -- here before any work is queued).  The elected scenes
    and their votes come back with each micro-batch's results, the way the gate states do: ``stats["scene"]`` and
    ``stats["scene_votes"]``, int [G], and ``.scene`` / ``.scene_votes`` on an ``EvalResult``.  ``capture=True`` is served (the
    vote is part of the captured step, which is keyed by ``SceneVote.key`` too), and the re-run of an irregular kNN
    micro-batch carries the elected scenes along as explicit scenes.

    ``postprocess="device"`` (default ``"host"``): the pose rule runs on the GPU behind every ``forward_map``
    (``query_pose.QueryPose.from_map`` on the map's poses and the device neighbours -- with a rule the rows ``forward_map`` has
    just chosen -- and on ``targets``, staged once as fp32), and 16 doubles per query come back instead of the absolute and
    relative poses and a model-built edge list.  Same return types; a map without poses returns its raw tensors either way.
    ``stats`` also receives ``postprocess`` and ``d2h_bytes``.

    ``fuse`` (None, ``"mean"``, ``"median"``) and ``max_edges``: as in ``evaluate_stream`` -- one pose per query from the
    estimates of all its K database images instead of the ``ref_node``-th one, on the host or on the device.
    ``fuse="consensus"`` with ``inlier_t`` / ``inlier_deg`` (as in ``evaluate_stream``, which see for their unit and defaults):
    the K estimates vote, a database image that retrieval got wrong is outvoted, and every query gets ``inliers`` and ``used``
    -- on the ``EvalResult`` when there are targets, else (the return value stays the poses [G, 7]) in ``stats["inliers"]`` /
    ``stats["used"]``, int [G]; a caller accepts a pose when ``inliers / used`` is high enough for its use.  On the device path
    the integers travel with the rows (8 more bytes per query in ``stats["d2h_bytes"]``); a captured step is keyed by the
    thresholds too, so other thresholds capture a new step instead of replaying the old one.

    ``weights="variance"`` / ``var_floor`` (as in ``evaluate_stream``, which see; needs ``model.mc_dropout`` with ``samples >=
    2``): the K estimates are weighted by the inverse of their Monte-Carlo variance and every query gets ``sigma_t`` and
    ``sigma_q``, the predicted standard deviation of its pose -- on the ``EvalResult`` when there are targets, else in
    ``stats["sigma_t"]`` / ``stats["sigma_q"]``, float [G].  On the device path they travel with the rows (16 more bytes per
    query); a captured step reads its own static variances and is keyed by ``weights`` and ``var_floor`` too.

    ``capture=True`` (GPU map only): a micro-batch's device step -- ``forward_map`` with its retrieval, and the device pose rule
    behind it -- is captured into a HIP graph once per shape (``graphed.GraphedForwardMap``: the full micro-batch and a ragged
    tail) and replayed with one launch per micro-batch instead of ~137.  Same kernels, same launch geometry, same order: the
    results are bit-identical to ``capture=False``.  The captured steps are kept on the model (``refresh_packed`` drops them; a
    step whose map has been extended is captured again), so a second call with the same shapes captures nothing.  What that
    class refuses (``droprate > 0`` without ``model.mc_dropout``, ``knn > 0`` without ``model.static_knn``, ``use_attention``, ``use_AP=False``, uint8 queries) raises here, before any
    work is queued.  ``stats`` also receives ``graphs_captured`` (by this call) and ``graph_replays``.

    ``outputs="query"`` (default ``"all"``): every micro-batch runs ``forward_map(outputs="query")``, which computes only what
    the pose rule reads -- the K relative poses into each query and the query's absolute pose -- and prunes the GNN's last
    recursion accordingly (which see, also for what it does not serve: those raise here, before any work is queued; an unknown
    value raises ValueError).  Same return types and, row for row, the poses of ``"all"`` up to GEMM summation order; the host
    rule then reads the reduced list (K columns per query, sources 1..K), so ``postprocess="host"`` copies K (K + 1) / K times
    fewer relative poses back (``stats["d2h_bytes"]``), and ``ref_node`` / ``fuse`` / ``rule`` / ``capture`` combine as before
    (a captured ``"all"`` step is never replayed for ``"query"``, nor the reverse).  A map without poses then returns the REDUCED
    raw tensors ``(abs_pose [G, 6], rel_pose [G*K, 6])``.  A map that is not on a GPU takes the synchronous path as for ``"all"``:
    the model's ``forward_map`` is called with ``outputs="query"`` and the host rule reads what it returns (``PoseNetX_R2`` itself
    has no CPU compute path and raises there).

    A model with ``knn > 0`` and ``model.static_knn`` set (``PoseNetX_R2.forward_map``, which see): every micro-batch builds its kNN
    graph at fixed positions, k' = min(knn, K) edges into every node, so ``outputs="query"`` and ``capture=True`` serve it and the
    device rule reads the step's edge list with a fixed cut.  ``ref_node >= k'`` raises ValueError up front (test.py:229 takes the
    ``ref_node``-th edge into the query, and there are k').  The count of nodes whose reference list is irregular (the same map
    row named knn + 1 times or more for one query, non-finite features) comes back with each micro-batch's results, one more
    word behind the same event; a micro-batch that reports one is run AGAIN through the general path (``static_knn`` off,
    ``outputs="all"``, uncaptured, on the neighbours it had) and its rows replaced, so every query's result is what the model gives
    without ``static_knn``.  ``stats["knn_irregular_batches"]`` counts these re-runs."""
    device = fmap.device
    if outputs not in ("all", "query"):
        raise ValueError(f"relocalize: outputs must be 'all' or 'query', got {outputs!r}")
    if outputs == "query":
        check = getattr(model, "_check_outputs", None)
        if check is not None:
            check(outputs, None)
        elif getattr(model, "knn", -1) > 0:
            raise NotImplementedError("relocalize(outputs='query') does not serve knn > 0 (a model-built kNN graph)")
    okw = {} if outputs == "all" else {"outputs": outputs}          # a model without the argument keeps serving "all"
    if not isinstance(capture, bool):
        raise TypeError(f"relocalize: capture must be a bool, got {type(capture).__name__}")
    if not torch.is_tensor(queries):
        raise TypeError("relocalize: queries must be a tensor [G, ...]")
    if (neighbours is None) == (rule is None):
        raise ValueError("relocalize: give neighbours or a retrieval rule (exactly one of them)")
    if rule is None and (query_descriptors is not None or query_groups is not None):
        raise ValueError("relocalize: query_descriptors / query_groups belong to retrieval: pass a rule (and no neighbours)")
    if micro_batch < 1:
        raise ValueError("relocalize: micro_batch must be >= 1")
    pr_all = gate_h = None
    if priors is not None or gate is not None:
        if rule is None:
            raise ValueError("relocalize: a pose gate restricts retrieval: pass a rule and no neighbours (given neighbours are used "
                             "as they are)")
        fmap.check_gate("relocalize", rule, priors, gate)
        pr_all = torch.as_tensor(priors)
        if pr_all.dim() != 2 or tuple(pr_all.shape) != (int(queries.shape[0]), 7) or not pr_all.dtype.is_floating_point:
            raise ValueError(f"relocalize: priors must be floating point [{int(queries.shape[0])}, 7] (t[3], q[4] per query), got "
                             f"{tuple(pr_all.shape)} {pr_all.dtype}")
        pr_all = pr_all.to(dtype=torch.float64)
        fmap.gate_rows(gate)                      # (a map without poses raises here, before any work is queued)
        gate_h = np.zeros((int(queries.shape[0]), 2), dtype=np.int32)
    gkw = {} if gate is None else {"gate": gate}
    from .retrieval import SceneVote
    sc_all = vote = scene_h = None
    if isinstance(scenes, SceneVote):
        vote = scenes
        if rule is None:
            raise ValueError("relocalize: a SceneVote finds the scene retrieval ranks in: pass a rule and no neighbours (given "
                             "neighbours are used as they are)")
        scene_h = np.zeros((int(queries.shape[0]), 2), dtype=np.int32)
    elif scenes is not None:
        sc_all = torch.as_tensor(scenes).cpu()
        if sc_all.dim() != 1 or sc_all.shape[0] != int(queries.shape[0]) or sc_all.dtype.is_floating_point or sc_all.dtype == torch.bool:
            raise ValueError(f"relocalize: scenes must be integers [{int(queries.shape[0])}] (one scene index per query), got "
                             f"{tuple(sc_all.shape)} {sc_all.dtype}")
        sc_all = sc_all.to(torch.int32).contiguous()
        if torch.device(device).type == "cuda":
            sc_all = sc_all.pin_memory()
    from .featmap import FeatureMap, SceneAtlas
    if rule is not None and isinstance(fmap, FeatureMap):          # refusals before any work is queued (an atlas without scenes, ...)
        from .frames import SceneFrameTransform
        for_frames = queries.dtype == torch.uint8 and isinstance(getattr(model, "frame_transform", None), SceneFrameTransform)
        if vote is not None:
            if for_frames:
                raise ValueError("relocalize: uint8 queries of a SceneFrameTransform need their scene's statistics before the "
                                 "encoder, and a SceneVote knows the scene only behind it: pass processed queries (or use a plain "
                                 "FrameTransform)")
            fmap._scope(vote, int(queries.shape[0]), rule, "relocalize")
        elif isinstance(fmap, SceneAtlas) or not for_frames:       # (one scene's map: scenes that only the frame transform reads)
            fmap._scope(None if sc_all is None else (sc_all.numpy().astype(np.int64), None), int(queries.shape[0]), rule, "relocalize")
    _check_postprocess("relocalize", postprocess, device)
    _check_fuse("relocalize", fuse, max_edges, ref_node, inlier_t, inlier_deg)
    inlier_t, inlier_deg = float(inlier_t), float(inlier_deg)
    weights, var_floor = _check_weights("relocalize", model, weights, fuse, var_floor)
    if capture:
        if torch.device(device).type != "cuda":
            raise ValueError(f"relocalize: capture=True replays a HIP graph, the feature map is on {device}")
        from .graphed import GraphedForwardMap
        GraphedForwardMap.refuse(model, queries)
    qd_all = qg_all = None
    if rule is None:
        nb = torch.as_tensor(neighbours)
        if nb.dtype != torch.int64 or nb.dim() != 2 or nb.shape[0] != queries.shape[0] or nb.shape[1] < 1:
            raise ValueError(f"relocalize: neighbours must be int64 [G, K >= 1] with G = {queries.shape[0]} queries, got "
                             f"{tuple(nb.shape)} {nb.dtype}")
        g_all, kk = nb.shape
        nb_dev = nb.to(device).contiguous()
        nb_h = nb.cpu().numpy()
    else:
        g_all, kk = int(queries.shape[0]), rule.k
        if fmap.descriptors is not None and query_descriptors is None:
            raise ValueError("relocalize: the map holds its own retrieval descriptors, so query_descriptors [G, Dd] must be given")
        if query_descriptors is not None:
            qd_all = torch.as_tensor(query_descriptors)
            if qd_all.dim() != 2 or qd_all.shape[0] != g_all or qd_all.dtype != torch.float32:
                raise ValueError(f"relocalize: query_descriptors must be fp32 [{g_all}, Dd], got {tuple(qd_all.shape)} {qd_all.dtype}")
        if query_groups is not None:
            qg_all = torch.as_tensor(query_groups).cpu()
            if qg_all.dim() != 1 or qg_all.shape[0] != g_all:
                raise ValueError(f"relocalize: query_groups must be integers [{g_all}], got {tuple(qg_all.shape)}")
        nb_dev = None
        nb_h = np.zeros((g_all, kk), dtype=np.int64)          # filled micro-batch by micro-batch as the copies land
    n_per = kk + 1
    # model.static_knn (PoseNetX_R2 with knn > 0): forward_map builds its kNN graph at fixed positions, k' columns into every node
    static_columns = getattr(model, "_static_columns", None)
    kp = static_columns(None, kk) if static_columns is not None and getattr(model, "knn", -1) > 0 else 0
    if kp and ref_node >= kp:
        raise ValueError(f"relocalize: ref_node = {ref_node}, but the kNN graph has k' = min(knn, K) = {kp} edges into a query "
                         f"(test.py:229 takes the ref_node-th of them)")
    n_irregular = 0
    mc = getattr(model, "mc_dropout", None)
    mc_draw = None if mc is None else mc.draw
    on_gpu = torch.device(device).type == "cuda"
    poses_h = None if fmap.poses is None else fmap.poses.cpu().numpy().astype(np.float64)
    targ_h = None if targets is None else np.asarray(torch.as_tensor(targets).cpu(), dtype=np.float64).reshape(g_all, 6)
    fc_edges = fc_edge_index(n_per).numpy()
    if outputs == "query":         # the columns forward_map(outputs="query") keeps of every graph: those into node 0, in order
        fc_edges = fc_edges[:, fc_edges[1] == 0]
    rows_per = 1 if outputs == "query" else n_per             # rows of abs_pose per graph
    qp = targ_dev = fc_first = None
    captured = model._map_captures if capture else None
    n_captured = n_replays = 0
    if postprocess == "device" and poses_h is not None:
        from .query_pose import QueryPose
        # a captured step counts its bad graphs in the status word of the rule it was captured with: that rule is kept with it
        qp_key = ("pose", tuple(float(v) for v in pose_m), tuple(float(v) for v in pose_s), ref_node, fuse, max_edges, inlier_t,
                  inlier_deg, weights, var_floor)
        qp = captured.get(qp_key) if capture else None
        if qp is None:
            qp = QueryPose(np.asarray(pose_m, dtype=np.float64), np.asarray(pose_s, dtype=np.float64), ref_node, fuse=fuse,
                           max_edges=max_edges, inlier_t=inlier_t, inlier_deg=inlier_deg, weights=weights, var_floor=var_floor)
            if capture:
                captured[qp_key] = qp
        if targets is not None:
            t32 = torch.as_tensor(targets).detach().to(dtype=torch.float32).reshape(g_all, 6)
            targ_dev = t32 if t32.is_cuda else (t32 if t32.is_pinned() else t32.pin_memory()).to(device, non_blocking=True)
        if model.knn <= 0:         # forward_map's own FC list: n (n - 1) columns per graph, graph after graph
            fc_first = torch.arange(min(micro_batch, g_all) + 1, dtype=torch.int64, device=device) * fc_edges.shape[1]
        elif kp:                   # the kNN list at fixed positions: k' columns per node (per query in the query mode)
            fc_first = torch.arange(min(micro_batch, g_all) + 1, dtype=torch.int64, device=device) * (kp if outputs == "query" else kp * n_per)
    acc = _PoseRows(pose_m, pose_s, ref_node, pose=qp, fuse=fuse, max_edges=max_edges, inlier_t=inlier_t,
                    inlier_deg=inlier_deg, weights=weights, var_floor=var_floor)
    raw_abs, raw_rel = [], []
    # static_knn: the nodes of a micro-batch whose reference kNN list is irregular are counted here (zeroed ahead of every eager
    # forward; a captured step has its own), and the word comes back behind the micro-batch's event with its other results
    irr_dev = torch.zeros(1, dtype=torch.int32, device=device) if kp and not capture else None
    ikw = {} if irr_dev is None else {"_irregular": irr_dev}

    # ... into ONE pinned block of the call, a word per micro-batch (a status word like the deferred counters': not in d2h_bytes)
    irr_host = torch.zeros(-(-g_all // micro_batch), dtype=torch.int32, pin_memory=True) if kp and on_gpu else None

    def irregular_back(t, b0):
        if t is None or irr_host is None:
            return None
        host = irr_host[b0 // micro_batch:b0 // micro_batch + 1]
        host.copy_(t, non_blocking=True)
        return host

    def captured_step(x, qd, targ):
        """The captured step of this micro-batch's shape and of this call's configuration: from the model's cache, or captured
        now with the micro-batch itself as the example."""
        nonlocal n_captured
        key = ("step", tuple(x.shape), x.dtype, kk, None if rule is None else (rule.sampling_period, rule.random), postprocess,
               fuse, max_edges, qd is not None, targ is not None, outputs, inlier_t, inlier_deg, weights, var_floor, kp,
               None if gate is None else gate.key, sc_all is not None, None if vote is None else vote.key,
               None if mc is None else (id(mc), mc.samples, mc.seed))       # the sampler's count and seed are baked into the step
        step = captured.get(key)
        if step is None or step.fmap is not fmap or step.pose is not qp or step.stale():
            if len(captured) >= 16:
                captured.clear()
                if qp is not None:
                    captured[qp_key] = qp
            step = captured[key] = GraphedForwardMap(model, fmap, x, kk, rule=rule, query_descriptors=qd, pose=qp,
                                                     pose_kwargs=None if targ is None else {"query_targets": targ}, **okw, **gkw,
                                                     **({"scenes": vote} if vote is not None else {} if sc_all is None or rule is None
                                                        else {"scenes": sc_all[:x.shape[0]]}))
            n_captured += 1
        return step

    def forward(chunk, x):
        nonlocal n_replays
        b0, b1 = chunk[0].first, chunk[0].first + x.shape[0]
        if mc is not None:
            # query b0's graph starts at node b0 (K + 1) of the stream, whatever micro_batch is, and the whole call is ONE draw; a
            # captured step reads both from the same device words, so they are sent ahead of the replay like its other inputs
            mc.place(mc_draw, b0 * n_per)
        if irr_dev is not None:
            irr_dev.zero_()
        skw = {} if sc_all is None else {"scenes": sc_all[b0:b1]}       # (a vote: the captured step's own; eager, below)
        if rule is None and not capture:
            ab, rel, ei = model.forward_map(x, nb_dev[b0:b1], fmap, **okw, **ikw, **skw)
            return _Forward(ab, rel, ei, nb_dev[b0:b1]), irregular_back(irr_dev, b0)
        qd = None
        if qd_all is not None:
            qd = qd_all[b0:b1]
            if on_gpu and not qd.is_cuda:
                qd = (qd if qd.is_pinned() else qd.pin_memory()).to(device, non_blocking=True)
        qg = None if qg_all is None else qg_all[b0:b1]
        pkw = {} if pr_all is None else {"prior": fmap.prior_tensor(pr_all[b0:b1], b1 - b0, "relocalize")}
        if capture:
            targ = None if qp is None or targ_dev is None else targ_dev[b0:b1]
            step = captured_step(x, qd, targ)
            ranks = None
            if rule is not None and (rule.random or qg is not None):
                # this call's rule draws, in query order, exactly what forward_map would have drawn from it
                ranks = rule.ranks(fmap.n_allowed(fmap._query_groups(qg, b1 - b0)[0], b1 - b0,
                                                  *(() if sc_all is None else (sc_all[b0:b1].numpy().astype(np.int64),))))
            # x is one of the pipeline's two staging buffers (the copy of micro-batch i + 1 into the other one runs under this
            # replay), so the step copies it into its one static input: a device copy of the queries, ~1 % of the step
            out = step(x, None if rule is not None else nb_dev[b0:b1], ranks=ranks, query_descriptors=qd, query_groups=qg,
                       query_targets=targ, **pkw, **({} if rule is None else skw))
            n_replays += 1
            # The outputs are the step's STATIC tensors, which the replay of the next micro-batch overwrites.  Their copies to
            # pinned memory (read_back here and in _MicroBatchRunner.launch, right after this returns) are enqueued on the stream
            # the replay ran on BEFORE the next launch() enqueues its replay there: stream order keeps micro-batch i's results.
            return (_Forward(out.abs_pose, out.rel_pose, out.edge_index, out.neighbours,
                             None if rule is None else runner.read_back(out.neighbours), step.packed, step.gate_info,
                             step.scene_info),
                    irregular_back(getattr(step, "irregular", None), b0))
        ab, rel, ei, nb_mb = model.forward_map(x, None, fmap, rule=rule, query_descriptors=qd, query_groups=qg, **okw, **ikw, **pkw, **gkw,
                                               **(skw if vote is None else {"scenes": vote}))
        return (_Forward(ab, rel, ei, nb_mb, runner.read_back(nb_mb), gate_info=model.gate_info if gate is not None else None,
                         scene_info=model.scene_info if vote is not None else None),
                irregular_back(irr_dev, b0))

    def read_back_of(chunk, x, fwd):
        fwd, irr = fwd
        if qp is None:
            # (a weighted host rule: the variances this forward -- or this replay -- has just left, row for row with rel_pose)
            return {"nb": fwd.host_neighbours, "abs": fwd.abs_pose, "rel": fwd.rel_pose,
                    "ei": fwd.edge_index if model.knn > 0 else None,
                    "var": mc.last.rel_var if weights is not None and poses_h is not None else None, "irr": irr,
                    "gate": fwd.gate_info, "scene": fwd.scene_info}
        back = fwd.back
        if back is None:                   # everything the rule writes travels back in one tensor, one copy
            b0, n = chunk[0].first, x.shape[0]
            out, ints, back, spread = qp.output_block(n, fwd.rel_pose.device)
            qp.from_map(fwd.rel_pose, fwd.edge_index, fmap, fwd.neighbours, out=out, inliers=ints, spread=spread,
                        rel_var=None if spread is None else mc.last.rel_var,
                        query_targets=None if targ_dev is None else targ_dev[b0:b0 + n],
                        edge_first=None if fc_first is None else fc_first[:n + 1])
        return {"nb": fwd.host_neighbours, "rel": back, "irr": irr, "gate": fwd.gate_info, "scene": fwd.scene_info}

    def general_again(b0, n):
        """A micro-batch that reported an irregular graph, once more through the general kNN build (static_knn off, the whole
        output, uncaptured) on the neighbours it had: -> its results on the host, in the layout of ``outputs="all"``.  Rare, so it
        simply waits."""
        x = queries[b0:b0 + n].to(device)
        nb_mb = torch.from_numpy(nb_h[b0:b0 + n]).to(device)
        model.static_knn = False
        try:
            if mc is not None:
                mc.place(mc_draw, b0 * n_per)
            # (a vote: the scenes this micro-batch elected -- they have landed with its neighbours -- as explicit scenes)
            again = {"scenes": sc_all[b0:b0 + n]} if sc_all is not None else (
                {"scenes": torch.from_numpy(scene_h[b0:b0 + n, 0].copy())} if vote is not None else {})
            ab, rel, ei = model.forward_map(x, nb_mb, fmap, **again)
            var = None if mc is None else mc.last.rel_var
            if qp is None:
                return {"nb": None, "abs": ab.cpu(), "rel": rel.cpu(), "ei": ei.cpu(),
                        "var": var.cpu() if weights is not None and poses_h is not None else None}
            out, ints, back, spread = qp.output_block(n, rel.device)
            qp.from_map(rel, ei, fmap, nb_mb, out=out, inliers=ints, spread=spread, rel_var=None if spread is None else var,
                        query_targets=None if targ_dev is None else targ_dev[b0:b0 + n])
            return {"nb": None, "rel": back.cpu()}
        finally:
            model.static_knn = True

    def target_block(g):
        target = np.zeros((n_per, 6))
        target[1:] = poses_h[nb_h[g]]
        if targ_h is not None:
            target[0] = targ_h[g]
        return target

    def finish(item):
        nonlocal n_irregular
        b0, host = item.chunk[0].first, item.host
        if host["nb"] is not None:
            nb_h[b0:b0 + host["nb"].shape[0]] = host["nb"].numpy()
        if host.get("gate") is not None:
            gate_h[b0:b0 + host["gate"].shape[0]] = host["gate"].numpy()
        if host.get("scene") is not None:
            scene_h[b0:b0 + host["scene"].shape[0]] = host["scene"].numpy()
        rows_of = rows_per
        if host.get("irr") is not None and int(host["irr"][0]):
            host, rows_of = general_again(b0, sum(int(c.x.shape[0]) for c in item.chunk)), n_per
            n_irregular += 1
        if qp is not None:
            acc.add_device(host["rel"].numpy())
        elif poses_h is None:
            if rows_of != rows_per:        # the query mode's rows of a micro-batch that was run again in full
                into = (host["ei"][1] % n_per) == 0
                host = dict(host, abs=host["abs"][::n_per], rel=host["rel"][into])
            raw_abs.append(host["abs"])
            raw_rel.append(host["rel"])
        else:
            n_g = host["abs"].shape[0] // rows_of
            ei = None if host["ei"] is None else host["ei"].numpy()      # a model-built (kNN) edge list
            acc.add(host["rel"].numpy(), (target_block(g) for g in range(b0, b0 + n_g)), cut_per_graph([n_per] * n_g, ei, [fc_edges] * n_g),
                    None if host.get("var") is None else host["var"].numpy())

    # only the queries are staged, by the rules of evaluate_stream; everything else of a micro-batch goes inside its launch
    runner = _MicroBatchRunner(model, device, micro_batch, bf16_input, pose=qp, collate=lambda chunk, x_dev: chunk[0].x if x_dev is None else x_dev,
                               forward=forward, outputs=read_back_of, capacity=min(micro_batch, g_all))
    runner.run(-(-g_all // micro_batch), lambda i: runner.pieces(queries[i * micro_batch:(i + 1) * micro_batch], i * micro_batch),
               finish, stats, postprocess)
    if mc is not None:
        mc.reset(mc_draw + 1)      # the next call draws the next masks, however many micro-batches this one took
    if stats is not None:
        stats["neighbours"] = nb_h
        if gate_h is not None:
            stats["gate_state"], stats["gate_rows"] = gate_h[:, 0].copy(), gate_h[:, 1].copy()
        if scene_h is not None:
            stats["scene"], stats["scene_votes"] = scene_h[:, 0].copy(), scene_h[:, 1].copy()
        if capture:
            stats.update(graphs_captured=n_captured, graph_replays=n_replays)
        if kp:
            stats["knn_irregular_batches"] = n_irregular
    if poses_h is None:
        return torch.cat(raw_abs), torch.cat(raw_rel)
    res = acc.result(with_targets=targ_h is not None)
    if targ_h is not None:
        res.neighbours = nb_h
        if gate_h is not None:
            res.gate_state = gate_h[:, 0].copy()
        if scene_h is not None:
            res.scene, res.scene_votes = scene_h[:, 0].copy(), scene_h[:, 1].copy()
    elif stats is not None and acc.ints is not None:          # no EvalResult to carry them: the two arrays go to stats
        ints = acc.integers()
        stats["inliers"], stats["used"] = ints[:, 0].copy(), ints[:, 1].copy()
    if targ_h is None and stats is not None and acc.spreads is not None:
        spread = acc.spread()
        stats["sigma_t"], stats["sigma_q"] = spread[:, 0].copy(), spread[:, 1].copy()
    return res
