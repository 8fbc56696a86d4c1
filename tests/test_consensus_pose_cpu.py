"""A query's reference edges fused by consensus, on the host: evaluate.consensus_support / consensus_inliers /
fuse_poses(..., "consensus") / consensus_query_row (the numpy statement of the rule, which is also what the device kernel is held
to), ``fuse="consensus"`` of the two streams on their CPU path and under gloo at world size 2, and the argument checks, none of
which needs a GPU.  Also the generator of the cases the GPU file runs (``consensus_cases``) with the condition it must meet.

What the rule states exactly is held exactly: hand-made candidates whose support is known by construction, thresholds that admit
everything (the bits of "mean") or nothing (candidate 0, the single-edge rule), the cut at ``max_edges``, the reduced edge list."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from relpose_gnn_amd import evaluate as E
from relpose_gnn_amd.graph import fc_edge_index, query_edge_columns
from test_distributed_cpu import _free_port
from test_fused_pose_cpu import PM, PS, ONE, ZERO, _fields, _graph, _same_bits, _star
from test_pipeline_cpu import G, K, _FakeMapModel, map_case  # noqa: F401  (map_case is a fixture)
from test_query_pose_cpu import _map_args, _targets_args, no_library  # noqa: F401  (no_library is a fixture)

ALL = dict(inlier_t=1e300, inlier_deg=360.0)              # thresholds that admit every finite candidate
NONE = dict(inlier_t=0.0, inlier_deg=0.0)                 # ... and none but the candidate itself (distinct candidates)
NAN7 = np.full(7, np.nan)


def _o(t, v=(0.0, 0.0, 0.0)):
    """One row [t, log q] of ``_star``: the candidate is (t, qexp(v))."""
    return list(t) + list(v)


def _rule(o, **kw):
    """The consensus rule over the candidates ``_star(o)`` makes: -> (row [16], inliers, used, I, support)."""
    rel, y, edges = _star(o)
    with np.errstate(all="ignore"):
        cands, _, _ = E.pose_candidates(rel, y, edges, ZERO, ONE)
        inl, support = E.consensus_inliers(cands, **kw)
        row, n_in, used = E.consensus_query_row(rel, y, edges, ZERO, ONE, **kw)
    assert n_in == inl.size and used == cands.shape[0]
    return row, n_in, used, inl.tolist(), support.tolist()


# ---- hand-made cases -------------------------------------------------------------------------------------------------------------
def test_a_cluster_outvotes_the_outliers():
    """Slots 1, 2, 4 lie within 0.1 of each other; 0 and 3 are 5 away from everything."""
    o = [_o((5.0, 0, 0)), _o((0.0, 0, 0)), _o((0.1, 0, 0)), _o((0, -5.0, 0)), _o((0, 0.1, 0))]
    row, n_in, used, inl, support = _rule(o)
    assert (n_in, used, inl, support) == (3, 5, [1, 2, 4], [1, 3, 3, 1, 3])
    cands = E.pose_candidates(*_star(o), ZERO, ONE)[0]
    assert _same_bits(row[:7], E.fuse_poses(cands[[1, 2, 4]], "mean"))
    assert _same_bits(row[:3], [(0.0 + 0.1 + 0.0) / 3, (0.0 + 0.0 + 0.1) / 3, 0.0])
    # "mean" is pulled by the two wrong edges, consensus is not
    assert abs(E.fuse_poses(cands, "mean")[0] - 1.02) < 1e-12 and abs(row[0]) < 0.04
    # the rotation votes too: the same translations, slot 2 turned by 2 * 0.2 rad = 22.9 degrees
    o[2] = _o((0.1, 0, 0), (0.2, 0, 0))
    _, n_in, _, inl, support = _rule(o)
    assert (n_in, inl, support) == (2, [1, 4], [1, 2, 1, 1, 2])
    assert _rule(o, inlier_t=0.25, inlier_deg=23.0)[3] == [1, 2, 4]
    # support is not transitive: a chain 0 - 1 - 2 with steps of 0.2; the middle one has both neighbours
    chain = [_o((0.0, 0, 0)), _o((0.2, 0, 0)), _o((0.4, 0, 0))]
    assert _rule(chain)[3:] == ([0, 1, 2], [2, 3, 2])
    assert E.consensus_support(E.pose_candidates(*_star(chain), ZERO, ONE)[0]).tolist() == [
        [True, True, False], [True, True, True], [False, True, True]]


def test_a_tie_in_support_goes_to_the_lowest_slot():
    """Two pairs, 10 apart: supports 2, 2, 2, 2 and slot 0 wins with its partner, wherever the partner sits."""
    a, b = (0.0, 0, 0), (10.0, 0, 0)
    for order, want in (((a, a, b, b), [0, 1]), ((a, b, b, a), [0, 3]), ((b, a, a, b), [0, 3]), ((b, a, b, a), [0, 2])):
        o = [_o(np.add(t, (0, 0.01 * i, 0))) for i, t in enumerate(order)]
        _, n_in, used, inl, support = _rule(o)
        assert (n_in, used, inl, support) == (2, 4, want, [2, 2, 2, 2]), order


def test_the_winner_need_not_be_candidate_0():
    o = [_o((3.0, 0, 0)), _o((-3.0, 0, 0)), _o((0.0, 0, 0)), _o((0.0, 0.2, 0)), _o((0.0, 0.4, 0))]
    row, n_in, _, inl, support = _rule(o)
    assert support == [1, 1, 2, 3, 2] and inl == [2, 3, 4] and n_in == 3          # the winner is slot 3
    # the sign of the quaternion sum follows the FIRST INLIER, not candidate 0: slot 0 sits in the other hemisphere
    u = np.array([1.0, 2.0, -2.0]) / 3.0
    o = [_o((3.0, 0, 0), (0.1 + np.pi) * u), _o((0.0, 0, 0), 0.1 * u), _o((0.0, 0.1, 0), 0.1 * u)]
    row, n_in, _, inl, _ = _rule(o)
    assert inl == [1, 2] and row[3] > 0.9 and E.qexp((0.1 + np.pi) * u)[0] < -0.9


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("where", [1, 4], ids=["translation", "rotation"])
def test_a_non_finite_candidate_is_an_outlier(value, where):
    o = np.array([_o((0.0, 0, 0)), _o((0.1, 0, 0)), _o((0, 0.1, 0)), _o((0.1, 0.1, 0))])
    clean = _rule(o)
    assert clean[1:4] == (4, 4, [0, 1, 2, 3])
    for c in range(4):
        o2 = o.copy()
        o2[c, where] = value
        row, n_in, used, inl, support = _rule(o2)
        rest = [d for d in range(4) if d != c]
        assert (n_in, used, inl) == (3, 4, rest) and support[c] == 0 and [support[d] for d in rest] == [3, 3, 3]
        want, _, _, _, _ = _rule(o[rest])                                 # the rest of the graph's consensus is unchanged
        assert _same_bits(row, want) and np.isfinite(row).all()
        # with admit-all thresholds too: a NaN dot would give the angle 360 <= 360 by the reference's clamp
        assert _rule(o2, **ALL)[3] == rest
        # "mean" and "median" are voided by it
        with np.errstate(invalid="ignore"):
            assert np.isnan(E.fused_query_pose(*_star(o2), ZERO, ONE, "mean")[0]).all()


def test_all_candidates_non_finite_give_nan_and_zero():
    o = np.array([_o((0.0, 0, 0)), _o((0.1, 0, 0)), _o((0, 0.1, 0))])
    o[0, 0], o[1, 5], o[2, 2] = np.nan, np.inf, -np.inf
    row, n_in, used, inl, support = _rule(o)
    assert (n_in, used, inl, support) == (0, 3, [], [0, 0, 0])
    assert np.isnan(row[:7]).all() and np.isnan(row[14:]).all() and np.isfinite(row[7:14]).all()
    with np.errstate(invalid="ignore"):
        assert _same_bits(E.fuse_poses(E.pose_candidates(*_star(o), ZERO, ONE)[0], "consensus"), NAN7)
    # one candidate, non-finite: there is no separate C = 1 case (the other modes return it as it is, with an error of 360)
    row, n_in, used, _, _ = _rule(o[1:2])
    assert (n_in, used) == (0, 1) and np.isnan(row[:7]).all() and np.isnan(row[14:]).all()


def test_one_candidate_comes_back_as_it_is():
    rel, y, edges = _graph(2, 5)
    want_p, want_t = E.query_pose(rel, y, edges, PM, PS, ref_node=0)
    for kw in ({}, NONE, ALL):
        p, t = E.fused_query_pose(rel, y, edges, PM, PS, "consensus", **kw)
        assert _same_bits(p, want_p) and _same_bits(t, want_t)
        row, n_in, used = E.consensus_query_row(rel, y, edges, PM, PS, **kw)
        r = E.errors(want_p[None], want_t[None])
        assert (n_in, used) == (1, 1) and _same_bits(row, np.hstack((want_p, want_t, r.t_loss, r.q_loss)))


# ---- exact identities ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 4, 8, 12])
def test_admit_all_is_mean_and_admit_none_is_candidate_0(n):
    rel, y, edges = _graph(n, 40 + n)
    cands, targ, _ = E.pose_candidates(rel, y, edges, PM, PS)
    assert _same_bits(E.fuse_poses(cands, "consensus", **ALL), E.fuse_poses(cands, "mean"))
    assert _same_bits(E.fused_query_row(rel, y, edges, PM, PS, "consensus", **ALL), E.fused_query_row(rel, y, edges, PM, PS, "mean"))
    row, n_in, used = E.consensus_query_row(rel, y, edges, PM, PS, **ALL)
    assert (n_in, used) == (n - 1, n - 1)
    # (0, 0): self-support comes from c == d, not from an angle test -- acos(|<q, q>|) need not be 0 -- so every support is 1
    p0, t0 = E.query_pose(rel, y, edges, PM, PS, ref_node=0)
    r0 = E.errors(p0[None], t0[None])
    row, n_in, used = E.consensus_query_row(rel, y, edges, PM, PS, **NONE)
    assert (n_in, used) == (1, n - 1) and _same_bits(row, np.hstack((p0, t0, r0.t_loss, r0.q_loss)))
    assert E.consensus_inliers(cands, **NONE)[1].tolist() == [1] * (n - 1)
    sup = E.consensus_support(cands)
    assert np.array_equal(sup, sup.T) and sup.diagonal().all()


def test_the_distance_is_summed_in_the_stated_order():
    """sqrt((dx dx + dy dy) + dz dz): with dx dx = X in [1, 2) and dy dy = dz dz = s = 0.75 * 2^-53, under half an ulp of X, the
    two small squares are lost one by one and the sum is X; summed the other way round, (s + s) + X is the next double.  A big
    coordinate is searched whose two sums also have different square roots, and the threshold is put at the smaller one."""
    tiny = float(np.sqrt(0.75 * 2.0 ** -53))
    s = tiny * tiny
    for k in range(1, 400):
        big = 1.0 + k * 0.0012345678
        lo, hi = float(np.sqrt((big * big + s) + s)), float(np.sqrt((s + s) + big * big))
        if lo != hi:
            break
    assert (big * big + s) + s == big * big and lo < hi
    o = [_o((0.0, 0, 0)), _o((big, tiny, tiny))]
    assert _rule(o, inlier_t=lo, inlier_deg=5.0)[3] == [0, 1]
    o = [_o((0.0, 0, 0)), _o((tiny, tiny, big))]
    assert _rule(o, inlier_t=lo, inlier_deg=5.0)[3] == [0] and _rule(o, inlier_t=hi, inlier_deg=5.0)[3] == [0, 1]
    # <= on both thresholds: a pair exactly at the translation threshold is in
    o = [_o((0.0, 0, 0)), _o((0.25, 0, 0))]
    assert _rule(o)[3] == [0, 1] and _rule(o, inlier_t=np.nextafter(0.25, 0.0), inlier_deg=5.0)[3] == [0]


# ---- invariances ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 4, 8])
def test_the_reduced_edge_list_and_the_cut_at_max_edges(n):
    rel, y, edges = _graph(n, 60 + n)
    kw = dict(inlier_t=0.9, inlier_deg=70.0)              # wide enough that these random candidates find supporters
    cols = query_edge_columns(edges, [0]).numpy()
    for max_edges in (1, 2, 3, 64):
        a = E.consensus_query_row(rel[cols], y, edges[:, cols], PM, PS, max_edges, **kw)
        b = E.consensus_query_row(rel, y, edges, PM, PS, max_edges, **kw)
        assert _same_bits(a[0], b[0]) and a[1:] == b[1:] and b[2] == min(n - 1, max_edges)
    # max_edges cuts exactly the used set: the rule over the first m candidates
    full, _, _ = E.pose_candidates(rel, y, edges, PM, PS)
    for m in range(1, n):
        p, _ = E.fused_query_pose(rel, y, edges, PM, PS, "consensus", m, **kw)
        assert _same_bits(p, E.fuse_poses(full[:m], "consensus", **kw))
        _, n_in, used = E.consensus_query_row(rel, y, edges, PM, PS, m, **kw)
        assert used == m and n_in == E.consensus_inliers(full[:m], **kw)[0].size
    # columns that are no edge into the query do not matter
    r2 = rel.copy()
    r2[[c for c in range(edges.shape[1]) if c not in cols]] = np.nan
    assert _same_bits(E.consensus_query_row(r2, y, edges, PM, PS, **kw)[0], E.consensus_query_row(rel, y, edges, PM, PS, **kw)[0])


# ---- argument checks ---------------------------------------------------------------------------------------------------------------
BAD_THRESHOLDS = ({"inlier_t": -1e-9}, {"inlier_t": np.nan}, {"inlier_t": np.inf}, {"inlier_deg": -1.0}, {"inlier_deg": 360.5},
                  {"inlier_deg": np.nan}, {"inlier_deg": np.inf}, {"inlier_t": "0.25"}, {"inlier_deg": None}, {"inlier_t": True})


def test_modes_and_defaults():
    assert E.FUSE_MODES == ("mean", "median", "consensus") and (E.INLIER_T, E.INLIER_DEG) == (0.25, 5.0)
    rel, y, edges = _graph(5, 70)
    cands, _, _ = E.pose_candidates(rel, y, edges, PM, PS)
    assert _same_bits(E.fuse_poses(cands, "consensus"), E.fuse_poses(cands, "consensus", inlier_t=0.25, inlier_deg=5.0))
    assert _same_bits(E.fused_query_row(rel, y, edges, PM, PS, "consensus"),
                      E.consensus_query_row(rel, y, edges, PM, PS, inlier_t=0.25, inlier_deg=5.0)[0])
    with pytest.raises(ValueError, match="consensus"):                    # the error text names the third mode
        E.fuse_poses(cands, "ransac")
    with pytest.raises(TypeError):
        E.fuse_poses(cands, "consensus", 0.25, 5.0)                       # keywords: the positional signature has not changed
    for kw in BAD_THRESHOLDS:
        with pytest.raises(ValueError, match="inlier_t|inlier_deg"):
            E.fuse_poses(cands, "consensus", **kw)
        with pytest.raises(ValueError, match="inlier_t|inlier_deg"):
            E.fused_query_pose(rel, y, edges, PM, PS, "consensus", **kw)
        with pytest.raises(ValueError, match="inlier_t|inlier_deg"):
            E.consensus_query_row(rel, y, edges, PM, PS, **kw)
    for ok in ({"inlier_t": 0}, {"inlier_deg": 360}, {"inlier_deg": 0.0}, {"inlier_t": np.float32(0.5)}):
        E.fuse_poses(cands, "consensus", **ok)
    # a bad graph raises reference_edge's error, as for the other modes
    with pytest.raises(ValueError, match="no edge into node 0"):
        E.consensus_query_row(rel[:2], y, np.array([[0, 2], [1, 1]]), PM, PS)


def test_streams_refuse_bad_thresholds(map_case):  # noqa: F811
    fmap, queries, nb, targets, graphs = map_case
    model = _FakeMapModel()
    for kw in BAD_THRESHOLDS:
        with pytest.raises(ValueError, match="inlier_t|inlier_deg"):
            E.evaluate_stream(model, graphs, "cpu", fuse="consensus", **kw)
        with pytest.raises(ValueError, match="inlier_t|inlier_deg"):
            E.relocalize(model, fmap, queries, nb, fuse="consensus", **kw)
    with pytest.raises(ValueError, match="consensus"):
        E.evaluate_stream(model, graphs, "cpu", fuse="vote")
    with pytest.raises(ValueError, match="ref_node"):
        E.relocalize(model, fmap, queries, nb, fuse="consensus", ref_node=1)


@pytest.mark.parametrize("form", ["targets", "map"])
def test_ops_and_the_object_refuse_bad_arguments(no_library, form):  # noqa: F811
    from relpose_gnn_amd import ops
    from relpose_gnn_amd.query_pose import QueryPose
    good = _targets_args() if form == "targets" else _map_args()
    g = 3

    def call(**change):
        kw = dict(good, fuse="consensus")
        kw.update(change)
        rel, ei = kw.pop("rel_pose"), kw.pop("edge_index")
        return ops.query_pose_fused(rel, ei, **kw)

    assert ops.FUSE_MODES == E.FUSE_MODES and (ops.INLIER_T, ops.INLIER_DEG) == (E.INLIER_T, E.INLIER_DEG)
    for kw in BAD_THRESHOLDS:
        with pytest.raises(ValueError, match="inlier_t|inlier_deg"):
            call(**kw)
        with pytest.raises(ValueError, match="inlier_t|inlier_deg"):
            QueryPose(fuse="consensus", **kw)
    with pytest.raises(TypeError):
        call(inliers=torch.zeros((g, 2), dtype=torch.int64))
    for kw in ({"inliers": torch.zeros((g, 3), dtype=torch.int32)}, {"inliers": torch.zeros((g + 1, 2), dtype=torch.int32)},
               {"inliers": torch.zeros((g, 4), dtype=torch.int32)[:, ::2]}, {"fuse": "mean", "inliers": torch.zeros((g, 2), dtype=torch.int32)},
               {"fuse": "vote"}):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(ValueError, match="query_pose_fused.*GPU"):       # everything right, but on the host
        call(inliers=torch.zeros((g, 2), dtype=torch.int32))
    qp = QueryPose((1.0, 2.0, 3.0), fuse="consensus", max_edges=7, inlier_t=0.5, inlier_deg=10)
    assert (qp.fuse, qp.max_edges, qp.inlier_t, qp.inlier_deg) == ("consensus", 7, 0.5, 10.0)
    assert (QueryPose(fuse="consensus").inlier_t, QueryPose(fuse="consensus").inlier_deg) == (0.25, 5.0)
    with pytest.raises(ValueError, match="ref_node"):
        QueryPose(fuse="consensus", ref_node=1)
    if form == "targets":
        t = good
        with pytest.raises(ValueError, match="inliers"):                  # an output of the consensus rule only
            QueryPose(fuse="median").from_targets(t["rel_pose"], t["edge_index"], t["node_first"], t["node_targets"],
                                                  inliers=torch.zeros((g, 2), dtype=torch.int32))
        with pytest.raises(ValueError, match="GPU"):
            qp.from_targets(t["rel_pose"], t["edge_index"], t["node_first"], t["node_targets"],
                            inliers=torch.zeros((g, 2), dtype=torch.int32))


def test_consensus_entry_point_is_declared_bound_and_built():
    import re
    from relpose_gnn_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "relpose_gnn_hip.h")) as f:
        header = f.read()
    assert "rpg_query_pose_consensus_f64" in _lib.SYMBOLS
    fused = re.search(r"\bint\s+rpg_query_pose_fused_f64\s*\(([^)]*)\)", header).group(1)
    decl = re.search(r"\bint\s+rpg_query_pose_consensus_f64\s*\(([^)]*)\)", header).group(1)
    names = [a.split()[-1].lstrip("*") for a in decl.split(",")]
    fused_names = [a.split()[-1].lstrip("*") for a in fused.split(",")]
    assert names == [a for a in fused_names if a != "fuse"][:-5] + ["inlier_t", "inlier_deg", "out", "cand", "count", "inliers",
                                                                   "status", "stream"]
    lib = _lib.lib()
    assert lib.rpg_abi_version() == 1

    def rc(max_edges=64, inlier_t=0.25, inlier_deg=5.0, out=256, inliers=None, rel=256):
        """Pointers that are never followed: every one of these calls is refused by the argument checks."""
        return lib.rpg_query_pose_consensus_f64(rel, 256, 256, 6, 256, None, 1, 256, 4, None, 0, None, 0, None, 0.0, 0.0, 0.0, 1.0,
                                                1.0, 1.0, max_edges, inlier_t, inlier_deg, out, None, None, inliers, 256, None)
    for kw in ({"rel": None}, {"out": None}, {"max_edges": 0}, {"max_edges": 65}, {"inlier_t": -1.0}, {"inlier_t": float("nan")},
               {"inlier_t": float("inf")}, {"inlier_deg": -0.5}, {"inlier_deg": 361.0}, {"inlier_deg": float("nan")},
               {"inliers": 260}):
        assert rc(**kw) == _lib.RPG_ERR_BAD_ARG, kw
    # the fused entry point keeps refusing the third mode's index
    assert lib.rpg_query_pose_fused_f64(256, 256, 256, 6, 256, None, 1, 256, 4, None, 0, None, 0, None, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0,
                                        2, 64, 256, None, None, 256, None) == _lib.RPG_ERR_BAD_ARG


# ---- the two streams on the CPU path -----------------------------------------------------------------------------------------------
STREAM_KW = dict(inlier_t=0.8, inlier_deg=60.0)           # at the scale of the fake model's candidates: some agree, some do not


def _per_graph(model, graphs, pm, ps, max_edges=64, **kw):
    """The per-graph loop over the fake model's relative poses: -> (rows [G, 16], inliers [G], used [G])."""
    rows, ints = [], []
    for g in graphs:
        ei = model.edges(1) if model.knn > 0 else g.edge_index
        rel = g.y[ei[1]] - g.y[ei[0]] + 0.01
        row, n_in, used = E.consensus_query_row(rel.numpy(), g.y.numpy(), ei.numpy(), np.asarray(pm), np.asarray(ps), max_edges, **kw)
        rows.append(row)
        ints.append((n_in, used))
    return np.stack(rows), np.array(ints)[:, 0], np.array(ints)[:, 1]


@pytest.mark.parametrize("knn", [-1, 1])
def test_streams_on_the_cpu_equal_the_per_graph_loop(map_case, knn):  # noqa: F811
    fmap, queries, nb, targets, graphs = map_case
    model = _FakeMapModel(knn)
    pm, ps = (1.0, 2.0, 3.0), (2.0, 2.0, 0.5)
    want, inl, used = _per_graph(model, graphs, pm, ps, **STREAM_KW)
    assert used.tolist() == [K if knn < 0 else 2] * G and inl.min() >= 1
    if knn < 0:
        assert len(set(inl.tolist())) > 1                                 # (the counts vary)
    stats = {}
    res = E.evaluate_stream(model, graphs, "cpu", micro_batch=2, pose_m=pm, pose_s=ps, fuse="consensus", stats=stats, **STREAM_KW)
    assert _same_bits(_fields(res), want) and stats["micro_batches"] == 3
    assert np.array_equal(res.inliers, inl) and np.array_equal(res.used, used) and res.inliers.dtype.kind == "i"
    rel = E.relocalize(model, fmap, queries, nb, micro_batch=2, pose_m=pm, pose_s=ps, targets=targets, fuse="consensus", **STREAM_KW)
    assert _same_bits(_fields(rel), want) and np.array_equal(rel.inliers, inl) and np.array_equal(rel.used, used)
    assert np.array_equal(rel.neighbours, nb.numpy())
    # without targets: the poses as before, the two arrays in stats
    stats = {}
    pred = E.relocalize(model, fmap, queries, nb, micro_batch=2, pose_m=pm, pose_s=ps, fuse="consensus", stats=stats, **STREAM_KW)
    assert isinstance(pred, np.ndarray) and _same_bits(pred, want[:, :7])
    assert np.array_equal(stats["inliers"], inl) and np.array_equal(stats["used"], used)
    # the thresholds and max_edges reach the rule
    for kw in (dict(ALL), dict(NONE), dict(STREAM_KW, max_edges=2), {}):
        w, i, u = _per_graph(model, graphs, pm, ps, **kw)
        res = E.evaluate_stream(model, graphs, "cpu", micro_batch=3, pose_m=pm, pose_s=ps, fuse="consensus", **kw)
        assert _same_bits(_fields(res), w) and np.array_equal(res.inliers, i) and np.array_equal(res.used, u), kw
    # every other mode leaves the two fields None, in the result and in stats
    for fuse in (None, "mean", "median"):
        stats = {}
        res = E.evaluate_stream(model, graphs, "cpu", micro_batch=2, fuse=fuse, stats=stats)
        assert res.inliers is None and res.used is None
        E.relocalize(model, fmap, queries, nb, fuse=fuse, stats=stats)
        assert "inliers" not in stats and "used" not in stats
    assert E.errors(np.zeros((1, 7)), np.zeros((1, 7))).inliers is None   # trailing dataclass fields with defaults


# ---- world size 2 (gloo) ---------------------------------------------------------------------------------------------------------------
class _Fake:             # rel = y[dst] - y[src]: deterministic, CPU-only stand-in for the model
    def __call__(self, b):
        return None, b.y[b.edge_index[1]] - b.y[b.edge_index[0]], b.edge_index


def _dist_graphs(n_graphs):
    from relpose_gnn_amd.graph import Data
    rng = np.random.RandomState(5)
    return [Data(x=torch.zeros(8, 12), edge_index=fc_edge_index(8), y=torch.from_numpy(rng.randn(8, 6) * 0.2).float())
            for _ in range(n_graphs)]


def _consensus_worker(rank, world, port, out_dir, n_graphs):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    res = E.evaluate_stream(_Fake(), _dist_graphs(n_graphs), "cpu", micro_batch=2, rank=rank, world=world, fuse="consensus", **STREAM_KW)
    np.savez(os.path.join(out_dir, f"c{rank}.npz"), pred=res.pred_poses, inliers=res.inliers, used=res.used)
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_stream_gathers_the_integers_in_graph_order(tmp_path):
    world, n_graphs = 2, 7                                                # 4 + 3: a ragged tail
    mp.spawn(_consensus_worker, args=(world, _free_port(), str(tmp_path), n_graphs), nprocs=world, join=True)
    ref = E.evaluate_stream(_Fake(), _dist_graphs(n_graphs), "cpu", micro_batch=3, fuse="consensus", **STREAM_KW)
    assert ref.used.tolist() == [7] * n_graphs and len(set(ref.inliers.tolist())) > 1
    for r in range(world):
        got = np.load(os.path.join(str(tmp_path), f"c{r}.npz"))
        assert np.array_equal(got["inliers"], ref.inliers) and np.array_equal(got["used"], ref.used)
        assert got["inliers"].dtype.kind == "i" and _same_bits(got["pred"], ref.pred_poses)


# ---- the drawn cases of the GPU file ---------------------------------------------------------------------------------------------------
CONSENSUS_SEED, CONSENSUS_GRAPHS, CONSENSUS_CAP = 43, 200, 0.05
CONSENSUS_T, CONSENSUS_DEG = 0.25, 5.0
NEAR_T, NEAR_DEG = 1e-6, 1e-5                             # |dist - inlier_t| / inlier_t, |angle - inlier_deg| in degrees


def near_a_threshold(cands, inlier_t=CONSENSUS_T, inlier_deg=CONSENSUS_DEG) -> bool:
    """Whether some pair of finite candidates sits within a hair of a threshold: the device's acos and sqrt can differ from
    numpy's by ulps, so such a pair's support decision is not comparable between the two."""
    c = cands.shape[0]
    for i in range(c):
        for d in range(i + 1, c):
            if not (np.isfinite(cands[i]).all() and np.isfinite(cands[d]).all()):
                continue
            dx, dy, dz = (float(v) for v in cands[i, :3] - cands[d, :3])
            dist_ = np.sqrt((dx * dx + dy * dy) + dz * dz)
            ang = E.quaternion_angular_error(cands[i, 3:], cands[d, 3:])
            if abs(dist_ - inlier_t) / inlier_t < NEAR_T or abs(ang - inlier_deg) < NEAR_DEG:
                return True
    return False


def consensus_cases(seed=CONSENSUS_SEED, n_graphs=CONSENSUS_GRAPHS, pm=PM, ps=PS):
    """Fully-connected graphs of 3..12 nodes around a true query pose: every database node is "good" with probability 0.6 and its
    edge into the query then estimates that pose up to noise of about 0.04 in un-normalised translation and 0.01 in log-rotation;
    a bad node's estimate is off by noise of 0.5 in both.  fp32 values in float64 arrays.
    -> [(rel [E, 6], y [n, 6], edges [2, E])], and per graph the oracle's (row [16], inliers, used, winner, near a threshold)."""
    rng = np.random.default_rng(seed)
    graphs, oracle = [], []
    for _ in range(n_graphs):
        n = int(rng.integers(3, 13))
        edges = fc_edge_index(n).numpy()
        y = rng.standard_normal((n, 6)) * 0.5
        rel = rng.standard_normal((edges.shape[1], 6)) * 0.3
        good = rng.random(n) < 0.6
        for c in np.flatnonzero(edges[1] == 0):
            s = int(edges[0, c])
            noise = rng.standard_normal(6) * (np.hstack((0.04 / np.asarray(ps), [0.01] * 3)) if good[s] else 0.5)
            rel[c] = y[s] - (y[0] + noise)                                # the estimate y[s] - rel is the true pose plus noise
        rel, y = rel.astype(np.float32).astype(np.float64), y.astype(np.float32).astype(np.float64)
        graphs.append((rel, y, edges))
        cands, _, _ = E.pose_candidates(rel, y, edges, np.asarray(pm), np.asarray(ps))
        _, support = E.consensus_inliers(cands, CONSENSUS_T, CONSENSUS_DEG)
        row, n_in, used = E.consensus_query_row(rel, y, edges, np.asarray(pm), np.asarray(ps), inlier_t=CONSENSUS_T,
                                                inlier_deg=CONSENSUS_DEG)
        oracle.append((row, n_in, used, int(np.argmax(support)), near_a_threshold(cands)))
    return graphs, oracle


def test_consensus_cases_meet_the_yardsticks_own_condition():
    """At most 5 % of the graphs may hold a pair within a hair of a threshold (they are left out of the device comparison); the
    inlier counts and the winners must vary, or the cases would not tell a wrong vote from a right one."""
    graphs, oracle = consensus_cases()
    near = sum(o[4] for o in oracle)
    counts, winners = sorted({o[1] for o in oracle}), sorted({o[3] for o in oracle})
    print(f"consensus cases: {len(oracle)} drawn, {near} near a threshold, inlier counts {counts}, winners {winners}")
    assert len(oracle) == CONSENSUS_GRAPHS and near <= CONSENSUS_CAP * len(oracle)
    assert len(counts) >= 6 and min(counts) >= 1 and len(winners) >= 3
    assert all(o[2] == y.shape[0] - 1 for o, (_, y, _) in zip(oracle, graphs))
    assert any(o[1] < o[2] for o in oracle) and any(o[1] == o[2] for o in oracle)
    assert all(np.isfinite(o[0]).all() for o in oracle)
