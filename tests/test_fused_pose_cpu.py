"""All of a query's reference edges fused into one pose, on the host: evaluate.pose_candidates / fuse_poses / fused_query_pose /
fused_query_row (the numpy statement of the rule, which is also what the device kernel is held to), ``fuse=`` of the two streams
on their CPU path, and the argument checks of ops.query_pose_fused / QueryPose(fuse=...), none of which needs a GPU.

The candidates are held to ``evaluate.query_pose`` (the reference rule, itself held to golden G6) edge by edge, bit for bit; the
two combinations are held to independent statements written here with other numpy calls (np.mean / np.median / a pairwise angle
matrix), at 1e-12: a handful of double roundings on values of order 1."""
import os
import re

import numpy as np
import pytest
import torch

from relpose_gnn_amd import evaluate as E
from relpose_gnn_amd.graph import fc_edge_index
from test_pipeline_cpu import G, K, _FakeMapModel, map_case  # noqa: F401  (map_case is a fixture)
from test_query_pose_cpu import _map_args, _targets_args, no_library  # noqa: F401  (no_library is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PM, PS = np.array([1.5, -0.25, 3.0]), np.array([2.0, 0.5, 1.25])
ZERO, ONE = np.zeros(3), np.ones(3)
MODES = ("mean", "median")


def _graph(n, seed):
    rng = np.random.default_rng(seed)
    edges = fc_edge_index(n).numpy()
    rel = (rng.standard_normal((edges.shape[1], 6)) * 0.3).astype(np.float32).astype(np.float64)
    y = (rng.standard_normal((n, 6)) * 0.5).astype(np.float32).astype(np.float64)
    return rel, y, edges


def _star(o):
    """A graph whose candidates are exactly the rows of o [C, 6] (pose_m = 0, pose_s = 1): node c + 1 -> node 0, targets 0, rel = -o."""
    o = np.asarray(o, dtype=np.float64)
    c = o.shape[0]
    edges = np.stack([np.arange(1, c + 1), np.zeros(c, dtype=np.int64)])
    return -o, np.zeros((c + 1, 6)), edges


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _want_mean(cands):
    """The rule by other means: np.mean, a matrix product for the signs."""
    t, q = cands[:, :3], cands[:, 3:]
    sign = np.where(q @ q[0] >= 0.0, 1.0, -1.0)
    s = (q * sign[:, None]).sum(0)
    return np.hstack((t.mean(0), s / np.linalg.norm(s)))


def _want_median(cands):
    t, q = cands[:, :3], cands[:, 3:]
    ang = 2.0 * np.degrees(np.arccos(np.clip(np.abs(q @ q.T), -1.0, 1.0)))
    np.fill_diagonal(ang, 0.0)
    return np.hstack((np.sort(t, 0)[[(len(t) - 1) // 2, len(t) // 2]].mean(0), q[int(np.argmin(ang.sum(1)))]))


# ---- the candidates ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 8, 12])
def test_candidates_are_the_single_edge_rule_edge_by_edge(n):
    rel, y, edges = _graph(n, n)
    cands, targ, count = E.pose_candidates(rel, y, edges, PM, PS)
    assert cands.shape == (n - 1, 7) and count == n - 1
    for c in range(n - 1):
        p, t = E.query_pose(rel, y, edges, PM, PS, ref_node=c)
        assert _same_bits(cands[c], p) and _same_bits(targ, t), c
    # a permuted edge list: the candidates follow the column order
    perm = np.random.default_rng(1).permutation(edges.shape[1])
    cands_p, _, _ = E.pose_candidates(rel[perm], y, edges[:, perm], PM, PS)
    for c in range(n - 1):
        assert _same_bits(cands_p[c], E.query_pose(rel[perm], y, edges[:, perm], PM, PS, ref_node=c)[0])


@pytest.mark.parametrize("fuse", MODES)
def test_one_candidate_is_returned_as_it_is(fuse):
    rel, y, edges = _graph(2, 5)
    want_p, want_t = E.query_pose(rel, y, edges, PM, PS, ref_node=0)
    p, t = E.fused_query_pose(rel, y, edges, PM, PS, fuse)
    assert _same_bits(p, want_p) and _same_bits(t, want_t)
    # max_edges = 1 of a larger graph: edge 0 alone
    rel, y, edges = _graph(8, 6)
    assert _same_bits(E.fused_query_pose(rel, y, edges, PM, PS, fuse, max_edges=1)[0], E.query_pose(rel, y, edges, PM, PS, 0)[0])
    # a non-finite value in the only candidate propagates as in the single-edge rule (no voiding: nothing is combined)
    rel, y, edges = _graph(2, 7)
    rel[1, 4] = np.nan
    with np.errstate(invalid="ignore"):
        row = E.fused_query_row(rel, y, edges, PM, PS, fuse)
        want_p, want_t = E.query_pose(rel, y, edges, PM, PS, 0)
        want = E.errors(want_p[None], want_t[None])
    assert np.isfinite(row[:3]).all() and np.isnan(row[3:7]).all() and row[15] == 360.0
    assert _same_bits(row, np.hstack((want_p, want_t, want.t_loss, want.q_loss)))


def test_max_edges_cuts_in_column_order_and_count_tells():
    rel, y, edges = _graph(8, 8)
    full, _, count = E.pose_candidates(rel, y, edges, PM, PS)
    assert count == 7
    for m in (1, 3, 6, 7, 64):
        cands, _, count = E.pose_candidates(rel, y, edges, PM, PS, max_edges=m)
        assert count == 7 and _same_bits(cands, full[:m])
        for fuse in MODES:
            assert _same_bits(E.fused_query_pose(rel, y, edges, PM, PS, fuse, max_edges=m)[0], E.fuse_poses(full[:m], fuse))


def test_a_self_edge_is_skipped():
    rel, y, edges = _graph(4, 9)
    hits = np.flatnonzero(edges[1] == 0)
    # a self-edge 0 -> 0 in front of, between and behind the edges into the query
    for at in (0, int(hits[1]), edges.shape[1]):
        e2 = np.insert(edges, at, [0, 0], axis=1)
        r2 = np.insert(rel, at, 7.0, axis=0)
        cands, _, count = E.pose_candidates(r2, y, e2, PM, PS)
        assert count == 3 and _same_bits(cands, E.pose_candidates(rel, y, edges, PM, PS)[0])
        for fuse in MODES:
            assert _same_bits(E.fused_query_pose(r2, y, e2, PM, PS, fuse)[0], E.fused_query_pose(rel, y, edges, PM, PS, fuse)[0])


# ---- the two combinations ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 4, 8, 9])
def test_random_graphs_against_the_independent_statements(n):
    """C = 2, 3 (even, odd), 7, 8."""
    rel, y, edges = _graph(n, 20 + n)
    cands, targ, _ = E.pose_candidates(rel, y, edges, PM, PS)
    for fuse, want in (("mean", _want_mean(cands)), ("median", _want_median(cands))):
        pred, t = E.fused_query_pose(rel, y, edges, PM, PS, fuse)
        assert np.abs(pred - want).max() <= 1e-12 and _same_bits(t, targ)
        assert abs(np.linalg.norm(pred[3:]) - 1.0) <= 1e-12
        row = E.fused_query_row(rel, y, edges, PM, PS, fuse)
        r = E.errors(pred[None], targ[None])
        assert _same_bits(row, np.hstack((pred, targ, r.t_loss, r.q_loss)))
    med = E.fuse_poses(cands, "median")
    assert any(_same_bits(med[3:], c[3:]) for c in cands)                 # the medoid is one of the candidates, not a blend


def test_mean_aligns_q_and_minus_q():
    """log q of norm |v| and of norm |v| + pi along the same axis are q and -q: one rotation (its angle 2 |v| has gone once round,
    2 pi more).  Unaligned their sum would cancel; aligned to q_0 they add up."""
    u = np.array([1.0, 2.0, -2.0]) / 3.0
    va, vb, vc = 0.2 * u, (0.2 + np.pi) * u, np.array([0.0, 0.3, 0.1])
    qa, qb, qc = E.qexp(va), E.qexp(vb), E.qexp(vc)
    assert np.abs(qa + qb).max() < 1e-14 and qb[0] < -0.9
    for order, lead in (((va, vb, vc), qa), ((vb, va, vc), qb), ((vc, vb, va), qc)):
        o = np.hstack((np.zeros((3, 3)), np.array(order)))
        pred, _ = E.fused_query_pose(*_star(o), ZERO, ONE, "mean")
        s = 2.0 * qa + qc                                                 # q_b counted as q_a
        want = s / np.linalg.norm(s) * np.sign(s @ lead)                  # in the hemisphere of candidate 0
        assert np.abs(pred[3:] - want).max() <= 1e-12, order
    # ... and the medoid counts q and -q as the same rotation (angle 0 between them)
    o = np.hstack((np.zeros((3, 3)), np.array((vc, va, vb))))
    pred, _ = E.fused_query_pose(*_star(o), ZERO, ONE, "median")
    assert _same_bits(pred[3:], qa) or _same_bits(pred[3:], qb)           # sums: c: 2 x;  a and b: x + (nearly) 0


def test_mean_of_a_zero_sum_is_candidate_0():
    """Unreachable from unit quaternions (the aligned sum has <S, q_0> >= 1), so stated on fuse_poses directly."""
    t = np.arange(9.0).reshape(3, 3)
    for q in (np.zeros((3, 4)), np.array([[0.0, 0, 0, 0], [1.0, 0, 0, 0], [-1.0, 0, 0, 0]])):
        pred = E.fuse_poses(np.hstack((t, q)), "mean")
        assert _same_bits(pred[:3], [3.0, 4.0, 5.0]) and _same_bits(pred[3:], q[0])


def test_mean_sums_in_column_order():
    """(a + b) + c in column order, not numpy's pairwise or a sorted sum: with a = 1, b = 2^-53, c = 2^-53 the first gives 1."""
    tiny = 2.0 ** -53
    cands = np.hstack((np.array([[1.0, 0, 0], [tiny, 0, 0], [tiny, 0, 0]]), np.tile([1.0, 0, 0, 0], (3, 1))))
    assert E.fuse_poses(cands, "mean")[0] == 1.0 / 3.0
    assert E.fuse_poses(cands[::-1], "mean")[0] == (2.0 * tiny + 1.0) / 3.0 != 1.0 / 3.0


def test_median_ties_and_even_counts():
    q = np.tile([1.0, 0, 0, 0], (4, 1))
    t = np.array([[3.0, 1.0, -2.0], [1.0, 1.0, 5.0], [3.0, 1.0, 0.0], [2.0, 7.0, -2.0]])
    pred = E.fuse_poses(np.hstack((t, q)), "median")
    assert pred[:3].tolist() == [2.5, 1.0, -1.0]                          # (2 + 3) / 2, (1 + 1) / 2, (-2 + 0) / 2
    assert E.fuse_poses(np.hstack((t[:3], q[:3])), "median")[:3].tolist() == [3.0, 1.0, 0.0]
    # medoid ties go to the lowest index: two candidates (both sums are the one angle), and four identical ones
    a, b = E.qexp([0.1, 0.0, 0.0]), E.qexp([0.0, 0.2, 0.0])
    assert _same_bits(E.fuse_poses(np.hstack((t[:2], [a, b])), "median")[3:], a)
    assert _same_bits(E.fuse_poses(np.hstack((t[:2], [b, a])), "median")[3:], b)
    # a symmetric triple: b in the middle of a and c wins; mirrored copies of a tie and the first one is taken
    qs = [E.qexp([0.1 * k, 0.0, 0.0]) for k in range(3)]
    assert _same_bits(E.fuse_poses(np.hstack((t[:3], qs)), "median")[3:], qs[1])
    # exact ties: orthogonal quaternions are 180 degrees apart, equal ones 0 (the dots are exactly 0 and 1)
    i, j, k = np.eye(4)[:3]
    assert E.medoid_angle_sums(np.array([j, i, k])).tolist() == [360.0, 360.0, 360.0]
    assert _same_bits(E.fuse_poses(np.hstack((t[:3], [j, i, k])), "median")[3:], j)
    assert E.medoid_angle_sums(np.array([j, i, i, j])).tolist() == [360.0] * 4
    assert _same_bits(E.fuse_poses(np.hstack((t, [j, i, i, j])), "median")[3:], j)
    assert _same_bits(E.fuse_poses(np.hstack((t, [k, i, i, i])), "median")[3:], i)       # sums 540, 180, 180, 180: the first i


@pytest.mark.parametrize("fuse", MODES)
@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("where", [1, 4], ids=["translation", "rotation"])
def test_a_non_finite_candidate_voids_the_fused_pose(fuse, value, where):
    rel, y, edges = _graph(4, 30)
    hits = np.flatnonzero(edges[1] == 0)
    clean = E.fused_query_row(rel, y, edges, PM, PS, fuse)
    for c in range(3):                                                    # whichever candidate it is, first, middle or last
        r2 = rel.copy()
        r2[hits[c], where] = value
        with np.errstate(invalid="ignore"):
            row = E.fused_query_row(r2, y, edges, PM, PS, fuse)
            pred, targ = E.fused_query_pose(r2, y, edges, PM, PS, fuse)
        assert np.isnan(pred).all() and np.isnan(row[:7]).all() and np.isnan(row[14:]).all()
        assert _same_bits(row[7:14], clean[7:14]) and _same_bits(targ, clean[7:14])
        if c:                                                             # beyond the cut it is not used
            assert _same_bits(E.fused_query_row(r2, y, edges, PM, PS, fuse, max_edges=c),
                              E.fused_query_row(rel, y, edges, PM, PS, fuse, max_edges=c))
    # in a column that is no edge into the query: nothing happens
    r2 = rel.copy()
    r2[[i for i in range(edges.shape[1]) if i not in hits], :] = value
    assert _same_bits(E.fused_query_row(r2, y, edges, PM, PS, fuse), clean)


@pytest.mark.parametrize("fuse", MODES)
def test_bad_graphs_raise_the_error_of_reference_edge(fuse):
    rel, y, edges = _graph(4, 31)
    with pytest.raises(ValueError) as ref:
        E.reference_edge(np.array([[0, 2], [1, 1]]))
    msg = re.escape(str(ref.value))
    for bad in (np.array([[0, 2], [1, 1]]),                               # no edge into node 0
                np.array([[0, 0, 1], [0, 0, 2]]),                         # only self-edges into it
                np.array([[1, 9, 2], [0, 0, 0]]),                         # a used edge from outside the graph
                np.array([[1, -1, 2], [0, 0, 0]])):
        with pytest.raises(ValueError, match=msg):
            E.fused_query_pose(rel[:bad.shape[1]], y, bad, PM, PS, fuse)
    # the outside source beyond the cut is not used: the graph is good
    E.fused_query_pose(rel[:3], y, np.array([[1, 2, 9], [0, 0, 0]]), PM, PS, fuse, max_edges=2)
    with pytest.raises(ValueError, match="fuse"):
        E.fuse_poses(np.zeros((2, 7)), "mode")


# ---- the drawn cases of the medoid-index check (the GPU test holds the kernel's index to the oracle's on these) ----------------
MEDOID_SEED, MEDOID_GRAPHS, MEDOID_GAP, MEDOID_CAP = 41, 200, 1e-6, 0.05


def medoid_cases(seed=MEDOID_SEED, n_graphs=MEDOID_GRAPHS):
    """Fully-connected graphs of 4..12 nodes (C = 3..11; with C = 2 both sums are the one angle, a tie by construction), fp32
    values in float64 arrays: -> [(rel [E, 6], y [n, 6], edges [2, E])], and per graph the oracle's (index, gap between the best
    and the second-best angle sum in degrees)."""
    rng = np.random.default_rng(seed)
    graphs, oracle = [], []
    for _ in range(n_graphs):
        n = int(rng.integers(4, 13))
        edges = fc_edge_index(n).numpy()
        rel = (rng.standard_normal((edges.shape[1], 6)) * 0.3).astype(np.float32).astype(np.float64)
        y = (rng.standard_normal((n, 6)) * 0.5).astype(np.float32).astype(np.float64)
        graphs.append((rel, y, edges))
        sums = E.medoid_angle_sums(E.pose_candidates(rel, y, edges, PM, PS)[0][:, 3:])
        best, second = np.sort(sums)[:2]
        oracle.append((int(np.argmin(sums)), float(second - best)))
    return graphs, oracle


def test_medoid_cases_leave_few_near_ties():
    """Cases whose best and second-best sums are closer than 1e-6 degrees are left out of the index check (acos near 1 moves an
    angle by up to 5e-6 degrees per 8 ulp of the dot, see test_hip_query_pose.py); at most 5 % may be.  For this seed: none."""
    _, oracle = medoid_cases()
    near = sum(gap < MEDOID_GAP for _, gap in oracle)
    print(f"medoid cases: {len(oracle)} drawn, {near} within {MEDOID_GAP} degrees, smallest gap {min(g for _, g in oracle):.3e}")
    assert len(oracle) == MEDOID_GRAPHS and near <= MEDOID_CAP * len(oracle)
    assert len({i for i, _ in oracle}) >= 8                               # the index is not always the same one


# ---- the two streams on the CPU path -----------------------------------------------------------------------------------------------
def _fields(r):
    return np.concatenate([r.pred_poses, r.targ_poses, r.t_loss[:, None], r.q_loss[:, None]], 1)


def _per_graph(model, graphs, pm, ps, fuse, max_edges=64):
    """The per-graph loop: the model's relative poses of each graph through fused_query_row (fuse=None: query_pose + errors)."""
    rows = []
    n = K + 1
    for g in graphs:
        if model.knn > 0:
            ei = model.edges(1)
            rel = g.y[ei[1]] - g.y[ei[0]] + 0.01
        else:
            ei = g.edge_index
            rel = g.y[ei[1]] - g.y[ei[0]] + 0.01
        assert g.y.shape[0] == n
        rel, y, ei = rel.numpy(), g.y.numpy(), ei.numpy()
        if fuse is None:
            p, t = E.query_pose(rel, y, ei, np.asarray(pm), np.asarray(ps))
            r = E.errors(p[None], t[None])
            rows.append(np.hstack((p, t, r.t_loss, r.q_loss)))
        else:
            rows.append(E.fused_query_row(rel, y, ei, np.asarray(pm), np.asarray(ps), fuse, max_edges))
    return np.stack(rows)


@pytest.mark.parametrize("knn", [-1, 1])
@pytest.mark.parametrize("fuse", MODES)
def test_streams_on_the_cpu_equal_the_per_graph_loop(map_case, knn, fuse):
    fmap, queries, nb, targets, graphs = map_case
    model = _FakeMapModel(knn)
    pm, ps = (1.0, 2.0, 3.0), (2.0, 2.0, 0.5)
    want = _per_graph(model, graphs, pm, ps, fuse)
    single = _per_graph(model, graphs, pm, ps, None)
    assert not np.array_equal(want[:, :7], single[:, :7])                 # (the fused pose is another pose)
    stats = {}
    res = E.evaluate_stream(model, graphs, "cpu", micro_batch=2, pose_m=pm, pose_s=ps, fuse=fuse, stats=stats)
    assert _same_bits(_fields(res), want) and stats["postprocess"] == "host" and stats["micro_batches"] == 3
    rel = E.relocalize(model, fmap, queries, nb, micro_batch=2, pose_m=pm, pose_s=ps, targets=targets, fuse=fuse)
    assert _same_bits(_fields(rel), want) and np.array_equal(rel.neighbours, nb.numpy())
    pred = E.relocalize(model, fmap, queries, nb, micro_batch=2, pose_m=pm, pose_s=ps, fuse=fuse)
    assert isinstance(pred, np.ndarray) and _same_bits(pred, want[:, :7])
    # max_edges reaches the rule
    cut = E.evaluate_stream(model, graphs, "cpu", micro_batch=2, pose_m=pm, pose_s=ps, fuse=fuse, max_edges=2)
    assert _same_bits(_fields(cut), _per_graph(model, graphs, pm, ps, fuse, 2))
    cut = E.relocalize(model, fmap, queries, nb, micro_batch=5, pose_m=pm, pose_s=ps, targets=targets, fuse=fuse, max_edges=1)
    assert _same_bits(_fields(cut), single)                               # one edge: the single-edge rule's rows
    # fuse=None is what it is without the argument
    for kw in ({}, {"fuse": None}):
        res = E.evaluate_stream(model, graphs, "cpu", micro_batch=2, pose_m=pm, pose_s=ps, **kw)
        assert _same_bits(_fields(res), single)
        rel = E.relocalize(model, fmap, queries, nb, micro_batch=2, pose_m=pm, pose_s=ps, targets=targets, **kw)
        assert _same_bits(_fields(rel), single)


def test_streams_refuse_bad_fuse_arguments(map_case):
    fmap, queries, nb, targets, graphs = map_case
    model = _FakeMapModel()
    for kw in ({"fuse": "avg"}, {"fuse": "mean", "ref_node": 1}, {"fuse": "median", "max_edges": 0},
               {"fuse": "median", "max_edges": 65}, {"fuse": "mean", "max_edges": 2.0}):
        with pytest.raises(ValueError, match="fuse|max_edges"):
            E.evaluate_stream(model, graphs, "cpu", **kw)
        with pytest.raises(ValueError, match="fuse|max_edges"):
            E.relocalize(model, fmap, queries, nb, **kw)
    # a graph without a usable edge: the host path's ValueError
    from relpose_gnn_amd.graph import Data
    bad = list(graphs)
    bad[3] = Data(x=graphs[3].x, edge_index=torch.tensor([[0, 2], [1, 1]]), y=graphs[3].y)
    with pytest.raises(ValueError, match="no edge into node 0"):
        E.evaluate_stream(model, bad, "cpu", micro_batch=2, fuse="mean")


# ---- argument checks of the device entry points (nothing is launched) ------------------------------------------------------------
@pytest.mark.parametrize("form", ["targets", "map"])
def test_ops_query_pose_fused_refuses_bad_arguments(no_library, form):  # noqa: F811
    from relpose_gnn_amd import ops
    good = _targets_args() if form == "targets" else _map_args()

    def call(**change):
        kw = dict(good, fuse="mean")
        kw.update(change)
        rel, ei = kw.pop("rel_pose"), kw.pop("edge_index")
        return ops.query_pose_fused(rel, ei, **kw)

    with pytest.raises(TypeError):
        call(rel_pose=good["rel_pose"].double())
    with pytest.raises(TypeError):
        call(max_edges=8.0)
    with pytest.raises(TypeError):
        call(max_edges=True)
    with pytest.raises(TypeError):
        call(candidates=torch.zeros((3, 64, 16), dtype=torch.float32))
    with pytest.raises(TypeError):
        call(counts=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(TypeError):
        call(ref_node=0)                                                  # there is no reference edge to choose
    for kw in ({"fuse": "avg"}, {"fuse": None}, {"fuse": 0}, {"max_edges": 0}, {"max_edges": 65},
               {"candidates": torch.zeros((3, 63, 16), dtype=torch.float64)},
               {"candidates": torch.zeros((3, 8, 16), dtype=torch.float64)},
               {"max_edges": 8, "candidates": torch.zeros((3, 64, 16), dtype=torch.float64)},
               {"counts": torch.zeros(4, dtype=torch.int32)}, {"out": torch.zeros((3, 15), dtype=torch.float64)},
               {"candidates": torch.zeros((3, 64, 32), dtype=torch.float64)[:, :, ::2]}):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(ValueError, match="query_pose_fused.*GPU"):       # everything right, but on the host
        call(candidates=torch.zeros((3, 64, 16), dtype=torch.float64), counts=torch.zeros(3, dtype=torch.int32))


def test_query_pose_object_with_fuse(no_library):  # noqa: F811
    from relpose_gnn_amd.query_pose import QueryPose
    for kw in ({"fuse": "avg"}, {"fuse": "mean", "ref_node": 1}, {"fuse": "median", "max_edges": 0}, {"fuse": "mean", "max_edges": 65}):
        with pytest.raises(ValueError):
            QueryPose(**kw)
    with pytest.raises(TypeError):
        QueryPose(fuse="mean", max_edges=1.5)
    plain = QueryPose(ref_node=2)
    assert plain.fuse is None and plain.ref_node == 2
    t = _targets_args()
    with pytest.raises(ValueError, match="candidates"):                   # outputs of the fused rule only
        plain.from_targets(t["rel_pose"], t["edge_index"], t["node_first"], t["node_targets"], counts=torch.zeros(3, dtype=torch.int32))
    qp = QueryPose((1.0, 2.0, 3.0), fuse="median", max_edges=7)
    assert (qp.fuse, qp.max_edges, qp.ref_node) == ("median", 7, 0)
    qp.check()
    qp.check(wait=False)
    with pytest.raises(ValueError, match="GPU"):
        qp.from_targets(t["rel_pose"], t["edge_index"], t["node_first"], t["node_targets"], edge_first=t["edge_first"])
    with pytest.raises(ValueError):
        qp.from_targets(t["rel_pose"], t["edge_index"], t["node_first"], t["node_targets"],
                        candidates=torch.zeros((3, 64, 16), dtype=torch.float64))       # max_edges is 7

    class Map:
        poses = None
    m = _map_args()
    with pytest.raises(ValueError, match="no poses"):
        qp.from_map(m["rel_pose"], m["edge_index"], Map(), m["neighbours"])
    Map.poses = m["map_poses"]
    with pytest.raises(ValueError, match="GPU"):
        qp.from_map(m["rel_pose"], m["edge_index"], Map(), m["neighbours"], query_targets=m["query_targets"])


def test_fused_entry_point_is_declared_bound_and_built():
    from relpose_gnn_amd import _lib, build
    with open(os.path.join(ROOT, "include", "relpose_gnn_hip.h")) as f:
        header = f.read()
    assert "rpg_query_pose_fused_f64" in _lib.SYMBOLS and "query_pose.hip" in build.SOURCES
    with open(os.path.join(ROOT, "relpose-gnn_amd", "csrc", "query_pose.hip")) as f:
        src = f.read()
    assert re.search(r'extern\s+"C"\s+int\s+rpg_query_pose_fused_f64\s*\(', src)
    decl = re.search(r"\bint\s+rpg_query_pose_fused_f64\s*\(([^)]*)\)", header).group(1)
    single = re.search(r"\bint\s+rpg_query_pose_f64\s*\(([^)]*)\)", header).group(1)
    names = [a.split()[-1].lstrip("*") for a in decl.split(",")]
    assert names == [a.split()[-1].lstrip("*") for a in single.split(",") if "ref_node" not in a][:-3] + [
        "fuse", "max_edges", "out", "cand", "count", "status", "stream"]

    class Fake:
        def __getattr__(self, name):
            holder = type("F", (), {})()
            setattr(self, name, holder)
            return holder
    fake = Fake()
    _lib._declare(fake)
    assert len(fake.rpg_query_pose_fused_f64.argtypes) == len(names) == 27
    # the library exports it and refuses bad arguments on the host, before any launch
    lib = _lib.lib()

    def rc(fuse=0, max_edges=64, out=256, cand=None, count=None, rel=256):
        """Pointers that are never followed: every one of these calls is refused by the argument checks."""
        return lib.rpg_query_pose_fused_f64(rel, 256, 256, 6, 256, None, 1, 256, 4, None, 0, None, 0, None, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0,
                                            fuse, max_edges, out, cand, count, 256, None)
    for kw in ({"rel": None}, {"out": None}, {"fuse": 2}, {"fuse": -1}, {"max_edges": 0}, {"max_edges": 65}, {"out": 264},
               {"cand": 264}, {"count": 258}):
        assert rc(**kw) == _lib.RPG_ERR_BAD_ARG, kw
