"""A query's reference edges weighted by their Monte-Carlo variance, on the host: evaluate.variance_weights / weighted_mean /
fuse_poses_weighted / weighted_query_row (the numpy statement of the rule, which is also what the device kernel is held to),
``weights="variance"`` of the two streams on their CPU path and under gloo at world size 2, and the argument checks, none of which
needs a GPU.  Also the generator of the variances the GPU file draws (``drawn_variances``).

What the rule states exactly is held exactly: with every ``v + var_floor`` the same power of two the weighted row is the unweighted
one bit for bit; hand-made weights give the hand-made mean; the spread is its formula."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from relpose_gnn_amd import evaluate as E
from relpose_gnn_amd.graph import fc_edge_index
from relpose_gnn_amd.mc_dropout import McDropout, McSpread
from test_consensus_pose_cpu import ALL, STREAM_KW, _dist_graphs, _o
from test_distributed_cpu import _free_port
from test_fused_pose_cpu import PM, PS, ONE, ZERO, _fields, _graph, _same_bits, _star
from test_pipeline_cpu import G, K, _FakeMapModel, map_case  # noqa: F401  (map_case is a fixture)
from test_query_pose_cpu import _map_args, _targets_args, no_library  # noqa: F401  (no_library is a fixture)

P2 = dict(var_floor=0.125)                # with variances of 0.125: every v + floor = 0.25, translation weights 4, rotation weights 2
TINY = 1e-30                              # a floor that is negligible next to every variance used here


def _var(c, v=0.125):
    return np.full((c, 6), v)


def _rule(o, var, fuse="mean", **kw):
    """The weighted rule over the candidates ``_star(o)`` makes, variance row c for candidate c: -> (row, spread, inliers, used)."""
    rel, y, edges = _star(o)
    with np.errstate(all="ignore"):
        return E.weighted_query_row(rel, np.asarray(var, dtype=np.float64), y, edges, ZERO, ONE, fuse, **kw)


# ---- hand-made cases -------------------------------------------------------------------------------------------------------------
def test_two_candidates_weigh_three_to_one():
    """Variances v and 3 v (the rotation's three add up to 3 v and 9 v): weights 3 : 1."""
    v = 0.01
    o = np.array([_o((0.3, -1.0, 2.0), (0.1, 0.2, -0.1)), _o((0.5, 1.0, -4.0), (0.12, 0.18, -0.05))])
    var = np.array([[v] * 6, [3 * v] * 6])
    row, spread, inl, used = _rule(o, var, var_floor=TINY)
    assert inl is None and used == 2
    want_t = (3.0 * o[0, :3] + o[1, :3]) / 4.0
    assert np.abs(row[:3] - want_t).max() <= 1e-15 * np.abs(want_t).max()
    q0, q1 = E.qexp(o[0, 3:]), E.qexp(o[1, 3:])
    s = 3.0 * q0 + q1
    want_q = s / np.linalg.norm(s)
    assert np.abs(row[3:7] - want_q).max() <= 1e-15
    # the spread: W_j = 1 / v + 1 / (3 v), Wq = 1 / (3 v) + 1 / (9 v)
    assert np.allclose(spread, [np.sqrt(3 * (3 * v / 4)), np.sqrt(9 * v / 4)], rtol=1e-14, atol=0)
    # per component: only x is uncertain on candidate 1 -- y and z stay the plain mean
    var = np.array([[v] * 6, [3 * v, v, v, v, v, v]])
    row = _rule(o, var, var_floor=TINY)[0]
    assert abs(row[0] - want_t[0]) <= 1e-15 and np.abs(row[1:3] - (o[0, 1:3] + o[1, 1:3]) / 2).max() <= 1e-15 * 4


@pytest.mark.parametrize("c", [1, 2, 7, 64])
def test_equal_power_of_two_weights_are_the_unweighted_rule_bit_for_bit(c):
    rel, y, edges = _graph(c + 1, 200 + c)
    var = np.full((rel.shape[0], 6), 0.125)
    cands, _, _ = E.pose_candidates(rel, y, edges, PM, PS)
    assert cands.shape[0] == c
    pose, _, inl = E.fuse_poses_weighted(cands, _var(c), "mean", PS, **P2)
    assert inl is None and _same_bits(pose, E.fuse_poses(cands, "mean"))
    row, spread, inl, used = E.weighted_query_row(rel, var, y, edges, PM, PS, "mean", **P2)
    assert _same_bits(row, E.fused_query_row(rel, y, edges, PM, PS, "mean")) and (inl, used) == (None, c)
    for kw in (dict(inlier_t=0.9, inlier_deg=70.0), ALL, {}):
        want, n_in, n_used = E.consensus_query_row(rel, y, edges, PM, PS, **kw)
        row, spread, inl, used = E.weighted_query_row(rel, var, y, edges, PM, PS, "consensus", **kw, **P2)
        assert _same_bits(row, want) and (inl, used) == (n_in, n_used)
    # other powers of two (v + floor for the translation, 3 v + floor for the rotation), and a variance of exactly 0 under a
    # power-of-two floor (McDropout(samples=1))
    for v, floor in ((0.0, 2.0 ** -40), (0.0, 1.0), (2.0 ** -20, 2.0 ** -20), (0.5, 0.5)):
        row = E.weighted_query_row(rel, np.full_like(var, v), y, edges, PM, PS, "mean", var_floor=floor)[0]
        assert _same_bits(row, E.fused_query_row(rel, y, edges, PM, PS, "mean")), (v, floor)


@pytest.mark.parametrize("c", [1, 2, 7])
def test_spread_is_its_formula(c):
    rng = np.random.default_rng(300 + c)
    rel, y, edges = _graph(c + 1, 300 + c)
    var = (10.0 ** rng.uniform(-8, -1, (rel.shape[0], 6))).astype(np.float32).astype(np.float64)
    floor = 1e-12
    cols = E.used_columns(edges)
    assert cols.tolist() == np.flatnonzero((edges[1] == 0) & (edges[0] != 0)).tolist() and cols.size == c
    row, spread, _, _ = E.weighted_query_row(rel, var, y, edges, PM, PS, "mean", var_floor=floor, **ALL)
    w = 1.0 / (var[cols, :3] + floor)
    wq = 1.0 / (var[cols, 3:].sum(1) + floor)
    want = [np.sqrt((PS * PS / w.sum(0)).sum()), np.sqrt(1.0 / wq.sum())]
    assert np.allclose(spread, want, rtol=1e-13, atol=0) and np.isfinite(row).all()
    # more candidates or smaller variances: a smaller deviation; and consensus that admits all has the same spread
    assert (E.weighted_query_row(rel, var * 0.25, y, edges, PM, PS, "mean", var_floor=floor)[1] < spread).all()
    got = E.weighted_query_row(rel, var, y, edges, PM, PS, "consensus", var_floor=floor, **ALL)
    assert _same_bits(got[1], spread) and got[2:] == (c, c)
    if c > 1:
        assert _same_bits(got[0], row)
        # one inlier: its own values
        one = E.weighted_query_row(rel, var, y, edges, PM, PS, "consensus", var_floor=floor, inlier_t=0.0, inlier_deg=0.0)
        assert one[2:] == (1, c)
        assert np.allclose(one[1], [np.sqrt((PS * PS / w[0]).sum()), np.sqrt(1.0 / wq[0])], rtol=1e-14, atol=0)


@pytest.mark.parametrize("bad", [np.nan, -1.0, np.inf], ids=["nan", "negative", "pinf"])
@pytest.mark.parametrize("where", [0, 4], ids=["translation", "rotation"])
def test_an_unusable_variance(bad, where):
    o = np.array([_o((0.0, 0, 0)), _o((0.1, 0, 0)), _o((0, 0.1, 0)), _o((0.1, 0.1, 0))])
    var = _var(4, 0.01)
    assert E.variance_weights(var)[2].all()
    for c in range(4):
        v2 = var.copy()
        v2[c, where] = bad
        assert E.variance_weights(v2)[2].tolist() == [d != c for d in range(4)]
        # "mean": voided like today's mean by a non-finite candidate; not a bad graph (nothing raises)
        row, spread, inl, used = _rule(o, v2)
        assert np.isnan(row[:7]).all() and np.isnan(row[14:]).all() and np.isfinite(row[7:14]).all() and np.isnan(spread).all()
        assert (inl, used) == (None, 4)
        # "consensus": it supports nothing and is supported by nothing -- the rule over the rest
        rest = [d for d in range(4) if d != c]
        row, spread, inl, used = _rule(o, v2, "consensus")
        want = _rule(o[rest], var[rest], "consensus")
        assert (inl, used) == (3, 4) and _same_bits(row, want[0]) and _same_bits(spread, want[1]) and np.isfinite(spread).all()
    # -0.0 is not negative, a large finite variance is usable
    v2 = var.copy()
    v2[1, where], v2[2, where] = -0.0, 3e38
    assert E.variance_weights(v2)[2].all() and np.isfinite(_rule(o, v2)[0]).all()
    # every variance unusable under consensus: NaN pose, 0 inliers
    row, spread, inl, used = _rule(o, np.full((4, 6), bad), "consensus")
    assert (inl, used) == (0, 4) and np.isnan(row[:7]).all() and np.isnan(row[14:]).all() and np.isnan(spread).all()
    # C = 1 under "mean": the candidate as it is, its spread NaN; under "consensus" it is an outlier like a non-finite one
    row, spread, inl, used = _rule(o[:1], np.full((1, 6), bad))
    assert _same_bits(row, E.fused_query_row(*_star(o[:1]), ZERO, ONE, "mean")) and np.isnan(spread).all()
    row, spread, inl, used = _rule(o[:1], np.full((1, 6), bad), "consensus")
    assert (inl, used) == (0, 1) and np.isnan(row[:7]).all() and np.isnan(spread).all()


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_a_non_finite_candidate(value):
    o = np.array([_o((0.0, 0, 0)), _o((0.1, 0, 0)), _o((0, 0.1, 0))])
    o[1, 1] = value
    var = _var(3, 0.01)
    row, spread, _, _ = _rule(o, var)
    assert np.isnan(row[:7]).all() and np.isnan(row[14:]).all() and np.isnan(spread).all()
    row, spread, inl, used = _rule(o, var, "consensus")
    want = _rule(o[[0, 2]], var[[0, 2]], "consensus")
    assert (inl, used) == (2, 3) and _same_bits(row, want[0]) and _same_bits(spread, want[1])
    # C = 1, non-finite, "mean": as it is (error 360 by the reference's clamp), and no deviation for a pose that is NaN
    o1 = np.array([_o((0.0, 0, 0), (np.nan, 0, 0))])
    row, spread, _, _ = _rule(o1, _var(1, 0.01))
    assert _same_bits(row, E.fused_query_row(*_star(o1), ZERO, ONE, "mean")) and np.isnan(spread).all()


def test_the_sign_follows_the_first_inlier():
    """Slot 0 is an outlier in the other hemisphere: the weighted quaternion sum is aligned to slot 1."""
    u = np.array([1.0, 2.0, -2.0]) / 3.0
    o = [_o((3.0, 0, 0), (0.1 + np.pi) * u), _o((0.0, 0, 0), 0.1 * u), _o((0.0, 0.1, 0), (0.11 + np.pi) * u)]
    var = np.array([[0.01] * 6, [0.01] * 6, [0.04] * 6])
    assert E.qexp(o[0][3:])[0] < -0.9 and E.qexp(o[1][3:])[0] > 0.9 and E.qexp(o[2][3:])[0] < -0.9
    row, spread, inl, used = _rule(o, var, "consensus", inlier_t=0.25, inlier_deg=5.0, var_floor=TINY)
    assert (inl, used) == (2, 3) and row[3] > 0.9
    q1, q2 = E.qexp(o[1][3:]), E.qexp(o[2][3:])
    s = 4.0 * q1 - q2                                                     # q2 is flipped onto q1's side; weights 4 : 1
    assert np.abs(row[3:7] - s / np.linalg.norm(s)).max() <= 1e-15
    assert abs(row[1] - 0.1 / 5.0) <= 1e-15 and np.isfinite(spread).all()


@pytest.mark.parametrize("n", [2, 4, 8])
def test_the_cut_at_max_edges(n):
    rng = np.random.default_rng(400 + n)
    rel, y, edges = _graph(n, 400 + n)
    var = (10.0 ** rng.uniform(-6, -2, (rel.shape[0], 6))).astype(np.float32).astype(np.float64)
    full, _, _ = E.pose_candidates(rel, y, edges, PM, PS)
    cols = E.used_columns(edges)
    for fuse, kw in (("mean", {}), ("consensus", dict(inlier_t=0.9, inlier_deg=70.0))):
        for m in (1, 2, 3):
            row, spread, inl, used = E.weighted_query_row(rel, var, y, edges, PM, PS, fuse, m, **kw)
            pose, sp, i2 = E.fuse_poses_weighted(full[:m], var[cols[:m]], fuse, PS, **kw)
            assert used == min(m, n - 1) and _same_bits(row[:7], pose) and _same_bits(spread, sp)
            assert inl == (None if i2 is None else i2.size)
            assert E.used_columns(edges, m).tolist() == cols[:m].tolist()
    # variances of columns that are no edge into the query do not matter
    v2 = var.copy()
    v2[[c for c in range(edges.shape[1]) if c not in cols]] = np.nan
    assert _same_bits(E.weighted_query_row(rel, v2, y, edges, PM, PS, "mean")[0], E.weighted_query_row(rel, var, y, edges, PM, PS, "mean")[0])


# ---- the planted outlier ---------------------------------------------------------------------------------------------------------
def test_a_planted_outlier_is_weighted_down():
    """200 graphs of 7 edges around a true pose (noise 0.01, variance 1e-4); one edge is displaced by 10 in translation and its
    variance is 1e4 times the others': the plain mean is pulled by 10 / 7, the weighted mean by about 10 * 1e-4 / 6."""
    rng = np.random.default_rng(77)
    worst_w, best_u = 0.0, np.inf
    for _ in range(200):
        truth = rng.standard_normal(6) * 0.5
        o = truth + rng.standard_normal((7, 6)) * 0.01
        var = np.full((7, 6), 1e-4)
        c = int(rng.integers(0, 7))
        axis = rng.standard_normal(3)
        o[c, :3] += 10.0 * axis / np.linalg.norm(axis)
        var[c] = 1.0
        rel, y, edges = _star(o)
        y[0] = truth
        rel = y[edges[0]] - o                                             # (targets 0 but for the query's own)
        row_w = E.weighted_query_row(rel, var, y, edges, ZERO, ONE, "mean")[0]
        row_u = E.fused_query_row(rel, y, edges, ZERO, ONE, "mean")
        assert row_w[14] < row_u[14], (row_w[14], row_u[14])
        worst_w, best_u = max(worst_w, row_w[14]), min(best_u, row_u[14])
    assert worst_w < 0.05 and best_u > 1.3


# ---- argument checks -------------------------------------------------------------------------------------------------------------
BAD_FLOORS = (0, 0.0, np.nan, 1e-40, -1.0, np.inf, "1e-12", None, True)


def test_modes_defaults_and_refusals():
    assert E.FUSE_MODES == ("mean", "median", "consensus") and E.VAR_FLOOR == 1e-12       # no fourth fuse mode
    rel, y, edges = _graph(5, 70)
    var = np.full((rel.shape[0], 6), 1e-3)
    cands, _, _ = E.pose_candidates(rel, y, edges, PM, PS)
    assert _same_bits(E.fuse_poses_weighted(cands, var[:4], "mean")[0], E.fuse_poses_weighted(cands, var[:4], "mean", var_floor=1e-12)[0])
    for fuse in (None, "median", "weighted"):
        with pytest.raises(ValueError, match="weights"):
            E.fuse_poses_weighted(cands, var[:4], fuse)
        with pytest.raises(ValueError, match="weights"):
            E.weighted_query_row(rel, var, y, edges, PM, PS, fuse)
    for floor in BAD_FLOORS:
        with pytest.raises(ValueError, match="var_floor"):
            E.fuse_poses_weighted(cands, var[:4], "mean", var_floor=floor)
    for ok in (1e-30, 1, np.float32(0.5)):
        E.fuse_poses_weighted(cands, var[:4], "mean", var_floor=ok)
    with pytest.raises(ValueError, match="no edge into node 0"):
        E.weighted_query_row(rel[:2], var[:2], y, np.array([[0, 2], [1, 1]]), PM, PS, "mean")
    r = E.errors(np.zeros((1, 7)), np.zeros((1, 7)))
    assert r.sigma_t is None and r.sigma_q is None                        # trailing dataclass fields with defaults


class _McFake(_FakeMapModel):
    """``_FakeMapModel`` with a sampler: the variances it leaves are a fixed function of the relative poses, row for row."""

    def __init__(self, knn=-1, samples=4):
        super().__init__(knn)
        self.mc_dropout = None if samples is None else McDropout(samples)

    @staticmethod
    def var_of(rel):
        return (rel * rel * 0.05 + 1e-4).float()

    def forward_map(self, x, nb, fmap):
        y, rel, ei = super().forward_map(x, nb, fmap)
        self.mc_dropout.last = McSpread(None, self.var_of(rel))
        return y, rel, ei

    def __call__(self, batch):
        ab, rel, ei = super().__call__(batch)
        self.mc_dropout.last = McSpread(None, self.var_of(rel))
        return ab, rel, ei


def test_streams_refuse_what_the_rule_refuses(map_case):  # noqa: F811
    fmap, queries, nb, targets, graphs = map_case
    model = _McFake()
    for fuse in (None, "median"):
        with pytest.raises(ValueError, match="weights"):
            E.evaluate_stream(model, graphs, "cpu", fuse=fuse, weights="variance")
        with pytest.raises(ValueError, match="weights"):
            E.relocalize(model, fmap, queries, nb, fuse=fuse, weights="variance")
    with pytest.raises(ValueError, match="weights"):
        E.evaluate_stream(model, graphs, "cpu", fuse="mean", weights="inverse")
    for floor in BAD_FLOORS:
        with pytest.raises(ValueError, match="var_floor"):
            E.evaluate_stream(model, graphs, "cpu", fuse="mean", weights="variance", var_floor=floor)
        with pytest.raises(ValueError, match="var_floor"):
            E.relocalize(model, fmap, queries, nb, fuse="mean", var_floor=floor)          # checked always
    # the sampler: none, or one sample (no variance)
    for bad in (_FakeMapModel(), _McFake(samples=1)):
        with pytest.raises(ValueError, match="mc_dropout"):
            E.evaluate_stream(bad, graphs, "cpu", fuse="mean", weights="variance")
        with pytest.raises(ValueError, match="mc_dropout"):
            E.relocalize(bad, fmap, queries, nb, fuse="consensus", weights="variance")
    # without weights nothing of this is asked for
    E.evaluate_stream(_FakeMapModel(), graphs, "cpu", fuse="mean")


@pytest.mark.parametrize("form", ["targets", "map"])
def test_ops_and_the_object_refuse_bad_arguments(no_library, form):  # noqa: F811
    from relpose_gnn_amd import ops
    from relpose_gnn_amd.query_pose import QueryPose
    good = _targets_args() if form == "targets" else _map_args()
    g, e = 3, good["rel_pose"].shape[0]
    var = torch.zeros(e, 6)

    def call(**change):
        kw = dict(good, fuse="mean", weights="variance", rel_var=var)
        kw.update(change)
        rel, ei = kw.pop("rel_pose"), kw.pop("edge_index")
        return ops.query_pose_fused(rel, ei, **kw)

    assert ops.VAR_FLOOR == E.VAR_FLOOR == 1e-12 and ops.FUSE_MODES == ("mean", "median", "consensus")
    for fuse in ("median",):
        with pytest.raises(ValueError, match="weights"):
            call(fuse=fuse)
        with pytest.raises(ValueError, match="weights"):
            QueryPose(fuse=fuse, weights="variance")
    with pytest.raises(ValueError, match="weights"):
        QueryPose(weights="variance")                                     # fuse=None: the single edge
    with pytest.raises(ValueError, match="weights"):
        call(weights="inverse")
    for floor in BAD_FLOORS:
        with pytest.raises(ValueError, match="var_floor"):
            call(var_floor=floor)
        with pytest.raises(ValueError, match="var_floor"):
            QueryPose(fuse="mean", var_floor=floor)                       # checked always
    with pytest.raises(ValueError, match="rel_var"):
        call(rel_var=None)
    with pytest.raises(ValueError, match="rel_var"):
        call(weights=None)                                                # rel_var without weights
    with pytest.raises(ValueError, match="spread"):
        call(weights=None, rel_var=None, spread=torch.zeros((g, 2), dtype=torch.float64))
    for bad in (torch.zeros(e, 5), torch.zeros(e + 1, 6), torch.zeros(e * 6)):
        with pytest.raises(ValueError, match="rel_var"):
            call(rel_var=bad)
    for bad in (torch.zeros(e, 6, dtype=torch.float64), torch.zeros(e, 6, dtype=torch.float16), np.zeros((e, 6), dtype=np.float32)):
        with pytest.raises(TypeError, match="rel_var"):
            call(rel_var=bad)
    with pytest.raises(TypeError, match="spread"):
        call(spread=torch.zeros((g, 2), dtype=torch.float32))
    for bad in (torch.zeros((g, 3), dtype=torch.float64), torch.zeros((g + 1, 2), dtype=torch.float64),
                torch.zeros((g, 4), dtype=torch.float64)[:, ::2]):
        with pytest.raises(ValueError, match="spread"):
            call(spread=bad)
    with pytest.raises(ValueError, match="inliers"):
        call(inliers=torch.zeros((g, 2), dtype=torch.int32))              # weighted "mean" has no integers
    for fuse in ("mean", "consensus"):
        with pytest.raises(ValueError, match="query_pose_fused.*GPU"):   # everything right, but on the host
            call(fuse=fuse, spread=torch.zeros((g, 2), dtype=torch.float64))
    qp = QueryPose(fuse="consensus", weights="variance", var_floor=1e-6)
    assert (qp.weights, qp.var_floor) == ("variance", 1e-6) and QueryPose(fuse="mean").weights is None
    assert QueryPose(fuse="mean", weights="variance").var_floor == 1e-12
    if form == "targets":
        t = good
        with pytest.raises(ValueError, match="rel_var"):                  # belongs to a weighted rule
            QueryPose(fuse="mean").from_targets(t["rel_pose"], t["edge_index"], t["node_first"], t["node_targets"], rel_var=var)
        with pytest.raises(ValueError, match="GPU"):
            qp.from_targets(t["rel_pose"], t["edge_index"], t["node_first"], t["node_targets"], rel_var=var)


def test_the_output_block_grows_by_the_spread():
    from relpose_gnn_amd.query_pose import QueryPose
    g = 5
    for kw, per_graph in ((dict(fuse=None), 128), (dict(fuse="mean"), 128), (dict(fuse="consensus"), 136),
                          (dict(fuse="mean", weights="variance"), 144), (dict(fuse="consensus", weights="variance"), 152)):
        qp = QueryPose(**kw)
        rows, ints, back, spread = qp.output_block(g, "cpu")
        assert back.numel() * back.element_size() == g * per_graph, kw
        assert (ints is None) == (kw["fuse"] != "consensus") and (spread is None) == ("weights" not in kw)
        rows.copy_(torch.arange(g * 16, dtype=torch.float64).view(g, 16))
        if ints is not None:
            ints.copy_(torch.arange(g * 2, dtype=torch.int32).view(g, 2))
        if spread is not None:
            spread.copy_(torch.arange(g * 2, dtype=torch.float64).view(g, 2) + 0.5)
            assert spread.data_ptr() - rows.data_ptr() == g * 128 and spread.data_ptr() % 16 == 0
            if ints is not None:
                assert ints.data_ptr() - rows.data_ptr() == g * 144
        for host in (back, back.numpy()):
            r, i, s = qp.cut_block(host)
            assert np.array_equal(np.asarray(r), rows.numpy())
            assert (i is None) == (ints is None) and (s is None) == (spread is None)
            assert i is None or np.array_equal(np.asarray(i), ints.numpy())
            assert s is None or np.array_equal(np.asarray(s), spread.numpy())


def test_weighted_entry_point_is_declared_bound_and_built():
    import re
    from relpose_gnn_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "relpose_gnn_hip.h")) as f:
        header = f.read()
    assert "rpg_query_pose_weighted_f64" in _lib.SYMBOLS
    cons = re.search(r"\bint\s+rpg_query_pose_consensus_f64\s*\(([^)]*)\)", header).group(1)
    decl = re.search(r"\bint\s+rpg_query_pose_weighted_f64\s*\(([^)]*)\)", header).group(1)
    names = [a.split()[-1].lstrip("*") for a in decl.split(",")]
    cons_names = [a.split()[-1].lstrip("*") for a in cons.split(",")]
    assert [a for a in names if a not in ("rel_var", "var_floor", "consensus", "spread")] == cons_names
    assert names[-3:] == ["spread", "status", "stream"]
    lib = _lib.lib()

    def rc(max_edges=64, inlier_t=0.25, inlier_deg=5.0, var=256, floor=1e-12, consensus=0, out=256, inliers=None, spread=None,
           rel=256):
        """Pointers that are never followed: every one of these calls is refused by the argument checks."""
        return lib.rpg_query_pose_weighted_f64(rel, 256, 256, 6, 256, None, 1, 256, 4, None, 0, None, 0, None, 0.0, 0.0, 0.0, 1.0,
                                               1.0, 1.0, max_edges, inlier_t, inlier_deg, var, floor, consensus, out, None, None,
                                               inliers, spread, 256, None)
    for kw in ({"rel": None}, {"out": None}, {"max_edges": 0}, {"max_edges": 65}, {"inlier_t": -1.0}, {"inlier_deg": float("nan")},
               {"var": None}, {"var": 258}, {"floor": 0.0}, {"floor": float("nan")}, {"floor": 1e-40}, {"floor": float("inf")},
               {"floor": -1.0}, {"consensus": 2}, {"consensus": -1}, {"spread": 264}, {"inliers": 256},
               {"consensus": 1, "inliers": 260}):
        assert rc(**kw) == _lib.RPG_ERR_BAD_ARG, kw


# ---- the two streams on the CPU path -----------------------------------------------------------------------------------------------
def _per_graph(model, graphs, pm, ps, fuse, max_edges=64, **kw):
    """The per-graph loop over the fake model's relative poses and variances: -> (rows [G, 16], spread [G, 2], ints [G, 2])."""
    rows, spreads, ints = [], [], []
    for g in graphs:
        ei = model.edges(1) if model.knn > 0 else g.edge_index
        rel = g.y[ei[1]] - g.y[ei[0]] + 0.01
        row, spread, n_in, used = E.weighted_query_row(rel.numpy(), model.var_of(rel).numpy(), g.y.numpy(), ei.numpy(), np.asarray(pm),
                                                       np.asarray(ps), fuse, max_edges, **kw)
        rows.append(row)
        spreads.append(spread)
        ints.append((-1 if n_in is None else n_in, used))
    return np.stack(rows), np.stack(spreads), np.array(ints)


@pytest.mark.parametrize("knn", [-1, 1])
@pytest.mark.parametrize("fuse", ["mean", "consensus"])
def test_streams_on_the_cpu_equal_the_per_graph_loop(map_case, knn, fuse):  # noqa: F811
    fmap, queries, nb, targets, graphs = map_case
    model = _McFake(knn)
    pm, ps = (1.0, 2.0, 3.0), (2.0, 2.0, 0.5)
    kw = dict(STREAM_KW, var_floor=1e-9) if fuse == "consensus" else dict(var_floor=1e-9)
    want, spread, ints = _per_graph(model, graphs, pm, ps, fuse, **kw)
    assert np.isfinite(spread).all() and len(set(spread[:, 0].tolist())) == G
    unweighted = E.evaluate_stream(model, graphs, "cpu", micro_batch=2, pose_m=pm, pose_s=ps, fuse=fuse, **kw)
    assert not _same_bits(_fields(unweighted), want) and unweighted.sigma_t is None and unweighted.sigma_q is None
    stats = {}
    res = E.evaluate_stream(model, graphs, "cpu", micro_batch=2, pose_m=pm, pose_s=ps, fuse=fuse, weights="variance", stats=stats, **kw)
    assert _same_bits(_fields(res), want) and stats["micro_batches"] == 3
    assert _same_bits(res.sigma_t, spread[:, 0]) and _same_bits(res.sigma_q, spread[:, 1])
    rel = E.relocalize(model, fmap, queries, nb, micro_batch=2, pose_m=pm, pose_s=ps, targets=targets, fuse=fuse, weights="variance",
                       **kw)
    assert _same_bits(_fields(rel), want) and _same_bits(rel.sigma_t, spread[:, 0]) and _same_bits(rel.sigma_q, spread[:, 1])
    if fuse == "consensus":
        assert np.array_equal(res.inliers, ints[:, 0]) and np.array_equal(res.used, ints[:, 1])
        assert np.array_equal(rel.inliers, ints[:, 0]) and np.array_equal(rel.used, ints[:, 1])
    else:
        assert res.inliers is None and rel.used is None
    # without targets: the poses as before, the two arrays in stats
    stats = {}
    pred = E.relocalize(model, fmap, queries, nb, micro_batch=3, pose_m=pm, pose_s=ps, fuse=fuse, weights="variance", stats=stats, **kw)
    assert isinstance(pred, np.ndarray) and _same_bits(pred, want[:, :7])
    assert _same_bits(stats["sigma_t"], spread[:, 0]) and _same_bits(stats["sigma_q"], spread[:, 1])
    assert ("inliers" in stats) == (fuse == "consensus")
    # the floor and max_edges reach the rule
    for kw2 in (dict(kw, var_floor=1e-3), dict(kw, max_edges=2)):
        w, s, _ = _per_graph(model, graphs, pm, ps, fuse, **kw2)
        res = E.evaluate_stream(model, graphs, "cpu", micro_batch=3, pose_m=pm, pose_s=ps, fuse=fuse, weights="variance", **kw2)
        assert _same_bits(_fields(res), w) and _same_bits(res.sigma_t, s[:, 0]), kw2
    # every unweighted mode leaves the two fields None, in the result and in stats
    stats = {}
    E.relocalize(model, fmap, queries, nb, fuse=fuse, stats=stats)
    assert "sigma_t" not in stats and "sigma_q" not in stats


# ---- world size 2 (gloo) ---------------------------------------------------------------------------------------------------------------
class _McDist:           # rel = y[dst] - y[src], variances a fixed function of it: deterministic, CPU-only stand-in for the model
    def __init__(self):
        self.mc_dropout = McDropout(4)

    def __call__(self, b):
        rel = b.y[b.edge_index[1]] - b.y[b.edge_index[0]]
        self.mc_dropout.last = McSpread(None, _McFake.var_of(rel))
        return None, rel, b.edge_index


def _weighted_worker(rank, world, port, out_dir, n_graphs, fuse):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    res = E.evaluate_stream(_McDist(), _dist_graphs(n_graphs), "cpu", micro_batch=2, rank=rank, world=world, fuse=fuse,
                            weights="variance", **STREAM_KW)
    np.savez(os.path.join(out_dir, f"w{rank}.npz"), pred=res.pred_poses, sigma_t=res.sigma_t, sigma_q=res.sigma_q,
             inliers=np.zeros(0) if res.inliers is None else res.inliers)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("fuse", ["mean", "consensus"])
def test_sharded_stream_gathers_the_spread_in_graph_order(tmp_path, fuse):
    world, n_graphs = 2, 7                                                # 4 + 3: a ragged tail
    mp.spawn(_weighted_worker, args=(world, _free_port(), str(tmp_path), n_graphs, fuse), nprocs=world, join=True)
    ref = E.evaluate_stream(_McDist(), _dist_graphs(n_graphs), "cpu", micro_batch=3, fuse=fuse, weights="variance", **STREAM_KW)
    assert len(set(ref.sigma_t.tolist())) == n_graphs and np.isfinite(ref.sigma_q).all()
    for r in range(world):
        got = np.load(os.path.join(str(tmp_path), f"w{r}.npz"))
        assert _same_bits(got["sigma_t"], ref.sigma_t) and _same_bits(got["sigma_q"], ref.sigma_q)
        assert _same_bits(got["pred"], ref.pred_poses)
        if fuse == "consensus":
            assert np.array_equal(got["inliers"], ref.inliers) and got["inliers"].dtype.kind == "i"


# ---- the variances of the GPU file -------------------------------------------------------------------------------------------------
VAR_SEED = 91


def drawn_variances(e: int, rng) -> np.ndarray:
    """fp32 variances [e, 6] spanning 1e-8 .. 1e-1 (log-uniform), about one value in twenty exactly 0; float64 array."""
    var = 10.0 ** rng.uniform(-8.0, -1.0, (e, 6))
    var[rng.random((e, 6)) < 0.05] = 0.0
    return var.astype(np.float32).astype(np.float64)


def test_drawn_variances_span_what_they_say():
    var = drawn_variances(4000, np.random.default_rng(VAR_SEED))
    pos = var[var > 0]
    assert (var == 0).mean() > 0.02 and pos.min() < 1e-7 and pos.max() > 1e-2 and pos.min() >= 0.99e-8 and pos.max() <= 0.1001
    assert E.variance_weights(var)[2].all()
