"""A query's reference edges weighted by their Monte-Carlo variance, on the device: rpg_query_pose_weighted_f64 (a further mode of
query_pose_fused_kernel) against the numpy statement of the rule (evaluate.weighted_query_row), and ``weights="variance"`` through
QueryPose, the two streams, ``outputs="query"`` and the captured map step.

The rows are held to the tolerances the fused kernel already has (test_hip_query_pose._agree: 1e-12 on poses and translation
error, 1e-5 degrees + 1e-9 relative on the rotation error): the weighted combination is convex and runs in the same operation
order on both sides, so it adds nothing beyond the sin / cos difference those tolerances cover.  The spread is held to 1e-12
relative; the integers, ``count`` and the candidates are exact, as are the identities the rule states exactly."""
import numpy as np
import pytest
import torch

from test_consensus_pose_cpu import CONSENSUS_CAP, CONSENSUS_DEG, CONSENSUS_T, consensus_cases, near_a_threshold
from test_hip_consensus_pose import SIZES, _ints
from test_hip_fused_pose import _bits, _outputs
from test_hip_mc_capture import MB, _map, _small, data  # noqa: F401  (data: a fixture; G = 10 queries, K = 3, M = 12)
from test_hip_mc_capture import G, K, M
from test_hip_query_pose import PM, PS, _agree, _agree_results, _fc_case, _Map, dev  # noqa: F401  (dev: a fixture)
from test_weighted_pose_cpu import VAR_SEED, drawn_variances

pytestmark = pytest.mark.gpu

WIDE = dict(inlier_t=2.0, inlier_deg=120.0)               # at the scale of _fc_case's random candidates: some agree, some do not
NAN_ROW, NAN2 = np.full(16, np.nan), np.full(2, np.nan)
P2 = 0.125                                                # variances and floor of the power-of-two identity


def _qp(fuse, max_edges=64, **kw):
    from relpose_gnn_amd.query_pose import QueryPose
    return QueryPose(PM, PS, fuse=fuse, max_edges=max_edges, weights="variance", **kw)


def _plain(fuse, max_edges=64, **kw):
    from relpose_gnn_amd.query_pose import QueryPose
    return QueryPose(PM, PS, fuse=fuse, max_edges=max_edges, **kw)


def _spread(g, dev):
    """The [G, 2] output filled with a pattern the kernel must overwrite everywhere."""
    return torch.full((g, 2), -7.0, dtype=torch.float64, device=dev)


def _var_for(rel, seed):
    return torch.from_numpy(drawn_variances(rel.shape[0], np.random.default_rng(seed)).astype(np.float32)).to(rel.device)


def _host(rel, var, ei, sizes, y, fuse, max_edges=64, **kw):
    """-> (rows [G, 16], spread [G, 2], (inliers, used) [G, 2], near a threshold [G]) of a collated batch by the numpy rule; a NaN
    row, a NaN spread and (0, min(count, max_edges)) for a bad graph.  ``inliers`` is -1 for weighted "mean"."""
    from relpose_gnn_amd import evaluate as E
    rel, var = rel.cpu().numpy().astype(np.float64), var.cpu().numpy().astype(np.float64)
    ei, y = ei.cpu().numpy(), y.cpu().numpy().astype(np.float64)
    first, per_graph = E.edges_per_graph(ei, sizes)
    pm, ps = np.asarray(PM), np.asarray(PS)
    t, deg = kw.get("inlier_t", 0.25), kw.get("inlier_deg", 5.0)
    rows, spreads, ints, near = [], [], [], []
    for k, (n, cols) in enumerate(zip(sizes, per_graph)):
        r, v, target, edges = rel[cols], var[cols], y[first[k]:first[k] + n], ei[:, cols] - first[k]
        with np.errstate(all="ignore"):
            try:
                row, spread, n_in, used = E.weighted_query_row(r, v, target, edges, pm, ps, fuse, max_edges, **kw)
                cands = E.pose_candidates(r, target, edges, pm, ps, max_edges)[0]
                cands[~E.variance_weights(v[E.used_columns(edges, max_edges)])[2]] = np.nan       # (they do not vote)
                near.append(fuse == "consensus" and t > 0 and deg > 0 and near_a_threshold(cands, t, deg))
            except ValueError:
                usable = int(((edges[1] == 0) & (edges[0] != 0)).sum())
                row, spread, n_in, used = NAN_ROW, NAN2, 0, min(usable, max_edges)
                near.append(False)
        rows.append(row)
        spreads.append(spread)
        ints.append((-1 if n_in is None else n_in, used))
    return np.stack(rows), np.stack(spreads), np.array(ints), np.array(near)


def _agree_spread(got, want):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
    assert (np.abs(got[fin] - want[fin]) <= 1e-12 * np.abs(want[fin])).all(), np.abs(got[fin] / want[fin] - 1).max()


def _check(got, spread, ints, want, want_spread, want_ints, near=None):
    keep = np.ones(len(want), dtype=bool) if near is None else ~near
    assert keep.sum() >= (1 - CONSENSUS_CAP) * len(want)
    if ints is not None:
        assert np.array_equal(ints.cpu().numpy()[keep], want_ints[keep]), (ints.cpu().numpy()[keep] != want_ints[keep]).nonzero()
    _agree(got.cpu().numpy()[keep], want[keep])
    _agree_spread(spread.cpu().numpy()[keep], want_spread[keep])


def _run(qp, rel, var, ei, nf, y, ef, g, dev, max_edges=64, check_candidates=True):
    """One weighted call with every optional output -> (rows, spread, ints | None); the candidates and the count are the
    unweighted call's, bit for bit."""
    cand, counts = _outputs(g, max_edges, dev)
    ints = _ints(g, dev) if qp.fuse == "consensus" else None
    spread = _spread(g, dev)
    got = qp.from_targets(rel, ei, nf, y, edge_first=ef, candidates=cand, counts=counts, inliers=ints, rel_var=var, spread=spread)
    if check_candidates:
        cand0, counts0 = _outputs(g, max_edges, dev)
        _plain("mean", max_edges).from_targets(rel, ei, nf, y, edge_first=ef, candidates=cand0, counts=counts0)
        assert torch.equal(_bits(cand), _bits(cand0)) and torch.equal(counts, counts0)
    return got, spread, ints


# ---- the drawn cases ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drawn(dev):  # noqa: F811
    """The 200 graphs of test_consensus_pose_cpu.consensus_cases as one collated batch on the device, with drawn variances."""
    graphs, oracle = consensus_cases()
    sizes = [y.shape[0] for _, y, _ in graphs]
    first = np.concatenate([[0], np.cumsum(sizes)])
    rel = torch.from_numpy(np.concatenate([r for r, _, _ in graphs]).astype(np.float32)).to(dev)
    y = torch.from_numpy(np.concatenate([t for _, t, _ in graphs]).astype(np.float32)).to(dev)
    ei = torch.from_numpy(np.concatenate([e + first[k] for k, (_, _, e) in enumerate(graphs)], 1)).to(dev)
    nf = torch.from_numpy(first).to(dev)
    ef = torch.from_numpy(np.concatenate([[0], np.cumsum([e.shape[1] for _, _, e in graphs])])).to(dev)
    var = _var_for(rel, VAR_SEED)
    near = np.array([o[4] for o in oracle])               # the voting is unweighted: the consensus cases' own flags
    return sizes, (rel, var, ei, nf, ef, y), near


@pytest.mark.parametrize("fuse", ["mean", "consensus"])
def test_drawn_cases_in_one_call(dev, drawn, fuse):  # noqa: F811
    sizes, (rel, var, ei, nf, ef, y), near = drawn
    g = len(sizes)
    kw = dict(inlier_t=CONSENSUS_T, inlier_deg=CONSENSUS_DEG)
    want, want_spread, want_ints, near2 = _host(rel, var, ei, sizes, y, fuse, **kw)
    assert (var == 0).any() and float(var.max()) > 1e-2 and 0 < float(var[var > 0].min()) < 1e-7
    assert np.array_equal(near2, near if fuse == "consensus" else np.zeros(g, dtype=bool)) and near.sum() <= CONSENSUS_CAP * g
    assert np.isfinite(want).all() and np.isfinite(want_spread).all()
    qp = _qp(fuse, **kw)
    for edge_first in (ef, None):                                         # cut by offsets, and by the columns' targets
        got, spread, ints = _run(qp, rel, var, ei, nf, y, edge_first, g, dev, check_candidates=edge_first is not None)
        _check(got, spread, ints, want, want_spread, want_ints, near2)
    if fuse == "consensus":
        assert ints[:, 1].cpu().tolist() == [n - 1 for n in sizes] and len(set(want_ints[:, 0].tolist())) >= 6
    # the weights matter: the unweighted rows differ
    assert not torch.equal(_bits(got), _bits(_plain(fuse, **kw).from_targets(rel, ei, nf, y, edge_first=ef)))
    qp.check()


# ---- shapes where the wave logic can go wrong ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fuse", ["mean", "consensus"])
@pytest.mark.parametrize("sizes", [SIZES[1], SIZES[4], SIZES[5], (3, 66, 8), (65,)], ids=["C1", "g4", "g5", "65-in-edges", "64-candidates"])
def test_fc_graphs_and_every_lane_live(dev, sizes, fuse):  # noqa: F811
    """C = 1, 2 and 7 in a full and a partial workgroup; a 66-node graph (65 edges into its query, 64 used, several 64-column
    steps) between two small ones; a 65-node graph (exactly 64 candidates)."""
    rel, ei, nf, ef, y = _fc_case(sizes, 60 if max(sizes) > 60 else 50 + len(sizes), dev)
    var = _var_for(rel, 7)
    kw = dict(inlier_t=1.6, inlier_deg=100.0) if max(sizes) > 60 else WIDE
    want, want_spread, want_ints, near = _host(rel, var, ei, sizes, y, fuse, **kw)
    assert not near.any() and np.isfinite(want).all() and np.isfinite(want_spread).all()
    qp = _qp(fuse, **kw)
    for edge_first in (ef, None):
        got, spread, ints = _run(qp, rel, var, ei, nf, y, edge_first, len(sizes), dev, check_candidates=edge_first is not None)
        _check(got, spread, ints, want, want_spread, want_ints)
    single0 = _plain(None).from_targets(rel, ei, nf, y, edge_first=ef)
    for k, n in enumerate(sizes):
        if n == 2:                                                        # one candidate: the single-edge rule's row, bit for bit
            assert torch.equal(_bits(got[k]), _bits(single0[k]))
    if max(sizes) > 60 and fuse == "consensus":
        big = int(np.argmax(sizes))
        assert want_ints[big, 1] == 64 and 1 < want_ints[big, 0] < 64
    qp.check()


@pytest.mark.parametrize("fuse", ["mean", "consensus"])
@pytest.mark.parametrize("max_edges", [1, 2, 3])
def test_max_edges_below_the_candidates(dev, max_edges, fuse):  # noqa: F811
    sizes = (8, 5, 3, 2, 12)
    rel, ei, nf, ef, y = _fc_case(sizes, 61, dev)
    var = _var_for(rel, 8)
    want, want_spread, want_ints, near = _host(rel, var, ei, sizes, y, fuse, max_edges, **WIDE)
    assert not near.any()
    qp = _qp(fuse, max_edges, **WIDE)
    got, spread, ints = _run(qp, rel, var, ei, nf, y, ef, 5, dev, max_edges)
    _check(got, spread, ints, want, want_spread, want_ints)
    if max_edges == 1:                                                    # every graph has one candidate: the single-edge rows
        assert torch.equal(_bits(got), _bits(_plain(None).from_targets(rel, ei, nf, y, edge_first=ef)))
    qp.check()


@pytest.mark.parametrize("fuse", ["mean", "consensus"])
def test_the_map_form(dev, fuse):  # noqa: F811
    """Graph g = query g and K rows of a map: the same rule over the other way of finding a source's pose."""
    from relpose_gnn_amd import evaluate as E
    from relpose_gnn_amd.graph import fc_edge_index
    g, k, m = 6, 7, 20
    gen = torch.Generator().manual_seed(12)
    poses, targets = torch.randn(m, 6, generator=gen) * 0.5, torch.randn(g, 6, generator=gen) * 0.5
    nb = torch.stack([torch.randperm(m, generator=gen)[:k] for _ in range(g)])
    edges = fc_edge_index(k + 1)
    ei = torch.cat([edges + j * (k + 1) for j in range(g)], 1)
    rel = torch.randn(ei.shape[1], 6, generator=gen) * 0.3
    var = _var_for(rel, 9).to(dev)
    rows, spreads, ints = [], [], []
    e_g = edges.shape[1]
    for j in range(g):
        target = np.vstack([targets[j].numpy(), poses[nb[j]].numpy()]).astype(np.float64)
        row, sp, n_in, used = E.weighted_query_row(rel[j * e_g:(j + 1) * e_g].numpy().astype(np.float64),
                                                   var[j * e_g:(j + 1) * e_g].cpu().numpy().astype(np.float64), target, edges.numpy(),
                                                   np.asarray(PM), np.asarray(PS), fuse, **WIDE)
        rows.append(row)
        spreads.append(sp)
        ints.append((-1 if n_in is None else n_in, used))
    qp = _qp(fuse, **WIDE)
    got_ints = _ints(g, dev) if fuse == "consensus" else None
    spread = _spread(g, dev)
    ef = torch.arange(g + 1, dtype=torch.int64, device=dev) * e_g
    for edge_first in (ef, None):
        got = qp.from_map(rel.to(dev), ei.to(dev), _Map(poses.to(dev)), nb.to(dev), query_targets=targets.to(dev), edge_first=edge_first,
                          inliers=got_ints, rel_var=var, spread=spread)
        _check(got, spread, got_ints, np.stack(rows), np.stack(spreads), np.array(ints))
    qp.check()


# ---- exact identities on the device ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [tuple(2 + (i * 4) % 9 for i in range(13)), (3, 66, 8), (65,)], ids=["2..10", "65-in-edges", "64"])
def test_equal_power_of_two_weights_are_the_unweighted_rows_bit_for_bit(dev, sizes):  # noqa: F811
    rel, ei, nf, ef, y = _fc_case(sizes, 65, dev)
    g = len(sizes)
    for v, floor in ((P2, P2), (0.0, 2.0 ** -40), (2.0 ** -20, 2.0 ** -20)):
        var = torch.full((rel.shape[0], 6), v, dtype=torch.float32, device=dev)
        spread = _spread(g, dev)
        got = _qp("mean", var_floor=floor).from_targets(rel, ei, nf, y, edge_first=ef, rel_var=var, spread=spread)
        assert torch.equal(_bits(got), _bits(_plain("mean").from_targets(rel, ei, nf, y, edge_first=ef))), (v, floor)
        # ... and the spread is exact too: C weights of 1 / (v + floor) each, 1 / (3 v + floor) for the rotation
        c = np.array([n - 1 for n in sizes], dtype=np.float64).clip(max=64)
        ps = np.asarray(PS)
        want = np.stack([np.sqrt(((ps * ps).sum() * (v + floor)) / c), np.sqrt((3 * v + floor) / c)], 1)
        assert np.allclose(spread.cpu().numpy(), want, rtol=1e-14, atol=0)
        for kw in (WIDE, {}, dict(inlier_t=1e300, inlier_deg=360.0)):
            ia, ib = _ints(g, dev), _ints(g, dev)
            a = _qp("consensus", var_floor=floor, **kw).from_targets(rel, ei, nf, y, edge_first=ef, rel_var=var, inliers=ia)
            b = _plain("consensus", **kw).from_targets(rel, ei, nf, y, edge_first=ef, inliers=ib)
            assert torch.equal(_bits(a), _bits(b)) and torch.equal(ia, ib), (v, floor, kw)


@pytest.mark.parametrize("fuse", ["mean", "consensus"])
def test_deterministic_and_graph_by_graph(dev, fuse):  # noqa: F811
    sizes = tuple(2 + (i * 4) % 9 for i in range(13))
    rel, ei, nf, ef, y = _fc_case(sizes, 65, dev)
    var = _var_for(rel, 10)
    qp = _qp(fuse, **WIDE)
    a = torch.empty((13, 16), dtype=torch.float64, device=dev)
    a.view(torch.uint8).fill_(0xFF)
    b = torch.zeros((13, 16), dtype=torch.float64, device=dev)
    sa, sb = _spread(13, dev), torch.zeros((13, 2), dtype=torch.float64, device=dev)
    assert qp.from_targets(rel, ei, nf, y, edge_first=ef, out=a, rel_var=var, spread=sa) is a
    qp.from_targets(rel, ei, nf, y, edge_first=ef, out=b, rel_var=var, spread=sb)         # a repeated call: the same bits
    assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(sa), _bits(sb)) and torch.isfinite(a).all() and (sa > 0).all()
    for k0, k1 in ((0, 6), (6, 13)):                                      # the batch split in two calls
        e0, e1, n0, n1 = int(ef[k0]), int(ef[k1]), int(nf[k0]), int(nf[k1])
        sp = _spread(k1 - k0, dev)
        part = qp.from_targets(rel[e0:e1].contiguous(), (ei[:, e0:e1] - n0).contiguous(), (nf[k0:k1 + 1] - n0).contiguous(),
                               y[n0:n1].contiguous(), edge_first=(ef[k0:k1 + 1] - e0).contiguous(), rel_var=var[e0:e1].contiguous(),
                               spread=sp)
        assert torch.equal(_bits(part), _bits(a[k0:k1])) and torch.equal(_bits(sp), _bits(sa[k0:k1]))
    for k, n in enumerate(sizes):                                         # every graph alone
        e0, e1, n0 = int(ef[k]), int(ef[k + 1]), int(nf[k])
        sp = _spread(1, dev)
        one = qp.from_targets(rel[e0:e1].contiguous(), (ei[:, e0:e1] - n0).contiguous(), torch.tensor([0, n], device=dev),
                              y[n0:n0 + n].contiguous(), rel_var=var[e0:e1].contiguous(), spread=sp)
        assert torch.equal(_bits(one[0]), _bits(a[k])) and torch.equal(_bits(sp[0]), _bits(sa[k])), k
    # captured and replayed: one launch, no allocation, no synchronisation
    out, sp = torch.zeros_like(a), _spread(13, dev)
    qp.check()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        qp.from_targets(rel, ei, nf, y, edge_first=ef, out=out, rel_var=var, spread=sp)
    out.zero_()
    sp.fill_(-7.0)
    graph.replay()
    qp.publish()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(a)) and torch.equal(_bits(sp), _bits(sa))
    qp.check()


# ---- variances that cannot be used, non-finite candidates, bad graphs ------------------------------------------------------------------
@pytest.mark.parametrize("value", [float("nan"), float("inf"), -1.0], ids=["nan", "pinf", "negative"])
def test_unusable_variances(dev, value):  # noqa: F811
    sizes = (8, 8, 4, 3, 2, 5, 2)
    rel, ei, nf, ef, y = _fc_case(sizes, 64, dev)
    var = _var_for(rel, 11)
    dst = ei[1].cpu().numpy()
    bad = var.clone()
    bad[np.flatnonzero(dst == 0)[3], 1] = value           # graph 0: translation variance of used candidate 3
    bad[np.flatnonzero(dst == 8)[6], 4] = value           # graph 1: rotation variance of the last used candidate
    bad[np.flatnonzero(dst == 17), 0] = value             # graph 2 (nodes 16..19): columns that are no edge into its query
    bad[np.flatnonzero(dst == 20)[:], 2] = value          # graph 3 (nodes 20..22): EVERY used edge
    bad[np.flatnonzero(dst == 23)[0], 5] = value          # graph 4 (nodes 23, 24): its only candidate
    rel2 = rel.clone()
    rel2[np.flatnonzero(dst == 30)[0], 4] = float("nan")  # graph 6 (nodes 30, 31): its only candidate has a NaN rotation itself
    for fuse in ("mean", "consensus"):
        qp = _qp(fuse, **WIDE)
        clean, clean_sp, _ = _run(qp, rel, var, ei, nf, y, ef, 7, dev)
        want, want_spread, want_ints, near = _host(rel2, bad, ei, sizes, y, fuse, **WIDE)
        assert not near.any()
        got, spread, ints = _run(qp, rel2, bad, ei, nf, y, ef, 7, dev)
        _check(got, spread, ints, want, want_spread, want_ints)
        qp.check()                                        # neither is a bad graph: the status is untouched
        got, spread = got.cpu().numpy(), spread.cpu().numpy()
        assert torch.equal(_bits(torch.from_numpy(got[[2, 5]])), _bits(clean[[2, 5]].cpu()))      # untouched graphs
        assert np.array_equal(spread[[2, 5]], clean_sp[[2, 5]].cpu().numpy()) and np.isfinite(got[:, 7:14]).all()
        if fuse == "mean":
            # C >= 2: voided; C = 1: the candidate as it is, without a deviation
            assert np.isnan(got[[0, 1, 3], :7]).all() and np.isnan(got[[0, 1, 3], 14:]).all() and np.isnan(spread[[0, 1, 3, 4, 6]]).all()
            assert torch.equal(_bits(torch.from_numpy(got[4])), _bits(clean[4].cpu())) and np.isnan(got[6, 3:7]).all() and got[6, 15] == 360.0
        else:
            # the planted candidate is an outlier, the rest of the graph's consensus stands; nothing usable: NaN and 0 inliers
            assert np.isfinite(got[:2]).all() and np.isfinite(spread[:2]).all() and ints[:2, 1].tolist() == [7, 7]
            for k, used in ((3, 2), (4, 1), (6, 1)):
                assert np.isnan(got[k, :7]).all() and np.isnan(got[k, 14:]).all() and np.isnan(spread[k]).all()
                assert ints[k].tolist() == [0, used]
    # a variance beyond the cut is not read into anything
    cut = _qp("mean", 3)
    a = cut.from_targets(rel, ei, nf, y, edge_first=ef, rel_var=var)
    v2 = var.clone()
    v2[np.flatnonzero(dst == 0)[3:], :] = value
    assert torch.equal(_bits(a), _bits(cut.from_targets(rel, ei, nf, y, edge_first=ef, rel_var=v2)))


@pytest.mark.parametrize("fuse", ["mean", "consensus"])
def test_bad_graphs_are_nan_rows_with_a_nan_spread(dev, fuse):  # noqa: F811
    from relpose_gnn_amd import ops
    sizes = (8, 3, 8, 4, 5)
    rel, ei, nf, ef, y = _fc_case(sizes, 63, dev)
    var = _var_for(rel, 12)
    kw = dict(fuse=fuse, weights="variance", rel_var=var, node_first=nf, node_targets=y, edge_first=ef, pose_m=PM, pose_s=PS, **WIDE)
    good_sp = _spread(5, dev)
    good = ops.query_pose_fused(rel, ei, spread=good_sp, **kw)
    dst = ei[1].cpu().numpy()
    # graph 1 (nodes 8..10): no edge into its query; graph 3 (nodes 19..22): only self-edges into it
    no_in = ei.clone()
    no_in[1, np.flatnonzero(dst == 8)] = 9
    no_in[0, np.flatnonzero(dst == 19)] = 19
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    sp = _spread(5, dev)
    ints = _ints(5, dev) if fuse == "consensus" else None
    got = ops.query_pose_fused(rel, no_in, status=status, spread=sp, inliers=ints, **kw)
    assert int(status) == 2 and torch.isnan(got[[1, 3]]).all() and torch.isnan(sp[[1, 3]]).all()
    assert torch.equal(_bits(got[[0, 2, 4]]), _bits(good[[0, 2, 4]])) and torch.equal(_bits(sp[[0, 2, 4]]), _bits(good_sp[[0, 2, 4]]))
    want, want_spread, want_ints, _ = _host(rel, var, no_in, sizes, y, fuse, **WIDE)
    _check(got, sp, ints, want, want_spread, want_ints)
    # graph 2 (nodes 11..18): a used edge starts in another graph
    outside = ei.clone()
    outside[0, np.flatnonzero(dst == 11)[3]] = 19
    got = ops.query_pose_fused(rel, outside, status=status, spread=sp, inliers=ints, **kw)
    assert int(status) == 3 and torch.isnan(got[2]).all() and torch.isnan(sp[2]).all()
    assert torch.equal(_bits(got[[0, 1, 3, 4]]), _bits(good[[0, 1, 3, 4]]))
    with pytest.raises(ValueError, match="no edge into node 0"):
        ops.query_pose_fused(rel, no_in, **kw)
    qp = _qp(fuse, **WIDE)
    qp.from_targets(rel, no_in, nf, y, edge_first=ef, rel_var=var)
    with pytest.raises(ValueError, match="no edge into node 0"):
        qp.check(wait=True)


# ---- the model: the small model and map of the Monte-Carlo tests -----------------------------------------------------------------------
KW = dict(pose_m=PM, pose_s=PS, inlier_t=1e300, inlier_deg=120.0)


@pytest.fixture(scope="module")
def setup(dev, data):  # noqa: F811
    m = _small(dev)
    return m, _map(m, data)


def _fields(r):
    return np.concatenate([r.pred_poses, r.targ_poses, r.t_loss[:, None], r.q_loss[:, None]], 1)


def _same(a, b, fields=("pred_poses", "targ_poses", "t_loss", "q_loss", "neighbours", "sigma_t", "sigma_q")):
    for f in fields:
        x, y = getattr(a, f), getattr(b, f)
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), f


@pytest.mark.parametrize("fuse", ["mean", "consensus"])
def test_relocalize_host_device_capture_and_bytes(dev, data, setup, fuse):  # noqa: F811
    from relpose_gnn_amd.evaluate import relocalize
    m, fmap = setup
    q, nb, targets = data["queries"], data["nb"], data["targets"]
    kw = dict(KW, micro_batch=MB, targets=targets, fuse=fuse, weights="variance")
    m.refresh_packed()                                                    # (drops the steps other tests left on the shared model)

    def run(draw=0, **more):
        m.mc_dropout.reset(draw)
        return relocalize(m, fmap, q, nb, **dict(kw, **more))
    sh, sd, su = {}, {}, {}
    host = run(stats=sh)
    devr = run(stats=sd, postprocess="device")
    _agree_results(devr, host)
    _agree_spread(np.stack([devr.sigma_t, devr.sigma_q], 1), np.stack([host.sigma_t, host.sigma_q], 1))
    assert np.isfinite(host.sigma_t).all() and (host.sigma_t > 0).all() and (host.sigma_q > 0).all()
    if fuse == "consensus":
        assert np.array_equal(devr.inliers, host.inliers) and np.array_equal(devr.used, host.used) and host.used.tolist() == [K] * G
    else:
        assert devr.inliers is None and host.used is None
    # the bytes: 16 more per query than the unweighted rule
    unweighted = run(stats=su, postprocess="device", weights=None)
    per_graph = 144 if fuse == "mean" else 152
    assert sd["d2h_bytes"] == G * per_graph == su["d2h_bytes"] + 16 * G and sd["d2h_bytes"] < sh["d2h_bytes"]
    assert unweighted.sigma_t is None and not np.array_equal(unweighted.pred_poses, devr.pred_poses)
    # without targets: the poses as before, the two arrays in stats
    st = {}
    pred = run(stats=st, postprocess="device", targets=None)
    assert np.array_equal(pred, devr.pred_poses) and np.array_equal(st["sigma_t"], devr.sigma_t) and np.array_equal(st["sigma_q"], devr.sigma_q)
    # capture=True: bit-identical rows and spread from the same draw, two shapes (a full micro-batch and the tail)
    sc = {}
    cap = run(capture=True, stats=sc, postprocess="device")
    _same(cap, devr)
    assert sc["graphs_captured"] == 2 and sc["graph_replays"] == 3 and sc["d2h_bytes"] == sd["d2h_bytes"]
    _same(run(capture=True, stats=sc, postprocess="device", draw=1), run(postprocess="device", draw=1))
    assert sc["graphs_captured"] == 0                                     # the same rule again: nothing to capture
    # the host rule on the captured step's own variances
    _agree_results(run(capture=True, stats=sc), host)
    # another floor, or no weights: a new step is captured, not the old one replayed
    other = run(capture=True, stats=sc, postprocess="device", var_floor=1e-3)
    assert sc["graphs_captured"] == 2 and not np.array_equal(other.pred_poses, cap.pred_poses)
    _same(other, run(postprocess="device", var_floor=1e-3))
    plain = run(capture=True, stats=sc, postprocess="device", weights=None)
    assert sc["graphs_captured"] == 2 and np.array_equal(plain.pred_poses, unweighted.pred_poses)
    m.check_edge_index()


def test_captured_step_replays_the_eager_rule_and_exposes_the_spread(dev, data, setup):  # noqa: F811
    """Replay i against the eager forward of draw i and the eager rule on ITS variances, bit for bit; ``step.sigma`` is static."""
    from relpose_gnn_amd.graphed import GraphedForwardMap, MapStep
    from relpose_gnn_amd.query_pose import QueryPose
    m, fmap = setup
    q, nb, targets = data["queries"][:MB].to(dev), data["nb"][:MB].contiguous().to(dev), data["targets"][:MB].to(dev)
    for outputs in ("all", "query"):
        rule = dict(fuse="consensus", weights="variance", inlier_t=1e300, inlier_deg=120.0)
        pose, eager = QueryPose(PM, PS, **rule), QueryPose(PM, PS, **rule)
        m.mc_dropout.reset(0)
        step = GraphedForwardMap(m, fmap, q, K, pose=pose, pose_kwargs={"query_targets": targets}, outputs=outputs)
        assert MapStep._fields == ("abs_pose", "rel_pose", "edge_index", "neighbours", "rows")
        assert step.sigma.shape == (MB, 2) and step.sigma.dtype == torch.float64 and step.inliers.shape == (MB, 2)
        assert step.packed.numel() == MB * 152
        want = []
        for i in range(3):
            m.mc_dropout.reset(i)
            ab, rel, ei = m.forward_map(q, nb, fmap, outputs=outputs)
            ints, sp = _ints(MB, dev), _spread(MB, dev)
            rows = eager.from_map(rel, ei, fmap, nb, query_targets=targets, inliers=ints, rel_var=m.mc_dropout.last.rel_var, spread=sp)
            want.append((rows.clone(), ints, sp))
        m.mc_dropout.reset(0)
        sigma = step.sigma
        for i in range(3):
            out = step(q, nb, query_targets=targets)
            assert step.sigma is sigma and m.mc_dropout.last is step.spread
            assert torch.equal(_bits(out.rows), _bits(want[i][0])) and torch.equal(step.inliers, want[i][1]), (outputs, i)
            assert torch.equal(_bits(step.sigma), _bits(want[i][2])) and torch.isfinite(step.sigma).all(), (outputs, i)
        assert not torch.equal(want[0][2], want[1][2])                    # consecutive draws differ
        pose.check()
    assert GraphedForwardMap(m, fmap, q, K, pose=QueryPose(PM, PS, fuse="mean")).sigma is None
    m.check_edge_index()


def test_both_output_modes_give_the_same_rows(dev, data, setup):  # noqa: F811
    """``rel_var`` is row for row with the reduced ``rel_pose``: the rule over the K columns into every query of an
    ``outputs="all"`` forward, cut out as ``outputs="query"`` returns them, gives the bits of the rule over the full list.  (The two
    FORWARDS agree only as differently tiled GEMMs do -- test_hip_mc_model holds them to 1e-4 and their variances to 1e-3 -- so
    the streams of the two modes are compared through the rule on one forward, and each against its own host path.)"""
    from relpose_gnn_amd.evaluate import relocalize
    from relpose_gnn_amd.query_pose import QueryPose
    m, fmap = setup
    q, nb, targets = data["queries"].to(dev), data["nb"].contiguous().to(dev), data["targets"].to(dev)
    m.mc_dropout.reset(0)
    ab, rel, ei = m.forward_map(q, nb, fmap)
    var = m.mc_dropout.last.rel_var
    cols = torch.isin(ei[1], torch.arange(G, device=dev) * (K + 1))
    assert int(cols.sum()) == G * K
    for fuse in ("mean", "consensus"):
        qp = QueryPose(PM, PS, fuse=fuse, weights="variance", inlier_t=1e300, inlier_deg=120.0)
        sa, sb = _spread(G, dev), _spread(G, dev)
        a = qp.from_map(rel, ei, fmap, nb, query_targets=targets, rel_var=var, spread=sa)
        b = qp.from_map(rel[cols].contiguous(), ei[:, cols].contiguous(), fmap, nb, query_targets=targets,
                        rel_var=var[cols].contiguous(), spread=sb, edge_first=torch.arange(G + 1, device=dev) * K)
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(sa), _bits(sb)) and torch.isfinite(sa).all()
        qp.check()
        # the stream of the reduced mode: its device path against its host path
        kw = dict(KW, micro_batch=MB, targets=data["targets"], fuse=fuse, weights="variance", outputs="query")
        m.mc_dropout.reset(0)
        host = relocalize(m, fmap, data["queries"], data["nb"], **kw)
        m.mc_dropout.reset(0)
        devr = relocalize(m, fmap, data["queries"], data["nb"], postprocess="device", **kw)
        _agree_results(devr, host)
        _agree_spread(np.stack([devr.sigma_t, devr.sigma_q], 1), np.stack([host.sigma_t, host.sigma_q], 1))
        m.mc_dropout.reset(0)
        _same(relocalize(m, fmap, data["queries"], data["nb"], postprocess="device", capture=True, **kw), devr)


def test_one_sample_under_a_power_of_two_floor_is_the_unweighted_mean(dev, data):  # noqa: F811
    """McDropout(samples=1) leaves variances of exactly 0: with var_floor = 2^-40 every weight is 2^40 and the rows are those of
    the unweighted rules bit for bit -- eagerly and from a captured step.  (The streams refuse one sample: it has no variance.)"""
    from relpose_gnn_amd.evaluate import relocalize
    from relpose_gnn_amd.graphed import GraphedForwardMap
    from relpose_gnn_amd.mc_dropout import McDropout
    from relpose_gnn_amd.query_pose import QueryPose
    m = _small(dev)
    m.mc_dropout = McDropout(samples=1, seed=5)
    fmap = _map(m, data)
    q, nb, targets = data["queries"][:MB].to(dev), data["nb"][:MB].contiguous().to(dev), data["targets"][:MB].to(dev)
    for fuse in ("mean", "consensus"):
        rule = dict(fuse=fuse, inlier_t=1e300, inlier_deg=120.0)
        m.mc_dropout.reset(0)
        ab, rel, ei = m.forward_map(q, nb, fmap)
        var = m.mc_dropout.last.rel_var
        assert var.shape == rel.shape and not var.any()
        want = QueryPose(PM, PS, **rule).from_map(rel, ei, fmap, nb, query_targets=targets)
        weighted = QueryPose(PM, PS, weights="variance", var_floor=2.0 ** -40, **rule)
        sp = _spread(MB, dev)
        got = weighted.from_map(rel, ei, fmap, nb, query_targets=targets, rel_var=var, spread=sp)
        assert torch.equal(_bits(got), _bits(want)) and torch.isfinite(sp).all()
        m.mc_dropout.reset(0)
        step = GraphedForwardMap(m, fmap, q, K, pose=weighted, pose_kwargs={"query_targets": targets})
        assert torch.equal(_bits(step(q, nb, query_targets=targets).rows), _bits(want))
    with pytest.raises(ValueError, match="mc_dropout"):
        relocalize(m, fmap, data["queries"], data["nb"], fuse="mean", weights="variance", postprocess="device")
    m.check_edge_index()


def test_relocalize_does_not_depend_on_micro_batch(dev, data, setup):  # noqa: F811
    """The masks follow the node ids, so micro-batches of 2 and of 5 see the same samples; their forwards differ as differently
    tiled GEMMs do.  The bar: test_hip_mc_model holds the poses of two such forwards to 1e-4 of the column's largest value and
    their variances to 1e-3 of the largest variance.  With a floor AT that largest variance every weight 1 / (v + floor) moves
    by at most 1e-3 relative, a convex combination moves by no more than its candidates do plus the weights' relative move
    times the candidates' spread (under twice the column's largest value), and sigma, the root of a sum of such weights, by
    half of it: (1e-4 + 2e-3) of the column's largest value bounds every column."""
    from relpose_gnn_amd.evaluate import relocalize
    m, fmap = setup
    m.mc_dropout.reset(0)
    m.forward_map(data["queries"].to(dev), data["nb"].contiguous().to(dev), fmap)
    floor = float(m.mc_dropout.last.rel_var.max())
    assert floor > 0
    res = {}
    for mb in (2, 5):
        m.mc_dropout.reset(0)
        r = relocalize(m, fmap, data["queries"], data["nb"], micro_batch=mb, postprocess="device", targets=data["targets"], fuse="mean",
                       weights="variance", var_floor=floor, **KW)
        res[mb] = np.concatenate([r.pred_poses, r.t_loss[:, None], r.sigma_t[:, None], r.sigma_q[:, None]], 1)
        assert m.mc_dropout.draw == 1
    a, b = res[2], res[5]
    assert np.isfinite(b).all()
    for col in range(a.shape[1]):
        assert np.abs(a[:, col] - b[:, col]).max() <= 2.1e-3 * np.abs(b[:, col]).max(), col
    m.mc_dropout.reset(1)
    nxt = relocalize(m, fmap, data["queries"], data["nb"], micro_batch=5, postprocess="device", targets=data["targets"], fuse="mean",
                     weights="variance", var_floor=floor, **KW)
    assert not np.array_equal(nxt.sigma_t, r.sigma_t)                     # the next draw: other samples, other variances


@pytest.mark.parametrize("fuse", ["mean", "consensus"])
def test_evaluate_stream_device_equals_host(dev, data, setup, fuse):  # noqa: F811
    from relpose_gnn_amd.evaluate import evaluate_stream
    from relpose_gnn_amd.graph import Data, fc_edge_index
    m, _ = setup
    gen = torch.Generator().manual_seed(3)
    imgs = data["queries"].reshape(G, -1)
    graphs = [Data(x=imgs[torch.randperm(G, generator=gen)[:4]], edge_index=fc_edge_index(4), y=torch.randn(4, 6, generator=gen) * 0.3)
              for _ in range(5)]
    kw = dict(KW, micro_batch=2, fuse=fuse, weights="variance")
    sh, sd = {}, {}
    m.mc_dropout.reset(0)
    host = evaluate_stream(m, graphs, dev, stats=sh, **kw)
    m.mc_dropout.reset(0)
    devr = evaluate_stream(m, graphs, dev, stats=sd, postprocess="device", **kw)
    _agree_results(devr, host)
    _agree_spread(np.stack([devr.sigma_t, devr.sigma_q], 1), np.stack([host.sigma_t, host.sigma_q], 1))
    assert np.isfinite(host.sigma_t).all() and sd["d2h_bytes"] == 5 * (144 if fuse == "mean" else 152) and sd["d2h_bytes"] < sh["d2h_bytes"]
    if fuse == "consensus":
        assert np.array_equal(devr.inliers, host.inliers) and host.used.tolist() == [3] * 5
    # the unweighted stream of the same draw: other poses, no deviations
    m.mc_dropout.reset(0)
    plain = evaluate_stream(m, graphs, dev, postprocess="device", **dict(kw, weights=None))
    assert plain.sigma_t is None and not np.array_equal(plain.pred_poses, devr.pred_poses)
    m.check_edge_index()
