"""All of a query's reference edges fused into one pose on the GPU (rpg_query_pose_fused_f64 / ops.query_pose_fused /
QueryPose(fuse=...), and ``fuse=`` of the two evaluation streams with postprocess="device") against the numpy statement of the
rule, evaluate.fused_query_row, on the same fp32 tensors.

Tolerances: those of test_hip_query_pose.py, for its reasons -- 1e-12 on poses and the translation error, 1e-5 degrees + 1e-9
relative on rotation errors (acos is ill-conditioned at 1), equal non-finite patterns.  The fused pose adds at most 64 double
additions and one division to a candidate, ~1e-14 on values of order 1 to 10, far inside 1e-12.  What must be EXACT is held
exactly: the candidates against the single-edge kernel, graphs with one candidate, the counts, the medoid's index, repeated and
split calls."""
import numpy as np
import pytest
import torch

from test_fused_pose_cpu import MEDOID_CAP, MEDOID_GAP, medoid_cases
from test_hip_query_pose import PM, PS, _agree, _agree_results, _fc_case, _Map, dev, models  # noqa: F401  (dev, models: fixtures)

pytestmark = pytest.mark.gpu

MODES = ("mean", "median")
NAN_ROW = np.full(16, np.nan)


def _qp(fuse, max_edges=64):
    from relpose_gnn_amd.query_pose import QueryPose
    return QueryPose(PM, PS, fuse=fuse, max_edges=max_edges)


def _single(ref_node):
    from relpose_gnn_amd.query_pose import QueryPose
    return QueryPose(PM, PS, ref_node)


def _host_row(rel, target, edges, fuse, max_edges=64):
    from relpose_gnn_amd import evaluate as E
    try:
        with np.errstate(all="ignore"):
            return E.fused_query_row(rel, target, edges, np.asarray(PM), np.asarray(PS), fuse, max_edges)
    except ValueError:
        return NAN_ROW


def _host_rows(rel, ei, sizes, y, fuse, max_edges=64):
    """[G, 16] of a collated batch by the numpy rule, cut per graph by the columns' targets; NaN rows for bad graphs."""
    from relpose_gnn_amd import evaluate as E
    rel, ei, y = rel.cpu().numpy(), ei.cpu().numpy(), y.cpu().numpy()
    first, per_graph = E.edges_per_graph(ei, sizes)
    return np.stack([_host_row(rel[cols], y[first[k]:first[k] + n], ei[:, cols] - first[k], fuse, max_edges)
                     for k, (n, cols) in enumerate(zip(sizes, per_graph))])


def _bits(t):
    return t.contiguous().view(torch.int64)


def _outputs(g, max_edges, dev):
    """Candidate and count tensors filled with a pattern the kernel must overwrite everywhere."""
    cand = torch.empty((g, max_edges, 16), dtype=torch.float64, device=dev)
    cand.view(torch.uint8).fill_(0x5A)
    return cand, torch.full((g,), -7, dtype=torch.int32, device=dev)


def _check_candidates(cand, counts, rel, ei, nf, ef, y, sizes, max_edges=64):
    """cand[g, c] is the single-edge kernel's row at ref_node = c, bit for bit; NaN past the graph's candidates; the counts."""
    assert counts.cpu().tolist() == [n - 1 for n in sizes]
    used = [min(n - 1, max_edges) for n in sizes]
    for c in range(max(used)):
        single = _single(c)
        rows = single.from_targets(rel, ei, nf, y, edge_first=ef)
        for k, u in enumerate(used):
            if c < u:
                assert torch.equal(_bits(cand[k, c]), _bits(rows[k])), (k, c)
        if any(c >= n - 1 for n in sizes):
            with pytest.raises(ValueError):
                single.check()
    for k, u in enumerate(used):
        assert torch.isnan(cand[k, u:]).all(), k


SIZES = {1: (8,), 4: (2, 3, 8, 5), 5: (8, 2, 3, 8, 4)}          # C = 1, 2 and 7 (and 3, 4); a full and a partial workgroup


@pytest.mark.parametrize("fuse", MODES)
@pytest.mark.parametrize("g", [1, 4, 5])
def test_fc_graphs(dev, g, fuse):  # noqa: F811
    sizes = SIZES[g]
    rel, ei, nf, ef, y = _fc_case(sizes, 50 + g, dev)
    want = _host_rows(rel, ei, sizes, y, fuse)
    assert np.isfinite(want).all()
    qp = _qp(fuse)
    single0 = _single(0).from_targets(rel, ei, nf, y, edge_first=ef)
    for edge_first in (ef, None):                                         # cut by offsets, and by the columns' targets
        cand, counts = _outputs(g, 64, dev)
        got = qp.from_targets(rel, ei, nf, y, edge_first=edge_first, candidates=cand, counts=counts)
        _agree(got, want)
        _check_candidates(cand, counts, rel, ei, nf, ef, y, sizes)
        for k, n in enumerate(sizes):
            if n == 2:                                                    # one candidate: the single-edge rule's row, bit for bit
                assert torch.equal(_bits(got[k]), _bits(single0[k]))
    qp.check()
    assert torch.equal(_bits(qp.from_targets(rel, ei, nf, y, edge_first=ef)), _bits(got))      # without the optional outputs


@pytest.mark.parametrize("fuse", MODES)
def test_more_in_edges_than_lanes_and_than_one_step(dev, fuse):  # noqa: F811
    """A 66-node graph has 65 edges into its query: 64 are used, count says 65, and they lie in several 64-column steps; two
    small graphs share the call."""
    sizes = (3, 66, 8)
    rel, ei, nf, ef, y = _fc_case(sizes, 60, dev)
    hits = np.flatnonzero(ei[1].cpu().numpy() == 3)
    assert len(hits) == 65 and len(set(hits // 64)) > 3
    want = _host_rows(rel, ei, sizes, y, fuse)
    cut = _host_rows(rel, ei, sizes, y, fuse, 64)
    assert np.array_equal(want, cut) and np.isfinite(want).all()
    dropped = ei.clone()                                                  # the 65th edge is not used: bend it away, same rows
    dropped[1, hits[64]] = 4
    assert np.array_equal(_host_rows(rel, dropped, sizes, y, fuse)[1], want[1])
    qp = _qp(fuse)
    for edge_first in (ef, None):
        cand, counts = _outputs(3, 64, dev)
        got = qp.from_targets(rel, ei, nf, y, edge_first=edge_first, candidates=cand, counts=counts)
        _agree(got, want)
        assert counts.cpu().tolist() == [2, 65, 7]
        assert torch.isfinite(cand[1]).all() and torch.isnan(cand[0, 2:]).all() and torch.isnan(cand[2, 7:]).all()
    for c in (0, 31, 63):
        assert torch.equal(_bits(cand[1, c]), _bits(_single(c).from_targets(rel, ei, nf, y, edge_first=ef)[1]))
    qp.check()


def test_exactly_64_candidates_fill_the_mean(dev):  # noqa: F811
    """A 65-node graph alone: exactly 64 candidates, one per lane and none cut -- the mean runs over the full slot mask."""
    sizes = (65,)
    rel, ei, nf, ef, y = _fc_case(sizes, 60, dev)
    want = _host_rows(rel, ei, sizes, y, "mean")
    assert np.isfinite(want).all()
    qp = _qp("mean")
    for edge_first in (ef, None):
        cand, counts = _outputs(1, 64, dev)
        _agree(qp.from_targets(rel, ei, nf, y, edge_first=edge_first, candidates=cand, counts=counts), want)
        assert counts.cpu().tolist() == [64] and torch.isfinite(cand).all()
    qp.check()


@pytest.mark.parametrize("fuse", MODES)
@pytest.mark.parametrize("max_edges", [1, 2, 4])
def test_max_edges_below_the_candidates(dev, fuse, max_edges):  # noqa: F811
    sizes = (8, 5, 3, 2, 12)
    rel, ei, nf, ef, y = _fc_case(sizes, 61, dev)
    qp = _qp(fuse, max_edges)
    cand, counts = _outputs(5, max_edges, dev)
    got = qp.from_targets(rel, ei, nf, y, edge_first=ef, candidates=cand, counts=counts)
    _agree(got, _host_rows(rel, ei, sizes, y, fuse, max_edges))
    _check_candidates(cand, counts, rel, ei, nf, ef, y, sizes, max_edges)
    if max_edges == 1:                                                    # every graph has one candidate: the single-edge rows
        assert torch.equal(_bits(got), _bits(_single(0).from_targets(rel, ei, nf, y, edge_first=ef)))
    qp.check()


@pytest.mark.parametrize("fuse", MODES)
def test_model_built_knn_list(dev, fuse):  # noqa: F811
    from relpose_gnn_amd import ops
    gen = torch.Generator().manual_seed(7)
    feat = torch.randn(24, 16, generator=gen).to(dev)
    batch = torch.arange(3).repeat_interleave(8).to(dev)
    ei = ops.knn_graph(feat, 4, batch)                                    # the model's own knn = 4 list of 3 graphs of 8 nodes
    rel = (torch.randn(96, 6, generator=gen) * 0.3).to(dev)
    y = (torch.randn(24, 6, generator=gen) * 0.5).to(dev)
    nf = torch.tensor([0, 8, 16, 24], device=dev)
    qp = _qp(fuse)
    counts = torch.zeros(3, dtype=torch.int32, device=dev)
    _agree(qp.from_targets(rel, ei, nf, y, counts=counts), _host_rows(rel, ei, (8, 8, 8), y, fuse))
    assert counts.cpu().tolist() == [4, 4, 4]
    qp.check()


@pytest.mark.parametrize("fuse", MODES)
def test_a_self_edge_is_skipped(dev, fuse):  # noqa: F811
    sizes = (4, 5)
    rel, ei, nf, ef, y = _fc_case(sizes, 62, dev)
    clean = _qp(fuse).from_targets(rel, ei, nf, y, edge_first=ef)
    first_hit = int(np.flatnonzero(ei[1].cpu().numpy() == 4)[0])          # graph 1: a self-edge 4 -> 4 before its first in-edge
    ei2 = torch.cat([ei[:, :first_hit], torch.tensor([[4], [4]], device=dev), ei[:, first_hit:]], 1).contiguous()
    rel2 = torch.cat([rel[:first_hit], torch.full((1, 6), 7.0, device=dev), rel[first_hit:]]).contiguous()
    ef2 = ef + torch.tensor([0, 0, 1], device=dev)
    qp = _qp(fuse)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    for edge_first in (ef2, None):
        got = qp.from_targets(rel2, ei2, nf, y, edge_first=edge_first, counts=counts)
        assert torch.equal(_bits(got), _bits(clean)) and counts.cpu().tolist() == [3, 4]
        _agree(got, _host_rows(rel2, ei2, sizes, y, fuse))
    qp.check()


def _map_rows(rel, nb, poses, targets, fuse, m, max_edges=64):
    from relpose_gnn_amd.graph import fc_edge_index
    g, k = nb.shape
    edges = fc_edge_index(k + 1).numpy()
    e_g = edges.shape[1]
    rows = []
    for j in range(g):
        target = np.zeros((k + 1, 6))
        target[1:] = poses.cpu().numpy().astype(np.float64)[np.clip(nb[j].cpu().numpy(), 0, m - 1)]
        if targets is not None:
            target[0] = targets[j].cpu().numpy()
        rows.append(_host_row(rel[j * e_g:(j + 1) * e_g].cpu().numpy(), target, edges, fuse, max_edges))
    return np.stack(rows)


@pytest.mark.parametrize("fuse", MODES)
@pytest.mark.parametrize("k", [7, 1])
def test_map_form(dev, k, fuse):  # noqa: F811
    from relpose_gnn_amd.graph import fc_batch
    g, m = 5, 16
    gen = torch.Generator().manual_seed(70 + k)
    poses = (torch.randn(m, 6, generator=gen) * 0.5).to(dev)
    targets = (torch.randn(g, 6, generator=gen) * 0.5).to(dev)
    nb = torch.randint(0, m, (g, k), generator=gen).to(dev)
    ei = fc_batch(torch.empty((g * (k + 1), 0)), k + 1).edge_index.to(dev)
    rel = (torch.randn(ei.shape[1], 6, generator=gen) * 0.3).to(dev)
    ef = (torch.arange(g + 1) * (k + 1) * k).to(dev)
    qp = _qp(fuse)
    for tg in (targets, None):
        want = _map_rows(rel, nb, poses, tg, fuse, m)
        cand, counts = _outputs(g, 64, dev)
        got = qp.from_map(rel, ei, _Map(poses), nb, query_targets=tg, edge_first=ef, candidates=cand, counts=counts)
        _agree(got, want)
        _agree(qp.from_map(rel, ei, _Map(poses), nb, query_targets=tg), want)
        assert counts.cpu().tolist() == [k] * g and torch.isnan(cand[:, k:]).all()
        for c in range(k):
            assert torch.equal(_bits(cand[:, c]), _bits(_single(c).from_map(rel, ei, _Map(poses), nb, query_targets=tg, edge_first=ef)))
        if k == 1:
            assert torch.equal(_bits(got), _bits(cand[:, 0]))
    # a neighbour outside [0, M): no fault, the row of the clamped index (as the single-edge kernel)
    for bad, clamped in ((m + 1000, m - 1), (-3, 0)):
        nb_bad, nb_ok = nb.clone(), nb.clone()
        nb_bad[2, k - 1], nb_ok[2, k - 1] = bad, clamped
        got = qp.from_map(rel, ei, _Map(poses), nb_bad, query_targets=targets, edge_first=ef)
        assert torch.equal(_bits(got), _bits(qp.from_map(rel, ei, _Map(poses), nb_ok, query_targets=targets, edge_first=ef)))
    qp.check()


def test_medoid_index_equals_the_oracles(dev):  # noqa: F811
    """The drawn cases of test_fused_pose_cpu.medoid_cases in one call: the fused quaternion IS one of the candidates, and it is
    the oracle's one.  Cases whose two best angle sums are closer than 1e-6 degrees are left out, at most 5 % of them."""
    graphs, oracle = medoid_cases()
    sizes = [y.shape[0] for _, y, _ in graphs]
    first = np.concatenate([[0], np.cumsum(sizes)])
    rel = torch.from_numpy(np.concatenate([r for r, _, _ in graphs]).astype(np.float32)).to(dev)
    y = torch.from_numpy(np.concatenate([t for _, t, _ in graphs]).astype(np.float32)).to(dev)
    ei = torch.from_numpy(np.concatenate([e + first[k] for k, (_, _, e) in enumerate(graphs)], 1)).to(dev)
    nf = torch.from_numpy(first).to(dev)
    ef = torch.from_numpy(np.concatenate([[0], np.cumsum([e.shape[1] for _, _, e in graphs])])).to(dev)
    qp = _qp("median")
    cand, counts = _outputs(len(graphs), 64, dev)
    got = qp.from_targets(rel, ei, nf, y, edge_first=ef, candidates=cand, counts=counts).cpu().numpy()
    qp.check()
    cand = cand.cpu().numpy()
    kept = wrong = 0
    for k, (index, gap) in enumerate(oracle):
        same = [c for c in range(sizes[k] - 1) if np.array_equal(cand[k, c, 3:7].view(np.int64), got[k, 3:7].view(np.int64))]
        assert same, k                                                    # a candidate's bits, never a blend
        if gap >= MEDOID_GAP:
            kept += 1
            wrong += same[0] != index
    print(f"medoid index: {kept} of {len(oracle)} cases held, {wrong} differ")
    assert len(oracle) - kept <= MEDOID_CAP * len(oracle)
    assert wrong == 0


@pytest.mark.parametrize("fuse", MODES)
def test_bad_graphs_are_nan_rows_and_counted(dev, fuse):  # noqa: F811
    from relpose_gnn_amd import ops
    sizes = (8, 3, 8, 4, 5)
    rel, ei, nf, ef, y = _fc_case(sizes, 63, dev)
    kw = dict(fuse=fuse, node_first=nf, node_targets=y, edge_first=ef, pose_m=PM, pose_s=PS)
    good = ops.query_pose_fused(rel, ei, **kw)
    _agree(good, _host_rows(rel, ei, sizes, y, fuse))
    dst = ei[1].cpu().numpy()
    # graph 1 (nodes 8..10): no edge into its query; graph 3 (nodes 19..22): only a self-edge into it
    no_in = ei.clone()
    no_in[1, np.flatnonzero(dst == 8)] = 9
    no_in[0, np.flatnonzero(dst == 19)] = 19
    # graph 2 (nodes 11..18): one used edge starts in another graph / past every node
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    cand, counts = _outputs(5, 64, dev)
    got = ops.query_pose_fused(rel, no_in, status=status, candidates=cand, counts=counts, **kw)
    assert int(status) == 2 and counts.cpu().tolist() == [7, 0, 7, 0, 4]
    assert torch.isnan(got[[1, 3]]).all() and torch.isnan(cand[[1, 3]]).all()
    assert torch.equal(_bits(got[[0, 2, 4]]), _bits(good[[0, 2, 4]]))
    _agree(got, _host_rows(rel, no_in, sizes, y, fuse))
    expected = 2
    for outside, which in ((0, 0), (19, 3), (30, 6), (-1, 6)):
        outside_ei = ei.clone()
        outside_ei[0, np.flatnonzero(dst == 11)[which]] = outside
        got = ops.query_pose_fused(rel, outside_ei, status=status, candidates=cand, **kw)      # the second call keeps counting
        expected += 1
        assert int(status) == expected
        assert torch.isnan(got[2]).all() and torch.isnan(cand[2]).all()
        assert torch.equal(_bits(got[[0, 1, 3, 4]]), _bits(good[[0, 1, 3, 4]]))
        # beyond the cut the edge is not used and the graph is good
        if which == 6:
            cut = ops.query_pose_fused(rel, outside_ei, status=status, max_edges=6, **kw)
            assert int(status) == expected and torch.isfinite(cut).all()
    # a node range past n: graph 4 is bad, nothing of it is read
    past = nf.clone()
    past[5] = y.shape[0] + 1
    got = ops.query_pose_fused(rel, ei, status=status, **dict(kw, node_first=past))
    assert int(status) == expected + 1 and torch.isnan(got[4]).all() and torch.equal(_bits(got[:4]), _bits(good[:4]))
    # without a status word of the caller's the count is read back and raised
    with pytest.raises(ValueError, match="no edge into node 0"):
        ops.query_pose_fused(rel, no_in, **kw)
    # the object: deferred, reported once, a good call after it is clean
    qp = _qp(fuse)
    got = qp.from_targets(rel, no_in, nf, y, edge_first=ef)
    assert torch.isnan(got[[1, 3]]).all()
    with pytest.raises(ValueError, match="no edge into node 0"):
        qp.check(wait=True)
    qp.check()
    qp.from_targets(rel, no_in, nf, y)                                    # again, cut by the columns' targets
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        qp.check(wait=False)
    assert torch.equal(_bits(qp.from_targets(rel, ei, nf, y, edge_first=ef)), _bits(good))
    qp.check()


@pytest.mark.parametrize("fuse", MODES)
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")], ids=["nan", "pinf", "ninf"])
def test_a_non_finite_candidate_voids_the_fused_pose(dev, fuse, value):  # noqa: F811
    sizes = (8, 8, 2, 4, 3)
    rel, ei, nf, ef, y = _fc_case(sizes, 64, dev)
    rel, y = rel.clone(), y.clone()
    dst = ei[1].cpu().numpy()
    rel[np.flatnonzero(dst == 0)[3], 1] = value           # graph 0: translation part of candidate 3
    rel[np.flatnonzero(dst == 8)[6], 4] = value           # graph 1: rotation part of the last candidate
    rel[np.flatnonzero(dst == 16)[0], 5] = value          # graph 2: its only candidate -- propagates as in the single-edge rule
    y[18, 2] = value                                      # graph 3: the query's own target
    rel[np.flatnonzero(dst != 22)[-1], 0] = value         # graph 4: a column that is no edge into the query
    want = _host_rows(rel, ei, sizes, y, fuse)
    qp = _qp(fuse)
    got = qp.from_targets(rel, ei, nf, y, edge_first=ef)
    _agree(got, want)
    qp.check()                                            # non-finite values are not bad graphs
    got = got.cpu().numpy()
    assert np.isnan(got[:2, :7]).all() and np.isnan(got[:2, 14:]).all() and np.isfinite(got[:2, 7:14]).all()
    assert torch.equal(_bits(torch.from_numpy(got[2])), _bits(_single(0).from_targets(rel, ei, nf, y, edge_first=ef)[2].cpu()))
    assert np.isfinite(got[3, :7]).all() and np.isfinite(got[4]).all()


@pytest.mark.parametrize("fuse", MODES)
def test_deterministic_and_graph_by_graph(dev, fuse):  # noqa: F811
    sizes = tuple(2 + (i * 4) % 9 for i in range(13))                      # 2 .. 10 nodes
    rel, ei, nf, ef, y = _fc_case(sizes, 65, dev)
    qp = _qp(fuse)
    a = torch.empty((13, 16), dtype=torch.float64, device=dev)
    a.view(torch.uint8).fill_(0xFF)
    b = torch.zeros((13, 16), dtype=torch.float64, device=dev)
    assert qp.from_targets(rel, ei, nf, y, edge_first=ef, out=a) is a                 # out= is used, every slot overwritten
    qp.from_targets(rel, ei, nf, y, edge_first=ef, out=b)
    assert torch.equal(_bits(a), _bits(b)) and torch.isfinite(a).all()
    # out= reuse: other inputs into the same tensor
    rel2, ei2, nf2, ef2, y2 = _fc_case(sizes, 66, dev)
    qp.from_targets(rel2, ei2, nf2, y2, edge_first=ef2, out=b)
    assert not torch.equal(_bits(a), _bits(b))
    _agree(b, _host_rows(rel2, ei2, sizes, y2, fuse))
    # every graph alone: the same bits as in the batch
    for k, n in enumerate(sizes):
        e0, e1, n0 = int(ef[k]), int(ef[k + 1]), int(nf[k])
        one = qp.from_targets(rel[e0:e1].contiguous(), (ei[:, e0:e1] - n0).contiguous(), torch.tensor([0, n], device=dev),
                              y[n0:n0 + n].contiguous())
        assert torch.equal(_bits(one[0]), _bits(a[k])), k
    qp.check()


def test_capture_and_replay_equals_eager(dev):  # noqa: F811
    sizes = (8, 5, 12, 2)
    rel, ei, nf, ef, y = _fc_case(sizes, 67, dev)
    qp = _qp("median")
    eager = qp.from_targets(rel, ei, nf, y, edge_first=ef)
    out = torch.zeros_like(eager)
    qp.check()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        qp.from_targets(rel, ei, nf, y, edge_first=ef, out=out)
    out.zero_()
    graph.replay()
    qp.publish()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(eager))
    qp.check()


# ---- the two streams ------------------------------------------------------------------------------------------------------------
def _fields(r):
    return np.concatenate([r.pred_poses, r.targ_poses, r.t_loss[:, None], r.q_loss[:, None]], 1)


def test_evaluate_stream_device_equals_host(dev, models):  # noqa: F811
    import relpose_gnn_amd.synth as S
    from relpose_gnn_amd.evaluate import evaluate_stream
    from relpose_gnn_amd.graph import Data, fc_edge_index
    m = models[-1]
    graphs = [Data(x=S.synth_images(8, 32, 40, seed=800 + i), edge_index=fc_edge_index(8), y=S.hash_normal(f"fp.y{i}", (8, 6), 0.3))
              for i in range(8)]
    kw = dict(micro_batch=3, pose_m=PM, pose_s=PS)
    plain = evaluate_stream(m, graphs, dev, postprocess="device", **kw)
    for fuse in MODES:
        sh, sd = {}, {}
        host = evaluate_stream(m, graphs, dev, fuse=fuse, stats=sh, **kw)
        devr = evaluate_stream(m, graphs, dev, fuse=fuse, stats=sd, postprocess="device", **kw)
        assert devr.pred_poses.shape == (8, 7) and np.isfinite(devr.q_loss).all()
        _agree_results(devr, host)
        assert sd["d2h_bytes"] == 8 * 16 * 8 and sd["d2h_bytes"] < sh["d2h_bytes"]
        assert not np.array_equal(devr.pred_poses, plain.pred_poses)
        # one candidate per graph is the single-edge rule: the rows of fuse=None, bit for bit
        one = evaluate_stream(m, graphs, dev, fuse=fuse, max_edges=1, postprocess="device", **kw)
        assert np.array_equal(_fields(one).view(np.int64), _fields(plain).view(np.int64))
    # fuse=None is the stream without the argument
    again = evaluate_stream(m, graphs, dev, postprocess="device", fuse=None, **kw)
    assert np.array_equal(_fields(again).view(np.int64), _fields(plain).view(np.int64))
    _agree_results(plain, evaluate_stream(m, graphs, dev, **kw))
    # a graph without an edge into its query node: the ValueError of the host path
    bad = list(graphs)
    bad[3] = Data(x=graphs[3].x, edge_index=torch.tensor([[0, 2], [1, 1]]), y=graphs[3].y)
    with pytest.raises(ValueError, match="no edge into node 0"):
        evaluate_stream(m, bad, dev, micro_batch=3, postprocess="device", fuse="mean")


@pytest.mark.parametrize("knn", [-1, 4])
def test_relocalize_device_equals_host(dev, models, knn):  # noqa: F811
    import relpose_gnn_amd.synth as S
    from relpose_gnn_amd.evaluate import relocalize
    from relpose_gnn_amd.featmap import FeatureMap
    m = models[knn]
    gen = torch.Generator().manual_seed(33)
    mimgs, queries = S.synth_images(20, 32, 40, seed=93), S.synth_images(8, 32, 40, seed=94)
    poses, targets = torch.randn(20, 6, generator=gen) * 0.3, torch.randn(8, 6, generator=gen) * 0.3
    fmap = FeatureMap.build(m, mimgs, poses=poses)
    nb = torch.stack([torch.randperm(20, generator=gen)[:7] for _ in range(8)])
    kw = dict(micro_batch=3, pose_m=PM, pose_s=PS)
    plain = relocalize(m, fmap, queries, nb, targets=targets, postprocess="device", **kw)
    for fuse in MODES:
        sd = {}
        host = relocalize(m, fmap, queries, nb, targets=targets, fuse=fuse, **kw)
        devr = relocalize(m, fmap, queries, nb, targets=targets, fuse=fuse, stats=sd, postprocess="device", **kw)
        _agree_results(devr, host)
        assert sd["d2h_bytes"] == 8 * 16 * 8 and np.array_equal(devr.neighbours, nb.numpy())
        pred = relocalize(m, fmap, queries.to(dev), nb.to(dev), fuse=fuse, postprocess="device", **kw)
        assert pred.shape == (8, 7) and np.abs(pred - devr.pred_poses).max() <= 1e-12 * (1 + np.abs(pred).max())
        one = relocalize(m, fmap, queries, nb, targets=targets, fuse=fuse, max_edges=1, postprocess="device", **kw)
        assert np.array_equal(_fields(one).view(np.int64), _fields(plain).view(np.int64))
    again = relocalize(m, fmap, queries, nb, targets=targets, postprocess="device", fuse=None, **kw)
    assert np.array_equal(_fields(again).view(np.int64), _fields(plain).view(np.int64))
