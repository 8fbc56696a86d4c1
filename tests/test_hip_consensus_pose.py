"""A query's reference edges fused by consensus on the GPU (rpg_query_pose_consensus_f64 / ops.query_pose_fused(fuse="consensus") /
QueryPose(fuse="consensus"), and ``fuse="consensus"`` of the two evaluation streams with postprocess="device", eager and captured)
against the numpy statement of the rule, evaluate.consensus_query_row, on the same fp32 tensors.

Tolerances: those of test_hip_fused_pose.py, for its reasons -- 1e-12 on poses and the translation error, 1e-5 degrees + 1e-9
relative on rotation errors, equal non-finite patterns.  What must be EXACT is held exactly: ``inliers`` and ``used``, the
candidates against the single-edge kernel, admit-all thresholds against "mean", (0, 0) against the single-edge rule, repeated and
split calls, a captured step against the eager one.  A support decision within a hair of a threshold is not comparable between the
device's acos / sqrt and numpy's: the drawn cases hold few such graphs (test_consensus_pose_cpu.consensus_cases asserts at most
5 %) and those are left out of the comparison."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from test_consensus_pose_cpu import (CONSENSUS_CAP, CONSENSUS_DEG, CONSENSUS_T, consensus_cases, near_a_threshold)
from test_hip_fused_pose import _bits, _check_candidates, _outputs, _single
from test_hip_query_pose import PM, PS, _agree, _agree_results, _fc_case, _Map, dev, models  # noqa: F401  (dev, models: fixtures)
from test_hip_relocalize_capture import G, H, K, M, MB, W, _small

pytestmark = pytest.mark.gpu

ALL = dict(inlier_t=1e300, inlier_deg=360.0)
NONE = dict(inlier_t=0.0, inlier_deg=0.0)
WIDE = dict(inlier_t=2.0, inlier_deg=120.0)               # at the scale of _fc_case's random candidates: some agree, some do not
NAN_ROW = np.full(16, np.nan)


def _qp(max_edges=64, **kw):
    from relpose_gnn_amd.query_pose import QueryPose
    return QueryPose(PM, PS, fuse="consensus", max_edges=max_edges, **kw)


def _ints(g, dev):
    """The [G, 2] output filled with a pattern the kernel must overwrite everywhere."""
    return torch.full((g, 2), -7, dtype=torch.int32, device=dev)


def _host(rel, ei, sizes, y, max_edges=64, **kw):
    """-> (rows [G, 16], (inliers, used) [G, 2], near a threshold [G]) of a collated batch by the numpy rule, cut per graph by the
    columns' targets; a NaN row and (0, min(count, max_edges)) for a bad graph."""
    from relpose_gnn_amd import evaluate as E
    rel, ei, y = rel.cpu().numpy().astype(np.float64), ei.cpu().numpy(), y.cpu().numpy().astype(np.float64)
    first, per_graph = E.edges_per_graph(ei, sizes)
    pm, ps = np.asarray(PM), np.asarray(PS)
    t, deg = kw.get("inlier_t", 0.25), kw.get("inlier_deg", 5.0)
    rows, ints, near = [], [], []
    for k, (n, cols) in enumerate(zip(sizes, per_graph)):
        r, target, edges = rel[cols], y[first[k]:first[k] + n], ei[:, cols] - first[k]
        with np.errstate(all="ignore"):
            try:
                row, n_in, used = E.consensus_query_row(r, target, edges, pm, ps, max_edges, **kw)
                cands = E.pose_candidates(r, target, edges, pm, ps, max_edges)[0]
                near.append(t > 0 and deg > 0 and near_a_threshold(cands, t, deg))
            except ValueError:
                usable = int(((edges[1] == 0) & (edges[0] != 0)).sum())
                row, n_in, used = NAN_ROW, 0, min(usable, max_edges)
                near.append(False)
        rows.append(row)
        ints.append((n_in, used))
    return np.stack(rows), np.array(ints), np.array(near)


def _check(got, ints, want, want_ints, near=None):
    keep = np.ones(len(want), dtype=bool) if near is None else ~near
    assert keep.sum() >= (1 - CONSENSUS_CAP) * len(want)
    assert np.array_equal(ints.cpu().numpy()[keep], want_ints[keep]), (ints.cpu().numpy()[keep] != want_ints[keep]).nonzero()
    _agree(got.cpu().numpy()[keep], want[keep])


# ---- the drawn cases ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drawn(dev):  # noqa: F811
    """The 200 graphs of test_consensus_pose_cpu.consensus_cases as one collated batch on the device, and the oracle's answers."""
    graphs, oracle = consensus_cases()
    sizes = [y.shape[0] for _, y, _ in graphs]
    first = np.concatenate([[0], np.cumsum(sizes)])
    rel = torch.from_numpy(np.concatenate([r for r, _, _ in graphs]).astype(np.float32)).to(dev)
    y = torch.from_numpy(np.concatenate([t for _, t, _ in graphs]).astype(np.float32)).to(dev)
    ei = torch.from_numpy(np.concatenate([e + first[k] for k, (_, _, e) in enumerate(graphs)], 1)).to(dev)
    nf = torch.from_numpy(first).to(dev)
    ef = torch.from_numpy(np.concatenate([[0], np.cumsum([e.shape[1] for _, _, e in graphs])])).to(dev)
    want = np.stack([o[0] for o in oracle])
    want_ints = np.array([(o[1], o[2]) for o in oracle])
    near = np.array([o[4] for o in oracle])
    return sizes, (rel, ei, nf, ef, y), want, want_ints, near


def test_drawn_cases_in_one_call(dev, drawn):  # noqa: F811
    sizes, (rel, ei, nf, ef, y), want, want_ints, near = drawn
    g = len(sizes)
    assert near.sum() <= CONSENSUS_CAP * g and len(set(want_ints[:, 0].tolist())) >= 6
    qp = _qp(inlier_t=CONSENSUS_T, inlier_deg=CONSENSUS_DEG)
    for edge_first in (ef, None):                                         # cut by offsets, and by the columns' targets
        cand, counts = _outputs(g, 64, dev)
        ints = _ints(g, dev)
        got = qp.from_targets(rel, ei, nf, y, edge_first=edge_first, candidates=cand, counts=counts, inliers=ints)
        _check(got, ints, want, want_ints, near)
        assert ints[:, 1].cpu().tolist() == [n - 1 for n in sizes]        # `used` is exact for every graph, near or not
    _check_candidates(cand, counts, rel, ei, nf, ef, y, sizes)
    qp.check()
    # the defaults are these thresholds; without the optional outputs the rows are the same bits
    assert torch.equal(_bits(_qp().from_targets(rel, ei, nf, y, edge_first=ef)), _bits(got))


# ---- shapes where the wave logic can go wrong ------------------------------------------------------------------------------------------
SIZES = {1: (2,), 4: (2, 3, 8, 5), 5: (8, 2, 3, 8, 4)}            # C = 1, 2 and 7 (and 3, 4); a full and a partial workgroup


@pytest.mark.parametrize("g", [1, 4, 5])
def test_fc_graphs(dev, g):  # noqa: F811
    sizes = SIZES[g]
    rel, ei, nf, ef, y = _fc_case(sizes, 50 + g, dev)
    single0 = _single(0).from_targets(rel, ei, nf, y, edge_first=ef)
    for kw in (WIDE, {}):
        want, want_ints, near = _host(rel, ei, sizes, y, **kw)
        assert not near.any() and np.isfinite(want).all()
        qp = _qp(**kw)
        for edge_first in (ef, None):
            cand, counts = _outputs(g, 64, dev)
            ints = _ints(g, dev)
            got = qp.from_targets(rel, ei, nf, y, edge_first=edge_first, candidates=cand, counts=counts, inliers=ints)
            _check(got, ints, want, want_ints)
            _check_candidates(cand, counts, rel, ei, nf, ef, y, sizes)
            for k, n in enumerate(sizes):
                if n == 2:                                                # one candidate: the single-edge rule's row, bit for bit
                    assert torch.equal(_bits(got[k]), _bits(single0[k])) and ints[k].tolist() == [1, 1]
        qp.check()
    if g > 1:
        assert len(set(_host(rel, ei, sizes, y, **WIDE)[1][:, 0].tolist())) > 1


@pytest.mark.parametrize("sizes", [(3, 66, 8), (65,)], ids=["65-in-edges", "64-candidates"])
def test_every_lane_live(dev, sizes):  # noqa: F811
    """A 66-node graph between two small ones: 65 edges into its query, 64 used, spread over several 64-column steps.  A 65-node
    graph: exactly 64 candidates.  Thresholds at which a good part of the 64 random candidates support the winner."""
    rel, ei, nf, ef, y = _fc_case(sizes, 60, dev)
    big = int(np.argmax(sizes))
    kw = dict(inlier_t=1.6, inlier_deg=100.0)
    want, want_ints, near = _host(rel, ei, sizes, y, **kw)
    assert not near.any() and want_ints[big, 1] == 64 and 1 < want_ints[big, 0] < 64
    qp = _qp(**kw)
    for edge_first in (ef, None):
        cand, counts = _outputs(len(sizes), 64, dev)
        ints = _ints(len(sizes), dev)
        got = qp.from_targets(rel, ei, nf, y, edge_first=edge_first, candidates=cand, counts=counts, inliers=ints)
        _check(got, ints, want, want_ints)
        assert counts.cpu().tolist() == [n - 1 for n in sizes] and torch.isfinite(cand[big]).all()
    # admit-all over 64 lanes: the bits of "mean"
    from relpose_gnn_amd.query_pose import QueryPose
    ints = _ints(len(sizes), dev)
    got = _qp(**ALL).from_targets(rel, ei, nf, y, edge_first=ef, inliers=ints)
    assert torch.equal(_bits(got), _bits(QueryPose(PM, PS, fuse="mean").from_targets(rel, ei, nf, y, edge_first=ef)))
    assert ints[big].tolist() == [64, 64]
    qp.check()


@pytest.mark.parametrize("max_edges", [1, 2, 3])
def test_max_edges_below_the_candidates(dev, max_edges):  # noqa: F811
    sizes = (8, 5, 3, 2, 12)
    rel, ei, nf, ef, y = _fc_case(sizes, 61, dev)
    want, want_ints, near = _host(rel, ei, sizes, y, max_edges, **WIDE)
    assert not near.any()
    qp = _qp(max_edges, **WIDE)
    cand, counts = _outputs(5, max_edges, dev)
    ints = _ints(5, dev)
    got = qp.from_targets(rel, ei, nf, y, edge_first=ef, candidates=cand, counts=counts, inliers=ints)
    _check(got, ints, want, want_ints)
    assert ints[:, 1].cpu().tolist() == [min(n - 1, max_edges) for n in sizes]
    _check_candidates(cand, counts, rel, ei, nf, ef, y, sizes, max_edges)
    if max_edges == 1:                                                    # every graph has one candidate: the single-edge rows
        assert torch.equal(_bits(got), _bits(_single(0).from_targets(rel, ei, nf, y, edge_first=ef)))
    qp.check()


# ---- exact identities on the device ------------------------------------------------------------------------------------------------
def test_admit_all_is_mean_and_admit_none_is_the_single_edge_rule(dev):  # noqa: F811
    from relpose_gnn_amd.query_pose import QueryPose
    sizes = tuple(2 + (i * 4) % 9 for i in range(13))                      # 2 .. 10 nodes
    rel, ei, nf, ef, y = _fc_case(sizes, 65, dev)
    ints = _ints(13, dev)
    got = _qp(**ALL).from_targets(rel, ei, nf, y, edge_first=ef, inliers=ints)
    assert torch.equal(_bits(got), _bits(QueryPose(PM, PS, fuse="mean").from_targets(rel, ei, nf, y, edge_first=ef)))
    assert ints.cpu().tolist() == [[n - 1, n - 1] for n in sizes]
    # (0, 0) on distinct candidates: every support is 1 (self-support is c == d, not an angle test), candidate 0 wins alone
    got = _qp(**NONE).from_targets(rel, ei, nf, y, edge_first=ef, inliers=ints)
    assert torch.equal(_bits(got), _bits(_single(0).from_targets(rel, ei, nf, y, edge_first=ef)))
    assert ints.cpu().tolist() == [[1, n - 1] for n in sizes]


def test_deterministic_and_graph_by_graph(dev):  # noqa: F811
    sizes = tuple(2 + (i * 4) % 9 for i in range(13))
    rel, ei, nf, ef, y = _fc_case(sizes, 65, dev)
    qp = _qp(**WIDE)
    a = torch.empty((13, 16), dtype=torch.float64, device=dev)
    a.view(torch.uint8).fill_(0xFF)
    b = torch.zeros((13, 16), dtype=torch.float64, device=dev)
    ia, ib = _ints(13, dev), torch.zeros((13, 2), dtype=torch.int32, device=dev)
    assert qp.from_targets(rel, ei, nf, y, edge_first=ef, out=a, inliers=ia) is a     # out= is used, every slot overwritten
    qp.from_targets(rel, ei, nf, y, edge_first=ef, out=b, inliers=ib)                 # a repeated call: the same bits
    assert torch.equal(_bits(a), _bits(b)) and torch.isfinite(a).all() and torch.equal(ia, ib) and int(ia.min()) >= 1
    want, want_ints, near = _host(rel, ei, sizes, y, **WIDE)
    assert not near.any()
    _check(a, ia, want, want_ints)
    # the batch split in two calls, and every graph alone: the same bits as in one call
    for k0, k1 in ((0, 6), (6, 13)):
        e0, e1, n0, n1 = int(ef[k0]), int(ef[k1]), int(nf[k0]), int(nf[k1])
        ints = _ints(k1 - k0, dev)
        part = qp.from_targets(rel[e0:e1].contiguous(), (ei[:, e0:e1] - n0).contiguous(), (nf[k0:k1 + 1] - n0).contiguous(),
                               y[n0:n1].contiguous(), edge_first=(ef[k0:k1 + 1] - e0).contiguous(), inliers=ints)
        assert torch.equal(_bits(part), _bits(a[k0:k1])) and torch.equal(ints, ia[k0:k1])
    for k, n in enumerate(sizes):
        e0, e1, n0 = int(ef[k]), int(ef[k + 1]), int(nf[k])
        ints = _ints(1, dev)
        one = qp.from_targets(rel[e0:e1].contiguous(), (ei[:, e0:e1] - n0).contiguous(), torch.tensor([0, n], device=dev),
                              y[n0:n0 + n].contiguous(), inliers=ints)
        assert torch.equal(_bits(one[0]), _bits(a[k])) and torch.equal(ints[0], ia[k]), k
    qp.check()


def test_capture_and_replay_equals_eager(dev):  # noqa: F811
    sizes = (8, 5, 12, 2)
    rel, ei, nf, ef, y = _fc_case(sizes, 67, dev)
    qp = _qp(**WIDE)
    want_ints = _ints(4, dev)
    eager = qp.from_targets(rel, ei, nf, y, edge_first=ef, inliers=want_ints)
    out, ints = torch.zeros_like(eager), _ints(4, dev)
    qp.check()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        qp.from_targets(rel, ei, nf, y, edge_first=ef, out=out, inliers=ints)
    out.zero_()
    ints.fill_(-7)
    graph.replay()
    qp.publish()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(eager)) and torch.equal(ints, want_ints)
    qp.check()


# ---- non-finite inputs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")], ids=["nan", "pinf", "ninf"])
def test_non_finite_inputs(dev, value):  # noqa: F811
    sizes = (8, 8, 4, 3, 2, 5)
    rel, ei, nf, ef, y = _fc_case(sizes, 64, dev)
    clean_ints = _ints(6, dev)
    qp = _qp(**WIDE)
    clean = qp.from_targets(rel, ei, nf, y, edge_first=ef, inliers=clean_ints)
    rel = rel.clone()
    dst = ei[1].cpu().numpy()
    rel[np.flatnonzero(dst == 0)[3], 1] = value           # graph 0: translation part of used candidate 3
    rel[np.flatnonzero(dst == 8)[6], 4] = value           # graph 1: rotation part of the last used candidate
    rel[np.flatnonzero(dst == 17), 0] = value             # graph 2 (nodes 16..19): columns that are no edge into its query
    rel[np.flatnonzero(dst == 20)[:], 2] = value          # graph 3 (nodes 20..22): EVERY used edge
    rel[np.flatnonzero(dst == 23)[0], 5] = value          # graph 4 (nodes 23, 24): its only candidate
    want, want_ints, near = _host(rel, ei, sizes, y, **WIDE)
    assert not near.any()
    ints = _ints(6, dev)
    got = qp.from_targets(rel, ei, nf, y, edge_first=ef, inliers=ints)
    _check(got, ints, want, want_ints)
    qp.check()                                            # non-finite values are not bad graphs: the status is untouched
    got = got.cpu().numpy()
    # graphs 0, 1: the planted candidate is an outlier, the rest of the graph's consensus stands (against numpy above) and is finite
    assert np.isfinite(got[:2]).all() and ints[:2, 1].tolist() == [7, 7]
    assert ints[2].tolist() == clean_ints[2].tolist() and np.array_equal(got[2], clean[2].cpu().numpy())
    assert torch.equal(_bits(torch.from_numpy(got[5])), _bits(clean[5].cpu()))                # an untouched graph
    # graphs 3, 4: nothing finite to vote -- NaN pred and errors, finite targ, 0 inliers
    for k, used in ((3, 2), (4, 1)):
        assert np.isnan(got[k, :7]).all() and np.isnan(got[k, 14:]).all() and np.isfinite(got[k, 7:14]).all()
        assert ints[k].tolist() == [0, used]
    # an edge beyond the cut is not used: planted there it changes nothing
    rel2, ei2, nf2, ef2, y2 = _fc_case((8, 4), 68, dev)
    cut = _qp(3, **WIDE)
    ia, ib = _ints(2, dev), _ints(2, dev)
    a = cut.from_targets(rel2, ei2, nf2, y2, edge_first=ef2, inliers=ia)
    rel2 = rel2.clone()
    rel2[np.flatnonzero(ei2[1].cpu().numpy() == 0)[3:], :] = value
    b = cut.from_targets(rel2, ei2, nf2, y2, edge_first=ef2, inliers=ib)
    assert torch.equal(_bits(a), _bits(b)) and torch.equal(ia, ib) and ia[:, 1].tolist() == [3, 3]
    cut.check()


# ---- bad graphs ------------------------------------------------------------------------------------------------------------------------
def test_bad_graphs_are_nan_rows_with_no_inliers(dev):  # noqa: F811
    from relpose_gnn_amd import ops
    sizes = (8, 3, 8, 4, 5)
    rel, ei, nf, ef, y = _fc_case(sizes, 63, dev)
    kw = dict(fuse="consensus", node_first=nf, node_targets=y, edge_first=ef, pose_m=PM, pose_s=PS, **WIDE)
    good_ints = _ints(5, dev)
    good = ops.query_pose_fused(rel, ei, inliers=good_ints, **kw)
    dst = ei[1].cpu().numpy()
    # graph 1 (nodes 8..10): no edge into its query; graph 3 (nodes 19..22): only self-edges into it
    no_in = ei.clone()
    no_in[1, np.flatnonzero(dst == 8)] = 9
    no_in[0, np.flatnonzero(dst == 19)] = 19
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ints = _ints(5, dev)
    got = ops.query_pose_fused(rel, no_in, status=status, inliers=ints, **kw)
    assert int(status) == 2 and torch.isnan(got[[1, 3]]).all() and ints[[1, 3]].tolist() == [[0, 0], [0, 0]]
    assert torch.equal(_bits(got[[0, 2, 4]]), _bits(good[[0, 2, 4]])) and torch.equal(ints[[0, 2, 4]], good_ints[[0, 2, 4]])
    want, want_ints, _ = _host(rel, no_in, sizes, y, **WIDE)
    _check(got, ints, want, want_ints)
    # graph 2 (nodes 11..18): a used edge starts in another graph
    outside = ei.clone()
    outside[0, np.flatnonzero(dst == 11)[3]] = 19
    got = ops.query_pose_fused(rel, outside, status=status, inliers=ints, **kw)
    assert int(status) == 3 and torch.isnan(got[2]).all() and ints[2].tolist() == [0, 7]
    assert torch.equal(_bits(got[[0, 1, 3, 4]]), _bits(good[[0, 1, 3, 4]]))
    # without a status word of the caller's the count is read back and raised; the object defers it to check()
    with pytest.raises(ValueError, match="no edge into node 0"):
        ops.query_pose_fused(rel, no_in, **kw)
    qp = _qp(**WIDE)
    got = qp.from_targets(rel, no_in, nf, y, edge_first=ef, inliers=ints)
    assert torch.isnan(got[[1, 3]]).all() and ints[[1, 3]].tolist() == [[0, 0], [0, 0]]
    with pytest.raises(ValueError, match="no edge into node 0"):
        qp.check(wait=True)
    assert torch.equal(_bits(qp.from_targets(rel, ei, nf, y, edge_first=ef)), _bits(good))
    qp.check()


# ---- the map path ----------------------------------------------------------------------------------------------------------------------
# the synthetic model's relative poses are of order 1 to 10 and disagree by as much, so the scene is scaled down (pose_s) until the
# K estimates of a query lie well inside inlier_t = 0.25 of each other -- unless their database image's pose is the far-off one
PS_MAP = (0.02, 0.005, 0.0125)
MAP_KW = dict(inlier_t=0.25, inlier_deg=360.0)
FAR = 3                                                   # the map row whose pose is far off


@pytest.fixture(scope="module")
def map_data():
    import relpose_gnn_amd.synth as S
    gen = torch.Generator().manual_seed(6)
    poses = torch.randn(M, 6, generator=gen) * 0.3
    poses[FAR, :3] += 400.0                               # 400 * pose_s = 8, 2 and 5 away
    nb = torch.stack([torch.randperm(M, generator=gen)[:K] for _ in range(G)])
    assert 0 < int((nb == FAR).any(1).sum()) < G          # some queries have the far-off neighbour, some do not
    return dict(mimgs=S.synth_images(M, H, W, seed=91), queries=S.synth_images(G, H, W, seed=92), poses=poses,
                targets=torch.randn(G, 6, generator=gen) * 0.3, nb=nb)


@pytest.fixture(scope="module")
def map_model(dev, map_data):  # noqa: F811
    from relpose_gnn_amd.featmap import FeatureMap
    m = _small(dev)
    return m, FeatureMap.build(m, map_data["mimgs"], poses=map_data["poses"])


def _map_host(rel, nb, poses, targets, outputs="all", **kw):
    """The host rule on one forward_map output: -> (rows [G, 16], ints [G, 2], near [G])."""
    from relpose_gnn_amd import evaluate as E
    from relpose_gnn_amd.graph import fc_edge_index
    g, k = nb.shape
    edges = fc_edge_index(k + 1).numpy()
    if outputs == "query":
        edges = edges[:, edges[1] == 0]
    e_g = edges.shape[1]
    rel = rel.cpu().numpy().astype(np.float64)
    pm, ps = np.asarray(PM), np.asarray(PS_MAP)
    rows, ints, near = [], [], []
    for j in range(g):
        target = np.zeros((k + 1, 6))
        target[1:] = poses.numpy().astype(np.float64)[nb[j].numpy()]
        target[0] = targets[j].numpy()
        r = rel[j * e_g:(j + 1) * e_g]
        row, n_in, used = E.consensus_query_row(r, target, edges, pm, ps, **kw)
        rows.append(row)
        ints.append((n_in, used))
        near.append(near_a_threshold(E.pose_candidates(r, target, edges, pm, ps)[0], kw["inlier_t"], kw["inlier_deg"]))
    return np.stack(rows), np.array(ints), np.array(near)


def test_from_map_equals_the_host_rule(dev, map_data, map_model):  # noqa: F811
    from relpose_gnn_amd.query_pose import QueryPose
    m, fmap = map_model
    q, nb, targets = map_data["queries"].to(dev), map_data["nb"].to(dev), map_data["targets"].to(dev)
    for outputs in ("all", "query"):
        ab, rel, ei = m.forward_map(q, nb, fmap, outputs=outputs)
        want, want_ints, near = _map_host(rel, map_data["nb"], map_data["poses"], map_data["targets"], outputs, **MAP_KW)
        assert not near.any()
        has_far = (map_data["nb"] == FAR).any(1).numpy()
        assert want_ints[:, 1].tolist() == [K] * G and (want_ints[has_far, 0] == K - 1).all() and (want_ints[~has_far, 0] == K).all()
        qp = QueryPose(PM, PS_MAP, fuse="consensus", **MAP_KW)
        ints = _ints(G, dev)
        got = qp.from_map(rel, ei, fmap, nb, query_targets=targets, inliers=ints)
        _check(got, ints, want, want_ints)
        # the far-off estimate pulls "mean" away and leaves consensus where the others are
        mean = QueryPose(PM, PS_MAP, fuse="mean").from_map(rel, ei, fmap, nb, query_targets=targets).cpu().numpy()
        got = got.cpu().numpy()
        assert (np.abs(mean[has_far, 0] - got[has_far, 0]) > 1.0).all()
        assert np.array_equal(mean[~has_far].view(np.int64), got[~has_far].view(np.int64))      # all K agree: the mean of all
        qp.check()
    m.check_edge_index()


def _same(a, b):
    for f in ("pred_poses", "targ_poses", "t_loss", "q_loss", "neighbours", "inliers", "used"):
        x, y = getattr(a, f), getattr(b, f)
        assert x.shape == y.shape and np.array_equal(x, y), f


def test_relocalize_host_device_query_and_capture(dev, map_data, map_model):  # noqa: F811
    from relpose_gnn_amd.evaluate import relocalize
    m, fmap = map_model
    q, nb, targets = map_data["queries"], map_data["nb"], map_data["targets"]
    kw = dict(micro_batch=MB, pose_m=PM, pose_s=PS_MAP, targets=targets, fuse="consensus", **MAP_KW)
    has_far = (nb == FAR).any(1).numpy()
    sh, sd, sm = {}, {}, {}
    host = relocalize(m, fmap, q, nb, stats=sh, **kw)
    devr = relocalize(m, fmap, q, nb, stats=sd, postprocess="device", **kw)
    _agree_results(devr, host)
    for r in (host, devr):
        assert r.inliers.dtype.kind == "i" and r.used.tolist() == [K] * G
        assert np.array_equal(r.inliers, np.where(has_far, K - 1, K))
    # 8 more bytes per query than the rows of another mode
    relocalize(m, fmap, q, nb, stats=sm, postprocess="device", **dict(kw, fuse="mean"))
    assert sd["d2h_bytes"] == G * (16 * 8 + 8) == sm["d2h_bytes"] + 8 * G and sd["d2h_bytes"] < sh["d2h_bytes"]
    # outputs="query": the integers exact, the rows at the bar of the forward between the two modes
    for postprocess in ("host", "device"):
        qr = relocalize(m, fmap, q, nb, outputs="query", postprocess=postprocess, **kw)
        assert np.array_equal(qr.inliers, host.inliers) and np.array_equal(qr.used, host.used)
        assert rel_err(qr.pred_poses[:, :3], host.pred_poses[:, :3]) < 1e-4
    # without targets: the poses as before, the integers in stats
    st = {}
    pred = relocalize(m, fmap, q, nb, stats=st, postprocess="device", **{k: v for k, v in kw.items() if k != "targets"})
    assert np.array_equal(pred, devr.pred_poses) and np.array_equal(st["inliers"], devr.inliers) and np.array_equal(st["used"], devr.used)
    # capture=True: bit-identical rows and integers, two shapes (a full micro-batch and the tail)
    sc = {}
    cap = relocalize(m, fmap, q, nb, capture=True, stats=sc, postprocess="device", **kw)
    _same(cap, devr)
    assert sc["graphs_captured"] == 2 and sc["graph_replays"] == 3 and sc["d2h_bytes"] == sd["d2h_bytes"]
    relocalize(m, fmap, q, nb, capture=True, stats=sc, postprocess="device", **kw)
    assert sc["graphs_captured"] == 0                                     # the same thresholds again: nothing to capture
    # other thresholds: a new step is captured, not the old one replayed
    tight = dict(kw, inlier_t=0.0, inlier_deg=0.0)
    cap0 = relocalize(m, fmap, q, nb, capture=True, stats=sc, postprocess="device", **tight)
    assert sc["graphs_captured"] == 2
    _same(cap0, relocalize(m, fmap, q, nb, postprocess="device", **tight))
    assert cap0.inliers.tolist() == [1] * G and not np.array_equal(cap0.pred_poses, cap.pred_poses)
    m.check_edge_index()


def test_captured_step_exposes_the_static_integers(dev, map_data, map_model):  # noqa: F811
    from relpose_gnn_amd.graphed import GraphedForwardMap, MapStep
    from relpose_gnn_amd.query_pose import QueryPose
    m, fmap = map_model
    q, nb, targets = map_data["queries"][:MB].to(dev), map_data["nb"][:MB].to(dev), map_data["targets"][:MB].to(dev)
    pose, eager = QueryPose(PM, PS_MAP, fuse="consensus", **MAP_KW), QueryPose(PM, PS_MAP, fuse="consensus", **MAP_KW)
    step = GraphedForwardMap(m, fmap, q, K, pose=pose, pose_kwargs={"query_targets": targets})
    assert MapStep._fields == ("abs_pose", "rel_pose", "edge_index", "neighbours", "rows")
    assert step.inliers.shape == (MB, 2) and step.inliers.dtype == torch.int32
    for seed in (1, 2):
        nb2 = torch.stack([torch.randperm(M, generator=torch.Generator().manual_seed(seed + j))[:K] for j in range(MB)]).to(dev)
        ab, rel, ei = m.forward_map(q, nb2, fmap)
        ints = _ints(MB, dev)
        rows = eager.from_map(rel, ei, fmap, nb2, query_targets=targets, inliers=ints)
        out = step(q, nb2, query_targets=targets)
        assert torch.equal(out.rows, rows) and torch.equal(step.inliers, ints)
    assert GraphedForwardMap(m, fmap, q, K, pose=QueryPose(PM, PS_MAP, fuse="mean")).inliers is None
    pose.check()
    m.check_edge_index()


# ---- evaluate_stream -------------------------------------------------------------------------------------------------------------------
def test_evaluate_stream_device_equals_host(dev, models):  # noqa: F811
    import relpose_gnn_amd.synth as S
    from relpose_gnn_amd.evaluate import evaluate_stream
    from relpose_gnn_amd.graph import Data, fc_edge_index
    m = models[-1]
    graphs = [Data(x=S.synth_images(8, 32, 40, seed=800 + i), edge_index=fc_edge_index(8), y=S.hash_normal(f"fp.y{i}", (8, 6), 0.3))
              for i in range(5)]
    kw = dict(micro_batch=2, pose_m=PM, pose_s=PS_MAP, fuse="consensus", **MAP_KW)
    sh, sd = {}, {}
    host = evaluate_stream(m, graphs, dev, stats=sh, **kw)
    devr = evaluate_stream(m, graphs, dev, stats=sd, postprocess="device", **kw)
    _agree_results(devr, host)
    assert np.array_equal(devr.inliers, host.inliers) and np.array_equal(devr.used, host.used) and host.used.tolist() == [7] * 5
    assert host.inliers.min() >= 1 and sd["d2h_bytes"] == 5 * (16 * 8 + 8) and sd["d2h_bytes"] < sh["d2h_bytes"]
    # admit-all: the rows of "mean", bit for bit, through the stream
    a = evaluate_stream(m, graphs, dev, postprocess="device", **dict(kw, **ALL))
    b = evaluate_stream(m, graphs, dev, postprocess="device", **dict(kw, fuse="mean"))
    assert np.array_equal(a.pred_poses.view(np.int64), b.pred_poses.view(np.int64)) and a.inliers.tolist() == [7] * 5
    assert b.inliers is None and b.used is None
