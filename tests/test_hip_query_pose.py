"""Pose recovery on the GPU (rpg_query_pose_f64 / ops.query_pose / query_pose.QueryPose, and postprocess="device" of the two
evaluation streams) against the host functions it replaces: evaluate.query_pose + evaluate.errors on the same fp32 tensors.

Tolerances, from the arithmetic and not from the results: both sides do a handful of double roundings and libm calls of <= 2 ulp
on values of order 1 to 10 (~1e-15), so rtol = atol = 1e-12 on pred, targ and t_err leaves FMA contraction and numpy's
sinc(n / pi) against sin(n) / n far inside while staying 1e5 below fp32.  acos is ill-conditioned at 1: an 8-ulp change of a dot
that rounds to 1 moves the angle by 2 sqrt(2 * 8 * 2^-53) rad = 4.8e-6 degrees, so q_err gets atol = 1e-5 degrees plus rtol = 1e-9.
The inputs keep that valid: |log q| < 8, pose_s, pose_m and targets of order 1.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PM, PS = (1.5, -0.25, 3.0), (2.0, 0.5, 1.25)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---- the truth: the host functions, graph by graph ---------------------------------------------------------------------------
def _host_row(rel, target, edges, ref_node, pm=PM, ps=PS):
    """One row of 16 by evaluate.query_pose + evaluate.errors; None where reference_edge refuses the graph."""
    from relpose_gnn_amd import evaluate as E
    try:
        ref = E.reference_edge(edges, ref_node)
    except ValueError:
        return None
    if not 0 <= edges[0, ref] < target.shape[0]:
        return None
    with np.errstate(all="ignore"):
        p, t = E.query_pose(rel, target, edges, np.asarray(pm, dtype=np.float64), np.asarray(ps, dtype=np.float64), ref_node)
        r = E.errors(p[None], t[None])
    return np.concatenate([p, t, r.t_loss, r.q_loss])


def _host_rows(rel, ei, sizes, y, ref_node, pm=PM, ps=PS):
    """[G, 16] of a collated batch, cut per graph by the columns' targets (evaluate.edges_per_graph): NaN rows for bad graphs."""
    from relpose_gnn_amd import evaluate as E
    rel, ei, y = rel.cpu().numpy(), ei.cpu().numpy(), y.cpu().numpy()
    first, per_graph = E.edges_per_graph(ei, sizes)
    rows = []
    for k, n in enumerate(sizes):
        cols = per_graph[k]
        row = _host_row(rel[cols], y[first[k]:first[k] + n], ei[:, cols] - first[k], ref_node, pm, ps)
        rows.append(np.full(16, np.nan) if row is None else row)
    return np.stack(rows)


def _agree(got, want):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.shape == want.shape and got.dtype == np.float64
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    assert np.array_equal(np.isinf(got), np.isinf(want)), (got, want)
    fin = np.isfinite(want)
    g, w = np.where(fin, got, 0.0), np.where(fin, want, 0.0)
    assert np.array_equal(got[np.isinf(want)], want[np.isinf(want)])
    err = np.abs(g - w)
    assert (err[:, :15] <= 1e-12 + 1e-12 * np.abs(w[:, :15])).all(), err[:, :15].max()
    assert (err[:, 15] <= 1e-5 + 1e-9 * np.abs(w[:, 15])).all(), err[:, 15].max()


def _agree_results(a, b):
    """Two EvalResults at the tolerances above."""
    _agree(np.concatenate([a.pred_poses, a.targ_poses, a.t_loss[:, None], a.q_loss[:, None]], 1),
           np.concatenate([b.pred_poses, b.targ_poses, b.t_loss[:, None], b.q_loss[:, None]], 1))


# ---- cases ----------------------------------------------------------------------------------------------------------------------
def _fc_case(sizes, seed, dev):
    """A collated batch of fully-connected graphs: (rel [E, 6], ei [2, E], node_first, edge_first, y [N, 6]) on the device."""
    from relpose_gnn_amd.graph import fc_edge_index
    gen = torch.Generator().manual_seed(seed)
    eis, off = [], 0
    for n in sizes:
        eis.append(fc_edge_index(n) + off)
        off += n
    ei = torch.cat(eis, 1)
    rel = torch.randn(ei.shape[1], 6, generator=gen) * 0.3
    y = torch.randn(off, 6, generator=gen) * 0.5
    node_first = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64)
    edge_first = torch.tensor(np.concatenate([[0], np.cumsum([n * (n - 1) for n in sizes])]), dtype=torch.int64)
    return tuple(t.to(dev) for t in (rel, ei, node_first, edge_first, y))


def _qp(ref_node=0):
    from relpose_gnn_amd.query_pose import QueryPose
    return QueryPose(PM, PS, ref_node)


@pytest.mark.parametrize("sizes", [(8,), (2, 8, 5)], ids=["one_graph", "ragged"])
def test_stored_fc_lists(dev, sizes):
    rel, ei, nf, ef, y = _fc_case(sizes, 3, dev)
    for ref_node in sorted({0, 3} | {n - 2 for n in sizes}):            # n - 2: the last valid one of an n-node graph
        qp = _qp(ref_node)
        want = _host_rows(rel, ei, sizes, y, ref_node)
        for edge_first in (ef, None):                                     # cut by offsets, and by the columns' targets
            got = qp.from_targets(rel, ei, nf, y, edge_first=edge_first)
            _agree(got, want)
            if any(ref_node > n - 2 for n in sizes):                      # ref_node past a graph's in-degree: NaN row, reported
                assert np.isnan(want).all(1).any()
                with pytest.raises(ValueError, match="no edge into node 0"):
                    qp.check()
            else:
                assert np.isfinite(want).all()
                qp.check()


def test_reference_edge_past_the_first_64_columns(dev):
    rel, ei, nf, ef, y = _fc_case((12,), 4, dev)
    hits = np.flatnonzero(ei[1].cpu().numpy() == 0)
    assert ei.shape[1] == 132 and hits.min() >= 64 and (np.diff(hits) > 1).all()
    for ref_node in (0, 5, 10):
        qp = _qp(ref_node)
        _agree(qp.from_targets(rel, ei, nf, y, edge_first=ef), _host_rows(rel, ei, (12,), y, ref_node))
        qp.check()


def test_many_graphs(dev):
    sizes = tuple(2 + (i * 5) % 7 for i in range(130))                    # 130 graphs: more than one wave, workgroup and grid row
    rel, ei, nf, ef, y = _fc_case(sizes, 5, dev)
    qp = _qp(0)
    want = _host_rows(rel, ei, sizes, y, 0)
    _agree(qp.from_targets(rel, ei, nf, y, edge_first=ef), want)
    _agree(qp.from_targets(rel, ei, nf, y), want)
    qp.check()


def test_model_built_knn_list(dev):
    from relpose_gnn_amd import ops
    gen = torch.Generator().manual_seed(7)
    feat = torch.randn(24, 16, generator=gen).to(dev)
    batch = torch.arange(3).repeat_interleave(8).to(dev)
    ei = ops.knn_graph(feat, 4, batch)                                    # the model's own knn = 4 list of 3 graphs of 8 nodes
    assert ei.shape == (2, 96)
    rel = (torch.randn(96, 6, generator=gen) * 0.3).to(dev)
    y = (torch.randn(24, 6, generator=gen) * 0.5).to(dev)
    nf = torch.tensor([0, 8, 16, 24], device=dev)
    for ref_node in (0, 3):
        qp = _qp(ref_node)
        _agree(qp.from_targets(rel, ei, nf, y), _host_rows(rel, ei, (8, 8, 8), y, ref_node))
        qp.check()


def test_permuted_columns_keep_column_order(dev):
    sizes = (8, 5, 12)
    rel, ei, nf, ef, y = _fc_case(sizes, 8, dev)
    gen = torch.Generator().manual_seed(12)
    perm = torch.cat([int(ef[k]) + torch.randperm(n * (n - 1), generator=gen) for k, n in enumerate(sizes)]).to(dev)
    rel, ei = rel[perm].contiguous(), ei[:, perm].contiguous()
    hits = np.flatnonzero(ei[1, :56].cpu().numpy() == 0)
    assert hits[0] > 0 and (np.diff(hits) > 1).all()                      # neither first nor adjacent
    for ref_node in (0, 2, 3):
        qp = _qp(ref_node)
        want = _host_rows(rel, ei, sizes, y, ref_node)
        _agree(qp.from_targets(rel, ei, nf, y, edge_first=ef), want)
        _agree(qp.from_targets(rel, ei, nf, y), want)
        qp.check()
    # whole-list permutation: columns of different graphs interleaved, only the target tells the graph
    perm = torch.randperm(ei.shape[1], generator=gen).to(dev)
    rel, ei = rel[perm].contiguous(), ei[:, perm].contiguous()
    qp = _qp(1)
    _agree(qp.from_targets(rel, ei, nf, y), _host_rows(rel, ei, sizes, y, 1))
    qp.check()


class _Map:
    def __init__(self, poses):
        self.poses = poses


def _map_rows(rel, nb, poses, targets, ref_node, m):
    """Host truth of the map form: relocalize's own post-processing (target row 0 = the query's, rows 1.. = the map's)."""
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
        rows.append(_host_row(rel[j * e_g:(j + 1) * e_g].cpu().numpy(), target, edges, ref_node))
    return np.stack(rows)


@pytest.mark.parametrize("k", [7, 1])
def test_map_form(dev, k):
    from relpose_gnn_amd.graph import fc_batch
    g, m = 5, 16
    gen = torch.Generator().manual_seed(20 + k)
    poses = (torch.randn(m, 6, generator=gen) * 0.5).to(dev)
    targets = (torch.randn(g, 6, generator=gen) * 0.5).to(dev)
    nb = torch.randint(0, m, (g, k), generator=gen).to(dev)
    ei = fc_batch(torch.empty((g * (k + 1), 0)), k + 1).edge_index.to(dev)
    rel = (torch.randn(ei.shape[1], 6, generator=gen) * 0.3).to(dev)
    ef = (torch.arange(g + 1) * (k + 1) * k).to(dev)
    for ref_node in (0, k - 1):
        qp = _qp(ref_node)
        for tg in (targets, None):
            want = _map_rows(rel, nb, poses, tg, ref_node, m)
            _agree(qp.from_map(rel, ei, _Map(poses), nb, query_targets=tg, edge_first=ef), want)
            _agree(qp.from_map(rel, ei, _Map(poses), nb, query_targets=tg), want)
        qp.check()
    # a neighbour outside [0, M): no fault, the row of the clamped index
    qp = _qp(0)
    for bad, clamped in ((m + 1000, m - 1), (-3, 0)):
        nb_bad, nb_ok = nb.clone(), nb.clone()
        nb_bad[2, 0], nb_ok[2, 0] = bad, clamped                          # node 1 of graph 2 is the source of its reference edge
        got = qp.from_map(rel, ei, _Map(poses), nb_bad, query_targets=targets, edge_first=ef)
        assert torch.equal(got, qp.from_map(rel, ei, _Map(poses), nb_ok, query_targets=targets, edge_first=ef))
        _agree(got, _map_rows(rel, nb_bad, poses, targets, 0, m))
    qp.check()


@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")], ids=["nan", "pinf", "ninf"])
def test_non_finite_inputs_propagate_like_the_host(dev, value):
    sizes = (8, 8, 8, 8)
    rel, ei, nf, ef, y = _fc_case(sizes, 11, dev)
    rel, y = rel.clone(), y.clone()
    rel[28, 1] = value                    # graph 0: translation part of the reference edge's rel pose (column 28 = 1 -> 0)
    rel[56 + 28, 4] = value               # graph 1: rotation part
    y[16, 0] = value                      # graph 2: the query's own target, translation
    y[24, 5] = value                      # graph 3: the query's own target, rotation
    qp = _qp(0)
    want = _host_rows(rel, ei, sizes, y, 0)
    got = qp.from_targets(rel, ei, nf, y, edge_first=ef)
    _agree(got, want)
    qp.check()                            # non-finite values are not bad graphs
    got = got.cpu().numpy()
    assert np.isnan(want[1, 3:7]).all() and np.isnan(want[3, 10:14]).all()
    assert want[1, 15] == 360.0 and want[3, 15] == 360.0      # a NaN dot: Python's max(-1.0, nan) = -1.0, acos(-1) = pi
    assert got[1, 15] == 360.0 and got[3, 15] == 360.0


def test_zero_rotation_is_the_unit_quaternion(dev):
    rel, ei, nf, ef, y = _fc_case((8, 8), 12, dev)
    rel, y = rel.clone(), y.clone()
    y[0, 3:] = 0.0                        # the query's own log q = 0
    rel[56 + 28, 3:] = y[9, 3:]           # graph 1: source - rel = 0 exactly
    got = _qp(0).from_targets(rel, ei, nf, y, edge_first=ef).cpu().numpy()
    assert got[0, 10:14].tolist() == [1.0, 0.0, 0.0, 0.0]
    assert got[1, 3:7].tolist() == [1.0, 0.0, 0.0, 0.0]
    _agree(got, _host_rows(rel, ei, (8, 8), y, 0))


def test_reference_golden_pose_utils(dev, golden_dir):
    """v, q, ang written by the reference's own pose_utils (qexp, quaternion_angular_error; ang[i] is the angle between q[i] and
    q[i + 1]), at the bounds test_eval_io.py holds the host functions to: 1e-12 on q, 1e-9 degrees on ang.

    The golden v are float64 values that fp32 cannot hold, and the kernel's inputs are fp32.  As the rotation RESIDUAL v[i] is
    fed exactly all the same: the source node's target holds hi = fp32(v[i]), the reference edge's relative pose -lo with
    lo = fp32(v[i] - hi), and hi - (-lo) in double is v[i] to 2^-48 |v| < 5e-15.  The query's own target is one fp32 row, so
    targ = qexp(fp32(v[i + 1])): its angle to q[i + 1] is at most 2 |d| rad with d = v[i + 1] - fp32(v[i + 1]) (exp is
    1-Lipschitz from log-quaternions to the unit sphere, and the rotation angle is twice the arc), and ang[i] is held to
    1e-9 + 2 |d| 180 / pi degrees (<= 1.5e-5): exactly 1e-9 where v[i + 1] is an fp32 value, which is ang[5] (v[0] = 0), and
    ang[0] too through one more graph with the roles of v[0] and v[1] swapped (the angle is symmetric)."""
    gold = np.load(os.path.join(golden_dir, "g6_pose_utils.npz"))
    v = gold["v"]
    pairs = [(i, (i + 1) % 6) for i in range(6)] + [(1, 0)]              # (residual, target)
    sizes = (2,) * len(pairs)
    rel, ei, nf, ef, y = _fc_case(sizes, 13, dev)
    rel, y = torch.zeros_like(rel), torch.zeros_like(y)
    slack = []
    for j, (a, b) in enumerate(pairs):
        hi = v[a].astype(np.float32)
        lo = (v[a] - hi.astype(np.float64)).astype(np.float32)
        assert np.abs(hi.astype(np.float64) + lo.astype(np.float64) - v[a]).max() < 5e-15
        y[2 * j + 1, 3:] = torch.from_numpy(hi)                          # node 1: the source of the reference edge 1 -> 0
        rel[2 * j + 1, 3:] = torch.from_numpy(-lo)                       # column 2 j + 1 is that edge
        w = v[b].astype(np.float32)
        y[2 * j, 3:] = torch.from_numpy(w)                               # node 0: the query's own target
        slack.append(2.0 * np.linalg.norm(v[b] - w.astype(np.float64)) * 180.0 / np.pi)
    assert slack[5] == 0.0 and slack[6] == 0.0 and max(slack) < 1.5e-5
    got = _qp(0).from_targets(rel, ei, nf, y, edge_first=ef).cpu().numpy()
    for j, (a, b) in enumerate(pairs):
        assert np.allclose(got[j, 3:7], gold["q"][a], atol=1e-12, rtol=0), j
        assert np.isclose(got[j, 15], gold["ang"][min(a, b) if {a, b} == {0, 1} else a], atol=1e-9 + slack[j], rtol=0), j
    assert np.allclose(got[5, 10:14], gold["q"][0], atol=1e-12, rtol=0)


def test_bad_graphs_are_nan_rows_and_reported(dev):
    sizes = (8, 3, 8)
    rel, ei, nf, ef, y = _fc_case(sizes, 14, dev)
    good = _host_rows(rel, ei, sizes, y, 0)
    # ref_node 2 is past the in-degree of the 3-node graph
    qp = _qp(2)
    want = _host_rows(rel, ei, sizes, y, 2)
    got = qp.from_targets(rel, ei, nf, y, edge_first=ef)
    assert np.isnan(want[1]).all() and np.isfinite(want[[0, 2]]).all()
    _agree(got, want)
    with pytest.raises(ValueError, match="no edge into node 0"):
        qp.check()
    qp.check()                                                            # reported once
    _agree(qp.from_targets(rel, ei, nf, y), want)                         # again, cut by the columns' targets
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        qp.check(wait=False)                                              # the report has landed: a look is enough
    rel2, ei2, nf2, ef2, y2 = _fc_case((8, 8), 15, dev)                   # a following good call is clean
    _agree(qp.from_targets(rel2, ei2, nf2, y2, edge_first=ef2), _host_rows(rel2, ei2, (8, 8), y2, 2))
    qp.check()
    # a reference edge whose source lies outside its graph
    qp = _qp(0)
    for outside in (0, 11, 30):                                           # another graph's node, before and after; past every node
        ei_bad = ei.clone()
        col = 56 + int(np.flatnonzero(ei[1, 56:62].cpu().numpy() == 8)[0])
        ei_bad[0, col] = outside
        got = qp.from_targets(rel, ei_bad, nf, y, edge_first=ef).cpu().numpy()
        assert np.isnan(got[1]).all()
        _agree(got[[0, 2]], good[[0, 2]])
        with pytest.raises(ValueError, match="no edge into node 0"):
            qp.check()
    _agree(qp.from_targets(rel, ei, nf, y, edge_first=ef), good)
    qp.check()
    # ops.query_pose without a status word reads the count back itself
    from relpose_gnn_amd import ops
    with pytest.raises(ValueError, match="no edge into node 0"):
        ops.query_pose(rel, ei, node_first=nf, node_targets=y, edge_first=ef, ref_node=2)


def test_deterministic_and_overwrites_every_slot(dev):
    sizes = tuple(2 + (i * 3) % 7 for i in range(40))
    rel, ei, nf, ef, y = _fc_case(sizes, 16, dev)
    qp = _qp(1)                                                           # 2-node graphs are bad: their rows are written too
    a = torch.empty((40, 16), dtype=torch.float64, device=dev)
    a.view(torch.uint8).fill_(0xFF)
    b = torch.zeros((40, 16), dtype=torch.float64, device=dev)
    assert qp.from_targets(rel, ei, nf, y, edge_first=ef, out=a) is a
    qp.from_targets(rel, ei, nf, y, edge_first=ef, out=b)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    assert torch.isnan(a).all(1).sum() == sum(n == 2 for n in sizes)
    with pytest.raises(ValueError):
        qp.check()


def test_capture_and_replay_equals_eager(dev):
    sizes = (8, 5, 12, 2)
    rel, ei, nf, ef, y = _fc_case(sizes, 17, dev)
    qp = _qp(0)
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
    assert torch.equal(out.view(torch.int64), eager.view(torch.int64))
    qp.check()


# ---- the two streams ------------------------------------------------------------------------------------------------------------
def _small(dev, seed=1, **kw):
    import relpose_gnn_amd.synth as S
    from relpose_gnn_amd.posenet import PoseNetX_R2
    from relpose_gnn_amd.resnet import ResNet
    planes, blocks = (8, 16, 32, 64), (1, 1, 1, 1)
    args = dict(droprate=0.0, knn=-1, use_AP=True, gnn_recursion=2, use_attention=False, L=1)
    args.update(kw)
    m = PoseNetX_R2(ResNet(blocks, planes), pretrained=False, feat_dim=64, edge_feat_dim=64, node_dim=64, input_img_height=32,
                    use_gnn=True, **args)
    sd = S.synth_state_dict(S.posenet_r2_param_shapes(64, 64, 64, planes, blocks), seed=seed)
    m.load_state_dict(sd)
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def models(dev):
    return {knn: _small(dev, knn=knn) for knn in (-1, 4)}


@pytest.mark.parametrize("knn", [-1, 4])
def test_evaluate_stream_device_equals_host(dev, models, knn):
    import relpose_gnn_amd.synth as S
    from relpose_gnn_amd.evaluate import evaluate_stream
    from relpose_gnn_amd.graph import Data, fc_edge_index
    m = models[knn]
    graphs = [Data(x=S.synth_images(8, 32, 40, seed=700 + i), edge_index=fc_edge_index(8), y=S.hash_normal(f"qp.y{i}", (8, 6), 0.3))
              for i in range(5)]
    sh, sd = {}, {}
    host = evaluate_stream(m, graphs, dev, micro_batch=2, pose_m=PM, pose_s=PS, stats=sh)
    devr = evaluate_stream(m, graphs, dev, micro_batch=2, pose_m=PM, pose_s=PS, stats=sd, postprocess="device")
    assert devr.pred_poses.shape == (5, 7) and devr.t_loss.shape == (5,) and np.isfinite(devr.q_loss).all()
    _agree_results(devr, host)
    assert (sh["postprocess"], sd["postprocess"]) == ("host", "device")
    assert sd["d2h_bytes"] == 5 * 16 * 8 and sd["d2h_bytes"] < sh["d2h_bytes"]
    assert sh["d2h_bytes"] >= 5 * 56 * 6 * 4 if knn < 0 else sh["d2h_bytes"] > 0
    # a graph without an edge into its query node: the ValueError of the host path
    bad = list(graphs)
    bad[3] = Data(x=graphs[3].x, edge_index=torch.tensor([[0, 2], [1, 1]]), y=graphs[3].y)
    if knn < 0:
        with pytest.raises(ValueError, match="no edge into node 0"):
            evaluate_stream(m, bad, dev, micro_batch=2, postprocess="device")


@pytest.mark.parametrize("knn", [-1, 4])
def test_relocalize_device_equals_host(dev, models, knn):
    import relpose_gnn_amd.synth as S
    from relpose_gnn_amd.evaluate import relocalize
    from relpose_gnn_amd.featmap import FeatureMap
    from relpose_gnn_amd.retrieval import RetrievalRule
    m = models[knn]
    gen = torch.Generator().manual_seed(31)
    mimgs, queries = S.synth_images(20, 32, 40, seed=91), S.synth_images(5, 32, 40, seed=92)
    poses, targets = torch.randn(20, 6, generator=gen) * 0.3, torch.randn(5, 6, generator=gen) * 0.3
    fmap = FeatureMap.build(m, mimgs, poses=poses, groups=torch.arange(20) // 4)
    nb = torch.stack([torch.randperm(20, generator=gen)[:7] for _ in range(5)])
    kw = dict(micro_batch=2, pose_m=PM, pose_s=PS)
    # given neighbours, with and without targets
    sh, sd = {}, {}
    host = relocalize(m, fmap, queries, nb, targets=targets, stats=sh, **kw)
    devr = relocalize(m, fmap, queries, nb, targets=targets, stats=sd, postprocess="device", **kw)
    _agree_results(devr, host)
    assert np.array_equal(devr.neighbours, host.neighbours) and np.array_equal(devr.neighbours, nb.numpy())
    assert (sh["postprocess"], sd["postprocess"]) == ("host", "device")
    assert sd["d2h_bytes"] == 5 * 16 * 8 and sd["d2h_bytes"] < sh["d2h_bytes"]
    pred_h = relocalize(m, fmap, queries, nb, **kw)
    pred_d = relocalize(m, fmap, queries.to(dev), nb.to(dev), postprocess="device", **kw)
    assert pred_d.shape == (5, 7) and pred_d.dtype == np.float64
    assert np.abs(pred_d - pred_h).max() <= 1e-12 * (1 + np.abs(pred_h).max())
    # a retrieval rule: the rows forward_map has just chosen feed the pose rule on the device
    qg = torch.arange(5) % 5
    rule_kw = dict(k=7, sampling_period=2)
    host = relocalize(m, fmap, queries, targets=targets, rule=RetrievalRule(**rule_kw), query_groups=qg, **kw)
    devr = relocalize(m, fmap, queries, targets=targets, rule=RetrievalRule(**rule_kw), query_groups=qg, postprocess="device", **kw)
    assert np.array_equal(devr.neighbours, host.neighbours)
    _agree_results(devr, host)
    pred_d = relocalize(m, fmap, queries, rule=RetrievalRule(**rule_kw), query_groups=qg, postprocess="device", **kw)
    assert np.abs(pred_d - host.pred_poses).max() <= 1e-12 * (1 + np.abs(host.pred_poses).max())
    # a map without poses keeps its raw return
    raw = relocalize(m, FeatureMap.build(m, mimgs), queries, nb, micro_batch=2, postprocess="device")
    assert isinstance(raw, tuple) and raw[0].shape == (40, 6)
