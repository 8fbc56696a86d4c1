"""``relocalize(..., capture=True)`` and ``graphed.GraphedForwardMap``: the micro-batch step of the map path replayed from a
captured HIP graph, against the same step issued eagerly.

The bar is bit-identity (``torch.equal`` / ``np.array_equal``), not a tolerance: the replay runs the same kernels with the same
launch geometry in the same stream order on the same inputs, so any difference is a bug of the capture -- a stale static buffer,
a missed dependency -- and not rounding.

Shapes: 64 x 64 images, a 12-row map with poses, K = 3, 10 queries in micro-batches of 4: two full chunks (the two-stream
schedule) and a tail of 2 (the one-stream path), so two captured shapes.  The model is the four-block encoder of
test_hip_featmap.py / test_hip_query_pose.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H = W = 64
M, K, G, MB = 12, 3, 10, 4
PM, PS = (1.5, -0.25, 3.0), (2.0, 0.5, 1.25)
RESULT_FIELDS = ("pred_poses", "targ_poses", "t_loss", "q_loss", "neighbours")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _small(dev, precision="f32", **kw):
    import relpose_gnn_amd.synth as S
    from relpose_gnn_amd.posenet import PoseNetX_R2
    from relpose_gnn_amd.resnet import ResNet
    planes, blocks = (8, 16, 32, 64), (1, 1, 1, 1)
    args = dict(droprate=0.0, knn=-1, use_AP=True, gnn_recursion=2, use_attention=False, L=1)
    args.update(kw)
    m = PoseNetX_R2(ResNet(blocks, planes), pretrained=False, feat_dim=64, edge_feat_dim=64, node_dim=64, input_img_height=H,
                    use_gnn=True, **args)
    m.load_state_dict(S.synth_state_dict(S.posenet_r2_param_shapes(64, 64, 64, planes, blocks, use_attention=args["use_attention"],
                                                                   use_AP=args["use_AP"], L=args["L"]), seed=1))
    m = m.to(dev).eval()
    m.encoder_dtype = m.gnn_dtype = precision
    return m


@pytest.fixture(scope="module")
def data():
    """Host inputs, made once: map images and poses, queries (rows 4..7 repeat rows 0..3: two micro-batches of the same images),
    targets, neighbours."""
    import relpose_gnn_amd.synth as S
    gen = torch.Generator().manual_seed(6)
    queries = S.synth_images(G, H, W, seed=92)
    queries[4:8] = queries[0:4]
    return dict(mimgs=S.synth_images(M, H, W, seed=91), queries=queries, poses=torch.randn(M, 6, generator=gen) * 0.3,
                targets=torch.randn(G, 6, generator=gen) * 0.3,
                nb=torch.randint(0, M, (G, K), generator=torch.Generator().manual_seed(11), dtype=torch.int64))


def _map(model, data, poses=True):
    from relpose_gnn_amd.featmap import FeatureMap
    return FeatureMap.build(model, data["mimgs"], poses=data["poses"] if poses else None)


def _rule():
    from relpose_gnn_amd.retrieval import RetrievalRule
    # the reference's draws (half of the positions dropped); seed 5 leaves every one of the 10 queries its 3 rows of 12
    return RetrievalRule.reference(k=K, sampling_period=1, seed=5)


def _same_results(a, b):
    for f in RESULT_FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert x.shape == y.shape and np.array_equal(x, y), f
    assert np.isfinite(a.pred_poses).all()


# ---- 1. bit-identity to the eager stream --------------------------------------------------------------------------------------
@pytest.mark.parametrize("fuse", [None, "mean"])
@pytest.mark.parametrize("postprocess", ["host", "device"])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_capture_equals_eager(dev, data, precision, postprocess, fuse):
    from relpose_gnn_amd.evaluate import relocalize
    m = _small(dev, precision)
    fmap, bare = _map(m, data), _map(m, data, poses=False)
    kw = dict(micro_batch=MB, pose_m=PM, pose_s=PS, targets=data["targets"], postprocess=postprocess, fuse=fuse)
    q, nb = data["queries"], data["nb"]
    # given neighbours
    st = {}
    _same_results(relocalize(m, fmap, q, nb, capture=True, stats=st, **kw), relocalize(m, fmap, q, nb, **kw))
    assert st["graphs_captured"] == 2 and st["graph_replays"] == 3 and st["micro_batches"] == 3
    # retrieved neighbours, a seeded random rule: the same draws from a fresh rule of the same seed
    cap, eager = relocalize(m, fmap, q, rule=_rule(), capture=True, **kw), relocalize(m, fmap, q, rule=_rule(), **kw)
    _same_results(cap, eager)
    # from queries that are already on the device (no staging)
    _same_results(relocalize(m, fmap, q.to(dev), nb.to(dev), capture=True, **kw), relocalize(m, fmap, q.to(dev), nb.to(dev), **kw))
    # without targets: the poses alone
    kw.pop("targets")
    assert np.array_equal(relocalize(m, fmap, q, nb, capture=True, **kw), relocalize(m, fmap, q, nb, **kw))
    # a map without poses: the raw (abs, rel) pair
    (ab, rel), (ab0, rel0) = relocalize(m, bare, q, nb, capture=True, **kw), relocalize(m, bare, q, nb, **kw)
    assert ab.shape == (G * (K + 1), 6) and rel.shape == (G * K * (K + 1), 6)
    assert torch.equal(ab, ab0) and torch.equal(rel, rel0) and torch.isfinite(rel).all()


# ---- 2. per-call inputs change under replay ------------------------------------------------------------------------------------
def test_random_rule_draws_anew_on_every_replay(dev, data):
    """Micro-batches 0 and 1 hold the SAME four images and replay the same graph: their neighbours differ because the host's
    draws, copied into the static ranks before each replay, differ -- exactly as they do eagerly."""
    from relpose_gnn_amd.evaluate import relocalize
    m = _small(dev)
    fmap = _map(m, data)
    kw = dict(micro_batch=MB, pose_m=PM, pose_s=PS, targets=data["targets"], postprocess="device")
    s_cap, s_eager = {}, {}
    cap = relocalize(m, fmap, data["queries"], rule=_rule(), capture=True, stats=s_cap, **kw)
    eager = relocalize(m, fmap, data["queries"], rule=_rule(), stats=s_eager, **kw)
    assert s_cap["graphs_captured"] == 2
    assert np.array_equal(s_cap["neighbours"], s_eager["neighbours"]) and np.array_equal(cap.neighbours, eager.neighbours)
    nb = cap.neighbours
    assert nb.shape == (G, K) and not np.array_equal(nb[0:4], nb[4:8])
    assert (np.diff(np.sort(nb, 1), axis=1) > 0).all() and nb.min() >= 0 and nb.max() < M     # K distinct map rows per query
    _same_results(cap, eager)


def test_replay_reads_the_neighbours_of_the_call(dev, data):
    from relpose_gnn_amd.graphed import GraphedForwardMap
    m = _small(dev)
    fmap = _map(m, data)
    q = data["queries"][:4].to(dev)
    step = GraphedForwardMap(m, fmap, q, K)
    for seed in (1, 2):
        nb = torch.randint(0, M, (4, K), generator=torch.Generator().manual_seed(seed), dtype=torch.int64).to(dev)
        want = [t.clone() for t in m.forward_map(q, nb, fmap)]
        out = step(q, nb)
        assert out.rows is None and torch.equal(out.neighbours, nb)
        assert torch.equal(out.abs_pose, want[0]) and torch.equal(out.rel_pose, want[1]) and torch.equal(out.edge_index, want[2])
    # the caller may fill the static input itself: a tensor that IS the static buffer is not copied
    step.queries.copy_(data["queries"][4:8].view_as(step.queries))            # rows 4..7 repeat rows 0..3
    out = step(step.queries, nb)
    assert torch.equal(out.abs_pose, want[0]) and torch.equal(out.rel_pose, want[1])


# ---- 3. cache and invalidation ---------------------------------------------------------------------------------------------------
def test_cache_and_invalidation(dev, data):
    import relpose_gnn_amd.synth as S
    from relpose_gnn_amd.evaluate import relocalize
    from relpose_gnn_amd.graphed import GraphedForwardMap
    m = _small(dev)
    fmap = _map(m, data)
    q, nb = data["queries"], data["nb"]
    kw = dict(micro_batch=MB, pose_m=PM, pose_s=PS, targets=data["targets"], postprocess="device")

    def run():
        st = {}
        res = relocalize(m, fmap, q, nb, capture=True, stats=st, **kw)
        _same_results(res, relocalize(m, fmap, q, nb, **kw))
        return st["graphs_captured"], st["graph_replays"]

    assert run() == (2, 3)
    assert run() == (0, 3)                                    # the same shapes again: nothing to capture
    qd, nbd = q[:4].to(dev), nb[:4].to(dev)
    held = GraphedForwardMap(m, fmap, qd, K)
    held(qd, nbd)
    m.refresh_packed()
    with pytest.raises(RuntimeError, match="stale"):
        held(qd, nbd)
    assert run() == (2, 3)                                    # ... captured again, over the re-packed weights
    assert run() == (0, 3)
    held = GraphedForwardMap(m, fmap, qd, K)
    fmap.extend(m, S.synth_images(3, H, W, seed=93), poses=torch.zeros(3, 6))
    with pytest.raises(RuntimeError, match="stale"):
        held(qd, nbd)                                         # the map's tensors were replaced: no replay over the old ones
    assert len(fmap) == M + 3 and run() == (2, 3)
    m.check_edge_index()


# ---- 4. the deferred index contract ------------------------------------------------------------------------------------------------
def test_bad_neighbour_is_reported_after_a_replay(dev, data):
    from relpose_gnn_amd.graphed import GraphedForwardMap
    m = _small(dev)
    fmap = _map(m, data)
    q = data["queries"][:4].to(dev)
    good = data["nb"][:4].to(dev)
    bad = good.clone()
    bad[2, 1] = M                                             # one past the map's last row: clamped and counted
    m.forward_map(q, bad, fmap)
    with pytest.raises(IndexError) as eager:
        m.check_edge_index()
    step = GraphedForwardMap(m, fmap, q, K)
    out = step(q, bad)
    assert torch.isfinite(out.rel_pose).all()
    with pytest.raises(IndexError, match="neighbours has 1 index") as replayed:
        m.check_edge_index()
    assert str(replayed.value) == str(eager.value)
    step(q, good)
    m.check_edge_index()                                      # the counters were cleared: a clean replay reports nothing


# ---- 5. one query at a time ------------------------------------------------------------------------------------------------------
def test_one_query_at_a_time(dev, data):
    from relpose_gnn_amd.graphed import GraphedForwardMap
    from relpose_gnn_amd.query_pose import QueryPose
    m = _small(dev)
    fmap = _map(m, data)
    q, nb, targets = data["queries"].to(dev), data["nb"].to(dev), data["targets"].to(dev)
    pose, eager_pose = QueryPose(PM, PS), QueryPose(PM, PS)
    step = GraphedForwardMap(m, fmap, q[:1], K, pose=pose, pose_kwargs={"query_targets": targets[:1]})
    for g in (0, 1, 2, 3, 9):
        ab, rel, ei = m.forward_map(q[g:g + 1], nb[g:g + 1], fmap)
        rows = eager_pose.from_map(rel, ei, fmap, nb[g:g + 1], query_targets=targets[g:g + 1])
        out = step(q[g:g + 1], nb[g:g + 1], query_targets=targets[g:g + 1])
        assert torch.equal(out.abs_pose, ab) and torch.equal(out.rel_pose, rel) and torch.equal(out.rows, rows)
        assert out.rows.shape == (1, 16) and torch.isfinite(out.rows).all()
    pose.check()
    m.check_edge_index()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(droprate=0.5), dict(knn=4)], ids=["droprate", "knn"])
def test_refused_models(dev, data, kw):
    from relpose_gnn_amd.evaluate import relocalize
    from relpose_gnn_amd.graphed import GraphedForwardMap
    m = _small(dev, **kw)
    fmap = _map(m, data)
    q, nb = data["queries"][:4].to(dev), data["nb"][:4].to(dev)
    with pytest.raises(NotImplementedError, match="graph capture covers the deterministic fully-connected path"):
        GraphedForwardMap(m, fmap, q, K)
    with pytest.raises(NotImplementedError, match="graph capture covers the deterministic fully-connected path"):
        relocalize(m, fmap, data["queries"], data["nb"], micro_batch=MB, capture=True)
    assert not m._map_captures
    ab, rel, _ = m.forward_map(q, nb, fmap)                   # nothing is left half-captured
    assert torch.isfinite(ab).all() and torch.isfinite(rel).all()
    m.check_edge_index()


def test_refused_inputs(dev, data):
    from relpose_gnn_amd.evaluate import relocalize
    from relpose_gnn_amd.graphed import GraphedForwardMap
    m = _small(dev)
    fmap = _map(m, data)
    q, nb = data["queries"][:4].to(dev), data["nb"][:4].to(dev)
    frames = torch.zeros((4, H, W, 3), dtype=torch.uint8, device=dev)
    with pytest.raises(TypeError, match="uint8"):
        GraphedForwardMap(m, fmap, frames, K)
    with pytest.raises(TypeError, match="uint8"):
        relocalize(m, fmap, frames, nb, micro_batch=MB, capture=True)
    step = GraphedForwardMap(m, fmap, q, K)
    want = [t.clone() for t in step(q, nb)[:2]]
    with pytest.raises(ValueError, match="captured for queries"):
        step(q[:3], nb[:3])
    with pytest.raises(ValueError, match="captured for neighbours"):
        step(q, nb[:, :2])
    with pytest.raises(ValueError, match="captured for queries"):
        step(q.to(torch.bfloat16), nb)
    with pytest.raises(ValueError, match="captured without"):
        step(q, nb, query_targets=data["targets"][:4].to(dev))
    out = step(q, nb)                                         # the refused calls touched nothing
    assert torch.equal(out.abs_pose, want[0]) and torch.equal(out.rel_pose, want[1])
    ab, rel, _ = m.forward_map(q, nb, fmap)
    assert torch.equal(ab, want[0]) and torch.equal(rel, want[1])
    m.check_edge_index()
