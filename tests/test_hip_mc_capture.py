"""The captured map step with the always-on dropout sampled by model.mc_dropout: graphed.GraphedForwardMap and
relocalize(capture=True) accept droprate > 0 when -- and only when -- the sampler is set; the kernel that advances the draw
counter is part of the graph, so replay i equals the eager forward of draw i bit for bit."""
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


def _small(dev, mc=True, **kw):
    import relpose_gnn_amd.synth as S
    from relpose_gnn_amd.mc_dropout import McDropout
    from relpose_gnn_amd.posenet import PoseNetX_R2
    from relpose_gnn_amd.resnet import ResNet
    planes, blocks = (8, 16, 32, 64), (1, 1, 1, 1)
    args = dict(droprate=0.5, knn=-1, use_AP=True, gnn_recursion=2, use_attention=False, L=1)
    args.update(kw)
    m = PoseNetX_R2(ResNet(blocks, planes), pretrained=False, feat_dim=64, edge_feat_dim=64, node_dim=64, input_img_height=H,
                    use_gnn=True, **args)
    m.load_state_dict(S.synth_state_dict(S.posenet_r2_param_shapes(64, 64, 64, planes, blocks), seed=1))
    m = m.to(dev).eval()
    if mc:
        m.mc_dropout = McDropout(samples=8, seed=2026)
    return m


@pytest.fixture(scope="module")
def data():
    import relpose_gnn_amd.synth as S
    gen = torch.Generator().manual_seed(6)
    return dict(mimgs=S.synth_images(M, H, W, seed=91), queries=S.synth_images(G, H, W, seed=92),
                poses=torch.randn(M, 6, generator=gen) * 0.3, targets=torch.randn(G, 6, generator=gen) * 0.3,
                nb=torch.randint(0, M, (G, K), generator=torch.Generator().manual_seed(11), dtype=torch.int64))


def _map(model, data):
    from relpose_gnn_amd.featmap import FeatureMap
    return FeatureMap.build(model, data["mimgs"], poses=data["poses"])


@pytest.mark.parametrize("outputs", ["all", "query"])
@pytest.mark.parametrize("with_pose", [False, True], ids=["forward", "pose"])
def test_replay_i_is_the_eager_forward_of_draw_i(dev, data, with_pose, outputs):
    from relpose_gnn_amd.graphed import GraphedForwardMap
    from relpose_gnn_amd.query_pose import QueryPose
    m = _small(dev)
    fmap = _map(m, data)
    q, nb, targets = data["queries"][:4].to(dev), data["nb"][:4].contiguous().to(dev), data["targets"][:4].to(dev)
    pose = eager_pose = None
    kw = {}
    if with_pose:
        pose, eager_pose = QueryPose(PM, PS), QueryPose(PM, PS)
        kw = dict(pose=pose, pose_kwargs={"query_targets": targets})
    m.mc_dropout.reset(0)
    step = GraphedForwardMap(m, fmap, q, K, outputs=outputs, **kw)
    assert m.mc_dropout.draw == 0                              # capturing a step draws nothing
    want = []
    for i in range(3):
        m.mc_dropout.reset(i)
        ab, rel, ei = m.forward_map(q, nb, fmap, outputs=outputs)
        rows = None if pose is None else eager_pose.from_map(rel, ei, fmap, nb, query_targets=targets)
        spread = m.mc_dropout.last
        want.append([t.clone() for t in (ab, rel, spread.abs_var, spread.rel_var)] + [None if rows is None else rows.clone()])
    m.mc_dropout.reset(0)
    got = []
    for i in range(3):
        out = step(q, nb, **({"query_targets": targets} if with_pose else {}))
        assert m.mc_dropout.draw == i + 1
        spread = m.mc_dropout.last
        got.append([t.clone() for t in (out.abs_pose, out.rel_pose, spread.abs_var, spread.rel_var)]
                   + [None if out.rows is None else out.rows.clone()])
    torch.cuda.synchronize()
    for i in range(3):
        for u, v in zip(got[i][:4], want[i][:4]):
            assert torch.equal(u, v), i
        if with_pose:
            assert torch.equal(got[i][4], want[i][4]) and torch.isfinite(got[i][4]).all()
    assert not torch.equal(got[1][1], got[0][1]) and not torch.equal(got[2][1], got[1][1])      # consecutive replays differ
    m.check_edge_index()
    if with_pose:
        pose.check()


def _same_results(a, b):
    for f in RESULT_FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert x.shape == y.shape and np.array_equal(x, y), f
    assert np.isfinite(a.pred_poses).all()


@pytest.mark.parametrize("postprocess", ["host", "device"])
def test_relocalize_capture_equals_eager(dev, data, postprocess):
    """From the same draw the captured stream equals the eager one field for field (three micro-batches, the last one ragged: two
    captured shapes), and both leave the counter one further."""
    from relpose_gnn_amd.evaluate import relocalize
    m = _small(dev)
    fmap = _map(m, data)
    kw = dict(micro_batch=MB, pose_m=PM, pose_s=PS, targets=data["targets"], postprocess=postprocess)
    st = {}
    m.mc_dropout.reset(0)
    cap = relocalize(m, fmap, data["queries"], data["nb"], capture=True, stats=st, **kw)
    assert st["graphs_captured"] == 2 and st["graph_replays"] == 3 and m.mc_dropout.draw == 1
    m.mc_dropout.reset(0)
    eager = relocalize(m, fmap, data["queries"], data["nb"], **kw)
    assert m.mc_dropout.draw == 1
    _same_results(cap, eager)
    again = relocalize(m, fmap, data["queries"], data["nb"], capture=True, stats=st, **kw)      # draw 1: replays of the held steps
    assert st["graphs_captured"] == 0 and not np.array_equal(again.pred_poses, cap.pred_poses)
    _same_results(again, relocalize_from(m, fmap, data, 1, kw))


def relocalize_from(m, fmap, data, draw, kw):
    from relpose_gnn_amd.evaluate import relocalize
    m.mc_dropout.reset(draw)
    return relocalize(m, fmap, data["queries"], data["nb"], **kw)


def test_refused_without_the_sampler(dev, data):
    from relpose_gnn_amd.evaluate import relocalize
    from relpose_gnn_amd.graphed import GraphedForwardMap
    m = _small(dev, mc=False)
    fmap = _map(m, data)
    q = data["queries"][:4].to(dev)
    with pytest.raises(NotImplementedError, match="graph capture covers the deterministic fully-connected path"):
        GraphedForwardMap(m, fmap, q, K)
    with pytest.raises(NotImplementedError, match="graph capture covers the deterministic fully-connected path"):
        relocalize(m, fmap, data["queries"], data["nb"], micro_batch=MB, capture=True)
    assert not m._map_captures
    knn = _small(dev, knn=4)                                   # the kNN refusal stays, sampler or not
    with pytest.raises(NotImplementedError, match="graph capture covers the deterministic fully-connected path"):
        GraphedForwardMap(knn, fmap, q, K)


def test_held_step_goes_stale(dev, data):
    from relpose_gnn_amd.graphed import GraphedForwardMap
    from relpose_gnn_amd.mc_dropout import McDropout
    m = _small(dev)
    fmap = _map(m, data)
    q, nb = data["queries"][:4].to(dev), data["nb"][:4].contiguous().to(dev)
    held = GraphedForwardMap(m, fmap, q, K)
    held(q, nb)
    assert held._held["mc_state"] is m.mc_dropout._state
    m.refresh_packed()
    with pytest.raises(RuntimeError, match="stale"):
        held(q, nb)
    held = GraphedForwardMap(m, fmap, q, K)
    held(q, nb)
    m.mc_dropout = McDropout(samples=8, seed=2026)             # another sampler: another state tensor than the graph reads
    with pytest.raises(RuntimeError, match="stale"):
        held(q, nb)
    m.check_edge_index()
