"""The pose gate through the map path on the GPU: forward_map(prior=, gate=) against forward_map(neighbours=<the reference's
rows>) bit for bit (both output modes, a static_knn model), relocalize(priors=, gate=) against itself captured, the reported gate
states against tests/pose_gate_ref.py, and a gated captured step going stale with its map.  The small model of
tests/test_hip_mc_capture.py, without dropout."""
import numpy as np
import pytest
import torch

import pose_gate_ref as R

pytestmark = pytest.mark.gpu

H = W = 64
M, K, G, MB = 24, 3, 10, 4
PM, PS = (1.5, -0.25, 3.0), (2.0, 0.5, 1.25)
RESULT_FIELDS = ("pred_poses", "targ_poses", "t_loss", "q_loss", "neighbours", "gate_state")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _small(dev, **kw):
    import relpose_gnn_amd.synth as S
    from relpose_gnn_amd.posenet import PoseNetX_R2
    from relpose_gnn_amd.resnet import ResNet
    planes, blocks = (8, 16, 32, 64), (1, 1, 1, 1)
    args = dict(droprate=0.0, knn=-1, use_AP=True, gnn_recursion=2, use_attention=False, L=1)
    static = kw.pop("static_knn", False)
    args.update(kw)
    m = PoseNetX_R2(ResNet(blocks, planes), pretrained=False, feat_dim=64, edge_feat_dim=64, node_dim=64, input_img_height=H,
                    use_gnn=True, **args)
    m.load_state_dict(S.synth_state_dict(S.posenet_r2_param_shapes(64, 64, 64, planes, blocks), seed=1))
    m = m.to(dev).eval()
    m.static_knn = static
    return m


@pytest.fixture(scope="module")
def data():
    """Map poses on a line, one unit apart in normalised x (two after pose_s), rotating 8 degrees about z per row; groups of
    three consecutive rows.  Priors: the gate row of a map row a little displaced (gated), NaN (no prior), far away (fallback),
    and one whose group leaves fewer than K rows inside (fallback)."""
    import relpose_gnn_amd.synth as S
    gen = torch.Generator().manual_seed(6)
    poses = torch.zeros(M, 6)
    poses[:, 0] = torch.arange(M, dtype=torch.float32)
    poses[:, 1:3] = torch.randn(M, 2, generator=gen) * 0.05
    poses[:, 5] = torch.deg2rad(torch.arange(M, dtype=torch.float32) * 8.0) / 2.0        # log q of a rotation about z
    return dict(mimgs=S.synth_images(M, H, W, seed=91), queries=S.synth_images(G, H, W, seed=92), poses=poses,
                targets=torch.randn(G, 6, generator=gen) * 0.3, groups=torch.arange(M) // 3)


def _map(model, data, groups=True):
    from relpose_gnn_amd.featmap import FeatureMap
    return FeatureMap.build(model, data["mimgs"], poses=data["poses"], groups=data["groups"] if groups else None)


def _gate():
    from relpose_gnn_amd.retrieval import PoseGate
    return PoseGate(5.0, 50.0, pose_m=PM, pose_s=PS)          # +-2 rows in translation (4 units), +-6 in rotation: 5 rows inside


def _priors(fmap, gate, g):
    rows = fmap.gate_rows(gate).cpu().numpy()
    prior = rows[(np.arange(g) * 5 + 3) % M].copy()
    prior[:, :3] += 0.01
    prior[1::4] = np.nan                                      # no prior
    prior[2::4, 1] += 500.0                                   # nothing inside
    return prior


def _reference(dev, model, fmap, gate, rule, queries, prior, qg):
    """(gate_info, neighbours) by the yardstick: pose_gate_ref's row set, ranked by the existing kernel per query."""
    from relpose_gnn_amd import ops
    g = queries.shape[0]
    ranks = rule.ranks([M] * g)
    info, used = R.gated_rows(fmap.gate_rows(gate).cpu().numpy(), prior, gate.r2, gate.cos_half if gate.rot else None, ranks,
                              qg, None if qg is None else fmap.groups_host.numpy())
    qf = model.encode(queries)
    one = torch.ones(1, dtype=torch.int64, device=dev)
    groups = torch.as_tensor(np.where(used, 0, 1).astype(np.int64)).to(dev)
    rt = torch.as_tensor(ranks).to(dev)
    nb = torch.cat([ops.retrieve(qf[i:i + 1], fmap.features, rt[i:i + 1], q_group=one, db_group=groups[i]) for i in range(g)])
    return info, nb


@pytest.mark.parametrize("kind", ["fc", "static_knn"])
@pytest.mark.parametrize("outputs", ["all", "query"])
def test_forward_map_gated_equals_given_reference_neighbours(dev, data, outputs, kind):
    from relpose_gnn_amd.retrieval import RetrievalRule
    m = _small(dev, **({"knn": 2, "static_knn": True} if kind == "static_knn" else {}))
    fmap, gate, rule = _map(m, data), _gate(), RetrievalRule(k=K)
    q = data["queries"].to(dev)
    prior = _priors(fmap, gate, G)
    # query 3: a group elsewhere (rows 0..2); query 4: the prior on the last row, 3 rows inside = need; query 8: the prior on row
    # 19, whose group (rows 18..20) leaves 2 rows inside -- fallback
    qg = [-1, -1, -1, 0, -1, -1, -1, -1, 6, -1]
    info, nb_ref = _reference(dev, m, fmap, gate, rule, q, prior, qg)
    assert set(info[:, 0].tolist()) == {0, 1, 2} and (info[info[:, 0] == 0, 1] >= K).all()
    ab, rel, ei, nb = m.forward_map(q, None, fmap, rule=rule, query_groups=qg, outputs=outputs, prior=prior, gate=gate)
    got_info = m.gate_info.clone()
    want = m.forward_map(q, nb_ref, fmap, outputs=outputs)
    assert m.gate_info is None                                # a call without a gate leaves none behind
    assert torch.equal(nb, nb_ref) and np.array_equal(got_info.cpu().numpy(), info)
    for u, v in zip((ab, rel, ei), want):
        assert torch.equal(u, v)
    assert torch.isfinite(rel).all()
    # the gate did change the rows of the gated queries, and a device prior is taken as it is
    plain = m.forward_map(q, None, fmap, rule=rule, query_groups=qg, outputs=outputs)[3]
    gated = torch.as_tensor(info[:, 0] == 0).to(dev)
    assert torch.equal(plain[~gated], nb[~gated]) and not torch.equal(plain[gated], nb[gated])
    again = m.forward_map(q, None, fmap, rule=rule, query_groups=qg, outputs=outputs, prior=torch.as_tensor(prior).to(dev), gate=gate)
    assert torch.equal(again[3], nb) and torch.equal(again[1], rel)
    m.check_edge_index()


@pytest.mark.parametrize("postprocess,fuse", [("host", None), ("device", None), ("device", "consensus")])
def test_relocalize_gated_capture_equals_eager(dev, data, postprocess, fuse):
    """Three micro-batches, the last one ragged (two captured shapes): every result field equal, the states the reference's."""
    from relpose_gnn_amd.evaluate import relocalize
    from relpose_gnn_amd.retrieval import RetrievalRule
    m = _small(dev)
    fmap, gate, rule = _map(m, data, groups=False), _gate(), RetrievalRule(k=K)
    prior = _priors(fmap, gate, G)
    info, nb_ref = _reference(dev, m, fmap, gate, rule, data["queries"].to(dev), prior, None)
    kw = dict(micro_batch=MB, pose_m=PM, pose_s=PS, targets=data["targets"], postprocess=postprocess, fuse=fuse, rule=rule,
              priors=prior, gate=gate, outputs="query")
    st_e, st_c = {}, {}
    eager = relocalize(m, fmap, data["queries"], stats=st_e, **kw)
    cap = relocalize(m, fmap, data["queries"], capture=True, stats=st_c, **kw)
    assert st_c["graphs_captured"] == 2 and st_c["graph_replays"] == 3
    for f in RESULT_FIELDS:
        x, y = getattr(cap, f), getattr(eager, f)
        assert x.shape == y.shape and np.array_equal(x, y), f
    assert np.isfinite(eager.pred_poses).all()
    for st in (st_e, st_c):
        assert np.array_equal(st["gate_state"], info[:, 0]) and np.array_equal(st["gate_rows"], info[:, 1])
    assert np.array_equal(eager.gate_state, info[:, 0]) and set(info[:, 0].tolist()) == {0, 1, 2}
    assert np.array_equal(eager.neighbours, nb_ref.cpu().numpy())
    # the held steps serve other priors (a device tensor this time) without a new capture, and another gate captures anew
    other = np.roll(prior, 1, axis=0)
    st = {}
    again = relocalize(m, fmap, data["queries"], capture=True, stats=st, **dict(kw, priors=torch.as_tensor(other).to(dev)))
    assert st["graphs_captured"] == 0
    assert np.array_equal(again.neighbours, relocalize(m, fmap, data["queries"], **dict(kw, priors=other)).neighbours)
    from relpose_gnn_amd.retrieval import PoseGate
    relocalize(m, fmap, data["queries"], capture=True, stats=st, **dict(kw, gate=PoseGate(7.0, pose_m=PM, pose_s=PS)))
    assert st["graphs_captured"] == 2
    with pytest.raises(ValueError, match="pose gate restricts retrieval"):
        relocalize(m, fmap, data["queries"], nb_ref, priors=prior, gate=gate)
    m.check_edge_index()


def test_gated_step_goes_stale_with_the_map(dev, data):
    from relpose_gnn_amd.graphed import GraphedForwardMap
    from relpose_gnn_amd.retrieval import RetrievalRule
    m = _small(dev)
    fmap, gate, rule = _map(m, data, groups=False), _gate(), RetrievalRule(k=K)
    q = data["queries"][:MB].to(dev)
    prior = _priors(fmap, gate, MB)
    step = GraphedForwardMap(m, fmap, q, rule=rule, gate=gate, outputs="query")
    assert torch.isnan(step.prior).all()                      # the capture ran without a prior
    out = step(q, prior=prior)
    info, nb_ref = _reference(dev, m, fmap, gate, rule, q, prior, None)
    assert torch.equal(out.neighbours, nb_ref) and np.array_equal(step.gate_info.cpu().numpy(), info)
    first = out.neighbours.clone()
    assert torch.equal(step(q).neighbours, first)             # prior=None: the buffer as it is
    held = step._held["gate_rows"]
    assert held is fmap.gate_rows(gate) and not step.stale()
    fmap.extend(m, data["mimgs"][:2], poses=data["poses"][:2])
    assert not fmap._gate_rows                                # dropped like the inverse norms
    assert step._sign(step._reads())[-1] != step._signature[-1]
    with pytest.raises(RuntimeError, match="stale"):
        step(q, prior=prior)
    with pytest.raises(ValueError, match="captured without a gate"):
        GraphedForwardMap(m, fmap, q, rule=rule, outputs="query")(q, prior=prior)
    m.check_edge_index()
