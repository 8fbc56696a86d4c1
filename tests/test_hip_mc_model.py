"""model.mc_dropout (mc_dropout.McDropout) on a small model (D = 64, droprate = 0.5, G = 4 queries, K = 3 map images each): the
forwards return the sample means of ops.pose_heads_mc over the features of the same launches, with masks that follow the node ids
-- so the output mode, the number of streams and the micro-batch size change a pose only as the GEMMs' tilings do (1e-4), where
the torch-drawn masks of the same model change it at order 1."""
import numpy as np
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

H = W = 64
M, K, G = 12, 3, 4
S, SEED = 16, 77
TOL = 1e-4                    # the project's fp32 parity bar


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _small(dev, precision="f32", **kw):
    import relpose_gnn_amd.synth as Sy
    from relpose_gnn_amd.posenet import PoseNetX_R2
    from relpose_gnn_amd.resnet import ResNet
    planes, blocks = (8, 16, 32, 64), (1, 1, 1, 1)
    args = dict(droprate=0.5, knn=-1, use_AP=True, gnn_recursion=2, use_attention=False, L=1)
    args.update(kw)
    m = PoseNetX_R2(ResNet(blocks, planes), pretrained=False, feat_dim=64, edge_feat_dim=64, node_dim=64, input_img_height=H,
                    use_gnn=True, **args)
    m.load_state_dict(Sy.synth_state_dict(Sy.posenet_r2_param_shapes(64, 64, 64, planes, blocks, use_AP=args["use_AP"]), seed=1))
    m = m.to(dev).eval()
    m.encoder_dtype = m.gnn_dtype = precision
    return m


@pytest.fixture(scope="module")
def data():
    import relpose_gnn_amd.synth as Sy
    gen = torch.Generator().manual_seed(6)
    return dict(mimgs=Sy.synth_images(M, H, W, seed=91), queries=Sy.synth_images(8, H, W, seed=92),
                poses=torch.randn(M, 6, generator=gen) * 0.3, targets=torch.randn(8, 6, generator=gen) * 0.3,
                nb=torch.randint(0, M, (8, K), generator=torch.Generator().manual_seed(11), dtype=torch.int64))


@pytest.fixture(scope="module")
def setup(dev, data):
    """One model with mc_dropout and its map, shared by the tests below (none changes the weights; each resets the draw)."""
    from relpose_gnn_amd.featmap import FeatureMap
    from relpose_gnn_amd.mc_dropout import McDropout
    m = _small(dev)
    m.mc_dropout = McDropout(samples=S, seed=SEED)
    return m, FeatureMap.build(m, data["mimgs"], poses=data["poses"])


def _forward_map(m, fmap, q, nb, outputs, streams, draw=0):
    m.hip_streams = streams
    m.mc_dropout.node_base = 0
    m.mc_dropout.reset(draw)
    out = m.forward_map(q, nb, fmap, outputs=outputs)
    torch.cuda.synchronize()
    m.check_edge_index()
    return out


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("outputs", ["all", "query"])
def test_forward_map_is_pose_heads_mc_on_the_features(dev, data, setup, outputs, streams):
    """Bit for bit: the outputs and .last are ops.pose_heads_mc over the features of the same GNN launches on the same shapes
    (per stream slot), node rows numbered by their node of the whole batch, edge rows by their end points."""
    from relpose_gnn_amd import _lib, ops
    m, fmap = setup
    q, nb = data["queries"][:G].to(dev), data["nb"][:G].contiguous().to(dev)
    ab, rel, ei = _forward_map(m, fmap, q, nb, outputs, streams, draw=5)
    last = m.mc_dropout.last
    n_per = K + 1
    assert ab.shape == ((G, 6) if outputs == "query" else (G * n_per, 6)) and rel.shape == (ei.shape[1], 6)
    assert last.abs_var.shape == ab.shape and last.rel_var.shape == rel.shape
    assert bool((last.abs_var > 0).all()) and bool((last.rel_var > 0).all())
    state = torch.tensor([5, 0], dtype=torch.int32, device=dev)
    t = m._gnn_packed
    want = {"ab": [], "rel": [], "abv": [], "relv": []}
    for g0, g1 in ([(0, G)] if streams == 1 else [(0, G // 2), (G // 2, G)]):
        n0 = g0 * n_per
        edges, _ = m._map_graph(g1 - g0, n_per, dev)
        nodes = ops.gather_graph_nodes(m.encode(q[g0:g1]), fmap.features, nb[g0:g1])
        if outputs == "query":
            sel, qn, sel_edges = m._map_query(g1 - g0, n_per, dev)
            node_f, edge_f = ops.gnn_forward_query(t, nodes, edges, sel, qn, 2, want_features=True)[2:]
            node_ids, edge_ids = qn, sel_edges
        else:
            n, e = nodes.shape[0], edges.shape[1]
            node_f, edge_f = torch.empty((n, 64), device=dev), torch.empty((e, 64), device=dev)
            scratch = torch.empty((n, 6), device=dev), torch.empty((e, 6), device=dev)
            m._gnn_call(_lib.lib(), nodes, edges.data_ptr(), edges.data_ptr() + 8 * e, 0, n, e, scratch[0], scratch[1], node_f, edge_f,
                        m._counters.counters[0:1], 5)
            node_ids, edge_ids = None, edges
        a_mean, a_var = ops.pose_heads_mc(node_f, t[18], t[19], 0.5, S, SEED, state, node_ids, n0)
        r_mean, r_var = ops.pose_heads_mc(edge_f, t[20], t[21], 0.5, S, SEED, state, edge_ids, n0)
        for key, v in zip(("ab", "abv", "rel", "relv"), (a_mean, a_var, r_mean, r_var)):
            want[key].append(v)
    torch.cuda.synchronize()
    assert torch.equal(ab, torch.cat(want["ab"])) and torch.equal(rel, torch.cat(want["rel"]))
    assert torch.equal(last.abs_var, torch.cat(want["abv"])) and torch.equal(last.rel_var, torch.cat(want["relv"]))


def _query_rows(ab, rel, ei):
    """The rows outputs="query" returns, cut out of an outputs="all" result: the query nodes, the columns into them in order."""
    cols = torch.isin(ei[1], torch.arange(G, device=ei.device) * (K + 1))
    return ab[::K + 1], rel[cols], ei[:, cols]


def test_modes_and_streams_agree(dev, data, setup):
    """The masks are the same whatever cuts the work, so "query" against the same rows of "all" and one stream against two differ
    as differently tiled GEMMs do.  On the torch-mask path of the same model the same comparisons differ at order 1 (a seeded
    generator draws over other shapes): asserted too, so that the first half cannot pass vacuously."""
    m, fmap = setup
    q, nb = data["queries"][:G].to(dev), data["nb"][:G].contiguous().to(dev)
    res = {(o, s): [t.clone() for t in _forward_map(m, fmap, q, nb, o, s)] for o in ("all", "query") for s in (1, 2)}
    spread = {}
    for s in (1, 2):
        ab_q, rel_q, ei_q = _query_rows(*res[("all", s)])
        assert torch.equal(ei_q, res[("query", s)][2])
        assert rel_err(res[("query", s)][0], ab_q) < TOL and rel_err(res[("query", s)][1], rel_q) < TOL
    for o in ("all", "query"):
        assert rel_err(res[(o, 2)][0], res[(o, 1)][0]) < TOL and rel_err(res[(o, 2)][1], res[(o, 1)][1]) < TOL
    # the variances as well (the same samples up to the GEMMs' rounding)
    for s in (1, 2):
        _forward_map(m, fmap, q, nb, "all", s)
        spread[s] = m.mc_dropout.last
    assert rel_err(spread[2].rel_var, spread[1].rel_var) < 1e-3

    plain = _small(dev)                               # the same weights, torch-drawn masks

    def seeded(outputs, streams):
        plain.hip_streams = streams
        torch.manual_seed(1234)
        out = [t.clone() for t in plain.forward_map(q, nb, fmap, outputs=outputs)]
        torch.cuda.synchronize()
        return out
    assert rel_err(seeded("all", 2)[1], seeded("all", 1)[1]) > 1e-2
    assert rel_err(seeded("query", 1)[1], _query_rows(*seeded("all", 1))[1]) > 1e-2


def test_consecutive_calls_differ_and_reset_reproduces(dev, data, setup):
    m, fmap = setup
    q, nb = data["queries"][:G].to(dev), data["nb"][:G].contiguous().to(dev)
    first = [t.clone() for t in _forward_map(m, fmap, q, nb, "all", 2)]
    assert m.mc_dropout.draw == 1
    second = [t.clone() for t in m.forward_map(q, nb, fmap)]
    assert m.mc_dropout.draw == 2
    assert not torch.equal(second[0], first[0]) and not torch.equal(second[1], first[1])
    again = _forward_map(m, fmap, q, nb, "all", 2)
    assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])
    other = _forward_map(m, fmap, q, nb, "all", 2, draw=1)
    assert torch.equal(other[0], second[0]) and torch.equal(other[1], second[1])


def test_forward_takes_the_same_branch(dev, data, setup):
    """``forward`` on the assembled images (the reference's call) returns the sample means too: its node ids are the data.x rows,
    so the fully connected batch gives what forward_map gives, up to the encoder's batching, and .last has the outputs' shapes."""
    from relpose_gnn_amd.graph import fc_batch
    m, fmap = setup
    q, nb = data["queries"][:G], data["nb"][:G]
    imgs = torch.cat([torch.cat([q[g:g + 1].reshape(1, -1), data["mimgs"][nb[g]].reshape(K, -1)]) for g in range(G)])
    want = [t.clone() for t in _forward_map(m, fmap, q.to(dev), nb.contiguous().to(dev), "all", 2)]
    m.mc_dropout.reset(0)
    ab, rel, ei = m(fc_batch(imgs, K + 1).to(dev))
    torch.cuda.synchronize()
    assert torch.equal(ei, want[2]) and rel_err(ab, want[0]) < TOL and rel_err(rel, want[1]) < TOL
    assert m.mc_dropout.last.abs_var.shape == ab.shape and m.mc_dropout.last.rel_var.shape == rel.shape


def _result_rows(r):
    return np.concatenate([r.pred_poses, r.t_loss[:, None], r.q_loss[:, None]], 1)


def test_relocalize_does_not_depend_on_micro_batch(dev, data, setup):
    """8 queries in micro-batches of 2 (one stream each) and of 4 (two stream slots): relocalize holds one draw for the whole call
    and numbers the nodes through the stream, so the EvalResults agree at the parity bar; the next call draws anew."""
    from relpose_gnn_amd.evaluate import relocalize
    m, fmap = setup
    m.hip_streams = 2
    kw = dict(targets=data["targets"], postprocess="device")
    res = {}
    for mb in (2, 4):
        m.mc_dropout.reset(0)
        res[mb] = relocalize(m, fmap, data["queries"], data["nb"], micro_batch=mb, **kw)
        assert m.mc_dropout.draw == 1
    a, b = _result_rows(res[2]), _result_rows(res[4])
    assert np.isfinite(b).all() and np.abs(a - b).max() <= TOL * np.abs(b).max()
    for col in range(a.shape[1]):
        assert np.abs(a[:, col] - b[:, col]).max() <= TOL * np.abs(b[:, col]).max(), col
    nxt = _result_rows(relocalize(m, fmap, data["queries"], data["nb"], micro_batch=4, **kw))
    assert np.abs(nxt - b).max() > 1e-3 * np.abs(b).max()
    # the torch-mask path of the same model depends on the cut at order 1 (on one stream: two slots of two graphs would draw over
    # the very shapes, in the very order, of two micro-batches of two)
    plain = _small(dev)
    plain.hip_streams = 1
    tm = {}
    for mb in (2, 4):
        torch.manual_seed(99)
        tm[mb] = _result_rows(relocalize(plain, fmap, data["queries"], data["nb"], micro_batch=mb, **kw))
    assert np.abs(tm[2] - tm[4]).max() > 1e-2 * np.abs(tm[4]).max()


def test_evaluate_stream_does_not_depend_on_micro_batch(dev, data, setup):
    from relpose_gnn_amd.evaluate import evaluate_stream
    from relpose_gnn_amd.graph import Data, fc_edge_index
    m, _ = setup
    m.hip_streams = 2
    gen = torch.Generator().manual_seed(3)
    imgs = data["queries"].reshape(8, -1)
    graphs = [Data(x=imgs[torch.randperm(8, generator=gen)[:4]], edge_index=fc_edge_index(4), y=torch.randn(4, 6, generator=gen))
              for _ in range(6)]
    res = {}
    for mb in (2, 4):
        m.mc_dropout.reset(0)
        res[mb] = _result_rows(evaluate_stream(m, graphs, dev, micro_batch=mb))
        assert m.mc_dropout.draw == 1
    assert np.isfinite(res[4]).all() and np.abs(res[2] - res[4]).max() <= TOL * np.abs(res[4]).max()


def test_knn_graph_edges_carry_their_end_points(dev, data):
    """knn = 2: the model-built edges of a slot are numbered within the slot; with the slot's first node added they are ids of the
    batch, so one stream and two give the same masks for the same edge."""
    from relpose_gnn_amd.graph import fc_batch
    from relpose_gnn_amd.mc_dropout import McDropout
    m = _small(dev, knn=2)
    m.mc_dropout = McDropout(samples=S, seed=SEED)
    imgs = torch.cat([data["queries"], data["mimgs"][:8]]).reshape(16, -1)
    batch = fc_batch(imgs, 4).to(dev)
    out = {}
    for streams in (1, 2):
        m.hip_streams = streams
        m.mc_dropout.reset(0)
        out[streams] = [t.clone() for t in m(batch)]
        torch.cuda.synchronize()
        assert m.mc_dropout.last.rel_var.shape == out[streams][1].shape
    assert torch.equal(out[1][2], out[2][2])
    assert rel_err(out[2][0], out[1][0]) < TOL and rel_err(out[2][1], out[1][1]) < TOL


def test_refusals(dev, data, setup):
    from relpose_gnn_amd.mc_dropout import McDropout
    _, fmap = setup
    q, nb = data["queries"][:G].to(dev), data["nb"][:G].contiguous().to(dev)
    m0 = _small(dev, droprate=0.0)
    m0.mc_dropout = McDropout()
    with pytest.raises(ValueError, match="droprate > 0"):
        m0.forward_map(q, nb, fmap)
    m0.mc_dropout = None
    ab, _, _ = m0.forward_map(q, nb, fmap)
    assert torch.isfinite(ab).all()
    pair = _small(dev, use_AP=False)
    pair.mc_dropout = McDropout()
    from relpose_gnn_amd.graph import fc_batch
    with pytest.raises(NotImplementedError, match="use_AP=False"):
        pair(fc_batch(data["queries"][:4].reshape(4, -1), 4).to(dev))
