"""The kNN map step at fixed positions on the GPU: ``ops.knn_graph_uniform`` (rpg_knn_graph_uniform_f32) against the general kernel
(``ops.knn_graph``) and the exact oracle (``graph_sweep_ref.knn_graph_exact`` through tests/knn_map_ref.py), then ``forward_map`` /
``GraphedForwardMap`` / ``relocalize`` of a ``knn = 4`` model with ``static_knn`` against the same model without it -- the general,
waiting path, which is the behaviour before this attribute existed.

Bars.  Edge lists: ``torch.equal``.  Poses: bit-identical where the two runs issue the same GNN launches on the same edge list (one
stream slot; the one-stream tail), else the bars of tests/test_hip_query_outputs.py between two tilings of one forward (1e-4 fp32,
5e-2 bf16 Linears).  Capture against eager, a poisoned pool against a clean one: bit for bit.  Monte-Carlo samples of the two output
modes: 1e-4 (tests/test_hip_mc_model.py).  relocalize: ``_agree_results`` of tests/test_hip_query_outputs.py.

Non-finite rows: ``knn_graph_exact`` is defined on integer features only, so the statement for the counter there is the general
kernel's own in-degrees (a node is irregular exactly when ``ops.knn_graph`` gives it other than k' edges).

Small model: 64 x 64 images, planes (8, 16, 32, 64), D = 64, a 12-row map with poses."""
import numpy as np
import pytest
import torch

import graph_sweep_ref as R
import knn_map_ref as KR
from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL_FP32 = 1e-4                  # tests/test_hip_query_outputs.py: TOL_FP32_ORACLE between the two modes of forward_map
TOL_BF16 = 5e-2                  # tests/test_hip_featmap.py::test_forward_map_bf16
TOL_MC = 1e-4                    # tests/test_hip_mc_model.py

H = W = 64
M, G, MB, KNN = 12, 10, 4, 4
PM, PS = (1.5, -0.25, 3.0), (2.0, 0.5, 1.25)
SENTINEL = -7777


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


# ----------------------------------------------------------------------------------------------------------------------
# 1. the kernel
# ----------------------------------------------------------------------------------------------------------------------
N_PER = [2, 3, 5, 6, 8, 9, 65]           # 65: past the 64 nodes up to which one workgroup holds a graph's distance matrix
KS = [1, 4, 7, 64]                        # k' = n_per - 1 and k' < n_per - 1
GS = [1, 2, 5, 33]


def _uniform(dev, x, g, n_per, k, node_offset=0):
    """-> (list [2, E] host, q list [2, g k'] host, counter): outputs pre-filled with a sentinel and padded by one column on
    either side, which must come back untouched."""
    from relpose_gnn_amd import ops
    kp = min(k, n_per - 1)
    e, q = g * n_per * kp, g * kp
    buf = torch.full((2, e + 2), SENTINEL, dtype=torch.int64, device=dev)
    qbuf = torch.full((2, q + 2), SENTINEL, dtype=torch.int64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.knn_graph_uniform(x, g, n_per, k, node_offset, out=(buf[0, 1:e + 1], buf[1, 1:e + 1]),
                          q_out=(qbuf[0, 1:q + 1], qbuf[1, 1:q + 1]), irregular=cnt)
    torch.cuda.synchronize()
    buf, qbuf = buf.cpu(), qbuf.cpu()
    assert bool((buf[:, 0] == SENTINEL).all()) and bool((buf[:, -1] == SENTINEL).all())
    assert bool((qbuf[:, 0] == SENTINEL).all()) and bool((qbuf[:, -1] == SENTINEL).all())
    ei, qe = buf[:, 1:-1], qbuf[:, 1:-1]
    assert not bool((ei == SENTINEL).any()) and not bool((qe == SENTINEL).any())          # every column written
    lo = node_offset + (torch.arange(g * n_per) // n_per * n_per).repeat_interleave(kp)    # first node of the column's graph
    assert bool((ei[0] >= lo).all()) and bool((ei[0] < lo + n_per).all()) and bool((ei[0] != ei[1]).all())
    assert torch.equal(ei[1], torch.arange(g * n_per).repeat_interleave(kp) + node_offset)
    assert torch.equal(qe, ei[:, KR.query_columns(g, n_per, k)])
    return ei, qe, int(cnt.item())


@pytest.mark.parametrize("d", [64, 2048])
@pytest.mark.parametrize("n_per", N_PER)
def test_uniform_knn_equals_the_general_kernel_on_random_features(dev, n_per, d):
    from relpose_gnn_amd import ops
    for g in GS:
        x = torch.randn(g * n_per, d, generator=torch.Generator().manual_seed(100 * n_per + g)).to(dev)
        batch = KR.uniform_batch(g, n_per).to(dev)
        for k in KS:
            want = ops.knn_graph(x, k, batch).cpu()
            ei, _, irregular = _uniform(dev, x, g, n_per, k)
            assert irregular == 0 and torch.equal(ei, want), (g, n_per, k, d)
    # node_offset: ids of a slot inside a larger batch
    ei_off, _, _ = _uniform(dev, x, g, n_per, 4, node_offset=1000)
    assert torch.equal(ei_off, ops.knn_graph(x, 4, batch).cpu() + 1000)


@pytest.mark.parametrize("d", [64, 2048])
@pytest.mark.parametrize("n_per", N_PER)
def test_uniform_knn_equals_the_exact_oracle_on_ties_and_duplicates(dev, n_per, d):
    from relpose_gnn_amd import ops
    for g in GS:
        x = KR.planted_ties(g, n_per, d, seed=7 * n_per + g)
        for k in KS:
            ei, _, irregular = _uniform(dev, x.to(dev), g, n_per, k)
            assert irregular == KR.irregular_nodes(x, g, n_per, k), (g, n_per, k, d)
            assert torch.equal(ei, KR.uniform_knn(x, g, n_per, k)), (g, n_per, k, d)
            if irregular == 0:
                assert torch.equal(ei, ops.knn_graph(x.to(dev), k, KR.uniform_batch(g, n_per).to(dev)).cpu())


@pytest.mark.parametrize("d", [8, 2048])
def test_uniform_knn_counts_the_duplicate_row_example(dev, d):
    """Rows 1..6 identical, k = 4: in-degrees [4, 4, 4, 4, 4, 4, 5, 4] in the reference, one irregular node; a batch that holds the
    graph twice counts two; with many copies (all rows equal) every node from k + 1 on is irregular."""
    x = KR.duplicate_rows_example(d)
    assert KR.reference_in_degrees(x, 1, 8, 4).tolist() == [4, 4, 4, 4, 4, 4, 5, 4]
    ei, _, irregular = _uniform(dev, x.to(dev), 1, 8, 4)
    assert irregular == 1 and torch.equal(ei, KR.uniform_knn(x, 1, 8, 4))
    x3 = torch.cat([x, R.integer_features(8, d, seed=9), x])
    ei, _, irregular = _uniform(dev, x3.to(dev), 3, 8, 4)
    assert irregular == 2 == KR.irregular_nodes(x3, 3, 8, 4) and torch.equal(ei, KR.uniform_knn(x3, 3, 8, 4))
    same = x[1:2].repeat(70, 1)
    for n_per in (10, 70):
        xs = same[:n_per]
        ei, _, irregular = _uniform(dev, xs.to(dev), 1, n_per, 4)
        assert irregular == n_per - 5 == KR.irregular_nodes(xs, 1, n_per, 4) and torch.equal(ei, KR.uniform_knn(xs, 1, n_per, 4))


@pytest.mark.parametrize("n_per", [8, 65])
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_uniform_knn_non_finite_rows(dev, n_per, bad):
    """Nothing out of range (``_uniform`` checks every source id), the counter is the number of nodes the general kernel gives
    other than k' edges, and every regular node's list is the general kernel's."""
    from relpose_gnn_amd import ops
    g, d, k = 3, 64, 4
    x = torch.randn(g * n_per, d, generator=torch.Generator().manual_seed(5))
    x[1] = bad                                    # a whole row
    x[n_per + 3, 5] = bad                         # one element
    x[2 * n_per + 2] = bad
    x[2 * n_per + 6] = bad                        # two such rows in one graph
    ref_ei, ref_irregular = KR.insertion_knn(x, g, n_per, k)          # the documented rule, restated on the host
    x = x.to(dev)
    ei, _, irregular = _uniform(dev, x, g, n_per, k)
    assert irregular == ref_irregular and torch.equal(ei, ref_ei)
    assert ref_irregular > 0                                          # ... or the rows planted above show nothing
    want = ops.knn_graph(x, k, KR.uniform_batch(g, n_per).to(dev)).cpu()
    deg = torch.bincount(want[1], minlength=g * n_per)
    assert irregular == int((deg != k).sum())
    first = torch.cumsum(deg, 0) - deg
    cols = (first[:, None] + torch.arange(k)[None, :]).reshape(-1)
    assert torch.equal(ei, want[:, cols])


# ----------------------------------------------------------------------------------------------------------------------
# 2. forward_map: static_knn against the general path
# ----------------------------------------------------------------------------------------------------------------------
def _small(dev, precision="f32", mc=False, **kw):
    import relpose_gnn_amd.synth as S
    from relpose_gnn_amd.mc_dropout import McDropout
    from relpose_gnn_amd.posenet import PoseNetX_R2
    from relpose_gnn_amd.resnet import ResNet
    planes, blocks = (8, 16, 32, 64), (1, 1, 1, 1)
    args = dict(droprate=0.5 if mc else 0.0, knn=KNN, use_AP=True, gnn_recursion=2, use_attention=False, L=1)
    args.update(kw)
    m = PoseNetX_R2(ResNet(blocks, planes), pretrained=False, feat_dim=64, edge_feat_dim=64, node_dim=64, input_img_height=H,
                    use_gnn=True, **args)
    m.load_state_dict(S.synth_state_dict(S.posenet_r2_param_shapes(64, 64, 64, planes, blocks), seed=1))
    m = m.to(dev).eval()
    m.encoder_dtype = m.gnn_dtype = precision
    if mc:
        m.mc_dropout = McDropout(samples=8, seed=2026)
    return m


@pytest.fixture(scope="module")
def data():
    import relpose_gnn_amd.synth as S
    gen = torch.Generator().manual_seed(6)
    # every query's map rows are distinct (a permutation's head): duplicated rows are section 5's business
    nb = torch.stack([torch.randperm(M, generator=torch.Generator().manual_seed(100 + i))[:7] for i in range(99)])
    return dict(mimgs=S.synth_images(M, H, W, seed=91), queries=S.synth_images(99, H, W, seed=92),
                poses=torch.randn(M, 6, generator=gen) * 0.3, targets=torch.randn(99, 6, generator=gen) * 0.3, nb=nb)


@pytest.fixture(scope="module")
def models(dev, data):
    """One knn = 4 model and map per precision, shared by the tests that change neither the weights nor the flags for good."""
    from relpose_gnn_amd.featmap import FeatureMap
    out = {}
    for precision in ("f32", "bf16"):
        m = _small(dev, precision)
        out[precision] = (m, FeatureMap.build(m, data["mimgs"], poses=data["poses"]))
    return out


def _general(m, *a, **kw):
    """forward_map through the general kNN build: the path before static_knn existed."""
    m.static_knn = False
    try:
        out = m.forward_map(*a, **kw)
        m.check_edge_index()
        return out
    finally:
        m.static_knn = True


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("k", [1, 3, 7])
@pytest.mark.parametrize("g", [1, 4, 33])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_forward_map_static_equals_general(dev, data, models, precision, g, k, streams):
    """The same edge list in both modes.  The ``"all"`` poses are bit-identical, because the two runs issue the same GNN launches:
    in fp32 the general path cuts the batch into the same stream slots, and in bf16 the static step keeps the general path's one
    stream at these sizes (slots of fewer than 32 graphs; two bf16 slots: the next test).  The query mode prunes the last
    recursion, so its rows are held to the bars between two tilings of one forward (1e-4 fp32, 5e-2 bf16 Linears)."""
    m, fmap = models[precision]
    tol = TOL_FP32 if precision == "f32" else TOL_BF16
    kp = min(KNN, k)
    q, nb = data["queries"][:g].to(dev), data["nb"][:g, :k].contiguous().to(dev)
    m.hip_streams = streams
    try:
        ab, rel, ei = _general(m, q, nb, fmap)
        m.static_knn = True
        ab_s, rel_s, ei_s = m.forward_map(q, nb, fmap)
        ab_q, rel_q, ei_q = m.forward_map(q, nb, fmap, outputs="query")
        m.check_edge_index()
    finally:
        m.hip_streams, m.static_knn = 2, False
    assert ei_s.shape == (2, g * (k + 1) * kp) and torch.equal(ei_s, ei)
    assert bool(torch.isfinite(rel).all()) and (g * k == 1 or float(rel.std(0).min()) > 0) and (g == 1 or float(ab[::k + 1].std(0).min()) > 0)
    assert torch.equal(ab_s, ab) and torch.equal(rel_s, rel)
    qn = torch.arange(g) * (k + 1)
    cols = KR.query_columns(g, k + 1, KNN).to(dev)
    assert torch.equal(cols.cpu(), torch.nonzero((ei[1].cpu() % (k + 1)) == 0).flatten())       # the general list's columns into the queries
    assert ab_q.shape == (g, 6) and rel_q.shape == (g * kp, 6) and torch.equal(ei_q, ei[:, cols])
    ea, er = rel_err(ab_q, ab[qn.to(dev)]), rel_err(rel_q, rel[cols])
    print(f"static query vs general {precision} G={g} K={k} streams={streams}: abs {ea:.3e} rel {er:.3e}")
    assert ea < tol and er < tol, (ea, er)


@pytest.mark.parametrize("g", [64, 71])
def test_forward_map_static_bf16_on_two_slots(dev, data, models, g):
    """From 32 graphs per slot on, the static step cuts a bf16 batch into stream slots, which the general path never does for the
    bf16 GNN: the same edge list, and poses at the bar between two tilings of one forward (5e-2; the figure is printed).  71 is two
    uneven slots; 63 graphs stay on one stream."""
    from relpose_gnn_amd import posenet
    m, fmap = models["bf16"]
    k = 3
    q, nb = data["queries"][:g].to(dev), data["nb"][:g, :k].contiguous().to(dev)
    ab, rel, ei = _general(m, q, nb, fmap)
    forked = []
    fork = m._fork
    m._fork = lambda n, d: forked.append(n) or fork(n, d)
    try:
        ab_s, rel_s, ei_s = m.forward_map(q, nb, fmap)
        ab_q, rel_q, ei_q = m.forward_map(q, nb, fmap, outputs="query")
        m.check_edge_index()
        assert forked == [2, 2] and posenet._STATIC_BF16_SLOT_GRAPHS == 32
        del forked[:]
        m.forward_map(q[:63], nb[:63], fmap)
        m.check_edge_index()
        assert forked == []                                   # one stream: the tail, which forks nothing for 63 images
    finally:
        m.__dict__.pop("_fork", None)
        m.static_knn = False
    cols = KR.query_columns(g, k + 1, KNN).to(dev)
    assert torch.equal(ei_s, ei) and torch.equal(ei_q, ei[:, cols])
    figures = {"abs": rel_err(ab_s, ab), "rel": rel_err(rel_s, rel), "abs_q": rel_err(ab_q, ab[::k + 1]), "rel_q": rel_err(rel_q, rel[cols])}
    print(f"static bf16 two slots vs general one stream G={g}: {figures}")
    assert all(v < TOL_BF16 for v in figures.values()), figures


def test_static_knn_unset_is_ignored_and_refused_as_before(dev, data, models):
    m, fmap = models["f32"]
    q, nb = data["queries"][:4].to(dev), data["nb"][:4, :3].contiguous().to(dev)
    assert m.static_knn is False and "static_knn" not in m.state_dict()
    with pytest.raises(NotImplementedError, match="knn"):
        m.forward_map(q, nb, fmap, outputs="query")
    from relpose_gnn_amd.graphed import GraphedForwardMap
    with pytest.raises(NotImplementedError, match="graph capture covers the deterministic fully-connected path"):
        GraphedForwardMap(m, fmap, q, 3)


# ----------------------------------------------------------------------------------------------------------------------
# 3. capture
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mc", [False, True], ids=["plain", "mc"])
@pytest.mark.parametrize("outputs", ["all", "query"])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_replays_rebuild_the_knn_edges(dev, data, precision, outputs, mc):
    """A step captured on one query set, replayed on two others whose nearest neighbours differ: each replay is the eager static
    step of its inputs, bit for bit, edge list included."""
    from relpose_gnn_amd.featmap import FeatureMap
    from relpose_gnn_amd.graphed import GraphedForwardMap
    m = _small(dev, precision, mc=mc)
    m.static_knn = True
    fmap = FeatureMap.build(m, data["mimgs"], poses=data["poses"])
    g, k = 4, 7
    sets = [(data["queries"][i * g:(i + 1) * g].to(dev), data["nb"][i * g:(i + 1) * g, :k].contiguous().to(dev)) for i in range(3)]
    if mc:
        m.mc_dropout.reset(0)
    step = GraphedForwardMap(m, fmap, sets[0][0], k, outputs=outputs)
    assert step.irregular is not None
    want = []
    for i, (q, nb) in enumerate(sets[1:]):
        if mc:
            m.mc_dropout.reset(i)
        want.append([t.clone() for t in m.forward_map(q, nb, fmap, outputs=outputs)])
    m.check_edge_index()
    captured = [t.clone() for t in m.forward_map(*sets[0], fmap, outputs=outputs)]
    if mc:
        m.mc_dropout.reset(0)
    for i, (q, nb) in enumerate(sets[1:]):
        out = step(q, nb)
        got = [out.abs_pose, out.rel_pose, out.edge_index]
        assert all(torch.equal(a, b) for a, b in zip(got, want[i])), i
        assert int(step.irregular.item()) == 0
    assert not torch.equal(want[0][2], captured[2]) and not torch.equal(want[1][2], captured[2])     # ... or this shows nothing
    assert not torch.equal(want[0][2], want[1][2]) and not torch.equal(want[0][1], want[1][1])
    m.check_edge_index()


# ----------------------------------------------------------------------------------------------------------------------
# 4. relocalize
# ----------------------------------------------------------------------------------------------------------------------
def _agree_results(a, b):
    """tests/test_hip_query_outputs.py::_agree_results."""
    got = np.concatenate([a.pred_poses, a.targ_poses, a.t_loss[:, None], a.q_loss[:, None]], 1)
    want = np.concatenate([b.pred_poses, b.targ_poses, b.t_loss[:, None], b.q_loss[:, None]], 1)
    assert got.shape == want.shape and np.isfinite(want).all()
    err = np.abs(got - want)
    assert (err[:, :15] <= 1e-12 + 1e-12 * np.abs(want[:, :15])).all(), err[:, :15].max()
    assert (err[:, 15] <= 1e-5 + 1e-9 * np.abs(want[:, 15])).all(), err[:, 15].max()


@pytest.fixture(scope="module")
def general_results(dev, data, models):
    """relocalize through the general path (static_knn off, outputs="all", uncaptured), once per (postprocess, fuse)."""
    from relpose_gnn_amd.evaluate import relocalize
    m, fmap = models["f32"]
    q, nb = data["queries"][:G], data["nb"][:G, :7].contiguous()
    out = {}
    for postprocess in ("host", "device"):
        for fuse in (None, "mean"):
            out[(postprocess, fuse)] = relocalize(m, fmap, q, nb, micro_batch=MB, pose_m=PM, pose_s=PS, targets=data["targets"][:G],
                                                  postprocess=postprocess, fuse=fuse)
    return out


@pytest.mark.parametrize("fuse", [None, "mean"])
@pytest.mark.parametrize("postprocess", ["host", "device"])
@pytest.mark.parametrize("capture", [False, True])
@pytest.mark.parametrize("outputs", ["all", "query"])
def test_relocalize_static_agrees_with_general(dev, data, models, general_results, outputs, capture, postprocess, fuse):
    from relpose_gnn_amd.evaluate import relocalize
    m, fmap = models["f32"]
    q, nb = data["queries"][:G], data["nb"][:G, :7].contiguous()
    st = {}
    m.static_knn = True
    try:
        got = relocalize(m, fmap, q, nb, micro_batch=MB, pose_m=PM, pose_s=PS, targets=data["targets"][:G], postprocess=postprocess,
                         fuse=fuse, outputs=outputs, capture=capture, stats=st)
    finally:
        m.static_knn = False
    assert st["knn_irregular_batches"] == 0 and st["micro_batches"] == 3
    want = general_results[(postprocess, fuse)]
    et, eq = rel_err(got.pred_poses[:, :3], want.pred_poses[:, :3]), rel_err(got.pred_poses[:, 3:], want.pred_poses[:, 3:])
    print(f"relocalize static {outputs} capture={capture} {postprocess} fuse={fuse} vs general: t {et:.3e} q {eq:.3e}")
    _agree_results(got, want)
    assert np.array_equal(got.neighbours, nb.numpy())


def test_relocalize_refuses_a_reference_edge_the_knn_list_does_not_have(dev, data, models):
    from relpose_gnn_amd.evaluate import relocalize
    m, fmap = models["f32"]
    m.static_knn = True
    try:
        with pytest.raises(ValueError, match="ref_node"):
            relocalize(m, fmap, data["queries"][:G], data["nb"][:G, :7].contiguous(), micro_batch=MB, ref_node=KNN)
    finally:
        m.static_knn = False


# ----------------------------------------------------------------------------------------------------------------------
# 5. irregular graphs
# ----------------------------------------------------------------------------------------------------------------------
def _irregular_neighbours(data, g=G, at=5):
    """Query ``at`` names one map row six times (K = 7, knn = 4): its nodes 1..6 are identical, node 6 keeps five edges."""
    nb = data["nb"][:g, :7].clone()
    nb[at, :6] = nb[at, 0]
    return nb.contiguous()


def test_forward_map_raises_for_an_irregular_graph(dev, data, models):
    from relpose_gnn_amd.posenet import IrregularKnnGraph
    m, fmap = models["f32"]
    q, nb = data["queries"][:G].to(dev), _irregular_neighbours(data).to(dev)
    ab, rel, ei = _general(m, q, nb, fmap)
    assert ei.shape[1] == G * 8 * KNN + 1                      # the reference's extra edge
    m.static_knn = True
    try:
        for outputs in ("all", "query"):
            m.index_check = "sync"
            with pytest.raises(IrregularKnnGraph, match="static_knn = False"):
                m.forward_map(q, nb, fmap, outputs=outputs)
            m.index_check = "deferred"
            out = m.forward_map(q, nb, fmap, outputs=outputs)  # a valid graph's outputs, reported at the next look
            assert bool(torch.isfinite(out[1]).all()) and int(out[2].max()) < G * 8 and int(out[2].min()) >= 0
            with pytest.raises(IrregularKnnGraph):
                m.check_edge_index()
            m.check_edge_index()                               # reported once
        assert issubclass(IrregularKnnGraph, ValueError)
        m.forward_map(q, data["nb"][:G, :7].contiguous().to(dev), fmap)
        m.check_edge_index()                                   # a regular call reports nothing
    finally:
        m.index_check, m.static_knn = "deferred", False


@pytest.mark.parametrize("fuse", [None, "mean"])
@pytest.mark.parametrize("postprocess", ["host", "device"])
@pytest.mark.parametrize("capture", [False, True])
@pytest.mark.parametrize("outputs", ["all", "query"])
def test_relocalize_runs_an_irregular_micro_batch_again(dev, data, models, outputs, capture, postprocess, fuse):
    """The micro-batch of the irregular query is run again through the general path: the general path's rows for EVERY query
    (``_agree_results`` over all of them), and the re-run micro-batch's bit for bit."""
    from relpose_gnn_amd.evaluate import relocalize
    m, fmap = models["f32"]
    q, nb = data["queries"][:G], _irregular_neighbours(data)
    kw = dict(micro_batch=MB, pose_m=PM, pose_s=PS, targets=data["targets"][:G], postprocess=postprocess, fuse=fuse)
    want = relocalize(m, fmap, q, nb, **kw)
    st = {}
    m.static_knn = True
    try:
        got = relocalize(m, fmap, q, nb, outputs=outputs, capture=capture, stats=st, **kw)
    finally:
        m.static_knn = False
    assert st["knn_irregular_batches"] == 1
    _agree_results(got, want)
    again = slice(MB, 2 * MB)                                  # query 5 is in the second micro-batch
    for f in ("pred_poses", "targ_poses", "t_loss", "q_loss"):
        assert np.array_equal(getattr(got, f)[again], getattr(want, f)[again]), f
    m.check_edge_index()


@pytest.mark.parametrize("weights", [None, "variance"])
@pytest.mark.parametrize("postprocess", ["host", "device"])
@pytest.mark.parametrize("capture", [False, True])
def test_relocalize_runs_an_irregular_micro_batch_again_with_mc_dropout(dev, data, capture, postprocess, weights):
    """The same with ``mc_dropout`` (the re-run places the sampler at the micro-batch's first node and, for a weighted rule, reads
    the variances of its own forward): masks follow node ids, so every query's rows are the general path's."""
    from relpose_gnn_amd.evaluate import relocalize
    from relpose_gnn_amd.featmap import FeatureMap
    m = _small(dev, mc=True)
    fmap = FeatureMap.build(m, data["mimgs"], poses=data["poses"])
    q, nb = data["queries"][:G], _irregular_neighbours(data)
    kw = dict(micro_batch=MB, pose_m=PM, pose_s=PS, targets=data["targets"][:G], postprocess=postprocess, fuse="mean", weights=weights)
    m.mc_dropout.reset(0)
    want = relocalize(m, fmap, q, nb, **kw)
    st = {}
    m.static_knn = True
    m.mc_dropout.reset(0)
    got = relocalize(m, fmap, q, nb, outputs="query", capture=capture, stats=st, **kw)
    assert st["knn_irregular_batches"] == 1 and m.mc_dropout.draw == 1
    _agree_results(got, want)
    if weights is not None:
        assert np.allclose(got.sigma_t, want.sigma_t, rtol=1e-9, atol=0) and np.allclose(got.sigma_q, want.sigma_q, rtol=1e-9, atol=0)
    m.check_edge_index()


def test_captured_step_reports_an_irregular_graph_and_stays_usable(dev, data, models):
    from relpose_gnn_amd.graphed import GraphedForwardMap
    m, fmap = models["f32"]
    m.static_knn = True
    try:
        q = data["queries"][4:8].to(dev)
        good, bad = data["nb"][4:8, :7].contiguous().to(dev), _irregular_neighbours(data)[4:8].contiguous().to(dev)
        step = GraphedForwardMap(m, fmap, q, 7, outputs="query")
        want = [t.clone() for t in m.forward_map(q, good, fmap, outputs="query")]
        step(q, bad)
        assert int(step.irregular.item()) == 1
        m.check_edge_index()                                   # the step's own counter, not the model's: nothing raises
        out = step(q, good)
        assert int(step.irregular.item()) == 0
        assert all(torch.equal(a, b) for a, b in zip((out.abs_pose, out.rel_pose, out.edge_index), want))
    finally:
        m.static_knn = False


# ----------------------------------------------------------------------------------------------------------------------
# 6. mc_dropout: both output modes draw the same masks
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("streams", [1, 2])
def test_mc_samples_of_the_query_mode_are_the_all_modes(dev, data, streams):
    from relpose_gnn_amd.featmap import FeatureMap
    m = _small(dev, mc=True)
    m.static_knn = True
    m.hip_streams = streams
    fmap = FeatureMap.build(m, data["mimgs"], poses=data["poses"])
    g, k = 6, 7
    q, nb = data["queries"][:g].to(dev), data["nb"][:g, :k].contiguous().to(dev)
    m.mc_dropout.reset(0)
    ab, rel, ei = m.forward_map(q, nb, fmap)
    var = m.mc_dropout.last
    m.mc_dropout.reset(0)
    ab_q, rel_q, ei_q = m.forward_map(q, nb, fmap, outputs="query")
    var_q = m.mc_dropout.last
    m.check_edge_index()
    qn, cols = (torch.arange(g) * (k + 1)).to(dev), KR.query_columns(g, k + 1, KNN).to(dev)
    assert torch.equal(ei_q, ei[:, cols])
    for name, a, b in (("abs", ab_q, ab[qn]), ("rel", rel_q, rel[cols]), ("abs_var", var_q.abs_var, var.abs_var[qn]),
                       ("rel_var", var_q.rel_var, var.rel_var[cols])):
        e = rel_err(a, b)
        print(f"mc query vs all streams={streams} {name}: {e:.3e}")
        assert e < TOL_MC, (name, e)
    # ... and the general path's, whose rows carry the same node ids
    m.static_knn = False
    m.mc_dropout.reset(0)
    ab_g, rel_g, ei_g = m.forward_map(q, nb, fmap)
    m.check_edge_index()
    assert torch.equal(ei_g, ei) and torch.equal(ab_g, ab) and torch.equal(rel_g, rel)


# ----------------------------------------------------------------------------------------------------------------------
# 7. workspace independence
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("outputs", ["all", "query"])
def test_poisoned_pool_gives_the_same_bits(dev, data, models, outputs):
    m, fmap = models["f32"]
    q, nb = data["queries"][:6].to(dev), data["nb"][:6, :7].contiguous().to(dev)
    m.static_knn = True
    try:
        want = [t.clone() for t in m.forward_map(q, nb, fmap, outputs=outputs)]
        torch.cuda.synchronize()
        for buf in m._ws_pool._buf.values():
            buf.view(torch.uint8).fill_(0xFF)                  # every fp32 word a NaN, every index -1
        got = m.forward_map(q, nb, fmap, outputs=outputs)
        m.check_edge_index()
        assert all(torch.equal(a, b) and bool(torch.isfinite(a.float()).all()) for a, b in zip(got, want))
    finally:
        m.static_knn = False
