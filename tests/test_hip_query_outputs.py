"""The query-only output mode on the GPU: ``ops.gnn_forward_query`` (rpg_gnn_forward_query_f32 / _bf16) on irregular graphs against
the oracle restricted to the same rows, its selection check, and ``forward_map`` / ``relocalize`` / ``GraphedForwardMap`` with
``outputs="query"`` against ``outputs="all"``.

The mode is dead-code elimination: what it still computes is what the full forward computes at the same row, up to the summation
order of differently tiled GEMMs.  So the bars are the full forward's own: on the irregular batch the rule and constants of
tests/test_hip_graph_sweep.py (rel_err < 1e-4 against the fp32 oracle, and no further from the float64 oracle than M_FWD = 2 x the
fp32 oracle is), 5e-2 for the bf16 Linears (tests/test_hip_featmap.py::test_forward_map_bf16), 1e-4 / 5e-2 between the two modes of
forward_map, bit-identity wherever two runs issue the same launches (capture against eager, the host rule against forward_map on the
same cut, a poisoned workspace against a clean one, dropout under one seed), and between the device and the host pose rule the bar
of tests/test_hip_query_pose.py.

Small model: 64 x 64 images, planes (8, 16, 32, 64), D = 64, a 12-row map with poses (tests/test_hip_relocalize_capture.py)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import graph_sweep_ref as R
from conftest import rel_err

pytestmark = pytest.mark.gpu

M_FWD = 2.0                      # tests/test_hip_graph_sweep.py
TOL_FP32_ORACLE = 1e-4
TOL_BF16 = 5e-2                  # tests/test_hip_featmap.py::test_forward_map_bf16

H = W = 64
M, K, G, MB = 12, 3, 10, 4
PM, PS = (1.5, -0.25, 3.0), (2.0, 0.5, 1.25)
RESULT_FIELDS = ("pred_poses", "targ_poses", "t_loss", "q_loss", "neighbours")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _record(section: str, case: str, figures: dict) -> None:
    """As tests/test_hip_graph_sweep.py: printed, and appended to the file RPG_SWEEP_RECORD names."""
    path = os.environ.get("RPG_SWEEP_RECORD")
    print(section, case, figures)
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"section": section, "case": case, **figures}) + "\n")


# ----------------------------------------------------------------------------------------------------------------------
# 1. the composite on irregular graphs
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def irr(dev):
    """The five-graph irregular batch of the composite sweep (3, 8, 12, 1 and 9 nodes), its HIP encoder features, the packed GNN
    weights, and the three query sets."""
    from relpose_gnn_amd.graph import query_edge_columns
    from relpose_gnn_amd.posenet import PoseNetX_R2
    from relpose_gnn_amd.resnet import ResNet
    m = PoseNetX_R2(ResNet(R.FWD_BLOCKS, R.FWD_PLANES), droprate=0.0, pretrained=False, feat_dim=R.FWD_D, edge_feat_dim=R.FWD_D,
                    node_dim=R.FWD_D, input_img_height=R.FWD_H, use_gnn=True, knn=-1, use_AP=True, gnn_recursion=2)
    sd = R.forward_state_dict()
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    x, local, ei, batch = R.forward_batch()
    n = x.shape[0]
    feat = m.encode(x.to(dev))
    m.gnn_dtype = "bf16"
    m._pack_gnn()
    offs = [sum(R.FORWARD_SIZES[:i]) for i in range(len(R.FORWARD_SIZES))]
    deg = R.in_degrees(ei, n)
    largest = [o + int(deg[o:o + s].argmax()) for o, s in zip(offs, R.FORWARD_SIZES)]
    assert sorted(int(deg[v]) for v in largest)[-2:] == [9, 11] and int(deg[offs[3]]) == 0
    sets = {"first": offs, "largest": largest, "all": list(range(n))}
    sel = {name: query_edge_columns(ei, q) for name, q in sets.items()}
    assert sel["all"].tolist() == list(range(ei.shape[1]))
    return {"sd": sd, "x": x, "ei": ei, "feat": feat, "packed": m._gnn_packed, "bf16": m._gnn_bf16, "sets": sets, "sel": sel,
            "model": m, "oracle": {}}


def _oracle(irr, recursion):
    """(abs, rel) of the fp32 and of the float64 oracle for ``recursion`` recursions, computed once (oracle_forward's own cast)."""
    if recursion not in irr["oracle"]:
        from oracle import posenet_ref as O
        out = []
        for dtype in (torch.float32, torch.float64):
            if recursion == 2:
                a, r, _ = R.oracle_forward(irr["sd"], irr["x"], irr["ei"], dtype)
            else:
                sd = {k: (v.to(dtype) if torch.is_floating_point(v) else v) for k, v in irr["sd"].items()}
                a, r, _ = O.posenet_forward(sd, irr["x"].to(dtype), irr["ei"], R.FWD_H, recursion)
            out.append((a, r))
        irr["oracle"][recursion] = out
    return irr["oracle"][recursion]


def _run_query(dev, irr, qset, recursion, bf16=False, **kw):
    from relpose_gnn_amd import ops
    q = torch.tensor(irr["sets"][qset], dtype=torch.int64, device=dev)
    return ops.gnn_forward_query(irr["packed"], irr["feat"], irr["ei"].to(dev), irr["sel"][qset].to(dev), q, recursion,
                                 weights_bf16=irr["bf16"] if bf16 else None, **kw)


def _against_oracles(case, irr, qset, recursion, got):
    (a32, r32), (a64, r64) = _oracle(irr, recursion)
    q, sel = torch.tensor(irr["sets"][qset]), irr["sel"][qset]
    for name, y, y32, z in (("abs", got[0].cpu(), a32[q], a64[q]), ("rel", got[1].cpu(), r32[sel], r64[sel])):
        assert bool(torch.isfinite(y).all())
        e_ref, e_hip, e_32 = rel_err(y32, z), rel_err(y, z), rel_err(y, y32)
        _record("query_forward", f"{case} {name}_pose", {"e_ref": e_ref, "e_hip": e_hip, "ratio": e_hip / e_ref, "vs_fp32_oracle": e_32})
        assert e_hip <= M_FWD * e_ref, (case, name, e_ref, e_hip)
        assert e_32 < TOL_FP32_ORACLE, (case, name, e_32)


@pytest.mark.parametrize("recursion", [1, 2, 3])
@pytest.mark.parametrize("qset", ["first", "largest", "all"])
def test_query_forward_irregular(dev, irr, qset, recursion):
    """Query sets: the first node of every graph (the one-node graph's query has in-degree 0: its aggregate is zeros); the node of
    largest in-degree per graph (9 and 11: a second round of the aggregation's 8 waves); all nodes with every column.  One, two
    and three recursions (one: the only recursion is the pruned one)."""
    got = _run_query(dev, irr, qset, recursion)
    assert got[0].shape == (len(irr["sets"][qset]), 6) and got[1].shape == (irr["sel"][qset].numel(), 6)
    _against_oracles(f"{qset} R={recursion}", irr, qset, recursion, got)


@pytest.mark.parametrize("split,fuse_agg", [(1, 0), (0, 1), (0, 0)])
def test_query_forward_irregular_other_formulations(dev, irr, split, fuse_agg):
    """The 22-tensor formulation and the unfused aggregation, as tests/test_hip_graph_sweep.py switches them."""
    from relpose_gnn_amd import ops
    with ops.tuned({ops.TUNE_GNN_SPLIT: split, ops.TUNE_GNN_FUSE_AGG: fuse_agg}):
        for qset in ("first", "largest"):
            got = _run_query(dev, irr, qset, 2)
            torch.cuda.synchronize()
            _against_oracles(f"{qset} R=2 split={split} fuse_agg={fuse_agg}", irr, qset, 2, got)


@pytest.mark.parametrize("fuse_agg", [1, 0])
@pytest.mark.parametrize("recursion", [1, 2])
def test_query_forward_irregular_bf16_linears(dev, irr, recursion, fuse_agg):
    from relpose_gnn_amd import ops
    with ops.tuned({ops.TUNE_GNN_FUSE_AGG: fuse_agg}):
        for qset in ("first", "largest", "all"):
            got = _run_query(dev, irr, qset, recursion, bf16=True)
            torch.cuda.synchronize()
            a32, r32 = _oracle(irr, recursion)[0]
            ea = rel_err(got[0].cpu(), a32[torch.tensor(irr["sets"][qset])])
            er = rel_err(got[1].cpu(), r32[irr["sel"][qset]])
            _record("query_forward_bf16", f"{qset} R={recursion} fuse_agg={fuse_agg}", {"abs": ea, "rel": er})
            assert ea < TOL_BF16 and er < TOL_BF16, (qset, ea, er)


def test_query_rows_are_the_full_forwards_rows(dev, irr):
    """Against the full composite on the same features: the same rows within the fp32 bar (only GEMM tiling differs), and the
    heads' inputs come back on request."""
    m = irr["model"]
    m.gnn_dtype = "f32"
    try:
        from relpose_gnn_amd import _lib
        lib, n, e = _lib.lib(), irr["feat"].shape[0], irr["ei"].shape[1]
        ei = irr["ei"].to(dev)
        ab, rel = torch.empty((n, 6), device=dev), torch.empty((e, 6), device=dev)
        nf, ef = torch.empty((n, R.FWD_D), device=dev), torch.empty((e, R.FWD_D), device=dev)
        st = torch.zeros(1, dtype=torch.int32, device=dev)
        m._gnn_call(lib, irr["feat"], ei.data_ptr(), ei.data_ptr() + 8 * e, 0, n, e, ab, rel, nf, ef, st, (900, 0))
    finally:
        m.gnn_dtype = "bf16"
    a, r, node_out, edge_out = _run_query(dev, irr, "largest", 2, want_features=True)
    q, sel = torch.tensor(irr["sets"]["largest"], device=dev), irr["sel"]["largest"].to(dev)
    assert int(st.item()) == 0
    assert rel_err(a, ab[q]) < TOL_FP32_ORACLE and rel_err(r, rel[sel]) < TOL_FP32_ORACLE
    assert rel_err(node_out, nf[q]) < TOL_FP32_ORACLE and rel_err(edge_out, ef[sel]) < TOL_FP32_ORACLE
    assert bool((node_out >= 0).all()) and bool((edge_out >= 0).all())


# ----------------------------------------------------------------------------------------------------------------------
# 2. the selection check
# ----------------------------------------------------------------------------------------------------------------------
def test_selection_check_counts_and_clamps(dev, irr):
    from relpose_gnn_amd import ops
    ei, n = irr["ei"], irr["feat"].shape[0]
    e = ei.shape[1]
    qn = torch.tensor(irr["sets"]["largest"])
    sel = irr["sel"]["largest"]
    into = set(sel.tolist())
    other = next(c for c in range(e) if c not in into)

    def count(sel_t, qn_t, ei_t=ei):
        st = torch.zeros(1, dtype=torch.int32, device=dev)
        a, r = ops.gnn_forward_query(irr["packed"], irr["feat"], ei_t.to(dev), sel_t.to(dev), qn_t.to(dev), 2, status=st)
        torch.cuda.synchronize()
        assert a.shape == (qn_t.numel(), 6) and r.shape == (sel_t.numel(), 6)
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(r).all())
        return int(st.item())

    assert count(sel, qn) == 0                                                  # a valid selection
    assert count(torch.cat([sel[:5], sel[6:]]), qn) == 1                        # misses one in-edge of a query
    extra = torch.sort(torch.cat([sel, torch.tensor([other])])).values
    assert count(extra, qn) == 2                                                # a column whose target is no query (+ the count)
    swapped = sel.clone()
    swapped[[3, 4]] = sel[[4, 3]]
    assert count(swapped, qn) == 1                                              # a descending pair
    past = sel.clone()
    past[-1] = e
    assert count(past, qn) >= 1                                                 # a column >= e
    dropped = ei.clone()
    dropped[0, int(sel[2])] = n                                                 # graph_prepare drops this column (source out of range)
    assert count(sel, qn, dropped) >= 2                                         # ... 1 there, and the selection holds a dropped column
    dup = torch.sort(torch.cat([qn, qn[1:2]])).values
    assert count(sel, dup) == 1                                                 # duplicate qnodes
    # without a status argument the count is read back and raised
    with pytest.raises(IndexError, match="index contract"):
        ops.gnn_forward_query(irr["packed"], irr["feat"], ei.to(dev), swapped.to(dev), qn.to(dev), 2)
    with pytest.raises(ValueError):
        ops.gnn_forward_query(irr["packed"], irr["feat"], ei.to(dev), torch.arange(e + 1).to(dev), qn.to(dev), 2)


# ----------------------------------------------------------------------------------------------------------------------
# 3. workspace independence
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True])
def test_poisoned_workspace_gives_the_same_bits(dev, irr, bf16):
    from relpose_gnn_amd import _lib
    n, e = irr["feat"].shape[0], irr["ei"].shape[1]
    for qset in ("first", "all"):
        need = int(_lib.lib().rpg_gnn_query_workspace_bytes(n, e, R.FWD_D, irr["sel"][qset].numel(), len(irr["sets"][qset])))
        clean = torch.zeros(need, dtype=torch.uint8, device=dev)
        poisoned = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)         # every fp32 word a NaN, every index -1
        a = _run_query(dev, irr, qset, 2, bf16=bf16, want_features=True, workspace=clean)
        b = _run_query(dev, irr, qset, 2, bf16=bf16, want_features=True, workspace=poisoned)
        for x, y in zip(a, b):
            assert bool(torch.isfinite(x).all()) and torch.equal(x, y)


# ----------------------------------------------------------------------------------------------------------------------
# 4. forward_map(outputs="query") against forward_map()
# ----------------------------------------------------------------------------------------------------------------------
def _small(dev, precision="f32", **kw):
    import relpose_gnn_amd.synth as S
    from relpose_gnn_amd.posenet import PoseNetX_R2
    from relpose_gnn_amd.resnet import ResNet
    planes, blocks = (8, 16, 32, 64), (1, 1, 1, 1)
    args = dict(droprate=0.0, knn=-1, use_AP=True, gnn_recursion=2, use_attention=False, L=1)
    args.update(kw)
    m = PoseNetX_R2(ResNet(blocks, planes), pretrained=False, feat_dim=64, edge_feat_dim=64, node_dim=64, input_img_height=H,
                    use_gnn=True, **args)
    m.load_state_dict(S.synth_state_dict(S.posenet_r2_param_shapes(64, 64, 64, planes, blocks), seed=1))
    m = m.to(dev).eval()
    m.encoder_dtype = m.gnn_dtype = precision
    return m


@pytest.fixture(scope="module")
def data():
    import relpose_gnn_amd.synth as S
    gen = torch.Generator().manual_seed(6)
    queries = S.synth_images(33, H, W, seed=92)
    return dict(mimgs=S.synth_images(M, H, W, seed=91), queries=queries, poses=torch.randn(M, 6, generator=gen) * 0.3,
                targets=torch.randn(33, 6, generator=gen) * 0.3,
                nb=torch.randint(0, M, (33, 7), generator=torch.Generator().manual_seed(11), dtype=torch.int64))


@pytest.fixture(scope="module")
def models(dev, data):
    """One model and map per precision, shared by the tests below (none of them changes the weights)."""
    from relpose_gnn_amd.featmap import FeatureMap
    out = {}
    for precision in ("f32", "bf16"):
        m = _small(dev, precision)
        out[precision] = (m, FeatureMap.build(m, data["mimgs"], poses=data["poses"]), FeatureMap.build(m, data["mimgs"]))
    return out


def _rule(k=K):
    from relpose_gnn_amd.retrieval import RetrievalRule
    return RetrievalRule.reference(k=k, sampling_period=1, seed=5)


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("k", [1, 3, 7])
@pytest.mark.parametrize("g", [1, 4, 33])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_forward_map_query_equals_all(dev, data, models, precision, g, k, streams):
    """abs poses at rows g (K + 1), rel poses at the query_edge_columns of the full list; G = 33 is two uneven stream slots."""
    from relpose_gnn_amd.graph import query_edge_columns
    m, fmap, _ = models[precision]
    tol = TOL_FP32_ORACLE if precision == "f32" else TOL_BF16
    q, nb = data["queries"][:g].to(dev), data["nb"][:g, :k].contiguous().to(dev)
    m.hip_streams = streams
    try:
        ab, rel, ei = m.forward_map(q, nb, fmap)
        ab_q, rel_q, ei_q = m.forward_map(q, nb, fmap, outputs="query")
        m.check_edge_index()
    finally:
        m.hip_streams = 2
    qn = torch.arange(g) * (k + 1)
    cols = query_edge_columns(ei.cpu(), qn).to(dev)
    assert ab_q.shape == (g, 6) and rel_q.shape == (g * k, 6) and torch.equal(ei_q, ei[:, cols])
    assert torch.equal(ei_q[1].cpu(), qn.repeat_interleave(k))
    assert torch.equal(ei_q[0].cpu(), (qn[:, None] + torch.arange(1, k + 1)[None, :]).reshape(-1))
    ea, er = rel_err(ab_q, ab[qn.to(dev)]), rel_err(rel_q, rel[cols])
    print(f"forward_map query vs all {precision} G={g} K={k} streams={streams}: abs {ea:.3e} rel {er:.3e}")
    assert ea < tol and er < tol, (ea, er)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_forward_map_query_with_a_rule(dev, data, models, precision):
    m, fmap, _ = models[precision]
    tol = TOL_FP32_ORACLE if precision == "f32" else TOL_BF16
    q = data["queries"][:G].to(dev)
    ab, rel, ei, nb = m.forward_map(q, None, fmap, rule=_rule())
    ab_q, rel_q, ei_q, nb_q = m.forward_map(q, None, fmap, rule=_rule(), outputs="query")
    m.check_edge_index()
    from relpose_gnn_amd.graph import query_edge_columns
    qn = torch.arange(G) * (K + 1)
    cols = query_edge_columns(ei.cpu(), qn).to(dev)
    assert torch.equal(nb_q, nb) and nb_q.shape == (G, K) and torch.equal(ei_q, ei[:, cols])
    assert rel_err(ab_q, ab[qn.to(dev)]) < tol and rel_err(rel_q, rel[cols]) < tol


def test_forward_map_all_is_untouched_by_a_query_call(dev, data, models):
    """outputs="all" runs the launches it ran before: the same bits before and after query calls of the same shape (which grow
    the shared workspace), and the full list comes back as the caller's own copy."""
    m, fmap, _ = models["f32"]
    q, nb = data["queries"][:4].to(dev), data["nb"][:4, :K].contiguous().to(dev)
    want = [t.clone() for t in m.forward_map(q, nb, fmap)]
    m.forward_map(q, nb, fmap, outputs="query")
    got = m.forward_map(q, nb, fmap, outputs="all")
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert got[2].data_ptr() != m._map_graphs[(4, K + 1, str(dev))][0].data_ptr()
    m.check_edge_index()


# ----------------------------------------------------------------------------------------------------------------------
# 5. dropout
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("streams", [1, 2])
def test_query_dropout_with_seeded_masks(dev, data, streams):
    """droprate = 0.5: the outputs are the heads on F.dropout of the query-mode features, drawn over [q, D] then [e_sel, D] per
    stream slot in slot order -- other masks than the full forward draws.  The features come from ops.gnn_forward_query on the
    slot's own node features (the same launches on the same shapes: the same bits)."""
    from relpose_gnn_amd import ops
    from relpose_gnn_amd.featmap import FeatureMap
    m = _small(dev, droprate=0.5)
    fmap = FeatureMap.build(m, data["mimgs"], poses=data["poses"])
    g = 4
    q, nb = data["queries"][:g].to(dev), data["nb"][:g, :K].contiguous().to(dev)
    m.hip_streams = streams
    torch.manual_seed(1234)
    ab, rel, ei = m.forward_map(q, nb, fmap, outputs="query")
    torch.cuda.synchronize()
    m.check_edge_index()
    slots = [(0, g)] if streams == 1 else [(0, 2), (2, 4)]
    feats = []
    for g0, g1 in slots:
        edges, _ = m._map_graph(g1 - g0, K + 1, dev)
        sel, qn, _ = m._map_query(g1 - g0, K + 1, dev)
        nodes = ops.gather_graph_nodes(m.encode(q[g0:g1]), fmap.features, nb[g0:g1])
        feats.append(ops.gnn_forward_query(m._gnn_packed, nodes, edges, sel, qn, 2, want_features=True)[2:])
    torch.cuda.synchronize()
    torch.manual_seed(1234)
    t = m._gnn_packed
    want_a, want_r = [], []
    for node_out, edge_out in feats:
        assert node_out.shape == (node_out.shape[0], 64) and edge_out.shape[0] == node_out.shape[0] * K
        want_a.append(ops.pose_heads(F.dropout(node_out, p=0.5), t[18], t[19]))
        want_r.append(ops.pose_heads(F.dropout(edge_out, p=0.5), t[20], t[21]))
    assert torch.equal(ab, torch.cat(want_a)) and torch.equal(rel, torch.cat(want_r))
    ab2, _, _ = m.forward_map(q, nb, fmap, outputs="query")                    # a fresh draw differs (always-on)
    assert not torch.equal(ab2, ab)


# ----------------------------------------------------------------------------------------------------------------------
# 6. relocalize(outputs="query")
# ----------------------------------------------------------------------------------------------------------------------
def _agree_results(a, b):
    """Two EvalResults at the bar tests/test_hip_query_pose.py holds between the device and the host rule."""
    got = np.concatenate([a.pred_poses, a.targ_poses, a.t_loss[:, None], a.q_loss[:, None]], 1)
    want = np.concatenate([b.pred_poses, b.targ_poses, b.t_loss[:, None], b.q_loss[:, None]], 1)
    assert got.shape == want.shape and np.isfinite(want).all()
    err = np.abs(got - want)
    assert (err[:, :15] <= 1e-12 + 1e-12 * np.abs(want[:, :15])).all(), err[:, :15].max()
    assert (err[:, 15] <= 1e-5 + 1e-9 * np.abs(want[:, 15])).all(), err[:, 15].max()


def _same_results(a, b):
    for f in RESULT_FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert x.shape == y.shape and np.array_equal(x, y), f
    assert np.isfinite(a.pred_poses).all()


@pytest.mark.parametrize("fuse", [None, "mean", "median"])
def test_relocalize_query(dev, data, models, fuse):
    from relpose_gnn_amd import evaluate as E
    m, fmap, _ = models["f32"]
    q, nb, targets = data["queries"][:G], data["nb"][:G, :K].contiguous(), data["targets"][:G]
    kw = dict(micro_batch=MB, pose_m=PM, pose_s=PS, targets=targets, fuse=fuse)
    s_all, s_q = {}, {}
    full = E.relocalize(m, fmap, q, nb, stats=s_all, **kw)
    host = E.relocalize(m, fmap, q, nb, outputs="query", stats=s_q, **kw)
    assert s_q["micro_batches"] == 3 and 0 < s_q["d2h_bytes"] < s_all["d2h_bytes"]
    assert s_q["d2h_bytes"] == G * 6 * 4 + G * K * 6 * 4                      # abs [G, 6] and rel [G K, 6], fp32
    # the host rule on forward_map(outputs="query") over the same micro-batch cut, bit for bit
    poses, local = data["poses"].double().numpy(), np.stack([np.arange(1, K + 1), np.zeros(K, dtype=np.int64)])
    preds, targs = [], []
    for b0 in range(0, G, MB):
        _, rel, ei = m.forward_map(q[b0:b0 + MB].to(dev), nb[b0:b0 + MB].to(dev), fmap, outputs="query")
        rel = rel.cpu().numpy()
        for j in range(rel.shape[0] // K):
            g = b0 + j
            assert torch.equal(ei[:, j * K:(j + 1) * K].cpu() - j * (K + 1), torch.from_numpy(local))
            target = np.concatenate([targets[g:g + 1].double().numpy(), poses[nb[g].numpy()]])
            if fuse is None:
                p, t = E.query_pose(rel[j * K:(j + 1) * K], target, local, np.asarray(PM), np.asarray(PS), 0)
            else:
                p, t = E.fused_query_pose(rel[j * K:(j + 1) * K], target, local, np.asarray(PM), np.asarray(PS), fuse)
            preds.append(p)
            targs.append(t)
    m.check_edge_index()
    assert np.array_equal(host.pred_poses, np.stack(preds)) and np.array_equal(host.targ_poses, np.stack(targs))
    assert np.array_equal(host.neighbours, nb.numpy())
    # the full mode's poses, at the bar of the forward (the pose rule is 1-Lipschitz in the relative pose up to pose_s)
    assert rel_err(host.pred_poses[:, :3], full.pred_poses[:, :3]) < TOL_FP32_ORACLE
    # the device rule
    s_d = {}
    devr = E.relocalize(m, fmap, q, nb, outputs="query", postprocess="device", stats=s_d, **kw)
    _agree_results(devr, host)
    assert s_d["d2h_bytes"] == G * 16 * 8
    # with a rule: the retrieved rows come back as before
    h_r = E.relocalize(m, fmap, q, rule=_rule(), outputs="query", **kw)
    d_r = E.relocalize(m, fmap, q, rule=_rule(), outputs="query", postprocess="device", **kw)
    f_r = E.relocalize(m, fmap, q, rule=_rule(), **kw)
    _agree_results(d_r, h_r)
    assert np.array_equal(h_r.neighbours, f_r.neighbours) and np.array_equal(d_r.neighbours, f_r.neighbours)
    assert rel_err(h_r.pred_poses[:, :3], f_r.pred_poses[:, :3]) < TOL_FP32_ORACLE
    if fuse is None:                       # another reference edge: ref_node-th edge into the query on the reduced list too
        a = E.relocalize(m, fmap, q, nb, outputs="query", ref_node=2, **{**kw, "fuse": None})
        b = E.relocalize(m, fmap, q, nb, ref_node=2, **{**kw, "fuse": None})
        assert rel_err(a.pred_poses[:, :3], b.pred_poses[:, :3]) < TOL_FP32_ORACLE


def test_relocalize_query_without_map_poses_returns_the_reduced_raw_tensors(dev, data, models):
    from relpose_gnn_amd import evaluate as E
    from relpose_gnn_amd.graph import query_edge_columns
    m, _, bare = models["f32"]
    q, nb = data["queries"][:G], data["nb"][:G, :K].contiguous()
    ab, rel = E.relocalize(m, bare, q, nb, micro_batch=MB)
    ab_q, rel_q = E.relocalize(m, bare, q, nb, micro_batch=MB, outputs="query")
    assert ab_q.shape == (G, 6) and rel_q.shape == (G * K, 6)
    qn = torch.arange(G) * (K + 1)
    ei = torch.cat([m._map_graph(1, K + 1, dev)[0].cpu() + g * (K + 1) for g in range(G)], 1)
    assert rel_err(ab_q, ab[qn]) < TOL_FP32_ORACLE and rel_err(rel_q, rel[query_edge_columns(ei, qn)]) < TOL_FP32_ORACLE


# ----------------------------------------------------------------------------------------------------------------------
# 7. capture
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("postprocess,fuse", [("host", None), ("device", None), ("device", "mean")])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_capture_equals_eager_in_query_mode(dev, data, precision, postprocess, fuse):
    """capture=True against capture=False, bit for bit, in the query mode (given and retrieved neighbours), then the same in the
    full mode on the same model: each mode captures its own two steps, and a repeated call in either mode captures nothing."""
    from relpose_gnn_amd.evaluate import relocalize
    from relpose_gnn_amd.featmap import FeatureMap
    m = _small(dev, precision)
    fmap = FeatureMap.build(m, data["mimgs"], poses=data["poses"])
    q, nb = data["queries"][:G], data["nb"][:G, :K].contiguous()
    kw = dict(micro_batch=MB, pose_m=PM, pose_s=PS, targets=data["targets"][:G], postprocess=postprocess, fuse=fuse, outputs="query")
    st = {}
    _same_results(relocalize(m, fmap, q, nb, capture=True, stats=st, **kw), relocalize(m, fmap, q, nb, **kw))
    assert st["graphs_captured"] == 2 and st["graph_replays"] == 3 and st["micro_batches"] == 3
    _same_results(relocalize(m, fmap, q, rule=_rule(), capture=True, **kw), relocalize(m, fmap, q, rule=_rule(), **kw))
    # a captured "query" step is not replayed for "all", nor the reverse
    kw_all = {**kw, "outputs": "all"}
    st = {}
    _same_results(relocalize(m, fmap, q, nb, capture=True, stats=st, **kw_all), relocalize(m, fmap, q, nb, **kw_all))
    assert st["graphs_captured"] == 2 and st["graph_replays"] == 3
    for kwargs in (kw, kw_all):
        st = {}
        relocalize(m, fmap, q, nb, capture=True, stats=st, **kwargs)
        assert st["graphs_captured"] == 0 and st["graph_replays"] == 3
    m.check_edge_index()


def test_captured_query_step_holds_its_selection_and_reports_a_bad_neighbour(dev, data, models):
    from relpose_gnn_amd.graphed import GraphedForwardMap
    m, fmap, _ = models["f32"]
    q = data["queries"][:4].to(dev)
    good = data["nb"][:4, :K].contiguous().to(dev)
    bad = good.clone()
    bad[2, 1] = M                                             # one past the map's last row: clamped and counted
    m.forward_map(q, bad, fmap, outputs="query")
    with pytest.raises(IndexError) as eager:
        m.check_edge_index()
    step = GraphedForwardMap(m, fmap, q, K, outputs="query")
    assert step._held["query_sel"] is m._map_queries[(4, K + 1, str(dev))] and step.edge_first is None
    want = [t.clone() for t in m.forward_map(q, good, fmap, outputs="query")]
    out = step(q, good)
    assert out.abs_pose.shape == (4, 6) and out.rel_pose.shape == (4 * K, 6)
    assert all(torch.equal(a, b) for a, b in zip((out.abs_pose, out.rel_pose, out.edge_index), want))
    m.check_edge_index()
    out = step(q, bad)
    assert torch.isfinite(out.rel_pose).all()
    with pytest.raises(IndexError, match="neighbours has 1 index") as replayed:
        m.check_edge_index()
    assert str(replayed.value) == str(eager.value)
    step(q, good)
    m.check_edge_index()                                      # the counters were cleared: a clean replay reports nothing
    # with a pose rule the default cut is K columns per graph
    from relpose_gnn_amd.query_pose import QueryPose
    pose = QueryPose(PM, PS)
    step = GraphedForwardMap(m, fmap, q, K, pose=pose, outputs="query")
    assert step.edge_first.tolist() == [0, K, 2 * K, 3 * K, 4 * K]
    rows = step(q, good).rows
    assert rows.shape == (4, 16) and bool(torch.isfinite(rows[:, :7]).all())
    pose.check()
