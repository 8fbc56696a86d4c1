"""The query-only output mode without a GPU: ``graph.query_edge_columns``, the host pose rules on the reduced rows against the
same rules on the full ones (exact: host float64 on the same values), and every argument error of ``forward_map`` /
``relocalize`` / ``GraphedForwardMap`` that is raised before any device work."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import graph_sweep_ref as R
from relpose_gnn_amd import evaluate as E
from relpose_gnn_amd.graph import fc_batch, fc_edge_index, query_edge_columns


# ---- 1. the selected columns ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g,n", [(1, 2), (3, 4), (5, 8)])
def test_query_edge_columns_on_fc_batches(g, n):
    k = n - 1
    ei = fc_batch(torch.empty((g * n, 0)), n).edge_index
    qn = torch.arange(g) * n
    cols = query_edge_columns(ei, qn)
    assert cols.dtype == torch.int64 and cols.shape == (g * k,)
    assert bool((cols[1:] > cols[:-1]).all()) or g * k == 1
    assert torch.equal(ei[1, cols], qn.repeat_interleave(k))
    assert torch.equal(ei[0, cols], (qn[:, None] + torch.arange(1, k + 1)[None, :]).reshape(-1))
    # graph after graph the list is one pattern: the first j k entries are the selection of j graphs, shifted per graph
    per = n * k
    assert torch.equal(cols, (cols[:k][None, :] + torch.arange(g)[:, None] * per).reshape(-1))
    # the reference edge of test.py:227-229, per graph: the same column through the reduced list as through the full one
    full = fc_edge_index(n).numpy()
    local = query_edge_columns(full, [0]).numpy()
    reduced = full[:, local]
    for ref_node in range(k):
        assert local[E.reference_edge(reduced, ref_node)] == E.reference_edge(full, ref_node)
    with pytest.raises(ValueError):
        E.reference_edge(reduced, k)
    # numpy and list inputs are taken too
    assert torch.equal(query_edge_columns(ei.numpy(), qn.tolist()), cols)


def test_query_edge_columns_on_an_irregular_list():
    """The 12-node graph of the composite sweep: self-loops, repeated edges, shuffled columns, an isolated node."""
    ei = R.forward_graph_edges()[2]
    n = 12
    assert R.has_repeat(ei, n) and bool((ei[0] == ei[1]).any())
    deg = R.in_degrees(ei, n)
    for qn in ([0], [int(deg.argmax())], [3, 7, 11], list(range(n)), [int((deg == 0).nonzero()[0])]):
        cols = query_edge_columns(ei, qn)
        want = [c for c in range(ei.shape[1]) if int(ei[1, c]) in qn]
        assert cols.tolist() == want
        assert len(want) == int(deg[qn].sum())
    assert query_edge_columns(ei, list(range(n))).tolist() == list(range(ei.shape[1]))
    with pytest.raises(ValueError):
        query_edge_columns(ei[0], [0])


# ---- 2. the host pose rules on the reduced rows -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 4, 8])
def test_host_pose_rules_on_the_reduced_rows_equal_the_full_ones(n):
    gen = torch.Generator().manual_seed(n)
    full = fc_edge_index(n).numpy()
    rel = (torch.randn(full.shape[1], 6, generator=gen) * 0.3).numpy()
    target = (torch.randn(n, 6, generator=gen) * 0.3).numpy()
    pm, ps = (1.5, -0.25, 3.0), (2.0, 0.5, 1.25)
    cols = query_edge_columns(full, [0]).numpy()
    rel_q, edges_q = rel[cols], full[:, cols]
    for ref_node in range(n - 1):
        a, b = E.query_pose(rel_q, target, edges_q, pm, ps, ref_node), E.query_pose(rel, target, full, pm, ps, ref_node)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for fuse in E.FUSE_MODES:
        for max_edges in (1, 2, 64):
            a = E.fused_query_pose(rel_q, target, edges_q, pm, ps, fuse, max_edges)
            b = E.fused_query_pose(rel, target, full, pm, ps, fuse, max_edges)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.array_equal(E.fused_query_row(rel_q, target, edges_q, pm, ps, fuse), E.fused_query_row(rel, target, full, pm, ps, fuse))


# ---- 3. argument errors, before any device work ---------------------------------------------------------------------------------------
def _model(**kw):
    import relpose_gnn_amd.synth as S
    from relpose_gnn_amd.posenet import PoseNetX_R2
    from relpose_gnn_amd.resnet import ResNet
    planes, blocks = (8, 16, 32, 64), (1, 1, 1, 1)
    args = dict(droprate=0.0, knn=-1, use_AP=True, use_attention=False)
    args.update(kw)
    m = PoseNetX_R2(ResNet(blocks, planes), pretrained=False, feat_dim=64, edge_feat_dim=64, node_dim=64, input_img_height=32,
                    use_gnn=True, **args)
    m.load_state_dict(S.synth_state_dict(S.posenet_r2_param_shapes(64, 64, 64, planes, blocks, use_attention=args["use_attention"],
                                                                   use_AP=args["use_AP"]), seed=1))
    return m.eval()


class _NoMap:
    """A feature map nothing may look at: the refusals come first."""
    device = torch.device("cpu")

    def __getattr__(self, name):
        raise AssertionError(f"the feature map was read ({name}) before the argument was refused")


Q, NB = torch.zeros(2, 3 * 32 * 32), torch.zeros((2, 3), dtype=torch.int64)


@pytest.mark.parametrize("bad", ["Query", "none", None, 1, True])
def test_unknown_outputs_is_a_value_error(bad):
    from relpose_gnn_amd.graphed import GraphedForwardMap
    m = _model()
    with pytest.raises(ValueError, match="outputs"):
        m.forward_map(Q, NB, _NoMap(), outputs=bad)
    with pytest.raises(ValueError, match="outputs"):
        E.relocalize(m, _NoMap(), Q, NB, outputs=bad)
    with pytest.raises(ValueError, match="outputs"):
        GraphedForwardMap(m, _NoMap(), Q, 3, outputs=bad)


@pytest.mark.parametrize("kw,call,flag", [(dict(knn=4), {}, "knn"), ({}, dict(k=2), "explicit k"),
                                          (dict(use_attention=True), {}, "use_attention"), (dict(use_AP=False), {}, "use_AP=False")],
                         ids=["knn", "k", "use_attention", "use_AP"])
def test_what_the_query_mode_does_not_serve_names_the_flag(kw, call, flag):
    from relpose_gnn_amd.graphed import GraphedForwardMap
    m = _model(**kw)
    with pytest.raises(NotImplementedError, match=flag):
        m.forward_map(Q, NB, _NoMap(), outputs="query", **call)
    assert m._gnn_packed is None                          # nothing was packed, nothing queued
    if not call:
        with pytest.raises(NotImplementedError, match=flag):
            E.relocalize(m, _NoMap(), Q, NB, outputs="query")
    # outputs="all" is not refused for any of them: it goes on to the device rule (there is no CPU compute path)
    fmap = SimpleNamespace(device=torch.device("cpu"))
    with pytest.raises(RuntimeError, match="queries must be on the GPU"):
        m.forward_map(Q, NB, fmap, **call)
    if not call:
        with pytest.raises(NotImplementedError):
            GraphedForwardMap(m, _NoMap(), Q, 3, outputs="query")


def test_forward_map_query_on_the_cpu_ends_at_the_device_rule():
    m = _model()
    fmap = SimpleNamespace(device=torch.device("cpu"))
    with pytest.raises(RuntimeError, match="queries must be on the GPU"):
        m.forward_map(Q, NB, fmap, outputs="query")


# ---- 4. relocalize on a map that is not on a GPU: the synchronous path, with the model's forward_map asked for "query" --------------
G, K, M = 5, 3, 9


class _FakeMapModel:
    """``_FakeMapModel`` of test_pipeline_cpu.py with the ``outputs`` argument: "query" returns the query rows / the columns into
    the query nodes of what "all" returns."""
    knn = -1

    def __init__(self):
        self.asked = []

    def forward_map(self, x, nb, fmap, outputs="all"):
        self.asked.append(outputs)
        n = K + 1
        table = fmap.poses if fmap.poses is not None else fmap.features
        y = torch.cat([x[:, None, :6], table[nb]], 1).reshape(-1, 6)
        ei = torch.cat([fc_edge_index(n) + g * n for g in range(x.shape[0])], 1)
        rel = y[ei[1]] - y[ei[0]] + 0.01
        if outputs == "all":
            return y, rel, ei
        qn = torch.arange(x.shape[0]) * n
        cols = query_edge_columns(ei, qn)
        return y[qn], rel[cols], ei[:, cols]


@pytest.fixture(scope="module")
def map_case():
    g = torch.Generator().manual_seed(7)
    table = torch.randn(M, 6, generator=g) * 0.3
    targets = torch.randn(G, 6, generator=g) * 0.3
    queries = torch.cat([targets, torch.zeros(G, 6)], 1)            # the "image" of a query carries its row of y
    nb = torch.randint(0, M, (G, K), generator=g)
    return SimpleNamespace(device=torch.device("cpu"), poses=table, features=table, descriptors=None), queries, nb, targets


@pytest.mark.parametrize("fuse", [None, "mean", "median"])
def test_relocalize_query_on_a_cpu_map_takes_the_synchronous_path(map_case, fuse):
    fmap, queries, nb, targets = map_case
    kw = dict(micro_batch=2, pose_m=(1.0, 2.0, 3.0), pose_s=(2.0, 2.0, 0.5), targets=targets, fuse=fuse)
    for ref_node in ((0, 2) if fuse is None else (0,)):
        full, reduced, stats = _FakeMapModel(), _FakeMapModel(), {}
        a = E.relocalize(full, fmap, queries, nb, ref_node=ref_node, **kw)
        b = E.relocalize(reduced, fmap, queries, nb, ref_node=ref_node, outputs="query", stats=stats, **kw)
        assert full.asked == ["all"] * 3 and reduced.asked == ["query"] * 3
        for f in ("pred_poses", "targ_poses", "t_loss", "q_loss", "neighbours"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
        assert stats["micro_batches"] == 3 and stats["h2d_bytes"] == 0
    # without targets: the poses alone
    kw.pop("targets")
    assert np.array_equal(E.relocalize(_FakeMapModel(), fmap, queries, nb, **kw),
                          E.relocalize(_FakeMapModel(), fmap, queries, nb, outputs="query", **kw))


def test_relocalize_query_without_map_poses_returns_the_reduced_raw_tensors(map_case):
    fmap, queries, nb, _ = map_case
    bare = SimpleNamespace(device=fmap.device, poses=None, features=fmap.features, descriptors=None)
    ab, rel = E.relocalize(_FakeMapModel(), bare, queries, nb, micro_batch=2)
    ab_q, rel_q = E.relocalize(_FakeMapModel(), bare, queries, nb, micro_batch=2, outputs="query")
    assert ab.shape == (G * (K + 1), 6) and rel.shape == (G * K * (K + 1), 6)
    assert ab_q.shape == (G, 6) and rel_q.shape == (G * K, 6)
    ei = torch.cat([fc_edge_index(K + 1) + g * (K + 1) for g in range(G)], 1)
    qn = torch.arange(G) * (K + 1)
    assert torch.equal(ab_q, ab[qn]) and torch.equal(rel_q, rel[query_edge_columns(ei, qn)])


def test_relocalize_query_refuses_a_knn_model_without_the_check(map_case):
    fmap, queries, nb, _ = map_case
    model = _FakeMapModel()
    model.knn = 2
    with pytest.raises(NotImplementedError, match="knn"):
        E.relocalize(model, fmap, queries, nb, micro_batch=2, outputs="query")
    assert model.asked == []


# ---- 5. the library's size function (no GPU needed) --------------------------------------------------------------------------------
def test_query_workspace_bytes():
    from relpose_gnn_amd import _lib
    lib = _lib.lib()
    assert "rpg_gnn_forward_query_f32" in _lib.SYMBOLS and "rpg_gnn_forward_query_bf16" in _lib.SYMBOLS
    full = lib.rpg_gnn_workspace_bytes(8, 56, 64)
    assert lib.rpg_gnn_query_workspace_bytes(8, 56, 64, 7, 1) > full + 7 * 64 * 6 + 64 * 8
    for bad in ((8, 56, 64, 0, 1), (8, 56, 64, 57, 1), (8, 56, 64, 7, 0), (8, 56, 64, 7, 9), (8, 56, 100, 7, 1)):
        assert lib.rpg_gnn_query_workspace_bytes(*bad) == 0
