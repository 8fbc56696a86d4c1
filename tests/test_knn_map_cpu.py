"""The kNN map step at fixed positions without a GPU: the reference statements of tests/knn_map_ref.py on integer features, and
the host contract of ``model.static_knn`` -- what is still refused, the cached selection, ``relocalize``'s ``ref_node`` rule and the
argument limits of ``rpg_knn_graph_uniform_f32``, all of which answer before any device work."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

import graph_sweep_ref as R
import knn_map_ref as KR
from relpose_gnn_amd import evaluate as E


# ---- 1. the reference statements ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g,n_per,k", [(1, 2, 1), (2, 3, 4), (3, 5, 4), (2, 8, 4), (1, 9, 7), (2, 8, 64), (1, 65, 4)])
def test_uniform_knn_layout(g, n_per, k):
    """Grouped by target in node order, k' = min(k, n_per - 1) columns each, nearest first, ties by index, sources within the
    target's graph -- and, the features being regular, the whole of knn_graph_exact's list."""
    x = KR.planted_ties(g, n_per, 16, seed=n_per + k)
    kp = min(k, n_per - 1)
    ei = KR.uniform_knn(x, g, n_per, k)
    assert ei.shape == (2, g * n_per * kp)
    assert torch.equal(ei[1], torch.arange(g * n_per).repeat_interleave(kp))
    assert bool((ei[0] // n_per == ei[1] // n_per).all()) and bool((ei[0] != ei[1]).all())
    xi = x.to(torch.int64)
    dist = ((xi[ei[0]] - xi[ei[1]]) ** 2).sum(1).reshape(g * n_per, kp)
    assert bool((dist[:, 1:] >= dist[:, :-1]).all())                                    # nearest first
    tie = dist[:, 1:] == dist[:, :-1]
    src = ei[0].reshape(g * n_per, kp)
    assert bool((src[:, 1:][tie] > src[:, :-1][tie]).all())                             # ties by index
    if n_per >= 3:                                                                      # the planted tie: node 0's two nearest
        assert src[0, 0].item() == 1 and (kp < 2 or src[0, 1].item() == 2)
    assert KR.irregular_nodes(x, g, n_per, k) == 0
    assert torch.equal(ei, R.knn_graph_exact(x, k, KR.uniform_batch(g, n_per)))
    assert torch.equal(KR.uniform_knn(x, g, n_per, k, node_offset=40), ei + 40)
    q = KR.query_columns(g, n_per, k)
    assert torch.equal(ei[1, q], (torch.arange(g) * n_per).repeat_interleave(kp))


def test_duplicate_rows_give_exactly_one_irregular_node():
    x = KR.duplicate_rows_example()
    assert KR.reference_in_degrees(x, 1, 8, 4).tolist() == [4, 4, 4, 4, 4, 4, 5, 4]
    assert R.knn_graph_exact(x, 4).shape[1] == 33 and KR.irregular_nodes(x, 1, 8, 4) == 1
    ei = KR.uniform_knn(x, 1, 8, 4)
    assert ei.shape == (2, 32) and ei[0, 24:28].tolist() == [1, 2, 3, 4]               # node 6: the first four of its five


@pytest.mark.parametrize("n_per", [2, 3, 5, 6])
@pytest.mark.parametrize("k", [5, 7, 64])
def test_small_graphs_are_never_irregular(n_per, k):
    """n_per - 1 <= k: the k + 1 nearest of a node are all nodes of its graph, itself included, whatever the rows are."""
    x = R.integer_features(3 * n_per, 8, seed=n_per)
    x[:n_per] = x[0]                                                                    # a graph of identical rows
    assert n_per - 1 <= k and KR.irregular_nodes(x, 3, n_per, k) == 0
    assert KR.uniform_knn(x, 3, n_per, k).shape == (2, 3 * n_per * (n_per - 1))


@pytest.mark.parametrize("g,n_per,k", [(2, 3, 4), (3, 8, 4), (1, 9, 7), (1, 12, 1)])
def test_insertion_statement_is_the_exact_oracle_on_integer_features(g, n_per, k):
    """The rule stated for any floats (the yardstick of the non-finite rows on the GPU) against knn_graph_exact where both apply:
    exact ties, duplicates and the irregular example."""
    for x in (KR.planted_ties(g, n_per, 16, seed=g + n_per), R.integer_features(g * n_per, 8, seed=k)):
        ei, irregular = KR.insertion_knn(x, g, n_per, k)
        assert irregular == KR.irregular_nodes(x, g, n_per, k) and torch.equal(ei, KR.uniform_knn(x, g, n_per, k))
    x = KR.duplicate_rows_example()
    ei, irregular = KR.insertion_knn(x, 1, 8, 4)
    assert irregular == 1 and torch.equal(ei, KR.uniform_knn(x, 1, 8, 4))
    x = torch.randn(8, 8, generator=torch.Generator().manual_seed(1))
    x[6] = float("nan")                                                                 # its self match is NaN and never enters
    ei, irregular = KR.insertion_knn(x, 1, 8, 4)
    assert irregular == 1 and ei[0, 24:28].tolist() == [0, 1, 2, 3] and int(ei[0].max()) < 8


# ---- 2. the host contract -----------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("kw,call,flag", [(dict(knn=4), {}, "knn"), ({}, dict(k=2), "explicit k"),
                                          (dict(use_attention=True), {}, "use_attention"), (dict(use_AP=False), {}, "use_AP=False")],
                         ids=["knn", "k", "use_attention", "use_AP"])
def test_without_static_knn_the_four_refusals_stand(kw, call, flag):
    """tests/test_query_outputs_cpu.py::test_what_the_query_mode_does_not_serve_names_the_flag, on a model that has the attribute
    and leaves it unset."""
    from relpose_gnn_amd.graphed import GraphedForwardMap
    m = _model(**kw)
    assert m.static_knn is False and "static_knn" not in m.state_dict()
    with pytest.raises(NotImplementedError, match=flag):
        m.forward_map(Q, NB, _NoMap(), outputs="query", **call)
    assert m._gnn_packed is None
    if not call:
        with pytest.raises(NotImplementedError, match=flag):
            E.relocalize(m, _NoMap(), Q, NB, outputs="query")
        with pytest.raises(NotImplementedError):
            GraphedForwardMap(m, _NoMap(), Q, 3, outputs="query")
    if kw.get("knn", -1) > 0:
        with pytest.raises(NotImplementedError, match="graph capture covers the deterministic fully-connected path"):
            GraphedForwardMap(m, _NoMap(), Q, 3)


def test_with_static_knn_the_query_mode_passes_knn_and_refuses_the_rest():
    m = _model(knn=4)
    m.static_knn = True
    m._check_outputs("query", None)
    m._check_outputs("all", None)
    with pytest.raises(NotImplementedError, match="explicit k"):
        m._check_outputs("query", 2)
    fmap = SimpleNamespace(device=torch.device("cpu"))
    with pytest.raises(RuntimeError, match="queries must be on the GPU"):           # past the refusals: the device rule
        m.forward_map(Q, NB, fmap, outputs="query")
    for kw, flag in ((dict(use_attention=True), "use_attention"), (dict(use_AP=False), "use_AP=False")):
        other = _model(knn=4, **kw)
        other.static_knn = True
        with pytest.raises(NotImplementedError, match=flag):
            other.forward_map(Q, NB, _NoMap(), outputs="query")
        assert other._static_columns(None, 7) == 0                                  # ... and outputs="all" keeps the general path
    assert m._static_columns(None, 7) == 4 and m._static_columns(None, 3) == 3 and m._static_columns(2, 7) == 0
    m.static_knn = False
    assert m._static_columns(None, 7) == 0
    assert _model()._static_columns(None, 7) == 0                                   # knn <= 0: nothing to build


@pytest.mark.parametrize("g,n_per,kp", [(1, 2, 1), (4, 8, 4), (33, 4, 3)])
def test_cached_selection_is_the_fixed_positions(g, n_per, kp):
    m = _model(knn=4)
    sel, qn = m._map_query_knn(g, n_per, kp, torch.device("cpu"))
    assert sel.dtype == qn.dtype == torch.int64
    assert sel.tolist() == [gi * n_per * kp + t for gi in range(g) for t in range(kp)]
    assert qn.tolist() == [gi * n_per for gi in range(g)]
    assert torch.equal(sel, KR.query_columns(g, n_per, kp))
    assert m._map_query_knn(g, n_per, kp, torch.device("cpu"))[0] is sel            # cached
    # the first j k' entries are the local selection of any j consecutive graphs
    assert torch.equal(sel[:kp], KR.query_columns(1, n_per, kp))


def test_relocalize_refuses_ref_node_past_the_knn_edges():
    m = _model(knn=4)
    m.static_knn = True
    for nb, ref_node in ((NB, 3), (torch.zeros((2, 7), dtype=torch.int64), 4)):     # k' = min(4, 3) = 3, min(4, 7) = 4
        with pytest.raises(ValueError, match="ref_node"):
            E.relocalize(m, _NoMap(), Q, nb, ref_node=ref_node)
    m.static_knn = False                                                            # unset: on to the map, as before
    with pytest.raises(AssertionError, match="the feature map was read"):
        E.relocalize(m, _NoMap(), Q, NB, ref_node=3)


def test_irregular_knn_graph_is_a_value_error_that_names_the_remedy():
    from relpose_gnn_amd.posenet import IrregularKnnGraph, _bad_index_error
    counts = torch.zeros(24, dtype=torch.int32)
    counts[17] = 2
    exc = _bad_index_error(counts)
    assert isinstance(exc, IrregularKnnGraph) and isinstance(exc, ValueError) and "static_knn = False" in str(exc)
    counts[3] = 1                                                                   # with a bad edge it stays the IndexError
    exc = _bad_index_error(counts)
    assert isinstance(exc, IndexError) and "static_knn" in str(exc)
    counts = torch.zeros(24, dtype=torch.int32)
    counts[9] = 1
    assert str(_bad_index_error(counts)).startswith("neighbours has 1 index")


def test_entry_point_argument_limits():
    from relpose_gnn_amd import _lib
    lib = _lib.lib()
    assert "rpg_knn_graph_uniform_f32" in _lib.SYMBOLS
    buf = (ctypes.c_char * 4096)()
    a = (ctypes.addressof(buf) + 15) // 16 * 16
    f = lib.rpg_knn_graph_uniform_f32

    def call(x=a, g=1, n_per=8, d=64, k=4, off=0, src=a, dst=a, q_src=None, q_dst=None, irregular=a):
        return f(x, g, n_per, d, k, off, src, dst, q_src, q_dst, irregular, None)
    bad = _lib.RPG_ERR_BAD_ARG
    assert call(n_per=1) == bad and call(n_per=2049) == bad
    assert call(k=65) == bad and call(k=0) == bad
    assert call(d=62) == bad and call(d=0) == bad
    assert call(x=a + 4) == bad                                                     # misaligned x
    assert call(q_src=a) == bad and call(q_dst=a) == bad                            # one of the pair
    assert call(x=None) == bad and call(src=None) == bad and call(dst=None) == bad and call(irregular=None) == bad
    assert call(g=0) == bad and call(off=-1) == bad
