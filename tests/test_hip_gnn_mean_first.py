"""The mean-first message path of the fp32 GNN forward on the GPU (rpg_gnn_forward_f32 / rpg_gnn_forward_query_f32 with the 30-tensor
table of params.pack_gnn_mean_first): mlp.2 applied behind the mean over a node's incoming edges, not per edge.

Every case runs the composite twice in one process -- RPG_TUNE_GNN_FUSE_AGG at its default (mean first) and at 2 (mlp.2 per edge,
the 26-tensor formulation) -- on the GNN alone (random node features, no encoder), against oracle/posenet_ref.gnn_forward in fp32
and in float64:
  * both results within 1e-4 (max-norm relative, the bar of tests/test_hip_model.py) of the CPU fp32 oracle;
  * the mean-first result no further from the float64 oracle than 1.5 x max(the CPU fp32 oracle's own distance, 3e-6): the noise-floor
    bar of tests/test_hip_bench_geometry.py.  The yardstick is the oracle, never the other kernel path.
The two distances and their ratio are printed and appended to the file RPG_SWEEP_RECORD names; profiles/gnn_mean_first_observed.json
holds one such run on an MI355X.

Shapes: the smallest at which the path can go wrong.  D = 64 (c = 8: K = 72 of the node Linear is no multiple of 16, one 64-channel
quarter in the aggregate kernel) and D = 256 (c = 32, K = 288); the ragged batch of fully connected graphs of 8, 5 and 8 nodes; the
8-node graph with in-degrees 0 .. 6, whose node 0 has no incoming edge (its aggregate must be exactly zero: the summed biases reach
the node Linear as a residual row that is zero there, never as a bias operand); repeated edges; 0, 1 and 2 recursions; the
query-only entry point, whose last recursion runs the same lines on the selected rows; and D = 2048 once (two 8-node graphs: the node
Linear at K = 2304).
"""
import ctypes
import json
import os

import pytest
import torch

import gnn_mean_first_ref as R
from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4                      # tests/test_hip_model.py
NOISE, FLOOR = 1.5, 3e-6        # tests/test_hip_bench_geometry.py::test_fp32_error_is_the_fp32_noise_floor
PER_EDGE = {"GNN_FUSE_AGG": 2}  # fused aggregation with mlp.2 on the edge rows


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _record(case, **figures):
    path = os.environ.get("RPG_SWEEP_RECORD")
    print("gnn_mean_first", case, figures)
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"section": "gnn_mean_first", "case": case, **figures}) + "\n")


_WEIGHTS = {}


def _weights(d, dev):
    """Per width, made once: the state dict, its float64 image, the 30-tensor table on the GPU."""
    if d not in _WEIGHTS:
        import relpose_gnn_amd.synth as S
        from relpose_gnn_amd.params import pack_gnn, pack_gnn_mean_first
        shapes = {k: v for k, v in S.posenet_r2_param_shapes(d, d, d, (8, 16, 32, 64), (1, 1, 1, 1)).items()
                  if not k.startswith("feature_extractor.")}
        # synth_state_dict's scales from torch.randn (its hashed normals take 9 s at D = 2048): weights of variance 2 / fan_in in front
        # of a ReLU, 1 / fan_in elsewhere, biases N(0, 0.05)
        g = torch.Generator().manual_seed(d)
        sd = {k: torch.randn(shp, generator=g) * (0.05 if len(shp) == 1 else ((2.0 if k.endswith(".0.weight") else 1.0) / shp[1]) ** 0.5)
              for k, shp in shapes.items()}
        t = pack_gnn(sd)
        assert len(t) == 26
        packed = [v.to(dev) for v in t + pack_gnn_mean_first(t)]
        _WEIGHTS[d] = (sd, {k: v.double() for k, v in sd.items()}, packed)
    return _WEIGHTS[d]


_GRAPHS = {"ragged_fc_8_5_8": R.ragged_fc_batch, "knn_like_isolated": R.knn_like_graph, "duplicated_edges": R.duplicated_edges_graph,
           "two_fc_8": lambda: R.ragged_fc_batch((8, 8))}
_ORACLE = {}


def _case(graph, d, recursion, dev):
    """Per (graph, width, recursions), made once and left unchanged: features, edge list, fp32 and float64 oracle outputs."""
    key = (graph, d, recursion)
    if key not in _ORACLE:
        import relpose_gnn_amd.synth as S
        from oracle import posenet_ref as O
        sd, sd64, _ = _weights(d, dev)
        ei, n = _GRAPHS[graph]()
        x = S.hash_normal(f"mean_first.{graph}.{d}", (n, d), 1.0, 0.0, seed=7)
        with torch.no_grad():
            o32 = O.gnn_forward(sd, x, ei, recursion)
            o64 = O.gnn_forward(sd64, x.double(), ei, recursion)
        _ORACLE[key] = (x, ei, n, o32, o64)
    return _ORACLE[key]


def _forward(packed, x, ei, recursion, dev):
    """rpg_gnn_forward_f32 on the whole graph -> (abs_pose [n, 6], rel_pose [e, 6]) on the host."""
    from relpose_gnn_amd import _lib
    lib = _lib.lib()
    feat, ei = x.to(dev).contiguous(), ei.to(dev).contiguous()
    (n, d), e = feat.shape, ei.shape[1]
    ws = torch.empty(int(lib.rpg_gnn_workspace_bytes(n, e, d)), dtype=torch.uint8, device=dev)
    a, r = torch.empty((n, 6), device=dev), torch.empty((e, 6), device=dev)
    status = torch.zeros(16, dtype=torch.int32, device=dev)
    rc = lib.rpg_gnn_forward_f32(_lib.ptr_array([t.data_ptr() for t in packed]), len(packed), feat.data_ptr(), ei[0].data_ptr(),
                                 ei[1].data_ptr(), 0, n, e, d, recursion, a.data_ptr(), r.data_ptr(), None, None, status.data_ptr(),
                                 ws.data_ptr(), ws.numel(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "gnn_forward")
    torch.cuda.synchronize()
    assert int(status[0]) == 0
    return a.cpu(), r.cpu()


def _check(case, on, off, o32, o64):
    """on / off / o32 / o64: (abs_pose, rel_pose) of the mean-first run, the per-edge run, the fp32 and the float64 oracle."""
    figures = {}
    for k, name in enumerate(("abs", "rel")):
        hip64, cpu64 = rel_err(on[k], o64[k]), rel_err(o32[k], o64[k])
        figures.update({f"hip_vs_fp64_{name}": hip64, f"cpu_fp32_vs_fp64_{name}": cpu64, f"ratio_{name}": hip64 / max(cpu64, 1e-30),
                        f"hip_vs_fp32_oracle_{name}": rel_err(on[k], o32[k]), f"per_edge_vs_fp32_oracle_{name}": rel_err(off[k], o32[k]),
                        f"per_edge_vs_fp64_{name}": rel_err(off[k], o64[k])})
    _record(case, **figures)
    for name in ("abs", "rel"):
        assert figures[f"hip_vs_fp32_oracle_{name}"] < TOL and figures[f"per_edge_vs_fp32_oracle_{name}"] < TOL, (case, figures)
        assert figures[f"hip_vs_fp64_{name}"] <= NOISE * max(figures[f"cpu_fp32_vs_fp64_{name}"], FLOOR), (case, figures)
    return figures


CASES = ([("ragged_fc_8_5_8", d, r) for d in (64, 256) for r in (0, 1, 2)]
         + [("knn_like_isolated", d, 2) for d in (64, 256)] + [("duplicated_edges", 64, 2), ("two_fc_8", 2048, 2)])


@pytest.mark.parametrize("graph,d,recursion", CASES)
def test_full_forward(dev, graph, d, recursion):
    from relpose_gnn_amd import ops
    assert ops.tuning_default("GNN_FUSE_AGG") == ops.get_tuning("GNN_FUSE_AGG") == 1          # mean first is the default
    packed = _weights(d, dev)[2]
    x, ei, n, o32, o64 = _case(graph, d, recursion, dev)
    ops.timing_enable(True)
    try:
        ops.timing_read()
        on = _forward(packed, x, ei, recursion, dev)
        launches_on = ops.timing_read()["linear"]["launches"]
        with ops.tuned(PER_EDGE):
            off = _forward(packed, x, ei, recursion, dev)
        launches_off = ops.timing_read()["linear"]["launches"]
    finally:
        ops.timing_enable(False)
    # the key selects the path: per recursion, mlp.2 on the edge rows is one Linear launch more
    assert launches_off - launches_on == recursion, (launches_on, launches_off)
    # ... and the 26-tensor table gives the per-edge result whatever the key says
    assert all(torch.equal(p, q) for p, q in zip(_forward(packed[:26], x, ei, recursion, dev), off))
    _check(f"{graph} D={d} recursion={recursion}", on, off, o32, o64)
    if graph == "knn_like_isolated":
        # the isolated node's outputs: its aggregate is zero in the oracle, so a bias that reached it would show here
        assert rel_err(on[0][R.ISOLATED:R.ISOLATED + 1], o32[0][R.ISOLATED:R.ISOLATED + 1]) < TOL


@pytest.mark.parametrize("d", [64, 256])
@pytest.mark.parametrize("recursion", [1, 2])
def test_query_only_forward(dev, d, recursion):
    """rpg_gnn_forward_query_f32 on the ragged batch, the first node of every graph as the query: the pruned last recursion runs the
    mean-first lines on the selected edge rows and the query node rows."""
    from relpose_gnn_amd import ops
    from relpose_gnn_amd.graph import query_edge_columns
    packed = _weights(d, dev)[2]
    x, ei, n, o32, o64 = _case("ragged_fc_8_5_8", d, recursion, dev)
    qn = torch.tensor([0, 8, 13], dtype=torch.int64)
    sel = query_edge_columns(ei, qn)
    assert sel.numel() == 7 + 4 + 7

    def run():
        a, r = ops.gnn_forward_query(packed, x.to(dev), ei.to(dev), sel.to(dev), qn.to(dev), recursion)
        return a.cpu(), r.cpu()
    on = run()
    with ops.tuned(PER_EDGE):
        off = run()
    _check(f"query_only ragged_fc_8_5_8 D={d} recursion={recursion}", on, off, (o32[0][qn], o32[1][sel]), (o64[0][qn], o64[1][sel]))


@pytest.mark.parametrize("d", [64, 256])
def test_aggregate_entry_point_isolated_node(dev, d):
    """rpg_attention_aggregate_hidden_f32 and the node Linear behind it on the graph with an isolated node: hbar is the scatter-mean
    of the hidden rows bit for bit (the same summation order), ybar is attention_aggregate's, the residual rows are the bias or
    zeros, and the isolated node's aggregate row is bit-zero; the other rows meet the float64 reference step."""
    from relpose_gnn_amd import ops
    ei, n = R.knn_like_graph()
    e, c = ei.shape[1], d // 8
    h, w2, b2, wg, bg, wa, ba = R.step_operands(d, e, seed=5, dtype=torch.float32)
    gtp = (h.double() @ (wg.double() @ w2.double()).T + (wg.double() @ b2.double() + bg.double())).float()
    bias = ba + b2
    gp = ops.graph_prepare(ei.to(dev), n)
    ybar, hbar, res = ops.attention_aggregate_hidden(gtp.to(dev), h.to(dev), gp["rowptr"], gp["perm"], n, bias.to(dev))
    y_ref, m_ref = ops.attention_aggregate(gtp.to(dev), h.to(dev), gp["rowptr"], gp["perm"], n)
    assert torch.equal(hbar, ops.scatter_mean(h.to(dev), gp["rowptr"], gp["perm"], n)) and torch.equal(hbar, m_ref)
    assert torch.equal(ybar, y_ref)
    indeg = torch.tensor(R.IN_DEGREES)
    want_res = torch.where((indeg > 0).unsqueeze(1), bias.unsqueeze(0), torch.zeros(1, d))
    assert torch.equal(res.cpu(), want_res)
    agg = ops.linear_gather([(hbar, None), (ybar, None)], torch.cat([w2, wa], 1).contiguous().to(dev), None, n, residual=res).cpu()
    iso = R.ISOLATED
    for t in (ybar.cpu(), hbar.cpu(), res.cpu(), agg):
        assert not t[iso].any() and not torch.signbit(t[iso]).any()                    # bit-zero: +0.0 in every element
    ref = R.step_reference(h.double(), ei[1], n, *(v.double() for v in (w2, b2, wg, bg, wa, ba)))
    assert not ref[iso].any()
    err = rel_err(agg, ref)
    _record(f"aggregate_entry_point D={d}", agg_vs_fp64=err)
    assert err < TOL
