"""The graph-side kernels of csrc/gnn_ops.hip and the composite GNN forward on IRREGULAR graphs, against exact references and against
float64 (tests/graph_sweep_ref.py; the oracle of oracle/posenet_ref.py is the reference throughout).

What the suite did not run before: in-degrees above 8 (a second round of attention_aggregate's 8 waves and of its 8-row mbar
chunk), C that is no multiple of 64, d / 4 that the workgroups of a node do not divide, every remainder of scatter_mean's 4-way
unroll in one launch, more than 1024 nodes through the chunked scans of graph_prepare and knn_compact, the kNN limits (k = 64,
2048 and 2049 nodes), exact distance ties on the GPU, self-loops, repeated edges, edge lists grouped by nothing, isolated nodes,
logits of +-80 and denormal logits, and gather_add2_relu on its own.

Three kinds of check.
  exact      integers, or fp32 in a stated order of IEEE operations: torch.equal.
  float64    the same operation in float64 on the same fp32 inputs, element-wise metric max |y - z| / (|z| + s) (s: the row's
             float64 root-mean-square; for pose_heads sum_k |x_k w_k| + |b|).  c_ref is that figure for the fp32 CPU statement of
             the operation (torch softmax / bmm, F.linear), c_hip the kernel's; asserted: c_hip <= M_KERNEL c_ref.
  composite  rel_err of the HIP poses against the float64 oracle <= M_FWD x rel_err of the fp32 oracle against it, and, unmoved,
             rel_err < 1e-4 against the fp32 oracle.

Margins.  No figures have been recorded on an MI355X yet (profiles/graph_sweep_observed.json does not exist), so both margins stand at
the ceilings reasoned beforehand, not at anything the kernels gave: M_KERNEL = 8 is what a different summation order plus a 1-2 ulp
hardware exp can cost over a correctly rounded fp32 evaluation, M_FWD = 2 is twice the 0.9-1.0 that README.md reports for the
same ratio on fully connected graphs.  Every case prints c_ref, c_hip and their ratio and appends them to the file that
RPG_SWEEP_RECORD names (see _record); once they are in profiles/, the margins come down to twice the worst recorded ratio, and
a ratio above these ceilings is a finding to explain or fix in the kernel, never a margin to adopt.
"""
import json
import os

import pytest
import torch
import torch.nn.functional as F

import graph_sweep_ref as R
from conftest import rel_err

pytestmark = pytest.mark.gpu

# the ceilings of the module docstring (to become twice the worst recorded c_hip / c_ref, resp. e_hip / e_ref, and never more than
# these: a worst ratio above 8 (kernels) or 2 (composite) is a finding, not a margin)
M_KERNEL = 8.0
M_FWD = 2.0
TOL_FP32_ORACLE = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _record(section: str, case: str, figures: dict) -> None:
    """Measured figures: printed, and appended as JSON lines to the file the environment variable RPG_SWEEP_RECORD names, if it
    is set (profiles/graph_sweep_observed.json is put together from such a file by hand)."""
    path = os.environ.get("RPG_SWEEP_RECORD")
    print(section, case, figures)
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"section": section, "case": case, **figures}) + "\n")


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


_GRAPHS = {}


def _graph(n, e):
    if (n, e) not in _GRAPHS:
        _GRAPHS[(n, e)] = R.sweep_graph(n, e)
    return _GRAPHS[(n, e)]


def _ratio(section, case, c_ref, c_hip, margin):
    assert c_ref > 0.0, "the fp32 CPU reference is exact here: the case measures nothing"
    _record(section, case, {"c_ref": c_ref, "c_hip": c_hip, "ratio": c_hip / c_ref})
    assert c_hip <= margin * c_ref, (case, c_ref, c_hip, c_hip / c_ref)


# ----------------------------------------------------------------------------------------------------------------------
# 2. exact checks
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,e", R.SWEEP_GRAPHS)
def test_graph_prepare_irregular(dev, n, e):
    """rpg_graph_prepare on self-loops, repeated edges, shuffled columns, in-degrees 0 .. 40 and trailing isolated nodes;
    N = 1030 takes two chunks of the 1024-lane scan, E = 1000 / 1024 / 2500 one, exactly one and three passes of the edge loops."""
    from relpose_gnn_amd import ops
    ei = _graph(n, e)
    g = ops.graph_prepare(ei.to(dev), n)
    assert int(g["status"].item()) == 0
    rowptr, perm = R.csr(ei, n)
    assert torch.equal(g["perm"].cpu().long(), perm)
    assert torch.equal(g["rowptr"].cpu().long(), rowptr)
    ends = g["ends"].cpu()
    assert torch.equal(ends[0], ei[0]) and torch.equal(ends[1], ei[1])
    assert torch.equal(ends[2], torch.minimum(ei[0], ei[1])) and torch.equal(ends[3], torch.maximum(ei[0], ei[1]))
    loops = ei[0] == ei[1]
    assert bool(loops.any()) and torch.equal(ends[2][loops], ends[3][loops])


def test_graph_prepare_reports_out_of_range_edges_past_one_pass(dev):
    """Two bad end points among 2500 edges (the second and third pass of the edge loops): counted, and absent from the CSR."""
    from relpose_gnn_amd import ops
    n = 1030
    ei = _graph(n, 2500).clone()
    ei[0, 1500], ei[1, 2400] = n, -1
    g = ops.graph_prepare(ei.to(dev), n)
    assert int(g["status"].item()) == 2
    keep = torch.ones(2500, dtype=torch.bool)
    keep[[1500, 2400]] = False
    ids = keep.nonzero().flatten()
    rowptr, perm = R.csr(ei[:, keep], n)
    assert torch.equal(g["rowptr"].cpu().long(), rowptr)
    assert torch.equal(g["perm"].cpu().long()[:2498], ids[perm])
    assert int(g["ends"].max()) < n and int(g["ends"].min()) >= 0


@pytest.mark.parametrize("d", [4, 200, 2048])
@pytest.mark.parametrize("n,e", R.SWEEP_GRAPHS)
def test_scatter_mean_exact_in_ascending_edge_order(dev, n, e, d):
    """rpg_scatter_mean_f32 == the fp32 sum in ascending edge id per target, one division by the in-degree: every remainder of
    the 4-way unroll (in-degrees 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 40) and isolated nodes in one launch; d = 4 is one float4
    column, d = 2048 two 1024-column slabs."""
    from relpose_gnn_amd import ops
    ei = _graph(n, e)
    msg = _rand(ei.shape[1], d, seed=13 + d)
    g = ops.graph_prepare(ei.to(dev), n)
    out = ops.scatter_mean(msg.to(dev), g["rowptr"], g["perm"], n).cpu()
    assert torch.equal(out, R.scatter_mean_ordered(msg, ei, n))
    assert float(out[-2:].abs().max()) == 0.0


@pytest.mark.parametrize("d", [4, 200])
@pytest.mark.parametrize("n,e", R.SWEEP_GRAPHS)
def test_edge_concat_gather_irregular(dev, n, e, d):
    from relpose_gnn_amd import ops
    from oracle.posenet_ref import edge_concat
    ei = _graph(n, e)
    x = _rand(n, d, seed=3)
    assert torch.equal(ops.edge_concat_gather(x.to(dev), ei.to(dev)).cpu(), edge_concat(x, ei))


@pytest.mark.parametrize("d,e", [(4, (1 << 21) + 1001), (64, 5003), (2048, 2500)])
def test_gather_add2_relu_exact(dev, d, e):
    """rpg_gather_add2_relu_f32 == relu((pq[lo][:, :d] + pq[hi][:, d:]) + bias) in fp32 with that association.  At d = 4 the
    launch has more float4 items (2^21 + 1001) than the capped grid has lanes (8192 x 256 = 2^21): the grid strides once, and
    the last pass is ragged."""
    from relpose_gnn_amd import ops
    rows = 1030
    g0 = torch.Generator().manual_seed(17 + d)
    pq, bias = _rand(rows, 2 * d, seed=d), _rand(d, seed=d + 1)
    lo = torch.randint(0, rows, (e,), generator=g0)
    hi = torch.maximum(lo, torch.randint(0, rows, (e,), generator=g0))       # lo <= hi, equal on "self-loops"
    out = ops.gather_add2_relu(pq.to(dev), lo.to(dev), hi.to(dev), bias.to(dev)).cpu()
    ref = R.gather_add2_relu_ref(pq, lo, hi, bias)
    assert torch.equal(out, ref)
    assert bool((ref == 0).any()) and bool((ref > 0).any())
    with pytest.raises(IndexError):
        ops.gather_add2_relu(pq.to(dev), lo[:8].to(dev), (hi[:8] + rows).to(dev), bias.to(dev))
    with pytest.raises(ValueError):
        ops.gather_add2_relu(pq.to(dev), lo[:8].to(dev), hi[:8].to(dev), bias[:-1].to(dev))


def _knn_both(dev, x, k, batch, ref_fn):
    from relpose_gnn_amd import ops
    got = ops.knn_graph(x.to(dev), k, None if batch is None else batch.to(dev)).cpu()
    ref = ref_fn(x, k, batch)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.equal(got, ref)
    return got


def test_knn_duplicate_rows_and_the_node_that_keeps_k_plus_one(dev):
    """Exact ties on the GPU: nodes 2, 5 .. 10 are the same point.  Strict '<' keeps the lower index, so node 10's k + 1 = 4 nearest
    are four of the six copies before it, itself not among them: it keeps 4 neighbours and E > n k (cnt[i] == k + 1 in the
    compaction)."""
    from oracle.posenet_ref import knn_graph
    x = R.integer_features(12, 8, seed=3)
    x[5:11] = x[2]
    ei = _knn_both(dev, x, 3, None, knn_graph)
    assert int(torch.bincount(ei[1], minlength=12)[10]) == 4 and ei.shape[1] > 12 * 3
    assert ei[0][ei[1] == 10].tolist() == [2, 5, 6, 7]


@pytest.mark.parametrize("k", [2, 4])
def test_knn_equidistant_neighbours(dev, k):
    """Nine points on a line, unit spacing: every inner node has its neighbours in equidistant pairs; the lower index comes first."""
    from oracle.posenet_ref import knn_graph
    x = torch.zeros(9, 4)
    x[:, 0] = torch.arange(9) - 4.0
    ei = _knn_both(dev, x, k, None, knn_graph)
    assert ei[0][ei[1] == 4].tolist() == [3, 5, 2, 6][:k]


def test_knn_ragged_batches_cross_the_compaction_chunk(dev):
    """1030 nodes in graphs of 1 .. 10 nodes, k = 4: knn_compact_kernel hands its running offset from the first 1024-node chunk to
    the second; graphs below k + 1 nodes give fewer than k edges per node, integer features give ties."""
    from oracle.posenet_ref import knn_graph
    g0 = torch.Generator().manual_seed(5)
    sizes = []
    while sum(sizes) < 1030:
        sizes.append(min(int(torch.randint(1, 11, (1,), generator=g0)), 1030 - sum(sizes)))
    assert sum(sizes) == 1030
    batch = torch.cat([torch.full((m,), i, dtype=torch.int64) for i, m in enumerate(sizes)])
    x = R.integer_features(1030, 8, seed=6)
    ei = _knn_both(dev, x, 4, batch, knn_graph)
    assert int(ei[1].max()) >= 1024 and ei.shape[1] < 1030 * 4
    assert torch.equal(ei, R.knn_graph_exact(x, 4, batch))


def test_knn_k_64_on_70_nodes(dev):
    """k = KNN_MAX_K: the 65-entry insertion list of knn_candidates_kernel, on integer features with ties."""
    from oracle.posenet_ref import knn_graph
    ei = _knn_both(dev, R.integer_features(70, 4, seed=7), 64, None, knn_graph)
    assert ei.shape[1] >= 70 * 64


def test_knn_one_graph_of_exactly_2048_nodes(dev):
    """KNN_MAX_GRAPH nodes fill the LDS distance row and two chunks of the compaction; 9^4 distinct points among 2048: many ties."""
    x = R.integer_features(2048, 4, seed=8)
    ei = _knn_both(dev, x, 2, None, R.knn_graph_exact)
    assert ei.shape[1] >= 2048 * 2


def test_knn_limits_are_refused(dev):
    from relpose_gnn_amd import ops
    with pytest.raises(ValueError, match="more than 2048 nodes"):
        ops.knn_graph(R.integer_features(2049, 4, seed=9).to(dev), 2)
    with pytest.raises(ValueError):
        ops.knn_graph(R.integer_features(70, 4, seed=7).to(dev), 65)


# ----------------------------------------------------------------------------------------------------------------------
# 3. float64 checks
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("c", [4, 8, 60, 64, 68, 256])
def test_attention_rows_float64(dev, c, regime):
    """rpg_attention_rows_f32 against float64, element-wise, no further from it than M_KERNEL x the fp32 CPU softmax / bmm; finite
    in every regime (logits up to +-80 with both shifts and a constant-theta row; denormal logits)."""
    from relpose_gnn_amd import ops
    gtp = R.attention_inputs(37, c, regime, seed=100 + c)
    z = R.attention_rows_ref(gtp)
    y = ops.attention_rows(gtp.to(dev)).cpu()
    assert bool(torch.isfinite(y).all())
    _ratio("attention_rows", f"C={c} {regime}", R.rowwise_err(R.attention_rows_ref(gtp, torch.float32), z), R.rowwise_err(y, z),
           M_KERNEL)


AGG_SHAPES = [(4, 4), (60, 64), (68, 200), (256, 200), (256, 2048), (8, 2048)]


@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("c,d", AGG_SHAPES)
def test_attention_aggregate_irregular(dev, c, d, regime):
    """rpg_attention_aggregate_f32 on the 37-node irregular graph (in-degrees 0 .. 40).
    mbar: exact -- the fp32 sum in ascending edge id / in-degree, plus the bias (one more fp32 addition) on nodes with an incoming
    edge, zero on isolated nodes.
    ybar: (i) exact against the kernel's own rows -- the same launch on a graph that gives every edge a target of its own yields
    y_e; ybar of an in-degree-1 node IS that row, and every ybar is the documented wave-order sum of them; zero on isolated nodes;
    (ii) against float64, element-wise, no further from it than M_KERNEL x the fp32 CPU statement (softmax / bmm, then the mean
    in ascending edge order).  C = 4: one lane of the min / max pass has data; C = 60, 68: masked lanes; (256, 200): 13 mbar
    columns per workgroup with two dead ones."""
    from relpose_gnn_amd import ops
    n = 37
    ei = _graph(n, None)
    e = ei.shape[1]
    deg = R.in_degrees(ei, n)
    gtp = R.attention_inputs(e, c, regime, seed=200 + c)
    msg, bias = _rand(e, d, seed=10 + d), _rand(d, seed=11)
    gp = ops.graph_prepare(ei.to(dev), n)
    ybar, mbar = ops.attention_aggregate(gtp.to(dev), msg.to(dev), gp["rowptr"], gp["perm"], n)
    ybar, mbar = ybar.cpu(), mbar.cpu()
    assert bool(torch.isfinite(ybar).all())
    # mbar
    mref = R.scatter_mean_ordered(msg, ei, n)
    assert torch.equal(mbar, mref)
    yb2, mb = ops.attention_aggregate(gtp.to(dev), msg.to(dev), gp["rowptr"], gp["perm"], n, bias.to(dev))
    has_in = (deg > 0).unsqueeze(1)
    assert torch.equal(mb.cpu(), torch.where(has_in, mref + bias, torch.zeros_like(mref)))
    assert torch.equal(yb2.cpu(), ybar)
    # ybar against the kernel's own per-edge rows
    own = torch.stack([ei[0], torch.arange(e)])                      # edge i -> a target of its own
    gq = ops.graph_prepare(own.to(dev), e)
    y_e, m_e = ops.attention_aggregate(gtp.to(dev), msg.to(dev), gq["rowptr"], gq["perm"], e)
    y_e = y_e.cpu()
    assert torch.equal(m_e.cpu(), msg)
    rowptr, perm = R.csr(ei, n)
    ones = (deg == 1).nonzero().flatten()
    assert ones.numel() > 0 and torch.equal(ybar[ones], y_e[perm[rowptr[ones]]])
    assert float(ybar[deg == 0].abs().max()) == 0.0 and int((deg == 0).sum()) >= 2
    assert torch.equal(ybar, R.wave_order_mean(y_e, ei, n))
    # ybar (and the rows themselves) against float64
    z_e = R.attention_rows_ref(gtp)
    z = R.scatter_mean_ordered(z_e, ei, n)
    y32 = R.scatter_mean_ordered(R.attention_rows_ref(gtp, torch.float32), ei, n)
    rows = (deg > 0).nonzero().flatten()
    _ratio("attention_aggregate_ybar", f"C={c} d={d} {regime}", R.rowwise_err(y32, z, rows), R.rowwise_err(ybar, z, rows), M_KERNEL)
    _ratio("attention_aggregate_rows", f"C={c} d={d} {regime}", R.rowwise_err(R.attention_rows_ref(gtp, torch.float32), z_e),
           R.rowwise_err(y_e, z_e), M_KERNEL)


def test_attention_aggregate_refuses_513_mbar_columns(dev):
    """(C, d) = (8, 2052): one workgroup per node would need 513 mbar columns, one more than it has threads."""
    from relpose_gnn_amd import ops
    n, ei = 37, _graph(37, None)
    gp = ops.graph_prepare(ei.to(dev), n)
    gtp, msg = _rand(ei.shape[1], 24, seed=1), _rand(ei.shape[1], 2052, seed=2)
    with pytest.raises(ValueError):
        ops.attention_aggregate(gtp.to(dev), msg.to(dev), gp["rowptr"], gp["perm"], n)
    ops.attention_aggregate(gtp.to(dev), msg[:, :2048].contiguous().to(dev), gp["rowptr"], gp["perm"], n)     # 512 are served


@pytest.mark.parametrize("r", [1, 5, 61])
@pytest.mark.parametrize("d", [4, 252, 2048])
def test_pose_heads_float64(dev, d, r):
    """rpg_pose_heads_f32 against float64 relative to sum |x_k w_k| + |b|, no further than M_KERNEL x F.linear in fp32.  d = 4: one
    float4 for 64 lanes; 252: 63 float4s, a ragged pass; R = 1, 5: fewer rows than the workgroup's 4 waves; 61: a ragged last
    workgroup."""
    from relpose_gnn_amd import ops
    x, w6, b6 = _rand(r, d, seed=2 + d), _rand(6, d, seed=3, scale=d ** -0.5), _rand(6, seed=4)
    y = ops.pose_heads(x.to(dev), w6.to(dev), b6.to(dev)).cpu()
    assert y.shape == (r, 6) and bool(torch.isfinite(y).all())
    c_ref = R.pose_heads_err(F.linear(x, w6, b6), x, w6, b6)
    c_hip = R.pose_heads_err(y, x, w6, b6)
    if c_ref == 0.0:                   # d = 4, a few rows: four products and a bias can round to the float64 value's nearest fp32
        c_ref = 2.0 ** -25             # then the bar is half an ulp of the element's scale (|z| <= s: (|z| + s) 2^-25 <= |z| ulp / 2 .. ulp)
    _ratio("pose_heads", f"d={d} R={r}", c_ref, c_hip, M_KERNEL)


# ----------------------------------------------------------------------------------------------------------------------
# 4. the composite forward
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fwd(dev):
    """The small model, the five-graph irregular batch (grouped by graph, and the same columns shuffled across graphs), and the
    oracle's poses for it in fp32 and in float64 -- computed once for the tests below."""
    from relpose_gnn_amd.graph import Batch, Data
    from relpose_gnn_amd.posenet import PoseNetX_R2
    from relpose_gnn_amd.resnet import ResNet
    m = PoseNetX_R2(ResNet(R.FWD_BLOCKS, R.FWD_PLANES), droprate=0.0, pretrained=False, feat_dim=R.FWD_D, edge_feat_dim=R.FWD_D,
                    node_dim=R.FWD_D, input_img_height=R.FWD_H, use_gnn=True, knn=-1, use_AP=True, gnn_recursion=2)
    sd = R.forward_state_dict()
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    x, local, ei, batch = R.forward_batch()
    off, graphs = 0, []
    for n, e in zip(R.FORWARD_SIZES, local):
        graphs.append(Data(x=x[off:off + n], edge_index=e))
        off += n
    grouped = Batch.from_data_list(graphs)
    assert torch.equal(grouped.edge_index, ei)
    perm = torch.randperm(ei.shape[1], generator=torch.Generator().manual_seed(3))
    shuffled = Batch(x=x, edge_index=ei[:, perm].contiguous(), batch=batch)
    a32, r32, _ = R.oracle_forward(sd, x, ei, torch.float32)
    a64, r64, _ = R.oracle_forward(sd, x, ei, torch.float64)
    return {"m": m, "sd": sd, "x": x, "ei": ei, "perm": perm, "grouped": grouped.to(dev), "shuffled": shuffled.to(dev),
            "o32": (a32, r32), "o64": (a64, r64)}


def _against_float64(case, got, o32, o64):
    for name, y, y32, z in zip(("abs", "rel"), got, o32, o64):
        e_ref, e_hip, e_32 = rel_err(y32, z), rel_err(y, z), rel_err(y, y32)
        _record("composite_forward", f"{case} {name}_pose", {"e_ref": e_ref, "e_hip": e_hip, "ratio": e_hip / e_ref,
                                                             "vs_fp32_oracle": e_32})
        assert e_hip <= M_FWD * e_ref, (case, name, e_ref, e_hip)
        assert e_32 < TOL_FP32_ORACLE, (case, name, e_32)


@pytest.mark.parametrize("fuse_agg", [1, 0])
@pytest.mark.parametrize("split", [1, 0])
def test_forward_irregular_batch_all_formulations(dev, fwd, split, fuse_agg):
    """All four formulations of gnn_forward_impl on graphs of 3, 8, 12, 1 and 9 nodes with in-degrees 0 .. 11, self-loops, repeated
    edges, isolated nodes and a graph without any edge: as close to the float64 oracle as the fp32 oracle is (x M_FWD), and within
    1e-4 of the fp32 oracle."""
    from relpose_gnn_amd import ops
    m = fwd["m"]
    m.hip_streams = 1
    with ops.tuned({ops.TUNE_GNN_SPLIT: split, ops.TUNE_GNN_FUSE_AGG: fuse_agg}):
        a, r, ei = m(fwd["grouped"])
        got = (a.cpu(), r.cpu())
    m.check_edge_index()
    assert torch.equal(ei.cpu(), fwd["ei"]) and bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())
    _against_float64(f"split={split} fuse_agg={fuse_agg}", got, fwd["o32"], fwd["o64"])


def test_forward_irregular_batch_two_streams_equal_one(dev, fwd):
    """The grouped batch cut at a graph boundary over two streams (graphs 0-1 | 2-4; the edge-less graph sits inside a part) gives
    the poses of one stream, to the standard of test_multi_stream_equals_single_stream."""
    m = fwd["m"]
    try:
        m.hip_streams = 1
        a1, r1, _ = m(fwd["grouped"])
        m.hip_streams = 2
        parts = m._partition(fwd["grouped"], 33, fwd["ei"].shape[1])
        assert parts is not None and len(parts) == 2 and parts[0][1] == 11
        a2, r2, _ = m(fwd["grouped"])
    finally:
        m.hip_streams = 1
    m.check_edge_index()
    assert rel_err(a2.cpu(), a1.cpu()) < 1e-5 and rel_err(r2.cpu(), r1.cpu()) < 1e-5


def test_forward_edges_shuffled_across_graphs(dev, fwd):
    """The same edges in an order grouped by nothing: no contiguous cut exists, so two streams fall back to one, and the poses are
    the grouped batch's with the edge rows permuted (only the summation order inside a target changes: 1e-5, as above)."""
    m = fwd["m"]
    try:
        m.hip_streams = 2
        assert m._partition(fwd["shuffled"], 33, fwd["ei"].shape[1]) is None
        a_s, r_s, ei_s = m(fwd["shuffled"])
        m.hip_streams = 1
        a_g, r_g, _ = m(fwd["grouped"])
    finally:
        m.hip_streams = 1
    m.check_edge_index()
    assert torch.equal(ei_s.cpu(), fwd["ei"][:, fwd["perm"]])
    assert rel_err(a_s.cpu(), a_g.cpu()) < 1e-5 and rel_err(r_s.cpu(), r_g.cpu()[fwd["perm"]]) < 1e-5
    _against_float64("shuffled", (a_s.cpu(), r_s.cpu()), (fwd["o32"][0], fwd["o32"][1][fwd["perm"]]),
                     (fwd["o64"][0], fwd["o64"][1][fwd["perm"]]))


def test_forward_knn_9_on_12_node_graphs(dev, fwd):
    """knn = 9 through the model-built graph: every node of two 12-node graphs has in-degree 9 (a second round of the 8 waves)."""
    import relpose_gnn_amd.synth as S
    from relpose_gnn_amd.graph import fc_batch
    m = fwd["m"]
    x = S.synth_images(24, R.FWD_H, R.FWD_W, seed=77)
    data = fc_batch(x, 12)
    try:
        m.knn = 9
        a, r, ei = m(data.to(dev))
    finally:
        m.knn = -1
    o32 = R.oracle_forward(fwd["sd"], x, data.edge_index, torch.float32, knn=9, batch=data.batch)
    o64 = R.oracle_forward(fwd["sd"], x, data.edge_index, torch.float64, knn=9, batch=data.batch)
    assert ei.shape == (2, 24 * 9) and torch.equal(ei.cpu(), o32[2]) and torch.equal(o64[2], o32[2])
    assert torch.equal(torch.bincount(ei[1].cpu()), torch.full((24,), 9))
    _against_float64("knn=9", (a.cpu(), r.cpu()), o32[:2], o64[:2])
