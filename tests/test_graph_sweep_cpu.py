"""CPU checks of what tests/test_hip_graph_sweep.py stands on (tests/graph_sweep_ref.py): the irregular-graph generator covers what
it claims, the exact and float64 references agree with the oracle's statements of the same operations, and the oracle runs in
float64.  No GPU, no library."""
import pytest
import torch
import torch.nn.functional as F

import graph_sweep_ref as R
from conftest import rel_err
from oracle import posenet_ref as O


@pytest.mark.parametrize("n,e", R.SWEEP_GRAPHS)
def test_generator_covers_what_it_claims(n, e):
    ei = R.sweep_graph(n, e)
    assert ei.dtype == torch.int64 and ei.shape[0] == 2 and ei.is_contiguous()
    if e is not None:
        assert ei.shape[1] == e
    deg = R.in_degrees(ei, n)
    assert set(deg.tolist()) <= set(R.IN_DEGREES)
    if n - 2 >= len(R.IN_DEGREES):
        assert set(deg.tolist()) == set(R.IN_DEGREES)                          # every in-degree class occurs
    assert bool((ei[0] == ei[1]).any()) and R.has_repeat(ei, n)                 # a self-loop, a repeated edge
    assert int(ei.max()) < n - 2 and int(ei.min()) >= 0                         # two trailing nodes without any edge
    assert torch.equal(ei, R.sweep_graph(n, e))                                 # deterministic per seed
    if ei.shape[1] > 40:
        assert bool((ei[1][1:] < ei[1][:-1]).any()) and bool((ei[0][1:] < ei[0][:-1]).any())   # grouped by neither end


def test_generator_sizes_hit_the_passes_of_graph_prepare():
    sizes = [(n, R.sweep_graph(n, e).shape[1]) for n, e in R.SWEEP_GRAPHS]
    assert {n for n, _ in sizes} == {3, 37, 1030}
    assert any(e < 1024 for _, e in sizes) and any(e == 1024 for _, e in sizes) and any(e > 2048 for _, e in sizes)
    assert dict(sizes)[37] < 1024
    assert not torch.equal(R.irregular_edges(37, 7), R.irregular_edges(37, 8))  # the seed matters


def test_forward_batch_is_what_the_composite_test_needs():
    x, local, ei, batch = R.forward_batch()
    assert tuple(e.shape[1] > 0 for e in local) == (True, True, True, False, True)      # the one-node graph has no edge
    assert x.shape[0] == sum(R.FORWARD_SIZES) == batch.numel()
    deg = R.in_degrees(ei, x.shape[0])
    assert int(deg[11:23].max()) == 11 and int(deg[24:].max()) == 9              # inside the 12- and the 9-node graph
    assert int((deg == 0).sum()) >= 3                                            # isolated nodes (one is the one-node graph)
    assert bool((ei[0] == ei[1]).any()) and R.has_repeat(ei, x.shape[0])
    assert torch.equal(batch[ei[0]], batch[ei[1]])                               # no edge leaves its graph
    gid = batch[ei[0]]
    assert bool((gid[1:] >= gid[:-1]).all())                                     # grouped by graph


def test_scatter_mean_ordered_is_the_sequential_sum():
    n, e = 37, None
    ei = R.sweep_graph(n, e)
    msg = torch.randn(ei.shape[1], 8, generator=torch.Generator().manual_seed(1))
    got = R.scatter_mean_ordered(msg, ei, n)
    ref = torch.zeros(n, 8)
    for v in range(n):                                       # the definition, one scalar row addition at a time
        ids = (ei[1] == v).nonzero().flatten().tolist()
        acc = torch.zeros(8)
        for i in ids:
            acc = acc + msg[i]
        ref[v] = acc / max(len(ids), 1)
    assert torch.equal(got, ref)
    assert float(got[-2:].abs().max()) == 0.0
    # and, in float64, the oracle's index_add_ statement up to its summation order
    m64 = msg.double()
    assert rel_err(R.scatter_mean_ordered(m64, ei, n), O.scatter_mean(m64, ei[1], n)) < 1e-14


def test_gather_add2_relu_ref_is_proj_edge():
    g = torch.Generator().manual_seed(2)
    n, d = 37, 16
    ei = R.sweep_graph(n, None)
    x = torch.randn(n, d, generator=g, dtype=torch.float64)
    w, b = torch.randn(d, 2 * d, generator=g, dtype=torch.float64), torch.randn(d, generator=g, dtype=torch.float64)
    pq = torch.cat([x @ w[:, :d].t(), x @ w[:, d:].t()], 1)
    lo, hi = torch.minimum(ei[0], ei[1]), torch.maximum(ei[0], ei[1])
    ref = F.relu(F.linear(O.edge_concat(x, ei), w, b))
    assert rel_err(R.gather_add2_relu_ref(pq, lo, hi, b), ref) < 1e-13


def _knn_small_cases():
    dup = R.integer_features(12, 8, seed=3)
    dup[5:11] = dup[2]                                       # nodes 2, 5 .. 10 identical: node 10 has six copies before it
    line = torch.zeros(9, 4)
    line[:, 0] = torch.arange(9) - 4.0                       # equidistant neighbours on both sides of every inner node
    ragged = R.integer_features(30, 4, seed=4)
    sizes = [1, 2, 3, 10, 4, 5, 1, 4]
    batch = torch.cat([torch.full((m,), i, dtype=torch.int64) for i, m in enumerate(sizes)])
    return [("dup", dup, 3, None), ("line", line, 2, None), ("line4", line, 4, None), ("ragged", ragged, 4, batch)]


@pytest.mark.parametrize("case", _knn_small_cases(), ids=lambda c: c[0])
def test_knn_graph_exact_is_the_oracle(case):
    _, x, k, batch = case
    assert torch.equal(R.knn_graph_exact(x, k, batch), O.knn_graph(x, k, batch))


def test_knn_duplicates_keep_k_plus_one_neighbours():
    _, x, k, _ = _knn_small_cases()[0]
    ei = O.knn_graph(x, k)
    cnt = torch.bincount(ei[1], minlength=x.shape[0])
    assert int(cnt[10]) == k + 1 and ei.shape[1] > x.shape[0] * k      # more than k copies precede node 10: self is not among its k + 1


def test_float64_references_and_metric():
    gtp = R.attention_inputs(9, 8, "normal", seed=1)
    z = R.attention_rows_ref(gtp)
    assert z.dtype == torch.float64
    g, th, ph = (gtp[:, i * 8:(i + 1) * 8].double() for i in range(3))
    for r in (0, 8):                                         # the definition, row by row: y_i = sum_j softmax_j(phi_i theta_j) g_j
        a = torch.softmax(ph[r][:, None] * th[r][None, :], dim=1)
        assert torch.allclose(z[r], a @ g[r], rtol=1e-14, atol=0)
    assert R.rowwise_err(R.attention_rows_ref(gtp, torch.float32), z) < 1e-5
    bad = z.clone()
    i = int(z[3].abs().argmin())
    bad[3, i] += 1e-3 * float(z[3].pow(2).mean().sqrt())    # a small element off by 1e-3 of the row's size
    assert R.rowwise_err(bad, z) > 4e-4
    x, w6, b6 = torch.randn(5, 12), torch.randn(6, 12), torch.randn(6)
    assert R.pose_heads_err(F.linear(x, w6, b6), x, w6, b6) < 1e-6
    assert R.pose_heads_err(F.linear(x, w6, b6) + 1e-3, x, w6, b6) > 1e-5


@pytest.mark.parametrize("regime", R.REGIMES)
def test_attention_regimes(regime):
    c = 8
    gtp = R.attention_inputs(64, c, regime, seed=2)
    th, ph = gtp[:, c:2 * c].double(), gtp[:, 2 * c:].double()
    top = float((ph.abs().max(1).values * th.abs().max(1).values).max())
    if regime == "large":
        assert 40 < top <= 80.001 and abs(float(th.abs().max() * ph.abs().max()) - 80) < 1e-3
        assert float(gtp[0, c:2 * c].max()) == float(gtp[0, c:2 * c].min())    # max theta == min theta in row 0
        assert bool((ph > 0).any()) and bool((ph < 0).any())
    elif regime == "tiny":
        assert top < 1e-37                                    # every logit below the smallest normal fp32
    assert bool(torch.isfinite(R.attention_rows_ref(gtp)).all())


def test_oracle_runs_in_float64_and_agrees_with_its_fp32_self():
    x, _, ei, _ = R.forward_batch()
    sd = R.forward_state_dict()
    a64, r64, _ = R.oracle_forward(sd, x, ei, torch.float64)
    a32, r32, _ = R.oracle_forward(sd, x, ei, torch.float32)
    assert a64.dtype == torch.float64 and r64.dtype == torch.float64 and a32.dtype == torch.float32
    assert a64.shape == (33, 6) and r64.shape == (ei.shape[1], 6)
    assert rel_err(a32, a64) < 1e-4 and rel_err(r32, r64) < 1e-4
