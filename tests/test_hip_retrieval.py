"""Retrieval on the GPU (rpg_retrieve_cosine_f32 / ops.retrieve, FeatureMap.retrieve, forward_map(rule=...), relocalize(rule=...))
against the float64 restatement of the rule in retrieval_ref.py.

Exact cases: inputs on which float rounding cannot change the order, so the indices must equal the oracle's.  Random cases: no
tuned tolerance -- with c_ref = max |s32 - s64| the error of the CPU fp32 reference (sklearn on fp32 input) on the same case,
returned sims within 4 c_ref of the float64 similarity of the returned row; position by position the float64 similarity of the
returned row within 8 c_ref of the oracle's row's; rows distinct, allowed and non-increasing up to that margin; at most 25 % of a
case's queries differ from the oracle in any index, which the fp32 CPU reference itself must also satisfy.  The observed figures
are appended as JSON lines to the file RPG_RETRIEVAL_REPORT names, when it is set."""
import json
import os

import numpy as np
import pytest
import torch

import retrieval_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _report(**kw):
    path = os.environ.get("RPG_RETRIEVAL_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(kw) + "\n")


def _run(dev, q, db, ranks, qg=None, dg=None, sims=False, **kw):
    from relpose_gnn_amd import ops
    t = lambda a, dt: None if a is None else torch.as_tensor(np.asarray(a), dtype=dt).to(dev)
    out = ops.retrieve(t(q, torch.float32), t(db, torch.float32), t(ranks, torch.int32), q_group=t(qg, torch.int64),
                       db_group=t(dg, torch.int64), return_sims=sims, **kw)
    return (out[0].cpu().numpy(), out[1].cpu().numpy()) if sims else out.cpu().numpy()


def _topk(g, k):
    return np.tile(np.arange(k, dtype=np.int32), (g, 1))


# ---- 1. exact cases ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["none", "self", "cross"])
@pytest.mark.parametrize("sp", [5, 10])
def test_g10(dev, config, sp):
    from relpose_gnn_amd.retrieval import RetrievalRule
    from test_retrieval_cpu import g10_case
    z = np.load(os.path.join(HERE, "golden", "g10_retrieval.npz"))
    q, db, qg, dg, seed, want = g10_case(z, config, sp)
    n = np.full(q.shape[0], db.shape[0]) if qg is None else R.n_allowed(db.shape[0], qg, dg)
    ranks = RetrievalRule.reference(k=int(z["k"]), sampling_period=sp, seed=seed).ranks(n)
    assert np.array_equal(_run(dev, q, db, ranks, qg, dg), want)


def test_constructed_grid_of_similarities(dev):
    """d_m = a_m q + sqrt(1 - a_m^2) u_m, u_m orthogonal to q, a_m a shuffled grid 1e-3 apart: fp32 error is ~3e-7."""
    rng = np.random.RandomState(2)
    m, d, g = 900, 2048, 5
    q = rng.standard_normal(d)
    q /= np.linalg.norm(q)
    a = rng.permutation(0.05 + 1e-3 * np.arange(m))
    u = rng.standard_normal((m, d))
    u -= np.outer(u @ q, q)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    db = (a[:, None] * q + np.sqrt(1 - a * a)[:, None] * u) * rng.uniform(0.5, 2.0, (m, 1))
    qs = np.stack([q * s for s in (1.0, 0.1, 7.0, 3.0, 0.5)]).astype(np.float32)
    db = db.astype(np.float32)
    ranks = np.stack([np.sort(rng.choice(400, 64, replace=False)).astype(np.int32) for _ in range(g)])
    want = R.retrieve_ref(qs, db, ranks)
    assert np.array_equal(want[0], np.argsort(-a)[ranks[0]])
    assert np.array_equal(_run(dev, qs, db, ranks), want)


@pytest.mark.parametrize("m", [16, 17, 33, 1000, 1003])
def test_duplicate_rows_tie_by_index(dev, m):
    """Bitwise-equal rows get bitwise-equal similarities wherever they sit (first row, last row, across 16-row tiles)."""
    rng = np.random.RandomState(m)
    d = 260
    db = rng.standard_normal((m, d)).astype(np.float32)
    dup = sorted(r for r in {0, 1, 15, 16, m // 2, m - 2, m - 1} if r < m)
    db[dup] = db[0]
    q = np.stack([db[0] + 0.01 * rng.standard_normal(d), rng.standard_normal(d)]).astype(np.float32)
    ranks = _topk(2, min(m, 12))
    nb, s = _run(dev, q, db, ranks, sims=True)
    assert np.array_equal(nb[0], R.retrieve_ref(q, db, ranks)[0])
    assert nb[0, :len(dup)].tolist() == dup and len(set(s[0, :len(dup)].tolist())) == 1
    pos = [int(np.flatnonzero(nb[1] == r)[0]) for r in dup if r in nb[1]]
    assert pos == sorted(pos)


def test_zero_norm_rows_and_queries(dev):
    rng = np.random.RandomState(4)
    db = rng.standard_normal((40, 16)).astype(np.float32)
    db[[3, 20, 39]] = 0
    q = rng.standard_normal((3, 16)).astype(np.float32)
    q[1] = 0
    ranks = _topk(3, 40)
    nb, s = _run(dev, q, db, ranks, sims=True)
    assert np.array_equal(nb, R.retrieve_ref(q, db, ranks))
    assert nb[1].tolist() == list(range(40)) and (s[1] == 0).all()            # zero query: every similarity 0, index order
    for g in (0, 2):
        assert (s[g][np.isin(nb[g], [3, 20, 39])] == 0).all()


def test_nonfinite_rows_and_query(dev):
    rng = np.random.RandomState(5)
    m, d = 50, 32
    db = rng.standard_normal((m, d)).astype(np.float32)
    db[7, 3], db[30, 0], db[49, 31], db[0, 5] = np.nan, np.inf, -np.inf, np.nan
    q = rng.standard_normal((4, d)).astype(np.float32)
    q[1, 2] = np.nan
    q[3, 0] = np.inf
    ranks = _topk(4, m)
    nb, s = _run(dev, q, db, ranks, sims=True)
    assert np.array_equal(nb, R.retrieve_ref(q, db, ranks))
    assert nb[0, -4:].tolist() == [0, 7, 30, 49] and np.isnan(s[0, -4:]).all() and np.isfinite(s[0, :-4]).all()
    assert nb[1].tolist() == list(range(m)) and nb[3].tolist() == list(range(m))      # a non-finite query: index order
    clean = _run(dev, q[[0, 2]], db, ranks[:2])
    assert np.array_equal(clean, nb[[0, 2]])                                          # the other queries are unaffected


def test_exclusion_modes(dev):
    rng = np.random.RandomState(6)
    m, d, g, k = 120, 64, 6, 7
    db = rng.standard_normal((m, d)).astype(np.float32)
    qi = np.array([0, 13, 59, 60, 119, 5])
    q = db[qi]
    rows = np.arange(m)
    ranks = _topk(g, k)
    assert _run(dev, q, db, ranks)[:, 0].tolist() == qi.tolist()                      # no exclusion: itself first
    for qg, dg in ((qi, rows), (qi // 10, rows // 10), (np.array([-1, 1, -1, 6, 11, -1]), rows // 10)):
        nb = _run(dev, q, db, ranks, qg, dg)
        assert np.array_equal(nb, R.retrieve_ref(q, db, ranks, qg, dg))
        for j in range(g):
            assert qg[j] == -1 or not (dg[nb[j]] == qg[j]).any()
    # a query whose whole neighbourhood (the 30 most similar rows) is excluded
    s = R.cosine_f64(q[:1], db)[0]
    dg = np.zeros(m, dtype=np.int64)
    dg[np.argsort(-s)[:30]] = 9
    nb = _run(dev, q[:1], db, ranks[:1], np.array([9]), dg)
    assert np.array_equal(nb, R.retrieve_ref(q[:1], db, ranks[:1], [9], dg)) and nb[0, 0] == np.argsort(-s)[30]


# ---- 2. random cases against float64 -----------------------------------------------------------------------------------------
def _iid(rng, g, m, d):
    return rng.standard_normal((g, d)).astype(np.float32), rng.standard_normal((m, d)).astype(np.float32)


def _trajectory(rng, g, m, d):
    """A random walk through descriptor space, ReLU'd; queries are perturbed copies of database rows."""
    walk = np.cumsum(rng.standard_normal((m, d)) * 0.05, axis=0) + rng.standard_normal(d)
    db = np.maximum(walk, 0).astype(np.float32)
    q = np.maximum(walk[rng.choice(m, g)] + 0.02 * rng.standard_normal((g, d)), 0).astype(np.float32)
    return q, db


@pytest.mark.parametrize("m,d", [(4000, 2048), (1000, 32768), (257, 260), (7, 8)])
@pytest.mark.parametrize("kind", ["iid", "trajectory"])
def test_random_against_float64(dev, m, d, kind):
    from relpose_gnn_amd.retrieval import RetrievalRule
    g = 64
    rng = np.random.RandomState(m + d)
    q, db = (_iid if kind == "iid" else _trajectory)(rng, g, m, d)
    s64 = R.cosine_f64(q, db)
    s32 = R.cosine_f32_cpu(q, db)
    c_ref = float(np.abs(s32.astype(np.float64) - s64).max())
    rules = {"top": _topk(g, min(64, m))}
    if m >= 1000:
        rules["ref5"] = RetrievalRule.reference(k=7, sampling_period=5, seed=m).ranks([m] * g)
        rules["ref10"] = RetrievalRule.reference(k=7, sampling_period=10, seed=m + 1).ranks([m] * g)
    for name, ranks in rules.items():
        want = R.retrieve_ref(q, db, ranks)
        cpu32 = R.retrieve_ref(q, db, ranks, sims=s32)
        nb, sims = _run(dev, q, db, ranks, sims=True)
        rows = np.arange(g)[:, None]
        got64, want64 = s64[rows, nb], s64[rows, want]
        c = float(np.abs(sims.astype(np.float64) - got64).max())
        gap = float(np.abs(got64 - want64).max())
        differ = int((nb != want).any(1).sum())
        differ_cpu = int((cpu32 != want).any(1).sum())
        _report(test="random", kind=kind, m=m, d=d, rule=name, c_ref=c_ref, c=c, gap=gap, queries_differ=differ,
                queries_differ_cpu_fp32=differ_cpu, queries=g)
        print(f"{kind} m={m} d={d} {name}: c_ref={c_ref:.3e} c={c:.3e} gap={gap:.3e} differ={differ}/{g} cpu32={differ_cpu}/{g}")
        assert c <= 4 * c_ref, (c, c_ref)
        assert gap <= 8 * c_ref, (gap, c_ref)
        assert all(len(set(r)) == len(r) for r in nb.tolist()) and nb.min() >= 0 and nb.max() < m
        assert (np.diff(got64, axis=1) <= 8 * c_ref).all()
        assert differ_cpu <= g // 4                                  # the condition holds for the fp32 CPU reference itself
        assert differ <= g // 4


# ---- 3. contract -----------------------------------------------------------------------------------------------------------------
def test_bit_identical_across_calls_workspaces_and_batches(dev):
    from relpose_gnn_amd import _lib, ops
    from relpose_gnn_amd.retrieval import RetrievalRule
    rng = np.random.RandomState(8)
    g, m, d = 40, 1500, 2048
    q, db = _trajectory(rng, g, m, d)
    qt, dbt = torch.from_numpy(q).to(dev), torch.from_numpy(db).to(dev)
    ranks = torch.from_numpy(RetrievalRule.reference(k=7, sampling_period=5, seed=1).ranks([m] * g)).to(dev)
    nb0, s0 = ops.retrieve(qt, dbt, ranks, return_sims=True)
    inv = ops.row_inv_norms(dbt)
    need = int(_lib.lib().rpg_retrieve_workspace_bytes(g, m, d))
    for fill in (0.0, float("nan")):
        ws = torch.full((need // 4 + 1,), fill, dtype=torch.float32, device=dev).view(torch.uint8)
        nb, s = ops.retrieve(qt, dbt, ranks, db_inv_norm=inv, return_sims=True, workspace=ws)
        assert torch.equal(nb, nb0) and torch.equal(s.view(torch.int32), s0.view(torch.int32))
    for j in (0, 1, 17, 39):                                         # a query's result does not depend on its batch
        nb, s = ops.retrieve(qt[j:j + 1], dbt, ranks[j:j + 1], return_sims=True)
        assert torch.equal(nb[0], nb0[j]) and torch.equal(s.view(torch.int32)[0], s0.view(torch.int32)[j])
    nb, s = ops.retrieve(qt[5:22], dbt, ranks[5:22], return_sims=True)
    assert torch.equal(nb, nb0[5:22]) and torch.equal(s.view(torch.int32), s0.view(torch.int32)[5:22])
    with pytest.raises(Exception, match="workspace too small"):
        ops.retrieve(qt, dbt, ranks, workspace=torch.empty(need - 256, dtype=torch.uint8, device=dev))


def test_more_than_64_queries(dev):
    rng = np.random.RandomState(9)
    q, db = _iid(rng, 150, 300, 64)
    ranks = _topk(150, 5)
    assert np.array_equal(_run(dev, q, db, ranks), R.retrieve_ref(q, db, ranks))


def test_bad_ranks_are_counted_and_clamped(dev):
    from relpose_gnn_amd import _lib, ops
    r_max = _lib.lib().rpg_retrieve_max_rank()
    rng = np.random.RandomState(10)
    m = 2 * r_max
    q, db = _iid(rng, 4, m, 16)
    dg2 = np.where(np.arange(m) < 5, 1, 0)                         # query 1 (group 0) is left 5 rows, group 2 excludes nothing
    ranks = np.array([[0, 1, r_max], [0, 4, 5], [2, 1, 3], [-1, 0, r_max - 1]], dtype=np.int32)
    qg = np.array([-1, 0, 2, 2])
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    nb = _run(dev, q, db, ranks, qg, dg2, status=status)
    # (0, 2): >= R_MAX; (1, 2): >= 5 allowed rows; row 2 does not ascend; (3, 0): negative
    assert int(status.item()) == 4
    assert nb.min() >= 0 and nb.max() < m
    fixed = np.array([[0, 1, r_max - 1], [0, 4, 4], [2, 1, 3], [0, 0, r_max - 1]], dtype=np.int32)
    assert np.array_equal(nb, R.retrieve_ref(q, db, fixed, qg, dg2))
    _run(dev, q, db, ranks, qg, dg2, status=status)
    assert int(status.item()) == 8                                  # accumulates
    with pytest.raises(IndexError):
        _run(dev, q, db, ranks, qg, dg2)
    # no allowed row at all: every rank is bad, row 0 keeps the output in range
    status.zero_()
    nb = _run(dev, q[:1], db, _topk(1, 3), np.array([7]), np.full(m, 7), status=status)
    assert int(status.item()) == 3 and nb.tolist() == [[0, 0, 0]]


def test_refuses_misaligned_and_mismatched(dev):
    from relpose_gnn_amd import ops
    q = torch.randn(2, 16, device=dev)
    db = torch.zeros(10 * 16 + 1, device=dev)[1:].view(10, 16)      # 4-byte aligned only
    ranks = torch.tensor(_topk(2, 3)).to(dev)
    with pytest.raises(ValueError, match="bad argument"):
        ops.retrieve(q, db, ranks)
    with pytest.raises(ValueError, match="bad argument"):
        ops.row_inv_norms(db)
    with pytest.raises(ValueError, match="d % 4 == 0"):
        ops.retrieve(torch.randn(2, 6, device=dev), torch.randn(4, 6, device=dev), ranks)
    with pytest.raises(ValueError, match="d % 4 == 0"):
        ops.row_inv_norms(torch.randn(4, 6, device=dev))
    with pytest.raises(ValueError, match="shapes do not agree"):
        ops.retrieve(q, torch.randn(4, 8, device=dev), ranks)
    with pytest.raises(ValueError, match="K <= M"):
        ops.retrieve(q, torch.randn(2, 16, device=dev), ranks)
    with pytest.raises(ValueError, match="both or neither"):
        ops.retrieve(q, torch.randn(4, 16, device=dev), ranks, q_group=torch.zeros(2, dtype=torch.int64, device=dev))


def test_row_inv_norms(dev):
    from relpose_gnn_amd import ops
    x = torch.randn(300, 2048, generator=torch.Generator().manual_seed(3))
    x[5] = 0
    inv = ops.row_inv_norms(x.to(dev)).cpu().double()
    want = 1.0 / x.double().norm(dim=1)
    want[5] = 0
    assert float(((inv - want).abs() / want.clamp_min(1e-30)).max()) < 1e-6 and inv[5] == 0


def test_graph_capture_and_replay(dev):
    from relpose_gnn_amd import _lib, ops
    rng = np.random.RandomState(11)
    g, m, d, k = 8, 500, 256, 7
    q1, db = _iid(rng, g, m, d)
    q2 = rng.standard_normal((g, d)).astype(np.float32)
    qt, dbt = torch.from_numpy(q1).to(dev), torch.from_numpy(db).to(dev)
    ranks = torch.tensor(_topk(g, k)).to(dev)
    inv = ops.row_inv_norms(dbt)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(int(_lib.lib().rpg_retrieve_workspace_bytes(g, m, d)), dtype=torch.uint8, device=dev)
    out = torch.empty((g, k), dtype=torch.int64, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.retrieve(qt, dbt, ranks, db_inv_norm=inv, status=status, workspace=ws, out=out)       # warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.retrieve(qt, dbt, ranks, db_inv_norm=inv, status=status, workspace=ws, out=out)
    qt.copy_(torch.from_numpy(q2))
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), R.retrieve_ref(q2, db, _topk(g, k))) and int(status.item()) == 0


def test_map_past_2_gib(dev):
    """64-bit row offsets: 300,000 rows of 2048 floats are 2.4 GB, past 2 GiB and past 2^29 float4."""
    from relpose_gnn_amd import ops
    m, d = 300000, 2048
    free = torch.cuda.mem_get_info(dev)[0]
    if free < 4 * m * d * 4:
        pytest.skip(f"needs {4 * m * d * 4 >> 30} GiB of free device memory, {free >> 30} GiB free")
    gen = torch.Generator(device=dev).manual_seed(12)
    db = torch.randn((m, d), generator=gen, device=dev)
    hot = [0, 262143, 262144, 262145, m - 1]
    q = db[hot] + 0.05 * torch.randn((len(hot), d), generator=gen, device=dev)
    nb, s = ops.retrieve(q, db, torch.tensor(_topk(len(hot), 3)).to(dev), return_sims=True)
    assert nb[:, 0].tolist() == hot and float(s[:, 0].min()) > 0.99 and float(s[:, 1].max()) < 0.2
    del db
    torch.cuda.empty_cache()


# ---- 4. model level ----------------------------------------------------------------------------------------------------------
def _small(dev, **kw):
    from test_hip_featmap import _small as make
    return make(dev, **kw)[0]


def _images(n, seed):
    import relpose_gnn_amd.synth as S
    return S.synth_images(n, 32, 32, seed=seed)


@pytest.mark.parametrize("g,kw", [(64, {}), (3, {}), (64, {"knn": 4}), (5, {"knn": 4})])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_forward_map_retrieves_what_it_reports(dev, g, kw, precision):
    from relpose_gnn_amd.featmap import FeatureMap
    from relpose_gnn_amd.retrieval import RetrievalRule
    model = _small(dev, **kw)
    model.encoder_dtype = precision
    model.hip_streams = 2                                          # >= 4 graphs: one retrieval per stream slot; 3 graphs: small path
    # query seed 136: on the CPU oracle's features the 64 queries' 30 best similarities are at least 3e-6 apart (the widest of
    # seeds 100..139), so the last bits by which the encoder differs between batch sizes cannot reorder them
    mimgs, q = _images(90, 21).to(dev), _images(g, 136).to(dev)
    fmap = FeatureMap.build(model, mimgs, groups=torch.arange(90) // 10)
    rule = RetrievalRule(k=7, sampling_period=2)
    qg = (torch.arange(g) % 9)
    ab, rel, ei, nb = model.forward_map(q, None, fmap, rule=rule, query_groups=qg)
    model.check_edge_index()
    assert nb.shape == (g, 7) and nb.dtype == torch.int64
    assert not (fmap.groups[nb] == qg.to(dev)[:, None]).any()
    ab2, rel2, ei2 = model.forward_map(q, nb, fmap)
    assert torch.equal(ab, ab2) and torch.equal(rel, rel2) and torch.equal(ei, ei2)
    assert torch.equal(nb, fmap.retrieve(model.encode(q), rule, qg))
    _report(test="forward_map", g=g, knn=kw.get("knn", -1), precision=precision, bit_identical=True)


def test_forward_map_with_external_descriptors(dev):
    from relpose_gnn_amd.featmap import FeatureMap
    from relpose_gnn_amd.retrieval import RetrievalRule
    model = _small(dev)
    rng = np.random.RandomState(13)
    qd, desc = _iid(rng, 64, 90, 128)
    fmap = FeatureMap.build(model, _images(90, 21).to(dev), descriptors=torch.from_numpy(desc))
    # period 2: the 14th survivor of 90 half-dropped positions always exists (period 5 would need the 35th of about 45)
    rule = RetrievalRule.reference(k=7, sampling_period=2, seed=4)
    ranks = RetrievalRule.reference(k=7, sampling_period=2, seed=4).ranks([90] * 64)
    q = _images(64, 23).to(dev)
    ab, rel, ei, nb = model.forward_map(q, None, fmap, rule=rule, query_descriptors=torch.from_numpy(qd).to(dev))
    assert np.array_equal(nb.cpu().numpy(), R.retrieve_ref(qd, desc, ranks))
    ab2, rel2, _ = model.forward_map(q, nb, fmap)
    assert torch.equal(ab, ab2) and torch.equal(rel, rel2)


def test_query_that_is_a_map_image(dev):
    from relpose_gnn_amd.featmap import FeatureMap
    from relpose_gnn_amd.retrieval import RetrievalRule
    model = _small(dev)
    mimgs = _images(60, 31).to(dev)
    fmap = FeatureMap.build(model, mimgs, groups=torch.arange(60))
    rows = torch.tensor([0, 17, 59, 30])
    rule = RetrievalRule(k=5)
    nb = model.forward_map(mimgs[rows], None, fmap, rule=rule)[3]
    assert nb[:, 0].cpu().tolist() == rows.tolist()
    nb = model.forward_map(mimgs[rows], None, fmap, rule=rule, query_groups=rows)[3]
    assert not (nb.cpu() == rows[:, None]).any()


@pytest.mark.parametrize("knn", [-1, 4])
def test_relocalize_with_rule_equals_given_neighbours(dev, knn):
    from relpose_gnn_amd.evaluate import relocalize
    from relpose_gnn_amd.featmap import FeatureMap
    from relpose_gnn_amd.retrieval import RetrievalRule
    model = _small(dev, **({"knn": knn} if knn > 0 else {}))
    gen = torch.Generator().manual_seed(41)
    poses = torch.randn(80, 6, generator=gen) * 0.3
    fmap = FeatureMap.build(model, _images(80, 41).to(dev), poses=poses, groups=torch.arange(80) // 8)
    g = 37                                                         # micro-batches of 16, 16, 5
    q = _images(g, 42)
    targets = torch.randn(g, 6, generator=gen) * 0.3
    qg = torch.arange(g) % 10
    st = {}
    res = relocalize(model, fmap, q, micro_batch=16, targets=targets, stats=st, rule=RetrievalRule(k=7, sampling_period=3),
                     query_groups=qg)
    nb = res.neighbours
    assert nb.shape == (g, 7) and np.array_equal(st["neighbours"], nb)
    assert not (fmap.groups_host.numpy()[nb] == qg.numpy()[:, None]).any()
    given = relocalize(model, fmap, q, torch.from_numpy(nb), micro_batch=16, targets=targets)
    assert np.array_equal(res.pred_poses, given.pred_poses) and np.array_equal(res.targ_poses, given.targ_poses)
    assert np.array_equal(res.t_loss, given.t_loss) and np.array_equal(res.q_loss, given.q_loss)
    on_dev = relocalize(model, fmap, q.to(dev), micro_batch=16, targets=targets, rule=RetrievalRule(k=7, sampling_period=3),
                        query_groups=qg)
    assert np.array_equal(on_dev.pred_poses, res.pred_poses) and np.array_equal(on_dev.neighbours, nb)
