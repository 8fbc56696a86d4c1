"""The retrieval kernels (csrc/retrieve.hip) over the sweep of tests/retrieval_sweep_ref.py: every case goes through the C ABI with
each array between moats and a workspace of exactly the bytes the size function returns, once pre-filled with NaN and once with
zeros.  Lattice and integer cases are held to the integer oracle exactly; float cases to the a-priori bound of the helper's
docstring (derived, not measured: a ratio above 1 is a finding to explain from the code); gate, scope and vote cases also to the
existing pose_gate_ref / scene_ref.oracle / scene_vote_ref.oracle.  tests/test_retrieval_sweep_cpu.py shows that each of these
checks fails under the planted defects.  The observed figures are appended as JSON lines to the file RPG_RETRIEVAL_SWEEP_REPORT
names, when it is set (profiles/retrieval_sweep_observed.json is such a run).

Where each path of the sweep runs: column-slice plans -- plan_* and float_* (a last slice of one 4-column block: m100_d6340 and
m1488_d6340; 9 + 8 blocks: m40_d1028; the slice count changing with m: m1488 / m1489); query tiling -- queries_g*; radix select
over several row digits -- select_m257* and up (digit 8), select_m65537*, scope_*, vote_* (digit 16), with lo > 0 in scope_*;
ties that reach the row digits -- the zero query and column 1 of every select_* case; the gate sweep's unroll lanes and second
outer step -- gate_m3073* and up, scope_groups_gate with lo = 557."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import pose_gate_ref as G
import retrieval_ref as R
import retrieval_sweep_ref as S
import scene_ref as SR
import scene_vote_ref as SV

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _report(**kw):
    path = os.environ.get("RPG_RETRIEVAL_SWEEP_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(kw) + "\n")


def _plan_of(c):
    ns, bps, nq, chunks = c.plan
    return {"g": c.g, "k": c.k, "m": c.m, "d": c.d, "nsplit": ns, "blocks_per_split": bps, "nq": nq, "chunks": chunks}


def _same_bits(a: S.Result, b: S.Result) -> bool:
    eq = lambda x, y: (x is None and y is None) or np.array_equal(x, y)
    return (eq(a.nbrs, b.nbrs) and eq(a.sims.view(np.uint32), b.sims.view(np.uint32)) and a.status == b.status and
            eq(a.gate_info, b.gate_info) and eq(a.scene_info, b.scene_info) and eq(a.q_scene, b.q_scene))


def _both_fills(c):
    """The case with the workspace pre-filled with NaN and with zeros: nothing found by the harness, identical bits."""
    dev = _dev()
    a, b = S.launch(c, dev, S.NAN_WORD), S.launch(c, dev, S.ZERO_WORD)
    assert a.findings == [] and b.findings == [], (c.id, a.findings, b.findings)
    assert _same_bits(a, b), (c.id, "the result depends on what the workspace held")
    return a


# ---- the plan ------------------------------------------------------------------------------------------------------------------------
def test_plan_and_workspace_sizes_equal_the_restatement():
    from relpose_gnn_amd import _lib
    lib = _lib.lib()
    out = (C.c_int32 * 4)()
    specs = [s for v in S.EXACT_LISTS.values() for s in v] + S.FLOAT_CASES
    for spec in specs:
        c = S.build(spec)
        assert lib.rpg_retrieve_plan(c.g, c.m, c.d, out) == 0 and tuple(out) == c.plan, spec.id
        assert int(lib.rpg_retrieve_workspace_bytes(c.g, c.m, c.d)) == S.ws_layout(c.g, c.m, c.d)["total"], spec.id
        assert int(lib.rpg_retrieve_elect_workspace_bytes(c.g, c.m, c.d)) == S.elect_layout(c.g, c.m, c.d)["total"], spec.id
    for (m, d), want in S.PLAN_WANT.items():
        assert lib.rpg_retrieve_plan(1, m, d, out) == 0 and tuple(out)[:2] == want, (m, d)


# ---- lattice and integer cases: exact -----------------------------------------------------------------------------------------------
EXACT = [s for name in ("plan", "tile", "queries", "select") for s in S.EXACT_LISTS[name]]


@pytest.mark.parametrize("spec", EXACT, ids=[s.id for s in EXACT])
def test_exact_case_equals_the_integer_oracle(spec):
    c = S.build(spec)
    res = _both_fills(c)
    bad = S.check_exact(c, res)
    _report(case=spec.id, why=spec.why, kind=c.kind, exact=True, passed=not bad, live_digits=list(S.live_digits(0, c.m)), **_plan_of(c))
    assert bad == [], (spec.id, spec.why, bad)


# ---- gate, scope and vote cases: the integer oracle and the existing references ------------------------------------------------------
def _gate_of(c, dev, rows=None):
    if c.gate is None:
        return None
    prior = c.gate["prior"] if rows is None else c.gate["prior"][rows]
    return (torch.from_numpy(c.gate["db_gate"]).to(dev), torch.from_numpy(np.ascontiguousarray(prior)).to(dev), float(c.gate["r2"]),
            0.0, False)


@pytest.mark.parametrize("spec", S.GATE_CASES, ids=[s.id for s in S.GATE_CASES])
def test_gate_case(spec):
    c = S.build(spec)
    res = _both_fills(c)
    want = S.oracle(c)
    bad = S.check_exact(c, res, want)
    _report(case=spec.id, why=spec.why, kind=c.kind, exact=True, passed=not bad, gate_states=want.gate_info[:, 0].tolist(),
            **_plan_of(c))
    assert bad == [], (spec.id, spec.why, bad)
    # pose_gate_ref: the decision from the gate's own arithmetic, then the float64 rule over the rows it leaves
    info, used = G.gated_rows(c.gate["db_gate"], c.gate["prior"], c.gate["r2"], None, c.ranks, c.q_group, c.db_group)
    assert np.array_equal(res.gate_info, info), spec.id
    sims = np.where(c.nonfinite, np.nan, c.score.astype(np.float64))
    for j in range(c.g):
        order = R.ranking(sims[j], used[j])
        assert np.array_equal(res.nbrs[j], order[S.clamp_ranks(c.ranks[j], int(used[j].sum()))[0]]), (spec.id, j)


SCOPED = S.SCOPE_CASES + S.VOTE_CASES


@pytest.mark.parametrize("spec", SCOPED, ids=[s.id for s in SCOPED])
def test_scope_and_vote_case_equals_the_integer_oracle(spec):
    c = S.build(spec)
    res = _both_fills(c)
    want = S.oracle(c)
    bad = S.check_exact(c, res, want)
    _report(case=spec.id, why=spec.why, kind=c.kind, exact=True, passed=not bad, vote_top=c.vote_top,
            scenes=None if want.q_scene is None else want.q_scene.tolist(), status=want.status, **_plan_of(c))
    assert bad == [], (spec.id, spec.why, bad)


@pytest.mark.parametrize("spec", S.ATLAS_LATTICE_CASES, ids=[s.id for s in S.ATLAS_LATTICE_CASES])
def test_atlas_on_lattice_rows_equals_both_oracles(spec):
    """Lattice rows carry their own norms, so scene_ref.oracle and scene_vote_ref.oracle -- the plain entry with emulated groups --
    rank them too: neighbours, the bits of the sims, gate_info, scenes and status all agree, and with the integer oracle."""
    dev = _dev()
    c = S.build(spec)
    res = _both_fills(c)
    want = S.oracle(c)
    bad = S.check_exact(c, res, want)
    _report(case=spec.id, why=spec.why, kind=c.kind, exact=True, passed=not bad, vote_top=c.vote_top, status=want.status, **_plan_of(c))
    assert bad == [], (spec.id, spec.why, bad)
    q, db, ranks = (torch.from_numpy(x).to(dev) for x in (c.q, c.db, c.ranks))
    bits = lambda t: t.numpy().view(np.uint32)
    if c.kind == "scoped":
        ok = np.flatnonzero((c.q_scene >= 0) & (c.q_scene < len(S.ATLAS_SIZES)))
        ix = torch.from_numpy(ok).to(dev)
        nb, sims, info, status = SR.oracle(dev, q[ix].contiguous(), db, ranks[ix].contiguous(), S.ATLAS_SIZES, c.q_scene[ok].tolist(),
                                           c.q_group[ok].tolist(), c.db_group, _gate_of(c, dev, ok))
        assert np.array_equal(res.nbrs[ok], nb.numpy()) and np.array_equal(res.sims[ok].view(np.uint32), bits(sims))
        assert np.array_equal(res.gate_info[ok], info.numpy()) and res.status == status + (c.g - len(ok))
    else:
        held = None if c.mode == S.ELECT_ALL else c.q_scene
        nb, sims, info, status, scenes, sinfo = SV.oracle(dev, q, db, ranks, S.ATLAS_SIZES, c.vote_top,
                                                          None if c.q_group is None else c.q_group.tolist(), c.db_group,
                                                          _gate_of(c, dev), held)
        assert np.array_equal(res.q_scene, scenes.numpy()) and np.array_equal(res.scene_info, sinfo.numpy())
        assert np.array_equal(res.nbrs, nb.numpy()) and np.array_equal(res.sims.view(np.uint32), bits(sims))
        assert res.status == status and (info is None or np.array_equal(res.gate_info, info.numpy()))


# ---- float cases: the a-priori bound ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", S.FLOAT_CASES, ids=[s.id for s in S.FLOAT_CASES])
def test_float_case_within_the_a_priori_bound(spec):
    c = S.build(spec)
    res = _both_fills(c)
    bad, fig = S.check_float(c, res)
    l_dot, l_n = S.chain_lengths(c.m, c.d)
    _report(case=spec.id, why=spec.why, kind=c.kind, exact=False, passed=not bad, l_dot=l_dot, l_norm=l_n, **fig, **_plan_of(c))
    print(spec.id, fig)
    assert bad == [], (spec.id, spec.why, bad, fig)


# ---- invariance: the bits of a similarity depend on the two rows and on (m, d) alone ------------------------------------------------
def _pair_bits(c, res):
    """{(query, row): bits of the similarity} of every returned pair."""
    b = res.sims.view(np.uint32)
    return {(j, int(res.nbrs[j, i])): int(b[j, i]) for j in range(c.g) for i in range(c.k)}


def _all_ranks_case(q, db, window=None):
    """Every row of a map of at most 64 rows -- or of a 64-row window that groups cut out of a larger one -- at its rank."""
    m = db.shape[0]
    k = min(m, 64) if window is None else len(window)
    c = S.Case("", "", "plain", q, db, np.tile(np.arange(k, dtype=np.int32), (q.shape[0], 1)))
    if window is not None:
        c.db_group = np.ones(m, dtype=np.int64)
        c.db_group[window] = 0
        c.q_group = np.ones(q.shape[0], dtype=np.int64)
    return c


@pytest.mark.parametrize("m,d", [(33, 64), (40, 1028), (64, 6340), (1489, 6340)])
def test_bits_do_not_depend_on_where_a_row_sits(m, d):
    rng = np.random.RandomState(m + d)
    g = 5
    q, db = rng.standard_normal((g, d)).astype(np.float32), rng.standard_normal((m, d)).astype(np.float32)
    window = None if m <= 64 else np.sort(rng.choice(m, 64, replace=False))
    base = _all_ranks_case(q, db, window)
    want = _pair_bits(base, _both_fills(base))
    assert len(want) == g * base.k
    for seed in range(2):
        perm = np.random.RandomState(seed).permutation(m)              # row perm[i] of db sits at i
        where = np.argsort(perm)                                       # row r of db sits at where[r]
        c = _all_ranks_case(q, np.ascontiguousarray(db[perm]), None if window is None else np.sort(where[window]))
        got = {(j, int(perm[r])): b for (j, r), b in _pair_bits(c, _both_fills(c)).items()}
        assert got == want, (m, d, seed)


@pytest.mark.parametrize("m,d", [(40, 260), (64, 1028)])
def test_bits_do_not_depend_on_the_batch(m, d):
    rng = np.random.RandomState(7 * m + d)
    q, db = rng.standard_normal((max(S.QUERY_G), d)).astype(np.float32), rng.standard_normal((m, d)).astype(np.float32)
    full = _all_ranks_case(q, db)
    res = _both_fills(full)
    want = _pair_bits(full, res)
    for g in S.QUERY_G:
        c = _all_ranks_case(np.ascontiguousarray(q[:g]), db)
        part = _both_fills(c)
        assert np.array_equal(part.nbrs, res.nbrs[:g]), (m, d, g)
        assert _pair_bits(c, part) == {kv: b for kv, b in want.items() if kv[0] < g}, (m, d, g)
    for j in (0, 16, 63, 64, 128):                                     # and a query alone, from every tile and chunk
        c = _all_ranks_case(np.ascontiguousarray(q[j:j + 1]), db)
        got = {(j, r): b for (_, r), b in _pair_bits(c, _both_fills(c)).items()}
        assert got == {kv: b for kv, b in want.items() if kv[0] == j}, (m, d, j)
