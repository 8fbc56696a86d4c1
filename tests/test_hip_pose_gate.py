"""The pose gate of the selection kernel (rpg_retrieve_cosine_gated_f32 / ops.retrieve_gated) on the GPU.

The yardstick is the existing kernel: a gated call must return the neighbours AND the similarities (torch.equal) of
``ops.retrieve`` run per query with ``q_group = 1`` and ``db_group = where(reference row set, 0, 1)``, the row set coming from
tests/pose_gate_ref.py (gate AND groups when gated, the groups alone in states 1 and 2).  Both paths rank the same similarity
bits from the same dot kernel, so no tolerance is involved; ``gate_info`` and the bad-rank count must equal the reference's."""
import numpy as np
import pytest
import torch

import pose_gate_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _unit(a):
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


def _scene(m, d, g, seed):
    """Descriptors, map gate rows in a 10-unit box, and per query a prior: NaN (state 1), a map row's own pose (inside rows
    around it), a pose far outside the box (nothing inside), in turn."""
    rng = np.random.RandomState(seed)
    db = rng.standard_normal((m, d)).astype(np.float32)
    q = rng.standard_normal((g, d)).astype(np.float32)
    gate_rows = np.concatenate([rng.uniform(-5, 5, (m, 3)), _unit(rng.standard_normal((m, 4)))], 1)
    prior = gate_rows[rng.randint(0, m, g)].copy()
    prior[:, :3] += rng.standard_normal((g, 3)) * 0.1
    kind = (np.arange(g) + seed) % 4
    prior[kind == 1, rng.randint(0, 7)] = np.nan
    prior[kind == 2, :3] += 1e3
    return q, db, gate_rows, prior


def _gated(dev, q, db, ranks, gate_rows, prior, r2, cos_half, qg=None, dg=None):
    from relpose_gnn_amd import ops
    t = lambda a, dt: None if a is None else torch.as_tensor(np.asarray(a), dtype=dt).to(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    nb, sims, info = ops.retrieve_gated(t(q, torch.float32), t(db, torch.float32), t(ranks, torch.int32), t(gate_rows, torch.float64),
                                        t(prior, torch.float64), r2, 0.0 if cos_half is None else cos_half, cos_half is not None,
                                        q_group=t(qg, torch.int64), db_group=t(dg, torch.int64), return_sims=True, status=status)
    return nb, sims, info.cpu().numpy(), int(status.item())


def _yardstick(dev, q, db, ranks, used):
    """ops.retrieve per query over the reference row set: -> (neighbours, sims, bad ranks)."""
    from relpose_gnn_amd import ops
    qt, dbt = torch.as_tensor(q).to(dev), torch.as_tensor(db).to(dev)
    rt = torch.as_tensor(np.asarray(ranks), dtype=torch.int32).to(dev)
    inv = ops.row_inv_norms(dbt)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    one = torch.ones(1, dtype=torch.int64, device=dev)
    groups = torch.as_tensor(np.where(used, 0, 1).astype(np.int64)).to(dev)
    nbs, sims = [], []
    for g in range(q.shape[0]):
        nb, s = ops.retrieve(qt[g:g + 1], dbt, rt[g:g + 1], db_inv_norm=inv, q_group=one, db_group=groups[g], return_sims=True,
                             status=status)
        nbs.append(nb)
        sims.append(s)
    return torch.cat(nbs), torch.cat(sims), int(status.item())


def _check(dev, q, db, ranks, gate_rows, prior, r2, cos_half, qg=None, dg=None):
    info, used = R.gated_rows(gate_rows, prior, r2, cos_half, ranks, qg, dg)
    nb, sims, got_info, bad = _gated(dev, q, db, ranks, gate_rows, prior, r2, cos_half, qg, dg)
    want_nb, want_sims, want_bad = _yardstick(dev, q, db, ranks, used)
    assert np.array_equal(got_info, info), (got_info.tolist(), info.tolist())
    assert torch.equal(nb, want_nb)
    assert torch.equal(sims.view(torch.int32), want_sims.view(torch.int32))       # bit for bit, NaN included
    assert bad == want_bad
    return info


@pytest.mark.parametrize("groups", [False, True], ids=["nogroups", "groups"])
@pytest.mark.parametrize("m", [17, 37, 1023, 1025, 1100])
def test_gated_equals_the_group_filtered_kernel(dev, m, groups):
    """M: a 16-row tail tile, and the select kernel's 1024-thread stride boundary; G crosses the dot kernel's 64-query chunk; K
    and the sampling period move the largest rank (need) across the number of rows inside.  Every launch mixes the three states."""
    seen = set()
    combos = [(d, g, k, sp) for d in (8, 64) for g in (1, 5, 65) for k in (1, 3, 7) for sp in (1, 3)]
    for n, (d, g, k, sp) in enumerate(combos):
        if (k - 1) * sp + 1 > m:                              # (no rule asks a map for more positions than it has rows)
            continue
        if g == 65 and n % 3:                                 # the 65-query launches: every third (K, period) combination
            continue
        q, db, gate_rows, prior = _scene(m, d, g, 100 * m + n)
        ranks = np.tile(np.arange(k, dtype=np.int32) * sp, (g, 1))
        qg = dg = None
        if groups:
            rng = np.random.RandomState(n)
            dg, qg = rng.randint(0, 3, m), rng.randint(-1, 3, g)
        # a radius that holds a handful of rows of the box: need = (K - 1) sp + 1 = 1 .. 19 falls on both sides of the rows inside
        info = _check(dev, q, db, ranks, gate_rows, prior, 1.4 ** 2 if m > 100 else 5.0 ** 2, None if n % 2 else 0.3, qg, dg)
        seen |= set(info[:, 0].tolist())
    assert seen == {0, 1, 2}


def test_every_row_and_no_row_inside(dev):
    q, db, gate_rows, prior = _scene(37, 8, 5, 3)
    prior = gate_rows[:5].copy()
    ranks = np.tile(np.arange(3, dtype=np.int32), (5, 1))
    info = _check(dev, q, db, ranks, gate_rows, prior, 1e6, None)                 # every row inside: gated, and the plain ranking
    assert info.tolist() == [[0, 37]] * 5
    info = _check(dev, q, db, ranks, gate_rows, prior, 1e6, -1.0)                 # max_deg = 360: the rotation gate passes all
    assert info.tolist() == [[0, 37]] * 5
    prior[:, 0] += 1e4
    info = _check(dev, q, db, ranks, gate_rows, prior, 1.0, None)                 # no row inside: fallback
    assert info.tolist() == [[2, 0]] * 5


def test_group_excludes_every_inside_row(dev):
    q, db, gate_rows, prior = _scene(37, 8, 3, 4)
    gate_rows[:, :3] = 100.0 + np.arange(37)[:, None] * 50.0
    gate_rows[:6, :3] = np.arange(6)[:, None] * 0.01                              # six rows near the origin ...
    dg = np.where(np.arange(37) < 6, 7, 0)                                        # ... all of group 7
    prior = np.tile(np.concatenate([np.zeros(3), [1.0, 0, 0, 0]]), (3, 1))
    ranks = np.tile(np.arange(2, dtype=np.int32), (3, 1))
    info = _check(dev, q, db, ranks, gate_rows, prior, 1.0, None, np.array([7, -1, 0]), dg)
    assert info.tolist() == [[2, 0], [0, 6], [0, 6]]          # query 0: nothing left inside -> the groups alone; the others gated


def test_boundaries(dev):
    """The hand cases of the CPU list, through the kernel: a row exactly on the radius, radius 0 on a map row, -q, a rotation
    exactly at max_deg, a NaN map row, and rows_inside == need / need - 1."""
    from relpose_gnn_amd.retrieval import PoseGate
    rng = np.random.RandomState(8)
    m, d = 17, 8
    db, q = rng.standard_normal((m, d)).astype(np.float32), rng.standard_normal((1, d)).astype(np.float32)
    ident = np.array([1.0, 0, 0, 0])
    far = np.concatenate([1e3 + np.arange(m)[:, None] * np.ones((1, 3)), np.tile(ident, (m, 1))], 1)
    prior = np.concatenate([[1.0, 2.0, 3.0], ident])[None]
    one = np.zeros((1, 1), dtype=np.int32)
    # (3, 4, 0) from the prior: d2 = 25 = r2, inside; one ulp further out in z: outside
    rows = far.copy()
    rows[4, :3], rows[9, :3] = (4.0, 6.0, 3.0), (4.0, 6.0, np.nextafter(3.0, 4.0) + 1e-7)
    assert _check(dev, q, db, one, rows, prior, 25.0, None).tolist() == [[0, 1]]
    # radius 0, the prior on row 11; row 12 an ulp away
    rows = far.copy()
    rows[11, :3], rows[12, :3] = (1.0, 2.0, 3.0), (1.0, 2.0, np.nextafter(3.0, 4.0))
    assert _check(dev, q, db, one, rows, prior, 0.0, None).tolist() == [[0, 1]]
    # -q is the same rotation; a rotation exactly at max_deg is inside, half a degree more is not
    for deg in (10.0, 33.3, 90.0):
        gate = PoseGate(1.0, deg)
        rows = far.copy()
        rows[:4, :3] = (1.0, 2.0, 3.0)
        rows[0, 3:], rows[1, 3:] = R.quat_about_z(deg), -R.quat_about_z(deg)
        rows[2, 3:], rows[3, 3:] = R.quat_about_z(deg + 0.5), -ident
        info = _check(dev, q, db, np.array([[0, 2]], dtype=np.int32), rows, prior, gate.r2, gate.cos_half)
        assert info.tolist() == [[0, 3]], deg                 # rows 0, 1, 3
    # a NaN / inf entry puts a row outside, with and without the rotation gate
    rows = far.copy()
    rows[:5, :3] = (1.0, 2.0, 3.0)
    rows[1, 1], rows[2, 4], rows[3, 6] = np.nan, np.inf, np.nan
    assert _check(dev, q, db, np.array([[0, 1]], dtype=np.int32), rows, prior, 1.0, None).tolist() == [[0, 2]]
    assert _check(dev, q, db, np.array([[0, 1]], dtype=np.int32), rows, prior, 1.0, 0.5).tolist() == [[0, 2]]
    # rows_inside == need: gated; == need - 1: fallback
    rows = far.copy()
    rows[3:8, :3] = (1.0, 2.0, 3.0)
    assert _check(dev, q, db, np.array([[0, 2, 4]], dtype=np.int32), rows, prior, 1.0, None).tolist() == [[0, 5]]
    assert _check(dev, q, db, np.array([[0, 2, 5]], dtype=np.int32), rows, prior, 1.0, None).tolist() == [[2, 5]]


def test_null_gate_pointers_are_the_plain_kernel(dev):
    """The new symbol without a gate against rpg_retrieve_cosine_f32: same neighbours, same similarity bits, same count."""
    from relpose_gnn_amd import _lib, ops
    lib = _lib.lib()
    rng = np.random.RandomState(12)
    for m, d, g, k in ((37, 8, 5, 3), (1025, 64, 65, 7)):
        q = torch.as_tensor(rng.standard_normal((g, d)).astype(np.float32)).to(dev)
        db = torch.as_tensor(rng.standard_normal((m, d)).astype(np.float32)).to(dev)
        ranks = torch.as_tensor(np.tile(np.arange(k, dtype=np.int32) * 2, (g, 1))).to(dev)
        qg = torch.as_tensor(rng.randint(-1, 3, g)).to(dev)
        dg = torch.as_tensor(rng.randint(0, 3, m)).to(dev)
        want_nb, want_s = ops.retrieve(q, db, ranks, q_group=qg, db_group=dg, return_sims=True)
        ws = torch.empty(int(lib.rpg_retrieve_workspace_bytes(g, m, d)), dtype=torch.uint8, device=dev)
        nb = torch.empty((g, k), dtype=torch.int64, device=dev)
        s = torch.empty((g, k), dtype=torch.float32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        rc = lib.rpg_retrieve_cosine_gated_f32(q.data_ptr(), db.data_ptr(), None, qg.data_ptr(), dg.data_ptr(), ranks.data_ptr(), g, k,
                                               m, d, None, None, 0.0, 0.0, 0, None, nb.data_ptr(), s.data_ptr(), ws.data_ptr(),
                                               ws.numel(), status.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        assert torch.equal(nb, want_nb) and torch.equal(s.view(torch.int32), want_s.view(torch.int32)) and int(status.item()) == 0


def test_feature_map_retrieve_with_a_host_prior(dev):
    """FeatureMap.retrieve(prior=, gate=): a host array is staged, gate_rows come from the map's poses, gate_info is written to the
    caller's tensor -- and the rows equal ops.retrieve_gated on the same inputs."""
    from relpose_gnn_amd import ops
    from relpose_gnn_amd.featmap import FeatureMap
    from relpose_gnn_amd.retrieval import PoseGate, RetrievalRule
    gen = torch.Generator().manual_seed(3)
    m, d, g = 37, 64, 5
    feats = torch.randn(m, d, generator=gen).to(dev)
    poses = torch.randn(m, 6, generator=gen)
    groups = torch.randint(0, 3, (m,), generator=gen)
    fmap = FeatureMap(feats, {"feat_dim": d, "precision": "f32", "encoder_digest": "0" * 16}, poses=poses, groups=groups)
    gate = PoseGate(1.5, 120.0, pose_m=(0.5, 0.0, -1.0), pose_s=(2.0, 1.0, 0.5))
    rule = RetrievalRule(k=3, sampling_period=2)
    rows = fmap.gate_rows(gate)
    prior = rows[:g].cpu().numpy().copy()
    prior[1] = np.nan
    prior[3, :3] += 100.0
    q = torch.randn(g, d, generator=gen).to(dev)
    qg = [0, -1, 2, 1, -1]
    info = torch.empty((g, 2), dtype=torch.int32, device=dev)
    nb = fmap.retrieve(q, rule, qg, prior=prior, gate=gate, gate_info=info)
    want_info, used = R.gated_rows(rows.cpu().numpy(), prior, gate.r2, gate.cos_half, rule.ranks([m] * g), qg, groups.numpy())
    assert np.array_equal(info.cpu().numpy(), want_info) and set(want_info[:, 0].tolist()) == {0, 1, 2}
    want_nb, _, bad = _yardstick(dev, q.cpu().numpy(), feats.cpu().numpy(), rule.ranks([m] * g), used)
    assert torch.equal(nb, want_nb) and bad == 0
    assert torch.equal(nb, fmap.retrieve(q, rule, qg, prior=torch.as_tensor(prior).to(dev), gate=gate))     # a device prior
    with pytest.raises(ValueError, match="float64"):
        fmap.retrieve(q, rule, qg, prior=torch.as_tensor(prior, dtype=torch.float32).to(dev), gate=gate)
    assert not torch.equal(nb, fmap.retrieve(q, rule, qg))                        # (the gate did change something)
