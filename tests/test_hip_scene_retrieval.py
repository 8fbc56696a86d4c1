"""Scene-scoped retrieval on the GPU (rpg_retrieve_cosine_scoped_f32 / ops.retrieve_scoped) against the existing entry points
on the same atlas with the rows outside a query's scene excluded through an emulated group array (scene_ref.oracle): neighbours,
similarities (as bits), gate states and the bad-rank count must be EQUAL -- the scope changes what is computed, never a bit of
what is returned.  Scene sizes (37, 91, 16, 5): boundaries inside the 16-row dot tiles, a scene of exactly one tile, and one
that ranks (0, 2, 4) exhaust."""
import numpy as np
import pytest
import torch

import scene_ref as SR

pytestmark = pytest.mark.gpu

SIZES, M = SR.SIZES, int(np.sum(SR.SIZES))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _ranks(g, ranks=SR.RANKS):
    return np.tile(np.asarray(ranks, dtype=np.int32), (g, 1))


def _scoped(dev, q, db, ranks, scenes, q_groups=None, db_group=None, gate=None, workspace=None, sizes=SIZES):
    """-> (neighbours, sims, gate_info or None, status) on the host, like scene_ref.oracle."""
    from relpose_gnn_amd import ops
    first = torch.from_numpy(SR.scene_first(sizes)).to(dev)
    qs = torch.as_tensor(np.asarray(scenes), dtype=torch.int32).to(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    qg = None if q_groups is None else torch.as_tensor(np.asarray(q_groups), dtype=torch.int64).to(dev)
    dg = None if db_group is None else torch.as_tensor(np.asarray(db_group), dtype=torch.int64).to(dev)
    kw = dict(q_group=qg, db_group=dg, return_sims=True, status=status, workspace=workspace)
    if gate is None:
        nb, sims = ops.retrieve_scoped(q, db, ranks, first, qs, **kw)
        info = None
    else:
        dbg, prior, r2, ch, rot = gate
        nb, sims, info = ops.retrieve_scoped(q, db, ranks, first, qs, dbg, prior, r2, ch, rot, **kw)
        info = info.cpu()
    return nb.cpu(), sims.cpu(), info, int(status.item())


def _same(got, want):
    assert torch.equal(got[0], want[0]), (got[0], want[0])
    assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
    if want[2] is not None:
        assert torch.equal(got[2], want[2]), (got[2], want[2])
    assert got[3] == want[3], (got[3], want[3])


def _case(dev, d, g, seed=0):
    q, db = SR.descriptors(d, g, seed)
    return torch.from_numpy(q).to(dev), torch.from_numpy(db).to(dev), torch.from_numpy(_ranks(g)).to(dev)


def _inside(nb, scenes):
    first = SR.scene_first()
    for row, s in zip(nb.tolist(), scenes):
        assert all(first[s] <= r < first[s + 1] for r in row), (row, s)


@pytest.mark.parametrize("d", [64, 2048])
@pytest.mark.parametrize("g", [1, 5, 70])
def test_every_scene(dev, d, g):
    """g = 70: two query chunks and a 6-query tail; d = 2048: four column slices."""
    q, db, ranks = _case(dev, d, g, seed=d + g)
    scenes = [(3 * i + 3) % 4 for i in range(g)]
    got = _scoped(dev, q, db, ranks, scenes)
    _same(got, SR.oracle(dev, q, db, ranks, SIZES, scenes))
    assert got[3] == 0
    _inside(got[0], scenes)


@pytest.mark.parametrize("d,g", [(64, 5), (2048, 70)])
def test_one_scene_reads_nothing_unwritten(dev, d, g):
    """All queries in scene 1: most dot workgroups return early and write nothing, so the workspace keeps what it held -- once
    all-ones bytes (NaN as floats, the largest key), once 1e30.  The results are the oracle's both times."""
    from relpose_gnn_amd import _lib as L
    q, db, ranks = _case(dev, d, g, seed=7)
    scenes = [1] * g
    want = SR.oracle(dev, q, db, ranks, SIZES, scenes)
    nbytes = int(L.lib().rpg_retrieve_workspace_bytes(g, M, d))
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
    _same(_scoped(dev, q, db, ranks, scenes, workspace=ws), want)
    ws = torch.full((nbytes // 4,), 1e30, dtype=torch.float32, device=dev).view(torch.uint8)
    _same(_scoped(dev, q, db, ranks, scenes, workspace=ws), want)


def test_duplicated_rows_stay_in_their_scene(dev):
    """Scene 1's first 37 rows are scene 0's, bit for bit, and the queries are those rows: a query of scene 0 finds its own row
    first in scene 0, one of scene 1 the copy in scene 1 -- never the other scene's."""
    d, g = 64, 8
    q, db = SR.descriptors(d, g, 3)
    db[37:37 + 37] = db[0:37]
    q[:] = db[[0, 5, 9, 36, 0, 5, 9, 36]]
    scenes = [0, 0, 0, 0, 1, 1, 1, 1]
    q, db, ranks = torch.from_numpy(q).to(dev), torch.from_numpy(db).to(dev), torch.from_numpy(_ranks(g)).to(dev)
    got = _scoped(dev, q, db, ranks, scenes)
    _same(got, SR.oracle(dev, q, db, ranks, SIZES, scenes))
    assert got[0][:, 0].tolist() == [0, 5, 9, 36, 37, 42, 46, 73]
    _inside(got[0], scenes)


@pytest.mark.parametrize("d,g", [(64, 5), (2048, 70)])
def test_groups_inside_scenes(dev, d, g):
    """Group ids repeat across scenes (row % 3): a query's group removes rows of its own scene only.  Scene 3 is left out here:
    its 5 rows minus a group cannot serve rank 4 (test_bad_ranks_counted_like_the_oracle has that)."""
    q, db, ranks = _case(dev, d, g, seed=11)
    db_group = np.arange(M) % 3
    scenes = [i % 3 for i in range(g)]
    q_groups = [(-1, 0, 1, 2)[(i // 3) % 4] for i in range(g)]
    got = _scoped(dev, q, db, ranks, scenes, q_groups, db_group)
    _same(got, SR.oracle(dev, q, db, ranks, SIZES, scenes, q_groups, db_group))
    assert got[3] == 0
    for row, s, c in zip(got[0].tolist(), scenes, q_groups):
        assert all(db_group[r] != c for r in row)


def _gate(dev, g, seed=5):
    """db_gate: positions ~ N(0, 1), unit quaternions; priors by query: the origin (about half of a scene inside radius 1.5), a
    far point (nothing inside), NaN (no prior)."""
    rng = np.random.RandomState(seed)
    dbg = np.concatenate([rng.standard_normal((M, 3)), rng.standard_normal((M, 4))], axis=1)
    dbg[:, 3:] /= np.linalg.norm(dbg[:, 3:], axis=1, keepdims=True)
    prior = np.zeros((g, 7))
    prior[:, 3] = 1.0
    prior[1::3, :3] = 100.0
    prior[2::3] = np.nan
    return torch.from_numpy(dbg).to(dev), torch.from_numpy(prior).to(dev), 1.5 ** 2, 0.0, False


@pytest.mark.parametrize("d,g", [(64, 5), (2048, 70)])
@pytest.mark.parametrize("groups", [False, True])
def test_gate_states(dev, d, g, groups):
    q, db, ranks = _case(dev, d, g, seed=13)
    gate = _gate(dev, g)
    scenes = [(0, 1, 1, 0, 2, 3)[i % 6] for i in range(g)] if not groups else [i % 2 for i in range(g)]
    db_group = np.arange(M) % 3 if groups else None
    q_groups = [i % 3 for i in range(g)] if groups else None
    got = _scoped(dev, q, db, ranks, scenes, q_groups, db_group, gate=gate)
    want = SR.oracle(dev, q, db, ranks, SIZES, scenes, q_groups, db_group, gate=gate)
    _same(got, want)
    assert set(want[2][:, 0].tolist()) == {0, 1, 2}            # gated, no prior, too few rows inside
    # the gate counts the scene's rows only: never more rows inside than the scene holds
    assert all(n <= SIZES[s] for n, s in zip(got[2][:, 1].tolist(), scenes))


def test_bad_ranks_counted_like_the_oracle(dev):
    """Ranks (0, 3, 6) against the 5-row scene: rank 6 is clamped and counted, as the oracle counts it; with a group taken out of
    the 5 rows rank 3 goes too."""
    d, g = 64, 5
    q, db, _ = _case(dev, d, g, seed=17)
    ranks = torch.from_numpy(_ranks(g, (0, 3, 6))).to(dev)
    scenes = [3, 0, 3, 1, 3]
    want = SR.oracle(dev, q, db, ranks, SIZES, scenes)
    assert want[3] == 3
    _same(_scoped(dev, q, db, ranks, scenes), want)
    db_group, q_groups = np.arange(M) % 3, [0, 1, 2, -1, 1]
    want = SR.oracle(dev, q, db, ranks, SIZES, scenes, q_groups, db_group)
    assert want[3] > 3
    _same(_scoped(dev, q, db, ranks, scenes, q_groups, db_group), want)


def test_scene_out_of_range_counted_once(dev):
    d, g = 64, 5
    q, db, ranks = _case(dev, d, g, seed=19)
    scenes = [0, -1, 1, len(SIZES), 3]
    nb, sims, _, status = _scoped(dev, q, db, ranks, scenes)
    assert status == 2                                          # one per query, whatever k is
    ok = [0, 2, 4]
    want = SR.oracle(dev, q[ok], db, ranks[ok], SIZES, [scenes[i] for i in ok])
    assert torch.equal(nb[ok], want[0]) and torch.equal(sims[ok].view(torch.int32), want[1].view(torch.int32))
    assert nb[[1, 3]].eq(0).all() and sims[[1, 3]].isnan().all()


def test_scene_first_is_clamped(dev):
    """Boundaries the map does not have: below 0, beyond m, descending.  Nothing is read out of bounds (the run ends clean) and
    the result is that of the clamped ranges [0, 37), [37, 149), [149, 149)."""
    from relpose_gnn_amd import ops
    d, g = 64, 6
    q, db, ranks = _case(dev, d, g, seed=23)
    first = torch.tensor([-5, 37, 10 ** 12, 3], dtype=torch.int64, device=dev)
    scenes = [0, 1, 0, 1, 0, 1]
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    nb, sims = ops.retrieve_scoped(q, db, ranks, first, torch.tensor(scenes, dtype=torch.int32, device=dev), return_sims=True,
                                   status=status)
    want = SR.oracle(dev, q, db, ranks, (37, 112), scenes)
    assert torch.equal(nb.cpu(), want[0]) and torch.equal(sims.cpu().view(torch.int32), want[1].view(torch.int32))
    assert int(status.item()) == 0


@pytest.mark.parametrize("gated", [False, True])
def test_null_scope_is_the_gated_entry(dev, gated):
    from relpose_gnn_amd import ops
    d, g = 2048, 70
    q, db, ranks = _case(dev, d, g, seed=29)
    if gated:
        dbg, prior, r2, ch, rot = _gate(dev, g)
        a = ops.retrieve_scoped(q, db, ranks, None, None, dbg, prior, r2, ch, rot, return_sims=True)
        b = ops.retrieve_gated(q, db, ranks, dbg, prior, r2, ch, rot, return_sims=True)
    else:
        a = ops.retrieve_scoped(q, db, ranks, None, None, return_sims=True)
        b = ops.retrieve(q, db, ranks, return_sims=True)
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)


def test_one_scope_pointer_is_refused(dev):
    from relpose_gnn_amd import ops
    q, db, ranks = _case(dev, 64, 5)
    first = torch.from_numpy(SR.scene_first()).to(dev)
    with pytest.raises(ValueError):
        ops.retrieve_scoped(q, db, ranks, first, None)
    with pytest.raises(ValueError):
        ops.retrieve_scoped(q, db, ranks, None, torch.zeros(5, dtype=torch.int32, device=dev))
