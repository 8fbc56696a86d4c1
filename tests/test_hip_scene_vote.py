"""The electing retrieval on the GPU (rpg_retrieve_cosine_elect_f32 / ops.retrieve_elect) against scene_vote_ref.oracle: the
voters through ``ops.retrieve(ranks=arange(V))``, the election in integers on the host, the ranking through scene_ref.oracle in
the elected scene.  Neighbours, similarities (as bits), gate states, scene_info, q_scene and the bad-rank count must be EQUAL."""
import numpy as np
import pytest
import torch

import scene_ref as SR
import scene_vote_ref as VR

pytestmark = pytest.mark.gpu

SIZES, M = SR.SIZES, int(np.sum(SR.SIZES))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _ranks(dev, g, ranks=SR.RANKS):
    return torch.from_numpy(np.tile(np.asarray(ranks, dtype=np.int32), (g, 1))).to(dev)


def _dev(dev, q, db):
    return torch.from_numpy(q).to(dev), torch.from_numpy(db).to(dev)


def _elect(dev, q, db, ranks, top, q_groups=None, db_group=None, gate=None, held=None, workspace=None, first=None):
    """-> (neighbours, sims, gate_info or None, status, q_scene, scene_info) on the host, like scene_vote_ref.oracle."""
    from relpose_gnn_amd import ops
    first = torch.from_numpy(SR.scene_first(SIZES) if first is None else np.asarray(first, dtype=np.int64)).to(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    qg = None if q_groups is None else torch.as_tensor(np.asarray(q_groups), dtype=torch.int64).to(dev)
    dg = None if db_group is None else torch.as_tensor(np.asarray(db_group), dtype=torch.int64).to(dev)
    # RPG_ELECT_ALL ignores what q_scene holds on entry: hand it scenes that do not exist
    qs = (torch.full((q.shape[0],), 77, dtype=torch.int32, device=dev) if held is None
          else torch.as_tensor(np.asarray(held), dtype=torch.int32).to(dev))
    kw = dict(q_scene=qs, lost_only=held is not None, q_group=qg, db_group=dg, return_sims=True, status=status, workspace=workspace)
    if gate is None:
        nb, sims, qs_out, info = ops.retrieve_elect(q, db, ranks, first, top, **kw)
        ginfo = None
    else:
        dbg, prior, r2, ch, rot = gate
        nb, sims, ginfo, qs_out, info = ops.retrieve_elect(q, db, ranks, first, top, db_gate=dbg, prior=prior, r2=r2, cos_half=ch,
                                                           rot_gate=rot, **kw)
        ginfo = ginfo.cpu()
    assert qs_out is qs
    return nb.cpu(), sims.cpu(), ginfo, int(status.item()), qs.cpu(), info.cpu()


def _same(got, want):
    assert torch.equal(got[5], want[5]), (got[5], want[5])                    # scene_info first: it explains the rest
    assert torch.equal(got[4], want[4]), (got[4], want[4])
    assert torch.equal(got[0], want[0]), (got[0], want[0])
    assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
    if want[2] is not None:
        assert torch.equal(got[2], want[2]), (got[2], want[2])
    assert got[3] == want[3], (got[3], want[3])


@pytest.mark.parametrize("top", [1, 7, 64])
@pytest.mark.parametrize("g", [1, 5, 70])
@pytest.mark.parametrize("d", [64, 2048])
@pytest.mark.parametrize("data", ["unstructured", "clustered"])
def test_every_query_elects(dev, data, d, g, top):
    """Unstructured normals make every election a close call; the clustered ones have a known answer.  g = 70: two query chunks
    and a 6-query tail; d = 2048: four column slices; top = 64: K_MAX, more voters than three of the four scenes hold."""
    # (clustered: one of the seeds 0-19 whose margins test_scene_vote_cpu.py asserts)
    q, db = _dev(dev, *(SR.descriptors(d, g, d + g + top) if data == "unstructured" else VR.clustered(d, g, (g + top) % 20)))
    ranks = _ranks(dev, g)
    got = _elect(dev, q, db, ranks, top)
    want = VR.oracle(dev, q, db, ranks, SIZES, top)
    _same(got, want)
    assert ((got[4] >= 0) & (got[4] < len(SIZES))).all() and (got[5][:, 1] >= 1).all() and (got[5][:, 1] <= top).all()
    if data == "clustered" and top in (1, 7):
        truth = np.arange(g) % len(SIZES)
        assert got[4].tolist() == truth.tolist()
        assert got[5][:, 1].tolist() == [min(top, SIZES[t]) for t in truth]
        assert got[3] == 0


def test_tie_goes_to_the_best_placed_voter(dev):
    """q = e0.  Scene 1 holds e0 (cosine 1) and e0 + 2 e1 (0.447), scene 0 two copies of e0 + e1 (0.707); every other row has a
    zero first component (cosine 0).  The four voters split 2 : 2 and scene 1 owns the best one: elected, not the lower index."""
    d = 64
    rng = np.random.RandomState(0)
    db = rng.standard_normal((M, d)).astype(np.float32)
    db[:, 0] = 0.0
    e0, e1 = np.eye(d, dtype=np.float32)[0], np.eye(d, dtype=np.float32)[1]
    db[3], db[20] = e0 + e1, e0 + e1
    db[40], db[100] = e0, e0 + 2 * e1
    q, db = _dev(dev, np.tile(e0, (3, 1)), db)
    ranks = _ranks(dev, 3)
    got = _elect(dev, q, db, ranks, 4)
    _same(got, VR.oracle(dev, q, db, ranks, SIZES, 4))
    assert got[5].tolist() == [[1, 2]] * 3 and got[4].tolist() == [1, 1, 1]
    assert got[0][:, 0].tolist() == [40, 40, 40]


def test_duplicated_rows_elect_the_lower_row(dev):
    """Scene 1's first 37 rows are scene 0's, bit for bit, and the queries are those rows: equal similarities, so the lower row
    is the one voter and scene 0 is elected."""
    d, g = 64, 4
    q, db = SR.descriptors(d, g, 3)
    db[37:37 + 37] = db[0:37]
    q[:] = db[[0, 5, 9, 36]]
    q, db = _dev(dev, q, db)
    ranks = _ranks(dev, g)
    got = _elect(dev, q, db, ranks, 1)
    _same(got, VR.oracle(dev, q, db, ranks, SIZES, 1))
    assert got[5].tolist() == [[0, 1]] * g and got[0][:, 0].tolist() == [0, 5, 9, 36]


@pytest.mark.parametrize("top", [1, 7])
def test_nan_and_zero_queries(dev, top):
    """A NaN query's similarities are all non-finite and a zero query's all 0: both orders are the row order, the voters are
    rows 0 .. V-1 and scene 0 is elected."""
    d, g = 64, 5
    q, db = VR.clustered(d, g, 11)
    q[1], q[3] = np.nan, 0.0
    q, db = _dev(dev, q, db)
    ranks = _ranks(dev, g)
    got = _elect(dev, q, db, ranks, top)
    _same(got, VR.oracle(dev, q, db, ranks, SIZES, top))
    assert got[5][[1, 3]].tolist() == [[0, top]] * 2
    assert got[1][1].isnan().all() and got[0][1].tolist() == [0, 2, 4]


@pytest.mark.parametrize("data", ["unstructured", "clustered"])
@pytest.mark.parametrize("d,g", [(64, 5), (2048, 70)])
def test_groups_apply_inside_the_elected_scene_only(dev, data, d, g):
    """Group ids repeat across scenes (row % 3).  The vote ignores them -- the oracle's voters are retrieved without groups -- and
    the selection leaves the query's group out of the elected scene.  Ranks (0, 1, 2): the 5-row scene minus a group keeps 3."""
    q, db = _dev(dev, *(SR.descriptors if data == "unstructured" else VR.clustered)(d, g, 11))
    ranks = _ranks(dev, g, (0, 1, 2))
    db_group = np.arange(M) % 3
    q_groups = [(-1, 0, 1, 2)[(i // 3) % 4] for i in range(g)]
    got = _elect(dev, q, db, ranks, 7, q_groups, db_group)
    _same(got, VR.oracle(dev, q, db, ranks, SIZES, 7, q_groups, db_group))
    assert got[3] == 0
    for row, c in zip(got[0].tolist(), q_groups):
        assert all(db_group[r] != c for r in row)
    # the election is the one without groups
    assert torch.equal(got[5], _elect(dev, q, db, ranks, 7)[5])


def _gate(dev, g, seed=5):
    """As test_hip_scene_retrieval._gate: priors by query the origin, a far point (nothing inside), NaN (no prior)."""
    rng = np.random.RandomState(seed)
    dbg = np.concatenate([rng.standard_normal((M, 3)), rng.standard_normal((M, 4))], axis=1)
    dbg[:, 3:] /= np.linalg.norm(dbg[:, 3:], axis=1, keepdims=True)
    prior = np.zeros((g, 7))
    prior[:, 3] = 1.0
    prior[1::3, :3] = 100.0
    prior[2::3] = np.nan
    return torch.from_numpy(dbg).to(dev), torch.from_numpy(prior).to(dev), 1.5 ** 2, 0.0, False


@pytest.mark.parametrize("d,g", [(64, 6), (2048, 70)])
def test_gate_states(dev, d, g):
    """RPG_ELECT_ALL with a gate: the vote is ungated, the selection gates inside the elected scene."""
    q, db = _dev(dev, *SR.descriptors(d, g, 13))
    ranks = _ranks(dev, g)
    gate = _gate(dev, g)
    got = _elect(dev, q, db, ranks, 7, gate=gate)
    want = VR.oracle(dev, q, db, ranks, SIZES, 7, gate=gate)
    _same(got, want)
    if g == 70:
        assert set(want[2][:, 0].tolist()) == {0, 1, 2}        # gated, no prior, too few rows inside


def _lost_case(dev, d, g, seed):
    q, db = _dev(dev, *VR.clustered(d, g, seed))
    gate = _gate(dev, g)                                        # NaN priors at 2, 5, 8, ...
    held = np.asarray([(1, -1, 2, 0, 3, 1, -1)[i % 7] for i in range(g)])
    return q, db, _ranks(dev, g), gate, held


@pytest.mark.parametrize("d,g", [(64, 7), (2048, 70)])
@pytest.mark.parametrize("gated", [False, True])
def test_lost_only(dev, d, g, gated):
    """Held entries, -1 entries, finite priors and NaN priors mixed.  The held queries equal the scoped entry (the oracle ranks
    them in the scene they hold); q_scene afterwards holds the elected values; a second call on it, with finite priors, holds
    everything and equals the scoped entry."""
    from relpose_gnn_amd import ops
    q, db, ranks, gate, held = _lost_case(dev, d, g, 17)
    got = _elect(dev, q, db, ranks, 7, gate=gate if gated else None, held=held)
    want = VR.oracle(dev, q, db, ranks, SIZES, 7, gate=gate if gated else None, held=held)
    _same(got, want)
    elects = held == -1
    if gated:
        elects = elects | ~np.isfinite(gate[1].cpu().numpy()).all(axis=1)
    assert elects.any() and not elects.all()
    truth = np.arange(g) % len(SIZES)
    assert got[4].tolist() == np.where(elects, truth, held).tolist()
    assert (got[5][:, 1] == 0).tolist() == (~elects).tolist()
    # again, on the scenes the first call left and with priors that are all finite: nothing elects
    gate2 = None
    if gated:
        prior2 = gate[1].clone()
        prior2[2::3] = prior2[0]
        gate2 = (gate[0], prior2, *gate[2:])
    again = _elect(dev, q, db, ranks, 7, gate=gate2, held=got[4].numpy())
    assert torch.equal(again[4], got[4]) and again[5][:, 1].eq(0).all() and torch.equal(again[5][:, 0], got[4])
    first = torch.from_numpy(SR.scene_first()).to(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    if gated:
        nb, sims, ginfo = ops.retrieve_scoped(q, db, ranks, first, got[4].to(dev), gate2[0], gate2[1], gate2[2], gate2[3], gate2[4],
                                              return_sims=True, status=status)
        assert torch.equal(again[2], ginfo.cpu())
    else:
        nb, sims = ops.retrieve_scoped(q, db, ranks, first, got[4].to(dev), return_sims=True, status=status)
    assert torch.equal(again[0], nb.cpu()) and torch.equal(again[1].view(torch.int32), sims.cpu().view(torch.int32))
    assert again[3] == int(status.item()) == 0


@pytest.mark.parametrize("d,g", [(64, 5), (2048, 70)])
def test_all_held_reads_nothing_unwritten(dev, d, g):
    """Every query held in scene 1: most dot workgroups return early, the vote returns at once, and the workspace keeps what it
    held -- once all-ones bytes, once 1e30.  The results are the scoped oracle's both times."""
    from relpose_gnn_amd import _lib as L
    q, db = _dev(dev, *SR.descriptors(d, g, 7))
    ranks = _ranks(dev, g)
    held = [1] * g
    want = SR.oracle(dev, q, db, ranks, SIZES, held)
    nbytes = int(L.lib().rpg_retrieve_elect_workspace_bytes(g, M, d))
    for ws in (torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev),
               torch.full((nbytes // 4,), 1e30, dtype=torch.float32, device=dev).view(torch.uint8)):
        got = _elect(dev, q, db, ranks, 7, held=held, workspace=ws)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
        assert got[3] == want[3] == 0 and got[4].tolist() == held and got[5].tolist() == [[1, 0]] * g


def test_held_out_of_range_counted_once(dev):
    d, g = 64, 5
    q, db = _dev(dev, *VR.clustered(d, g, 19))
    ranks = _ranks(dev, g)
    held = [0, len(SIZES), -1, -7, 2]
    got = _elect(dev, q, db, ranks, 7, held=held)
    _same(got, VR.oracle(dev, q, db, ranks, SIZES, 7, held=held))
    assert got[3] == 2                                          # one per query, whatever k is
    assert got[4].tolist() == [0, len(SIZES), 2, -7, 2] and got[5].tolist() == [[0, 0], [len(SIZES), 0], [2, 7], [-7, 0], [2, 0]]
    assert got[0][[1, 3]].eq(0).all() and got[1][[1, 3]].isnan().all()


def test_scene_first_is_clamped(dev):
    """Boundaries the map does not have: below 0, beyond m, descending.  Nothing is read out of bounds (the run ends clean) and
    the result is that of the clamped scenes [0, 37), [37, 149), [149, 149)."""
    d, g = 64, 6
    q, db = _dev(dev, *SR.descriptors(d, g, 23))
    ranks = _ranks(dev, g)
    raw = [-5, 37, 10 ** 12, 3]
    got = _elect(dev, q, db, ranks, 7, first=raw)
    _same(got, VR.oracle(dev, q, db, ranks, (37, 112), 7, first=raw))
    assert got[3] == 0 and set(got[4].tolist()) <= {0, 1}


def test_rows_without_a_scene_do_not_vote(dev):
    """Boundaries that start at row 60 and end at row 100: the voters below and above belong to no scene.  Query 0 is a copy of
    row 3 and, with one voter, elects nothing: -1, no votes, row 0, NaN, one count."""
    d, g = 64, 6
    q, db = SR.descriptors(d, g, 29)
    q[0] = db[3]
    q, db = _dev(dev, q, db)
    ranks = _ranks(dev, g)
    raw = [60, 80, 100]
    for top in (1, 16):
        got = _elect(dev, q, db, ranks, top, first=raw)
        first = torch.tensor(raw, dtype=torch.int64, device=dev)
        # scene_ref's oracle cannot state scenes that do not start at row 0: the scoped entry on the elected scenes is the reference
        from relpose_gnn_amd import ops
        voters = ops.retrieve(q, db, torch.arange(top, dtype=torch.int32, device=dev).repeat(g, 1)).cpu().numpy()
        info = np.asarray([VR.vote(v, raw, M) for v in voters], dtype=np.int32)
        assert got[5].tolist() == info.tolist() and got[4].tolist() == info[:, 0].tolist()
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        nb, sims = ops.retrieve_scoped(q, db, ranks, first, got[4].to(dev), return_sims=True, status=status)
        assert torch.equal(got[0], nb.cpu()) and torch.equal(got[1].view(torch.int32), sims.cpu().view(torch.int32))
        assert got[3] == int(status.item()) == int((info[:, 0] < 0).sum())
        if top == 1:
            assert got[5][0].tolist() == [-1, 0] and got[0][0].eq(0).all() and got[1][0].isnan().all()


def test_existing_entries_keep_their_bits(dev):
    """The three existing entry points on the same buffers -- workspace included -- before and after electing calls."""
    from relpose_gnn_amd import _lib as L, ops
    d, g = 2048, 70
    q, db = _dev(dev, *SR.descriptors(d, g, 37))
    ranks = _ranks(dev, g)
    dbg, prior, r2, ch, rot = _gate(dev, g)
    first = torch.from_numpy(SR.scene_first()).to(dev)
    scenes = torch.as_tensor([i % 4 for i in range(g)], dtype=torch.int32, device=dev)
    ws = torch.zeros(int(L.lib().rpg_retrieve_elect_workspace_bytes(g, M, d)), dtype=torch.uint8, device=dev)

    def existing():
        a = ops.retrieve(q, db, ranks, return_sims=True, workspace=ws)
        b = ops.retrieve_gated(q, db, ranks, dbg, prior, r2, ch, rot, return_sims=True, workspace=ws)
        c = ops.retrieve_scoped(q, db, ranks, first, scenes, dbg, prior, r2, ch, rot, return_sims=True, workspace=ws)
        return [t.clone().view(torch.int32) if t.dtype == torch.float32 else t.clone() for t in (*a, *b, *c)]
    before = existing()
    _elect(dev, q, db, ranks, 7, workspace=ws)
    _elect(dev, q, db, ranks, 64, gate=(dbg, prior, r2, ch, rot), held=[(-1, 2)[i % 2] for i in range(g)], workspace=ws)
    after = existing()
    assert len(before) == len(after) == 8
    for x, y in zip(before, after):
        assert torch.equal(x, y)
    assert torch.equal(scenes.cpu(), torch.as_tensor([i % 4 for i in range(g)], dtype=torch.int32))
