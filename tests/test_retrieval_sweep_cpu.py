"""The retrieval sweep's helper (tests/retrieval_sweep_ref.py) held to hand-worked values, its case lists to the axes they are meant
to cover, its integer oracle to the float64 restatement of the rule, and its emulation to the oracle -- without a defect on every
case, and with each planted defect failing a case of the list meant to pin it.  No GPU: the library is loaded for its host-only
planner and size functions."""
import ctypes as C

import numpy as np
import pytest

import pose_gate_ref as G
import retrieval_ref as R
import retrieval_sweep_ref as S
import scene_vote_ref as SV


# ---- the restated rule at hand-worked values -------------------------------------------------------------------------------------
def test_split_plan_by_hand():
    # (m, d): tiles = ceil(m / 16), nblk = ceil(d / 64), s = min(ceil(1024 / tiles), max(1, nblk // 8), 16), bps = ceil(nblk / s)
    assert S.split_plan(1, 4) == (1, 1) and S.split_plan(7, 8) == (1, 1)             # one block
    assert S.split_plan(17, 60) == (1, 1) and S.split_plan(33, 64) == (1, 1)
    assert S.split_plan(40, 260) == (1, 5)                                           # 5 blocks: nblk // 8 == 0 caps s at 1
    assert S.split_plan(40, 1028) == (2, 9)                                          # 17 blocks, s = 2: 9 + 8
    assert S.split_plan(100, 6340) == (12, 9)                                        # 100 blocks, s = 12: 11 x 9 + 1
    assert S.split_plan(17, 8192) == (16, 8)                                         # 128 blocks, s = 16
    assert S.split_plan(1488, 6340) == (12, 9)                                       # 93 tiles: ceil(1024 / 93) = 12
    assert S.split_plan(1489, 6340) == (10, 10)                                      # 94 tiles: ceil(1024 / 94) = 11, bps 10
    assert S.split_plan(300000, 2048) == (1, 32)
    for shape, want in S.PLAN_WANT.items():
        assert S.split_plan(*shape) == want, shape
    assert S.slice_blocks(40, 1028) == [(0, 9), (9, 17)]
    assert S.slice_blocks(100, 6340)[-1] == (99, 100) and 6340 - 99 * 64 == 4        # one block, 4 live columns, wave 0 alone
    assert S.slice_blocks(1489, 6340)[-1] == (90, 100)


def test_query_tiling_by_hand():
    want = {1: (1, 1), 15: (1, 1), 16: (1, 1), 17: (2, 1), 32: (2, 1), 33: (4, 1), 48: (4, 1), 49: (4, 1), 64: (4, 1), 65: (4, 2),
            81: (4, 2), 129: (4, 3)}
    assert set(want) == set(S.QUERY_G)
    for g, (nq, chunks) in want.items():
        assert S.plan(g, 40, 260)[2:] == (nq, chunks), g


def test_digit_skips_by_hand():
    key = (56, 48, 40, 32)
    assert S.live_digits(0, 1) == key                                                # one row: every row digit skipped
    assert S.live_digits(0, 149) == key + (0,) == S.live_digits(0, 200) == S.live_digits(200, 256) == S.live_digits(0, 256)
    assert S.live_digits(0, 257) == key + (8, 0) == S.live_digits(256, 257) == S.live_digits(0, 65536)
    assert S.live_digits(0, 65537) == key + (16, 8, 0) == S.live_digits(557, 65557) == S.live_digits(65557, 66257)
    assert S.skipped_digits(0, 65537) == (24,) and S.skipped_digits(0, 256) == (24, 16, 8)


def test_gate_steps_by_hand():
    assert S.gate_step(0) == (0, 0) and S.gate_step(1023) == (0, 0) and S.gate_step(1024) == (0, 1)
    assert S.gate_step(3071) == (0, 2) and S.gate_step(3072) == (0, 3) and S.gate_step(4095) == (0, 3)
    assert S.gate_step(4096) == (1, 0) and S.gate_step(8199) == (2, 0)
    assert S.gate_step(557 + 4096 + 3072, lo=557) == (1, 3)


def test_workspace_layouts_by_hand():
    assert S.ws_layout(5, 40, 260) == {"q_inv": 0, "db_inv": 256, "part": 512, "total": 512 + 1024}      # 1 x 5 x 40 x 4 = 800
    assert S.elect_layout(5, 40, 260) == {"q_inv": 0, "db_inv": 256, "part": 512, "vkeys": 1536, "total": 2560}
    assert S.ws_layout(65, 40, 1028)["total"] == 512 + 256 + 2 * 65 * 40 * 4 + (-2 * 65 * 40 * 4) % 256


def test_library_plan_and_sizes_equal_the_restatement():
    from relpose_gnn_amd import _lib
    lib = _lib.lib()
    out = (C.c_int32 * 4)()
    shapes = [(g, 40, 260) for g in S.QUERY_G] + [(S._plan_g(m, d), m, d) for m, d in S.PLAN_SHAPES]
    shapes += [(3, m, 8) for m in S.SELECT_M + S.GATE_M] + [(12, 66257, 8), (70, 300000, 2048)]
    for g, m, d in shapes:
        assert lib.rpg_retrieve_plan(g, m, d, out) == 0 and tuple(out) == S.plan(g, m, d), (g, m, d)
        assert int(lib.rpg_retrieve_workspace_bytes(g, m, d)) == S.ws_layout(g, m, d)["total"], (g, m, d)
        assert int(lib.rpg_retrieve_elect_workspace_bytes(g, m, d)) == S.elect_layout(g, m, d)["total"], (g, m, d)
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, 6), (1, 4, 0), (1, 1 << 31, 4)):
        assert lib.rpg_retrieve_plan(*bad, out) == _lib.RPG_ERR_BAD_ARG, bad
    assert lib.rpg_retrieve_plan(1, 4, 4, None) == _lib.RPG_ERR_BAD_ARG


def test_bound_chain_lengths_by_hand():
    assert S.chain_lengths(7, 8) == (1 + 64 + 3, 14)
    assert S.chain_lengths(1488, 6340) == (1 + 64 * 3 + 3 + 11, 13 + 7)              # bps 9: a wave owns at most 3 blocks
    assert S.chain_lengths(17, 8192) == (1 + 64 * 2 + 3 + 15, 21)
    assert S.gamma(100) == 100 * 2.0 ** -24 / (1 - 100 * 2.0 ** -24)


# ---- the case lists ----------------------------------------------------------------------------------------------------------------
def test_case_lists_hold_every_axis_value():
    ids = {k: [s.id for s in v] for k, v in S.EXACT_LISTS.items()}
    assert ids["plan"] == [f"plan_m{m}_d{d}" for m, d in S.PLAN_SHAPES] and len(S.PLAN_SHAPES) == 10
    assert ids["tile"] == [f"tile_m{m}" for m in (15, 16, 17, 31, 32, 33)]
    assert ids["queries"] == [f"queries_g{g}" for g in (1, 15, 16, 17, 32, 33, 48, 49, 64, 65, 81, 129)]
    for m in (1, 2, 255, 256, 257, 1023, 1024, 1025, 65535, 65536, 65537):
        for r in {min(r, m) for r in (1, 2, 511, 512)}:
            assert f"select_m{m}_R{r}" in ids["select"]
        assert f"select_m{m}_end" in ids["select"] and f"select_m{m}_spread" in ids["select"]
    assert ids["gate"] == [f"gate_m{m}_{w}" for m in (2047, 2049, 3073, 4095, 4097, 8200) for w in ("plain", "groups")]
    assert S.atlas_first().tolist() == [0, 200, 256, 257, 557, 65557, 66257]
    assert {s.id for s in S.VOTE_CASES} == {f"vote_{w}_top{v}" for w in ("all", "lost") for v in (1, 7, 64)}
    assert [s.id for s in S.FLOAT_CASES] == [f"float_{kd}_m{m}_d{d}" for m, d in S.PLAN_SHAPES for kd in ("iid", "trajectory")]
    every = [s.id for v in S.EXACT_LISTS.values() for s in v] + [s.id for s in S.FLOAT_CASES]
    assert len(set(every)) == len(every)


def test_cases_reach_the_paths_they_are_named_for():
    for spec in S.PLAN_CASES:
        c = S.build(spec)
        if c.m * 48 >= 4 * c.d:                                       # enough non-zeros to go round
            assert S.coverage(c.db.astype(np.int8)) == {"blocks_missing": 0, "offsets_missing": 0, "last_float4_missing": 0}, spec.id
        assert len(set(np.abs(c.db).sum(1).tolist())) == 1            # one weight: one inverse norm, bit for bit
    sel = {s.id: s for s in S.SELECT_CASES}
    c = S.build(sel["select_m65537_R512"])
    assert c.ranks.max() == 511 and c.k == 12 and not (np.diff(c.ranks, axis=1) == 1).all()
    want = S.oracle(c)
    assert {255, 256} <= set(want.nbrs[3].tolist())                   # the tie class of 9s across row 255 / 256, beyond R
    assert (c.score[3] == 9).sum() > S.R_MAX
    # the zero query: one tie class of every finite row, in index order
    assert want.nbrs[2].tolist() == np.flatnonzero(~c.nonfinite[2])[c.ranks[2]].tolist()
    c = S.build(sel["select_m65537_end"])
    assert np.flatnonzero(c.db_group == 0).min() == 65537 - 511
    want = S.oracle(c)
    assert 65536 in want.nbrs[2].tolist() and 65535 not in np.flatnonzero(c.nonfinite[0]).tolist()
    assert want.status == 2                                           # allowed == R - 1 twice: one bad rank each
    c = S.build(sel["select_m65537_spread"])
    want = S.oracle(c)
    assert any(c.nonfinite[j, want.nbrs[j]].any() and not c.nonfinite[j, want.nbrs[j]].all() for j in range(4))     # straddled
    assert any((c.score[j, want.nbrs[j]] < 0).any() for j in range(c.g))
    for spec in S.GATE_CASES:
        c = S.build(spec)
        steps = {S.gate_step(r) for r in np.flatnonzero(c.gate["inside"])}
        lanes = {(o, l) for o in range(-(-c.m // 4096)) for l in range(4) if o * 4096 + l * 1024 < c.m}
        assert steps == lanes, spec.id
        assert S.oracle(c).gate_info[:, 0].tolist() == [0, 0, 1, 2], spec.id
    assert (1, 3) in {S.gate_step(r) for r in S.gate_rows(8200)} and (2, 0) in {S.gate_step(r) for r in S.gate_rows(8200)}
    c = S.build(S.SCOPE_CASES[1])
    info = S.oracle(c).gate_info
    assert {0, 1, 2} <= set(info[:, 0].tolist())
    assert (1, 3) in {S.gate_step(r, 557) for r in np.flatnonzero(c.gate["inside"][557:65557]) + 557}
    votes = {s.id: S.oracle(S.build(s)) for s in S.VOTE_CASES}
    # query 3 (column 2, a > 0): voters 198, 199 | 200 ...: scene 0 with one voter, scene 1 from seven on
    assert [int(votes[f"vote_all_top{v}"].scene_info[3, 0]) for v in (1, 7, 64)] == [0, 1, 1]
    assert votes["vote_all_top64"].scene_info[3].tolist() == [1, 56]
    # query 11 (column 2, a < 0) sees the two-valued zeros first; query 2 / 5 elect over the lattice load
    assert len({tuple(v.q_scene.tolist()) for v in votes.values()}) > 1


# ---- the oracle and the emulation -----------------------------------------------------------------------------------------------
LATTICE = S.PLAN_CASES[:8] + S.TILE_CASES + S.QUERY_CASES[:4]


@pytest.mark.parametrize("spec", LATTICE, ids=[s.id for s in LATTICE])
def test_lattice_oracle_equals_the_float64_rule(spec):
    c = S.build(spec)
    # float64 similarities from the exact integer dots: equal dots stay equal (cosine_f64 normalises the rows first, so its last
    # bit breaks a tie by rounding noise, not by row) -- and they are cosine_f64's to the last few bits
    q64, d64 = c.q.astype(np.float64), c.db.astype(np.float64)
    s64 = c.score / np.sqrt((q64 * q64).sum(1))[:, None] / np.sqrt((d64 * d64).sum(1))[None, :]
    assert np.abs(s64 - R.cosine_f64(c.q, c.db)).max() < 1e-14
    assert np.array_equal(S.oracle(c).nbrs, R.retrieve_ref(c.q, c.db, c.ranks, sims=s64))
    s32 = (c.q @ c.db.T) * S._inv_norms(c.q)[:, None] * S._inv_norms(c.db)[None, :]
    for j in range(c.g):                                              # fp32 order == integer order, equal dots bit-equal
        assert len(set(s32[j].tolist())) == len(set(c.score[j].tolist()))
        assert np.array_equal(np.lexsort((np.arange(c.m), -s32[j])), np.lexsort((np.arange(c.m), -c.score[j])))


def test_integer_oracle_equals_the_existing_references():
    c = S.build(S.SELECT_CASES[[s.id for s in S.SELECT_CASES].index("select_m1025_spread")])
    sims = np.where(c.nonfinite, np.nan, c.score.astype(np.float64))
    fixed = np.stack([S.clamp_ranks(c.ranks[j], len(S.oracle(c).allowed[j]))[0] for j in range(c.g)])
    assert np.array_equal(S.oracle(c).nbrs, R.retrieve_ref(c.q, c.db, fixed, c.q_group, c.db_group, sims=sims))
    c = S.build(S.GATE_CASES[-1])
    info, used = G.gated_rows(c.gate["db_gate"], c.gate["prior"], c.gate["r2"], None, c.ranks, c.q_group, c.db_group)
    want = S.oracle(c)
    assert np.array_equal(info, want.gate_info)
    assert all(np.array_equal(np.flatnonzero(used[j]), want.allowed[j]) for j in range(c.g))
    assert np.array_equal(G.gate_mask(c.gate["db_gate"], c.gate["prior"][0], 1.0), c.gate["inside"])
    first = S.atlas_first()
    for voters in ([198, 199, 200], [255, 256, 0, 256], [66256, 65556, 65557], [5], []):
        assert S.vote_int(voters, first, 66257) == SV.vote(voters, first, 66257)


ALL_EXACT = [s for v in S.EXACT_LISTS.values() for s in v]


@pytest.mark.parametrize("spec", ALL_EXACT, ids=[s.id for s in ALL_EXACT])
def test_emulation_without_a_defect_passes(spec):
    c = S.build(spec)
    want = S.oracle(c)
    for fill in (float("nan"), 0.0):
        assert S.check_exact(c, S.emulate(c, fill=fill), want) == [], (spec.id, spec.why, fill)


FLOAT_SMALL = [s for s in S.FLOAT_CASES if "m148" not in s.id]


@pytest.mark.parametrize("spec", FLOAT_SMALL, ids=[s.id for s in FLOAT_SMALL])
def test_emulation_passes_the_float_bound(spec):
    c = S.build(spec)
    bad, fig = S.check_float(c, S.emulate(c))
    assert bad == [], (spec.id, bad, fig)


# cases that must fail a defect by name, beyond "some case of each list meant to pin it": the paths the issue names
MUST_FAIL = {"drop_block": ("plan_m100_d6340",), "ragged_float4": ("plan_m17_d60", "plan_m100_d6340"),
             "last_slice_out": ("plan_m40_d1028", "plan_m1489_d6340"), "tail_column_stored": ("tile_m17", "plan_m1489_d6340"),
             "mislaid_tile": ("queries_g17", "queries_g33", "queries_g65"), "ignore_digit16": ("select_m65537_R2",),
             "gate_lane3": ("gate_m3073_plain", "gate_m8200_groups"), "vote_beyond_top": ("vote_all_top1", "vote_lost_top7")}


def _fails(spec, defect):
    c = S.build(spec)
    return any(S.check_exact(c, S.emulate(c, defect=defect, fill=fill)) for fill in (float("nan"), 0.0))


@pytest.mark.parametrize("defect", list(S.PINNED_BY), ids=list(S.PINNED_BY))
def test_each_planted_defect_fails_a_case_meant_to_pin_it(defect):
    every = {s.id: s for v in S.EXACT_LISTS.values() for s in v}
    for name in S.PINNED_BY[defect]:                                  # every list named for it holds a case that fails
        assert any(_fails(spec, defect) for spec in S.EXACT_LISTS[name]), (defect, name)
    for cid in MUST_FAIL.get(defect, ()):
        assert _fails(every[cid], defect), (defect, cid)


def test_dot_defects_fail_the_float_bound_too():
    c = S.build(S.FLOAT_CASES[[s.id for s in S.FLOAT_CASES].index("float_trajectory_m100_d6340")])
    for defect in ("drop_block", "ragged_float4", "last_slice_out"):
        assert S.check_float(c, S.emulate(c, defect=defect))[0], defect


def test_the_unmasked_skip_is_unobservable():
    """A skipped digit that is not added to the mask changes nothing (every row and the prefix hold 0 there): the emulation says so
    on every selection, scope and vote case, which is why PINNED_BY holds the skip by range length in its place."""
    assert set(S.PINNED_BY) | set(S.UNOBSERVABLE) == set(S.DEFECTS)
    for spec in S.SELECT_CASES[::5] + S.SCOPE_CASES + S.VOTE_CASES[:2]:
        c = S.build(spec)
        a, b = S.emulate(c), S.emulate(c, defect="unmasked_skip")
        assert np.array_equal(a.nbrs, b.nbrs) and np.array_equal(a.sims.view(np.uint32), b.sims.view(np.uint32)), spec.id


def test_keys_order_as_the_rule_says():
    s = np.array([1.0, 0.5, 1e-45, 0.0, -0.0, -1e-45, -0.5, -1.0, np.inf, -np.inf, np.nan], dtype=np.float32)
    k = S.sim_keys(s)
    assert k[3] == k[4] and (np.diff(k[:4].astype(np.int64)) > 0).all() and (np.diff(k[4:8].astype(np.int64)) > 0).all()
    assert (k[8:] == S.KEY_NONFINITE).all() and k[7] < S.KEY_NONFINITE
    back = S.key_sims(k)
    assert np.array_equal(back[:8], s[:8] + np.float32(0)) and np.isnan(back[8:]).all() and not np.signbit(back[4])
