"""The scene vote without a GPU: the election rule in integers on hand-written cases, the margins of the clustered descriptors
that the GPU tests' known elections rest on, the new entry point's argument checks through ctypes, its symbols, and every
refusal of ``retrieval.SceneVote`` that needs no device."""
import os
import re

import numpy as np
import pytest
import torch

import scene_ref as SR
import scene_vote_ref as VR

META = {"feat_dim": 8, "precision": "f32", "encoder_digest": "abc"}


def test_vote_hand_written():
    first = [0, 10, 20, 30]
    assert VR.vote([14], first) == (1, 1)                                     # V = 1: the best row's scene
    assert VR.vote([3, 25, 4, 11, 5], first) == (0, 3)                        # a clear majority
    # 2 : 2, and scene 2 owns the best-placed voter: it wins although scene 0 has the lower index
    assert VR.vote([21, 1, 2, 29], first) == (2, 2)
    assert VR.vote([1, 21, 29, 2], first) == (0, 2)
    # a row no scene owns does not vote: rows >= 30 here, and the gap of boundaries that start above 0
    assert VR.vote([35, 36, 12], first) == (1, 1)
    assert VR.vote([2, 3, 12], [5, 10, 20]) == (1, 1)
    assert VR.vote([35, 36], first) == (-1, 0)                                # no voter at all
    assert VR.vote([], first) == (-1, 0)
    # boundaries clamped into [0, m] as the scoped entry clamps them: [0, 37), [37, 149), an empty third scene
    raw = [-5, 37, 10 ** 12, 3]
    assert VR.vote([0, 36, 37], raw, m=149) == (0, 2)
    assert VR.vote([148, 40, 2], raw, m=149) == (1, 2)


@pytest.mark.parametrize("d,margin", [(64, 0.22), (2048, 0.70)])
def test_clustered_elects_the_truth(d, margin):
    g = 70
    truth = np.arange(g) % len(SR.SIZES)
    own = SR.scene_of_rows()[None, :] == truth[:, None]
    first = SR.scene_first()
    for seed in range(20):
        q, db = VR.clustered(d, g, seed)
        assert q.dtype == np.float32 and db.dtype == np.float32
        for dtype in (np.float64, np.float32):
            sim = VR.cosines(q, db, dtype)
            gap = np.where(own, sim, np.inf).min(axis=1) - np.where(own, -np.inf, sim).max(axis=1)
            assert gap.min() >= margin, (seed, dtype, gap.min())
        for top in (1, 7):
            voters = VR.voters_ref(sim, top)                                  # (fp32 here)
            got = [VR.vote(v, first) for v in voters]
            assert [s for s, _ in got] == truth.tolist(), (seed, top)
            assert all(n == min(top, SR.SIZES[t]) for (_, n), t in zip(got, truth)), (seed, top)


def test_symbols_are_declared_and_exported():
    from relpose_gnn_amd import _lib
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "relpose_gnn_hip.h")).read()
    lib = _lib.lib()
    for name in ("rpg_retrieve_elect_workspace_bytes", "rpg_retrieve_cosine_elect_f32"):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
        assert re.search(r"\b" + name + r"\(", header), name
    assert re.search(r"#define RPG_ELECT_ALL 1\b", header) and re.search(r"#define RPG_ELECT_LOST 2\b", header)
    from relpose_gnn_amd import retrieval
    assert (retrieval.ELECT_ALL, retrieval.ELECT_LOST) == (1, 2)
    for g, m, d in ((1, 8, 8), (70, 149, 2048), (64, 100000, 2048)):
        assert lib.rpg_retrieve_elect_workspace_bytes(g, m, d) >= lib.rpg_retrieve_workspace_bytes(g, m, d) + 4 * g * m
    assert lib.rpg_retrieve_elect_workspace_bytes(0, 8, 8) == 0


def test_argument_checks_come_before_any_launch():
    """Refused by the host-side check: nothing is launched, so host pointers serve as placeholders."""
    from relpose_gnn_amd import _lib
    lib, bad = _lib.lib(), _lib.RPG_ERR_BAD_ARG
    g, k, m, d = 2, 2, 8, 8
    q, db = torch.zeros(g, d), torch.zeros(m, d)
    ranks, nb = torch.zeros((g, k), dtype=torch.int32), torch.zeros((g, k), dtype=torch.int64)
    ws = torch.zeros(int(lib.rpg_retrieve_elect_workspace_bytes(g, m, d)) + 64, dtype=torch.uint8)
    status, info = torch.zeros(1, dtype=torch.int32), torch.zeros((g, 2), dtype=torch.int32)
    first, qs = torch.tensor([0, 4, 8], dtype=torch.int64), torch.zeros(g, dtype=torch.int32)
    gate = torch.zeros((m, 7), dtype=torch.float64)
    wp = (ws.data_ptr() + 15) & ~15

    def elect(first_p=first.data_ptr(), qs_p=qs.data_ptr(), n=2, top=2, mode=1, info_p=info.data_ptr(), m_=m, k_=k, gate_p=None,
              prior_p=None, ginfo_p=None, r2=0.0, ws_bytes=ws.numel() - 16):
        return lib.rpg_retrieve_cosine_elect_f32(q.data_ptr(), db.data_ptr(), None, None, None, ranks.data_ptr(), g, k_, m_, d, gate_p,
                                                 prior_p, r2, 0.0, 0, ginfo_p, first_p, qs_p, n, top, mode, info_p, nb.data_ptr(),
                                                 None, wp, ws_bytes, status.data_ptr(), None)
    assert elect(first_p=None) == bad and elect(qs_p=None) == bad and elect(info_p=None) == bad
    assert elect(first_p=None, qs_p=None) == bad                              # the scopes are not optional here
    assert elect(n=0) == bad and elect(n=-1) == bad
    for top in (0, -1, 65, 9):                                                # outside [1, 64], above m = 8
        assert elect(top=top) == bad, top
    for mode in (0, 3, -1):
        assert elect(mode=mode) == bad, mode
    assert elect(first_p=first.data_ptr() + 4) == bad                         # alignment
    assert elect(qs_p=qs.data_ptr() + 2) == bad and elect(info_p=info.data_ptr() + 2) == bad
    assert elect(m_=1) == bad and elect(k_=65) == bad and elect(k_=0) == bad  # everything the scoped entry refuses
    assert elect(gate_p=gate.data_ptr()) == bad                               # the gate's three pointers go together
    assert elect(gate_p=gate.data_ptr(), prior_p=gate.data_ptr(), ginfo_p=info.data_ptr(), r2=-1.0) == bad
    for mode in (1, 2):                                                       # a valid call gets as far as the workspace check
        assert elect(mode=mode, top=8, ws_bytes=int(lib.rpg_retrieve_workspace_bytes(g, m, d))) == _lib.RPG_ERR_WORKSPACE


def test_scene_vote_arguments():
    from relpose_gnn_amd.retrieval import SceneVote
    v = SceneVote()
    assert (v.top, v.lost_only, v.mode) == (16, False, 1) and SceneVote(7, lost_only=True).mode == 2
    assert SceneVote(1).top == 1 and SceneVote(64).top == 64
    assert v.key == SceneVote(16).key and v.key != SceneVote(7).key and v.key != SceneVote(16, True).key
    assert hash(v.key) is not None and "16" in repr(v)
    for bad in (0, -1, 65, 2.5, True):
        with pytest.raises(ValueError, match="top"):
            SceneVote(bad)
    with pytest.raises(ValueError, match="lost_only"):
        SceneVote(4, lost_only=1)


def _atlas(sizes=(5, 9, 4)):
    from relpose_gnn_amd.featmap import FeatureMap, SceneAtlas
    gen = torch.Generator().manual_seed(0)
    return SceneAtlas.concat([FeatureMap(torch.randn(n, 8, generator=gen), META, poses=torch.randn(n, 6, generator=gen),
                                         groups=torch.arange(n) % 3) for n in sizes])


def test_scope_takes_a_vote_and_refuses_what_it_cannot_serve():
    from relpose_gnn_amd.retrieval import RetrievalRule, SceneVote
    atlas = _atlas()
    vote = SceneVote(7)
    assert atlas._scope(vote, 3, RetrievalRule(k=4), "retrieve") == (None, None, vote)
    with pytest.raises(ValueError, match="random"):
        atlas._scope(vote, 3, RetrievalRule.reference(k=3, seed=1), "retrieve")
    with pytest.raises(ValueError, match="random"):
        atlas._scope(vote, 3, RetrievalRule(k=3, drop=0.5), "retrieve")
    with pytest.raises(ValueError, match="smallest scene"):
        atlas._scope(vote, 3, RetrievalRule(k=5), "retrieve")
    with pytest.raises(ValueError, match="18"):                               # top above the atlas's row count
        atlas._scope(SceneVote(19), 3, RetrievalRule(k=3), "retrieve")
    with pytest.raises(ValueError, match="lost_only"):
        atlas._scope(SceneVote(7, lost_only=True), 3, RetrievalRule(k=3), "retrieve")
    lost = SceneVote(7, lost_only=True)
    assert atlas._scope(lost, 3, RetrievalRule(k=3), "Tracker", lost_ok=True) == (None, None, lost)
    # the ranks of a vote are checked against the smallest scene, as for scenes on the device only
    assert atlas.n_allowed(None, 3, None).tolist() == [4, 4, 4]


def test_refusals_without_a_device():
    from relpose_gnn_amd import ops
    from relpose_gnn_amd.retrieval import RetrievalRule, SceneVote
    atlas = _atlas()
    q = torch.zeros(3, 8)
    with pytest.raises(ValueError, match="SceneAtlas"):                       # one scene's map refuses a vote as it refuses scenes
        atlas.scene(0).retrieve(q, RetrievalRule(k=3), scenes=SceneVote(3))
    with pytest.raises(ValueError, match="random"):
        atlas.retrieve(q, RetrievalRule.reference(k=3, seed=0), scenes=SceneVote(3))
    with pytest.raises(ValueError, match="lost_only"):
        atlas.retrieve(q, RetrievalRule(k=3), scenes=SceneVote(3, lost_only=True))
    with pytest.raises(ValueError, match="18"):
        atlas.retrieve(q, RetrievalRule(k=3), scenes=SceneVote(19))
    with pytest.raises(ValueError, match="scene_info"):
        atlas.retrieve(q, RetrievalRule(k=3), scenes=[0, 1, 2], scene_info=torch.zeros((3, 2), dtype=torch.int32))
    db, ranks, first = torch.zeros(8, 8), torch.zeros((3, 2), dtype=torch.int32), torch.tensor([0, 4, 8])
    for top in (0, 65, 9):
        with pytest.raises(ValueError, match="top"):
            ops.retrieve_elect(q, db, ranks, first, top)
    with pytest.raises(ValueError, match="go together"):
        ops.retrieve_elect(q, db, ranks, first, 2, db_gate=torch.zeros((8, 7), dtype=torch.float64))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.retrieve_elect(q, db, ranks, first, 2)
