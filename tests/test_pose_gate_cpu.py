"""Pose-gated retrieval and the tracking loop without a GPU: the numpy statement of the gate (tests/pose_gate_ref.py) on hand
cases, csrc/pose_gate.h compiled by the host compiler against it bit for bit, the update rule on a table of its branches, and
the argument checks of the Python layers (all made before any launch)."""
import os

import numpy as np
import pytest
import torch

import pose_gate_ref as R
from conftest import ROOT

NEW_SYMBOLS = ("rpg_retrieve_cosine_gated_f32", "rpg_track_update_f64")
Q0 = np.array([1.0, 0.0, 0.0, 0.0])


def _row(t, q=Q0):
    return np.concatenate([np.asarray(t, dtype=np.float64), np.asarray(q, dtype=np.float64)])


# ---- the gate, by hand -------------------------------------------------------------------------------------------------------
def test_row_exactly_on_the_radius_is_inside():
    prior = _row((1.0, 2.0, 3.0))
    db = np.stack([_row((4.0, 6.0, 3.0)), _row((4.0, 6.0, 3.0 + 1e-7))])      # offsets (3, 4, 0): d2 = 25 exactly; a hair beyond
    assert R.gate_mask(db, prior, 5.0 * 5.0).tolist() == [True, False]


def test_radius_zero_with_the_prior_on_a_row():
    prior = _row((0.25, -7.0, 1e3))
    db = np.stack([prior, _row((0.25, -7.0, np.nextafter(1e3, 2e3)))])
    assert R.gate_mask(db, prior, 0.0).tolist() == [True, False]


def test_antipodal_quaternion_is_the_same_rotation():
    q = R.quat_about_z(33.0)
    db = np.stack([_row((0, 0, 0), q), _row((0, 0, 0), -q)])
    assert R.gate_mask(db, _row((0, 0, 0), q), 1.0, float(np.cos(np.deg2rad(1.0 / 2.0)))).tolist() == [True, True]


def test_rotation_exactly_at_max_deg():
    """The row's quaternion is (cos(max_deg / 2), 0, 0, sin) from the SAME expression the gate's cos_half comes from, the prior
    the identity: the dot is that cosine itself, times 1.0, plus zeros -- equal, and >= is inclusive."""
    from relpose_gnn_amd.retrieval import PoseGate
    for deg in (0.0, 10.0, 33.3, 90.0, 179.0, 180.0):
        gate = PoseGate(1.0, deg)
        assert gate.cos_half == float(np.cos(np.deg2rad(deg / 2.0)))
        db = np.stack([_row((0, 0, 0), R.quat_about_z(deg)), _row((0, 0, 0), R.quat_about_z(deg + 0.5))])
        want = [True, deg + 0.5 > 180.0]            # past 180 degrees |dot| grows again: the same rotation the other way round
        assert R.gate_mask(db, _row((0, 0, 0)), gate.r2, gate.cos_half).tolist() == want, deg


def test_nan_prior_is_state_one_and_nan_row_is_outside():
    db = np.stack([_row((0, 0, 0)), _row((0, np.nan, 0)), _row((0, 0, 0), (1.0, np.inf, 0, 0)), _row((0, 0, 0), (np.nan, 0, 0, 0))])
    assert R.gate_mask(db, _row((0, 0, 0)), 1.0).tolist() == [True, False, False, False]      # (no rotation gate: still outside)
    assert R.gate_mask(db, _row((0, 0, 0)), 1.0, 0.5).tolist() == [True, False, False, False]
    prior = _row((0, 0, 0))
    for i in range(7):
        p = prior.copy()
        p[i] = np.nan if i % 2 else np.inf
        info, used = R.gated_rows(db, p[None], 1.0, None, [[0]])
        assert info.tolist() == [[1, 0]] and used.all()


def test_need_boundary_and_groups_combined():
    db = np.stack([_row((float(i), 0, 0)) for i in range(8)])
    mask = R.gate_mask(db, _row((0, 0, 0)), 3.0 * 3.0)                          # rows 0..3
    assert mask.tolist() == [True] * 4 + [False] * 4
    allowed = np.ones(8, dtype=bool)
    state, inside, used = R.gate_decision(mask, allowed, 4)                     # rows_inside == need: gated
    assert (state, inside, used.tolist()) == (0, 4, mask.tolist())
    state, inside, used = R.gate_decision(mask, allowed, 5)                     # rows_inside == need - 1: fallback
    assert (state, inside, used.all()) == (2, 4, True)
    groups = np.array([5, 5, 0, 0, 0, 0, 5, 0])
    info, used = R.gated_rows(db, np.stack([_row((0, 0, 0))] * 3), 9.0, None, [[0, 1], [0, 2], [0, 1]], [5, 5, -1], groups)
    assert info.tolist() == [[0, 2], [2, 2], [0, 4]]
    assert used[0].tolist() == [False, False, True, True, False, False, False, False]       # gate AND groups
    assert used[1].tolist() == (groups != 5).tolist()                                       # groups alone
    assert used[2].tolist() == mask.tolist()


# ---- the header on the host -----------------------------------------------------------------------------------------------------
def _near_radius_cases(n, seed):
    """Rows whose d2 lies within a few ulp of r2, on both sides and on it: a random offset, r2 = its d2 moved by -3..3 ulp."""
    rng = np.random.RandomState(seed)
    prior = np.concatenate([rng.randn(n, 3) * 10.0, rng.randn(n, 4)], 1)
    prior[:, 3:] /= np.linalg.norm(prior[:, 3:], axis=1, keepdims=True)
    rows = np.concatenate([prior[:, :3] + rng.randn(n, 3) * rng.choice([1e-3, 1.0, 50.0], (n, 1)), rng.randn(n, 4)], 1)
    rows[:, 3:] /= np.linalg.norm(rows[:, 3:], axis=1, keepdims=True)
    dx, dy, dz = (rows[:, i] - prior[:, i] for i in range(3))
    d2 = (dx * dx + dy * dy) + dz * dz
    r2 = d2.copy()
    for i, step in enumerate(rng.randint(-3, 4, n)):
        for _ in range(abs(int(step))):
            r2[i] = np.nextafter(r2[i], np.inf if step > 0 else -np.inf)
    # the rotation side: cos_half within a few ulp of |dot| for half the cases, no rotation gate for a quarter
    dot = np.abs(((rows[:, 3] * prior[:, 3] + rows[:, 4] * prior[:, 4]) + rows[:, 5] * prior[:, 5]) + rows[:, 6] * prior[:, 6])
    cos_half = np.where(rng.rand(n) < 0.5, dot, rng.rand(n))
    for i, step in enumerate(rng.randint(-2, 3, n)):
        for _ in range(abs(int(step))):
            cos_half[i] = np.nextafter(cos_half[i], np.inf if step > 0 else -np.inf)
    rot = rng.rand(n) < 0.75
    return rows, prior, np.maximum(r2, 0.0), cos_half, rot


def _special_cases():
    nan, inf = np.nan, np.inf
    p0 = _row((1.0, 2.0, 3.0))
    out = [(_row((4.0, 6.0, 3.0)), p0, 25.0, 0.0, False), (p0, p0, 0.0, 1.0, True), (_row((1, 2, 3), -Q0), p0, 0.0, 1.0, True),
           (_row((nan, 2, 3)), p0, inf, 0.0, False), (_row((1, 2, 3), (inf, 0, 0, 0)), p0, 1.0, 0.0, False),
           (_row((1, 2, 3), (inf, 0, 0, 0)), p0, 1.0, 0.5, True), (p0, _row((1, nan, 3)), 1.0, 0.0, False),
           (p0, _row((1, 2, 3), (1, 0, inf, 0)), 1.0, 0.0, False), (_row((1e200, 0, 0)), _row((-1e200, 0, 0)), 1e308, 0.0, False),
           (p0, p0, 1.0, -1.0, True)]
    return out


def test_header_on_the_host_equals_numpy(tmp_path):
    """csrc/pose_gate.h is plain C++: the host compiler builds tests/pose_gate_check.cpp with -Wall -Wextra -Werror (and without
    contraction, as the kernel's pragma asks); the program's verdict on 12 000 rows whose d2 lies within 3 ulp of r2 -- and its
    update of every row of the table below -- must be the numpy statement's, bit for bit."""
    import shutil
    import subprocess
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "pose_gate_check")
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "pose_gate_check.cpp")], check=True)
    rows, prior, r2, cos_half, rot = _near_radius_cases(12000, 5)
    cases = [(rows[i], prior[i], r2[i], cos_half[i], bool(rot[i])) for i in range(rows.shape[0])] + _special_cases()
    lines, want = [], []
    for row, pr, rr, ch, ro in cases:
        lines.append(" ".join(["g", R.bits(rr), R.bits(ch), str(int(ro))] + [R.bits(v) for v in row] + [R.bits(v) for v in pr]))
        has = bool(R.finite7(pr))
        want.append(f"g {int(has)} {int(has and bool(R.gate_mask(row[None], pr, rr, ch if ro else None)[0]))}")
    for case in UPDATE_TABLE:
        pose, i, u, pr, lost, mi, mr, ml = case[:8]
        lines.append(" ".join(["u", str(mi), R.bits(mr), str(ml), str(i), str(u), str(lost)] + [R.bits(v) for v in pose]
                              + [R.bits(v) for v in pr]))
        p, l, a = R.track_update_ref(pose[None], [i], [u], pr[None], [lost], mi, mr, ml)
        want.append(" ".join(["u", str(int(a[0])), str(int(l[0]))] + [R.bits(v) for v in p[0]]))
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr
    got = run.stdout.splitlines()
    assert got[-1] == f"pose_gate: ok {len(lines)}"
    assert got[:-1] == want
    # the generated cases do sit on both sides of the radius, and on it
    verdicts = [w.split()[2] for w in want[:12000]]
    assert 3000 < verdicts.count("1") < 9000


# ---- the update rule ---------------------------------------------------------------------------------------------------------
POSE = _row((0.5, -1.5, 2.0), R.quat_about_z(20.0))
OLD = _row((9.0, 9.0, 9.0))
NANS = np.full(7, np.nan)
BAD = POSE.copy()
BAD[5] = np.inf
# pose, inliers, used, prior, lost, min_inliers, min_ratio, max_lost -> accepted, lost, prior
UPDATE_TABLE = [
    (POSE, 3, 4, OLD, 2, 2, 0.5, 3, 1, 0, POSE),                   # accepted: the pose is the prior, lost returns to 0
    (POSE, 2, 4, OLD, 0, 2, 0.5, 3, 1, 0, POSE),                   # the ratio boundary: 2 == 0.5 * 4 is accepted
    (POSE, 3, 7, OLD, 0, 2, 0.5, 3, 0, 1, OLD),                    # 3 < 3.5: not accepted, the prior stays
    (POSE, 1, 1, OLD, 0, 2, 0.5, 3, 0, 1, OLD),                    # too few inliers, whatever the ratio
    (POSE, 2, 2, OLD, 0, 2, 1.0, 3, 1, 0, POSE),                   # min_inliers boundary, ratio 1
    (BAD, 4, 4, OLD, 1, 2, 0.5, 3, 0, 2, OLD),                     # a non-finite pose is never accepted
    (NANS, 0, 0, OLD, 2, 0, 0.0, 3, 0, 3, OLD),                    # lost == max_lost: the prior is kept one more frame
    (NANS, 0, 0, OLD, 3, 0, 0.0, 3, 0, 4, NANS),                   # lost passes max_lost: the prior is forgotten
    (POSE, 0, 3, OLD, 0, 1, 0.0, 0, 0, 1, NANS),                   # max_lost = 0: the first lost frame forgets it
    (POSE, 0, 0, NANS, 7, 0, 0.5, 3, 1, 0, POSE),                  # min_inliers 0, used 0: 0 >= 0 -- a finite pose recovers a lost camera
    (POSE, 1, 4, NANS, R.INT32_MAX, 2, 0.5, 3, 0, R.INT32_MAX, NANS),      # lost saturates
    (POSE, 1, 4, OLD, R.INT32_MAX - 1, 2, 0.5, 3, 0, R.INT32_MAX, NANS),
]


def test_track_update_table():
    for n, (pose, i, u, prior, lost, mi, mr, ml, acc, lost_after, prior_after) in enumerate(UPDATE_TABLE):
        p, l, a = R.track_update_ref(pose[None], [i], [u], prior[None], [lost], mi, mr, ml)
        assert (int(a[0]), int(l[0])) == (acc, lost_after), n
        assert np.array_equal(p[0], prior_after, equal_nan=True), n
    # S cameras at once are S cameras one by one
    poses, priors = np.stack([c[0] for c in UPDATE_TABLE[:6]]), np.stack([c[3] for c in UPDATE_TABLE[:6]])
    p, l, a = R.track_update_ref(poses, [c[1] for c in UPDATE_TABLE[:6]], [c[2] for c in UPDATE_TABLE[:6]], priors,
                                 [c[4] for c in UPDATE_TABLE[:6]], 2, 0.5, 3)
    assert a.tolist() == [1, 1, 0, 0, 1, 0] and l.tolist() == [0, 0, 1, 1, 0, 2]


# ---- the library and the Python layers -----------------------------------------------------------------------------------------
def test_symbols_declared_and_exported():
    from relpose_gnn_amd import _lib
    header = open(os.path.join(ROOT, "include", "relpose_gnn_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS and f"int {name}(" in header
        getattr(_lib.lib(), name)
    assert "relpose-gnn_amd/csrc/pose_gate.h".split("/")[-1] in os.listdir(os.path.join(ROOT, "relpose-gnn_amd", "csrc"))


def test_launchers_refuse_bad_arguments_before_any_launch():
    """Null / half-given gate pointers and a radius that is no number: RPG_ERR_BAD_ARG, decided on the host."""
    import ctypes as C
    from relpose_gnn_amd import _lib
    lib = _lib.lib()
    buf = (C.c_char * 4096)()
    a = C.addressof(buf)                        # 16-byte alignment is not guaranteed: round up
    a = (a + 15) // 16 * 16
    args = lambda dbg, pr, info, r2=1.0: (a, a, None, None, None, a, 1, 1, 4, 4, dbg, pr, r2, 0.0, 0, info, a, None, a, 1 << 20, a, None)
    for dbg, pr, info in ((a, None, None), (None, a, None), (None, None, a), (a, a, None), (a + 4, a, a)):
        assert lib.rpg_retrieve_cosine_gated_f32(*args(dbg, pr, info)) == _lib.RPG_ERR_BAD_ARG
    assert lib.rpg_retrieve_cosine_gated_f32(*args(a, a, a, r2=float("nan"))) == _lib.RPG_ERR_BAD_ARG
    assert lib.rpg_retrieve_cosine_gated_f32(*args(a, a, a, r2=-1.0)) == _lib.RPG_ERR_BAD_ARG
    assert lib.rpg_track_update_f64(None, a, 1, 2, 0.5, 3, a, a, a, None) == _lib.RPG_ERR_BAD_ARG
    assert lib.rpg_track_update_f64(a, a, 0, 2, 0.5, 3, a, a, a, None) == _lib.RPG_ERR_BAD_ARG
    assert lib.rpg_track_update_f64(a, a, 1, 2, float("nan"), 3, a, a, a, None) == _lib.RPG_ERR_BAD_ARG


def test_pose_gate_ranges():
    from relpose_gnn_amd.retrieval import PoseGate
    g = PoseGate(2.5, 90.0, pose_m=(1, 2, 3), pose_s=(2, 2, 2))
    assert g.r2 == 6.25 and isinstance(g.r2, float) and isinstance(g.cos_half, float) and g.rot
    assert g.cos_half == float(np.cos(np.deg2rad(45.0)))
    assert PoseGate(0.0).r2 == 0.0 and not PoseGate(0.0).rot
    assert PoseGate(1.0, 0.0).cos_half == 1.0 and PoseGate(1.0, 360.0).cos_half == -1.0
    assert PoseGate(1.0, 30.0).key == PoseGate(1.0, 30.0).key != PoseGate(1.0, 31.0).key
    for radius in (-1e-9, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="radius"):
            PoseGate(radius)
    for deg in (-0.1, 360.1, float("nan")):
        with pytest.raises(ValueError, match="max_deg"):
            PoseGate(1.0, deg)


def _host_map(poses=True, groups=None):
    from relpose_gnn_amd.featmap import FeatureMap
    feats = torch.randn(6, 32, generator=torch.Generator().manual_seed(1))
    return FeatureMap(feats, {"feat_dim": 32, "precision": "f32", "encoder_digest": "0" * 16},
                      poses=torch.randn(6, 6, generator=torch.Generator().manual_seed(2)) if poses else None, groups=groups)


def test_gate_rows_are_the_rows_of_the_pose_rule_and_are_cached():
    from relpose_gnn_amd.evaluate import qexp
    from relpose_gnn_amd.retrieval import PoseGate
    fmap = _host_map()
    gate = PoseGate(1.0, pose_m=(1.0, -2.0, 0.5), pose_s=(2.0, 0.5, 3.0))
    rows = fmap.gate_rows(gate)
    assert rows.dtype == torch.float64 and tuple(rows.shape) == (6, 7)
    p = fmap.poses.numpy().astype(np.float64)
    for i in range(6):
        assert np.array_equal(rows[i, :3].numpy(), p[i, :3] * np.array(gate.pose_s) + np.array(gate.pose_m))
        assert np.array_equal(rows[i, 3:].numpy(), qexp(p[i, 3:]))
    assert fmap.gate_rows(PoseGate(7.0, 10.0, pose_m=gate.pose_m, pose_s=gate.pose_s)) is rows      # per (pose_m, pose_s)
    assert fmap.gate_rows(PoseGate(1.0)) is not rows
    fmap._append(torch.randn(2, 32), torch.randn(2, 6), None, None)
    assert not fmap._gate_rows and tuple(fmap.gate_rows(gate).shape) == (8, 7)                       # dropped like _inv_norms
    with pytest.raises(ValueError, match="holds no poses"):
        _host_map(poses=False).gate_rows(gate)


def test_argument_checks_of_the_layers():
    from relpose_gnn_amd.posenet import PoseNetX_R2
    from relpose_gnn_amd.query_pose import QueryPose
    from relpose_gnn_amd.resnet import ResNet
    from relpose_gnn_amd.retrieval import PoseGate, RetrievalRule
    from relpose_gnn_amd.tracking import Tracker
    fmap, gate = _host_map(), PoseGate(1.0, 30.0)
    q, prior = torch.randn(2, 32), torch.full((2, 7), float("nan"), dtype=torch.float64)
    with pytest.raises(ValueError, match="random draws"):
        fmap.retrieve(q, RetrievalRule.reference(k=2, sampling_period=1, seed=0), prior=prior, gate=gate)
    with pytest.raises(ValueError, match="go together"):
        fmap.retrieve(q, RetrievalRule(k=2), prior=prior)
    with pytest.raises(ValueError, match="go together"):
        fmap.retrieve(q, RetrievalRule(k=2), gate=gate)
    with pytest.raises(ValueError, match="holds no poses"):
        _host_map(poses=False).retrieve(q, RetrievalRule(k=2), prior=prior, gate=gate)
    with pytest.raises(ValueError, match=r"prior must be floating point \[2, 7\]"):
        fmap.retrieve(q, RetrievalRule(k=2), prior=prior[:1], gate=gate)
    model = PoseNetX_R2(ResNet((1, 1, 1, 1), (8, 16, 32, 64)), pretrained=False, feat_dim=32, edge_feat_dim=32, node_dim=32,
                        input_img_height=64, use_gnn=True, droprate=0.0, knn=-1, use_AP=True, gnn_recursion=2)
    nb = torch.zeros((2, 2), dtype=torch.int64)
    with pytest.raises(ValueError, match="pose gate restricts retrieval"):
        model.forward_map(torch.zeros(2, 3, 64, 64), nb, fmap, prior=prior, gate=gate)
    with pytest.raises(ValueError, match="random draws"):
        model.forward_map(torch.zeros(2, 3, 64, 64), None, fmap, rule=RetrievalRule.reference(k=2, seed=0), prior=prior, gate=gate)
    for pose in (QueryPose(), QueryPose(fuse="mean"), QueryPose(fuse="median"), None):
        with pytest.raises(ValueError, match="fuse='consensus'"):
            Tracker(model, fmap, RetrievalRule(k=2), gate, pose, capture=False)
    cons = QueryPose(fuse="consensus")
    with pytest.raises(ValueError, match="random draws"):
        Tracker(model, fmap, RetrievalRule.reference(k=2, seed=0), gate, cons, capture=False)
    with pytest.raises(ValueError, match="holds no poses"):
        Tracker(model, _host_map(poses=False), RetrievalRule(k=2), gate, cons, capture=False)
    with pytest.raises(ValueError, match="min_ratio"):
        Tracker(model, fmap, RetrievalRule(k=2), gate, cons, min_ratio=1.5, capture=False)
    with pytest.raises(ValueError, match="example frames"):
        Tracker(model, fmap, RetrievalRule(k=2), gate, cons, capture=True)
