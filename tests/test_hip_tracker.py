"""tracking.Tracker on the GPU: the captured loop equals the eager loop equals a host-driven loop -- which reads every frame's
rows back, applies tests/pose_gate_ref.py's update rule and hands the prior to forward_map(prior=...) explicitly -- bit for bit on
rows, inliers, accepted, gate_info and neighbours at every one of 12 frames.

The scene is built so that the sequence must visit every state.  The map has two parts: rows 0..11 packed within 0.11 units
(place A), rows 12..23 a million units apart (place B); the map's own retrieval descriptors point at e0 for A and e1 for B, and a
frame's descriptor says which place it looks like.  The consensus thresholds are wide open, so every finite frame is accepted;
a frame of NaN pixels gives a NaN pose and is not.  A camera then goes: no prior (state 1) -> accepted in A -> gated (state 0),
where a frame that LOOKS like B is still matched inside the gate -> two NaN frames, max_lost = 1: lost, the prior forgotten ->
state 1, a B frame accepted far from everything -> too few rows inside (state 2)."""
import numpy as np
import pytest
import torch

import pose_gate_ref as R

pytestmark = pytest.mark.gpu

H = W = 64
M, K, FRAMES = 24, 3, 12
PM, PS = (0.5, -0.25, 1.0), (2.0, 0.5, 1.25)
MIN_INLIERS, MIN_RATIO, MAX_LOST = 2, 0.5, 1
# per frame what a camera sees: "A" / "B" = a finite frame whose descriptor looks like that place, "n" = NaN pixels
SCRIPTS = ["AABnnBBAnABA", "AAAAAAAAAAAA", "BBnnAAABnnBA"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _small(dev, **kw):
    from test_hip_pose_gate_map import _small as small
    return small(dev, **kw)


@pytest.fixture(scope="module")
def scene():
    import relpose_gnn_amd.synth as S
    gen = torch.Generator().manual_seed(4)
    poses = torch.zeros(M, 6)
    poses[:12, 0] = torch.arange(12, dtype=torch.float32) * 0.005
    poses[12:, 0] = (torch.arange(12, dtype=torch.float32) + 1.0) * 1e6
    poses[:, 3:] = torch.randn(M, 3, generator=gen) * 0.05
    desc = torch.randn(M, 8, generator=gen) * 0.05
    desc[:12, 0] += 1.0
    desc[12:, 1] += 1.0
    frames = S.synth_images(FRAMES * 3, H, W, seed=93).reshape(FRAMES, 3, -1)
    qdesc = torch.randn(FRAMES, 3, 8, generator=gen) * 0.05
    for s, script in enumerate(SCRIPTS):
        for f, c in enumerate(script):
            qdesc[f, s, 0 if c == "A" else 1] += 1.0 if c != "n" else 0.0
            qdesc[f, s, f % 2] += 1.0 if c == "n" else 0.0          # (a NaN frame still has a descriptor)
            if c == "n":
                frames[f, s] = float("nan")
    return dict(mimgs=S.synth_images(M, H, W, seed=91), poses=poses, desc=desc, frames=frames, qdesc=qdesc)


def _setup(dev, scene, **model_kw):
    from relpose_gnn_amd.featmap import FeatureMap
    from relpose_gnn_amd.retrieval import PoseGate, RetrievalRule
    m = _small(dev, **model_kw)
    fmap = FeatureMap.build(m, scene["mimgs"], poses=scene["poses"], descriptors=scene["desc"])
    return m, fmap, RetrievalRule(k=K), PoseGate(1000.0, pose_m=PM, pose_s=PS)


def _pose():
    from relpose_gnn_amd.query_pose import QueryPose
    return QueryPose(PM, PS, fuse="consensus", inlier_t=1e12, inlier_deg=360.0)


def _snapshot(out):
    return [t.clone() for t in (out.rows, out.inliers, out.accepted, out.gate_info, out.neighbours)]


def _host_loop(dev, m, fmap, rule, gate, frames, qdesc, per_node):
    """The loop with the host in it: every frame's rows come back, the update rule runs in numpy, the prior goes in explicitly.
    ``frames`` [F, S, ...], ``qdesc`` [F, S, 8]."""
    pose = _pose()
    s = frames.shape[1]
    prior, lost = np.full((s, 7), np.nan), np.zeros(s, dtype=np.int32)
    edge_first = torch.arange(s + 1, dtype=torch.int64, device=dev) * per_node
    out, states = [], []
    for f in range(frames.shape[0]):
        ab, rel, ei, nb = m.forward_map(frames[f].to(dev), None, fmap, rule=rule, query_descriptors=qdesc[f].to(dev),
                                        outputs="query", prior=prior, gate=gate)
        info = m.gate_info
        rows, ints, _, _ = pose.output_block(s, dev)
        pose.from_map(rel, ei, fmap, nb, edge_first=edge_first, out=rows, inliers=ints)
        rows_h, ints_h = rows.cpu().numpy(), ints.cpu().numpy()
        prior, lost, acc = R.track_update_ref(rows_h[:, :7], ints_h[:, 0], ints_h[:, 1], prior, lost, MIN_INLIERS, MIN_RATIO, MAX_LOST)
        out.append([rows.clone(), ints.clone(), torch.as_tensor(acc).to(dev), info.clone(), nb.clone()])
        states.append((info.cpu().numpy()[:, 0].copy(), acc.copy(), lost.copy(), np.isnan(prior).any(1)))
    return out, states


def _same(a, b, what):
    assert len(a) == len(b)
    for f, (x, y) in enumerate(zip(a, b)):
        for name, u, v in zip(("rows", "inliers", "accepted", "gate_info", "neighbours"), x, y):
            if u.dtype == torch.float64:                       # bit for bit, NaN rows included
                u, v = u.view(torch.int64), v.view(torch.int64)
            assert torch.equal(u, v), (what, f, name)


def _trackers(dev, m, fmap, rule, gate, frames, qdesc, states):
    """The eager and the captured tracker over the sequence -> {capture: per-frame snapshots}; their final state must be the
    host loop's, and reset() must give a stream its next frame without a prior."""
    from relpose_gnn_amd.tracking import Tracker
    s = frames.shape[1]
    results = {}
    for capture in (False, True):
        tr = Tracker(m, fmap, rule, gate, _pose(), streams=s, min_inliers=MIN_INLIERS, min_ratio=MIN_RATIO, max_lost=MAX_LOST,
                     capture=capture, example=frames[0].to(dev), query_descriptors=qdesc[0].to(dev))
        st = tr.state()
        assert np.isnan(st["prior"]).all() and not st["lost"].any()            # (the capture's warm-up left nothing behind)
        results[capture] = [_snapshot(tr.step(frames[f].to(dev), qdesc[f].to(dev))) for f in range(frames.shape[0])]
        st = tr.state()
        assert np.array_equal(st["lost"], states[-1][2]) and np.array_equal(st["accepted"], states[-1][1])
        assert np.array_equal(np.isnan(st["prior"]).any(1), states[-1][3])
        assert not np.isnan(st["prior"]).all()
        tr.reset([0])                                          # stream 0's next frame has no prior again
        info = tr.step(frames[0].to(dev), qdesc[0].to(dev)).gate_info.cpu().numpy()
        assert info[0].tolist() == [1, 0]
        tr.reset()
        assert np.isnan(tr.state()["prior"]).all() and not tr.state()["lost"].any()
    return results


@pytest.mark.parametrize("which", [[0], [0, 1, 2]], ids=["S1", "S3"])
def test_captured_equals_eager_equals_host_loop(dev, scene, which):
    m, fmap, rule, gate = _setup(dev, scene)
    frames, qdesc = scene["frames"][:, which], scene["qdesc"][:, which]
    host, states = _host_loop(dev, m, fmap, rule, gate, frames, qdesc, K)
    # the sequence is not vacuous: every gate state, a camera that is lost past max_lost and accepted again afterwards
    seen = np.concatenate([st[0] for st in states])
    assert {0, 1, 2} == set(seen.tolist())
    acc0 = [int(st[1][0]) for st in states]
    forgot = [bool(st[3][0]) for st in states]
    assert acc0.count(0) >= 3 and any(forgot[f] and 1 in acc0[f + 1:] for f in range(1, FRAMES - 1))
    assert any(int(st[0][0]) == 1 for st in states[1:])                        # ... relocalised against the whole map again
    assert int(states[2][0][0]) == 0 and int(host[2][4][0].max()) < 12        # the B look-alike frame stayed inside the gate (A)
    results = _trackers(dev, m, fmap, rule, gate, frames, qdesc, states)
    _same(results[False], host, "eager vs host loop")
    _same(results[True], results[False], "captured vs eager")
    m.check_edge_index()


def test_static_knn_model_is_tracked(dev, scene):
    """A knn > 0 model with static_knn, where GraphedForwardMap accepts it: four finite frames of the camera that stays in A (a
    NaN frame would be an irregular kNN graph, which that model reports on its own)."""
    m, fmap, rule, gate = _setup(dev, scene, knn=2, static_knn=True)
    frames, qdesc = scene["frames"][:4, [1]], scene["qdesc"][:4, [1]]
    host, states = _host_loop(dev, m, fmap, rule, gate, frames, qdesc, 2)
    assert [int(st[0][0]) for st in states] == [1, 0, 0, 0] and all(int(st[1][0]) for st in states)
    results = _trackers(dev, m, fmap, rule, gate, frames, qdesc, states)
    _same(results[False], host, "eager vs host loop")
    _same(results[True], results[False], "captured vs eager")
    m.check_edge_index()


def test_step_checks_its_frames(dev, scene):
    from relpose_gnn_amd.tracking import Tracker
    m, fmap, rule, gate = _setup(dev, scene)
    tr = Tracker(m, fmap, rule, gate, _pose(), streams=2, capture=False)
    with pytest.raises(ValueError, match="one per stream"):
        tr.step(scene["frames"][0, :3].to(dev), scene["qdesc"][0, :3].to(dev))
    with pytest.raises(IndexError):
        tr.reset([2])
