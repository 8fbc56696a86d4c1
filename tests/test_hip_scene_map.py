"""A SceneAtlas through the map path on the GPU: forward_map(rule=, scenes=) on mixed uint8 queries against
forward_map(neighbours=<the oracle's rows>) on the queries transformed scene by scene, bit for bit (both output modes, a
static_knn model, the gate); relocalize(scenes=) eager and captured; a GraphedForwardMap whose static scenes change between
replays; a Tracker whose camera moves to another scene against a host-driven loop; and every refusal.  The small model of
tests/test_hip_pose_gate_map.py; the retrieval oracle of tests/scene_ref.py."""
import numpy as np
import pytest
import torch

import pose_gate_ref as R
import scene_ref as SR

pytestmark = pytest.mark.gpu

H, W = 64, 64
FH, FW = 80, 100                   # camera frames: Resize(64) makes them 64 x 80
SIZES = (9, 14, 7)
M, K, G, MB = sum(SIZES), 3, 6, 4
SCENES = [2, 0, 1, 1, 0, 2]
PM, PS = (1.5, -0.25, 3.0), (2.0, 0.5, 1.25)
MEANS = ((0.485, 0.456, 0.406), (0.1, 0.7, 0.3), (0.52, 0.5, 0.9))
STDS = ((0.229, 0.224, 0.225), (0.5, 0.25, 1.75), (0.3, 0.31, 0.27))
RESULT_FIELDS = ("pred_poses", "targ_poses", "t_loss", "q_loss", "neighbours")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _small(dev, **kw):
    from test_hip_pose_gate_map import _small as small
    return small(dev, **kw)


@pytest.fixture(scope="module")
def data():
    """Per scene a line of map poses one unit apart in normalised x, the scenes 100 units apart; groups of three rows."""
    import relpose_gnn_amd.synth as S
    gen = torch.Generator().manual_seed(8)
    poses = torch.zeros(M, 6)
    first = SR.scene_first(SIZES)
    for s, n in enumerate(SIZES):
        poses[first[s]:first[s + 1], 0] = torch.arange(n, dtype=torch.float32) + 100.0 * s
    poses[:, 1:3] = torch.randn(M, 2, generator=gen) * 0.05
    poses[:, 3:] = torch.randn(M, 3, generator=gen) * 0.05
    return dict(mimgs=S.synth_images(M, H, W, seed=95), poses=poses, groups=torch.arange(M) // 3,
                frames=torch.randint(0, 256, (G, FH, FW, 3), generator=gen, dtype=torch.uint8),
                targets=torch.randn(G, 6, generator=gen) * 0.3)


def _sft():
    from relpose_gnn_amd.frames import SceneFrameTransform
    return SceneFrameTransform(H, MEANS, STDS)


def _atlas(model, data, groups=False):
    from relpose_gnn_amd.featmap import FeatureMap, SceneAtlas
    first = SR.scene_first(SIZES)
    maps = [FeatureMap.build(model, data["mimgs"][a:b], poses=data["poses"][a:b], groups=data["groups"][a:b] if groups else None)
            for a, b in zip(first[:-1], first[1:])]
    return SceneAtlas.concat(maps, names=["chess", "fire", "heads"])


def _by_scene(dev, frames, scenes):
    """The queries transformed scene by scene through the plain FrameTransform of each: fp32 [n, 3, 64, 80]."""
    sft = _sft()
    out = torch.empty((frames.shape[0], 3, *sft.output_size(FH, FW)), dtype=torch.float32, device=dev)
    for i, s in enumerate(scenes):
        out[i:i + 1] = sft.scene(s).apply(frames[i:i + 1].to(dev))
    return out


def _oracle_rows(dev, model, atlas, rule, qx, scenes, q_groups=None, gate=None, prior=None):
    g = qx.shape[0]
    ranks = torch.from_numpy(rule.ranks([min(SIZES)] * g)).to(dev)
    gt = None
    if gate is not None:
        gt = (atlas.gate_rows(gate), torch.as_tensor(prior, dtype=torch.float64).to(dev), gate.r2, gate.cos_half, gate.rot)
    nb, _, info, status = SR.oracle(dev, model.encode(qx), atlas.features, ranks, SIZES, scenes, q_groups,
                                    None if q_groups is None else atlas.groups_host.numpy(), gate=gt)
    assert status == 0
    return nb.to(dev), info


def _gate():
    from relpose_gnn_amd.retrieval import PoseGate
    return PoseGate(5.0, pose_m=PM, pose_s=PS)                # +-2 rows of a scene's line (4 units): 5 rows inside


def _priors(atlas, gate, scenes):
    """Query i's prior: row 3 of its scene a little displaced (gated) -- query 1 has none, query 2's is far away (fallback),
    query 3's lies in ANOTHER scene's room: none of its own scene's rows is inside (fallback), whatever that room holds."""
    rows = atlas.gate_rows(gate).cpu().numpy()
    prior = rows[[int(atlas.scene_first_host[s]) + 3 for s in scenes]].copy()
    prior[:, :3] += 0.01
    prior[1] = np.nan
    prior[2, 1] += 500.0
    prior[3] = rows[int(atlas.scene_first_host[(scenes[3] + 1) % len(SIZES)]) + 3]
    return prior


@pytest.mark.parametrize("kind", ["fc", "static_knn"])
@pytest.mark.parametrize("outputs", ["all", "query"])
@pytest.mark.parametrize("gated", [False, True])
def test_forward_map_scenes_equals_given_oracle_neighbours(dev, data, outputs, kind, gated):
    from relpose_gnn_amd.retrieval import RetrievalRule
    m = _small(dev, **({"knn": 2, "static_knn": True} if kind == "static_knn" else {}))
    m.frame_transform = _sft()
    atlas, rule = _atlas(m, data, groups=True), RetrievalRule(k=K)
    frames = data["frames"].to(dev)
    qx = _by_scene(dev, data["frames"], SCENES)
    qg = [-1, 0, -1, 4, -1, -1]                               # group ids of the atlas: 0 = rows 0..2 (scene 0), 4 = rows 12..14 (scene 1)
    gate = _gate() if gated else None
    prior = _priors(atlas, gate, SCENES) if gated else None
    nb_ref, info = _oracle_rows(dev, m, atlas, rule, qx, SCENES, qg, gate, prior)
    gkw = dict(prior=prior, gate=gate) if gated else {}
    ab, rel, ei, nb = m.forward_map(frames, None, atlas, rule=rule, query_groups=qg, outputs=outputs, scenes=SCENES, **gkw)
    if gated:
        assert torch.equal(m.gate_info.cpu(), info) and info[:, 0].tolist() == [0, 1, 2, 2, 0, 0]
    want = m.forward_map(qx, nb_ref, atlas, outputs=outputs)
    assert torch.equal(nb, nb_ref)
    for u, v in zip((ab, rel, ei), want):
        assert torch.equal(u, v)
    assert torch.isfinite(rel).all()
    first = atlas.scene_first_host
    for row, s in zip(nb.tolist(), SCENES):
        assert all(first[s] <= r < first[s + 1] for r in row)
    # given neighbours: scenes only feed the frame transform; the int32 device form serves both
    sc_dev = torch.tensor(SCENES, dtype=torch.int32, device=dev)
    again = m.forward_map(frames, nb_ref, atlas, outputs=outputs, scenes=sc_dev)
    assert torch.equal(again[1], rel)
    again = m.forward_map(frames, None, atlas, rule=rule, query_groups=qg, outputs=outputs, scenes=sc_dev, **gkw)
    assert torch.equal(again[3], nb) and torch.equal(again[1], rel)
    assert torch.equal(m.encode(frames, scenes=SCENES), m.encode(qx))
    m.check_edge_index()


@pytest.mark.parametrize("postprocess", ["host", "device"])
def test_relocalize_scenes_eager_and_captured(dev, data, postprocess):
    """Two micro-batches, the second ragged.  Eager on the uint8 frames; captured on the transformed queries (frames stay outside
    a graph); both against relocalize(neighbours=<the oracle's rows>) on the queries transformed scene by scene."""
    from relpose_gnn_amd.evaluate import relocalize
    from relpose_gnn_amd.retrieval import RetrievalRule
    m = _small(dev)
    m.frame_transform = _sft()
    atlas, rule = _atlas(m, data), RetrievalRule(k=K)
    qx = _by_scene(dev, data["frames"], SCENES)
    nb_ref, _ = _oracle_rows(dev, m, atlas, rule, qx, SCENES)
    kw = dict(micro_batch=MB, pose_m=PM, pose_s=PS, targets=data["targets"], postprocess=postprocess, outputs="query")
    want = relocalize(m, atlas, qx.cpu(), nb_ref.cpu(), **kw)
    st_c = {}
    eager = relocalize(m, atlas, data["frames"], rule=rule, scenes=SCENES, **kw)
    cap = relocalize(m, atlas, qx.cpu(), rule=rule, scenes=np.asarray(SCENES), capture=True, stats=st_c, **kw)
    assert st_c["graphs_captured"] == 2 and st_c["graph_replays"] == 2
    for f in RESULT_FIELDS:
        for got in (eager, cap):
            x, y = getattr(got, f), getattr(want, f)
            assert x.shape == y.shape and np.array_equal(x, y), f
    assert np.isfinite(eager.pred_poses).all()
    # the held steps serve other scenes without a new capture
    other = [1, 1, 2, 0, 2, 0]
    st = {}
    again = relocalize(m, atlas, qx.cpu(), rule=rule, scenes=other, capture=True, stats=st, **kw)
    assert st["graphs_captured"] == 0
    assert np.array_equal(again.neighbours, _oracle_rows(dev, m, atlas, rule, qx, other)[0].cpu().numpy())
    with pytest.raises(ValueError, match="scenes"):
        relocalize(m, atlas, qx.cpu(), rule=rule, **kw)
    m.check_edge_index()


def test_graphed_step_follows_its_static_scenes(dev, data):
    from relpose_gnn_amd.graphed import GraphedForwardMap
    from relpose_gnn_amd.retrieval import RetrievalRule
    m = _small(dev)
    atlas, rule = _atlas(m, data), RetrievalRule(k=K)
    qx = _by_scene(dev, data["frames"], SCENES)
    step = GraphedForwardMap(m, atlas, qx, rule=rule, outputs="query", scenes=SCENES)
    assert step.scenes.dtype == torch.int32 and step.scenes.tolist() == SCENES
    graph = step.graph

    def same(out, scenes):
        got = [t.clone() for t in (out.abs_pose, out.rel_pose, out.edge_index, out.neighbours)]
        want = m.forward_map(qx, None, atlas, rule=rule, outputs="query", scenes=scenes)
        for u, v in zip(got, want):
            assert torch.equal(u, v)
        assert torch.equal(got[3], _oracle_rows(dev, m, atlas, rule, qx, scenes)[0])

    same(step(qx), SCENES)
    other = [0, 1, 2, 0, 1, 2]
    same(step(qx, scenes=other), other)                       # copied into the static tensor ...
    same(step(qx), other)                                     # ... where it stays
    third = [1, 2, 0, 2, 0, 1]
    step.scenes.copy_(torch.tensor(third, dtype=torch.int32)) # written on the device by someone else (a tracker's move)
    same(step(qx), third)
    assert not step.stale() and step.graph is graph           # no new capture
    with pytest.raises(IndexError):
        step(qx, scenes=[0, 1, 2, 0, 1, 3])
    with pytest.raises(ValueError, match="captured without"):
        GraphedForwardMap(m, atlas.scene(0), qx, rule=rule, outputs="query")(qx, scenes=SCENES)
    m.check_edge_index()


def test_tracker_moves_a_camera_to_another_scene(dev, data):
    """Two cameras, six frames; camera 0 stands in scene 1 and is moved to scene 2 ahead of frame 3, camera 1 stays in scene 0.
    The eager and the captured tracker against a loop with the host in it (pose_gate_ref's update rule, the prior handed to
    forward_map explicitly, a move = that camera's prior and lost count forgotten): bit for bit at every frame."""
    from relpose_gnn_amd.query_pose import QueryPose
    from relpose_gnn_amd.retrieval import RetrievalRule
    from relpose_gnn_amd.tracking import Tracker
    m = _small(dev)
    atlas, rule, gate = _atlas(m, data), RetrievalRule(k=K), _gate()
    pose = lambda: QueryPose(PM, PS, fuse="consensus", inlier_t=1e12, inlier_deg=360.0)
    s, n_frames, move_at = 2, 6, 3
    start, moved = [1, 0], [2, 0]
    frames = _by_scene(dev, data["frames"].repeat(2, 1, 1, 1), [0] * 12).reshape(n_frames, s, 3, H, -1)

    # ---- the host-driven loop of the eager pieces
    qp = pose()
    prior, lost = np.full((s, 7), np.nan), np.zeros(s, dtype=np.int32)
    edge_first = torch.arange(s + 1, dtype=torch.int64, device=dev) * K
    host, states, scenes = [], [], list(start)
    for f in range(n_frames):
        if f == move_at:
            scenes = list(moved)
            prior[0], lost[0] = np.nan, 0
        ab, rel, ei, nb = m.forward_map(frames[f], None, atlas, rule=rule, outputs="query", prior=prior, gate=gate, scenes=scenes)
        info = m.gate_info
        rows, ints, _, _ = qp.output_block(s, dev)
        qp.from_map(rel, ei, atlas, nb, edge_first=edge_first, out=rows, inliers=ints)
        rows_h, ints_h = rows.cpu().numpy(), ints.cpu().numpy()
        prior, lost, acc = R.track_update_ref(rows_h[:, :7], ints_h[:, 0], ints_h[:, 1], prior, lost, 2, 0.5, 1)
        host.append([rows.clone(), ints.clone(), torch.as_tensor(acc).to(dev), info.clone(), nb.clone()])
        states.append(info.cpu().numpy()[:, 0].tolist())
        first = atlas.scene_first_host
        assert all(first[c] <= r < first[c + 1] for row, c in zip(nb.tolist(), scenes) for r in row)
    # camera 0: no prior, then gated or fallen back inside scene 1; no prior again right after the move
    assert states[0] == [1, 1] and states[move_at][0] == 1 and all(st[0] != 1 for st in states[1:move_at])

    for capture in (False, True):
        tr = Tracker(m, atlas, rule, gate, pose(), streams=s, min_inliers=2, min_ratio=0.5, max_lost=1, capture=capture,
                     example=frames[0], scenes=start)
        graph = tr._step.graph if capture else None
        for f in range(n_frames):
            if f == move_at:
                tr.move(0, moved[0])
            out = tr.step(frames[f])
            for name, u, v in zip(("rows", "inliers", "accepted", "gate_info", "neighbours"),
                                  (out.rows, out.inliers, out.accepted, out.gate_info, out.neighbours), host[f]):
                if u.dtype == torch.float64:
                    u, v = u.view(torch.int64), v.view(torch.int64)
                assert torch.equal(u, v), (capture, f, name)
        assert tr.scenes.tolist() == moved
        if capture:
            assert tr._step.graph is graph and not tr._step.stale()
        with pytest.raises(IndexError):
            tr.move(0, len(SIZES))
        with pytest.raises(IndexError):
            tr.move(s, 0)
    m.check_edge_index()


def test_refusals(dev, data):
    from relpose_gnn_amd.evaluate import relocalize
    from relpose_gnn_amd.graphed import GraphedForwardMap
    from relpose_gnn_amd.query_pose import QueryPose
    from relpose_gnn_amd.retrieval import RetrievalRule
    from relpose_gnn_amd.tracking import Tracker
    m = _small(dev)
    atlas, rule = _atlas(m, data), RetrievalRule(k=K)
    frames = data["frames"].to(dev)
    qx = _by_scene(dev, data["frames"], SCENES)
    nb = torch.zeros((G, K), dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match="scenes"):           # a rule on an atlas ranks inside scenes only
        m.forward_map(qx, None, atlas, rule=rule)
    with pytest.raises(ValueError, match="smallest scene"):
        m.forward_map(qx, None, atlas, rule=RetrievalRule(k=min(SIZES) + 1), scenes=SCENES)
    with pytest.raises(ValueError, match="host integers"):    # random draws are sized on the host
        m.forward_map(qx, None, atlas, rule=RetrievalRule.reference(k=K, sampling_period=1, seed=0),
                      scenes=torch.tensor(SCENES, dtype=torch.int32, device=dev))
    with pytest.raises(IndexError):
        m.forward_map(qx, None, atlas, rule=rule, scenes=[0, 1, 2, 3, 0, 1])
    with pytest.raises(ValueError):
        m.forward_map(qx, None, atlas, rule=rule, scenes=SCENES[:-1])
    with pytest.raises(ValueError, match="SceneAtlas"):       # one scene's map takes no scenes
        m.forward_map(qx, None, atlas.scene(1), rule=rule, scenes=SCENES)
    m.frame_transform = _sft()
    with pytest.raises(ValueError, match="scenes"):           # per-scene statistics need every frame's scene
        m.forward_map(frames, nb, atlas)
    with pytest.raises(ValueError, match="scenes"):
        m.encode(frames)
    m.frame_transform = None
    with pytest.raises(ValueError, match="scenes"):
        relocalize(m, atlas, qx.cpu(), rule=rule)
    with pytest.raises(ValueError, match="scenes"):
        GraphedForwardMap(m, atlas, qx, rule=rule, outputs="query")
    pose = QueryPose(PM, PS, fuse="consensus")
    with pytest.raises(ValueError, match="scenes"):
        Tracker(m, atlas, rule, _gate(), pose, streams=G, capture=False)
    with pytest.raises(ValueError, match="SceneAtlas"):
        Tracker(m, atlas.scene(1), rule, _gate(), pose, streams=G, capture=False).move(0, 1)
    with pytest.raises(NotImplementedError, match="concat"):
        atlas.extend(m, data["mimgs"][:2], poses=data["poses"][:2])
    m.check_edge_index()


BIG = (20, 30, 25)                 # scenes large enough for the reference's half-drop and a sampling period of 2 with K = 3


def _big_atlas(dev, model):
    from relpose_gnn_amd.featmap import FeatureMap, SceneAtlas
    gen = torch.Generator().manual_seed(12)
    meta = FeatureMap.model_meta(model)
    return SceneAtlas.concat([FeatureMap(torch.randn(n, 64, generator=gen).relu_().to(dev), meta, torch.randn(n, 6, generator=gen) * 0.1)
                              for n in BIG])


def _reference_rule():
    from relpose_gnn_amd.retrieval import RetrievalRule
    return RetrievalRule.reference(k=K, sampling_period=2, seed=0)       # a fresh generator: every user draws the same stream


@pytest.mark.parametrize("postprocess", ["host", "device"])
def test_relocalize_reference_rule_on_an_atlas_captured(dev, data, postprocess):
    """The reference's own rule (half-drop, random start: draws sized by each query's allowed rows INSIDE ITS SCENE, on the host,
    in query order) with host scenes: eager, captured, and the oracle's rows for the ranks the same seed draws."""
    from relpose_gnn_amd.evaluate import relocalize
    m = _small(dev)
    atlas = _big_atlas(dev, m)
    qx = _by_scene(dev, data["frames"], SCENES)
    ranks = _reference_rule().ranks(np.asarray(BIG)[SCENES])
    assert (ranks != np.arange(K)).any()                     # not the plain top-K the capture warms up with
    nb_ref, _, _, status = SR.oracle(dev, m.encode(qx), atlas.features, torch.from_numpy(ranks).to(dev), BIG, SCENES)
    assert status == 0
    kw = dict(micro_batch=MB, pose_m=PM, pose_s=PS, targets=data["targets"], postprocess=postprocess, outputs="query", scenes=SCENES)
    want = relocalize(m, atlas, qx.cpu(), nb_ref, **kw)
    eager = relocalize(m, atlas, qx.cpu(), rule=_reference_rule(), **kw)
    st = {}
    cap = relocalize(m, atlas, qx.cpu(), rule=_reference_rule(), capture=True, stats=st, **kw)
    assert st["graphs_captured"] == 2 and st["graph_replays"] == 2
    assert np.array_equal(eager.neighbours, nb_ref.numpy())
    for f in RESULT_FIELDS:
        for got in (eager, cap):
            x, y = getattr(got, f), getattr(want, f)
            assert x.shape == y.shape and np.array_equal(x, y), f
    m.check_edge_index()


def test_graphed_step_with_a_random_rule_needs_host_scenes(dev, data):
    from relpose_gnn_amd.graphed import GraphedForwardMap
    m = _small(dev)
    atlas = _big_atlas(dev, m)
    qx = _by_scene(dev, data["frames"], SCENES)
    sc_dev = torch.tensor(SCENES, dtype=torch.int32, device=dev)
    step = GraphedForwardMap(m, atlas, qx, rule=_reference_rule(), outputs="query", scenes=sc_dev)     # the capture draws nothing
    want = m.forward_map(qx, None, atlas, rule=_reference_rule(), outputs="query", scenes=SCENES)
    out = step(qx, scenes=SCENES)
    for u, v in zip((out.abs_pose, out.rel_pose, out.edge_index, out.neighbours), want):
        assert torch.equal(u, v)
    with pytest.raises(ValueError, match="host integers"):   # the draws are sized inside each query's scene: the host must know it
        step(qx)
    with pytest.raises(ValueError, match="host integers"):
        step(qx, scenes=sc_dev)
    ranks = _reference_rule().ranks(np.asarray(BIG)[SCENES])
    assert torch.equal(step(qx, ranks=ranks).neighbours, want[3])            # the caller's own ranks: the static scenes serve
    m.check_edge_index()


def test_scenes_for_the_frame_transform_alone_on_one_scenes_map(dev, data):
    """One scene's map with a rule, uint8 queries and per-scene statistics: scenes feed the transform, the map takes none."""
    from relpose_gnn_amd.evaluate import relocalize
    from relpose_gnn_amd.retrieval import RetrievalRule
    m = _small(dev)
    m.frame_transform = _sft()
    fmap, rule = _atlas(m, data).scene(1), RetrievalRule(k=K)
    frames, qx = data["frames"].to(dev), _by_scene(dev, data["frames"], SCENES)
    got = m.forward_map(frames, None, fmap, rule=rule, scenes=SCENES)
    want = m.forward_map(qx, None, fmap, rule=rule)
    for u, v in zip(got, want):
        assert torch.equal(u, v)
    a = relocalize(m, fmap, data["frames"], rule=rule, scenes=SCENES, micro_batch=MB, pose_m=PM, pose_s=PS)
    b = relocalize(m, fmap, qx.cpu(), rule=rule, micro_batch=MB, pose_m=PM, pose_s=PS)
    assert np.array_equal(a, b)
    with pytest.raises(ValueError, match="SceneAtlas"):       # fp32 queries: nothing reads the scenes
        m.forward_map(qx, None, fmap, rule=rule, scenes=SCENES)
    with pytest.raises(IndexError):                          # host scenes are checked against the transform's scenes
        m.forward_map(frames, None, fmap, rule=rule, scenes=[0, 1, 2, 3, 0, 1])
    m.check_edge_index()
