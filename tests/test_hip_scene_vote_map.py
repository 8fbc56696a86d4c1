"""A SceneVote through the map path on the GPU: forward_map / relocalize (eager and captured) / GraphedForwardMap / Tracker with
``scenes=SceneVote(...)`` against the same calls with the elected scenes given explicitly, bit for bit, and against
scene_vote_ref.oracle for what was elected.  The small model, atlas sizes and image sizes of tests/test_hip_scene_map.py, but
processed fp32 queries and an atlas with its own retrieval descriptors made like scene_vote_ref.clustered, so that the elected
scenes are known: query i's descriptor lies in the cluster of scene TRUTH[i]."""
import numpy as np
import pytest
import torch

import pose_gate_ref as R
import scene_ref as SR
import scene_vote_ref as VR

pytestmark = pytest.mark.gpu

H, W = 64, 80
SIZES = (9, 14, 7)
M, K, G, MB, D = sum(SIZES), 3, 6, 4, 64
TOP = 7                             # the smallest scene's size: a query of that scene gets all of its rows' votes
TRUTH = [i % len(SIZES) for i in range(G)]
PM, PS = (1.5, -0.25, 3.0), (2.0, 0.5, 1.25)
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
    """Map poses as in test_hip_scene_map.py (a line per scene, the scenes 100 units apart); descriptors: three clusters.  The
    margin that makes the elections certain is asserted here, on the host, in float64."""
    import relpose_gnn_amd.synth as S
    gen = torch.Generator().manual_seed(8)
    poses = torch.zeros(M, 6)
    first = SR.scene_first(SIZES)
    for s, n in enumerate(SIZES):
        poses[first[s]:first[s + 1], 0] = torch.arange(n, dtype=torch.float32) + 100.0 * s
    poses[:, 1:3] = torch.randn(M, 2, generator=gen) * 0.05
    poses[:, 3:] = torch.randn(M, 3, generator=gen) * 0.05
    qd, desc = VR.clustered(D, 2 * G, 2, SIZES)               # 2 G queries: the second half serves as "new queries"
    sim = VR.cosines(qd, desc, np.float64)
    own = SR.scene_of_rows(SIZES)[None, :] == (np.arange(2 * G) % len(SIZES))[:, None]
    assert (np.where(own, sim, np.inf).min(axis=1) - np.where(own, -np.inf, sim).max(axis=1)).min() > 0.1
    return dict(mimgs=S.synth_images(M, H, W, seed=95), poses=poses, desc=torch.from_numpy(desc), qd=torch.from_numpy(qd),
                queries=S.synth_images(2 * G, H, W, seed=96).reshape(2 * G, 3, H, W), targets=torch.randn(G, 6, generator=gen) * 0.3)


def _atlas(model, data):
    from relpose_gnn_amd.featmap import FeatureMap, SceneAtlas
    first = SR.scene_first(SIZES)
    return SceneAtlas.concat([FeatureMap.build(model, data["mimgs"][a:b], poses=data["poses"][a:b], descriptors=data["desc"][a:b])
                              for a, b in zip(first[:-1], first[1:])])


def _gate():
    from relpose_gnn_amd.retrieval import PoseGate
    return PoseGate(5.0, pose_m=PM, pose_s=PS)


def _priors(atlas, gate, scenes):
    """Query i's prior: row 3 of its scene a little displaced (gated); query 1 has none, query 2's is far away (fallback)."""
    rows = atlas.gate_rows(gate).cpu().numpy()
    prior = rows[[int(atlas.scene_first_host[s]) + 3 for s in scenes]].copy()
    prior[:, :3] += 0.01
    prior[1] = np.nan
    prior[2, 1] += 500.0
    return prior


def _oracle(dev, atlas, rule, qd, gate=None, prior=None, held=None):
    g = qd.shape[0]
    ranks = torch.from_numpy(rule.ranks([min(SIZES)] * g)).to(dev)
    gt = None
    if gate is not None:
        gt = (atlas.gate_rows(gate), torch.as_tensor(prior, dtype=torch.float64).to(dev), gate.r2, gate.cos_half, gate.rot)
    return VR.oracle(dev, qd, atlas.descriptors, ranks, SIZES, TOP, gate=gt, held=held)


@pytest.mark.parametrize("outputs", ["all", "query"])
@pytest.mark.parametrize("gated", [False, True])
def test_forward_map_vote_equals_the_elected_scenes_given(dev, data, outputs, gated):
    from relpose_gnn_amd.retrieval import RetrievalRule, SceneVote
    m = _small(dev)
    atlas, rule = _atlas(m, data), RetrievalRule(k=K)
    qx, qd = data["queries"][:G].to(dev), data["qd"][:G].to(dev)
    gate = _gate() if gated else None
    prior = _priors(atlas, gate, TRUTH) if gated else None
    gkw = dict(prior=prior, gate=gate) if gated else {}
    got = m.forward_map(qx, None, atlas, rule=rule, query_descriptors=qd, outputs=outputs, scenes=SceneVote(TOP), **gkw)
    info = m.scene_info.clone()
    ginfo = m.gate_info.clone() if gated else None
    assert info.dtype == torch.int32 and tuple(info.shape) == (G, 2) and info.is_cuda
    assert info[:, 0].tolist() == TRUTH and info[:, 1].tolist() == [TOP] * G
    want_rows = _oracle(dev, atlas, rule, qd, gate, prior)
    assert torch.equal(info.cpu(), want_rows[5]) and torch.equal(got[3].cpu(), want_rows[0]) and want_rows[3] == 0
    want = m.forward_map(qx, None, atlas, rule=rule, query_descriptors=qd, outputs=outputs, scenes=info[:, 0].tolist(), **gkw)
    assert m.scene_info is None                               # every call without a vote
    for u, v in zip(got, want):
        assert torch.equal(u, v)
    assert torch.isfinite(got[1]).all()
    if gated:
        assert torch.equal(ginfo, m.gate_info) and torch.equal(ginfo.cpu(), want_rows[2])
        assert ginfo[:, 0].tolist() == [0, 1, 2, 0, 0, 0]
    m.check_edge_index()


@pytest.mark.parametrize("kind", ["static_knn", "mc_dropout"])
def test_forward_map_vote_with_static_knn_and_mc_dropout(dev, data, kind):
    from relpose_gnn_amd.retrieval import RetrievalRule, SceneVote
    m = _small(dev, **({"knn": 2, "static_knn": True} if kind == "static_knn" else {"droprate": 0.5}))
    if kind == "mc_dropout":
        from relpose_gnn_amd.mc_dropout import McDropout
        m.mc_dropout = McDropout(samples=4, seed=3)
    atlas, rule = _atlas(m, data), RetrievalRule(k=K)
    qx, qd = data["queries"][:G].to(dev), data["qd"][:G].to(dev)
    if kind == "mc_dropout":
        m.mc_dropout.reset(0)
    got = m.forward_map(qx, None, atlas, rule=rule, query_descriptors=qd, outputs="query", scenes=SceneVote(TOP))
    assert m.scene_info[:, 0].tolist() == TRUTH
    if kind == "mc_dropout":
        m.mc_dropout.reset(0)
    want = m.forward_map(qx, None, atlas, rule=rule, query_descriptors=qd, outputs="query", scenes=TRUTH)
    for u, v in zip(got, want):
        assert torch.equal(u, v)
    m.check_edge_index()


@pytest.mark.parametrize("postprocess", ["host", "device"])
def test_relocalize_vote_eager_and_captured(dev, data, postprocess):
    """Two micro-batches, the second ragged: the same poses as with the scenes given, the elections in stats and on the result;
    a second captured call replays and captures nothing."""
    from relpose_gnn_amd.evaluate import relocalize
    from relpose_gnn_amd.retrieval import RetrievalRule, SceneVote
    m = _small(dev)
    atlas, rule = _atlas(m, data), RetrievalRule(k=K)
    qx, qd = data["queries"][:G], data["qd"][:G]
    kw = dict(micro_batch=MB, pose_m=PM, pose_s=PS, targets=data["targets"], postprocess=postprocess, outputs="query", rule=rule,
              query_descriptors=qd)
    want = relocalize(m, atlas, qx, scenes=TRUTH, **kw)
    votes = _oracle(dev, atlas, rule, qd.to(dev))[5].numpy()
    st_e, st_c, st_2 = {}, {}, {}
    eager = relocalize(m, atlas, qx, scenes=SceneVote(TOP), stats=st_e, **kw)
    cap = relocalize(m, atlas, qx, scenes=SceneVote(TOP), capture=True, stats=st_c, **kw)
    again = relocalize(m, atlas, qx, scenes=SceneVote(TOP), capture=True, stats=st_2, **kw)
    assert st_c["graphs_captured"] == 2 and st_c["graph_replays"] == 2
    assert st_2["graphs_captured"] == 0 and st_2["graph_replays"] == 2
    for got, st in ((eager, st_e), (cap, st_c), (again, st_2)):
        for f in RESULT_FIELDS:
            x, y = getattr(got, f), getattr(want, f)
            assert x.shape == y.shape and np.array_equal(x, y), f
        assert st["scene"].tolist() == TRUTH and np.array_equal(st["scene"], votes[:, 0])
        assert np.array_equal(st["scene_votes"], votes[:, 1]) and st["scene_votes"].shape == (G,)
        assert np.array_equal(got.scene, st["scene"]) and np.array_equal(got.scene_votes, st["scene_votes"])
    assert want.scene is None and want.scene_votes is None
    # another vote is another step
    st_3 = {}
    relocalize(m, atlas, qx, scenes=SceneVote(1), capture=True, stats=st_3, **kw)
    assert st_3["graphs_captured"] == 2 and st_3["scene"].tolist() == TRUTH and st_3["scene_votes"].tolist() == [1] * G
    m.check_edge_index()


def _same_step(m, atlas, rule, out, qx, qd, scenes, **gkw):
    got = [t.clone() for t in (out.abs_pose, out.rel_pose, out.edge_index, out.neighbours)]
    want = m.forward_map(qx, None, atlas, rule=rule, query_descriptors=qd, outputs="query", scenes=scenes, **gkw)
    for u, v in zip(got, want):
        assert torch.equal(u, v)


def test_graphed_step_elects_anew_on_every_replay(dev, data):
    from relpose_gnn_amd.graphed import GraphedForwardMap
    from relpose_gnn_amd.retrieval import RetrievalRule, SceneVote
    m = _small(dev)
    atlas, rule = _atlas(m, data), RetrievalRule(k=K)
    qx, qd = data["queries"][:G].to(dev), data["qd"][:G].to(dev)
    step = GraphedForwardMap(m, atlas, qx, rule=rule, query_descriptors=qd, outputs="query", scenes=SceneVote(TOP))
    assert step.scenes.dtype == torch.int32 and tuple(step.scenes.shape) == (G,)
    assert step.scene_info.dtype == torch.int32 and tuple(step.scene_info.shape) == (G, 2)
    graph = step.graph
    out = step(qx, query_descriptors=qd)
    assert step.scenes.tolist() == TRUTH and step.scene_info.tolist() == [[t, TOP] for t in TRUTH]
    assert m.scene_info is step.scene_info
    _same_step(m, atlas, rule, out, qx, qd, TRUTH)
    # new queries, of other scenes: queries G + 1 .. 2 G - 1 and G, whose clusters are TRUTH rolled by one
    ix = [G + (i + 1) % G for i in range(G)]
    qx2, qd2 = data["queries"][ix].to(dev), data["qd"][ix].to(dev)
    other = [(i + 1) % len(SIZES) for i in TRUTH]
    out = step(qx2, query_descriptors=qd2)
    assert step.scenes.tolist() == other and step.scene_info[:, 1].tolist() == [TOP] * G
    _same_step(m, atlas, rule, out, qx2, qd2, other)
    assert step.graph is graph and not step.stale()           # no new capture
    with pytest.raises(ValueError, match="every query elects"):
        step(qx, query_descriptors=qd, scenes=TRUTH)
    m.check_edge_index()


def test_graphed_step_lost_only_holds_what_it_elected(dev, data):
    from relpose_gnn_amd.graphed import GraphedForwardMap
    from relpose_gnn_amd.retrieval import RetrievalRule, SceneVote
    m = _small(dev)
    atlas, rule, gate = _atlas(m, data), RetrievalRule(k=K), _gate()
    qx, qd = data["queries"][:G].to(dev), data["qd"][:G].to(dev)
    step = GraphedForwardMap(m, atlas, qx, rule=rule, query_descriptors=qd, outputs="query", gate=gate,
                             scenes=SceneVote(TOP, lost_only=True))
    assert step.scenes.tolist() == [-1] * G and torch.isnan(step.prior).all()        # the warm-up left nothing behind
    graph = step.graph
    nan = np.full((G, 7), np.nan)
    out = step(qx, query_descriptors=qd)                      # no prior, scenes -1: everyone elects
    assert step.scenes.tolist() == TRUTH and step.scene_info.tolist() == [[t, TOP] for t in TRUTH]
    _same_step(m, atlas, rule, out, qx, qd, TRUTH, prior=nan, gate=gate)
    # descriptors of OTHER scenes, finite priors: held in the scenes of the first replay
    ix = [G + (i + 1) % G for i in range(G)]
    qx2, qd2 = data["queries"][ix].to(dev), data["qd"][ix].to(dev)
    other = [(i + 1) % len(SIZES) for i in TRUTH]
    prior = _priors(atlas, gate, TRUTH)
    prior[1], prior[2, 1] = prior[0], prior[2, 1] - 500.0     # all finite and near
    out = step(qx2, query_descriptors=qd2, prior=prior)
    assert step.scenes.tolist() == TRUTH and step.scene_info.tolist() == [[t, 0] for t in TRUTH]
    _same_step(m, atlas, rule, out, qx2, qd2, TRUTH, prior=prior, gate=gate)
    # camera 4's prior is lost, camera 0 is told to elect: those two move, the others stay
    prior[4] = np.nan
    out = step(qx2, query_descriptors=qd2, prior=prior, scenes=[-1] + TRUTH[1:])
    mixed = [other[i] if i in (0, 4) else TRUTH[i] for i in range(G)]
    assert step.scenes.tolist() == mixed
    assert step.scene_info.tolist() == [[mixed[i], TOP if i in (0, 4) else 0] for i in range(G)]
    _same_step(m, atlas, rule, out, qx2, qd2, mixed, prior=prior, gate=gate)
    assert step.graph is graph and not step.stale()
    with pytest.raises(IndexError):
        step(qx, query_descriptors=qd, scenes=[-2] + TRUTH[1:])
    with pytest.raises(IndexError):
        step(qx, query_descriptors=qd, scenes=[len(SIZES)] + TRUTH[1:])
    m.check_edge_index()


def test_tracker_finds_the_room_and_finds_it_again(dev, data):
    """Two cameras, ten frames.  Camera 1 stays in scene 0.  Camera 0 starts in scene 1; from frame 4 on its descriptors are
    scene 2's, and frames 4 and 5 are NaN images (the way through the door): it is held in scene 1 while its prior lives, loses
    it after the second rejected frame (max_lost = 1) and elects scene 2 at frame 6.  Against a loop with the host in it, built
    from what existed before the vote: the prior is read back, the cameras without one vote through the oracle, and the frame
    runs as forward_map(scenes=<explicit>, prior=, gate=) + QueryPose + pose_gate_ref's update rule.  Eager and captured."""
    from relpose_gnn_amd.query_pose import QueryPose
    from relpose_gnn_amd.retrieval import RetrievalRule, SceneVote
    from relpose_gnn_amd.tracking import Tracker
    m = _small(dev)
    atlas, rule, gate = _atlas(m, data), RetrievalRule(k=K), _gate()
    pose = lambda: QueryPose(PM, PS, fuse="consensus", inlier_t=1e12, inlier_deg=360.0)
    s, n_frames, door = 2, 10, 4
    # queries 1, 4, 7, 10 lie in scene 1's cluster, 2, 5, 8, 11 in scene 2's, 0, 3, 6, 9 in scene 0's
    cam0 = [1, 4, 7, 10, 2, 5, 8, 11, 2, 5]
    cam1 = [0, 3, 6, 9, 0, 3, 6, 9, 0, 3]
    frames = torch.stack([data["queries"][[a, b]] for a, b in zip(cam0, cam1)]).to(dev).contiguous()
    frames[door:door + 2, 0] = float("nan")
    qds = torch.stack([data["qd"][[a, b]] for a, b in zip(cam0, cam1)]).to(dev).contiguous()

    # ---- the host-driven loop
    qp = pose()
    prior, lost = np.full((s, 7), np.nan), np.zeros(s, dtype=np.int32)
    scenes = np.full(s, -1, dtype=np.int64)
    edge_first = torch.arange(s + 1, dtype=torch.int64, device=dev) * K
    host, elected_at = [], []
    for f in range(n_frames):
        elects = np.isnan(prior).any(axis=1) | (scenes == -1)
        info = np.stack([scenes, np.zeros(s, dtype=np.int64)], axis=1)
        if elects.any():
            voted = _oracle(dev, atlas, rule, qds[f])[5].numpy()
            info[elects] = voted[elects]
            scenes = info[:, 0].copy()
        elected_at.append(elects.tolist())
        ab, rel, ei, nb = m.forward_map(frames[f], None, atlas, rule=rule, query_descriptors=qds[f], outputs="query", prior=prior,
                                        gate=gate, scenes=scenes.tolist())
        ginfo = m.gate_info
        rows, ints, _, _ = qp.output_block(s, dev)
        qp.from_map(rel, ei, atlas, nb, edge_first=edge_first, out=rows, inliers=ints)
        rows_h, ints_h = rows.cpu().numpy(), ints.cpu().numpy()
        prior, lost, acc = R.track_update_ref(rows_h[:, :7], ints_h[:, 0], ints_h[:, 1], prior, lost, 2, 0.5, 1)
        host.append(dict(rows=rows.clone(), inliers=ints.clone(), accepted=torch.as_tensor(acc).to(dev), gate_info=ginfo.clone(),
                         neighbours=nb.clone(), scene_info=torch.as_tensor(info, dtype=torch.int32).to(dev),
                         scenes=scenes.tolist(), prior=prior.copy(), lost=lost.copy()))
    # the story the docstring tells
    assert elected_at[0] == [True, True] and not any(e for row in elected_at[1:door + 2] for e in row)
    assert elected_at[door + 2] == [True, False] and not any(e for row in elected_at[door + 3:] for e in row)
    assert [h["scenes"] for h in host] == [[1, 0]] * (door + 2) + [[2, 0]] * (n_frames - door - 2)

    for capture in (False, True):
        tr = Tracker(m, atlas, rule, gate, pose(), streams=s, min_inliers=2, min_ratio=0.5, max_lost=1, capture=capture,
                     example=frames[0], query_descriptors=qds[0], scenes=SceneVote(TOP))
        assert tr.scenes.tolist() == [-1, -1]
        graph = tr._step.graph if capture else None
        for f in range(n_frames):
            out = tr.step(frames[f], query_descriptors=qds[f])
            assert out._fields[-1] == "scene_info"
            for name in ("rows", "inliers", "accepted", "gate_info", "neighbours", "scene_info"):
                u, v = getattr(out, name), host[f][name]
                if u.dtype == torch.float64:
                    u, v = u.view(torch.int64), v.view(torch.int64)
                assert torch.equal(u, v), (capture, f, name)
            st = tr.state()
            assert tr.scenes.tolist() == host[f]["scenes"], (capture, f)
            assert np.array_equal(st["prior"].view(np.int64), host[f]["prior"].view(np.int64)), (capture, f)
            assert np.array_equal(st["lost"], host[f]["lost"]), (capture, f)
        if capture:
            assert tr._step.graph is graph and not tr._step.stale()
        # reset forgets the room too: the next frame elects it again, for that camera alone
        tr.reset([1])
        assert tr.scenes.tolist() == [2, -1]
        out = tr.step(frames[0], query_descriptors=qds[0])
        assert tr.scenes.tolist() == [2, 0] and out.scene_info.tolist() == [[2, 0], [0, TOP]]
        with pytest.raises(ValueError, match="finds the rooms itself"):
            tr.move(0, 1)
    m.check_edge_index()


def test_refusals(dev, data):
    from relpose_gnn_amd.evaluate import relocalize
    from relpose_gnn_amd.frames import FrameTransform, SceneFrameTransform
    from relpose_gnn_amd.graphed import GraphedForwardMap
    from relpose_gnn_amd.query_pose import QueryPose
    from relpose_gnn_amd.retrieval import RetrievalRule, SceneVote
    from relpose_gnn_amd.tracking import Tracker
    m = _small(dev)
    atlas, rule, vote = _atlas(m, data), RetrievalRule(k=K), SceneVote(TOP)
    qx, qd = data["queries"][:G].to(dev), data["qd"][:G].to(dev)
    kw = dict(rule=rule, query_descriptors=qd)
    random_rule = RetrievalRule.reference(k=K, sampling_period=1, seed=0)
    nb = torch.zeros((G, K), dtype=torch.int64, device=dev)
    frames = torch.zeros((G, 80, 100, 3), dtype=torch.uint8, device=dev)
    pose = QueryPose(PM, PS, fuse="consensus")
    rkw = dict(micro_batch=MB, pose_m=PM, pose_s=PS)
    # a rule with random draws
    with pytest.raises(ValueError, match="random"):
        m.forward_map(qx, None, atlas, rule=random_rule, query_descriptors=qd, scenes=vote)
    with pytest.raises(ValueError, match="random"):
        relocalize(m, atlas, qx.cpu(), rule=random_rule, query_descriptors=qd, scenes=vote, **rkw)
    with pytest.raises(ValueError, match="random"):
        GraphedForwardMap(m, atlas, qx, rule=random_rule, query_descriptors=qd, scenes=vote)
    # given neighbours
    with pytest.raises(ValueError, match="neighbours"):
        m.forward_map(qx, nb, atlas, scenes=vote)
    with pytest.raises(ValueError, match="neighbours"):
        relocalize(m, atlas, qx.cpu(), nb.cpu(), scenes=vote, **rkw)
    with pytest.raises(ValueError):
        GraphedForwardMap(m, atlas, qx, K, scenes=vote)
    # top above the atlas's row count
    with pytest.raises(ValueError, match=str(M)):
        m.forward_map(qx, None, atlas, scenes=SceneVote(M + 1), **kw)
    with pytest.raises(ValueError, match=str(M)):
        relocalize(m, atlas, qx.cpu(), scenes=SceneVote(M + 1), **kw, **rkw)
    # lost_only outside a step with static scenes, and without a gate
    lost = SceneVote(TOP, lost_only=True)
    with pytest.raises(ValueError, match="lost_only"):
        m.forward_map(qx, None, atlas, scenes=lost, **kw)
    with pytest.raises(ValueError, match="lost_only"):
        atlas.retrieve(qd, rule, scenes=lost)
    with pytest.raises(ValueError, match="lost_only"):
        relocalize(m, atlas, qx.cpu(), scenes=lost, **kw, **rkw)
    with pytest.raises(ValueError, match="lost_only"):
        GraphedForwardMap(m, atlas, qx, outputs="query", scenes=lost, **kw)
    # one scene's map
    with pytest.raises(ValueError, match="SceneAtlas"):
        m.forward_map(qx, None, atlas.scene(1), scenes=vote, **kw)
    with pytest.raises(ValueError, match="SceneAtlas"):
        Tracker(m, atlas.scene(1), rule, _gate(), pose, streams=G, capture=False, scenes=vote)
    # uint8 queries: per-scene statistics are refused, a plain transform is served
    m.frame_transform = SceneFrameTransform(H, ((0.5, 0.5, 0.5),) * 3, ((0.25, 0.25, 0.25),) * 3)
    with pytest.raises(ValueError, match="SceneFrameTransform"):
        m.forward_map(frames, None, atlas, scenes=vote, **kw)
    with pytest.raises(ValueError, match="SceneFrameTransform"):
        relocalize(m, atlas, frames.cpu(), scenes=vote, **kw, **rkw)
    m.frame_transform = FrameTransform(H, (0.5, 0.5, 0.5), (0.25, 0.25, 0.25))
    got = m.forward_map(frames, None, atlas, scenes=vote, **kw)
    assert m.scene_info[:, 0].tolist() == TRUTH
    want = m.forward_map(m.frame_transform.apply(frames), None, atlas, scenes=TRUTH, **kw)
    for u, v in zip(got, want):
        assert torch.equal(u, v)
    m.frame_transform = None
    # the tensor-level pieces
    info = torch.zeros((G, 2), dtype=torch.int32, device=dev)
    assert torch.equal(atlas.retrieve(qd, rule, scenes=vote, scene_info=info), want[3]) and info[:, 0].tolist() == TRUTH
    with pytest.raises(ValueError, match="scene_info"):
        atlas.retrieve(qd, rule, scenes=TRUTH, scene_info=info)
    m.check_edge_index()
