"""SceneAtlas and the scene arguments without a GPU: concat's bookkeeping and refusals, the save / load round trip, n_allowed
against a numpy count, the oracle identity of scene-scoped retrieval on tests/retrieval_ref.py (so that the GPU tests' oracle is
itself checked against the float64 restatement of the rule), SceneFrameTransform's validation, and the new entry points'
argument checks through ctypes."""
import numpy as np
import pytest
import torch

import retrieval_ref as RR
import scene_ref as SR

META = {"feat_dim": 8, "precision": "f32", "encoder_digest": "abc"}


def _maps(sizes=(5, 9, 4), poses=True, groups=True, desc=None, meta=META, seed=0):
    from relpose_gnn_amd.featmap import FeatureMap
    gen = torch.Generator().manual_seed(seed)
    out = []
    for n in sizes:
        out.append(FeatureMap(torch.randn(n, 8, generator=gen), meta, poses=torch.randn(n, 6, generator=gen) if poses else None,
                              descriptors=torch.randn(n, desc, generator=gen) if desc else None,
                              groups=torch.arange(n) % 3 if groups else None))
    return out


def test_concat_bookkeeping():
    from relpose_gnn_amd.featmap import FeatureMap, SceneAtlas
    maps = _maps(desc=12)
    atlas = SceneAtlas.concat(maps, names=["chess", "fire", "heads"])
    assert isinstance(atlas, FeatureMap) and len(atlas) == 18 and atlas.n_scenes == 3
    assert atlas.scene_first_host.dtype == np.int64 and atlas.scene_first_host.tolist() == [0, 5, 14, 18]
    assert atlas.scene_first.dtype == torch.int64 and atlas.scene_first.tolist() == [0, 5, 14, 18]
    assert atlas.names == ["chess", "fire", "heads"] and atlas.scene_index("fire") == 1
    assert atlas.scene_of_rows().tolist() == [0] * 5 + [1] * 9 + [2] * 4
    for what in ("features", "poses", "descriptors", "groups_host"):
        assert torch.equal(getattr(atlas, what), torch.cat([getattr(m, what) for m in maps])), what
    assert atlas.meta == META
    # a dict carries its names, in its order; a sequence without names numbers them
    by_name = SceneAtlas.concat({"b": maps[1], "a": maps[0]})
    assert by_name.names == ["b", "a"] and by_name.scene_first_host.tolist() == [0, 9, 14]
    assert SceneAtlas.concat(maps).names == ["0", "1", "2"]
    assert SceneAtlas.concat(maps[:1]).scene_first_host.tolist() == [0, 5]


def test_scene_shares_storage():
    from relpose_gnn_amd.featmap import FeatureMap, SceneAtlas
    maps = _maps(desc=12)
    atlas = SceneAtlas.concat(maps)
    for i, m in enumerate(maps):
        sc = atlas.scene(i)
        assert type(sc) is FeatureMap and len(sc) == len(m) and sc.meta == atlas.meta
        a = int(atlas.scene_first_host[i])
        for what in ("features", "poses", "descriptors", "groups_host", "groups"):
            t = getattr(sc, what)
            assert torch.equal(t, getattr(m, what)), what
            assert t.data_ptr() == getattr(atlas, what)[a:].data_ptr(), what
    with pytest.raises(IndexError):
        atlas.scene(3)
    with pytest.raises(IndexError):
        atlas.scene(-1)


def test_save_load_round_trip(tmp_path):
    from relpose_gnn_amd.featmap import FeatureMap, SceneAtlas
    atlas = SceneAtlas.concat(_maps(desc=12), names=["x", "y", "z"])
    path = tmp_path / "atlas.pt"
    atlas.save(path)
    back = SceneAtlas.load(path, "cpu")
    assert back.names == atlas.names and np.array_equal(back.scene_first_host, atlas.scene_first_host)
    for what in ("features", "poses", "descriptors", "groups_host"):
        assert torch.equal(getattr(back, what), getattr(atlas, what)), what
    # the keys sit beside the existing format: the same file is one plain map to FeatureMap.load
    plain = FeatureMap.load(path, "cpu")
    assert type(plain) is FeatureMap and torch.equal(plain.features, atlas.features)
    # ... and a plain map's file is not an atlas
    atlas.scene(0).save(tmp_path / "one.pt")
    assert len(FeatureMap.load(tmp_path / "one.pt", "cpu")) == 5
    with pytest.raises(ValueError, match="without scenes"):
        SceneAtlas.load(tmp_path / "one.pt", "cpu")
    bare = SceneAtlas.concat(_maps(poses=False, groups=False))
    bare.save(path)
    back = SceneAtlas.load(path, "cpu")
    assert back.poses is None and back.groups is None and back.descriptors is None and back.names == ["0", "1", "2"]


def test_concat_refusals():
    from relpose_gnn_amd.featmap import SceneAtlas
    maps = _maps()
    with pytest.raises(ValueError, match="another encoder"):
        SceneAtlas.concat([maps[0], _maps(meta=dict(META, encoder_digest="other"))[1]])
    with pytest.raises(ValueError, match="another encoder"):
        SceneAtlas.concat([maps[0], _maps(meta=dict(META, precision="bf16"))[1]])
    with pytest.raises(ValueError, match="poses"):
        SceneAtlas.concat([maps[0], _maps(poses=False)[1]])
    with pytest.raises(ValueError, match="groups"):
        SceneAtlas.concat([maps[0], _maps(groups=False)[1]])
    with pytest.raises(ValueError, match="descriptors"):
        SceneAtlas.concat([maps[0], _maps(desc=12)[1]])
    with pytest.raises(ValueError, match="columns"):
        SceneAtlas.concat([_maps(desc=12)[0], _maps(desc=16)[1]])
    with pytest.raises(ValueError):
        SceneAtlas.concat([])
    with pytest.raises(ValueError):
        SceneAtlas.concat([maps[0], "not a map"])
    with pytest.raises(ValueError, match="names"):
        SceneAtlas.concat(maps, names=["a", "b"])
    with pytest.raises(ValueError, match="names"):
        SceneAtlas.concat(maps, names=["a", "b", "a"])
    with pytest.raises(ValueError, match="names"):
        SceneAtlas.concat({"a": maps[0]}, names=["a"])
    feats = torch.cat([m.features for m in maps])
    for first in ([0, 5, 14], [1, 5, 18], [0, 5, 5, 18], [0, 14, 5, 18], [18]):
        with pytest.raises(ValueError, match="scene_first"):
            SceneAtlas(feats, META, scene_first=first)
    with pytest.raises(ValueError, match="scene_first"):
        SceneAtlas(feats, META)
    with pytest.raises(NotImplementedError, match="concat"):
        SceneAtlas.concat(maps).extend(None, None)


def test_n_allowed_counts_inside_the_scene():
    from relpose_gnn_amd.featmap import SceneAtlas
    sizes = (5, 9, 4)
    atlas = SceneAtlas.concat(_maps(sizes))
    db_group = atlas.groups_host.numpy()
    scenes = np.asarray([0, 1, 2, 2, 1, 0, 1])
    q_groups = np.asarray([0, -1, 2, 7, 1, 2, 0])
    got = atlas.n_allowed(torch.as_tensor(q_groups), 7, scenes)
    assert got.dtype == np.int64 and np.array_equal(got, SR.n_allowed_ref(sizes, scenes, q_groups, db_group))
    assert np.array_equal(atlas.n_allowed(None, 7, scenes), np.asarray(sizes)[scenes])
    assert np.array_equal(SceneAtlas.concat(_maps(sizes, groups=False)).n_allowed(None, 7, scenes), np.asarray(sizes)[scenes])
    # scenes on the device only: the smallest scene, what a rule without draws is checked against
    assert atlas.n_allowed(None, 3).tolist() == [4, 4, 4]
    with pytest.raises(IndexError):
        atlas.n_allowed(None, 2, np.asarray([0, 3]))
    with pytest.raises(IndexError):
        atlas.n_allowed(None, 3, np.asarray([0, 1]))
    with pytest.raises(ValueError, match="SceneAtlas"):       # one scene's map takes no scenes
        atlas.scene(0).n_allowed(None, 2, np.asarray([0, 0]))


def test_scope_refusals():
    from relpose_gnn_amd.featmap import SceneAtlas
    from relpose_gnn_amd.retrieval import RetrievalRule
    atlas = SceneAtlas.concat(_maps((5, 9, 4)))
    host, dev = atlas._scope([2, 0, 1], 3, RetrievalRule(k=4), "retrieve")
    assert host.tolist() == [2, 0, 1] and dev.dtype == torch.int32 and dev.tolist() == [2, 0, 1]
    with pytest.raises(ValueError, match="scenes"):
        atlas._scope(None, 3, RetrievalRule(k=3), "retrieve")
    with pytest.raises(ValueError, match="smallest scene"):
        atlas._scope([2, 0, 1], 3, RetrievalRule(k=5), "retrieve")
    with pytest.raises(IndexError):
        atlas._scope([2, 0, 3], 3, RetrievalRule(k=3), "retrieve")
    with pytest.raises(IndexError):
        atlas._scope([2, -1, 0], 3, RetrievalRule(k=3), "retrieve")
    for bad in ([0, 1], [0.0, 1.0, 2.0], [[0, 1, 2]], [True, False, True]):
        with pytest.raises(ValueError):
            atlas._scope(bad, 3, RetrievalRule(k=3), "retrieve")
    with pytest.raises(ValueError, match="SceneAtlas"):
        atlas.scene(0).retrieve(torch.zeros(3, 8), RetrievalRule(k=3), scenes=[0, 0, 0])


@pytest.mark.parametrize("with_groups", [False, True])
def test_oracle_identity_on_the_float64_rule(with_groups):
    """Ranking the scene's slice and adding its offset equals ranking the whole map with the rows outside excluded -- which is
    how the GPU tests' oracle (scene_ref.emulated_groups on the unscoped entry) states the scoped entry point."""
    sizes, d, g = SR.SIZES, 64, 12
    q, db = SR.descriptors(d, g, seed=4)
    first = SR.scene_first(sizes)
    rng = np.random.RandomState(5)
    scenes = rng.randint(0, len(sizes), g)
    db_group = np.arange(db.shape[0]) % 3 if with_groups else None
    q_groups = rng.randint(-1, 3, g) if with_groups else None
    ranks = np.tile(np.asarray([0, 1, 2], dtype=np.int32), (g, 1))       # (the 5-row scene minus a group keeps >= 3 rows)
    for i in range(g):
        s, a, b = int(scenes[i]), int(first[scenes[i]]), int(first[scenes[i] + 1])
        qg = -1 if q_groups is None else int(q_groups[i])
        inside = RR.retrieve_ref(q[i:i + 1], db[a:b], ranks[i:i + 1], None if db_group is None else [qg],
                                 None if db_group is None else db_group[a:b]) + a
        whole = RR.retrieve_ref(q[i:i + 1], db, ranks[i:i + 1], [1], SR.emulated_groups(sizes, s, qg, db_group))
        assert np.array_equal(inside, whole) and ((inside >= a) & (inside < b)).all()
    # the counts the ranks are sized by agree with the emulated groups, too
    want = [int((SR.emulated_groups(sizes, int(s), -1 if q_groups is None else int(c), db_group) == 0).sum())
            for s, c in zip(scenes, q_groups if q_groups is not None else [-1] * g)]
    assert SR.n_allowed_ref(sizes, scenes, q_groups, db_group).tolist() == want


def test_scene_frame_transform_validation(tmp_path):
    from relpose_gnn_amd.frames import FrameTransform, SceneFrameTransform
    means, stds = [[0.1, 0.2, 0.3], [0.4, 0.5, 0.6]], [[1.0, 2.0, 3.0], [0.5, 0.25, 0.125]]
    sft = SceneFrameTransform(256, means, stds)
    assert len(sft) == 2 and sft.output_size(480, 640) == (256, 341)
    one = sft.scene(1)
    assert isinstance(one, FrameTransform) and one.resize == 256
    ref = FrameTransform(256, mean=means[1], std=stds[1])
    assert one.mean == ref.mean and one.std == ref.std          # rounded to fp32 the same way
    assert sft.stats("cpu").dtype == torch.float32 and sft.stats("cpu").tolist() == [list(ref2.mean + ref2.std) for ref2 in
                                                                                     (sft.scene(0), sft.scene(1))]
    with pytest.raises(IndexError):
        sft.scene(2)
    for bad_m, bad_s in (([[0, 0, 0]], [[1, 0, 1]]), ([[0, 0, 0]], [[1, float("inf"), 1]]), ([[0, 0, 0]], [[1, float("nan"), 1]]),
                         ([[0, float("nan"), 0]], [[1, 1, 1]]), ([[0, float("inf"), 0]], [[1, 1, 1]]), ([[0, 0, 0]], [[1, 1e-60, 1]]),
                         ([[0, 0, 0]], [[1, 1e60, 1]])):
        with pytest.raises(ValueError, match="finite"):
            SceneFrameTransform(256, bad_m, bad_s)
    for bad_m, bad_s in (([0, 0, 0], [1, 1, 1]), ([[0, 0, 0]], [[1, 1, 1], [1, 1, 1]]), ([[0, 0]], [[1, 1]]), ([], [])):
        with pytest.raises(ValueError):
            SceneFrameTransform(256, bad_m, bad_s)
    with pytest.raises(ValueError):
        SceneFrameTransform(0, means, stds)
    with pytest.raises(RuntimeError, match="GPU"):
        sft.apply(torch.zeros((2, 8, 8, 3), dtype=torch.uint8), [0, 1])
    # stats files: mean and VARIANCE per channel, std = sqrt(var) in float64, as FrameTransform.from_stats_file reads one
    paths = []
    for i, (m, v) in enumerate(((means[0], [0.04, 0.09, 0.16]), (means[1], [0.25, 0.36, 0.49]))):
        paths.append(tmp_path / f"stats{i}.txt")
        np.savetxt(paths[-1], np.asarray([m, v]))
    from_files = SceneFrameTransform.from_stats_files(paths, resize=128)
    for i, p in enumerate(paths):
        ref = FrameTransform.from_stats_file(p, resize=128)
        assert from_files.scene(i).mean == ref.mean and from_files.scene(i).std == ref.std and from_files.scene(i).resize == 128


def test_new_symbols_and_their_argument_checks():
    from relpose_gnn_amd import _lib
    lib = _lib.lib()
    for name in ("rpg_retrieve_cosine_scoped_f32", "rpg_frames_u8_to_f32_scenes", "rpg_frames_u8_to_bf16_scenes"):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
    assert lib.rpg_abi_version() == 1
    g, k, m, d = 2, 2, 8, 8
    q, db = torch.zeros(g, d), torch.zeros(m, d)
    ranks, nb = torch.zeros((g, k), dtype=torch.int32), torch.zeros((g, k), dtype=torch.int64)
    ws = torch.zeros(int(lib.rpg_retrieve_workspace_bytes(g, m, d)) + 64, dtype=torch.uint8)
    status = torch.zeros(1, dtype=torch.int32)
    first, qs = torch.tensor([0, 4, 8], dtype=torch.int64), torch.zeros(g, dtype=torch.int32)
    wp = (ws.data_ptr() + 15) & ~15

    def scoped(first_p, qs_p, n, m_=m, k_=k):
        # refused before anything is launched: the checks come first, so host pointers do here
        return lib.rpg_retrieve_cosine_scoped_f32(q.data_ptr(), db.data_ptr(), None, None, None, ranks.data_ptr(), g, k_, m_, d, None,
                                                  None, 0.0, 0.0, 0, None, first_p, qs_p, n, nb.data_ptr(), None, wp, ws.numel() - 16,
                                                  status.data_ptr(), None)
    assert scoped(first.data_ptr(), None, 2) == _lib.RPG_ERR_BAD_ARG          # exactly one of the two NULL
    assert scoped(None, qs.data_ptr(), 2) == _lib.RPG_ERR_BAD_ARG
    assert scoped(first.data_ptr(), qs.data_ptr(), 0) == _lib.RPG_ERR_BAD_ARG
    assert scoped(first.data_ptr() + 4, qs.data_ptr(), 2) == _lib.RPG_ERR_BAD_ARG         # alignment
    assert scoped(first.data_ptr(), qs.data_ptr() + 2, 2) == _lib.RPG_ERR_BAD_ARG
    assert scoped(first.data_ptr(), qs.data_ptr(), 2, m_=1) == _lib.RPG_ERR_BAD_ARG       # the gated entry's own checks hold
    assert scoped(first.data_ptr(), qs.data_ptr(), 2, k_=65) == _lib.RPG_ERR_BAD_ARG
    assert lib.rpg_retrieve_cosine_scoped_f32(q.data_ptr(), db.data_ptr(), None, None, None, ranks.data_ptr(), g, k, m, d, None, None,
                                              0.0, 0.0, 0, None, first.data_ptr(), qs.data_ptr(), 2, nb.data_ptr(), None, wp, 16,
                                              status.data_ptr(), None) == _lib.RPG_ERR_WORKSPACE

    frames, out = torch.zeros((2, 4, 4, 3), dtype=torch.uint8), torch.zeros((2, 3, 4, 4))
    stats, scene = torch.ones((2, 6)), torch.zeros(2, dtype=torch.int32)
    for fn in (lib.rpg_frames_u8_to_f32_scenes, lib.rpg_frames_u8_to_bf16_scenes):
        def call(stats_p=stats.data_ptr(), scene_p=scene.data_ptr(), n=2, status_p=status.data_ptr(), out_p=out.data_ptr(), oh=4):
            return fn(frames.data_ptr(), 2, 4, 4, oh, 4, None, None, None, None, stats_p, scene_p, n, status_p, out_p, None, 0, None)
        assert call(stats_p=None) == _lib.RPG_ERR_BAD_ARG
        assert call(scene_p=None) == _lib.RPG_ERR_BAD_ARG
        assert call(status_p=None) == _lib.RPG_ERR_BAD_ARG
        assert call(out_p=None) == _lib.RPG_ERR_BAD_ARG
        assert call(n=0) == _lib.RPG_ERR_BAD_ARG
        assert call(stats_p=stats.data_ptr() + 2) == _lib.RPG_ERR_BAD_ARG
        assert call(oh=2) == _lib.RPG_ERR_BAD_ARG                            # a resized axis without its tables


def test_wrappers_refuse_cpu_tensors():
    from relpose_gnn_amd import ops
    q, db, ranks = torch.zeros(2, 8), torch.zeros(8, 8), torch.zeros((2, 2), dtype=torch.int32)
    first, qs = torch.tensor([0, 4, 8]), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="go together"):
        ops.retrieve_scoped(q, db, ranks, first, None)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.retrieve_scoped(q, db, ranks, first, qs)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.frames_u8_to_f32_scenes(torch.zeros((2, 4, 4, 3), dtype=torch.uint8), (4, 4), (None,) * 4, torch.ones(2, 6), qs)
