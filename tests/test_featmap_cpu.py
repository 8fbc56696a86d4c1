"""The map path's host side without a GPU: FeatureMap metadata, the encoder digest and its invalidation, the save / load format,
and the argument checks of PoseNetX_R2.forward_map / evaluate.relocalize / ops.gather_graph_nodes (all raised before any kernel
is enqueued)."""
import os
import re

import pytest
import torch


def _model(seed=1, **kw):
    import relpose_gnn_amd.synth as S
    from relpose_gnn_amd.posenet import PoseNetX_R2
    from relpose_gnn_amd.resnet import ResNet
    planes, blocks = (8, 16, 32, 64), (1, 1, 1, 1)
    m = PoseNetX_R2(ResNet(blocks, planes), droprate=0.0, pretrained=False, feat_dim=64, edge_feat_dim=64, node_dim=64,
                    input_img_height=32, use_gnn=True, **kw)
    m.load_state_dict(S.synth_state_dict(S.posenet_r2_param_shapes(64, 64, 64, planes, blocks), seed=seed))
    return m.eval()


def _map(model, rows=5, poses=True):
    from relpose_gnn_amd.featmap import FeatureMap
    feats = torch.randn(rows, 64, generator=torch.Generator().manual_seed(rows))
    p = torch.randn(rows, 6, generator=torch.Generator().manual_seed(rows + 1)) if poses else None
    return FeatureMap(feats, FeatureMap.model_meta(model), p)


def test_digest_is_stable_cached_and_follows_the_encoder_weights():
    a, b = _model(seed=1), _model(seed=1)
    d = a.encoder_digest()
    assert re.fullmatch(r"[0-9a-f]{64}", d)
    assert a.encoder_digest() is d                    # cached
    assert b.encoder_digest() == d                    # a function of the weights
    assert _model(seed=2).encoder_digest() != d
    # the GNN's weights are not part of it: a map serves any GNN on the same encoder
    with torch.no_grad():
        a.proj_edge.weight.add_(1.0)
    a.refresh_packed()
    assert a.encoder_digest() == d


def test_digest_cache_is_cleared_where_the_packed_weights_are():
    m = _model(seed=1)
    d = m.encoder_digest()
    with torch.no_grad():
        m.feature_extractor.fc.bias.add_(1.0)
    assert m.encoder_digest() == d                    # in-place mutation: stale until refresh_packed, like the packed weights
    m.refresh_packed()
    assert m.encoder_digest() != d
    m.load_state_dict(_model(seed=1).state_dict())
    assert m.encoder_digest() == d
    m._enc_digest = "x"
    m.encoder_dtype = "bf16"
    assert m._enc_digest is None
    m._enc_digest = "x"
    m.float()                                         # _apply
    assert m._enc_digest is None


def test_map_metadata_and_check():
    from relpose_gnn_amd.featmap import FeatureMap
    m = _model(seed=1)
    fm = _map(m)
    assert fm.meta == {"feat_dim": 64, "precision": "f32", "encoder_digest": m.encoder_digest()}
    assert len(fm) == 5 and fm.feat_dim == 64 and "rows=5" in repr(fm)
    fm.check(m)
    with pytest.raises(ValueError, match="other encoder weights"):
        fm.check(_model(seed=2))
    m.load_state_dict(_model(seed=3).state_dict())
    with pytest.raises(ValueError, match="other encoder weights"):
        fm.check(m)
    m2 = _model(seed=1)
    m2.encoder_dtype = "bf16"
    with pytest.raises(ValueError, match="'f32' encoder.*'bf16'"):
        fm.check(m2)
    bad = FeatureMap(torch.zeros(2, 32), dict(fm.meta, feat_dim=32))
    with pytest.raises(ValueError, match="feat_dim 32"):
        bad.check(m)


def test_map_constructor_validation():
    from relpose_gnn_amd.featmap import FeatureMap
    meta = {"feat_dim": 64, "precision": "f32", "encoder_digest": "0" * 64}
    with pytest.raises(ValueError, match="fp32 tensor"):
        FeatureMap(torch.zeros(2, 64, dtype=torch.float64), meta)
    with pytest.raises(ValueError, match="lacks 'encoder_digest'"):
        FeatureMap(torch.zeros(2, 64), {"feat_dim": 64, "precision": "f32"})
    with pytest.raises(ValueError, match="metadata says feat_dim = 32"):
        FeatureMap(torch.zeros(2, 64), dict(meta, feat_dim=32))
    with pytest.raises(ValueError, match=r"poses must be \[2, 6\]"):
        FeatureMap(torch.zeros(2, 64), meta, torch.zeros(3, 6))


def test_save_load_round_trip_is_bit_identical(tmp_path):
    from relpose_gnn_amd.featmap import FORMAT, FeatureMap
    m = _model()
    for poses in (True, False):
        fm = _map(m, rows=7, poses=poses)
        path = os.path.join(tmp_path, f"map_{poses}.pt")
        fm.save(path)
        raw = torch.load(path, weights_only=True)      # plain tensors + metadata: the safe loader reads it
        assert raw["format"] == FORMAT and raw["meta"] == fm.meta and set(raw) == {"format", "meta", "features"} | (
            {"poses"} if poses else set())
        back = FeatureMap.load(path, "cpu")
        assert torch.equal(back.features, fm.features) and back.meta == fm.meta
        assert (back.poses is None) == (not poses)
        if poses:
            assert torch.equal(back.poses, fm.poses)
        back.check(m)


def test_load_refuses_other_files(tmp_path):
    from relpose_gnn_amd.featmap import FeatureMap
    path = os.path.join(tmp_path, "other.pt")
    torch.save({"features": torch.zeros(1, 64)}, path)
    with pytest.raises(ValueError, match="not a saved FeatureMap"):
        FeatureMap.load(path, "cpu")


def test_extend_validation():
    m = _model()
    fm = _map(m, poses=True)
    with pytest.raises(ValueError, match="poses must be given exactly when"):
        fm.extend(m, torch.zeros(1, 3 * 32 * 32))
    with pytest.raises(ValueError, match="other encoder weights"):
        fm.extend(_model(seed=5), torch.zeros(1, 3 * 32 * 32), poses=torch.zeros(1, 6))


def test_build_needs_a_gpu_model():
    from relpose_gnn_amd.featmap import FeatureMap
    with pytest.raises(RuntimeError, match="on the GPU"):
        FeatureMap.build(_model(), torch.zeros(2, 3 * 32 * 32))
    with pytest.raises(ValueError, match="chunk must be >= 1"):
        list(__import__("relpose_gnn_amd.featmap", fromlist=["_chunks"])._chunks(torch.zeros(2, 4), 0))
    with pytest.raises(TypeError, match="iterable of tensors"):
        list(__import__("relpose_gnn_amd.featmap", fromlist=["_chunks"])._chunks([torch.zeros(2, 4), "x"], 4))


def test_forward_map_argument_checks():
    m = _model()
    fm = _map(m)
    q = torch.zeros(2, 3 * 32 * 32)
    nb = torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(TypeError, match="int64 tensor"):
        m.forward_map(q, nb.int(), fm)
    with pytest.raises(TypeError, match="int64 tensor"):
        m.forward_map(q, torch.zeros(6, dtype=torch.int64), fm)
    with pytest.raises(ValueError, match="K >= 1"):
        m.forward_map(q, torch.zeros(2, 0, dtype=torch.int64), fm)
    with pytest.raises(ValueError, match="3 queries but neighbours has 2 rows"):
        m.forward_map(torch.zeros(3, 3 * 32 * 32), nb, fm)
    with pytest.raises(RuntimeError, match="queries must be on the GPU"):
        m.forward_map(q, nb, fm)
    with pytest.raises(RuntimeError, match="on the GPU"):
        m.encode(q)


def test_relocalize_argument_checks():
    from relpose_gnn_amd.evaluate import relocalize
    m = _model()
    fm = _map(m)
    q = torch.zeros(2, 3 * 32 * 32)
    with pytest.raises(ValueError, match=r"int64 \[G, K >= 1\] with G = 2"):
        relocalize(m, fm, q, torch.zeros(3, 7, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"int64 \[G, K >= 1\]"):
        relocalize(m, fm, q, torch.zeros(2, 0, dtype=torch.int64))
    with pytest.raises(ValueError, match="micro_batch"):
        relocalize(m, fm, q, torch.zeros(2, 7, dtype=torch.int64), micro_batch=0)
    with pytest.raises(TypeError, match="queries must be a tensor"):
        relocalize(m, fm, [q], torch.zeros(2, 7, dtype=torch.int64))


def test_gather_graph_nodes_rejects_host_tensors():
    from relpose_gnn_amd import ops
    with pytest.raises(RuntimeError, match="on the GPU"):
        ops.gather_graph_nodes(torch.zeros(2, 8), torch.zeros(4, 8), torch.zeros(2, 3, dtype=torch.int64))


def test_abi_declares_and_binds_the_gather():
    from relpose_gnn_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "relpose_gnn_hip.h")) as f:
        header = f.read()
    assert "int rpg_gather_graph_nodes_f32(" in header
    assert "rpg_gather_graph_nodes_f32" in _lib.SYMBOLS
    if os.path.exists(_lib.LIB_PATH):                # build() made it: the symbol is exported, the ABI version unchanged
        lib = _lib.lib()
        assert lib.rpg_abi_version() == 1
        assert lib.rpg_gather_graph_nodes_f32(None, None, None, 1, 1, 1, 4, None, None, None) == _lib.RPG_ERR_BAD_ARG
