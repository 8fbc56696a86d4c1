"""Retrieval without a GPU: the host half of the rule (RetrievalRule) and its float64 restatement (retrieval_ref.py) against the
indices the reference's own obtain_KNNs returned (golden G10, tests/golden/make_retrieval_golden.py), FeatureMap's descriptor /
group fields, the exported symbols, and the argument errors raised before the device is touched."""
import os
import re

import numpy as np
import pytest
import torch

import retrieval_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_SYMBOLS = ("rpg_retrieve_workspace_bytes", "rpg_retrieve_max_rank", "rpg_row_inv_norms_f32", "rpg_retrieve_cosine_f32")


@pytest.fixture(scope="module")
def g10():
    return np.load(os.path.join(HERE, "golden", "g10_retrieval.npz"))


def g10_case(z, config, sp):
    """(q, db, q_group, db_group, seed, indices) of one recorded configuration, in the kernel's terms."""
    db, q_index, m = z["db"], z["q_index"], z["db"].shape[0]
    rows = np.arange(m, dtype=np.int64)
    if config == "none":
        q, qg, dg = z["q"], None, None
    elif config == "self":
        q, qg, dg = db[q_index], q_index, rows
    else:
        ssl = int(z["scene_seq_len"])
        q, qg, dg = db[q_index], q_index // ssl, rows // ssl
    return q, db, qg, dg, int(z[f"{config}_sp{sp}_seed"]), z[f"{config}_sp{sp}_indices"]


@pytest.mark.parametrize("config", ["none", "self", "cross"])
@pytest.mark.parametrize("sp", [5, 10])
def test_reference_rule_reproduces_g10(g10, config, sp):
    from relpose_gnn_amd.retrieval import RetrievalRule
    q, db, qg, dg, seed, want = g10_case(g10, config, sp)
    n = np.full(q.shape[0], db.shape[0]) if qg is None else R.n_allowed(db.shape[0], qg, dg)
    ranks = RetrievalRule.reference(k=int(g10["k"]), sampling_period=sp, seed=seed).ranks(n)
    assert ranks.dtype == np.int32 and (np.diff(ranks, axis=1) > 0).all()
    assert int(ranks.max()) == int(g10[f"{config}_sp{sp}_max_rank"])
    assert np.array_equal(R.retrieve_ref(q, db, ranks, qg, dg), want)


def test_reference_rule_is_the_legacy_global_stream():
    """The draws written out literally (dataset_7Scenes_multi.py:256-260) on numpy's global generator."""
    from relpose_gnn_amd.retrieval import RetrievalRule
    n_allowed, k, sp = [300, 290, 299, 300], 7, 5
    np.random.seed(77)
    want = []
    for n in n_allowed:
        surviving = np.random.random(n) < 0.5
        start = np.random.randint(0, sp, 1)[0]
        want.append(np.arange(n)[surviving][start::sp][:k])
    rule = RetrievalRule.reference(k=k, sampling_period=sp, seed=77)
    assert np.array_equal(rule.ranks(n_allowed[:2], limit=300), np.stack(want[:2]))
    assert np.array_equal(rule.ranks(n_allowed[2:], limit=300), np.stack(want[2:]))      # the stream runs on between calls


def test_deterministic_ranks():
    from relpose_gnn_amd.retrieval import RetrievalRule
    assert np.array_equal(RetrievalRule(k=7).ranks([100, 7]), np.tile(np.arange(7, dtype=np.int32), (2, 1)))
    assert np.array_equal(RetrievalRule(k=4, sampling_period=5).ranks([16]), [[0, 5, 10, 15]])
    assert RetrievalRule(k=3).ranks([]).shape == (0, 3)
    for bad in (dict(k=0), dict(k=65), dict(sampling_period=0), dict(drop=1.0), dict(drop=-0.1)):
        with pytest.raises(ValueError):
            RetrievalRule(**bad)


def test_too_few_survivors_and_rank_limit_raise():
    from relpose_gnn_amd.retrieval import RetrievalRule, max_rank
    with pytest.raises(ValueError, match="query 1 gets 6 database rows"):
        RetrievalRule(k=7).ranks([7, 6])
    with pytest.raises(ValueError, match="query 0"):
        RetrievalRule(k=4, sampling_period=5).ranks([15])
    with pytest.raises(ValueError, match="query 2 gets"):
        RetrievalRule.reference(k=7, sampling_period=5, seed=1).ranks([300, 300, 30])
    r_max = max_rank()
    assert r_max >= 256
    assert RetrievalRule(k=2, sampling_period=r_max - 1).ranks([10 * r_max])[0, 1] == r_max - 1
    with pytest.raises(ValueError, match=f"R_MAX = {r_max}"):
        RetrievalRule(k=2, sampling_period=r_max).ranks([10 * r_max])
    # the reference's defaults fit with room to spare (expected last position near 70 / 140)
    RetrievalRule.reference(k=7, sampling_period=10, seed=5).ranks([4000] * 64)


def test_ref_ordering_ties_nonfinite_and_zero_rows():
    db = np.zeros((6, 4))
    db[0], db[1], db[2], db[4], db[5] = [1, 0, 0, 0], [2, 0, 0, 0], [1, 1, 0, 0], [np.nan, 0, 0, 0], [-1, 0, 0, 0]
    q = np.array([[3.0, 0, 0, 0]])
    s = R.cosine_f64(q, db)
    assert s[0, 3] == 0.0                                              # zero row: similarity 0
    order = R.ranking(s[0], np.ones(6, dtype=bool))
    assert order.tolist() == [0, 1, 2, 3, 5, 4]                        # ties by row, NaN last
    assert R.retrieve_ref(q, db, [[0, 2]], [1], [0, 1, 1, 0, 0, 0]).tolist() == [[0, 5]]     # rows 0, 3, 5, 4 are left


def _meta():
    return {"feat_dim": 8, "precision": "f32", "encoder_digest": "0" * 64}


def test_featmap_descriptors_groups_save_load(tmp_path):
    from relpose_gnn_amd.featmap import FORMAT, FeatureMap
    gen = torch.Generator().manual_seed(1)
    feats, desc = torch.randn(5, 8, generator=gen), torch.randn(5, 12, generator=gen)
    groups = torch.tensor([0, 0, 1, 1, 2])
    fm = FeatureMap(feats, _meta(), torch.randn(5, 6, generator=gen), descriptors=desc, groups=groups)
    assert fm.descriptor_matrix is fm.descriptors and fm.groups.dtype == torch.int64 and fm.groups_host.device.type == "cpu"
    assert fm.n_allowed(torch.tensor([0, 2, -1, 9]), 4).tolist() == [3, 4, 5, 5]
    fm.save(tmp_path / "m.pt")
    obj = torch.load(tmp_path / "m.pt", weights_only=True)
    assert "inv_norms" not in obj and set(obj) == {"format", "meta", "features", "poses", "descriptors", "groups"}
    back = FeatureMap.load(tmp_path / "m.pt", "cpu")
    assert torch.equal(back.descriptors, desc) and torch.equal(back.groups, groups) and torch.equal(back.features, feats)
    # a file written before the fields existed
    torch.save({"format": FORMAT, "meta": _meta(), "features": feats}, tmp_path / "old.pt")
    old = FeatureMap.load(tmp_path / "old.pt", "cpu")
    assert old.descriptors is None and old.groups is None and old.descriptor_matrix is old.features
    assert old.n_allowed(None, 3).tolist() == [5, 5, 5]
    for bad in (dict(descriptors=torch.randn(4, 12)), dict(descriptors=torch.randn(5, 10)), dict(groups=torch.zeros(4, dtype=torch.int64)),
                dict(groups=torch.zeros(5))):
        with pytest.raises(ValueError):
            FeatureMap(feats, _meta(), **bad)


def test_featmap_extend_all_or_none():
    from relpose_gnn_amd.featmap import FeatureMap
    fm = FeatureMap(torch.zeros(3, 8), _meta(), descriptors=torch.ones(3, 4), groups=[0, 1, 2])
    with pytest.raises(ValueError, match="descriptors must be given exactly when"):
        fm._check_extend(None, None, [3])
    with pytest.raises(ValueError, match="groups must be given exactly when"):
        fm._check_extend(None, torch.ones(1, 4), None)
    with pytest.raises(ValueError, match="poses must be given exactly when"):
        fm._check_extend(torch.zeros(1, 6), torch.ones(1, 4), [3])
    fm._check_extend(None, torch.ones(1, 4), [3])
    fm._inv_norms = "stale"
    fm._append(torch.zeros(2, 8), None, torch.ones(2, 4), [3, 3])
    assert len(fm) == 5 and fm.descriptors.shape == (5, 4) and fm.groups_host.tolist() == [0, 1, 2, 3, 3]
    assert fm._inv_norms is None and fm.n_allowed(torch.tensor([3]), 1).tolist() == [3]
    with pytest.raises(ValueError, match="columns"):
        fm._append(torch.zeros(1, 8), None, torch.ones(1, 8), [4])
    plain = FeatureMap(torch.zeros(3, 8), _meta())
    with pytest.raises(ValueError, match="descriptors must be given exactly when"):
        plain._check_extend(None, torch.ones(1, 4), None)


def test_new_symbols_exported_and_declared():
    from relpose_gnn_amd import _lib
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "relpose_gnn_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(lib, name)
        assert re.search(rf"\b{name}\s*\(", header), name
    assert lib.rpg_abi_version() == 1
    assert lib.rpg_retrieve_max_rank() >= 256
    small, big = lib.rpg_retrieve_workspace_bytes(1, 4000, 2048), lib.rpg_retrieve_workspace_bytes(64, 4000, 2048)
    assert 0 < small < big and big >= 64 * 4000 * 4


def _tiny_model():
    import relpose_gnn_amd.synth as S
    from relpose_gnn_amd.posenet import PoseNetX_R2
    from relpose_gnn_amd.resnet import ResNet
    planes, blocks = (8, 16, 32, 64), (1, 1, 1, 1)
    m = PoseNetX_R2(ResNet(blocks, planes), pretrained=False, feat_dim=64, edge_feat_dim=64, node_dim=64, input_img_height=32,
                    use_gnn=True, droprate=0.0, knn=-1, use_AP=True, gnn_recursion=2)
    m.load_state_dict(S.synth_state_dict(S.posenet_r2_param_shapes(64, 64, 64, planes, blocks), seed=1))
    return m.eval()


def test_forward_map_and_relocalize_argument_errors():
    from relpose_gnn_amd.evaluate import relocalize
    from relpose_gnn_amd.featmap import FeatureMap
    from relpose_gnn_amd.retrieval import RetrievalRule
    m = _tiny_model()
    meta = {"feat_dim": 64, "precision": "f32", "encoder_digest": "0" * 64}
    plain = FeatureMap(torch.zeros(10, 64), meta)
    with_desc = FeatureMap(torch.zeros(10, 64), meta, descriptors=torch.ones(10, 16))
    q = torch.zeros(2, 3, 32, 32)
    nb = torch.zeros(2, 3, dtype=torch.int64)
    rule = RetrievalRule(k=3)
    with pytest.raises(ValueError, match="not both"):
        m.forward_map(q, nb, plain, rule=rule)
    with pytest.raises(ValueError, match="pass a rule"):
        m.forward_map(q, nb, plain, query_descriptors=torch.zeros(2, 16))
    with pytest.raises(ValueError, match="query_descriptors"):
        m.forward_map(q, None, with_desc, rule=rule)
    with pytest.raises(ValueError, match="holds no descriptors"):
        m.forward_map(q, None, plain, rule=rule, query_descriptors=torch.zeros(2, 16))
    with pytest.raises(ValueError, match="must be fp32"):
        m.forward_map(q, None, with_desc, rule=rule, query_descriptors=torch.zeros(2, 12))
    with pytest.raises(ValueError, match="the map has 10"):
        m.forward_map(q, None, plain, rule=RetrievalRule(k=11))
    with pytest.raises(TypeError):
        m.forward_map(q, None, plain)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.forward_map(q, None, plain, rule=rule)
    with pytest.raises(ValueError, match="exactly one"):
        relocalize(m, plain, q, nb, rule=rule)
    with pytest.raises(ValueError, match="exactly one"):
        relocalize(m, plain, q)
    with pytest.raises(ValueError, match="pass a rule"):
        relocalize(m, plain, q, nb, query_groups=[0, 1])
    with pytest.raises(ValueError, match="query_descriptors"):
        relocalize(m, with_desc, q, rule=rule)
    with pytest.raises(ValueError, match="query_groups must be"):
        relocalize(m, plain, q, rule=rule, query_groups=[0, 1, 2])
