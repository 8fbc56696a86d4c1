"""Host-side logic that needs no GPU: state-dict contract, weight packing, graph containers, and that the C-ABI
library loads and exports every symbol include/relpose_gnn_hip.h declares (no compute calls here)."""
import os
import re

import pytest
import torch

import relpose_gnn_amd.synth as S
from conftest import ROOT
from relpose_gnn_amd.graph import Batch, Data, fc_batch, fc_edge_index


def test_library_exports_every_declared_symbol():
    from relpose_gnn_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "relpose_gnn_hip.h")).read()
    declared = set(re.findall(r"\b(rpg_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    lib = _lib.lib()                                    # loads without a GPU
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.rpg_abi_version() == 1
    # pure host-side argument validation paths (no kernel is launched)
    assert lib.rpg_maxpool3x3s2_nhwc_f32(None, None, 1, 4, 4, 8, None) == _lib.RPG_ERR_BAD_ARG
    assert lib.rpg_gnn_workspace_bytes(8, 56, 2048) > 5 * 56 * 2048 * 4
    assert lib.rpg_gnn_workspace_bytes(8, 56, 100) == 0          # d % 32 != 0
    planes = _lib.int_array([64, 128, 256, 512])
    ws = lib.rpg_resnet_workspace_bytes(256, 224, 224, planes)
    assert ws >= 4 * (256 * 224 * 224 * 4 + 256 * 112 * 112 * 64 + 4 * 256 * 56 * 56 * 64)
    with pytest.raises(ValueError):
        _lib.check(_lib.RPG_ERR_BAD_ARG, "x")


def test_tuning_and_timer_constants_match_the_header():
    """ops.TUNE_* and the timer classes are the header's #defines (they are passed across the ABI as plain ints), and
    rpg_set_tuning validates keys / values on the host side (no GPU involved).  rpg_get_tuning reads every key back: its default
    before any set, the value as passed after a set, the default again after ops.reset_tuning(); the test ends in the default state
    (the defaults themselves are pinned by tests/tuning_check.cpp)."""
    from relpose_gnn_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "relpose_gnn_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(RPG_[A-Z0-9_]+)\s+(-?\d+)\b", hdr)}
    tune = {k[len("RPG_TUNE_"):]: v for k, v in defs.items() if k.startswith("RPG_TUNE_")}
    assert len(set(tune.values())) == len(tune)                       # no two knobs share a key
    for name, key in tune.items():
        assert getattr(ops, "TUNE_" + name) == key, name
    assert {k for k in dir(ops) if k.startswith("TUNE_")} == {"TUNE_" + k for k in tune}
    lib = _lib.lib()
    accepts_any = {"TILE", "EPILOGUE", "STREAMK", "GNN_SPLIT", "FAST_LOADER", "BF16_FAST", "FUSED_STEM", "WAVES8", "GNN_FUSE_AGG",
                   "BF16_LEAN_EPI", "BF16_PERSIST", "BF16_FUSE_BLOCK", "FIXUP_PRIO", "BF16_PAIR"}      # flags and masked keys: no value is refused
    assert lib.rpg_set_tuning(12345, 0) == _lib.RPG_ERR_BAD_ARG       # unknown key
    assert lib.rpg_set_tuning(defs["RPG_TUNE_BK"], 24) == _lib.RPG_ERR_BAD_ARG
    assert lib.rpg_set_tuning(defs["RPG_TUNE_WINOGRAD"], 7) == _lib.RPG_ERR_BAD_ARG
    # read-back: the default before any set, the value as passed after a set, the default again after ops.reset_tuning()
    ops.reset_tuning()
    probe = {"BK": 16, "BF16_BK": 64, "WINOGRAD": 40, "WINO_SPLIT": 96, "FUSED_STEM": 129 | (5 << 8), "BF16_PATCH": 14, "SK_MIN_ITS": 4096,
             "BF16_CHUNK": 8 | (128 << 12), "BF16_LINEAR_DMA": 12, "FOLD_K": 64, "BF16_FUSE_BLOCK": 11, "BF16_WS64": 0, "WINO2D": 0}
    assert list(ops.TUNING_KEYS) == [name for name, _ in sorted(tune.items(), key=lambda kv: kv[1])]
    for name, key in tune.items():
        default = ops.tuning_default(key)
        assert ops.get_tuning(key) == default == ops.tuning_default(name) == ops.get_tuning("TUNE_" + name), name
        value = probe.get(name, 0 if default else 1)
        ops.set_tuning(key, value)
        assert ops.get_tuning(key) == value, name
        assert lib.rpg_set_tuning(key, -7) == (0 if name in accepts_any else _lib.RPG_ERR_BAD_ARG), name
        assert ops.get_tuning(key) == (-7 if name in accepts_any else value), name            # a refused value changes nothing
    ops.reset_tuning()
    for name, key in tune.items():
        assert ops.get_tuning(key) == ops.tuning_default(key), name
    assert lib.rpg_get_tuning(12345, None, None) == lib.rpg_get_tuning(-1, None, None) == _lib.RPG_ERR_BAD_ARG
    assert lib.rpg_get_tuning(0, None, None) == _lib.RPG_OK
    # ops.tuned: the keys hold inside the block; afterwards EVERY key is at its default, also when a set is refused half-way
    with ops.tuned({"FIXUP_PRIO": 1, ops.TUNE_BF16_FUSE_BLOCK: 1}):
        assert ops.get_tuning("FIXUP_PRIO") == 1 and ops.get_tuning("BF16_FUSE_BLOCK") == 1
        ops.set_tuning(ops.TUNE_TILE, 2)
    with pytest.raises(ValueError):
        with ops.tuned({"STREAMK": 0, "BK": 24}):
            raise AssertionError("entered with a refused key")
    for name, key in tune.items():
        assert ops.get_tuning(key) == ops.tuning_default(key), name
    # the weights-stationary probe kernel is not part of the product library (tools/probes/conv3x3_bf16_ws64.inc)
    assert lib.rpg_set_tuning(defs["RPG_TUNE_BF16_WS64"], 1) == _lib.RPG_ERR_BAD_ARG
    # ... and neither is the nested 2-D Winograd kernel (tools/probes/winograd2d.hip)
    assert lib.rpg_set_tuning(defs["RPG_TUNE_WINO2D"], 1) == _lib.RPG_ERR_BAD_ARG and lib.rpg_wino43_weights_floats(2, 3) == 18 * 6


def test_state_dict_contract_matches_reference_inventory():
    from relpose_gnn_amd.posenet import PoseNetX_R2
    from relpose_gnn_amd.resnet import resnet34
    m = PoseNetX_R2(resnet34(), droprate=0.0, pretrained=True, feat_dim=2048, edge_feat_dim=2048, node_dim=2048,
                    use_gnn=True, knn=-1, gnn_recursion=2, input_img_height=224)
    sd = m.state_dict()
    shapes = S.posenet_r2_param_shapes()                 # checked against the instantiated reference in make_golden.py
    assert list(sd.keys()) == list(shapes.keys()) and len(sd) == 248
    assert all(tuple(sd[k].shape) == tuple(v) for k, v in shapes.items())
    assert sum(p.numel() for p in m.parameters()) == 74805836
    assert m.feature_extractor.fc.in_features == 512 and m.feature_extractor.fc.out_features == 2048
    # pretrained=True re-initialises only the six top-level Linears (bias 0), posenet.py:981-997
    assert float(m.proj_edge.bias.abs().max()) == 0.0 and float(m.gnn1.mlp[0].bias.abs().max()) > 0.0
    m.load_state_dict(S.synth_state_dict(shapes, seed=3))
    with pytest.raises(RuntimeError):                    # no CPU fallback
        m(fc_batch(torch.zeros(8, 3 * 224 * 224), 8))
    with pytest.raises(NotImplementedError):
        PoseNetX_R2(resnet34(), use_gnn=False)
    # unequal dims: the reference's own forward raises a shape error for them (posenet.py:974-975,1085-1086)
    for dims in ((64, 32, 64), (64, 64, 32), (32, 64, 64)):
        with pytest.raises(ValueError):
            PoseNetX_R2(resnet34(), feat_dim=dims[0], edge_feat_dim=dims[1], node_dim=dims[2], use_gnn=True)
    # the other constructor flags keep the reference's state-dict inventory (checked against it in make_golden.py)
    m2 = PoseNetX_R2(resnet34(), feat_dim=64, edge_feat_dim=64, node_dim=64, use_gnn=True, use_attention=True,
                     use_AP=False, L=2)
    assert list(m2.state_dict().keys()) == list(S.posenet_r2_param_shapes(64, 64, 64, use_attention=True, use_AP=False, L=2).keys())
    assert m2.fc_xyz.in_features == 128
    assert torch.equal(m.compute_RP(torch.arange(12.).view(4, 3), torch.tensor([[0, 3], [1, 1]])),
                       torch.tensor([[-3., -3., -3.], [6., 6., 6.]]))


def test_weight_packing():
    from oracle import posenet_ref as O
    from relpose_gnn_amd.params import pack_gnn, pack_resnet
    planes, blocks = (8, 16, 32, 64), (1, 2, 1, 1)
    sd = S.synth_state_dict(S.posenet_r2_param_shapes(64, 64, 64, planes, blocks), seed=2)
    t, b, p = pack_resnet(sd)
    assert b == list(blocks) and p == list(planes)
    assert len(t) == 4 + 8 * 5 + 4 * 3 + 2                 # {w, scale, shift, u_wino} per conv; u is None without a GPU
    assert all(v is None for v in t[3:-2:4]) and all(v is not None for i, v in enumerate(t) if i % 4 != 3 or i >= len(t) - 2)
    assert t[0].shape == (8, 7, 7, 4) and float(t[0][..., 3].abs().max()) == 0.0
    assert torch.equal(t[0][..., :3], sd["feature_extractor.conv1.weight"].permute(0, 2, 3, 1))
    # folded BN == eval-mode batch norm
    x = S.hash_normal("pk.x", (2, 8, 5, 5))
    ref = O._bn(sd, "feature_extractor.bn1.", x)
    assert torch.allclose(x * t[1].view(1, -1, 1, 1) + t[2].view(1, -1, 1, 1), ref, atol=1e-6)
    g = pack_gnn(sd)
    assert len(g) == 26 and g[22].shape == (128, 64) and g[23].shape == (192, 64) and g[24].shape == (64, 64)
    assert torch.equal(g[23][128:], sd["gnn1.mlp.0.weight"][:, :64]) and torch.equal(g[25], sd["gnn1.mlp.0.weight"][:, 64:])
    assert g[10].shape == (24, 64) and g[18].shape == (6, 64) and g[21].shape == (6,)
    assert torch.equal(g[10][8:16], sd["gnn1.att.theta.weight"]) and torch.equal(g[20][3:], sd["fc_wpqr_R.weight"])
    bad = dict(sd)
    bad.pop("feature_extractor.layer2.0.downsample.0.weight")
    with pytest.raises(ValueError):
        pack_resnet(bad)


def test_graph_containers():
    from oracle import posenet_ref as O
    assert torch.equal(fc_edge_index(8), O.fc_edge_index(8)) and torch.equal(fc_edge_index(4), O.fc_edge_index(4))
    x = torch.arange(24.).view(12, 2)
    y = torch.arange(72.).view(12, 6)
    b = fc_batch(x, 4, y)
    assert torch.equal(b.edge_index, O.batch_edge_index(4, 3)) and b.num_graphs == 3 and len(b) == 3
    assert torch.equal(b.batch, torch.tensor([0] * 4 + [1] * 4 + [2] * 4))
    assert torch.equal(b.edge_attr, y[b.edge_index[1]] - y[b.edge_index[0]])          # dataset_7Scenes_multi.py:425-429
    graphs = [Data(x=x[i * 4:(i + 1) * 4], edge_index=fc_edge_index(4), y=y[i * 4:(i + 1) * 4]) for i in range(3)]
    c = Batch.from_data_list(graphs)
    assert torch.equal(c.edge_index, b.edge_index) and torch.equal(c.x, x) and torch.equal(c.batch, b.batch)
    d = c.to("cpu")
    assert d is not c and torch.equal(d.x, c.x)


def test_synth_is_deterministic_and_reasonable():
    a = S.hash_normal("w", (1000,), 2.0, 1.0, seed=5)
    b = S.hash_normal("w", (1000,), 2.0, 1.0, seed=5)
    assert torch.equal(a, b) and not torch.equal(a, S.hash_normal("w", (1000,), 2.0, 1.0, seed=6))
    big = S.hash_normal("n", (200000,))
    assert abs(float(big.mean())) < 0.01 and abs(float(big.std()) - 1.0) < 0.01
    u = S.hash_range("u", (1000,), 0.5, 1.5)
    assert float(u.min()) >= 0.5 and float(u.max()) <= 1.5
    # pinned values: the GPU box must regenerate exactly these (the goldens were produced from this generator)
    assert [round(v, 5) for v in S.hash_normal("pin", (3,)).tolist()] == [-1.97496, -0.28621, -1.54145]


def test_stream_partition_from_pyg_batch_tables():
    """A torch_geometric Batch (what the reference's DataLoader hands the model, testing/test.py:193) carries no
    `graph_sizes`; the cut at graph boundaries comes from its collation tables or from ptr / batch."""
    import types
    from relpose_gnn_amd.graph import fc_batch
    from relpose_gnn_amd.posenet import PoseNetX_R2
    from relpose_gnn_amd.resnet import ResNet
    ref = fc_batch(torch.zeros(8 * 6, 12), 8)
    n, e = 48, 56 * 6
    want = ([8] * 6, [56] * 6)
    cum_n, cum_e = torch.arange(7) * 8, torch.arange(7) * 56
    pyg2 = types.SimpleNamespace(x=ref.x, edge_index=ref.edge_index, batch=ref.batch,
                                 _slice_dict={"x": cum_n, "edge_index": cum_e, "y": cum_n}, num_graphs=6)
    pyg1 = types.SimpleNamespace(x=ref.x, edge_index=ref.edge_index, batch=ref.batch,
                                 __slices__={"x": cum_n.tolist(), "edge_index": cum_e.tolist()})
    with_ptr = types.SimpleNamespace(x=ref.x, edge_index=ref.edge_index, batch=ref.batch, ptr=cum_n)
    only_batch = types.SimpleNamespace(x=ref.x, edge_index=ref.edge_index, batch=ref.batch)
    for d in (ref, pyg2, pyg1, with_ptr, only_batch):
        assert PoseNetX_R2._graph_sizes(d, n, e) == want
    # ragged graphs through `batch` only
    from relpose_gnn_amd.graph import Batch, Data, fc_edge_index
    rag = Batch.from_data_list([Data(x=torch.zeros(k, 12), edge_index=fc_edge_index(k)) for k in (3, 8, 5, 2)])
    bare = types.SimpleNamespace(x=rag.x, edge_index=rag.edge_index, batch=rag.batch)
    assert PoseNetX_R2._graph_sizes(bare, 18, rag.edge_index.shape[1]) == ([3, 8, 5, 2], [6, 56, 20, 2])
    # edges not grouped by graph: no contiguous cut
    perm = torch.randperm(rag.edge_index.shape[1], generator=torch.Generator().manual_seed(0))
    mixed = types.SimpleNamespace(x=rag.x, edge_index=rag.edge_index[:, perm], batch=rag.batch)
    assert PoseNetX_R2._graph_sizes(mixed, 18, rag.edge_index.shape[1]) is None
    # stale tables are rejected
    assert PoseNetX_R2._graph_sizes(pyg2, n + 8, e) is None
    m = PoseNetX_R2(ResNet((1, 1, 1, 1), (8, 16, 32, 64)), droprate=0.0, pretrained=False, feat_dim=64, edge_feat_dim=64,
                    node_dim=64, use_gnn=True)
    assert m._partition(pyg2, n, e) == [(0, 24, 0, 168, 0), (24, 48, 168, 336, 1)]
    assert m._partition(types.SimpleNamespace(x=ref.x[:8], edge_index=ref.edge_index[:, :56], batch=ref.batch[:8],
                                              num_graphs=1), 8, 56) is None
    # explicit schedules must cover every graph exactly once (equal total length is not enough)
    m.stream_schedule = [(0, 2, 0), (2, 6, 1)]
    assert m._partition(pyg2, n, e) == [(0, 16, 0, 112, 0), (16, 48, 112, 336, 1)]
    m.stream_schedule = [(3, 6, 1), (0, 3, 0)]                     # issue order is the caller's business
    assert m._partition(pyg2, n, e) == [(24, 48, 168, 336, 1), (0, 24, 0, 168, 0)]
    for bad in ([(0, 3, 0), (2, 5, 1)], [(0, 2, 0), (1, 3, 1), (3, 6, 0)], [(0, 3, 0), (4, 6, 1)], [(0, 3, 0), (3, 5, 1)],
                [(0, 4, 0), (2, 4, 1), (4, 6, 1)]):
        m.stream_schedule = bad
        with pytest.raises(ValueError):
            m._partition(pyg2, n, e)
    m.stream_schedule = None


def test_deferred_counters_are_idle_until_a_call_runs(monkeypatch):
    """A model and a QueryPose on which nothing has run have nothing to report and nothing to publish: every public entry of the
    deferred check returns without touching CUDA, and status.DeferredCounters creates no buffer at construction."""
    from relpose_gnn_amd.posenet import PoseNetX_R2
    from relpose_gnn_amd.query_pose import QueryPose
    from relpose_gnn_amd.resnet import ResNet
    from relpose_gnn_amd.status import DeferredCounters

    def touched(*a, **k):
        raise AssertionError("CUDA was touched")
    for name in ("_lazy_init", "is_current_stream_capturing", "current_stream", "Event", "Stream"):
        monkeypatch.setattr(torch.cuda, name, touched)
    monkeypatch.setattr(torch.Tensor, "pin_memory", touched)
    c = DeferredCounters(3, lambda counts: IndexError(str(counts.tolist())))
    assert c.counters is None and c._host is None and c._event is None and not c._pending
    m = PoseNetX_R2(ResNet((1, 1, 1, 1), (8, 16, 32, 64)), droprate=0.0, pretrained=False, feat_dim=64, edge_feat_dim=64,
                    node_dim=64, use_gnn=True)
    qp = QueryPose()
    for index_check in ("deferred", "sync"):
        m.index_check = index_check
        m.check_edge_index()
        m.check_edge_index(wait=False)
        m.publish_status()
    qp.check()
    qp.check(wait=False)
    qp.publish()
    c.check()
    c.check(wait=False)
    c.poll()
    c.publish()
    c.publish(sync=True)
    assert m._counters.counters is None and qp._bad.counters is None and c.counters is None


def test_stem_pair_table_matches_the_kernel():
    """params.stem_pair_table (what pack_stem_pairs packs by) == rpg_stem_pair_table (what csrc/stem.hip reads by)."""
    import ctypes as C
    from relpose_gnn_amd import _lib
    from relpose_gnn_amd.params import pack_stem_pairs, stem_pair_table
    ta, tb = (C.c_int * 222)(), (C.c_int * 222)()
    assert _lib.lib().rpg_stem_pair_table(ta, tb) == 0
    a, b = stem_pair_table()
    assert len(a) == len(b) == 74
    assert [tuple(ta[3 * i: 3 * i + 3]) for i in range(74)] == a
    assert [None if tb[3 * i] < 0 else tuple(tb[3 * i: 3 * i + 3]) for i in range(74)] == b
    taps = sorted(a + [t for t in b if t is not None])
    assert taps == sorted((c, kh, kw) for c in range(3) for kh in range(7) for kw in range(7))      # every tap exactly once
    w = torch.arange(64 * 147, dtype=torch.float32).view(64, 3, 7, 7)
    sc = torch.full((64,), 2.0)
    wp_all = pack_stem_pairs(w, sc)
    assert wp_all.shape == ((74 + 75) * 2 * 64,)                                                    # tile-kernel image, then the strip-march image
    wp = wp_all[:74 * 2 * 64].view(74, 2, 64)
    st = wp_all[74 * 2 * 64:].view(2, 75, 64)                                                       # [nf][MFMA of a convolution row][lane]
    # strip image: kernel row 0, channel 1, horizontal pair 2 = entry 3 * 1 + 2: taps (1, 0, 4) | (1, 0, 5); entry 9 * 1 + 9 + 2 = the
    # vertical pair (kh 0 | 1, kw 6) of channel 2; the last three entries are the lone (6, 6) taps with a zero partner
    assert float(st[1, 5, 7]) == 2.0 * float(w[39, 1, 0, 4]) and float(st[1, 5, 32 + 7]) == 2.0 * float(w[39, 1, 0, 5])
    assert float(st[0, 20, 3]) == 2.0 * float(w[3, 2, 0, 6]) and float(st[0, 20, 32 + 3]) == 2.0 * float(w[3, 2, 1, 6])
    assert float(st[0, 74, 3]) == 2.0 * float(w[3, 2, 6, 6]) and float(st[0, 74, 32 + 3]) == 0.0
    assert float(wp[5, 1, 7]) == 2.0 * float(w[39, a[5][0], a[5][1], a[5][2]])                      # first tap, channel 32 + 7
    assert float(wp[5, 1, 32 + 7]) == 2.0 * float(w[39, b[5][0], b[5][1], b[5][2]])                # second tap
    assert float(wp[73, 0, 40]) == 0.0                                                              # the missing partner


def test_host_f32_to_bf16_is_round_to_nearest_even():
    """rpg_host_f32_to_bf16 (the staging threads of evaluate_stream round the bf16 encoder's node images with it) against torch's
    fp32 -> bf16 conversion -- which is also what the stem kernel's own (__bf16)float does -- on normal values across the whole
    exponent range, ties, zeros, infinities, denormals, the largest finite value (rounds to inf) and every NaN payload class."""
    from relpose_gnn_amd import _lib
    lib = _lib.lib()
    g = torch.Generator().manual_seed(11)
    x = torch.randn(1 << 18, generator=g) * torch.logspace(-40, 38, 1 << 18)
    x[:10] = torch.tensor([float("nan"), float("inf"), -float("inf"), 0.0, -0.0, 1e-45, 3.3895313892515355e38, -1.0, 1.00390625, 1.01171875])
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (1 << 18,), dtype=torch.int64, generator=g).to(torch.int32).view(torch.float32)
    for t in (x, bits):
        out = torch.empty(t.shape, dtype=torch.bfloat16)
        assert lib.rpg_host_f32_to_bf16(t.data_ptr(), out.data_ptr(), t.numel()) == _lib.RPG_OK
        ref = t.bfloat16()
        nan = torch.isnan(ref)
        assert torch.equal(out.view(torch.int16)[~nan], ref.view(torch.int16)[~nan])
        assert torch.isnan(out[nan]).all() and nan.sum() == torch.isnan(t).sum()
    assert lib.rpg_host_f32_to_bf16(None, None, 0) == _lib.RPG_OK and lib.rpg_host_f32_to_bf16(None, None, 4) == _lib.RPG_ERR_BAD_ARG
    # round 6: the vector variants (AVX2 / AVX-512F where this CPU has them) are the scalar loop's arithmetic on 8 / 16 lanes: bit for bit
    # the same, at every length (scalar head up to the 32-byte store alignment, vector body, scalar tail) and destination alignment
    both = torch.cat([x, bits])
    want = torch.empty(both.shape, dtype=torch.bfloat16)
    assert lib.rpg_host_f32_to_bf16_isa(both.data_ptr(), want.data_ptr(), both.numel(), 1) == _lib.RPG_OK
    ran = 0
    for isa in (0, 2, 3):
        for n, off in ((both.numel(), 0), (1000, 3), (31, 1), (16, 0), (15, 5), (1, 0), (0, 0)):
            out = torch.full((n + off + 16,), 7.0, dtype=torch.bfloat16)
            rc = lib.rpg_host_f32_to_bf16_isa(both.data_ptr(), out.data_ptr() + 2 * off, n, isa)
            if rc == _lib.RPG_ERR_BAD_ARG and isa in (2, 3):
                break                                                              # this CPU lacks the instruction set
            assert rc == _lib.RPG_OK
            assert torch.equal(out.view(torch.int16)[off:off + n], want.view(torch.int16)[:n]), (isa, n, off)
            assert bool((out[:off] == 7.0).all()) and bool((out[off + n:] == 7.0).all()), (isa, n, off)      # nothing written outside
            ran += 1
    assert ran >= 7
    assert lib.rpg_host_f32_to_bf16_isa(both.data_ptr(), want.data_ptr(), 4, 9) == _lib.RPG_ERR_BAD_ARG


# ---- the composite forwards' workspace plan (csrc/composite_plan.h) ---------------------------------------------------------------
# Bytes every size function returned BEFORE the layouts moved into composite_plan.h, recorded from a build of that commit (256 CUs:
# the count the library assumes without a GPU, and the MI355X's).  Every buffer keeps its place, so the sizes keep their value.
_RESNET34, _TINY, _STEEP = (64, 128, 256, 512), (8, 16, 32, 64), (8, 64, 512, 4096)      # _STEEP: the LAST layer owns the largest block buffer
ENCODER_BYTES = [    # (planes, (n, h, w), fp32, bf16)
    (_RESNET34, (1, 224, 224), 110069760, 5907456),
    (_RESNET34, (8, 256, 341), 203948032, 58032128),
    (_RESNET34, (256, 224, 224), 1953054720, 1029758976),
    (_RESNET34, (3, 33, 47), 103568128, 2292480),
    (_TINY, (2, 32, 40), 102924800, 1954048),
    (_STEEP, (2, 64, 64), 103596032, 2334720),
]
GNN_BYTES = [        # ((n, e, d), bytes); (3, 1, 32) and (2000, 100, 64): e < 2n
    ((8, 56, 2048), 109488640), ((256, 1792, 2048), 223323392), ((8, 56, 64), 105933312), ((3, 1, 32), 105822976),
    ((2000, 100, 64), 110098944), ((1, 1, 32), 105820928),
]
QUERY_BYTES = [      # ((n, e, d, e_sel, q), bytes)
    ((8, 56, 64, 7, 1), 107559168), ((256, 1792, 2048, 224, 32), 228229120), ((8, 56, 64, 56, 8), 107582976),
]


def test_workspace_size_functions_return_what_they_always_did():
    from relpose_gnn_amd import _lib
    lib = _lib.lib()
    for planes, (n, h, w), f32, bf16 in ENCODER_BYTES:
        p = _lib.int_array(list(planes))
        assert lib.rpg_resnet_workspace_bytes(n, h, w, p) == f32, (planes, n, h, w)
        assert lib.rpg_resnet_bf16_workspace_bytes(n, h, w, p) == bf16, (planes, n, h, w)
    for shape, nbytes in GNN_BYTES:
        assert lib.rpg_gnn_workspace_bytes(*shape) == nbytes, shape
    for shape, nbytes in QUERY_BYTES:
        assert lib.rpg_gnn_query_workspace_bytes(*shape) == nbytes, shape
    # refused shapes: 0
    p = _lib.int_array(list(_RESNET34))
    for fn in (lib.rpg_resnet_workspace_bytes, lib.rpg_resnet_bf16_workspace_bytes):
        for bad in ((0, 224, 224), (1, 0, 224), (1, 224, 0), (-1, 224, 224)):
            assert fn(*bad, p) == 0, bad
        assert fn(1, 224, 224, None) == 0
    for bad in ((0, 56, 64), (8, 0, 64), (8, 56, 0), (8, 56, 100), (-8, 56, 64)):          # n = 0, e = 0, d = 0, d % 32 != 0
        assert lib.rpg_gnn_workspace_bytes(*bad) == 0, bad
    for bad in ((8, 56, 64, 0, 1), (8, 56, 64, 57, 1), (8, 56, 64, 7, 0), (8, 56, 64, 7, 9), (8, 56, 100, 7, 1),      # e_sel = 0, e_sel > e, q = 0, q > n
                (0, 56, 64, 7, 1), (8, 0, 64, 7, 1), (8, 56, 0, 7, 1)):
        assert lib.rpg_gnn_query_workspace_bytes(*bad) == 0, bad


def test_set_tuning_accepts_what_it_always_did():
    """tests/tuning_accepted.json: for every key, the values among -3 .. 4100, (64 << 12) | 8, 1 << 20, INT_MAX and INT_MIN that
    rpg_set_tuning accepted BEFORE the keys moved into csrc/tuning.h, recorded from a build of that commit as closed intervals.
    The table's predicates must give the same answer for every key and value."""
    import json
    from relpose_gnn_amd import _lib, ops
    lib = _lib.lib()
    accepted = json.load(open(os.path.join(ROOT, "tests", "tuning_accepted.json")))
    assert list(accepted) == list(ops.TUNING_KEYS)
    values = list(range(-3, 4101)) + [1 << 12, (64 << 12) | 8, 1 << 20, 2 ** 31 - 1, -2 ** 31]
    try:
        for name, intervals in accepted.items():
            key = getattr(ops, "TUNE_" + name)
            for v in values:
                want = any(lo <= v <= hi for lo, hi in intervals)
                assert (lib.rpg_set_tuning(key, v) == _lib.RPG_OK) == want, (name, v)
    finally:
        ops.reset_tuning()


def _build_and_run_host_check(tmp_path, name):
    import shutil
    import subprocess
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / name)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", name + ".cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_tuning_header_stands_alone(tmp_path):
    """tests/tuning_check.cpp includes nothing of the project but csrc/tuning.h (which needs the C header and no HIP): every key's
    raw default against a list of its own, the decoded default state field by field, and the packed keys' decoding at chosen values."""
    assert "tuning: ok (32 keys)" in _build_and_run_host_check(tmp_path, "tuning_check")


def test_composite_plan_header_stands_alone(tmp_path):
    """tests/composite_plan_check.cpp includes nothing of the project but csrc/composite_plan.h: the host compiler alone builds it
    (the header needs no HIP).  It carves every buffer set into a host buffer of exactly the dry run's size, tags every buffer over
    its full extent, re-reads the tags (overlap), checks alignment and bounds, and walks ResnetWalk against plain nested loops."""
    assert "composite_plan: ok" in _build_and_run_host_check(tmp_path, "composite_plan_check")
