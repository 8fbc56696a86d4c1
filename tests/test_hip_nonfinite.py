"""Non-finite inputs: the HIP kernels and the HIP forward propagate NaN / inf like the reference (tests/test_nonfinite_cpu.py pins
the reference's contract on the CPU oracle).

Per kernel, one bad value (+NaN, -NaN, +inf, -inf) goes into one image (or row) that has clean neighbours on both sides in the
launch, and the result is compared with the same launch on clean input and with a float64 CPU statement of the op:
  (a) isolation: every output of the other images / rows is bit-identical to the clean launch (a multiply-by-zero of a
      neighbour's value would break this: NaN * 0 = NaN);
  (b) no swallowing: where the reference is NaN the kernel is NaN, where it is +-inf the kernel is non-finite;
  (c) footprint: for the direct convolutions, the Linears and the pools the non-finite mask is the reference's; the Winograd
      F(4,3) kernel poisons its whole 4 x 4 output tile (and inf - inf = NaN) by construction, and the stems' packings add
      zero-weight taps next to the 7 x 7 window, so those are held to a stated superset inside the poisoned image.
Model level: every abs row of the poisoned graph and every rel row of its edges is non-finite, every other graph bit-identical
to the forward of the clean batch (same shapes, so the same launch geometry)."""

import pytest
import torch
import torch.nn.functional as F

from relpose_gnn_amd import ops

pytestmark = pytest.mark.gpu

NEG_NAN = torch.tensor([0xFFC00000 - 2 ** 32], dtype=torch.int32).view(torch.float32).item()      # 0xFFC00000: a quiet NaN, sign bit set
BAD = {"nan": float("nan"), "-nan": NEG_NAN, "inf": float("inf"), "-inf": float("-inf")}
BITS32 = {"nan": 0x7FC00000, "-nan": 0xFFC00000, "inf": 0x7F800000, "-inf": 0xFF800000}


def _put(t, idx, kind):
    """t[idx] = the value `kind`, written as a bit pattern: element assignment (and Tensor.bfloat16()) canonicalizes a NaN, which
    would turn -NaN into +NaN on the bf16 paths.  A finite `kind` (a float) is assigned as is."""
    if not isinstance(kind, str):
        t[idx] = kind
        return
    b = BITS32[kind]
    if t.dtype == torch.bfloat16:
        h = b >> 16
        t.view(torch.int16)[idx] = h - (1 << 16) if h >= 1 << 15 else h
    else:
        assert t.dtype == torch.float32
        t.view(torch.int32)[idx] = b - (1 << 32) if b >= 1 << 31 else b


def _vid(v):
    return ",".join(f"{k}={x}" for k, x in v.items()) or "default"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _check(got, clean, ref, img, exact=True, within=None, whole=True):
    """got / clean: kernel outputs (poisoned / clean input), ref: float64 reference of the poisoned input (whole = False: of the
    poisoned image / row alone); dim 0 = image or row.  within: optional bool mask of the poisoned image's outputs the kernel may
    poison beyond the reference (superset bound)."""
    got, clean, ref = got.double().cpu(), clean.double().cpu(), ref.double().cpu()
    others = torch.ones(got.shape[0], dtype=torch.bool)
    others[img] = False
    assert bool(torch.isfinite(clean).all())
    assert torch.equal(got[others], clean[others]), "a bad value leaked into another image / row"          # (a)
    g, r = got[img], (ref[img] if whole else ref)
    assert bool(torch.isnan(r).any()) or bool(torch.isinf(r).any()), "test input does not reach the output"
    assert bool(torch.isnan(g)[torch.isnan(r)].all()), "NaN swallowed"                                       # (b)
    assert bool((~torch.isfinite(g))[torch.isinf(r)].all()), "inf swallowed"
    if exact:                                                                                                 # (c)
        assert torch.equal(~torch.isfinite(g), ~torch.isfinite(r)), "non-finite footprint differs from the reference"
        z = g[r == 0]
        if z.numel():
            # ReLU zeros (those from -inf among them) stay zeros, up to the kernel's rounding next to zero (the bf16 parity bar)
            assert bool(torch.isfinite(z).all()), "a ReLU zero became non-finite"
            assert float(z.abs().max()) <= 1e-2 * float(r[torch.isfinite(r)].abs().max()), "a ReLU zero moved"
    elif within is not None:
        assert bool(within[~torch.isfinite(g)].all()), "non-finite outputs beyond the kernel's stated bound"
    return g, r


# ---------------------------------------------------------------------------------------------------------------------------- fp32
@pytest.mark.parametrize("kind", list(BAD))
@pytest.mark.parametrize("k,stride,pad,relu", [(3, 2, 1, True), (1, 2, 0, False), (3, 1, 1, True)])
def test_conv_f32(dev, kind, k, stride, pad, relu):
    from relpose_gnn_amd import ops
    n, h, w, cin, cout = 3, 14, 14, 64, 128
    x = _rand(n, h, w, cin, seed=1)
    wt = _rand(cout, k, k, cin, seed=2, scale=(2.0 / (cin * k * k)) ** 0.5)
    sc, sh = torch.rand(cout, generator=torch.Generator().manual_seed(3)) + 0.5, _rand(cout, seed=4, scale=0.1)
    args = (wt.to(dev), sc.to(dev), sh.to(dev), None)
    clean = ops.conv2d_bn_act_nhwc(x.to(dev), *args, stride=stride, pad=pad, relu=relu)
    for (y, xx) in ((0, 0), (6, 8), (h - 1, w - 1)):                 # corner (padding taps), interior (even: stride 2 samples it), last
        xb = x.clone()
        _put(xb, (1, y, xx, 5), kind)
        got = ops.conv2d_bn_act_nhwc(xb.to(dev), *args, stride=stride, pad=pad, relu=relu)
        ref = F.conv2d(xb.double().permute(0, 3, 1, 2), wt.double().permute(0, 3, 1, 2), None, stride=stride, padding=pad)
        ref = ref * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
        ref = (F.relu(ref) if relu else ref).permute(0, 2, 3, 1)
        if not bool((~torch.isfinite(ref[1])).any()):
            continue                                                 # the stride skips this pixel
        _check(got, clean, ref, 1)


@pytest.mark.parametrize("kind", list(BAD))
@pytest.mark.parametrize("relu", [True, False])
def test_wino43_f32(dev, kind, relu):
    from relpose_gnn_amd import ops
    n, h, w, c = 3, 28, 28, 64
    x = _rand(n, h, w, c, seed=5)
    wt = _rand(c, 3, 3, c, seed=6, scale=(2.0 / (9 * c)) ** 0.5)
    sc, sh = torch.rand(c, generator=torch.Generator().manual_seed(7)) + 0.5, _rand(c, seed=8, scale=0.1)
    u = ops.wino43_transform_weights(wt.to(dev))
    clean = ops.conv3x3_wino43_bn_act_nhwc(x.to(dev), u, sc.to(dev), sh.to(dev), None, relu=relu)
    for (y, xx) in ((0, 0), (13, 9), (h - 1, w - 1)):
        xb = x.clone()
        _put(xb, (1, y, xx, 3), kind)
        got = ops.conv3x3_wino43_bn_act_nhwc(xb.to(dev), u, sc.to(dev), sh.to(dev), None, relu=relu)
        ref = F.conv2d(xb.double().permute(0, 3, 1, 2), wt.double().permute(0, 3, 1, 2), None, padding=1)
        ref = ref * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
        ref = (F.relu(ref) if relu else ref).permute(0, 2, 3, 1)
        # bound: the 4 x 4 output tiles whose 6 x 6 input tile holds the bad pixel (tiles start at multiples of 4, input rows 4t-1..4t+4)
        within = torch.zeros(h, w, c, dtype=torch.bool)
        for ty in range(0, h, 4):
            for tx in range(0, w, 4):
                if ty - 1 <= y <= ty + 4 and tx - 1 <= xx <= tx + 4:
                    within[ty:ty + 4, tx:tx + 4] = True
        g, r = _check(got, clean, ref, 1, exact=False, within=within)
        if not relu:
            # the defect this case was written for: "no ReLU" as max(y, -inf) turned a NaN into -inf
            assert not bool((torch.isnan(r) & torch.isinf(g)).any())


@pytest.mark.parametrize("kind", list(BAD))
def test_maxpool_f32(dev, kind):
    from relpose_gnn_amd import ops
    x = _rand(3, 15, 16, 64, seed=9)
    clean = ops.maxpool3x3s2_nhwc(x.to(dev))
    for (y, xx) in ((0, 0), (7, 8), (14, 15)):
        xb = x.clone()
        _put(xb, (1, y, xx, 7), kind)
        got = ops.maxpool3x3s2_nhwc(xb.to(dev))
        ref = F.max_pool2d(xb.double().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
        if kind == "-inf":                                           # -inf never wins a max: every output is the reference's, exactly
            assert torch.equal(got.cpu().double(), ref)
            continue
        _check(got, clean, ref, 1)


@pytest.mark.parametrize("kind", list(BAD))
@pytest.mark.parametrize("relu", [False, True])
def test_linear_gather(dev, kind, relu):
    from relpose_gnn_amd import ops
    m, k, n_out = 112 * 3, 192, 128                                  # exact-fit 112-row tiles
    a = _rand(m, k, seed=10)
    wt, b = _rand(n_out, k, seed=11, scale=k ** -0.5), _rand(n_out, seed=12, scale=0.1)
    clean, clean_r = ops.linear_gather_ex([(a.to(dev), None)], wt.to(dev), b.to(dev), m, relu=relu, want_relu_copy=True)
    for row in (0, 111, 112, m - 1):
        ab = a.clone()
        _put(ab, (row, 17), kind)
        got, got_r = ops.linear_gather_ex([(ab.to(dev), None)], wt.to(dev), b.to(dev), m, relu=relu, want_relu_copy=True)
        ref = ab.double() @ wt.double().T + b.double()
        _check(got, clean, F.relu(ref) if relu else ref, row)
        _check(got_r, clean_r, F.relu(ref), row)
        got1 = ops.linear_gather([(ab.to(dev), None)], wt.to(dev), b.to(dev), m, relu=relu)
        _check(got1, ops.linear_gather([(a.to(dev), None)], wt.to(dev), b.to(dev), m, relu=relu), F.relu(ref) if relu else ref, row)


def _stem_ref(x, wt, sc, sh, bf16):
    xx, ww = (x.bfloat16().double(), wt.bfloat16().double()) if bf16 else (x.double(), wt.double())
    conv = F.conv2d(xx, ww, None, stride=2, padding=3) * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
    return F.max_pool2d(F.relu(conv), 3, 2, 1).permute(0, 2, 3, 1)


# Input rows / columns a convolution output (oy, ox) of each stem kernel reads, relative to (2 oy, 2 ox); the 7 x 7 window is
# -3 .. +3, and each packing adds one zero-weight tap on ONE side (params.pack_stem_pairs / pack_stem_bf16, csrc/stem*.hip):
STEM_READS = {
    ("f32", 1): ((-3, 3), (-3, 4)),        # tile: the lone last tap pair (2, 6, 6) | next column (2, 6, 7)
    ("f32", 129): ((-3, 4), (-3, 3)),      # strip: the lone (6, 6) taps as a vertical pair with kernel row 7
    ("bf16", 1): ((-3, 4), (-4, 3)),       # strip: kernel row 7 and window column -1 carry zero weights
    ("bf16", 33): ((-3, 4), (-4, 3)),
    ("bf16", 3): ((-3, 3), (-3, 4)),       # tile: 8th kernel column (the zero 22nd (c, kh) row re-reads row (2, 6))
}


def _stem_bound(h, w, y, xx, reads):
    """pooled outputs the bad input pixel (y, xx) may reach through the kernel's widened window -> convolution outputs -> pool"""
    (r0, r1), (c0, c1) = reads
    hc, wc = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    hp, wp = (hc - 1) // 2 + 1, (wc - 1) // 2 + 1
    conv = torch.zeros(hc, wc, dtype=torch.bool)
    for oy in range(hc):
        for ox in range(wc):
            conv[oy, ox] = 2 * oy + r0 <= y <= 2 * oy + r1 and 2 * ox + c0 <= xx <= 2 * ox + c1
    pooled = F.max_pool2d(conv.double().view(1, 1, hc, wc), 3, 2, 1).view(hp, wp) > 0
    return pooled.view(hp, wp, 1).expand(hp, wp, 64)


@pytest.mark.parametrize("kind", list(BAD))
@pytest.mark.parametrize("kernel", [1, 1 + 128])                        # RPG_TUNE_FUSED_STEM of the fp32 stem: tile, strip
def test_fused_stem_f32(dev, kind, kernel):
    from relpose_gnn_amd import ops
    from relpose_gnn_amd.params import pack_stem_pairs
    n, h, w = 3, 37, 53
    x = _rand(n, 3, h, w, seed=13)
    wt = _rand(64, 3, 7, 7, seed=2, scale=(2.0 / 147) ** 0.5)
    sc, sh = torch.rand(64, generator=torch.Generator().manual_seed(3)) + 0.5, _rand(64, seed=4, scale=0.3)
    wp = pack_stem_pairs(wt, sc).to(dev)
    with ops.tuned({ops.TUNE_FUSED_STEM: kernel}):
        clean = ops.stem_conv_bn_relu_maxpool(x.to(dev), wp, sh.to(dev))
        for (c, y, xx) in ((0, 0, 0), (1, 20, 27), (2, h - 1, w - 1)):
            xb = x.clone()
            _put(xb, (1, c, y, xx), kind)
            got = ops.stem_conv_bn_relu_maxpool(xb.to(dev), wp, sh.to(dev))
            ref = _stem_ref(xb, wt, sc, sh, False)
            if kind == "-inf" and not bool((~torch.isfinite(ref[1])).any()):
                continue                                             # -inf after a ReLU and a max-pool is often gone
            _check(got, clean, ref, 1, exact=False, within=_stem_bound(h, w, y, xx, STEM_READS[("f32", kernel)]))


@pytest.mark.parametrize("kind", list(BAD))
@pytest.mark.parametrize("kernel", [1, 33, 3])                          # RPG_TUNE_FUSED_STEM of the bf16 stem: strip (2 / 1 halves per wave), tile
@pytest.mark.parametrize("in_bf16", [False, True])
def test_fused_stem_bf16(dev, kind, kernel, in_bf16):
    """37 x 53: 3 h w is odd, so with bf16 input the images of odd index start 2 bytes into a dword and the last element of one
    image shares a dword with the first of the next: the bad value sits in the first / last element of the middle image."""
    from relpose_gnn_amd import ops
    from relpose_gnn_amd.params import pack_stem_bf16
    n, h, w = 3, 37, 53
    x = _rand(n, 3, h, w, seed=14)
    wt = _rand(64, 3, 7, 7, seed=2, scale=(2.0 / 147) ** 0.5)
    sc, sh = torch.rand(64, generator=torch.Generator().manual_seed(3)) + 0.5, _rand(64, seed=4, scale=0.3)
    wp = pack_stem_bf16(wt).to(dev)
    xin = x.bfloat16() if in_bf16 else x
    with ops.tuned({ops.TUNE_FUSED_STEM: kernel}):
        clean = ops.stem_conv_bn_relu_maxpool_bf16(xin.to(dev), wp, sc.to(dev), sh.to(dev))
        for (c, y, xx) in ((0, 0, 0), (1, 20, 27), (2, h - 1, w - 1)):
            xb = xin.clone()
            _put(xb, (1, c, y, xx), kind)                            # the sign of the NaN reaches the kernel (bit pattern)
            got = ops.stem_conv_bn_relu_maxpool_bf16(xb.to(dev), wp, sc.to(dev), sh.to(dev))
            ref = _stem_ref(xb.float(), wt, sc, sh, True)
            if kind == "-inf" and not bool((~torch.isfinite(ref[1])).any()):
                continue
            _check(got.float(), clean.float(), ref, 1, exact=False, within=_stem_bound(h, w, y, xx, STEM_READS[("bf16", kernel)]))


@pytest.mark.parametrize("kind", list(BAD) + ["3e38"])
@pytest.mark.parametrize("fast", [1, 0], ids=["interleaved", "general"])
@pytest.mark.parametrize("k,stride,pad,relu", [(3, 1, 1, True), (1, 2, 0, False)])
def test_conv_bf16(dev, kind, fast, k, stride, pad, relu):
    from relpose_gnn_amd import ops
    n, h, w, cin, cout = 3, 14, 14, 64, 128
    x = _rand(n, h, w, cin, seed=15).bfloat16()
    wt = _rand(cout, k, k, cin, seed=16, scale=(2.0 / (cin * k * k)) ** 0.5).bfloat16()
    sc, sh = torch.rand(cout, generator=torch.Generator().manual_seed(17)) + 0.5, _rand(cout, seed=18, scale=0.1)
    v = 3e38 if kind == "3e38" else kind
    with ops.tuned({ops.TUNE_BF16_FAST: fast}):
        run = lambda t: ops.conv2d_bn_act_nhwc_bf16(t.to(dev), wt.to(dev), sc.to(dev), sh.to(dev), None, stride=stride, pad=pad, relu=relu)
        clean = run(x)
        for (y, xx) in ((0, 0), (6, 8), (h - 1, w - 1)):
            xb = x.clone()
            _put(xb, (1, y, xx, 5), v)
            if kind == "3e38":                                       # finite in bf16, overflows once multiplied and accumulated
                _put(xb, (1, y, xx, 6), v)
            got = run(xb)
            ref = F.conv2d(xb.double().permute(0, 3, 1, 2), wt.double().permute(0, 3, 1, 2), None, stride=stride, padding=pad)
            ref = ref * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
            ref = (F.relu(ref) if relu else ref).permute(0, 2, 3, 1)
            if kind == "3e38":
                ref = ref.float().bfloat16().double()                # what overflows is the bf16 output
            if not bool((~torch.isfinite(ref[1])).any()):
                continue
            _check(got.float(), clean.float(), ref, 1, exact=kind != "3e38")


# --------------------------------------------------------------------------------------------------------------------- model level
def _model(dev, sd_patch=None, knn=-1, img_h=32):
    import relpose_gnn_amd.synth as S
    from relpose_gnn_amd.posenet import PoseNetX_R2
    from relpose_gnn_amd.resnet import ResNet
    D, planes, blocks = 64, (64, 16, 32, 64), (1, 1, 1, 1)
    m = PoseNetX_R2(ResNet(blocks, planes), droprate=0.0, pretrained=False, feat_dim=D, edge_feat_dim=D, node_dim=D,
                    input_img_height=img_h, use_gnn=True, knn=knn, use_AP=True, gnn_recursion=2)
    sd = S.synth_state_dict(S.posenet_r2_param_shapes(D, D, D, planes, blocks), seed=1)
    if sd_patch:
        sd_patch(sd)
    m.load_state_dict(sd)
    return m.to(dev).eval()


def _poison(x, img, h, w, pos, kind):
    xb = x.clone()
    flat = {"first": 0, "mid": (3 * h * w) // 2 + w // 3, "last": 3 * h * w - 1}[pos]
    _put(xb, (img, flat), kind)
    return xb


def _graph_check(a, r, a0, r0, ei, g, nodes=8):
    a, r, a0, r0, ei = a.cpu(), r.cpu(), a0.cpu(), r0.cpu(), ei.cpu()
    rows = torch.zeros(a.shape[0], dtype=torch.bool)
    rows[g * nodes:(g + 1) * nodes] = True
    edges = (ei[0] // nodes == g) & (ei[1] // nodes == g)
    assert bool(torch.isfinite(a0).all()) and bool(torch.isfinite(r0).all())
    assert bool((~torch.isfinite(a[rows])).any(dim=1).all()), "a poisoned graph's abs pose came out finite"
    assert bool((~torch.isfinite(r[edges])).any(dim=1).all()), "a poisoned graph's rel pose came out finite"
    assert torch.equal(a[~rows], a0[~rows]) and torch.equal(r[~edges], r0[~edges]), "another graph changed"


@pytest.mark.parametrize("kind", list(BAD))
@pytest.mark.parametrize("enc,gnn,streams", [("f32", "f32", 1), ("f32", "f32", 2), ("f32", "f32", 3), ("bf16", "f32", 2),
                                             ("bf16", "bf16", 1), ("bf16", "bf16", 3)])
def test_model_bad_pixel_poisons_its_graph_only(dev, kind, enc, gnn, streams):
    import relpose_gnn_amd.synth as S
    from relpose_gnn_amd.graph import fc_batch
    h, w = (32, 40) if enc == "f32" else (37, 53)                   # bf16: an odd-sized image (3 h w odd)
    m = _model(dev, img_h=h)
    m.encoder_dtype, m.gnn_dtype, m.hip_streams = enc, gnn, streams
    x = S.synth_images(4 * 8, h, w, seed=21)
    a0, r0, ei = [t.clone() for t in m(fc_batch(x, 8).to(dev))]
    for img, pos in ((9, "mid"), (16, "first"), (15, "last")):      # graph 1 inside / first node of graph 2 / last node of graph 1
        d = fc_batch(_poison(x, img, h, w, pos, kind), 8).to(dev)
        a, r, _ = m(d)
        _graph_check(a, r, a0, r0, ei, img // 8)


@pytest.mark.parametrize("kind", list(BAD))
def test_graph_replay_and_knn_bad_pixel(dev, kind):
    import relpose_gnn_amd.synth as S
    from relpose_gnn_amd.graph import fc_batch
    from relpose_gnn_amd.graphed import GraphedForward
    m = _model(dev)
    x = S.synth_images(4 * 8, 32, 40, seed=22)
    d0 = fc_batch(x, 8).to(dev)
    a0, r0, ei = [t.clone() for t in m(d0)]
    runner = GraphedForward(m, fc_batch(x, 8).to(dev))
    a, r, _ = runner(fc_batch(_poison(x, 20, 32, 40, "mid", kind), 8).to(dev))
    _graph_check(a, r, a0, r0, ei, 2)
    # kNN graph (knn = 4): the other graphs' edges and poses are unchanged, every index stays inside its own graph
    mk = _model(dev, knn=4)
    ak0, rk0, ek0 = [t.clone().cpu() for t in mk(d0)]
    ak, rk, ek = [t.cpu() for t in mk(fc_batch(_poison(x, 20, 32, 40, "mid", kind), 8).to(dev))]
    assert bool((ek[0] // 8 == ek[1] // 8).all())
    keep0, keep = ek0[0] // 8 != 2, ek[0] // 8 != 2
    assert torch.equal(ek0[:, keep0], ek[:, keep]) and torch.equal(rk0[keep0], rk[keep])
    rows = torch.arange(32) // 8 != 2
    assert torch.equal(ak0[rows], ak[rows]) and bool((~torch.isfinite(ak[20])).any())


@pytest.mark.parametrize("kind", list(BAD))
@pytest.mark.parametrize("bf16", [False, True])
def test_evaluate_stream_bad_frame(dev, bf16, kind):
    import relpose_gnn_amd.synth as S
    from relpose_gnn_amd import evaluate as E
    from relpose_gnn_amd.graph import Data, fc_edge_index
    m = _model(dev)
    if bf16:
        m.encoder_dtype, m.gnn_dtype = "bf16", "bf16"
    xs = [S.synth_images(8, 32, 40, seed=300 + i) for i in range(5)]
    ys = [S.hash_normal(f"nf.y{i}", (8, 6), 0.3) for i in range(5)]
    graphs = [Data(x=x, edge_index=fc_edge_index(8), y=y) for x, y in zip(xs, ys)]
    p0 = E.evaluate_stream(m, graphs, dev, micro_batch=2).pred_poses
    bad = [Data(x=g.x.clone(), edge_index=g.edge_index, y=g.y) for g in graphs]
    _put(bad[2].x, (3, 100), kind)
    p = E.evaluate_stream(m, bad, dev, micro_batch=2).pred_poses
    p, p0 = torch.as_tensor(p), torch.as_tensor(p0)
    assert bool((~torch.isfinite(p[2])).any()), "the bad frame's graph came out finite"
    keep = torch.arange(p.shape[0]) != 2
    assert torch.equal(p[keep], p0[keep])


@pytest.mark.parametrize("enc", ["f32", "bf16"])
def test_model_nan_weight_poisons_everything(dev, enc):
    import relpose_gnn_amd.synth as S
    from relpose_gnn_amd.graph import fc_batch

    def patch(sd):
        w = sd["feature_extractor.layer3.0.conv1.weight"].clone()
        w.view(-1)[w.numel() // 3] = float("nan")
        sd["feature_extractor.layer3.0.conv1.weight"] = w
    m = _model(dev, sd_patch=patch)
    m.encoder_dtype = enc
    a, r, _ = m(fc_batch(S.synth_images(3 * 8, 32, 40, seed=23), 8).to(dev))
    assert bool(torch.isnan(a).any(dim=1).all()) and bool(torch.isnan(r).any(dim=1).all())


# ------------------------------------------------------------------------------------------------- kernel variants (tuning keys)
# The variants of tests/test_hip_ops.py and tests/test_hip_bf16.py, at shapes on which they are dispatched; the bad value goes into
# an image in the middle of the launch (and, for the Winograd split-K tail, into one of the last images).  References are float64
# statements of the poisoned image alone, shared by the variants of one shape.
_REF_CACHE = {}


def _conv_ref1(key, x1, w, sc, sh, stride, pad, relu, r1=None, bf16_out=False):
    """float64 conv + BN (+ residual) (+ ReLU) of ONE image x1 [h][w][cin] (NHWC) -> [ho][wo][cout]; cached under key"""
    if key not in _REF_CACHE:
        y = F.conv2d(x1.double().permute(2, 0, 1)[None], w.double().permute(0, 3, 1, 2), None, stride=stride, padding=pad)[0]
        y = y * sc.double().view(-1, 1, 1) + sh.double().view(-1, 1, 1)
        if r1 is not None:
            y = y + r1.double().permute(2, 0, 1)
        y = (F.relu(y) if relu else y).permute(1, 2, 0)
        _REF_CACHE[key] = y.float().bfloat16().double() if bf16_out else y
    return _REF_CACHE[key]


def _positions(h, w):
    return ((0, 0), (h // 2 & ~1, w // 2 & ~1), (h - 1, w - 1))     # corner (padding taps), interior (even: stride 2 samples it), last


CONV_F32_VARIANTS = [{}, {"TILE": 0, "STREAMK": 0, "BK": 16}, {"TILE": 1, "STREAMK": 1, "BK": 32}, {"TILE": 2, "STREAMK": 0, "EPILOGUE": 0},
                     {"TILE": 3, "STREAMK": 1, "BK": 16}, {"TILE": 0, "STREAMK": 1}, {"FAST_LOADER": 0}, {"WAVES8": 0}]
CONV_F32_SHAPES = [(9, 28, 28, 128, 256, 3, 2, 1, True, True),   # 8-wave tiles with a stream-K remainder, residual
                   (7, 30, 22, 64, 160, 1, 2, 0, False, False),  # 1x1/2 downsample, no ReLU
                   (3, 13, 17, 64, 72, 3, 2, 1, True, True)]     # buffer loaders: ragged M and N, padding taps


@pytest.mark.parametrize("kind", list(BAD))
@pytest.mark.parametrize("shape", CONV_F32_SHAPES, ids=lambda s: "x".join(map(str, s[:8])))
@pytest.mark.parametrize("variant", CONV_F32_VARIANTS, ids=_vid)
def test_conv_f32_variants(dev, variant, shape, kind):
    from relpose_gnn_amd import ops
    n, h, w, cin, cout, k, st, pad, res, relu = shape
    x = _rand(n, h, w, cin, seed=41)
    wt = _rand(cout, k, k, cin, seed=42, scale=(2.0 / (cin * k * k)) ** 0.5)
    sc, sh = torch.rand(cout, generator=torch.Generator().manual_seed(43)) + 0.5, _rand(cout, seed=44, scale=0.1)
    ho, wo = (h + 2 * pad - k) // st + 1, (w + 2 * pad - k) // st + 1
    r = _rand(n, ho, wo, cout, seed=45) if res else None
    img = n // 2
    args = (wt.to(dev), sc.to(dev), sh.to(dev), None if r is None else r.to(dev))
    with ops.tuned(variant):
        clean = ops.conv2d_bn_act_nhwc(x.to(dev), *args, stride=st, pad=pad, relu=relu)
        for (y, xx) in _positions(h, w):
            xb = x.clone()
            _put(xb, (img, y, xx, 5), kind)
            got = ops.conv2d_bn_act_nhwc(xb.to(dev), *args, stride=st, pad=pad, relu=relu)
            ref = _conv_ref1(("f32", shape, kind, y, xx), xb[img], wt, sc, sh, st, pad, relu, None if r is None else r[img])
            if not bool((~torch.isfinite(ref)).any()):
                continue
            _check(got, clean, ref, img, whole=False)


WINO_VARIANTS = [{}, {"WINOGRAD": 2}, {"WINOGRAD": 3}, {"WINOGRAD": 3, "WINO_PERSIST": 1, "WINO_SPLIT": 1},
                 {"WINOGRAD": 3, "WINO_PERSIST": 0, "WINO_SPLIT": 1}, {"WINOGRAD": 3, "WINO_PERSIST": 1, "WINO_SPLIT": 0}]


def _wino_within(h, w, c, y, xx):
    """the 4 x 4 output tiles whose 6 x 6 input tile holds (y, xx): tiles start at multiples of 4, input rows 4t-1 .. 4t+4"""
    within = torch.zeros(h, w, c, dtype=torch.bool)
    for ty in range(0, h, 4):
        for tx in range(0, w, 4):
            if ty - 1 <= y <= ty + 4 and tx - 1 <= xx <= tx + 4:
                within[ty:ty + 4, tx:tx + 4] = True
    return within


@pytest.mark.parametrize("kind", list(BAD))
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("shape", [(33, 56, 56, 64, 64, True), (60, 28, 28, 128, 128, False)], ids=["809tiles_res", "184x2tiles"])
@pytest.mark.parametrize("variant", WINO_VARIANTS, ids=_vid)
def test_wino43_variants(dev, variant, shape, relu, kind):
    """wave4 / wave8 / persistent / split-K tail (the tail tiles are the last ones: image n - 2 sits in them)"""
    from relpose_gnn_amd import ops
    n, h, w, cin, cout, res = shape
    x = _rand(n, h, w, cin, seed=51)
    wt = _rand(cout, 3, 3, cin, seed=52, scale=(2.0 / (9 * cin)) ** 0.5)
    sc, sh = torch.rand(cout, generator=torch.Generator().manual_seed(53)) + 0.5, _rand(cout, seed=54, scale=0.1)
    r = _rand(n, h, w, cout, seed=55) if res else None
    u = ops.wino43_transform_weights(wt.to(dev))
    args = (u, sc.to(dev), sh.to(dev), None if r is None else r.to(dev))
    with ops.tuned(variant):
        clean = ops.conv3x3_wino43_bn_act_nhwc(x.to(dev), *args, relu=relu)
        for img in (1, n - 2):
            for (y, xx) in ((0, 0), (h // 2 + 1, w // 2 - 3), (h - 1, w - 1)):
                xb = x.clone()
                _put(xb, (img, y, xx, 3), kind)
                got = ops.conv3x3_wino43_bn_act_nhwc(xb.to(dev), *args, relu=relu)
                ref = _conv_ref1(("wino", shape, relu, kind, img, y, xx), xb[img], wt, sc, sh, 1, 1, relu, None if r is None else r[img])
                g, rr = _check(got, clean, ref, img, exact=False, within=_wino_within(h, w, cout, y, xx), whole=False)
                assert not bool((torch.isnan(rr) & torch.isinf(g)).any()), "a NaN came out as inf"


CONV_BF16_CASES = (
    [({"BF16_FAST": f}, s) for f in (1, 0) for s in ("l3", "ds")]
    + [({"BF16_DMA": 10 + c}, s) for c in range(10) for s in ("l3", "ds")]
    + [({"BF16_PATCH": m}, s) for m in (2, 3, 12) for s in ("l3", "l1")]
    + [({"BF16_PATCH": 2, "BF16_PERSIST": 1}, "l1p")]
    + [({"BF16_LEAN_EPI": e}, s) for e in (1, 0) for s in ("ds", "l2")])
CONV_BF16_SHAPES = {  # n, h, w, cin, cout, k, stride, pad, residual, relu
    "l3": (9, 14, 14, 256, 256, 3, 1, 1, False, True),     # layer-3 shape: tiles span 2 images
    "ds": (4, 14, 14, 64, 128, 1, 2, 0, False, False),     # the 1x1/2 downsample, no ReLU
    "l1": (40, 56, 56, 64, 64, 3, 1, 1, True, True),       # layer-1 shape, residual
    "l1p": (70, 56, 56, 64, 64, 3, 1, 1, True, True),      # 429 tiles on 256 CUs: the persistent form is dispatched
    "l2": (24, 28, 28, 128, 128, 3, 1, 1, True, True),
}


@pytest.mark.parametrize("kind", list(BAD))
@pytest.mark.parametrize("variant,shape", CONV_BF16_CASES, ids=lambda v: v if isinstance(v, str) else _vid(v))
def test_conv_bf16_variants(dev, variant, shape, kind):
    from relpose_gnn_amd import ops
    n, h, w, cin, cout, k, st, pad, res, relu = CONV_BF16_SHAPES[shape]
    x = _rand(n, h, w, cin, seed=61).bfloat16()
    wt = _rand(cout, k, k, cin, seed=62, scale=(2.0 / (cin * k * k)) ** 0.5).bfloat16()
    sc, sh = torch.rand(cout, generator=torch.Generator().manual_seed(63)) + 0.5, _rand(cout, seed=64, scale=0.1)
    ho, wo = (h + 2 * pad - k) // st + 1, (w + 2 * pad - k) // st + 1
    r = _rand(n, ho, wo, cout, seed=65).bfloat16() if res else None
    img = n // 2
    args = (wt.to(dev), sc.to(dev), sh.to(dev), None if r is None else r.to(dev))
    with ops.tuned(variant):
        clean = ops.conv2d_bn_act_nhwc_bf16(x.to(dev), *args, stride=st, pad=pad, relu=relu)
        for (y, xx) in _positions(h, w):
            xb = x.clone()
            _put(xb, (img, y, xx, 5), kind)
            got = ops.conv2d_bn_act_nhwc_bf16(xb.to(dev), *args, stride=st, pad=pad, relu=relu)
            ref = _conv_ref1(("bf16", shape, kind, y, xx), xb[img].float(), wt.float(), sc, sh, st, pad, relu,
                             None if r is None else r[img].float(), bf16_out=True)
            if not bool((~torch.isfinite(ref)).any()):
                continue
            _check(got.float(), clean.float(), ref, img, whole=False)


@pytest.mark.parametrize("kind", list(BAD))
@pytest.mark.parametrize("shape", [(9, 64, 86), (96, 56, 56), (3, 56, 56)], ids=["two_strip", "many_tiles", "small"])
@pytest.mark.parametrize("fuse", [3, 1, 5], ids=["persistent", "tile_per_wg", "two_group"])
def test_basicblock64_bf16(dev, fuse, shape, kind):
    """the fused BasicBlock64 (RPG_TUNE_BF16_FUSE_BLOCK): two-strip form at 64 x 86 (the 256 x 341 layer-1 map), persistent form on
    more tiles than CUs; bad value at a corner, next to the strips' cut, and the last pixel of an image in the middle"""
    from relpose_gnn_amd import ops
    n, h, w = shape
    g = torch.Generator().manual_seed(71 + w)
    x = torch.randn((n, h, w, 64), generator=g).bfloat16()
    w1 = (torch.randn((64, 3, 3, 64), generator=g) * (2.0 / 576) ** 0.5).bfloat16()
    w2 = (torch.randn((64, 3, 3, 64), generator=g) * (2.0 / 576) ** 0.5).bfloat16()
    s1, b1 = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.2
    s2, b2 = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.2
    wd = [t.to(dev) for t in (w1, s1, b1, w2, s2, b2)]
    img = n // 2
    with ops.tuned({"BF16_FUSE_BLOCK": fuse}):
        clean = ops.basicblock64_bf16(x.to(dev), *wd)
        for (y, xx) in ((0, 0), (h // 2, (w + 1) // 2), (h - 1, w - 1)):
            xb = x.clone()
            _put(xb, (img, y, xx, 9), kind)
            got = ops.basicblock64_bf16(xb.to(dev), *wd)
            key = ("block", shape, kind, y, xx)
            if key not in _REF_CACHE:
                t = _conv_ref1(key + ("t",), xb[img].float(), w1.float(), s1, b1, 1, 1, True, bf16_out=True)   # stored in bf16
                _conv_ref1(key, t, w2.float(), s2, b2, 1, 1, True, xb[img].float(), bf16_out=True)
            _check(got.float(), clean.float(), _REF_CACHE[key], img, whole=False)


@pytest.mark.parametrize("kind", list(BAD))
@pytest.mark.parametrize("m,k,n_out,cfg", [(333, 192, 100, 0), (1792, 2048, 768, 0), (1801, 2048, 2056, 10), (1801, 2048, 2056, 11),
                                           (1801, 2048, 2056, 13), (1801, 2048, 2056, 17), (1801, 2048, 2056, 18)])
@pytest.mark.parametrize("relu", [True, False])
def test_linear_bf16(dev, m, k, n_out, cfg, relu, kind):
    """rpg_linear_bf16: general (K % 64 != 0) and interleaved kernels, and the LDS-DMA configurations (RPG_TUNE_BF16_LINEAR_DMA)"""
    from relpose_gnn_amd import ops
    a = _rand(m, k, seed=81).bfloat16()
    w, b = _rand(n_out, k, seed=82, scale=k ** -0.5).bfloat16(), _rand(n_out, seed=83)
    res = _rand(m, n_out, seed=84)
    with ops.tuned({"BF16_LINEAR_DMA": cfg}):
        run = lambda t: ops.linear_bf16(t.to(dev), w.to(dev), b.to(dev), res.to(dev), relu=relu)
        clean = run(a)
        for row in (0, m // 2, m - 1):
            ab = a.clone()
            _put(ab, (row, 17), kind)
            ref = ab[row].double() @ w.double().T + b.double() + res[row].double()
            _check(run(ab), clean, F.relu(ref) if relu else ref, row, whole=False)


# ---------------------------------------------------------------------------------------------------------------- pools and GNN
@pytest.mark.parametrize("kind", list(BAD))
def test_global_avgpool(dev, kind):
    from relpose_gnn_amd import ops
    x = _rand(5, 7, 9, 64, seed=91)
    clean = ops.global_avgpool_nhwc(x.to(dev))
    xb = x.clone()
    _put(xb, (2, 3, 4, 10), kind)
    _check(ops.global_avgpool_nhwc(xb.to(dev)), clean, xb.double().mean(dim=(1, 2)), 2)


@pytest.mark.parametrize("kind", list(BAD))
@pytest.mark.parametrize("part", ["g", "theta", "phi"])
def test_attention_rows(dev, part, kind):
    from relpose_gnn_amd import ops
    r, c = 130, 64
    gtp = _rand(r, 3 * c, seed=92, scale=1.5)
    clean = ops.attention_rows(gtp.to(dev))
    gb = gtp.clone()
    _put(gb, (57, {"g": 0, "theta": 1, "phi": 2}[part] * c + 11), kind)
    d = gb[57:58].double()
    g, th, ph = d[:, :c], d[:, c:2 * c], d[:, 2 * c:]
    ref = torch.bmm(torch.softmax(ph.unsqueeze(2) * th.unsqueeze(1), dim=-1), g.unsqueeze(2)).squeeze(2)[0]
    _check(ops.attention_rows(gb.to(dev)), clean, ref, 57, whole=False)


def _ragged_graph(sizes, trailing=2):
    from oracle.posenet_ref import fc_edge_index
    eis, off = [], 0
    for n_nodes in sizes:
        if n_nodes > 1:
            eis.append(fc_edge_index(n_nodes) + off)
        off += n_nodes
    return torch.cat(eis, 1), off + trailing                    # trailing nodes (and 1-node graphs) have no incoming edge


@pytest.mark.parametrize("kind", list(BAD))
@pytest.mark.parametrize("where", ["g", "theta", "phi", "msg"])
def test_attention_aggregate_and_scatter_mean(dev, where, kind):
    """attention rows + mean aggregation (one kernel) and scatter_mean on ragged graphs with an isolated node: the bad value in one
    edge's g / theta / phi / message reaches that edge's target node only; isolated nodes stay 0"""
    from relpose_gnn_amd import ops
    from oracle.posenet_ref import scatter_mean
    ei, n = _ragged_graph((8, 4, 1, 6))
    e, c, d = ei.shape[1], 8, 64
    gtp, msg = _rand(e, 3 * c, seed=93, scale=1.5), _rand(e, d, seed=94)
    gp = ops.graph_prepare(ei.to(dev), n)
    y0, m0 = ops.attention_aggregate(gtp.to(dev), msg.to(dev), gp["rowptr"], gp["perm"], n)
    s0 = ops.scatter_mean(msg.to(dev), gp["rowptr"], gp["perm"], n)
    edge = 61                                                      # an edge of the 4-node graph
    tgt = int(ei[1, edge])
    gb, mb = gtp.clone(), msg.clone()
    if where == "msg":
        _put(mb, (edge, 5), kind)
    else:
        _put(gb, (edge, {"g": 0, "theta": 1, "phi": 2}[where] * c + 3), kind)
    y, mm = ops.attention_aggregate(gb.to(dev), mb.to(dev), gp["rowptr"], gp["perm"], n)
    s = ops.scatter_mean(mb.to(dev), gp["rowptr"], gp["perm"], n)
    dd = gb.double()
    att = torch.bmm(torch.softmax(dd[:, 2 * c:].unsqueeze(2) * dd[:, c:2 * c].unsqueeze(1), dim=-1), dd[:, :c].unsqueeze(2)).squeeze(2)
    yref, mref = scatter_mean(att, ei[1], n), scatter_mean(mb.double(), ei[1], n)
    if where == "msg":
        _check(mm, m0, mref, tgt)
        _check(s, s0, mref, tgt)
        assert torch.equal(y.cpu(), y0.cpu())
    else:
        _check(y, y0, yref, tgt)
        assert torch.equal(mm.cpu(), m0.cpu())
    assert float(y[-2:].abs().max()) == 0.0 and float(mm[-2:].abs().max()) == 0.0


@pytest.mark.parametrize("kind", list(BAD))
def test_pose_heads_and_edge_concat(dev, kind):
    from relpose_gnn_amd import ops
    from oracle.posenet_ref import edge_concat
    x, w6, b6 = _rand(61, 2048, seed=95), _rand(6, 2048, seed=96, scale=0.02), _rand(6, seed=97)
    clean = ops.pose_heads(x.to(dev), w6.to(dev), b6.to(dev))
    xb = x.clone()
    _put(xb, (30, 100), kind)
    _check(ops.pose_heads(xb.to(dev), w6.to(dev), b6.to(dev)), clean, xb.double() @ w6.double().T + b6.double(), 30)
    # the edge concat is a gather: bit-exact, the bad value in the rows of the edges that touch node 11 and nowhere else
    from relpose_gnn_amd.graph import fc_edge_index
    ei = torch.cat([fc_edge_index(8) + 8 * g for g in range(3)], 1)
    f = _rand(24, 64, seed=98)
    _put(f, (11, 7), kind)
    got, ref = ops.edge_concat_gather(f.to(dev), ei.to(dev)).cpu(), edge_concat(f, ei)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.equal(torch.nan_to_num(got), torch.nan_to_num(ref))
    assert bool((~torch.isfinite(got)).any())


@pytest.mark.parametrize("kind", ["nan", "-nan", "inf"])
def test_knn_graph_with_bad_features(dev, kind):
    """knn_graph with a non-finite feature in one graph: the other graphs' edges are the oracle's, and every index of the bad
    graph stays inside that graph (its own edge list is not asserted: the oracle's order for NaN distances is unspecified)"""
    from relpose_gnn_amd import ops
    from oracle.posenet_ref import knn_graph
    sizes, k, d = (8, 9, 8, 3), 4, 64
    b = torch.cat([torch.full((s,), i, dtype=torch.int64) for i, s in enumerate(sizes)])
    x = _rand(sum(sizes), d, seed=99)
    _put(x, (12, 5), kind)                                           # node 4 of graph 1
    got = ops.knn_graph(x.to(dev), k, b.to(dev)).cpu()
    ref = knn_graph(x, k, b)
    assert bool((b[got[0]] == b[got[1]]).all())
    keep_g, keep_r = b[got[1]] != 1, b[ref[1]] != 1
    assert torch.equal(got[:, keep_g], ref[:, keep_r])


# ------------------------------------------------------------------------------------------------ model level at the bench shapes
_BIG = {}


def _big_model(dev, h):
    if h not in _BIG:
        import relpose_gnn_amd.synth as S
        from relpose_gnn_amd.posenet import PoseNetX_R2
        from relpose_gnn_amd.resnet import resnet34
        D = 2048
        m = PoseNetX_R2(resnet34(), droprate=0.0, pretrained=False, feat_dim=D, edge_feat_dim=D, node_dim=D,
                        input_img_height=h, use_gnn=True, knn=-1, use_AP=True, gnn_recursion=2)
        m.load_state_dict(S.synth_state_dict(S.posenet_r2_param_shapes(D, D, D), seed=1))
        _BIG.clear()
        _BIG[h] = m.to(dev).eval()
    return _BIG[h]


@pytest.mark.parametrize("cfg", ["f32_224_32graphs", "bf16enc_256x341_64graphs", "bf16all_256x341_64graphs"])
def test_model_bench_shapes_bad_pixel(dev, cfg):
    """BASELINE configs[1] (32 graphs x 8 nodes, 224 x 224, fp32) and the bf16 encoder with the f32 / bf16 GNN at the 256 x 341
    evaluation shape with 64 graphs (layer 1 runs the persistent two-strip fused BasicBlock, layers 2-4 the paired downsample)"""
    from relpose_gnn_amd.graph import fc_batch
    h, w, graphs = (224, 224, 32) if cfg.startswith("f32") else (256, 341, 64)
    m = _big_model(dev, h)
    m.encoder_dtype, m.gnn_dtype = {"f32": ("f32", "f32"), "bf16enc": ("bf16", "f32"), "bf16all": ("bf16", "bf16")}[cfg.split("_")[0]]
    try:
        x = torch.randn(graphs * 8, 3 * h * w, generator=torch.Generator().manual_seed(7))
        a0, r0, ei = [t.clone() for t in m(fc_batch(x, 8).to(dev))]
        for kind in BAD:
            for img, pos in ((9, "mid"), (16, "first"), (graphs * 8 - 9, "last")):
                a, r, _ = m(fc_batch(_poison(x, img, h, w, pos, kind), 8).to(dev))
                _graph_check(a, r, a0, r0, ei, img // 8)
    finally:
        m.encoder_dtype, m.gnn_dtype = "f32", "f32"


@pytest.mark.parametrize("kind", list(BAD))
@pytest.mark.parametrize("variant", [{"FUSED_STEM": 0}, {"GNN_SPLIT": 0}, {"GNN_FUSE_AGG": 0}], ids=_vid)
def test_model_variants_bad_pixel(dev, variant, kind):
    """the three-kernel bf16 stem (its bf16 max-pool kernel), and the GNN without the node split (gather_add2_relu is the split
    form's edge ReLU) / without the fused attention aggregation"""
    import relpose_gnn_amd.synth as S
    from relpose_gnn_amd.graph import fc_batch
    m = _model(dev)
    if "FUSED_STEM" in variant:
        m.encoder_dtype = "bf16"
    x = S.synth_images(4 * 8, 32, 40, seed=24)
    with ops.tuned(variant):
        a0, r0, ei = [t.clone() for t in m(fc_batch(x, 8).to(dev))]
        a, r, _ = m(fc_batch(_poison(x, 13, 32, 40, "mid", kind), 8).to(dev))
    _graph_check(a, r, a0, r0, ei, 1)
