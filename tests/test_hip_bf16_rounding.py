"""Every bf16 kernel variant held to CORRECT ROUNDING against a float64 reference (tests/bf16_rounding.py).

The kernels accumulate exact bf16 x bf16 products in fp32, apply the BatchNorm affine, the residual and the ReLU in fp32 and round
ONCE to bf16 (nearest even) at the store.  So every output element must lie in [bf16(act(z - c u S)), bf16(act(z + c u S))], z the
float64 result, S the conditioning sum, u = 2^-24, c = 4 c_ref with c_ref measured per case on the CPU fp32 evaluation of the same
op -- no tolerance is chosen here.  Every case also asserts that at most 2 % of its elements have two acceptable answers.  This is
what proves the claim of test_hip_bf16.py that "the difference is the final bf16 rounding"; its 1e-2 max-norm bar passes a store
that truncates, a BatchNorm scale rounded to bf16 and a double rounding around the residual (test_bf16_rounding_cpu.py).

Operands: the distributions of the older tests ("unit": scale in [0.5, 1.5)), and per-channel scales spread over 2^-6 .. 2^6 with
about 20 % negative and shifts scaled with them ("wide": channels four orders of magnitude apart in one tensor).  Residuals are
bf16 where the entry point takes bf16 and fp32 where it takes fp32.

rpg_basicblock64_bf16 needs no interval test of its own: test_fused_basicblock64_equals_two_convolutions holds it BIT-IDENTICAL to
two convolution launches of the patch kernel, and those launches are held to correct rounding here
(test_basicblock_reference_pair: first convolution against the exact answer, second against the exact answer on the KERNEL'S OWN
bf16 intermediate, so a legitimate rounding flip of the intermediate does not leak into the second interval).

Measured on an MI355X (profiles/bf16_rounding_observed.json; c_observed = max |y - z| / (u S) of the fp32-output kernels, to be
read against the allowed c = 4 c_ref):
  fc as a 1 x 1 convolution (37 x 512 -> 2048, and the encoder's own fc at 8 images), out_f32, interleaved / general kernel, default
  dispatch and all ten LDS-DMA configurations:  c_ref 0.92-1.24, c_observed 1.35-1.65: at most 0.42 of the allowance.  Every
  kernel gives the SAME figure per case: each walks K in ascending order per output element, 16 at a time.
  linear_bf16, K = 72 .. 4096, default kernels and LDS-DMA configurations 0, 1, 3, 7, 8:  c_ref 0.78-1.96, c_observed 0.76-2.06: at
  most 0.64 of the allowance (K = 4096; the MFMA chain over all of K against the CPU's blocked sums).
The factor 4 holds everywhere with room; no case needed another.  Largest share of elements with two acceptable answers: 0.9 % in
the op-level cases, 1.1 % in the per-layer checks of the encoder test (cap 2 %).
Wall time on an MI355X host, same run of the whole suite: 31.6 s for this file (316 cases, float64 references cached per shape) next
to 28.4 s for tests/test_hip_bf16.py.
"""
import pytest
import torch
import torch.nn.functional as F

import bf16_rounding as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.set_num_threads(min(16, torch.get_num_threads()))           # the float64 references run on the CPU
    return torch.device("cuda:0")


def _record(case: str, rep: dict) -> None:
    """Observed figures (c_ref, c_observed, ambiguous share, distances) go into the parity report that the neighbouring tests
    append to (test_hip_eval_geometry._report: a scratch file, summarised by hand into profiles/)."""
    from test_hip_eval_geometry import _report
    _report({"case": case, **{k: v for k, v in rep.items() if k != "first"}})


# n, h, w, cin, cout, k, stride, pad
SHAPES = {
    "tiny_cin8": (2, 9, 11, 8, 16, 3, 1, 1),            # ragged M, K = 72 (K tail), general kernel only
    "stem7x7": (1, 16, 16, 8, 64, 7, 2, 3),             # the stem's convolution on the 8-channel image
    "ragged_s2": (3, 13, 17, 192, 72, 3, 2, 1),         # ragged M (189) and N (72), 3 K steps per tap (odd), padding taps, stride 2
    "ragged_s1": (5, 23, 19, 64, 72, 3, 1, 1),          # ragged M (2185) and N, odd number of K steps per workgroup, stride 1
    "ragged_192": (3, 13, 17, 192, 72, 3, 1, 1),        # the patch kernel's odd case: 6 chunks, ragged N (on the 256 x 128 tile, mode 3, only)
    "cin96": (5, 9, 11, 96, 40, 3, 1, 1),               # only the 32-wide K step configurations apply
    "ds1x1": (2, 14, 14, 64, 128, 1, 2, 0),             # downsample 1x1 / stride 2: a single K step
    "layer1": (40, 56, 56, 64, 64, 3, 1, 1),            # model shapes (224 x 224 input)
    "layer2": (24, 28, 28, 128, 128, 3, 1, 1),
    "layer2_64": (64, 28, 28, 128, 128, 3, 1, 1),       # 392 tiles of 128 x 128
    "layer3": (9, 14, 14, 256, 256, 3, 1, 1),           # ragged M (1764), 36 K steps of 64
    "layer4": (8, 7, 7, 512, 512, 3, 1, 1),
    "tiny_img": (2, 5, 3, 128, 128, 3, 1, 1),           # a FALL-BACK case: 244 patch pieces on the 512 x 128 tile, 125 on 256 x 128 (64 fit) -- no
                                                        # patch tile takes it, 30 rows are too few for the LDS-DMA kernel: the interleaved kernel runs
    "fc": (37, 1, 1, 512, 2048, 1, 1, 0),               # the fc as a 1x1 convolution on a 1x1 image (fp32 output in the model)
    "persist_ragged": (100, 40, 40, 64, 64, 3, 1, 1),   # 313 tiles of 512 rows (more than one round: the persistent form), ragged
    "tail_l3_res": (400, 14, 14, 256, 256, 3, 1, 1),    # the shapes of test_patch_kernel_tail_retiling_is_bit_identical
    "tail_l2": (400, 28, 28, 128, 128, 3, 1, 1),
    "tail_l3": (340, 14, 14, 256, 256, 3, 1, 1),
}
_cache = {}


def _conv_case(name, dist, res):
    """Operands (CPU, NCHW / OIHW) and the float64 reference of a convolution case, cached across kernel variants."""
    key = (name, dist, bool(res))
    if key not in _cache:
        n, h, w, cin, cout, k, stride, pad = SHAPES[name]
        g = torch.Generator().manual_seed(sum(map(ord, name)))
        x = torch.randn((n, cin, h, w), generator=g).bfloat16()
        wt = (torch.randn((cout, cin, k, k), generator=g) * (2.0 / (cin * k * k)) ** 0.5).bfloat16()
        scale, shift = (R.wide_scales if dist == "wide" else R.unit_scales)(cout, 3 + cout)
        ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        r = torch.randn((n, cout, ho, wo), generator=g).bfloat16() if res else None
        ref = R.conv_ref(x, wt, scale, shift, r, stride, pad)
        if len(_cache) >= 6:                                  # a handful of references alive at a time (the largest hold 0.5 GB)
            _cache.pop(next(iter(_cache)))
        _cache[key] = (x, wt, scale, shift, r, ref, {"c_ref": ref.c_ref})
    return _cache[key]


def _nhwc(t, dev):
    return None if t is None else t.permute(0, 2, 3, 1).contiguous().to(dev)


def _conv_check(dev, name, dist, res, relu, tuning, out_f32=False, what="", family=None):
    """family: the kernel family the case is meant to run ("patch", "dma", ...).  The observed route (rpg_conv_bf16_last_route) must
    then be that family AND equal the dispatcher's rule restated in bf16_sweep_ref.py for this device."""
    import bf16_sweep_ref as B
    from relpose_gnn_amd import ops
    x, wt, scale, shift, r, ref, memo = _conv_case(name, dist, res)
    stride, pad = SHAPES[name][6], SHAPES[name][7]
    with ops.tuned(tuning):
        y = ops.conv2d_bn_act_nhwc_bf16(_nhwc(x, dev), _nhwc(wt, dev), scale.to(dev), shift.to(dev), _nhwc(r, dev), stride=stride,
                                        pad=pad, relu=relu, out_f32=out_f32)
        route = ops.conv_bf16_last_route()
        torch.cuda.synchronize()
    if family is not None:
        got = (route["family"], route["bm"], route["bn"], route["detail"], route["launches"])
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        want = B.bf16_route({ops.TUNING_KEYS[k]: v for k, v in tuning.items()}, *SHAPES[name], res, out_f32, cus)
        assert got == want and got[0] == family, (name, what, "observed", got, "restated", want, "meant", family)
    tag = f"conv {name} {dist} res={int(bool(res))} relu={int(relu)} {what}"
    if out_f32:
        assert y.dtype == torch.float32
        rep = R.check_f32(y, ref, relu, what=tag)
        print(tag, {k: rep[k] for k in ("c_ref", "c_observed")})
        _record(tag, rep)
        y = y.bfloat16()                                      # and the same values through the interval (their rounding is exact)
    assert y.dtype == torch.bfloat16
    rep = R.check(y, ref, relu, c_ref=memo["c_ref"], what=tag)
    print(tag, {k: rep[k] for k in ("c_ref", "ambiguous")})
    assert rep["bad"] == 0 and rep["ambiguous"] <= R.AMBIGUOUS_CAP
    return y


# (shape, dist, residual, relu, out_f32): every variant below sees at least one ragged shape and one model shape
_BOTH_KERNELS = [("tiny_cin8", "unit", False, True, False), ("tiny_cin8", "wide", False, True, False),
                 ("stem7x7", "wide", False, True, False), ("ragged_s2", "unit", True, True, False),
                 ("ragged_s2", "wide", True, True, False), ("ragged_s1", "wide", True, False, False),
                 ("ds1x1", "unit", False, False, False), ("ds1x1", "wide", False, False, False),
                 ("layer1", "wide", True, True, False), ("layer2_64", "wide", True, True, False),
                 ("fc", "unit", False, False, True), ("fc", "wide", False, False, True)]


@pytest.mark.parametrize("fast", [1, 0], ids=["interleaved", "general"])
@pytest.mark.parametrize("name,dist,res,relu,f32out", _BOTH_KERNELS, ids=lambda v: str(v))
def test_conv_interleaved_and_general_kernel(dev, name, dist, res, relu, f32out, fast):
    """RPG_TUNE_BF16_FAST 1 / 0 with the LDS-DMA and patch kernels off, so that the buffer-load kernels themselves run: 1x1, 3x3,
    7x7, stride 1 and 2, with / without residual and ReLU, bf16 and fp32 output.
    Observed on an MI355X for the fp32 output (fc, 37 x 512 -> 2048): c_observed 1.65 (unit) / 1.62 (wide) against c_ref 1.18 / 1.24,
    the same from both kernels: 0.35 / 0.33 of the 4 c_ref allowed."""
    from relpose_gnn_amd import ops
    _conv_check(dev, name, dist, res, relu, {ops.TUNE_BF16_FAST: fast, ops.TUNE_BF16_DMA: 0, ops.TUNE_BF16_PATCH: 0}, f32out, f"fast={fast}")


@pytest.mark.parametrize("name,dist,res,relu,f32out", _BOTH_KERNELS, ids=lambda v: str(v))
def test_conv_default_dispatch(dev, name, dist, res, relu, f32out):
    """The same cases through the dispatcher as the model uses it (LDS-DMA kernel by shape, patch kernel by shape)."""
    _conv_check(dev, name, dist, res, relu, {}, f32out, "default")


@pytest.mark.parametrize("tile", [0, 1, 2, 3], ids=["64x64", "128x128", "256x64", "128x64"])
@pytest.mark.parametrize("name,dist", [("ragged_s1", "unit"), ("ragged_s1", "wide"), ("layer2", "wide")])
def test_conv_interleaved_tiles(dev, name, dist, tile):
    """RPG_TUNE_BF16_TILE 0-3: every tile of the interleaved kernel (the LDS-DMA and patch kernels off, or they would take the shape)."""
    from relpose_gnn_amd import ops
    _conv_check(dev, name, dist, True, True, {ops.TUNE_BF16_TILE: tile, ops.TUNE_BF16_DMA: 0, ops.TUNE_BF16_PATCH: 0}, what=f"tile={tile}")


@pytest.mark.parametrize("bk", [32, 64])
@pytest.mark.parametrize("name,dist", [("ragged_s2", "unit"), ("ragged_s2", "wide"), ("layer2_64", "wide"), ("cin96", "wide")])
def test_conv_general_kernel_k_step(dev, name, dist, bk):
    """RPG_TUNE_BF16_BK at both values the library accepts, on the general kernel (the K step is its template parameter; 64 is
    dispatched from K = 128 up on the 128 x 128 tile: layer2_64 has 392 of them), and Cin = 96 where only the general kernel applies."""
    from relpose_gnn_amd import _lib, ops
    _conv_check(dev, name, dist, True, True, {ops.TUNE_BF16_BK: bk, ops.TUNE_BF16_FAST: 0, ops.TUNE_BF16_DMA: 0, ops.TUNE_BF16_PATCH: 0},
                what=f"bk={bk}")
    assert _lib.lib().rpg_set_tuning(ops.TUNE_BF16_BK, 48) == _lib.RPG_ERR_BAD_ARG          # 32 and 64 are all it accepts


@pytest.mark.parametrize("cfg", range(10))
@pytest.mark.parametrize("name,dist,res,relu,f32out", [
    ("ragged_s2", "wide", True, True, False), ("cin96", "wide", True, False, False), ("ds1x1", "wide", False, False, False),
    ("layer2", "wide", True, True, False), ("layer3", "unit", False, True, False), ("fc", "wide", False, False, True)],
    ids=lambda v: str(v))
def test_conv_dma_configs(dev, cfg, name, dist, res, relu, f32out):
    """RPG_TUNE_BF16_DMA = 10 + cfg: every configuration of the LDS-DMA kernel (tile, wave grid, K step, LDS images); where one is
    not eligible (Cin % K step) the launcher falls back and the check still holds.
    Observed on an MI355X for the fp32 output (fc, wide): c_observed 1.62 against c_ref 1.24 on every configuration.
    The route is observed: the configuration where Cin is a multiple of its K step, else the fall-back the rule names."""
    import bf16_sweep_ref as B
    from relpose_gnn_amd import ops
    bk = B.DMA_CONFIGS[cfg][2]
    fallback = "interleaved" if SHAPES[name][3] % 64 == 0 else "general"          # (Cin = 96: configurations 6, 7 and 9 only)
    _conv_check(dev, name, dist, res, relu, {ops.TUNE_BF16_DMA: 10 + cfg}, f32out, f"dma={cfg}",
                family="dma" if SHAPES[name][3] % bk == 0 else fallback)


@pytest.mark.parametrize("mode", [2, 3, 12], ids=["by_width", "tile256x128", "by_width_3stages"])
@pytest.mark.parametrize("name,dist,res,relu", [
    ("ragged_192", "unit", True, False), ("ragged_192", "wide", True, False), ("tiny_img", "wide", True, True),
    ("layer1", "wide", True, True), ("layer2", "wide", False, True), ("layer3", "wide", True, True), ("layer4", "wide", True, True)],
    ids=lambda v: str(v))
def test_conv_patch_kernel(dev, mode, name, dist, res, relu):
    """RPG_TUNE_BF16_PATCH 2 / 3 / 12: the patch kernel wherever eligible, by output width, on the 256 x 128 tile, and without
    the four-weight-stage form.  The route is observed: the patch kernel, but for two fall-backs to the interleaved kernel that ran
    unnoticed before the route was read -- tiny_img under every mode, and ragged_192 under the by-width modes (Cout = 72 asks for
    the 512 x 128 tile, whose patch on 13 x 17 maps is 40 rows of 32 slots = 80 pieces; the 256 x 128 tile of mode 3 takes it, 46
    pieces).  tests/test_hip_bf16_sweep.py runs the patch tiles on their smallest maps."""
    from relpose_gnn_amd import ops
    fallback = name == "tiny_img" or (name == "ragged_192" and mode != 3)
    _conv_check(dev, name, dist, res, relu, {ops.TUNE_BF16_PATCH: mode}, what=f"patch={mode}",
                family="interleaved" if fallback else "patch")


@pytest.mark.parametrize("name,dist,res,relu", [("persist_ragged", "wide", True, True), ("persist_ragged", "unit", False, True),
                                                ("layer1", "wide", True, False)], ids=lambda v: str(v))
def test_conv_patch_kernel_persistent(dev, name, dist, res, relu):
    """RPG_TUNE_BF16_PERSIST = 1 with the patch kernel: 313 ragged tiles on 256 CUs (the persistent form walks them), and the
    layer-1 shape whose 245 tiles fit one round (not eligible: one workgroup per tile)."""
    from relpose_gnn_amd import ops
    _conv_check(dev, name, dist, res, relu, {ops.TUNE_BF16_PATCH: 2, ops.TUNE_BF16_PERSIST: 1}, what="persistent",
                family="patch_persistent" if name == "persist_ragged" else "patch")


@pytest.mark.parametrize("lean", [1, 0], ids=["lean", "general_epilogue"])
@pytest.mark.parametrize("res", [True, False], ids=["res", "nores"])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("name,dist,tuning", [("ragged_s2", "wide", "default"), ("ragged_s2", "unit", "default"),
                                              ("layer2", "wide", "default"), ("layer3", "wide", "patch")])
def test_conv_epilogues(dev, name, dist, tuning, relu, res, lean):
    """RPG_TUNE_BF16_LEAN_EPI 1 / 0 with and without residual and ReLU, under the buffer-load kernel (ragged), the LDS-DMA kernel
    (layer 2 by shape) and the patch kernel."""
    from relpose_gnn_amd import ops
    keys = {ops.TUNE_BF16_LEAN_EPI: lean}
    if tuning == "patch":
        keys[ops.TUNE_BF16_PATCH] = 2
    _conv_check(dev, name, dist, res, relu, keys, what=f"lean={lean} {tuning}")


@pytest.mark.parametrize("name,res", [("tail_l3_res", True), ("tail_l2", False), ("tail_l3", False)])
def test_conv_patch_kernel_tail_retiling(dev, name, res):
    """RPG_TUNE_BF16_TAIL = 3 (both re-tilings: the rows beyond the last full round of tiles go to a second launch with smaller
    tiles) at the shapes of test_patch_kernel_tail_retiling_is_bit_identical -- every image, main and tail launch."""
    from relpose_gnn_amd import ops
    _conv_check(dev, name, "wide", res, True, {ops.TUNE_BF16_TAIL: 3}, what="tail=3", family="patch")
    assert ops.conv_bf16_last_route()["launches"] == 2


@pytest.mark.parametrize("n,h,w,cin,cout", [(48, 56, 56, 64, 128), (48, 28, 28, 128, 256), (64, 34, 50, 64, 128)],
                         ids=["layer2_224px_48img", "layer3_224px_48img", "layer2_136x200_64img"])
@pytest.mark.parametrize("dist", ["unit", "wide"])
def test_conv_paired_downsample_launch(dev, n, h, w, cin, cout, dist):
    """RPG_TUNE_BF16_PAIR: the 3x3 / stride-2 convolution (+ ReLU) and the 1x1 / stride-2 shortcut (no ReLU) of a down-sampling
    block as ONE launch (rpg_conv_pair_bf16), at the layer shapes of test_bf16_encoder_paired_downsample_launch_is_bit_identical
    (224 x 224 with 48 images: layers 2 and 3 pair; 136 x 200 with 64 images: odd 17 x 25 output maps)."""
    from relpose_gnn_amd import ops
    g = torch.Generator().manual_seed(n + h + cout)
    x = torch.randn((n, cin, h, w), generator=g).bfloat16()
    wa = (torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (9 * cin)) ** 0.5).bfloat16()
    wb = (torch.randn((cout, cin, 1, 1), generator=g) * (2.0 / cin) ** 0.5).bfloat16()
    mk = R.wide_scales if dist == "wide" else R.unit_scales
    (sa, ha), (sb, hb) = mk(cout, 11), mk(cout, 12)
    ya, yb = ops.conv_pair_bf16(_nhwc(x, dev), _nhwc(wa, dev), sa.to(dev), ha.to(dev), _nhwc(wb, dev), sb.to(dev), hb.to(dev), stride=2, pad=1)
    torch.cuda.synchronize()
    ra = R.check(ya, R.conv_ref(x, wa, sa, ha, None, 2, 1), True, what="pair: 3x3 / 2")
    rb = R.check(yb, R.conv_ref(x, wb, sb, hb, None, 2, 0), False, what="pair: 1x1 / 2 shortcut")
    assert ra["bad"] == 0 and rb["bad"] == 0 and max(ra["ambiguous"], rb["ambiguous"]) <= R.AMBIGUOUS_CAP
    with ops.tuned({ops.TUNE_BF16_PAIR: 0}):                # switched off, the entry point refuses (the caller launches one by one)
        with pytest.raises(ValueError):
            ops.conv_pair_bf16(_nhwc(x, dev), _nhwc(wa, dev), sa.to(dev), ha.to(dev), _nhwc(wb, dev), sb.to(dev), hb.to(dev))


# ---------------------------------------------------------------------------------------------------------------- Linear
_lin_cache = {}


def _linear_case(m, k, n_out, gather, dist):
    key = (m, k, n_out, gather, dist)
    if key not in _lin_cache:
        g = torch.Generator().manual_seed(m + k + n_out)
        a = torch.randn((m, k), generator=g).bfloat16()
        w = torch.randn((n_out, k), generator=g) * k ** -0.5
        bias = torch.randn(n_out, generator=g)
        if dist == "wide":                                    # output columns spread over 2^-6 .. 2^6, about 20 % negated
            col, _ = R.wide_scales(n_out, 21)
            w, bias = w * col.view(-1, 1), bias * col.abs()
        w = w.bfloat16()
        table = idx = idx2 = None
        parts = []
        if gather == 0:
            table = torch.randn((m, n_out), generator=g)      # plain fp32 residual rows
            parts = [table]
        else:
            table = torch.randn((50, 3 * n_out), generator=g)  # rows of [r1 | r2 | unused], pitch 3 n_out
            idx = torch.randint(0, 50, (m,), generator=g)
            parts = [table[idx, :n_out]]
            if gather == 2:
                idx2 = torch.randint(0, 50, (m,), generator=g)
                parts.append(table[idx2, n_out:2 * n_out])
        if len(_lin_cache) >= 3:
            _lin_cache.pop(next(iter(_lin_cache)))
        _lin_cache[key] = (a, w, bias, table, idx, idx2, R.linear_ref(a, w, bias, parts))
    return _lin_cache[key]


def _linear_run(ops, dev, case, gather, n_out, **kw):
    a, w, bias, table, idx, idx2, _ = case
    t = table.to(dev)
    r2 = t[:, n_out:] if gather == 2 else None                # same storage, column offset (a view: common row pitch)
    return ops.linear_bf16_ex(a.to(dev), w.to(dev), bias.to(dev), t, None if idx is None else idx.to(dev), r2,
                              None if idx2 is None else idx2.to(dev), **kw)


_LINEAR_SMALL = [(333, 192, 100, 2), (130, 256, 2048, 1), (64, 72, 40, 0), (1792, 2048, 768, 0)]
_LINEAR_DMA = [(1801, 2048, 2056, 1), (3584, 2048, 2048, 2), (1792, 4096, 2048, 0)]


# default kernels: every shape, both distributions; LDS-DMA configurations (incl. 10 and 11): the shapes with >= 192 tiles of 128 x 128
# (below that the launcher does not take them and the default kernel, checked above, runs)
_LINEAR_CASES = [(s, None, d) for s in _LINEAR_SMALL + _LINEAR_DMA for d in ("unit", "wide")]
_LINEAR_CASES += [(s, c, "wide") for s in _LINEAR_DMA for c in (0, 1, 3, 7, 8)]
_LINEAR_CASES.sort(key=lambda v: (v[0], v[2]))                # one float64 reference per (shape, distribution), cached


@pytest.mark.parametrize("shape,cfg,dist", _LINEAR_CASES,
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else ("default" if v is None else f"dma{10 + v}" if isinstance(v, int) else v))
def test_linear_bf16_outputs(dev, shape, cfg, dist):
    """rpg_linear_bf16 / rpg_linear_bf16_ex, default kernels (interleaved for K % 64 == 0, general else) and
    RPG_TUNE_BF16_LINEAR_DMA = 10 + cfg (taken from 192 tiles of 128 x 128 up; below, the default kernel runs and the check still
    holds): bias, plain / gathered / twice gathered fp32 residual rows, ReLU.  (i) the fp32 output within c u S of the exact value
    (observed c recorded); (ii) the same GEMM with a bf16 primary output: correctly rounded; (iii) the second output out2 =
    bf16(relu2 ? max(y, 0) : y) next to an fp32 ReLU primary, relu2 on and off: correctly rounded, and the primary is unchanged
    by it bit for bit.
    Observed on an MI355X (c_ref -> c_observed, unit | wide; the LDS-DMA configurations give the default kernel's figure to the
    last digit): 64x72->40 1.14 -> 0.76 | 1.17 -> 1.08;  333x192->100 1.35 -> 1.45 | 1.96 -> 1.30;  130x256->2048 1.19 -> 1.52 |
    1.17 -> 1.35;  1792x2048->768 0.80 -> 1.81 | 0.82 -> 1.82;  1801x2048->2056 0.86 -> 1.95 | 0.82 -> 2.05;  3584x2048->2048
    0.89 -> 1.94 | 1.62 -> 1.99;  1792x4096->2048 0.82 -> 1.89 | 0.78 -> 1.99: at most 0.64 of the 4 c_ref allowed."""
    from relpose_gnn_amd import ops
    m, k, n_out, gather = shape
    case = _linear_case(m, k, n_out, gather, dist)
    ref = case[-1]
    tag = f"linear {m}x{k}->{n_out} gather={gather} {dist} cfg={cfg}"
    with ops.tuned({ops.TUNE_BF16_LINEAR_DMA: 0 if cfg is None else 10 + cfg}):
        y32, none2 = _linear_run(ops, dev, case, gather, n_out, relu=True)
        plain = ops.linear_bf16(case[0].to(dev), case[1].to(dev), case[2].to(dev), relu=False) if gather == 0 else None
        y16, _ = _linear_run(ops, dev, case, gather, n_out, relu=False, out_dtype=torch.bfloat16)
        outs2 = {r2: _linear_run(ops, dev, case, gather, n_out, relu=True, out2=True, relu2=bool(r2)) for r2 in (0, 1)}
        only2 = _linear_run(ops, dev, case, gather, n_out, relu=True, out_dtype=None, out2=True, relu2=True)
        torch.cuda.synchronize()
    assert none2 is None and y32.dtype == torch.float32 and y16.dtype == torch.bfloat16
    rep = R.check_f32(y32, ref, True, what=tag)
    print(tag, {kk: rep[kk] for kk in ("c_ref", "c_observed")})
    _record(tag, rep)
    if plain is not None:                                     # the entry point without residual: bias only
        R.check_f32(plain, R.linear_ref(case[0], case[1], case[2]), False, what=tag + " (no residual)")
    r16 = R.check(y16, ref, False, c_ref=rep["c_ref"], what=tag + " bf16 primary")
    assert r16["bad"] == 0 and r16["ambiguous"] <= R.AMBIGUOUS_CAP
    for r2, (p, o2) in outs2.items():
        assert o2.dtype == torch.bfloat16 and torch.equal(p, y32)
        rr = R.check(o2, ref, bool(r2), c_ref=rep["c_ref"], what=tag + f" out2 relu2={r2}")
        assert rr["bad"] == 0 and rr["ambiguous"] <= R.AMBIGUOUS_CAP
    assert only2[0] is None and torch.equal(only2[1], outs2[1][1])


# ------------------------------------------------------------------------------------------------------------------ stem
_stem_cache = {}


def _stem_case(n, h, w, dist):
    key = (n, h, w, dist)
    if key not in _stem_cache:
        g = torch.Generator().manual_seed(1000 * h + w)
        x = torch.randn((n, 3, h, w), generator=g)
        wt = torch.randn((64, 3, 7, 7), generator=g) * (2.0 / 147) ** 0.5
        if dist == "wide":
            scale, shift = R.wide_scales(64, 31, shift_scale=0.3)
        else:                                                 # the distribution of test_fused_stem_bf16: some negative gammas
            scale = (torch.rand(64, generator=g) + 0.5) * torch.where(torch.rand(64, generator=g) < 0.15, -1.0, 1.0)
            shift = torch.randn(64, generator=g) * 0.3
        # the kernel rounds the fp32 image to bf16 itself; the reference starts from the rounded image (that rounding is a
        # specified step of the op, not an error of it), so S has no term for it
        ref = R.conv_ref(x.bfloat16(), wt.bfloat16(), scale, shift, None, 2, 3, nhwc=False)
        if len(_stem_cache) >= 4:
            _stem_cache.pop(next(iter(_stem_cache)))
        _stem_cache[key] = (x, wt, scale, shift, ref, ref.c_ref)
    return _stem_cache[key]


def _pool_nhwc(t):
    return F.max_pool2d(t, 3, 2, 1).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("xdtype", [torch.float32, torch.bfloat16], ids=["x_f32", "x_bf16"])
@pytest.mark.parametrize("kernel", [1, 33, 1 + (7 << 8), 33 + (14 << 8), 3],
                         ids=["strip", "strip_half_per_wave", "strip_bands7", "strip_half_bands14", "tile"])
@pytest.mark.parametrize("dist", ["unit", "wide"])
@pytest.mark.parametrize("n,h,w", [(2, 224, 224), (1, 256, 341), (3, 37, 53), (2, 9, 5), (9, 64, 72)])
def test_stem_bf16(dev, n, h, w, dist, kernel, xdtype):
    """rpg_stem_conv7x7s2_bn_relu_maxpool_bf16 (fp32 and bf16 images), RPG_TUNE_FUSED_STEM 1 / 33 / banded forms / 3.  Max-pool
    commutes with the monotone rounding: the exact answer is bf16(maxpool(relu(z))) and the interval is the max-pool of lo / hi."""
    from relpose_gnn_amd import ops
    from relpose_gnn_amd.params import pack_stem_bf16
    x, wt, scale, shift, ref, c_ref = _stem_case(n, h, w, dist)
    with ops.tuned({ops.TUNE_FUSED_STEM: kernel}):
        y = ops.stem_conv_bn_relu_maxpool_bf16(x.to(xdtype).to(dev), pack_stem_bf16(wt).to(dev), scale.to(dev), shift.to(dev))
        torch.cuda.synchronize()
    rep = R.check(y, ref, True, post=_pool_nhwc, c_ref=c_ref, what=f"stem {n}x{h}x{w} {dist} kernel={kernel} {xdtype}")
    assert rep["bad"] == 0 and rep["ambiguous"] <= R.AMBIGUOUS_CAP


# ------------------------------------------------------------------------------------------- fused BasicBlock: the missing link
@pytest.mark.parametrize("shape,cols", [((3, 56, 56), None), ((2, 64, 86), (0, 45)), ((2, 64, 86), (41, 86))],
                         ids=["3x56x56", "2x64x86_left_strip_view", "2x64x86_right_strip_view"])
def test_basicblock_reference_pair(dev, shape, cols):
    """The patch-kernel pair that test_fused_basicblock64_equals_two_convolutions uses as `want` (RPG_TUNE_BF16_PATCH = 2), on the
    whole 56 x 56 map and on the two strip VIEWS (ceil(86 / 2) + 2 = 45 columns each) of the 64 x 86 map: the first convolution
    against the exact answer; the second against the exact answer computed from the KERNEL'S OWN bf16 intermediate."""
    from relpose_gnn_amd import ops
    n, h, w = shape
    g = torch.Generator().manual_seed(1000 + n * h + w)
    x = torch.randn((n, h, w, 64), generator=g).bfloat16()
    if cols is not None:
        x = x[:, :, cols[0]:cols[1], :].contiguous()
    w1 = (torch.randn((64, 3, 3, 64), generator=g) * (2.0 / 576) ** 0.5).bfloat16()
    w2 = (torch.randn((64, 3, 3, 64), generator=g) * (2.0 / 576) ** 0.5).bfloat16()
    (s1, b1), (s2, b2) = R.wide_scales(64, 41, 0.2), R.unit_scales(64, 42, 0.2)
    xd = x.to(dev)
    with ops.tuned({ops.TUNE_BF16_PATCH: 2}):
        t = ops.conv2d_bn_act_nhwc_bf16(xd, w1.to(dev), s1.to(dev), b1.to(dev), None, stride=1, pad=1, relu=True)
        y = ops.conv2d_bn_act_nhwc_bf16(t, w2.to(dev), s2.to(dev), b2.to(dev), xd, stride=1, pad=1, relu=True)
        torch.cuda.synchronize()
    nchw = lambda v: v.cpu().permute(0, 3, 1, 2)
    r1 = R.check(t, R.conv_ref(nchw(x), nchw(w1), s1, b1, None, 1, 1), True, what="block conv1")
    r2 = R.check(y, R.conv_ref(nchw(t), nchw(w2), s2, b2, nchw(x), 1, 1), True, what="block conv2 on the kernel's intermediate")
    assert r1["bad"] == 0 and r2["bad"] == 0 and max(r1["ambiguous"], r2["ambiguous"]) <= R.AMBIGUOUS_CAP
    if w <= 62 and cols is None:                              # and the fused kernel equals the pair (the link itself, restated)
        assert torch.equal(ops.basicblock64_bf16(xd, w1.to(dev), s1.to(dev), b1.to(dev), w2.to(dev), s2.to(dev), b2.to(dev)), y)


# ----------------------------------------------------------------------------------------------------------- f32_to_bf16
def _f32_from_bits(bits):
    b = torch.tensor(bits, dtype=torch.int64)
    return torch.where(b >= 2 ** 31, b - 2 ** 32, b).to(torch.int32).view(torch.float32)


def test_f32_to_bf16_special_values_strided(dev):
    """rpg_f32_to_bf16 with ld_src != cols and col_off > 0, bit-exact against Tensor.bfloat16(): ties (exactly half-way, both
    parities, both signs, at 1.0, in the bf16-subnormal range and below the smallest bf16), fp32 and bf16 subnormals, +-0, the
    largest finite fp32 (rounds to inf), +-inf, the largest bf16; around them random values of every exponent."""
    from relpose_gnn_amd import _lib as L
    special = _f32_from_bits([
        0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,       # 1 + 2^-8 (tie, even below -> down), 1 + 3 * 2^-8 (tie, odd below -> up), negated
        0x3F808001, 0x3F807FFF, 0x3F818001, 0x3F817FFF,       # just beside the ties
        0x00008000, 0x00018000, 0x80008000, 0x80018000,       # ties between bf16 subnormals
        0x00000001, 0x00007FFF, 0x00008001, 0x007FFFFF,       # fp32 subnormals: below half of the smallest bf16, just above it, the largest
        0x00010000, 0x00800000, 0x007F8000,                   # smallest bf16 subnormal, smallest normal, a tie onto the smallest normal
        0x00000000, 0x80000000,                               # +-0
        0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F0000, 0x7F7F8000,       # largest finite (-> inf), its negative, largest bf16 (stays), the tie above it (-> inf)
        0x7F800000, 0xFF800000,                               # +-inf
    ])
    rows, cols, ld_src, col_off, ld_dst = 37, 64, 72, 24, 96
    g = torch.Generator().manual_seed(9)
    src = torch.randn((rows, ld_src), generator=g) * torch.exp2(torch.randint(-140, 127, (rows, ld_src), generator=g).float())
    flat = src.view(-1)
    at = torch.randperm(rows * ld_src, generator=g)[:special.numel() * 8]
    flat[at] = special.repeat(8)                              # sprinkled over rows and columns (some land in the unread pad columns)
    for r in range(rows):
        src[r, (r * 5) % cols] = special[r % special.numel()]  # ... and every one of them inside the converted columns
    want = src[:, :cols].bfloat16()
    assert int((want.float().abs() == float("inf")).sum()) >= 4 and int((want.float() == 0).sum()) >= 4
    dst = torch.full((rows, ld_dst), 7.0, dtype=torch.bfloat16, device=dev)
    sd = src.to(dev)
    L.check(L.lib().rpg_f32_to_bf16(sd.data_ptr(), ld_src, dst.data_ptr(), ld_dst, col_off, rows, cols,
                                    torch.cuda.current_stream().cuda_stream), "f32_to_bf16")
    got = dst.cpu()
    assert torch.equal(got[:, col_off:col_off + cols].view(torch.int16), want.view(torch.int16))
    assert bool((got[:, :col_off].float() == 7.0).all()) and bool((got[:, col_off + cols:].float() == 7.0).all())   # nothing else written


# --------------------------------------------------------------------------------------------------------- encoder level
@pytest.mark.parametrize("h,w,nimg", [(224, 224, 8), (256, 341, 8)], ids=["224x224", "256x341"])
def test_bf16_encoder_vs_bf16_emulating_oracle(dev, h, w, nimg):
    """test_bf16_encoder_forward_vs_fp32_oracle measures bf16 itself (5e-2 against the fp32 oracle).  Here the reference has the
    kernels' own rounding points (bf16_rounding.emulate_encoder_bf16: image, stem after the pool, every conv + BN (+ identity)
    (+ ReLU) output, the pooled features; the fc output stays fp32), evaluated in float64 (E64) and in float32 (E32), R3 dims,
    synthetic weights, 8 images:
        d_ref = rel_l2(E32 features, E64 features)            measured, reference against reference
        rel_l2(HIP bf16 features, E64 features) <= 3 d_ref    (3: margin for the kernels' different summation order)
    Rounding flips amplify through 36 layers, so no per-element interval holds at this level; per LAYER it does: every convolution of
    the encoder (the stem through the fused stem kernel, the fc with its fp32 output) runs through its op-level entry point on
    E64's bf16 input to that layer and passes the interval check.  (The global average pool, the max-pool and the re-layout are
    covered by the feature distance here; tests/test_hip_bf16_sweep.py holds each bit-exact through its own entry point.)
    Measured on an MI355X (profiles/bf16_rounding_observed.json), 8 images: 224 x 224: d_ref 2.32e-3, HIP 2.20e-3; 256 x 341:
    d_ref 2.01e-3, HIP 2.01e-3 -- the kernels are as far from E64 as the float32 evaluation of the same rounding points is, a
    third of the 3 d_ref allowed; all 36 convolutions pass per layer, the fc's observed c is 1.35 / 1.54 (c_ref 1.14 / 0.92)."""
    import relpose_gnn_amd.synth as S
    from relpose_gnn_amd import ops
    from relpose_gnn_amd.params import pack_resnet_bf16
    from relpose_gnn_amd.posenet import PoseNetX_R2
    from relpose_gnn_amd.resnet import resnet34
    D = 2048
    m = PoseNetX_R2(resnet34(), droprate=0.0, pretrained=False, feat_dim=D, edge_feat_dim=D, node_dim=D,
                    input_img_height=h, use_gnn=True, knn=-1, use_AP=True, gnn_recursion=2)
    m.load_state_dict(S.synth_state_dict(S.posenet_r2_param_shapes(D, D, D), seed=1))
    m = m.to(dev).eval()
    m.encoder_dtype = "bf16"
    x = S.synth_images(nimg, h, w, seed=6).view(nimg, 3, h, w)
    feat = m._enc.run(m.feature_extractor.state_dict, "", x.to(dev)).float().cpu()
    tensors, blocks, planes = pack_resnet_bf16({k: v.detach().cpu() for k, v in m.feature_extractor.state_dict().items()}, "")
    trace = []
    e64 = R.emulate_encoder_bf16(tensors, blocks, planes, x, torch.float64, trace)
    e32 = R.emulate_encoder_bf16(tensors, blocks, planes, x, torch.float32)
    d_ref, d_hip = R.rel_l2(e32, e64), R.rel_l2(feat, e64)
    rep = {"d_ref_E32_vs_E64": d_ref, "d_hip_vs_E64": d_hip, "images": nimg}
    print(f"encoder {h}x{w}", rep)
    _record(f"bf16_encoder_R3_{h}x{w}_{nimg}img_vs_bf16_emulating_oracle", rep)
    # per layer, on E64's input to the layer
    worst = 0.0
    for d in trace[:-1]:
        if d["name"] == "stem":
            ref = R.conv_ref(d["x"], d["w"], d["scale"], d["shift"], None, 2, 3, nhwc=False)
            y = ops.stem_conv_bn_relu_maxpool_bf16(d["x"][:, :3].contiguous().to(dev), tensors[-1].to(dev), d["scale"].to(dev), d["shift"].to(dev))
            r = R.check(y, ref, True, post=_pool_nhwc, what=f"encoder {h}x{w} stem")
        else:
            ref = R.conv_ref(d["x"], d["w"], d["scale"], d["shift"], d["residual"], d["stride"], d["pad"])
            y = ops.conv2d_bn_act_nhwc_bf16(_nhwc(d["x"].bfloat16(), dev), _nhwc(d["w"].bfloat16(), dev), d["scale"].to(dev), d["shift"].to(dev),
                                            None if d["residual"] is None else _nhwc(d["residual"].bfloat16(), dev),
                                            stride=d["stride"], pad=d["pad"], relu=d["relu"])
            r = R.check(y, ref, d["relu"], what=f"encoder {h}x{w} {d['name']}")
        assert r["bad"] == 0 and r["ambiguous"] <= R.AMBIGUOUS_CAP, (d["name"], r)
        worst = max(worst, r["ambiguous"])
    fc = trace[-1]                                            # the fc on E64's pooled bf16 features: fp32 output
    yfc = ops.conv2d_bn_act_nhwc_bf16(fc["x"].bfloat16().view(nimg, 1, 1, -1).to(dev), fc["w"].bfloat16().view(D, 1, 1, -1).to(dev), None,
                                      fc["bias"].to(dev), None, stride=1, pad=0, relu=False, out_f32=True)
    rfc = R.check_f32(yfc.view(nimg, D), R.linear_ref(fc["x"], fc["w"], fc["bias"]), False, what="encoder fc")
    _record(f"bf16_encoder_R3_{h}x{w}_fc_f32", rfc)
    print(f"encoder {h}x{w}: {len(trace) - 1} convolutions pass, worst ambiguous share {worst:.4f}, fc c_observed {rfc['c_observed']:.3f}")
    assert d_hip <= 3.0 * d_ref, (d_hip, d_ref)

