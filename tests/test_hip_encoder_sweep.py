"""The fp32 encoder kernels -- the Winograd F(4,3) convolutions of csrc/winograd.hip on every launch route, the tile-engine
convolutions the encoder runs outside Winograd, the fp32 stem, the re-layout, the pools and the composite rpg_resnet_forward_f32
-- held to float64 per element, inside a memory harness (tests/encoder_sweep_ref.py; its own tests are test_encoder_sweep_cpu.py).

What the suite did not run before: the persistent Winograd kernel below H = 24 (H = 2 and 3, W < 4, a Cout tail, a last
workgroup of fewer than 128 tiles, its H = 1 fallback), a split tail of more parts than the in-kernel combine takes, post-ReLU
inputs with an outlier channel, the grid-stride loops of the re-layout and the pools, and a composite forward whose late layers
shrink to 2 x 2 and 1 x 1 and whose layers disagree about Winograd.

Every kernel is called through the C ABI with pointers into harness buffers: each operand lies in the middle of one allocation
of this test, between two moats of max(64 KiB, 4 image rows); the input moats hold NaN, the output and its moats one NaN bit
pattern nobody computes.  After the launch the moats are bit-identical, no element of the output still holds the pattern, and
the output is finite -- a load outside the image that reached an accumulator would be a NaN, a stray store a changed moat.

The bar.  c(y) = max |y - z| / (u S) before the activation (z exact in float64, S the same pass on absolute values, u = 2^-24);
behind a ReLU the same c as an interval, act(z - c u S) <= y <= act(z + c u S).  Asserted: c_hip <= M_KERNEL c_ref, where c_ref is
c of the CPU fp32 statement of the same algorithm over >= 2^16 outputs (never of a kernel).  Every case runs with its ReLU and
once without, so the magnitude check cannot go hollow.  Unmoved beside it: rel_err < 2e-5 (Winograd) / 1e-5 (direct, stem)
against the fp32 CPU result.  Composite: rel_err against the float64 network <= M_FWD x the larger rel_err of the fp32 CPU
network with torch's convolutions and with the Winograd statement, and rel_err < 1e-4 against the fp32 network.

Margins.  M_KERNEL starts at 4 (bf16_rounding.FACTOR, for the same reason: 32x32x2 MFMA blocks and a K loop cut into parts
against a correctly ordered fp32 evaluation of the same algorithm), M_FWD at 2 (the graph sweep's).  Every case prints c_ref,
c_hip and their ratio and appends them to the file RPG_SWEEP_RECORD names; profiles/encoder_sweep_observed.json holds one such
run on an MI355X at the starting margins.  Worst kernel ratio there: 1.839 (Winograd, whole tiles, n64 h2 w2 Cin 48 -- a case
whose c_ref is only 2.4); direct convolutions and average pool <= 1.0, stem <= 0.93.  So M_KERNEL came down to twice that,
3.68.  Worst composite ratio: 1.057 (one image of 40 x 56; the others 0.73-0.82); twice that is above the starting value, so
M_FWD stays at 2.  Neither rises again without the arithmetic that justifies it written here, and never above 8 / 4: a ratio
above the margin is a finding to fix in the kernel or to explain.

What pins what (reasoned from the case lists of encoder_sweep_ref.py, not tried: no broken kernel is run on a GPU).
`wo + 2 < W` turned into `wo + 2 <= W` in an epilogue: at W = 3 and 7 a pixel column that does not exist is stored -- pixel 0 of the
next row, which another lane also writes, and behind the last row of the last image the moat: W = 3 and 7 are in every route's
list (n63h1w3, n32h2w3, n33h1w7, n13h5w7, ...).  `h >= 2` dropped from the persistent condition: the H = 1 shapes of the two
persistent lists would then run persistently, with kernel row 1 never loaded -- wrong by O(1) in every element.  A tile position
swapped, a kernel-row term dropped at the top row, low mantissa bits lost, a stray store, an unwritten element, a padding tap that
reads outside: each is planted in the CPU statement or the harness by test_encoder_sweep_cpu.py and caught there by this check;
on the GPU the shapes with H <= 3 and W < 4 put every output element on an edge.  A combine limit read wrongly by the launcher
changes which kernel adds the ten parts of the Cin = 160 shapes, not the sum: the routes asked for it both ways are checked for
their result, the launcher's choice itself is restated (wino_taken), not observed.

What the "act" cases can and cannot see.  A Winograd tile's rounding error is that of its LARGEST pixels, while S is the
element's own 3 x 3 window; with a 1e3 outlier channel next to clamped zeros c_ref is in the hundreds to thousands (the
algorithm's figure, shared by the fp32 CPU statement and the kernels) and its maximum is heavy-tailed, so there the bar
catches wrong offsets, dropped terms and outside loads, and the N(0, 1) cases (c_ref 2-16) are the ones that weigh mantissa bits.
"""
import pytest
import torch
import torch.nn.functional as F

import encoder_sweep_ref as R
from conftest import rel_err
from relpose_gnn_amd import ops
from test_hip_graph_sweep import _record

pytestmark = pytest.mark.gpu

M_KERNEL = 3.68               # 2 x 1.839, the worst ratio of profiles/encoder_sweep_observed.json (started at R.M_START = 4; ceiling 8)
M_FWD = R.M_FWD_START         # 2: twice the worst recorded ratio (1.057) would be above the starting value (ceiling 4)
assert M_KERNEL <= R.M_START and M_FWD <= R.M_FWD_START


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from relpose_gnn_amd import _lib
    return _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ratio(section, case, c_ref, c_hip, margin):
    assert c_ref > 0.0, "the fp32 CPU reference is exact here: the case measures nothing"
    _record(section, case, {"c_ref": c_ref, "c_hip": c_hip, "ratio": c_hip / c_ref})
    assert c_hip <= margin * c_ref, (case, c_ref, c_hip, c_hip / c_ref)


def _opt(buf):
    return None if buf is None else buf.ptr()


class _ConvBuffers:
    """The operands of one convolution case in harness buffers (``weights``: what the kernel reads as its weight operand)."""

    def __init__(self, case, weights, dev):
        self.case = case
        self.x, self.w = R.Moated(case.x.shape, dev, case.x), R.Moated(weights.shape, dev, weights)
        self.scale, self.shift = R.Moated(case.scale.shape, dev, case.scale), R.Moated(case.shift.shape, dev, case.shift)
        self.res = None if case.residual is None else R.Moated(case.residual.shape, dev, case.residual)
        n, cout = case.x.shape[0], case.w.shape[0]
        self.out_shape = (n, *case.out_hw(), cout)
        self.inputs = [b for b in (self.x, self.w, self.scale, self.shift, self.res) if b is not None]

    def run(self, launch, dev):
        """launch(y) -> status; returns the output on the CPU after the harness has looked at the launch."""
        y = R.Moated(self.out_shape, dev)
        rc = launch(y)
        torch.cuda.synchronize()
        assert rc == 0, rc
        assert R.harness_findings(self.inputs, y) == []
        return y.t.cpu()


# ----------------------------------------------------------------------------------------------------------------------
# Winograd: every route on every edge
# ----------------------------------------------------------------------------------------------------------------------
_WINO = {}


def _wino_ref(shape):
    if shape not in _WINO:
        n, h, w, cin, cout, res, dist = shape
        case = R.conv_case(n, h, w, cin, cout, 3, 1, 1, res, dist, seed=R.WINO_SHAPES.index(shape))
        ref = R.conv_ref(case, "wino")
        _WINO[shape] = (case, ref, R.conv_direct(case, torch.float32))
    return _WINO[shape]


def _wino_id(route, shape):
    """<route asked>-<shape>-to-<route it is meant to take> (the latter as on the 256 CUs of an MI355X; the test works it out for
    the device it runs on)."""
    return f"{route}-{R.wino_shape_id(shape)}-to-{R.wino_expected(route, shape, 256).replace(':', '_x')}"


_WINO_PARAMS = [pytest.param(route, shape, id=_wino_id(route, shape)) for route in R.ROUTES for shape in R.wino_cases(route)]


@pytest.mark.parametrize("route,shape", _WINO_PARAMS)
def test_winograd_route(dev, lib, route, shape):
    """One (route, shape) of encoder_sweep_ref.WINO_SHAPES: the launcher's rule, restated, must send the shape where the case
    list means it to go on THIS device (a failure, not a skip, if it cannot); then the harness, the element-wise bar with and
    without ReLU, the old max-norm bar, and for whole-tile persistent launches the one-workgroup-per-tile result to 1e-6."""
    from relpose_gnn_amd import ops
    n, h, w, cin, cout, _, _ = shape
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    taken = R.wino_taken(R.ROUTES[route], n, h, w, cin, cout, cus)
    assert taken == R.wino_expected(route, shape, cus), (route, shape, cus, taken)
    case, ref, y32 = _wino_ref(shape)
    u = ops.wino43_transform_weights(case.w.to(dev))
    buf = _ConvBuffers(case, u.cpu(), dev)

    def launch(relu):
        return lambda y: lib.rpg_conv3x3_wino43_bn_act_nhwc_f32(buf.x.ptr(), buf.w.ptr(), buf.scale.ptr(), buf.shift.ptr(), _opt(buf.res),
                                                               y.ptr(), n, h, w, cin, cout, relu, _stream())
    with ops.tuned(R.ROUTES[route]):
        y_relu, y_lin = buf.run(launch(1), dev), buf.run(launch(0), dev)
    assert rel_err(y_relu, torch.relu(y32)) < 2e-5 and rel_err(y_lin, y32) < 2e-5
    c_relu, c_lin = R.c_of(y_relu, ref.z, ref.S, relu=True), R.c_of(y_lin, ref.z, ref.S)
    assert c_relu <= M_KERNEL * ref.c_ref, (taken, ref.c_ref, c_relu)
    _ratio("winograd", f"{route}-{R.wino_shape_id(shape)}->{taken}", ref.c_ref, c_lin, M_KERNEL)
    if taken == "persist_whole":
        with ops.tuned(R.ROUTES["wave8_whole"]):
            y_whole = buf.run(launch(0), dev)
        assert rel_err(y_lin, y_whole) < 1e-6


# ----------------------------------------------------------------------------------------------------------------------
# the direct convolutions of the encoder
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("streamk", [1, 0], ids=["default", "streamk0"])
@pytest.mark.parametrize("extent", R.DIRECT_EXTENTS, ids=lambda e: f"{e[0]}x{e[1]}")
@pytest.mark.parametrize("kind", list(R.DIRECT_KINDS))
def test_direct_convolution(dev, lib, kind, extent, streamk):
    """3x3 / 2, 1x1 / 2 (no activation) and 7x7 / 2 with Cin = 4 on inputs of 1, 2, 7, 13 and 14 pixels (an all-padding window, odd
    extents that halve unevenly), at the default tuning -- RPG_TUNE_STREAMK = 1, the key test_tile_engine_variants walks: the
    3x3 cases (K = 576) are then cut by stream-K, the other two have fewer K steps than the engine splits -- and with it off."""
    k, stride, pad, cin, cout, relu = R.DIRECT_KINDS[kind]
    case = R.direct_case(kind, extent)
    ref, y32 = R.conv_ref(case, "direct"), R.conv_direct(case, torch.float32)
    buf = _ConvBuffers(case, case.w, dev)
    n, h, w = case.x.shape[:3]

    def launch(act):
        return lambda y: lib.rpg_conv2d_bn_act_nhwc_f32(buf.x.ptr(), buf.w.ptr(), buf.scale.ptr(), buf.shift.ptr(), None, y.ptr(), n, h, w,
                                                       cin, cout, k, k, stride, pad, act, _stream())
    with ops.tuned({"STREAMK": streamk}):
        y_lin = buf.run(launch(0), dev)
        y_relu = buf.run(launch(1), dev) if relu else None
    assert rel_err(y_lin, y32) < 1e-5
    if relu:
        assert rel_err(y_relu, torch.relu(y32)) < 1e-5
        assert R.c_of(y_relu, ref.z, ref.S, relu=True) <= M_KERNEL * ref.c_ref
    _ratio("direct", f"{kind}-{extent[0]}x{extent[1]}-streamk{streamk}", ref.c_ref, R.c_of(y_lin, ref.z, ref.S), M_KERNEL)


# ----------------------------------------------------------------------------------------------------------------------
# fp32 stem
# ----------------------------------------------------------------------------------------------------------------------
_STEM = {}


def _stem_ref(h, w):
    """(operands, z, S, c_ref): c_ref of torch's fp32 convolution + affine over the case and, where it is small, over extra images."""
    if (h, w) not in _STEM:
        x, wt, scale, shift = R.stem_operands(h, w)
        z, S = R.stem_exact(x, wt, scale, shift)
        c_ref, per = R.c_of(R.stem_fp32(x, wt, scale, shift), z, S), z.numel() // z.shape[0]
        if z.numel() < R.MIN_REF_ELEMS:
            xe = torch.randn(-(-(R.MIN_REF_ELEMS - z.numel()) // per), 3, h, w, generator=torch.Generator().manual_seed(50 + h))
            c_ref = max(c_ref, R.c_of(R.stem_fp32(xe, wt, scale, shift), *R.stem_exact(xe, wt, scale, shift)))
        _STEM[(h, w)] = ((x, wt, scale, shift), z, S, c_ref)
    return _STEM[(h, w)]


@pytest.mark.parametrize("kernel", [1, 1 + 128], ids=["tile", "strip"])
@pytest.mark.parametrize("h,w", R.STEM_SIZES)
def test_stem(dev, lib, h, w, kernel):
    """rpg_stem_conv7x7s2_bn_relu_maxpool_f32, tile and strip-march kernel, on 1 x 1 .. 61 x 63 images (all-border tiles, a ragged
    last strip and band): the harness, and the float64 bound carried through ReLU and max-pool."""
    from relpose_gnn_amd.params import pack_stem_pairs
    (x, wt, scale, shift), z, S, c_ref = _stem_ref(h, w)
    n = x.shape[0]
    xb, wp, sh = R.Moated(x.shape, dev, x), pack_stem_pairs(wt, scale), R.Moated(shift.shape, dev, shift)
    wpb = R.Moated(wp.shape, dev, wp)
    hp, wpool = ((h - 1) // 2 + 1 - 1) // 2 + 1, ((w - 1) // 2 + 1 - 1) // 2 + 1
    y = R.Moated((n, hp, wpool, 64), dev)
    with ops.tuned({"FUSED_STEM": kernel}):
        rc = lib.rpg_stem_conv7x7s2_bn_relu_maxpool_f32(xb.ptr(), wpb.ptr(), sh.ptr(), y.ptr(), n, h, w, _stream())
        torch.cuda.synchronize()
    assert rc == 0
    assert R.harness_findings([xb, wpb, sh], y) == []
    got = y.t.cpu()
    assert rel_err(got, R.stem_post(R.stem_fp32(x, wt, scale, shift))) < 1e-5
    _ratio("stem", f"{'strip' if kernel & 128 else 'tile'}-{h}x{w}", c_ref, R.c_post(got, z, S, R.stem_post), M_KERNEL)


# ----------------------------------------------------------------------------------------------------------------------
# re-layout and pools
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w", [(3, 900, 800), (2, 1, 1), (1, 3, 5)])
def test_relayout(dev, lib, n, h, w):
    """nchw3_to_nhwc4, bit-exact; 3 x 900 x 800 pixels is more than 8192 x 256: the grid-stride loop with a ragged last stride."""
    x = torch.randn(n, 3, h, w, generator=torch.Generator().manual_seed(h))
    xb, y = R.Moated(x.shape, dev, x), R.Moated((n, h, w, 4), dev)
    assert lib.rpg_nchw3_to_nhwc4_f32(xb.ptr(), y.ptr(), n, h, w, _stream()) == 0
    torch.cuda.synchronize()
    assert R.harness_findings([xb], y) == []
    assert torch.equal(y.t.cpu(), F.pad(x.permute(0, 2, 3, 1), (0, 1)))


@pytest.mark.parametrize("n,h,w,c", [(5, 129, 131, 512), (2, 1, 1, 8), (2, 1, 2, 8), (2, 2, 1, 8), (3, 2, 2, 4), (2, 1, 5, 8), (2, 5, 1, 4)])
def test_maxpool(dev, lib, n, h, w, c):
    """maxpool3x3s2, bit-exact; 5 x 65 x 66 x 128 output quads are more than 8192 x 256; H or W of 1 and 2."""
    x = torch.randn(n, h, w, c, generator=torch.Generator().manual_seed(h + w))
    ref = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous()
    xb, y = R.Moated(x.shape, dev, x), R.Moated(ref.shape, dev)
    assert lib.rpg_maxpool3x3s2_nhwc_f32(xb.ptr(), y.ptr(), n, h, w, c, _stream()) == 0
    torch.cuda.synchronize()
    assert R.harness_findings([xb], y) == []
    assert torch.equal(y.t.cpu(), ref)


@pytest.mark.parametrize("n,hw,c", [(16385, 3, 512), (3, 1, 8), (5, 49, 16)])
def test_global_avgpool(dev, lib, n, hw, c):
    """global_avgpool: n c / 4 = 2,097,280 lanes of work are just above 8192 x 256; hw = 1 and 49.  The kernel states its order
    (ascending sum, one division), so the fp32 statement in that order is exact -- and it is held to the float64 bound."""
    x = R.activations((n, hw, c), "act", seed=hw)
    z, S = R.avgpool_exact(x)
    ordered = R.avgpool_ordered(x)
    xb, y = R.Moated(x.shape, dev, x), R.Moated((n, c), dev)
    assert lib.rpg_global_avgpool_nhwc_f32(xb.ptr(), y.ptr(), n, hw, c, _stream()) == 0
    torch.cuda.synchronize()
    assert R.harness_findings([xb], y) == []
    got = y.t.cpu()
    assert torch.equal(got, ordered)
    c_ref, c_hip = R.c_of(ordered, z, S), R.c_of(got, z, S)
    if hw == 1:
        assert c_ref == 0.0 and c_hip == 0.0                              # the mean of one value is that value
    else:
        _ratio("avgpool", f"n{n}hw{hw}c{c}", c_ref, c_hip, M_KERNEL)


# ----------------------------------------------------------------------------------------------------------------------
# the composite encoder
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def encoder(dev):
    from relpose_gnn_amd import _lib, ops
    from relpose_gnn_amd.params import pack_resnet
    module = R.encoder_module()
    sd = {k: v.detach().to(dev) for k, v in module.state_dict().items()}
    tensors, blocks, planes = pack_resnet(sd, "", wino_fn=ops.wino43_transform_weights)
    assert tuple(blocks) == R.FWD_BLOCKS and tuple(planes) == R.FWD_PLANES
    ptrs = _lib.ptr_array([None if t is None else t.data_ptr() for t in tensors])
    return module, tensors, ptrs


@pytest.mark.parametrize("n,h,w", R.FWD_CASES)
def test_composite_forward(dev, lib, encoder, n, h, w):
    """rpg_resnet_forward_f32 at sizes whose late layers see 2 x 2 and 1 x 1 maps and odd extents; with the larger n of each size
    wino_pays (restated in encoder_sweep_ref.layer_plan) takes Winograd in some layers and not in others -- 33 x 47, n = 48:
    layers 1, 2 and 4 (21, 16, 16 units), not layer 3 (12) --, with n = 1 in none.  The output from a workspace of 0xFF bytes
    is bit-identical to the one from a zeroed workspace."""
    from relpose_gnn_amd import _lib
    module, tensors, ptrs = encoder
    took = [t for t, _ in R.layer_plan(n, h, w)]
    assert (any(took) and not all(took)) if n > 1 else not any(took)
    if (n, h, w) == (48, 33, 47):
        assert R.layer_plan(n, h, w) == [(True, 21), (True, 16), (False, 12), (True, 16)]
    x = torch.randn(n, 3, h, w, generator=torch.Generator().manual_seed(n + h))
    xd = x.to(dev)
    planes = _lib.int_array(R.FWD_PLANES)
    need = int(lib.rpg_resnet_workspace_bytes(n, h, w, planes))
    assert need > 0
    feats = []
    for fill in (0xFF, 0x00):
        ws = torch.full((need,), fill, dtype=torch.uint8, device=dev)
        feat = torch.full((n, R.FWD_FEAT), float("nan"), device=dev)
        rc = lib.rpg_resnet_forward_f32(ptrs, len(tensors), _lib.int_array(R.FWD_BLOCKS), planes, R.FWD_FEAT, xd.data_ptr(), n, h, w,
                                        feat.data_ptr(), ws.data_ptr(), need, _stream())
        torch.cuda.synchronize()
        assert rc == 0, (rc, lib.rpg_last_error())
        feats.append(feat.cpu())
    assert bool(torch.isfinite(feats[0]).all()) and torch.equal(feats[0], feats[1])
    f64 = R.encoder_forward(module, x, torch.float64)
    f32 = R.encoder_forward(module, x, torch.float32)
    e_ref = max(rel_err(f32, f64), rel_err(R.encoder_forward(module, x, torch.float32, wino=True), f64))
    e_hip = rel_err(feats[0], f64)
    assert rel_err(feats[0], f32) < 1e-4
    assert e_ref > 0.0
    _record("composite", f"n{n}-{h}x{w}", {"e_ref": e_ref, "e_hip": e_hip, "ratio": e_hip / e_ref})
    assert e_hip <= M_FWD * e_ref, (e_ref, e_hip)
