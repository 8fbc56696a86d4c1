"""The bf16 encoder kernels -- csrc/conv_bf16.hip on every launch route, the paired down-sampling launch, the fused BasicBlock of
csrc/block_bf16.inc, the fused stem of csrc/stem_bf16.hip, the max-pool, the average pool, the re-layout and the composite
rpg_resnet_forward_bf16 / _xbf16 -- held to CORRECT ROUNDING against float64 (tests/bf16_rounding.py, the bar of
test_hip_bf16_rounding.py, unchanged) on the route each case MEANS, inside a memory harness (tests/bf16_sweep_ref.py; its own tests
are test_bf16_sweep_cpu.py).

Every kernel is called through the C ABI with pointers into harness buffers: each operand lies in the middle of one allocation,
between two moats of max(64 KiB, 4 image rows); the input moats hold NaN, a bf16 output and its moats a signalling-NaN half-word
nobody computes.  After the launch the moats are bit-identical, no half-word of the output still holds the pattern and the
output is finite.  These kernels address through buffer resources of 2 GiB with nothing clamped: a wrong predicate is a load or
a store somewhere in the allocation next door, and only the moats see it.

Every case then reads rpg_conv_bf16_last_route and compares it with the dispatcher's rule restated in bf16_sweep_ref.py for the
device it runs on: a case whose shape the launcher quietly hands to another kernel FAILS.  (That is how the old `tiny_img` cases
went unnoticed: 244 patch pieces where 64 fit, six cases that always ran the interleaved kernel.)

What pins what (reasoned from the enumerated lists; no broken kernel is run on a GPU).
  Patch kernel, per route -- (tile, weight stages, form, one launch or main + tail) -- the accepted map with the smallest H and
  H W, the one with the smallest W, and the one with the most patch pieces: 1 x 13 and 13 x 5 for 256 x 128; 4 x 13 and 13 x 10 for the
  512-row tiles, alone, persistent and in front of a 256- or 128-row tail; 2 x 12 and 13 x 7 for 256 x 256 with four weight stages,
  2 x 10 and 11 x 6 with three, alone and in front of the 160 x 256 tail.  The flat maps put 10-20 images with their zero rows between
  them under one tile and fill 63-64 of the 64 patch pieces: a piece count off by one or an image-gap row mis-placed is a wrong
  value in every image.  The narrow ones have 38+ patch rows of 16 slots under a tile and the smallest divisors the magic
  divisions by W see.  Every case has a ragged last tile (a row predicate off by one stores into the moat or leaves payload),
  more than one workgroup, and the smallest map a twin with Cout = tile - 4 (the lean epilogue's column predicate).  The
  persistent form and the six tail re-tilings (three tails behind a four-stage and behind a three-stage main tile) run on 257+
  tiles of those maps; `launches` == 2 proves the split happened.
  Routes that take anything (general kernel on 64 x 64 / 128 x 128 / 256 x 64 at K steps 32 and 64, interleaved tiles 0-3, LDS-DMA
  configurations 0-9): 1 x 1, 2 x 2, 1 x 14, 2 x 7, 7 x 7, 13 x 14 and 14 x 13 inputs under 3x3/1, 3x3/2, 1x1/2 and 7x7/2 (Cin 8): on 1 x 1
  eight of nine taps are padding, stride 2 on odd extents halves unevenly, Cout = 72 / 60 leaves a channel tail on every tile;
  residual, ReLU, lean / general epilogue and fp32 output walk through all combinations per route.  Where a route's kernel does
  not apply (Cin = 8, K = 64 below a K step of 64) the rule names the fall-back and the fall-back is what must be observed; the
  Cin = 8 kind runs on the general routes and on one interleaved and one LDS-DMA route (the fall-back is the same launch for all).
  Pair: 8,192 x 1 x 1, 4,096 x 2 x 3, 168 x 13 x 14 -- the fewest pixels the launcher takes -- both outputs, and one image fewer is refused.
  Fused block: the acceptance boundary (5 x 14, the narrowest and the widest one- and two-strip maps) under forms 1, 3 and 5,
  bit-identical to the patch-kernel pair; each refused neighbour returns RPG_ERR_BAD_ARG and launches nothing.
  Pools and re-layout: bit-exact, through the grid-stride loop's second sweep and on H, W of 1 and 2; the max-pool with NaN pixels.
  Composite: late layers of 2 x 2 and 1 x 1 pixels, a run of two identity blocks, with the fused block, the pair and the
  depth-first chunking engaged and not -- OBSERVED through the per-launch timing slots (rpg_timing_read counts one per convolution
  launch): the count must change by what the fused block, the pair and the chunking each add or save; 0xFF workspace against
  zeroed, fp32 images against bf16 images, bit for bit.

Figures of one run on an MI355X are in profiles/bf16_sweep_observed.json (RPG_SWEEP_RECORD): per case the route, c_ref, the
ambiguous share, for fp32 outputs the observed c, for the composite the timing-slot counts.  Every observed route equals the
restated one there: 31 distinct (family, tile, detail, launches) records, the 16 patch routes with the persistent form and the six
two-launch tails among them.  Worst observed c of the 64 fp32-output cases: 0.795 c_ref (general kernel, 128 x 128 tile, K step 32,
3x3/1 on 2,332 images of 2 x 7: c_ref 2.54, observed 2.02), a fifth of the 4 c_ref allowed; the others 0.46-0.79 c_ref.  c_ref of
the convolution cases: 1.41-4.18.  Largest ambiguous share: 1.23 % (cap 2 %).  Composite: d_hip <= 1.10 d_ref (274 images of
33 x 47 without block fusion and chunked; 3 d_ref allowed).
Wall time on an MI355X host: 39.6 s for this file (613 cases, float64 references shared per convolution; the slowest case 1.3 s) next to
the 31.6 s of test_hip_bf16_rounding.py.

What the route assertions found in the OLDER tests (fixed there as comments and expectations, no bar moved): besides tiny_img,
`ragged_192` under the by-width patch modes, 1 x 64 x 86 and 300 x 13 x 17 with 64 channels in test_hip_bf16.py never ran the patch
kernel (66-80 pieces), and the layer-1 shape of test_conv_bf16_dma_configs ran the patch kernel in front of every forced LDS-DMA
configuration.
"""
import pytest
import torch
import torch.nn.functional as F

import bf16_rounding as R
import bf16_sweep_ref as B
import encoder_sweep_ref as E
from test_hip_graph_sweep import _record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.set_num_threads(min(16, torch.get_num_threads()))           # the float64 references run on the CPU
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from relpose_gnn_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _observed() -> tuple:
    from relpose_gnn_amd import ops
    r = ops.conv_bf16_last_route()
    return (r["family"], r["bm"], r["bn"], r["detail"], r["launches"])


def _opt(buf):
    return None if buf is None else buf.ptr()


class _Buffers:
    """A convolution's operands in harness buffers."""

    def __init__(self, op: B.Operands, dev):
        self.x, self.w = B.Moated16(op.x.shape, dev, op.x), B.Moated16(op.w.shape, dev, op.w)
        self.scale, self.shift = E.Moated(op.scale.shape, dev, op.scale), E.Moated(op.shift.shape, dev, op.shift)
        self.res = None if op.residual is None else B.Moated16(op.residual.shape, dev, op.residual)
        self.inputs = [b for b in (self.x, self.w, self.scale, self.shift, self.res) if b is not None]


_BUF = {}


def _buffers(case, dev):
    """Operands and their device buffers, shared by the cases that run the same convolution (the list is sorted by it)."""
    key = (case.n, case.h, case.w, case.cin, case.cout, case.k, case.stride, case.pad, case.res)
    if key not in _BUF:
        _BUF.clear()
        _BUF[key] = (B.case_operands(case), _Buffers(B.case_operands(case), dev))
    return _BUF[key]


_CASES = sorted(B.all_cases(), key=lambda c: (c.n, c.h, c.w, c.cin, c.cout, c.k, c.stride, c.pad, c.res, c.route))


@pytest.mark.parametrize("case", _CASES, ids=lambda c: c.id)
def test_conv_route(dev, lib, cus, case):
    """One (route, case) of bf16_sweep_ref: rc == 0, the observed route is the restated one on THIS device -- and for a patch route
    the one the list means --, the harness has no findings, every element is inside the correct-rounding interval at FACTOR c_ref
    and at most AMBIGUOUS_CAP of them have two acceptable answers."""
    from relpose_gnn_amd import ops
    want = case.expected(cus)
    if case.route in B.PATCH_ROUTES:
        assert want == B.PATCH_ROUTES[case.route]["want"], (case.id, cus, want)
    op, buf = _buffers(case, dev)
    ho, wo = case.out_hw
    y = (E.Moated if case.out_f32 else B.Moated16)((case.n, ho, wo, case.cout), dev)
    with ops.tuned(case.keys):
        rc = lib.rpg_conv2d_bn_act_nhwc_bf16(buf.x.ptr(), buf.w.ptr(), buf.scale.ptr(), buf.shift.ptr(), _opt(buf.res), y.ptr(), case.n,
                                             case.h, case.w, case.cin, case.cout, case.k, case.k, case.stride, case.pad, int(case.relu),
                                             int(case.out_f32), _stream())
        got = _observed()
        torch.cuda.synchronize()
    assert rc == 0, (rc, lib.rpg_last_error())
    assert got == want, (case.id, "observed", got, "restated", want)
    assert B.harness_findings(buf.inputs, y) == []
    out = y.t.cpu()
    figures = {"route": list(got), "c_ref": op.c_ref}
    if case.out_f32:
        # |y - act(z)| <= FACTOR c_ref u S per element (bf16_rounding.check_f32's rule, at the c_ref over >= 2^16 outputs)
        err = (out.double() - (op.ref.z.clamp_min(0.0) if case.relu else op.ref.z)).abs()
        figures["c_observed"] = R._ratio_max(torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err), op.ref.S)
        assert figures["c_observed"] <= R.FACTOR * op.c_ref, (case.id, figures)
        out = out.bfloat16()                                  # and the same values through the interval (their rounding is exact)
    rep = R.check(out, op.ref, case.relu, c_ref=op.c_ref, what=case.id)
    assert rep["bad"] == 0 and rep["ambiguous"] <= R.AMBIGUOUS_CAP
    _record("conv", case.id, {**figures, "ambiguous": rep["ambiguous"]})


# ----------------------------------------------------------------------------------------------------------------------
# the paired down-sampling launch
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout", B.PAIR_CHANNELS, ids=lambda v: str(v))
@pytest.mark.parametrize("n,h,w", B.PAIR_SHAPES, ids=lambda v: str(v))
def test_pair(dev, lib, cus, n, h, w, cin, cout):
    """rpg_conv_pair_bf16 at the fewest output pixels the launcher takes (8192 on 1 x 1 and 1 x 2 output maps, 8232 on 7 x 7):
    both outputs inside their intervals, every buffer's moat intact, the route observed; one image fewer is refused."""
    from relpose_gnn_amd import _lib
    a = B.conv_operands(n, h, w, cin, cout, 3, 2, 1, False, seed=h)
    g = torch.Generator().manual_seed(77 + h)
    wb = (torch.randn((cout, 1, 1, cin), generator=g) * (2.0 / cin) ** 0.5).bfloat16()
    sb, hb = R.wide_scales(cout, 12, shift_scale=2.0)
    nchw = lambda t: t.permute(0, 3, 1, 2)
    ref_b = R.conv_ref(nchw(a.x), nchw(wb), sb, hb, None, 2, 0)
    buf = _Buffers(a, dev)
    wbb, sbb, hbb = B.Moated16(wb.shape, dev, wb), E.Moated(sb.shape, dev, sb), E.Moated(hb.shape, dev, hb)
    ho, wo = B.conv_out(h, 3, 2, 1), B.conv_out(w, 3, 2, 1)
    ya, yb = B.Moated16((n, ho, wo, cout), dev), B.Moated16((n, ho, wo, cout), dev)
    args = lambda nn: (buf.x.ptr(), buf.w.ptr(), buf.scale.ptr(), buf.shift.ptr(), ya.ptr(), wbb.ptr(), sbb.ptr(), hbb.ptr(), yb.ptr(), nn, h, w,
                       cin, cout, 3, 2, 1, _stream())
    want = B.pair_route({}, n, h, w, cin, cout, 3, 2, 1, cus)
    assert want[0] == "pair"
    if n * ho * wo - ho * wo < 8192:
        assert lib.rpg_conv_pair_bf16(*args(n - 1)) == _lib.RPG_ERR_BAD_ARG and _observed() == B.NONE
        torch.cuda.synchronize()
        assert ya.unwritten() == ya.numel and yb.unwritten() == yb.numel
    rc = lib.rpg_conv_pair_bf16(*args(n))
    got = _observed()
    torch.cuda.synchronize()
    assert rc == 0 and got == want, (rc, got, want)
    inputs = buf.inputs + [wbb, sbb, hbb]
    assert B.harness_findings(inputs, ya) == [] and B.harness_findings(inputs, yb) == []
    ra = R.check(ya.t.cpu(), a.ref, True, c_ref=a.c_ref, what="pair: 3x3 / 2")
    rb = R.check(yb.t.cpu(), ref_b, False, what="pair: 1x1 / 2 shortcut")
    assert ra["bad"] == 0 and rb["bad"] == 0 and max(ra["ambiguous"], rb["ambiguous"]) <= R.AMBIGUOUS_CAP
    _record("pair", f"n{n}h{h}w{w}c{cin}o{cout}", {"route": list(got), "c_ref": a.c_ref, "c_ref_shortcut": rb["c_ref"],
                                                  "ambiguous": max(ra["ambiguous"], rb["ambiguous"])})


# ----------------------------------------------------------------------------------------------------------------------
# the fused BasicBlock
# ----------------------------------------------------------------------------------------------------------------------
def _block_boundary():
    """(accepted, refused) maps on the fused block's acceptance boundary, enumerated from block_plan: the smallest H W, the
    narrowest map, the widest one-strip and the narrowest and widest two-strip maps with their smallest H; and of each the
    neighbours with one row or one column less (or more, at the wide end) that the launcher refuses."""
    ok = {(h, w) for h in range(1, 41) for w in range(1, 125) if B.block_plan(3, h, w) is not None}
    one = {e for e in ok if B.block_plan(3, *e)["strips"] == 1}
    picks = [min(ok, key=lambda e: (e[0] * e[1], e[0])), min(ok, key=lambda e: (e[1], e[0])),
             min((e for e in one if e[1] == max(w for _, w in one)), key=lambda e: e[0]),
             min((e for e in ok - one if e[1] == min(w for _, w in ok - one)), key=lambda e: e[0]),
             min((e for e in ok if e[1] == max(w for _, w in ok)), key=lambda e: e[0])]
    picks = list(dict.fromkeys(picks))
    refused = list(dict.fromkeys(e for h, w in picks for e in ((h - 1, w), (h, w - 1), (h, w + 1)) if e[0] >= 1 and e[1] >= 1 and e not in ok))
    return picks, refused


_BLOCK_OK, _BLOCK_REFUSED = _block_boundary()


def _block_operands(n, h, w, dev):
    g = torch.Generator().manual_seed(1000 + n * h + w)
    x = torch.randn((n, h, w, 64), generator=g).bfloat16()
    w1 = (torch.randn((64, 3, 3, 64), generator=g) * (2.0 / 576) ** 0.5).bfloat16()
    w2 = (torch.randn((64, 3, 3, 64), generator=g) * (2.0 / 576) ** 0.5).bfloat16()
    (s1, b1), (s2, b2) = R.wide_scales(64, 41, 0.2), R.unit_scales(64, 42, 0.2)
    bufs = [B.Moated16(x.shape, dev, x), B.Moated16(w1.shape, dev, w1), E.Moated(s1.shape, dev, s1), E.Moated(b1.shape, dev, b1),
            B.Moated16(w2.shape, dev, w2), E.Moated(s2.shape, dev, s2), E.Moated(b2.shape, dev, b2)]
    return bufs


def _block_call(lib, bufs, y, n, h, w):
    return lib.rpg_basicblock64_bf16(*[b.ptr() for b in bufs], y.ptr(), n, h, w, _stream())


@pytest.mark.parametrize("form", [1, 3, 5], ids=["one_tile_per_workgroup", "persistent", "two_group"])
@pytest.mark.parametrize("h,w", _BLOCK_OK, ids=lambda v: str(v))
def test_fused_block_boundary(dev, lib, cus, h, w, form):
    """rpg_basicblock64_bf16 on the acceptance boundary under RPG_TUNE_BF16_FUSE_BLOCK = 1 / 3 / 5 (3 images; the persistent form
    with as many as make more than one round of tiles): the route observed, the harness, and the output BIT-IDENTICAL to the two
    launches of the patch kernel (on each strip's view where the map runs as two strips), as
    test_fused_basicblock64_equals_two_convolutions demands at its sizes.  Those two launches are checked to BE the patch kernel."""
    from relpose_gnn_amd import ops
    plan = B.block_plan(3, h, w)
    n = 3 if form != 3 else -(-((cus & ~7) * 512 + 1) // (h * plan["view"] * plan["strips"]))
    want = B.block_route({"BF16_FUSE_BLOCK": form}, n, h, w, cus)
    assert want[0] == {1: "block", 3: "block_persistent", 5: "block_two_group"}[form] or (form == 5 and plan["lds"] + 4096 > B.LDS_MAX)
    bufs = _block_operands(n, h, w, dev)
    y = B.Moated16((n, h, w, 64), dev)
    with ops.tuned({"BF16_FUSE_BLOCK": form}):
        rc = _block_call(lib, bufs, y, n, h, w)
        got = _observed()
        torch.cuda.synchronize()
    assert rc == 0 and got == want, (rc, got, want)
    assert B.harness_findings(bufs, y) == []
    x, w1, s1, b1, w2, s2, b2 = (b.t for b in bufs)

    def two_launches(xx):
        t = ops.conv2d_bn_act_nhwc_bf16(xx, w1, s1, b1, None, stride=1, pad=1, relu=True)
        r1 = _observed()
        out = ops.conv2d_bn_act_nhwc_bf16(t, w2, s2, b2, xx, stride=1, pad=1, relu=True)
        assert r1[0] == "patch" and _observed()[0] == "patch", (r1, _observed())
        return out
    with ops.tuned({"BF16_PATCH": 2}):
        if plan["strips"] == 1:
            ref = two_launches(x.contiguous())
        else:
            ws, wv = (w + 1) // 2, plan["view"]
            y0, y1 = two_launches(x[:, :, :wv, :].contiguous()), two_launches(x[:, :, w - wv:, :].contiguous())
            ref = torch.cat([y0[:, :, :ws, :], y1[:, :, ws - (w - wv):, :]], dim=2)
        torch.cuda.synchronize()
    bad = (y.t != ref).nonzero()
    assert bad.numel() == 0, ((h, w), int(bad.shape[0]), bad[:5].tolist())
    _record("block", f"n{n}h{h}w{w}-form{form}", {"route": list(got), "strips": plan["strips"], "view": plan["view"], "pieces": plan["pieces"]})


@pytest.mark.parametrize("h,w", _BLOCK_REFUSED, ids=lambda v: str(v))
def test_fused_block_refuses_the_neighbours(dev, lib, h, w):
    from relpose_gnn_amd import _lib
    assert B.block_plan(3, h, w) is None
    bufs = _block_operands(3, h, w, dev)
    y = B.Moated16((3, h, w, 64), dev)
    assert _block_call(lib, bufs, y, 3, h, w) == _lib.RPG_ERR_BAD_ARG and _observed() == B.NONE
    torch.cuda.synchronize()
    assert y.unwritten() == y.numel and y.moats_intact()


# ----------------------------------------------------------------------------------------------------------------------
# the fused stem
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xdtype", [torch.float32, torch.bfloat16], ids=["x_f32", "x_bf16"])
@pytest.mark.parametrize("form", list(B.STEM_FORMS))
@pytest.mark.parametrize("h,w", B.STEM_SIZES)
def test_stem(dev, lib, h, w, form, xdtype):
    """rpg_stem_conv7x7s2_bn_relu_maxpool_bf16 / _xbf16 on 1 x 1 .. 61 x 63 images under every form of the kernel: the harness and
    the interval carried through ReLU and max-pool (both monotone; the pool commutes with the rounding)."""
    from relpose_gnn_amd import ops
    from relpose_gnn_amd.params import pack_stem_bf16
    x, wt, scale, shift, ref, c_ref = B.stem_reference(h, w)
    n = x.shape[0]
    wp = pack_stem_bf16(wt)
    xb = E.Moated(x.shape, dev, x) if xdtype == torch.float32 else B.Moated16(x.shape, dev, x.bfloat16())
    wpb, sc, sh = B.Moated16(wp.shape, dev, wp), E.Moated(scale.shape, dev, scale), E.Moated(shift.shape, dev, shift)
    half = lambda v: (v - 1) // 2 + 1
    y = B.Moated16((n, half(half(h)), half(half(w)), 64), dev)
    fn = lib.rpg_stem_conv7x7s2_bn_relu_maxpool_bf16 if xdtype == torch.float32 else lib.rpg_stem_conv7x7s2_bn_relu_maxpool_bf16_xbf16
    with ops.tuned({"FUSED_STEM": B.STEM_FORMS[form]}):
        rc = fn(xb.ptr(), wpb.ptr(), sc.ptr(), sh.ptr(), y.ptr(), n, h, w, _stream())
        torch.cuda.synchronize()
    assert rc == 0, (rc, lib.rpg_last_error())
    assert B.harness_findings([xb, wpb, sc, sh], y) == []
    rep = R.check(y.t.cpu(), ref, True, post=B.stem_pool, c_ref=c_ref, what=f"stem {h}x{w} {form} {xdtype}")
    assert rep["bad"] == 0 and rep["ambiguous"] <= R.AMBIGUOUS_CAP
    _record("stem", f"{h}x{w}-{form}-{'bf16' if xdtype == torch.bfloat16 else 'f32'}", {"c_ref": c_ref, "ambiguous": rep["ambiguous"]})


# ----------------------------------------------------------------------------------------------------------------------
# re-layout and pools
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xdtype", [torch.float32, torch.bfloat16], ids=["x_f32", "x_bf16"])
@pytest.mark.parametrize("n,h,w", B.RELAYOUT_SHAPES)
def test_relayout(dev, lib, n, h, w, xdtype):
    """rpg_nchw3_to_nhwc8_bf16, bit-exact against torch's rounding; 3 x 900 x 800 pixels is more than 8192 x 256: the grid-stride
    loop with a ragged last stride.  (An odd number of bf16 source pixels is padded to whole words for the harness.)"""
    x = torch.randn(n, 3, h, w, generator=torch.Generator().manual_seed(h))
    want = F.pad(x.bfloat16().permute(0, 2, 3, 1), (0, 5))
    if xdtype == torch.float32:
        xb = E.Moated(x.shape, dev, x)
    else:
        flat = x.bfloat16().reshape(-1)
        flat = torch.cat([flat, torch.full((flat.numel() % 2,), float("nan")).bfloat16()])
        xb = B.Moated16(flat.shape, dev, flat)
    y = B.Moated16((n, h, w, 8), dev)
    assert lib.rpg_nchw3_to_nhwc8_bf16(xb.ptr(), int(xdtype == torch.bfloat16), y.ptr(), n, h, w, _stream()) == 0
    torch.cuda.synchronize()
    assert B.harness_findings([xb], y) == []
    assert torch.equal(y.t.cpu().view(torch.int16), want.contiguous().view(torch.int16))


@pytest.mark.parametrize("n,h,w,c", B.MAXPOOL_SHAPES)
def test_maxpool(dev, lib, n, h, w, c):
    """rpg_maxpool3x3s2_nhwc_bf16, bit-exact; 5 x 65 x 66 x 128 output lanes are more than 8192 x 256; H or W of 1 and 2."""
    x = torch.randn(n, h, w, c, generator=torch.Generator().manual_seed(h + w)).bfloat16()
    ref = F.max_pool2d(x.float().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous().bfloat16()
    xb, y = B.Moated16(x.shape, dev, x), B.Moated16(ref.shape, dev)
    assert lib.rpg_maxpool3x3s2_nhwc_bf16(xb.ptr(), y.ptr(), n, h, w, c, _stream()) == 0
    torch.cuda.synchronize()
    assert B.harness_findings([xb], y) == []
    assert torch.equal(y.t.cpu().view(torch.int16), ref.view(torch.int16))


@pytest.mark.parametrize("n,hw,c", B.AVGPOOL_SHAPES)
def test_global_avgpool(dev, lib, n, hw, c):
    """rpg_global_avgpool_nhwc_bf16: n c / 8 = 2,097,280 lanes are just above 8192 x 256; hw of 1, 2, 4 (the composite's late
    layers) and 49.  Bit-exact against the CPU statement of the kernel's order: ascending fp32 sum, one division, one rounding."""
    x = E.activations((n, hw, c), "act", seed=hw).bfloat16()
    want = B.avgpool_ordered_bf16(x)
    xb, y = B.Moated16(x.shape, dev, x), B.Moated16((n, c), dev)
    assert lib.rpg_global_avgpool_nhwc_bf16(xb.ptr(), y.ptr(), n, hw, c, _stream()) == 0
    torch.cuda.synchronize()
    assert B.harness_findings([xb], y) == []
    assert torch.equal(y.t.cpu().view(torch.int16), want.view(torch.int16))


def test_maxpool_propagates_nan(dev, lib):
    """A NaN pixel (one channel of an inner pixel, one of a corner pixel) is the maximum of every window that covers it, as the
    header says and torch does; every other output is the plain maximum."""
    n, h, w, c = 2, 5, 6, 16
    x = torch.randn(n, h, w, c, generator=torch.Generator().manual_seed(3)).bfloat16()
    x[0, 1, 1, 5] = float("nan")                           # rows and columns 1 lie in two windows each: four outputs
    x[1, 4, 5, 9] = float("nan")
    nchw = x.float().permute(0, 3, 1, 2)
    pool = lambda t: F.max_pool2d(t, 3, 2, 1).permute(0, 2, 3, 1)
    want_nan = pool(torch.isnan(nchw).float()) > 0
    want = pool(torch.nan_to_num(nchw, nan=float("-inf"))).bfloat16()
    assert int(want_nan.sum()) == 4 + 1
    xb, y = B.Moated16(x.shape, dev, x), B.Moated16(want.shape, dev)
    assert lib.rpg_maxpool3x3s2_nhwc_bf16(xb.ptr(), y.ptr(), n, h, w, c, _stream()) == 0
    torch.cuda.synchronize()
    assert B.harness_findings([xb], y) == ["the output is not finite"]            # (moats intact, every half-word written)
    got = y.t.cpu()
    assert torch.equal(torch.isnan(got.float()), want_nan)
    assert torch.equal(got[~want_nan].view(torch.int16), want[~want_nan].view(torch.int16))


def test_streaming_entry_points_refuse_bad_arguments(dev, lib):
    from relpose_gnn_amd import _lib
    t = torch.zeros(64, dtype=torch.bfloat16, device=dev)
    assert lib.rpg_nchw3_to_nhwc8_bf16(t.data_ptr(), 1, t.data_ptr(), 1, 65536, 32768, None) == _lib.RPG_ERR_BAD_ARG       # h w = 2^31
    assert lib.rpg_maxpool3x3s2_nhwc_bf16(t.data_ptr(), t.data_ptr(), 1, 65536, 32768, 8, None) == _lib.RPG_ERR_BAD_ARG
    assert lib.rpg_maxpool3x3s2_nhwc_bf16(t.data_ptr(), t.data_ptr(), 1, 2, 2, 12, None) == _lib.RPG_ERR_BAD_ARG         # c % 8
    assert lib.rpg_global_avgpool_nhwc_bf16(t.data_ptr(), None, 1, 2, 8, None) == _lib.RPG_ERR_BAD_ARG
    assert lib.rpg_nchw3_to_nhwc8_bf16(t.data_ptr(), 1, t.data_ptr() + 2, 1, 1, 1, None) == _lib.RPG_ERR_BAD_ARG         # y not 16-byte aligned


def test_a_refused_launch_records_no_route(dev, lib):
    """Family 0 means refused, for every launcher that records: a convolution that ran, then a Linear and a convolution with bad
    arguments."""
    from relpose_gnn_amd import _lib, ops
    x = torch.zeros((1, 2, 2, 8), dtype=torch.bfloat16, device=dev)
    wt = torch.zeros((8, 1, 1, 8), dtype=torch.bfloat16, device=dev)
    for bad in (lambda: lib.rpg_linear_bf16(None, wt.data_ptr(), None, None, None, None, None, 0, x.data_ptr(), 4, 8, 8, 0, None),
                lambda: lib.rpg_conv2d_bn_act_nhwc_bf16(x.data_ptr(), wt.data_ptr(), None, None, None, None, 1, 2, 2, 8, 8, 1, 1, 1, 0, 0, 0, None)):
        ops.conv2d_bn_act_nhwc_bf16(x, wt, None, None, None, stride=1, pad=0, relu=False)
        assert _observed()[0] != "none"
        assert bad() == _lib.RPG_ERR_BAD_ARG and _observed() == B.NONE
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------------
# the composite encoder
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def encoder(dev):
    from relpose_gnn_amd.params import pack_resnet_bf16
    module = B.fwd_module()
    tensors, blocks, planes = pack_resnet_bf16({k: v.detach() for k, v in module.state_dict().items()}, "")
    assert tuple(blocks) == B.FWD_BLOCKS and tuple(planes) == B.FWD_PLANES and len(tensors) == 3 + 6 + 6 + 9 * 3 + 2 + 1
    return tensors, [t.to(dev) for t in tensors]


_FWD_CONFIGS = {"default": {}, "three_kernel_stem": {"FUSED_STEM": 0}, "no_block_fusion": {"BF16_FUSE_BLOCK": 0}, "no_pair": {"BF16_PAIR": 0},
                "chunked": {"BF16_CHUNK": B.FWD_CHUNK}}


@pytest.mark.parametrize("large", [False, True], ids=["n2", "large_n"])
@pytest.mark.parametrize("h,w", B.FWD_SIZES, ids=lambda v: str(v))
def test_composite_forward(dev, lib, cus, encoder, h, w, large):
    """rpg_resnet_forward_bf16 / _xbf16 with blocks (2, 1, 1, 1) at sizes whose late layers see 2 x 2 and 1 x 1 maps.  n = 2: no
    layer has the 8192 pixels of the large-M routes.  Large n (911 | 274 | 235 images): layer 1 has them (33 x 47 and 40 x 56:
    the fused block takes the 9 x 12 and 10 x 14 maps; 17 x 17: its 5 x 5 maps are refused and two launches run), layer 2's pair
    launch has them, and RPG_TUNE_BF16_CHUNK = 24 images from 1 MB walks layer 1's run of two identity blocks depth-first.
    Per configuration: rel_l2 to the float64 emulation <= 3 x that of its fp32 evaluation (the bar of
    test_bf16_encoder_vs_bf16_emulating_oracle); a 0xFF workspace gives the bits of a zeroed one; bf16 images give the bits of
    fp32 images.  Across configurations bit-identity is asserted only where the project claims it: the pair launch against two
    launches (test_bf16_encoder_paired_downsample_launch_is_bit_identical).
    That the paths ENGAGE is observed, not inferred: with rpg_timing_enable every convolution launch of the forward takes one
    timing slot (a fused block one for its two convolutions, a pair one for its two, a refused fused block one and then two), so
    the slot count of each configuration must differ from the default's by exactly what the restated conditions predict."""
    from relpose_gnn_amd import _lib, ops
    cpu_tensors, tensors = encoder
    n = B.fwd_large_n(h, w) if large else 2
    (h1, w1), (h2, w2) = E.layer_extents(h, w)[:2]
    if large:
        assert n * h1 * w1 >= 8192 and B.pair_route({}, n, h1, w1, 64, 128, 3, 2, 1, cus)[0] == "pair"
        assert (B.block_plan(n, h1, w1) is not None) == ((h, w) != (17, 17))
        assert n > 24 and n * h1 * w1 * 64 * 2 >= 1 << 20
    else:
        assert n * h1 * w1 < 8192
    x = torch.randn(n, 3, h, w, generator=torch.Generator().manual_seed(n + h))
    xd, xd16 = x.to(dev), x.bfloat16().to(dev)
    ptrs = _lib.ptr_array([t.data_ptr() for t in tensors])
    blocks, planes = _lib.int_array(B.FWD_BLOCKS), _lib.int_array(B.FWD_PLANES)
    need = int(lib.rpg_resnet_bf16_workspace_bytes(n, h, w, planes))
    assert need > 0

    def forward(fn, xin, fill):
        ws = torch.full((need,), fill, dtype=torch.uint8, device=dev)
        feat = torch.full((n, B.FWD_FEAT), float("nan"), device=dev)
        rc = fn(ptrs, len(tensors), blocks, planes, B.FWD_FEAT, xin.data_ptr(), n, h, w, feat.data_ptr(), ws.data_ptr(), need, _stream())
        torch.cuda.synchronize()
        assert rc == 0, (rc, lib.rpg_last_error())
        return feat.cpu()
    e64 = R.emulate_encoder_bf16(cpu_tensors, B.FWD_BLOCKS, B.FWD_PLANES, x, torch.float64)
    e32 = R.emulate_encoder_bf16(cpu_tensors, B.FWD_BLOCKS, B.FWD_PLANES, x, torch.float32)
    d_ref = R.rel_l2(e32, e64)
    assert d_ref > 0.0
    feats, slots = {}, {}
    for name, keys in _FWD_CONFIGS.items():
        with ops.tuned(keys):
            f = forward(lib.rpg_resnet_forward_bf16, xd, 0xFF)
            assert torch.equal(f, forward(lib.rpg_resnet_forward_bf16, xd, 0x00)), name
            assert torch.equal(f, forward(lib.rpg_resnet_forward_bf16_xbf16, xd16, 0xFF)), name
            ops.timing_enable(True)
            try:
                ops.timing_read()                                       # (empties the slots)
                forward(lib.rpg_resnet_forward_bf16, xd, 0x00)
                slots[name] = ops.timing_read()["conv"]["launches"]
            finally:
                ops.timing_enable(False)
        assert bool(torch.isfinite(f).all())
        d_hip = R.rel_l2(f, e64)
        _record("composite", f"n{n}-{h}x{w}-{name}", {"d_ref": d_ref, "d_hip": d_hip, "ratio": d_hip / d_ref})
        assert d_hip <= 3.0 * d_ref, (name, d_hip, d_ref)
        feats[name] = f
    assert torch.equal(feats["default"], feats["no_pair"])
    # what engaged, from the slot counts: the pair saves one slot per down-sampling layer it takes; per layer-1 block the fused
    # kernel saves one, a refused one costs one; the chunked walk runs layer 1's four convolutions once per group of 24 images
    ext = E.layer_extents(h, w)
    pairs = sum(B.pair_route({}, n, *ext[l - 1], B.FWD_PLANES[l - 1], B.FWD_PLANES[l], 3, 2, 1, cus) != B.NONE for l in (1, 2, 3))
    fused = 0 if n * h1 * w1 < 8192 else (-1 if B.block_plan(n, h1, w1) is not None else 1)
    chunked = n > 24 and n * h1 * w1 * 64 * 2 >= 1 << 20
    assert pairs == (1 if large else 0) and (fused != 0) == large and chunked == large
    assert slots["no_pair"] - slots["default"] == pairs, slots
    assert slots["default"] - slots["no_block_fusion"] == B.FWD_BLOCKS[0] * fused, slots
    assert slots["chunked"] - slots["no_block_fusion"] == ((-(-n // 24) - 1) * 4 if chunked else 0), slots
    _record("composite_slots", f"n{n}-{h}x{w}", slots)
