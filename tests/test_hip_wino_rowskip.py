"""The row-per-item order of the one-tile 8-wave Winograd kernel (csrc/winograd.hip, RowOrder / wino43_conv8_kernel<true>): launches
whose n * Tw is a multiple of 128 put one image row into every workgroup and do not issue the kernel rows that would multiply
zero padding in the top and bottom image row.  Held to float64 per element with the bar of tests/test_hip_encoder_sweep.py
(c_hip <= M_KERNEL c_ref, c_ref of the fp32 CPU statement of the same algorithm, tests/encoder_sweep_ref.py), with and without
a residual and a ReLU.

Routes (RPG_TUNE_ keys; the default WINOGRAD = 1 would send these small shapes to the 4-wave kernel, which has no such order):
  wave8          one workgroup per tile, split-K parts where the launcher cuts them (every tile, at these sizes: the order is taken)
  wave8_whole    the same without split-K
  persist_whole  the persistent kernel, WINO_PERSIST = 2: it keeps the consecutive-row order (only in the bitwise test)
Shapes (n, H, W, Cin, Cout):
  (64, 7, 7, 64, 64)     Tw = 2, exactly one workgroup per image row
  (128, 7, 7, 32, 128)   two blocks of output channels; `wave8` cuts every tile into two parts
  (32, 14, 14, 32, 64)   Tw = 4
  (64, 2, 8, 32, 64)     H = 2: every row is a border row, two kernel rows everywhere
  (32, 3, 16, 48, 64)    three channel blocks: the middle row is 9 K steps, an odd number
  (32, 3, 16, 40, 64)    a channel tail (Cin % 16 != 0)
  (24, 7, 7, 32, 64)     n * Tw = 48: the other order; bitwise equal to what the parent commit computed (tests/golden)
"""
import hashlib
import json
import os

import pytest
import torch

import encoder_sweep_ref as R
from relpose_gnn_amd import ops
from test_hip_encoder_sweep import M_KERNEL

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wino_rowskip_parent.json")
ROUTES = {
    "wave8": {"WINOGRAD": 3, "WINO_SPLIT": 1, "WINO_PERSIST": 0, "INKERNEL_FIXUP": 0},
    "wave8_whole": {"WINOGRAD": 3, "WINO_SPLIT": 0, "WINO_PERSIST": 0},
    "persist_whole": {"WINOGRAD": 3, "WINO_SPLIT": 0, "WINO_PERSIST": 2},
}
SHAPES = {
    (64, 7, 7, 64, 64): ("wave8", "wave8_whole"),
    (128, 7, 7, 32, 128): ("wave8", "wave8_whole"),
    (32, 14, 14, 32, 64): ("wave8", "wave8_whole"),
    (64, 2, 8, 32, 64): ("wave8", "wave8_whole"),
    (32, 3, 16, 48, 64): ("wave8", "wave8_whole"),
    (32, 3, 16, 40, 64): ("wave8", "wave8_whole"),
}
OLD_ORDER_SHAPE = (24, 7, 7, 32, 64)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


_CASES = {}


def _case(shape):
    """(case with a residual, {res: (z, S, c_ref)}): the float64 statement of the case with and without its residual"""
    if shape not in _CASES:
        n, h, w, cin, cout = shape
        case = R.conv_case(n, h, w, cin, cout, 3, 1, 1, True, "normal", seed=700 + (n + 3 * h + 5 * w + 7 * cin + 11 * cout) % 100)
        plain = R.ConvCase(case.x, case.w, case.scale, case.shift, None, 1, 1, case.dist)
        z, S = R.conv_exact(plain)                   # once: the residual is added to z, its magnitude to S (as conv_exact does)
        refs = {}
        for res, c in ((True, case), (False, plain)):
            c_ref = R.conv_ref(c, "wino").c_ref
            refs[res] = (z + case.residual.double(), S + case.residual.double().abs(), c_ref) if res else (z, S, c_ref)
        _CASES[shape] = (case, refs)
    return _CASES[shape]


def _run(case, dev, res, relu):
    u = ops.wino43_transform_weights(case.w.to(dev))
    r = case.residual.to(dev) if res else None
    y = ops.conv3x3_wino43_bn_act_nhwc(case.x.to(dev), u, case.scale.to(dev), case.shift.to(dev), r, relu=relu)
    torch.cuda.synchronize()
    return y.cpu()


def _hold(case, refs, dev, tag):
    for res in (True, False):
        z, S, c_ref = refs[res]
        assert c_ref > 0.0
        for relu in (True, False):
            y = _run(case, dev, res, relu)
            c = R.c_of(y, z, S, relu=relu)
            print(f"{tag} res={int(res)} relu={int(relu)}: c_ref {c_ref:.3f} c_hip {c:.3f} ratio {c / c_ref:.3f}")
            assert c <= M_KERNEL * c_ref, (tag, res, relu, c_ref, c)


@pytest.mark.parametrize("route,shape", [pytest.param(r, s, id=f"{r}-" + "x".join(map(str, s))) for s, rs in SHAPES.items() for r in rs])
def test_rowskip_against_float64(dev, route, shape):
    case, refs = _case(shape)
    with ops.tuned(ROUTES[route]):
        _hold(case, refs, dev, f"{route} {shape}")


def _sha(t):
    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()


@pytest.mark.parametrize("route", ["wave8", "wave8_whole", "persist_whole"])
def test_other_order_is_bitwise_the_parent(dev, route):
    """n * Tw = 48 is not a multiple of 128: the launch keeps the consecutive-row order, whose code path must compute what it did
    before the row order existed.  tests/golden/wino_rowskip_parent.json holds the SHA-256 of the output bytes of the parent
    commit's library on an MI355X for the same seeded operands (route x residual x ReLU), and of the operands themselves."""
    with open(GOLDEN) as f:
        gold = json.load(f)
    case, refs = _case(OLD_ORDER_SHAPE)
    assert _sha(case.x) == gold["x"] and _sha(case.w) == gold["w"], "the seeded operands differ from the golden's: nothing to compare"
    with ops.tuned(ROUTES[route]):
        _hold(case, refs, dev, f"{route} {OLD_ORDER_SHAPE}")
        for res in (True, False):
            for relu in (True, False):
                assert _sha(_run(case, dev, res, relu)) == gold[f"{route}-res{int(res)}-relu{int(relu)}"], (route, res, relu)


# ---- non-finite inputs in the border rows (the pattern of tests/test_hip_nonfinite.py::test_wino43_variants; helpers copied)
def _put_nan(t, idx):
    t.view(torch.int32)[idx] = 0x7FC00000


def _wino_within(h, w, c, y, xx):
    """the 4-wide output tiles whose 6-wide input tile holds (y, xx), on the three rows a 3 x 3 kernel reaches"""
    within = torch.zeros(h, w, c, dtype=torch.bool)
    for ty in range(max(0, y - 1), min(h, y + 2)):
        for tx in range(0, w, 4):
            if tx - 1 <= xx <= tx + 4:
                within[ty, tx:tx + 4] = True
    return within


@pytest.mark.parametrize("route,shape", [("wave8", (64, 7, 7, 64, 64)), ("wave8_whole", (32, 14, 14, 32, 64)),
                                         ("wave8", (128, 7, 7, 32, 128)), ("wave8_whole", (64, 2, 8, 32, 64))],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_nan_in_border_rows(dev, route, shape):
    """One NaN pixel in row 0 and one in row H - 1: every output the float64 reference makes NaN is NaN (a skipped kernel row
    must not be one that reads it), no other image changes, and nothing outside the tiles that hold the pixel turns non-finite."""
    n, h, w, cin, cout = shape
    case, _ = _case(shape)
    img = n // 2
    with ops.tuned(ROUTES[route]):
        clean = _run(case, dev, True, False)
        assert bool(torch.isfinite(clean).all())
        for (y, xx) in ((0, 1), (h - 1, w - 2)):
            xb = case.x.clone()
            _put_nan(xb, (img, y, xx, 3))
            bad = R.ConvCase(xb, case.w, case.scale, case.shift, case.residual, 1, 1, case.dist)
            got = _run(bad, dev, True, False)
            ref = R.conv_direct(R.ConvCase(xb[img:img + 1], case.w, case.scale, case.shift, case.residual[img:img + 1], 1, 1), torch.float64)[0]
            others = torch.ones(n, dtype=torch.bool)
            others[img] = False
            assert torch.equal(got[others], clean[others]), "a NaN leaked into another image"
            g = got[img]
            assert bool(torch.isnan(ref).any()), "the test input does not reach the output"
            assert bool(torch.isnan(g)[torch.isnan(ref)].all()), "NaN swallowed"
            assert bool(_wino_within(h, w, cout, y, xx)[~torch.isfinite(g)].all()), "non-finite outputs beyond the tiles that hold the pixel"
            # the rows the reference reaches, exactly: the kernel row range of a border item reads neither more nor fewer rows
            assert torch.equal(torch.isnan(g).any(dim=2).any(dim=1), torch.isnan(ref).any(dim=2).any(dim=1))
