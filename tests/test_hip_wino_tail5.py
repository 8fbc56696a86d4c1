"""The tail-uniform row layout of the one-tile 8-wave Winograd kernel (csrc/winograd.hip, wino43_conv8_kernel<true, true>) and the
dead sixth position of a row's last tile.  Where a launch takes the row order and Tw = 2, rows 0-63 of a workgroup are the first
tiles of 64 images and rows 64-127 their last tiles; where W % 4 != 0 the last tile's fourth output column is outside the image,
it is the only reader of Winograd position 5, and the waves that hold last tiles do not issue that position's MFMAs, its input
transform or its operand reads.  Nothing that is stored may change: every case is held to float64 with the bar of
tests/test_hip_encoder_sweep.py (c_hip <= M_KERNEL c_ref) AND its output bytes are compared with what the parent commit's library
computed on an MI355X for the same seeded operands (tests/golden/wino_tail5_parent.json: SHA-256 per route x residual x ReLU,
and of the operands themselves), with and without a residual and a ReLU.

Routes (RPG_TUNE_ keys, as in tests/test_hip_wino_rowskip.py):
  wave8          one workgroup per tile, split-K parts where the launcher cuts them, separate fix-up launch
  wave8_whole    the same without split-K
  wave8_combine  split-K parts added by the last workgroup to arrive (wino43_combine_last); first two shapes only
Shapes (n, H, W, Cin, Cout):
  (64, 7, 7, 64, 64)     one workgroup per image row, split and whole
  (128, 7, 7, 32, 128)   two channel blocks and two image halves per row
  (64, 2, 6, 32, 64)     two live columns in the last tile; every row is a border row
  (64, 3, 5, 48, 64)     one live column; 9 K steps in the middle row
  (64, 3, 7, 40, 64)     channel tail
  (64, 4, 8, 32, 64)     W % 4 == 0: nothing may be skipped
  (32, 14, 14, 32, 64)   Tw = 4: untouched route, same bits
  (24, 7, 7, 32, 64)     the other tile order: untouched route, same bits
The matrix work the launcher reports (ops.timing_read()["conv_wino"]["executed"]) tells which route was taken: the skipping
launches issue 44 of 48 MFMAs per wave and K step on average (waves 4-7: 40), every other launch all 48."""
import hashlib
import json
import os

import pytest
import torch

import encoder_sweep_ref as R
from relpose_gnn_amd import ops
from test_hip_encoder_sweep import M_KERNEL

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wino_tail5_parent.json")
ROUTES = {
    "wave8": {"WINOGRAD": 3, "WINO_SPLIT": 1, "WINO_PERSIST": 0, "INKERNEL_FIXUP": 0},
    "wave8_whole": {"WINOGRAD": 3, "WINO_SPLIT": 0, "WINO_PERSIST": 0},
    "wave8_combine": {"WINOGRAD": 3, "WINO_SPLIT": 1, "WINO_PERSIST": 0, "INKERNEL_FIXUP": 2},
}
SHAPES = ((64, 7, 7, 64, 64), (128, 7, 7, 32, 128), (64, 2, 6, 32, 64), (64, 3, 5, 48, 64), (64, 3, 7, 40, 64), (64, 4, 8, 32, 64),
          (32, 14, 14, 32, 64), (24, 7, 7, 32, 64))
CASES = [(r, s) for s in SHAPES for r in ("wave8", "wave8_whole")] + [("wave8_combine", s) for s in SHAPES[:2]]


def shape_id(shape):
    return "x".join(map(str, shape))


def expected_executed(shape):
    """Matrix-pipe FLOP of one launch of the one-tile 8-wave kernel: workgroups x K steps x MFMAs per wave x 8 waves x 4096.
    Row order (n * Tw a multiple of 128, H >= 2): 2 kernel rows in the top and bottom image row; tail-uniform layout with a dead
    position (Tw = 2, W % 4 != 0): 44 MFMAs per wave on average."""
    n, h, w, cin, cout = shape
    tw = (w + 3) // 4
    kpr = (cin + 15) // 16
    tiles = -(-(n * h * tw) // 128) * -(-cout // 64)
    rm = (n * tw) % 128 == 0 and h >= 2
    steps = tiles // h * kpr * (3 * h - 2) if rm else tiles * 3 * kpr
    mfmas = 44 if rm and tw == 2 and w % 4 else 48
    return steps * mfmas * 8.0 * 4096.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


_CASES = {}


def make_case(shape):
    """(case with a residual, {res: (z, S, c_ref)}): the float64 statement of the case with and without its residual"""
    if shape not in _CASES:
        n, h, w, cin, cout = shape
        case = R.conv_case(n, h, w, cin, cout, 3, 1, 1, True, "normal", seed=700 + (n + 3 * h + 5 * w + 7 * cin + 11 * cout) % 100)
        plain = R.ConvCase(case.x, case.w, case.scale, case.shift, None, 1, 1, case.dist)
        z, S = R.conv_exact(plain)
        refs = {}
        for res, c in ((True, case), (False, plain)):
            c_ref = R.conv_ref(c, "wino").c_ref
            refs[res] = (z + case.residual.double(), S + case.residual.double().abs(), c_ref) if res else (z, S, c_ref)
        _CASES[shape] = (case, refs)
    return _CASES[shape]


def run_case(case, dev, res, relu):
    u = ops.wino43_transform_weights(case.w.to(dev))
    r = case.residual.to(dev) if res else None
    y = ops.conv3x3_wino43_bn_act_nhwc(case.x.to(dev), u, case.scale.to(dev), case.shift.to(dev), r, relu=relu)
    torch.cuda.synchronize()
    return y.cpu()


def sha(t):
    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()


def golden_key(route, res, relu):
    return f"{route}-res{int(res)}-relu{int(relu)}"


@pytest.fixture(scope="module")
def gold():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("route,shape", [pytest.param(r, s, id=f"{r}-{shape_id(s)}") for r, s in CASES])
def test_tail5_against_float64_and_the_parent(dev, gold, route, shape):
    case, refs = make_case(shape)
    g = gold[shape_id(shape)]
    assert sha(case.x) == g["x"] and sha(case.w) == g["w"], "the seeded operands differ from the golden's: nothing to compare"
    with ops.tuned(ROUTES[route]):
        for res in (True, False):
            z, S, c_ref = refs[res]
            assert c_ref > 0.0
            for relu in (True, False):
                y = run_case(case, dev, res, relu)
                c = R.c_of(y, z, S, relu=relu)
                print(f"{route} {shape} res={int(res)} relu={int(relu)}: c_ref {c_ref:.3f} c_hip {c:.3f} ratio {c / c_ref:.3f}")
                assert c <= M_KERNEL * c_ref, (route, shape, res, relu, c_ref, c)
                assert sha(y) == g[golden_key(route, res, relu)], (route, shape, res, relu)


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_executed_matrix_work_names_the_route(dev, shape):
    """One launch per route with the timers on: the executed FLOP are those of the route the shape must take -- 44 MFMAs per wave
    and K step where position 5 of the last tiles is dead, 48 everywhere else (W = 8, Tw = 4, the other tile order)."""
    case, _ = make_case(shape)
    want = expected_executed(shape)
    for route in ("wave8", "wave8_whole"):
        with ops.tuned(ROUTES[route]):
            ops.timing_enable(True)
            try:
                ops.timing_read()
                run_case(case, dev, True, True)
                got = ops.timing_read()["conv_wino"]
            finally:
                ops.timing_enable(False)
        print(f"{route} {shape}: executed {got['executed']:.6e} expected {want:.6e} launches {got['launches']}")
        assert got["launches"] == 1
        assert got["executed"] == want, (route, shape, got["executed"], want)
