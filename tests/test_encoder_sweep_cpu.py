"""Host-only tests of tests/encoder_sweep_ref.py, the yardstick of tests/test_hip_encoder_sweep.py: the Winograd statement is the
convolution, the check catches each planted defect and passes the unmodified fp32 statement, the memory harness sees a stray
store, an unwritten element and a load outside the image, and the GPU module's case lists reach what they name and keep the
ReLU from hollowing the check out.  Nothing here needs a GPU."""
import pytest
import torch

import encoder_sweep_ref as R

CUS = 256        # compute units of an MI355X; the GPU module asks the device


@pytest.mark.parametrize("h", [1, 2, 3, 5])
@pytest.mark.parametrize("w", [1, 2, 3, 4, 5, 6, 7, 8, 9, 13])
def test_winograd_statement_in_float64_is_the_convolution(h, w):
    """Every W mod 4, W < 4 and H = 1: the float64 form of the statement against F.conv2d in float64 to 1e-12."""
    case = R.conv_case(3, h, w, 20, 12, 3, 1, 1, True, "normal", seed=10 * h + w)
    got, ref = R.conv_wino(case, torch.float64), R.conv_direct(case, torch.float64)
    assert got.shape == ref.shape
    assert float((got - ref).abs().max() / ref.abs().max()) < 1e-12


def test_weight_transform_is_rounded_once():
    w = torch.randn(8, 3, 3, 4, generator=torch.Generator().manual_seed(1))
    u64, u32 = R.wino43_weights(w, torch.float64), R.wino43_weights(w, torch.float32)
    assert u32.dtype == torch.float32 and torch.equal(u32, u64.float()) and not torch.equal(u32.double(), u64)


@pytest.mark.parametrize("dist", R.DISTS)
@pytest.mark.parametrize("cin", [16, 64, 160])
def test_c_ref_of_the_fp32_statements(cin, dist):
    """The figures the margins multiply, printed: c_ref of the fp32 Winograd statement and of F.conv2d in fp32, over 2^16 outputs.
    The fp32 statements pass their own check at the starting margin, and the max-norm error they make is two orders below 2e-5."""
    case = R.conv_case(4, 7, 9, cin, 64, 3, 1, 1, True, dist, seed=cin)
    for kind in ("wino", "direct"):
        ref = R.conv_ref(case, kind)
        fp32 = (R.conv_wino if kind == "wino" else R.conv_direct)(case, torch.float32)
        c = R.c_of(fp32, ref.z, ref.S)
        print(f"c_ref[{kind}, Cin {cin}, {dist}] = {ref.c_ref:.3f} over {ref.ref_elems} elements (the case alone: {c:.3f})")
        assert ref.ref_elems >= R.MIN_REF_ELEMS and 0.0 < c <= ref.c_ref
        # N(0, 1): a few units.  "act": the 1e3 channel makes a Winograd tile's error that of its LARGEST pixels, while S is the
        # element's own 3 x 3 window -- hundreds of units where the window holds clamped zeros: the algorithm's own figure,
        # which is why the bar is a multiple of c_ref and not a constant
        assert ref.c_ref < (16.0 if dist == "normal" else 4096.0)
        assert R.c_of(torch.relu(fp32), ref.z, ref.S, relu=True) <= ref.c_ref
        assert float((fp32.double() - ref.z).abs().max() / ref.z.abs().max()) < 2e-6


def _shift_heavy_case():
    """A case whose outputs are dominated by one term (a BatchNorm shift of +-30 on K = 36 small products): |z| ~ S, so an error
    of a few ulps of the OUTPUT is an error of a few u S."""
    case = R.conv_case(40, 5, 9, 4, 64, 3, 1, 1, False, "normal", seed=77)
    case.shift = torch.where(case.shift < 0, -30.0, 30.0) + case.shift
    return case


def test_planted_arithmetic_defects_are_caught():
    """Each defect of the list fails c <= M c_ref; the unmodified fp32 statement passes, with and without ReLU."""
    for w in (7, 8):
        case = R.conv_case(6, 3, w, 20, 12, 3, 1, 1, True, "act", seed=5 + w)
        ref = R.conv_ref(case, "wino")
        bar = R.M_START * ref.c_ref
        good = R.conv_wino(case)
        assert R.c_of(good, ref.z, ref.S) <= bar and R.c_of(torch.relu(good), ref.z, ref.S, relu=True) <= bar
        for defect in R.WINO_DEFECTS:
            bad = R.conv_wino(case, defect=defect)
            assert R.c_of(bad, ref.z, ref.S) > bar, (w, defect)
            assert R.c_of(torch.relu(bad), ref.z, ref.S, relu=True) > bar, (w, defect, "relu")
    case = _shift_heavy_case()
    ref = R.conv_ref(case, "wino")
    good = R.conv_wino(case)
    c_good, c_bad = R.c_of(good, ref.z, ref.S), R.c_of(R.clear_low_bits(good, 3), ref.z, ref.S)
    print(f"three low bits cleared: c {c_good:.3f} -> {c_bad:.3f}, bar {R.M_START * ref.c_ref:.3f}")
    assert c_good <= R.M_START * ref.c_ref < c_bad
    assert R.c_of(torch.relu(R.clear_low_bits(good, 3)), ref.z, ref.S, relu=True) > R.M_START * ref.c_ref


def test_relu_check_per_element():
    z, S = torch.tensor([1.0, -1.0, 1e-9, -1e-9, 2.0]).double(), torch.ones(5).double()
    y = torch.tensor([1.0, 0.0, 0.0, 1e-9, -0.5])
    c = R.c_elements(y, z, S, relu=True)
    assert c[0] == 0 and c[1] == 0 and c[4] == float("inf")
    assert abs(float(c[2]) - 1e-9 / R.U) < 1e-6 and abs(float(c[3]) - 2e-9 / R.U) < 1e-6
    assert R.c_of(torch.tensor([float("nan")]), z[:1], S[:1]) == float("inf")
    assert R.c_of(torch.tensor([1e-30]), torch.zeros(1).double(), torch.zeros(1).double()) == float("inf")


def test_stem_bound_through_relu_and_maxpool():
    x, wt, scale, shift = R.stem_operands(7, 9)
    z, S = R.stem_exact(x, wt, scale, shift)
    y32 = R.stem_fp32(x, wt, scale, shift)
    c_ref = R.c_of(y32, z, S)
    c = R.c_post(R.stem_post(y32), z, S, R.stem_post)
    assert 0.0 < c <= 1.02 * c_ref
    bad = R.stem_post(y32).clone()
    bad[0, 0, 0, 5] += 1e-3
    assert R.c_post(bad, z, S, R.stem_post, c_max=R.M_START * c_ref) == float("inf")


def test_avgpool_statement():
    x = R.activations((5, 49, 8), "act", 3)
    z, S = R.avgpool_exact(x)
    assert R.c_of(R.avgpool_ordered(x), z, S) < 49.0
    assert float((R.avgpool_ordered(x.double()) - z).abs().max()) < 1e-12 * float(z.abs().max())


def test_memory_harness_catches_a_stray_store_an_unwritten_element_and_a_load_outside():
    dev = torch.device("cpu")
    case = R.conv_case(2, 3, 5, 8, 4, 3, 1, 1, False, "normal", seed=1)
    xb = R.Moated(case.x.shape, dev, case.x)
    out = R.Moated((2, 3, 5, 4), dev)
    assert out.moat * 4 >= 64 * 1024 and out.moat >= 4 * 5 * 4 and out.ptr() % 16 == 0 and out.moat % 64 == 0
    assert R.moat_words((1, 129, 131, 512)) >= 4 * 131 * 512
    assert R.harness_findings([xb], out) == ["40 output elements were never written".replace("40", str(out.numel)), "the output is not finite"]
    out.t.copy_(R.conv_wino(case))
    assert R.harness_findings([xb], out) == []
    out.raw[out.moat + out.numel + 3] = 0                                  # one word of the moat behind y
    assert R.harness_findings([xb], out) == ["the output's moat was written"]
    out.raw[out.moat + out.numel + 3] = R.PAYLOAD_BITS
    out.raw[out.moat - 1] = 0                                              # ... and in front of it
    assert R.harness_findings([xb], out) == ["the output's moat was written"]
    out.raw[out.moat - 1] = R.PAYLOAD_BITS
    out.raw[out.moat + 17] = R.PAYLOAD_BITS                                # one element left unwritten
    assert R.harness_findings([xb], out) == ["1 output elements were never written", "the output is not finite"]
    out.t.copy_(R.conv_wino(case, first_left_tap=xb.words_before(8)))      # a padding tap reads the moat in front of x
    assert R.harness_findings([xb], out) == ["the output is not finite"]
    xb.raw[3] = 0
    assert R.harness_findings([xb], out)[0] == "the moat of input 0 was written"


@pytest.mark.parametrize("route", list(R.ROUTES))
def test_routes_reach_what_their_cases_name(route):
    """On the reference alone: the launcher's rule, restated, sends every (route, shape) where the case list means it to go; every
    route has cases at H <= 3 and at W < 4; the persistent list has H = 1 shapes, and they fall back."""
    cases = R.wino_cases(route)
    assert len(cases) >= 20
    taken = [R.wino_taken(R.ROUTES[route], *s[:5], CUS) for s in cases]
    assert taken == [R.wino_expected(route, s, CUS) for s in cases]
    head = {"wave4": "wave4", "wave8_whole": "wave8_whole", "split_launch": "wave8_split_launch", "split_inkernel8": "wave8_split_inkernel",
            "split_inkernel32": "wave8_split_inkernel", "persist_whole": "persist_whole", "persist_split": "persist_split"}[route]
    own = [s for s, t in zip(cases, taken) if t.split(":")[0] == head]
    assert any(s[1] <= 3 for s in own) and any(s[2] < 4 for s in own) and any(s[1] <= 3 and s[2] < 4 for s in own)
    if route == "split_inkernel8":
        assert any(t == "wave8_split_launch:10" for t in taken)            # above the combine limit of 8: the fix-up launch
    if route == "split_inkernel32":
        assert any(t == "wave8_split_inkernel:10" for t in taken)
    if route.startswith("persist"):
        assert all(s[3] % 16 == 0 for s in cases)
        assert all((s[1] == 1) == (not t.startswith("persist")) for s, t in zip(cases, taken)) and any(s[1] == 1 for s in cases)
        for want in ([lambda s: s[1] in (2, 3), lambda s: s[2] < 4, lambda s: s[4] % 64 != 0, lambda s: (s[0] * s[1] * ((s[2] + 3) // 4)) % 128 != 0]):
            assert any(want(s) for s in own)


def test_case_lists_cover_the_edges():
    sh = R.WINO_SHAPES
    assert {s[2] for s in sh} == {1, 2, 3, 4, 5, 7, 8, 9} and {s[1] for s in sh} == {1, 2, 3, 5}
    assert {s[3] for s in sh} == {4, 12, 16, 20, 32, 48, 160} and {s[4] for s in sh} == {4, 60, 64, 68, 132}
    tiles = {s[0] * s[1] * ((s[2] + 3) // 4) for s in sh}
    assert {31, 32, 33, 63, 64, 65, 127, 128, 129} <= tiles and {62, 66, 126, 130} <= tiles
    assert {(s[5], s[6]) for s in sh} == {(False, "normal"), (True, "normal"), (False, "act"), (True, "act")}
    assert len(set(map(R.wino_shape_id, sh))) == len(sh)


@pytest.mark.parametrize("shape", R.WINO_SHAPES, ids=R.wino_shape_id)
def test_relu_clamps_at_most_60_percent_wino(shape):
    n, h, w, cin, cout, res, dist = shape
    z, _ = R.conv_exact(R.conv_case(n, h, w, cin, cout, 3, 1, 1, res, dist, seed=R.WINO_SHAPES.index(shape)))
    assert R.clamped_share(z) <= R.CLAMP_CAP, R.clamped_share(z)


def test_relu_clamps_at_most_60_percent_direct_and_stem():
    for kind, spec in R.DIRECT_KINDS.items():
        for extent in R.DIRECT_EXTENTS:
            if spec[5]:
                z, _ = R.conv_exact(R.direct_case(kind, extent))
                assert R.clamped_share(z) <= R.CLAMP_CAP, (kind, extent, R.clamped_share(z))
    assert {e[0] for e in R.DIRECT_EXTENTS} | {e[1] for e in R.DIRECT_EXTENTS} >= {1, 2, 7, 13, 14}
    for h, w in R.STEM_SIZES:
        z, _ = R.stem_exact(*R.stem_operands(h, w))
        pooled = R.stem_post(z)
        assert float((pooled <= 0).double().mean()) <= R.CLAMP_CAP, (h, w)


def test_the_route_models_constants_are_the_librarys_defaults():
    """wino_taken's four constants (encoder_sweep_ref.WINO_MODEL_DEFAULTS) against the library's own defaults (no GPU needed)."""
    from relpose_gnn_amd import ops
    for name, value in R.WINO_MODEL_DEFAULTS.items():
        assert ops.tuning_default(name) == value, name


def test_composite_plan_mixes_the_routes():
    """33 x 47, n = 48, by the rule: layers 1, 2 and 4 take Winograd (21, 16, 16 units), layer 3 does not (12); one image never does."""
    assert R.layer_extents(33, 47) == [(9, 12), (5, 6), (3, 3), (2, 2)]
    assert R.layer_extents(17, 17) == [(5, 5), (3, 3), (2, 2), (1, 1)]
    assert R.layer_plan(48, 33, 47) == [(True, 21), (True, 16), (False, 12), (True, 16)]
    for n, h, w in R.FWD_CASES:
        took = [t for t, _ in R.layer_plan(n, h, w)]
        assert (any(took) and not all(took)) if n > 1 else not any(took), (n, h, w, R.layer_plan(n, h, w))


def test_encoder_statements_agree():
    """The CPU module in float64 with and without the Winograd statement: the same network."""
    m = R.encoder_module()
    x = torch.randn(2, 3, 33, 47, generator=torch.Generator().manual_seed(4))
    a, b = R.encoder_forward(m, x, torch.float64), R.encoder_forward(m, x, torch.float64, wino=True)
    assert a.shape == (2, R.FWD_FEAT) and float((a - b).abs().max() / a.abs().max()) < 1e-12
    e32 = float((R.encoder_forward(m, x, torch.float32).double() - a).abs().max() / a.abs().max())
    assert 0.0 < e32 < 1e-5
