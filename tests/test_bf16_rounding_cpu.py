"""The correct-rounding check of tests/bf16_rounding.py has teeth, shown without a GPU: the CPU fp32 result rounded correctly
passes it; the three epilogue defects that the 1e-2 max-norm bar of the older bf16 tests lets through (store truncates, BatchNorm
scale rounded to bf16, double rounding around the residual add) fail it on a large share of the elements; and so does a single
element one bf16 ulp off in a low-magnitude channel, which no max-norm over the tensor can see."""
import pytest
import torch
import torch.nn.functional as F

import bf16_rounding as R

# n, h, w, cin, cout, k, stride, pad : a strided layer-2-like shape, a ragged one, the fc-like 1x1
SHAPES = [(2, 14, 14, 64, 128, 3, 2, 1), (3, 13, 17, 192, 72, 3, 2, 1), (37, 1, 1, 512, 256, 1, 1, 0)]
_cache = {}


def _case(shape, wide):
    key = (shape, wide)
    if key not in _cache:
        n, h, w, cin, cout, k, stride, pad = shape
        g = torch.Generator().manual_seed(100 + cin + cout)
        x = torch.randn((n, cin, h, w), generator=g).bfloat16()
        wt = (torch.randn((cout, cin, k, k), generator=g) * (2.0 / (cin * k * k)) ** 0.5).bfloat16()
        scale, shift = (R.wide_scales if wide else R.unit_scales)(cout, 7)
        ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        res = torch.randn((n, cout, ho, wo), generator=g).bfloat16()
        acc32 = F.conv2d(x.float(), wt.float(), None, stride=stride, padding=pad).permute(0, 2, 3, 1).contiguous()
        _cache[key] = (R.conv_ref(x, wt, scale, shift, res, stride, pad), R.conv_ref(x, wt, scale, shift, None, stride, pad),
                       acc32, scale, shift, res.float().permute(0, 2, 3, 1).contiguous())
    return _cache[key]


def test_bf16_rne_is_the_projects_rounding():
    g = torch.Generator().manual_seed(1)
    v = torch.randn(100000, generator=g) * torch.exp2(torch.randint(-60, 60, (100000,), generator=g).float())
    ties = torch.tensor([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x00008000, 0x00018000, 0x7F7FFFFF, 0x80000000, 0x00000001],
                        dtype=torch.int64)
    ties = torch.where(ties >= 2 ** 31, ties - 2 ** 32, ties).to(torch.int32).view(torch.float32)
    v = torch.cat([v, ties])
    got = R.bf16_rne(v)
    assert torch.equal(got.view(torch.int32), v.bfloat16().float().view(torch.int32))
    assert torch.equal(R.bf16_ordinal(R.bf16_step(got[:5].abs(), 3)) - R.bf16_ordinal(got[:5].abs()), torch.full((5,), 3))


@pytest.mark.parametrize("wide", [False, True], ids=["unit_scales", "wide_scales"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
def test_correctly_rounded_fp32_reference_passes(shape, wide, relu):
    """(a) bf16_rne(act(y32)) of the CPU fp32 evaluation is inside the interval at c = 4 c_ref everywhere (it is inside at
    c = c_ref by the definition of c_ref), with and without the residual, and the ambiguous share stays under the 2 % cap."""
    for ref in _case(shape, wide)[:2]:
        y = R.bf16_rne(F.relu(ref.y32) if relu else ref.y32)
        rep = R.check(y, ref, relu, what=str(shape))
        assert rep["bad"] == 0 and rep["ambiguous"] <= R.AMBIGUOUS_CAP
        assert 0.1 < rep["c_ref"] < 8.0, rep                    # the reference's own noise is of the order of u S
        rep32 = R.check_f32(F.relu(ref.y32) if relu else ref.y32, ref, relu)
        assert rep32["c_observed"] <= rep32["c_ref"] * (1 + 1e-12)


@pytest.mark.parametrize("wide", [False, True], ids=["unit_scales", "wide_scales"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("defect", ["truncating_store", "bf16_scale", "double_rounding"])
def test_planted_epilogue_defects_fail(shape, wide, defect):
    """(b) each defect, built on the CPU from the fp32 accumulators, violates the interval on at least 5 % of the elements
    (and passes the old bar: max-norm error under 1e-2, where that bar is meaningful -- one magnitude in every channel)."""
    ref, _, acc32, scale, shift, res = _case(shape, wide)
    if defect == "truncating_store":
        y = R.bf16_trunc(F.relu(acc32 * scale + shift + res))
    elif defect == "bf16_scale":
        y = R.bf16_rne(F.relu(acc32 * R.bf16_rne(scale) + shift + res))
    else:
        y = R.bf16_rne(F.relu(R.bf16_rne(acc32 * scale + shift) + res))
    rep = R.examine(y, ref, True)
    assert rep["bad"] >= 0.05 * rep["n"], rep
    with pytest.raises(AssertionError, match="outside the correct-rounding interval"):
        R.check(y, ref, True)
    if not wide:
        want = F.relu(ref.y32)
        assert float((y - want).abs().max() / want.abs().max()) < 1e-2


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_one_ulp_in_a_low_magnitude_channel_fails(shape):
    """(c) one element of the channel with the smallest |scale| (no residual: its values are four orders of magnitude below the
    tensor's maximum) moved by one bf16 ulp: the max-norm error of the tensor stays at the rounding level, the check fails with
    exactly one violation."""
    _, ref, _, scale, _, _ = _case(shape, True)
    y = R.bf16_rne(ref.y32)
    lo, hi = R.interval(ref, False, R.FACTOR * ref.c_ref)
    ch = int(scale.abs().argmin())
    sure = ((lo == hi) & (y > 0))[..., ch].nonzero()                       # an element with ONE acceptable answer
    assert sure.shape[0] > 0
    i = tuple(sure[0].tolist()) + (ch,)
    assert R.examine(y, ref, False)["bad"] == 0
    before = float((y - ref.y32).abs().max() / ref.y32.abs().max())
    y[i] = R.bf16_step(y[i], 1)
    after = float((y - ref.y32).abs().max() / ref.y32.abs().max())
    assert after == before and after < 1e-2                               # invisible to the max-norm
    rep = R.examine(y, ref, False)
    assert rep["bad"] == 1 and rep["first"][0]["index"] == list(i) and rep["first"][0]["ulps"] == 1, rep
    with pytest.raises(AssertionError):
        R.check(y, ref, False)


def test_linear_reference_and_fp32_check():
    """linear_ref + check_f32: the CPU fp32 Linear with two gathered fp32 residuals is within its own c_ref; one output moved by
    8 c_ref u S is reported."""
    g = torch.Generator().manual_seed(5)
    a, w = torch.randn((130, 256), generator=g).bfloat16(), (torch.randn((72, 256), generator=g) / 16).bfloat16()
    bias, table = torch.randn(72, generator=g), torch.randn((50, 3 * 72), generator=g)
    i1, i2 = torch.randint(0, 50, (130,), generator=g), torch.randint(0, 50, (130,), generator=g)
    ref = R.linear_ref(a, w, bias, (table[i1, :72], table[i2, 72:144]))
    y = F.relu(ref.y32)
    rep = R.check_f32(y, ref, True)
    assert rep["bad"] == 0 and rep["c_observed"] <= rep["c_ref"]
    j = (ref.z > 1.0).nonzero()[0]
    y[j[0], j[1]] += float(8 * rep["c_ref"] * R.U * ref.S[j[0], j[1]])
    with pytest.raises(AssertionError, match="further than c u S"):
        R.check_f32(y, ref, True)


def test_encoder_emulation_matches_plain_fp32_model_loosely_and_is_deterministic():
    """emulate_encoder_bf16 on a tiny ResNet table: E32 and E64 agree to bf16-flip level (not bit level), the run is
    deterministic, and the trace lists every convolution and the fc with the bf16 input it saw."""
    g = torch.Generator().manual_seed(3)
    blocks, planes = [1, 1, 1, 1], [64, 64, 128, 128]
    rn = lambda *s, k=1.0: torch.randn(*s, generator=g) * k
    aff = lambda c: [torch.rand(c, generator=g) + 0.5, rn(c, k=0.1)]
    t = [F.pad(rn(64, 7, 7, 3, k=(2 / 147) ** 0.5), (0, 5)).bfloat16(), *aff(64)]
    cin = 64
    for l, c in enumerate(planes):
        ds = l > 0
        t += [rn(c, 3, 3, cin, k=(2 / (9 * cin)) ** 0.5).bfloat16(), *aff(c), rn(c, 3, 3, c, k=(1 / (9 * c)) ** 0.5).bfloat16(), *aff(c)]
        if ds:
            t += [rn(c, 1, 1, cin, k=(1 / cin) ** 0.5).bfloat16(), *aff(c)]
        cin = c
    t += [rn(32, cin, k=cin ** -0.5).bfloat16(), rn(32)]
    x = rn(2, 3, 64, 48)
    trace = []
    e64 = R.emulate_encoder_bf16(t, blocks, planes, x, torch.float64, trace)
    e32 = R.emulate_encoder_bf16(t, blocks, planes, x, torch.float32)
    assert e64.dtype == torch.float64 and e32.dtype == torch.float32 and e64.shape == (2, 32)
    assert [d["name"] for d in trace] == ["stem", "layer1.0.conv1", "layer1.0.conv2", "layer2.0.conv1", "layer2.0.downsample",
                                          "layer2.0.conv2", "layer3.0.conv1", "layer3.0.downsample", "layer3.0.conv2",
                                          "layer4.0.conv1", "layer4.0.downsample", "layer4.0.conv2", "fc"]
    assert all(torch.equal(d["x"], d["x"].bfloat16().float()) for d in trace)       # every layer input is a bf16 tensor
    assert R.rel_l2(e32, e64) < 2e-2
    assert torch.equal(e64, R.emulate_encoder_bf16(t, blocks, planes, x, torch.float64))
