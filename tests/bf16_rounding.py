"""Correct-rounding check for the bf16 kernels (test infrastructure; the cases are in test_bf16_rounding_cpu.py and
test_hip_bf16_rounding.py).

What a bf16 kernel of this project promises: bf16 x bf16 products are exact in fp32, the accumulation, the BatchNorm affine, the
residual add and the ReLU are fp32, and there is ONE rounding to bf16 (nearest even) at the store.  So an output element is the
correctly rounded exact answer, except where fp32 summation noise carries it across a rounding boundary.  The check states that
per element, with no tolerance chosen by hand:

    z      exact result in float64, BEFORE the ReLU and before the final rounding
    S      conditioning sum |scale| * sum_k |x_k| |w_k| + |shift| + |residual| (the same float64 pass on absolute values)
    u      2^-24
    delta  c * u * S                                           per element
    lo     bf16_rne(act(z - delta)),  hi = bf16_rne(act(z + delta))
    every element:  lo <= y_kernel <= hi                       (rounding, ReLU and max-pool are monotone)

c is not picked either: c_ref = max |y32 - z| / (u S) is measured on the CPU fp32 evaluation y32 of the same op on the same
operands (a measurement of the REFERENCE, never of the kernel), and c = 4 c_ref.  The factor 4 is the margin for the kernels'
different summation order (32x32x16 MFMA blocks, tap-major against chunk-major K walks, FMA contraction of v * sc + sh).
The share of elements with lo != hi (two acceptable answers) is capped at 2 %, so the check cannot go hollow.
"""
from dataclasses import dataclass
from typing import Callable, Optional

import torch
import torch.nn.functional as F

U = 2.0 ** -24
FACTOR = 4.0            # margin over the reference's own c_ref
AMBIGUOUS_CAP = 0.02    # largest share of elements that may have two acceptable answers


def bf16_rne(t: torch.Tensor) -> torch.Tensor:
    """Round to bf16, nearest even, as the project does (csrc/host_ops.hip round_one: (u + 0x7fff + ((u >> 16) & 1)) >> 16 on the
    fp32 bits; equal to Tensor.bfloat16() on finite values), returned as fp32.
    A float64 input is rounded to fp32 first.  That double rounding can differ from a direct float64 -> bf16 rounding only for
    values within 2^-24 relative of a bf16 tie; it is applied to the END POINTS z -+ delta of an interval whose half width
    delta >= c u S >= c 2^-24 |z| is larger than that, so it moves an end point by less than the interval's own slack: harmless
    at these magnitudes."""
    f = t.detach().to(torch.float32).contiguous()
    bits = f.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    rounded = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16) & 0xFFFF
    nan = ((bits >> 16) | 0x40) & 0xFFFF
    out = torch.where((bits & 0x7FFFFFFF) > 0x7F800000, nan, rounded) << 16
    out = torch.where(out >= 2 ** 31, out - 2 ** 32, out).to(torch.int32)
    return out.view(torch.float32).view(f.shape)


def bf16_trunc(t: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16 by dropping the low 16 bits (a planted defect for the CPU tests), as fp32."""
    f = t.detach().to(torch.float32).contiguous()
    return (f.view(torch.int32) & -65536).view(torch.float32).view(f.shape)


def bf16_ordinal(t: torch.Tensor) -> torch.Tensor:
    """Position of a bf16-representable value on the line of bf16 numbers (int64; -0 and +0 share 0): ulp distances."""
    b = t.detach().to(torch.float32).contiguous().view(torch.int32).to(torch.int64) >> 16
    return torch.where(b < 0, -(b & 0x7FFF), b).view(t.shape)


def bf16_step(t: torch.Tensor, ulps: int) -> torch.Tensor:
    """The bf16 value `ulps` steps up (down if negative) from the bf16-representable, positive, finite t (as fp32)."""
    b = (t.detach().to(torch.float32).contiguous().view(torch.int32).to(torch.int64) >> 16) + ulps
    return (b << 16).to(torch.int32).view(torch.float32).view(t.shape)


@dataclass
class Ref:
    """Float64 reference of one op, before ReLU and rounding: z exact, S conditioning sum, y32 the CPU fp32 evaluation."""
    z: torch.Tensor
    S: torch.Tensor
    y32: torch.Tensor

    @property
    def c_ref(self) -> float:
        return _ratio_max((self.y32.double() - self.z).abs(), self.S)

    def map(self, fn: Callable[[torch.Tensor], torch.Tensor]) -> "Ref":
        return Ref(fn(self.z), fn(self.S), fn(self.y32))


def _ratio_max(err: torch.Tensor, S: torch.Tensor) -> float:
    """max err / (u S); an element with S == 0 is exact by construction (every term is zero) and must have err == 0."""
    zero = S == 0
    if bool((err[zero] != 0).any()):
        return float("inf")
    return float((err / (U * S.masked_fill(zero, 1.0))).max())


def conv_ref(x_nchw: torch.Tensor, w_oihw: torch.Tensor, scale: Optional[torch.Tensor], shift: Optional[torch.Tensor],
             residual_nchw: Optional[torch.Tensor], stride: int, pad: int, nhwc: bool = True) -> Ref:
    """conv + BatchNorm affine (+ residual) on the given (already bf16-rounded) operands; tensors NHWC unless nhwc=False."""
    cout = w_oihw.shape[0]
    sc = torch.ones(cout) if scale is None else scale.detach().cpu().float()
    sh = torch.zeros(cout) if shift is None else shift.detach().cpu().float()
    x32, w32 = x_nchw.detach().cpu().float(), w_oihw.detach().cpu().float()
    x64, w64 = x32.double(), w32.double()
    v = lambda t: t.view(1, -1, 1, 1)
    z = F.conv2d(x64, w64, None, stride=stride, padding=pad) * v(sc.double()) + v(sh.double())
    S = F.conv2d(x64.abs(), w64.abs(), None, stride=stride, padding=pad) * v(sc.double().abs()) + v(sh.double().abs())
    y32 = F.conv2d(x32, w32, None, stride=stride, padding=pad) * v(sc) + v(sh)
    if residual_nchw is not None:
        r32 = residual_nchw.detach().cpu().float()
        z, S, y32 = z + r32.double(), S + r32.double().abs(), y32 + r32
    ref = Ref(z, S, y32)
    return ref.map(lambda t: t.permute(0, 2, 3, 1).contiguous()) if nhwc else ref


def linear_ref(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], residuals=()) -> Ref:
    """a @ w.T + bias + sum(residuals) on the given (already bf16-rounded) a / w; residuals: fp32 [m][n_out] (already gathered)."""
    a32, w32 = a.detach().cpu().float(), w.detach().cpu().float()
    z = a32.double() @ w32.double().t()
    S = a32.double().abs() @ w32.double().abs().t()
    y32 = F.linear(a32, w32, None if bias is None else bias.detach().cpu().float())
    if bias is not None:
        b = bias.detach().cpu().double()
        z, S = z + b, S + b.abs()
    for r in residuals:
        r32 = r.detach().cpu().float()
        z, S, y32 = z + r32.double(), S + r32.double().abs(), y32 + r32
    return Ref(z, S, y32)


def interval(ref: Ref, relu: bool, c: float, post: Optional[Callable] = None):
    """(lo, hi) as fp32 tensors of bf16 values; `post` is a monotone map applied after the activation and before the rounding
    (the stem's max-pool: it commutes with the rounding)."""
    delta = (c * U) * ref.S
    lo, hi = ref.z - delta, ref.z + delta
    if relu:
        lo, hi = lo.clamp_min(0.0), hi.clamp_min(0.0)
    if post is not None:
        lo, hi = post(lo), post(hi)
    return bf16_rne(lo), bf16_rne(hi)


def examine(y: torch.Tensor, ref: Ref, relu: bool, post: Optional[Callable] = None, factor: float = FACTOR,
            c_ref: Optional[float] = None) -> dict:
    """The interval check of a bf16 output y (any float dtype holding bf16 values, the reference's layout) as a report: number of
    elements, of violations, their first indices with values and ulp distance, c_ref, c, share of ambiguous elements."""
    c_ref = ref.c_ref if c_ref is None else c_ref
    c = factor * c_ref
    lo, hi = interval(ref, relu, c, post)
    yf = y.detach().cpu().float()
    if yf.shape != lo.shape:
        raise AssertionError(f"shape {tuple(yf.shape)} != reference {tuple(lo.shape)}")
    bad = ~((lo <= yf) & (yf <= hi))                      # (a NaN output violates)
    rep = {"n": yf.numel(), "bad": int(bad.sum()), "c_ref": c_ref, "c": c, "ambiguous": float((lo != hi).double().mean())}
    if rep["bad"]:
        idx = bad.nonzero()
        oy, ol, oh = bf16_ordinal(yf[bad]), bf16_ordinal(lo[bad]), bf16_ordinal(hi[bad])
        ulps = torch.maximum(ol - oy, oy - oh)
        rep["max_ulps"] = int(ulps.max())
        rep["first"] = [{"index": idx[i].tolist(), "y": float(yf[bad][i]), "lo": float(lo[bad][i]), "hi": float(hi[bad][i]),
                         "ulps": int(ulps[i])} for i in range(min(5, idx.shape[0]))]
    return rep


def check(y: torch.Tensor, ref: Ref, relu: bool, post: Optional[Callable] = None, factor: float = FACTOR,
          c_ref: Optional[float] = None, what: str = "") -> dict:
    """Raises AssertionError unless EVERY element of y lies in [lo, hi] and at most 2 % of the elements have lo != hi."""
    rep = examine(y, ref, relu, post, factor, c_ref)
    if rep["bad"]:
        raise AssertionError(f"{what}: {rep['bad']} of {rep['n']} outputs are outside the correct-rounding interval "
                             f"(c_ref {rep['c_ref']:.3f}, c {rep['c']:.3f}), up to {rep['max_ulps']} bf16 ulps off; first: {rep['first']}")
    if not rep["ambiguous"] <= AMBIGUOUS_CAP:
        raise AssertionError(f"{what}: {rep['ambiguous']:.4f} of the outputs have two acceptable values (cap {AMBIGUOUS_CAP}): "
                             f"the check is hollow here (c_ref {rep['c_ref']:.3f})")
    return rep


def check_f32(y: torch.Tensor, ref: Ref, relu: bool, factor: float = FACTOR, what: str = "") -> dict:
    """An fp32 output: |y - act(z)| <= delta on every element (|relu(a) - relu(b)| <= |a - b|).  Reports the kernel's own
    observed c = max |y - act(z)| / (u S): how much of the factor is used."""
    c_ref = ref.c_ref
    zt = ref.z.clamp_min(0.0) if relu else ref.z
    yd = y.detach().cpu().double()
    if yd.shape != zt.shape:
        raise AssertionError(f"shape {tuple(yd.shape)} != reference {tuple(zt.shape)}")
    err = (yd - zt).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    bad = err > (factor * c_ref * U) * ref.S
    rep = {"n": yd.numel(), "bad": int(bad.sum()), "c_ref": c_ref, "c": factor * c_ref, "c_observed": _ratio_max(err, ref.S)}
    if rep["bad"]:
        idx = bad.nonzero()
        raise AssertionError(f"{what}: {rep['bad']} of {rep['n']} fp32 outputs are further than c u S from the exact value "
                             f"(c_ref {c_ref:.3f}, c {rep['c']:.3f}, observed c {rep['c_observed']:.3f}); first: {idx[:5].tolist()}")
    return rep


def wide_scales(cout: int, seed: int, shift_scale: float = 0.1):
    """Per-channel BatchNorm scales spread over 2^-6 .. 2^6, about 20 % negative, and shifts scaled with them: channels that differ
    by four orders of magnitude in one tensor (a max-norm over the tensor sees only the largest)."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.exp2(torch.rand(cout, generator=g) * 12.0 - 6.0)
    sign = torch.where(torch.rand(cout, generator=g) < 0.2, -1.0, 1.0)
    shift = torch.randn(cout, generator=g) * shift_scale * mag
    return (mag * sign).float().contiguous(), shift.float().contiguous()


def unit_scales(cout: int, seed: int, shift_scale: float = 0.1):
    """The distribution of the older bf16 tests: scale in [0.5, 1.5), shift ~ N(0, shift_scale^2)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(cout, generator=g) + 0.5).contiguous(), (torch.randn(cout, generator=g) * shift_scale).contiguous()


# ----------------------------------------------------------------------------------------------------------------------------------
# Encoder level: a CPU restatement of rpg_resnet_forward_bf16 with ITS rounding points, in float64 (E64) or float32 (E32) arithmetic
# ----------------------------------------------------------------------------------------------------------------------------------
def emulate_encoder_bf16(tensors, blocks, planes, x_nchw: torch.Tensor, dtype: torch.dtype, trace: Optional[list] = None) -> torch.Tensor:
    """The bf16 encoder (csrc/conv_bf16.hip resnet_forward_bf16_impl) on the CPU, arithmetic in `dtype` (float64: E64, float32:
    E32), from the packed tensors of params.pack_resnet_bf16 (bf16 weights, fp32 folded BatchNorm scale / shift).  Rounding
    points, read off the code:
      1. the fp32 image is rounded to bf16 (stem kernel / re-layout pass);
      2. stem: conv 7x7/2 (bf16 weights, Cin padded with zeros) -> scale, shift -> ReLU -> max-pool 3x3/2 pad 1 -> ONE rounding
         to bf16 (the fused kernel pools the fp32 values; the three-kernel stem rounds, then pools bf16: the same, max-pool
         commutes with the rounding);
      3. every BasicBlock: conv1 -> scale, shift -> ReLU -> bf16;  where the block down-samples, conv 1x1 -> scale, shift -> bf16
         (no ReLU);  conv2 -> scale, shift -> + identity (bf16 values, added in fp32) -> ReLU -> bf16;
      4. global average pool: sum over the pixels, divided by their number, -> bf16;
      5. fc: bf16 pooled features x bf16 weights + fp32 bias, NOT rounded (fp32 output).
    Nothing else is rounded to bf16; everything between two rounding points is computed in `dtype`.
    trace (optional list): receives one dict per convolution -- name, input x (NCHW, bf16 values as float32), weight (OIHW), scale,
    shift, residual (or None), stride, pad, relu -- so that a layer can be re-run on exactly this input; and a last one for the fc
    (name "fc", x the pooled bf16 features, w [feat][C], bias)."""
    t = [v.detach().cpu() for v in tensors]
    rnd = lambda v: bf16_rne(v).to(dtype)
    v4 = lambda s: s.to(dtype).view(1, -1, 1, 1)

    def conv(name, x, i, stride, pad, relu, residual=None, k=None):
        w = t[i].float().permute(0, 3, 1, 2).contiguous()              # OHWI -> OIHW
        if trace is not None:
            trace.append({"name": name, "x": x.float(), "w": w, "scale": t[i + 1], "shift": t[i + 2],
                          "residual": None if residual is None else residual.float(), "stride": stride, "pad": pad, "relu": relu})
        y = F.conv2d(x, w.to(dtype), None, stride=stride, padding=pad) * v4(t[i + 1]) + v4(t[i + 2])
        if residual is not None:
            y = y + residual
        return F.relu(y) if relu else y

    x = rnd(x_nchw.detach().cpu().float())
    x = F.pad(x, (0, 0, 0, 0, 0, 5))                                   # Cin 3 -> 8 (zero channels, like the packed stem weight)
    y = conv("stem", x, 0, 2, 3, True)
    x = rnd(F.max_pool2d(y, 3, 2, 1))
    ti, cin = 3, planes[0]
    for l in range(4):
        for b in range(blocks[l]):
            stride = 2 if (l > 0 and b == 0) else 1
            c = planes[l]
            ds = stride != 1 or cin != c
            name = f"layer{l + 1}.{b}"
            tmid = rnd(conv(name + ".conv1", x, ti, stride, 1, True))
            identity = rnd(conv(name + ".downsample", x, ti + 6, stride, 0, False)) if ds else x
            x = rnd(conv(name + ".conv2", tmid, ti + 3, 1, 1, True, identity))
            ti += 9 if ds else 6
            cin = c
    hw = x.shape[2] * x.shape[3]
    pooled = rnd(x.sum(dim=(2, 3)) / hw)
    if trace is not None:
        trace.append({"name": "fc", "x": pooled.float(), "w": t[ti].float(), "bias": t[ti + 1]})
    return pooled @ t[ti].to(dtype).t() + t[ti + 1].to(dtype)


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / b.norm().clamp(min=1e-300))
