"""Helpers shared by tests/test_hip_encoder_sweep.py (GPU) and tests/test_encoder_sweep_cpu.py: float64 statements of the fp32
encoder's operations with their conditioning sums, an fp32 CPU statement of the 1-D Winograd F(4,3) algorithm of csrc/winograd.hip,
the element-wise check, the launcher's route rule restated, the case lists, and a memory harness that puts every operand between
two moats inside one allocation.  Test helper (like bf16_rounding.py and graph_sweep_ref.py): no test lives here, and nothing here
needs a GPU.

The element-wise rule (the fp32 counterpart of bf16_rounding.py):

    z      exact result in float64, BEFORE the activation
    S      the same pass on absolute values: |scale| * sum |x| |w| + |shift| + |residual|
    u      2^-24
    c(y)   max over the elements of |y - z| / (u S)
    with an activation:  act(z - delta) <= y <= act(z + delta),  delta = c u S   (ReLU and max-pool are monotone)

c_ref is c of the CPU fp32 statement of the SAME algorithm (the Winograd statement below for the Winograd routes, F.conv2d in fp32
for the direct ones) over at least 2^16 output elements -- a small case gets extra images, for the reference only, because the
maximum over a 3 x 3 map is a much smaller number than the maximum over a 14 x 14 one of the same kind.  It is never measured on
a kernel.  A kernel passes with c_hip <= M c_ref.
"""
import math
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

U = 2.0 ** -24
M_START = 4.0                # where the kernel margin starts (bf16_rounding.FACTOR, for the same reason); ceiling 8
M_FWD_START = 2.0            # where the composite margin starts (as in the graph sweep); ceiling 4
MIN_REF_ELEMS = 1 << 16      # c_ref is a maximum over at least this many output elements
CLAMP_CAP = 0.60             # largest share of outputs that ReLU may clamp to zero in a case
DISTS = ("normal", "act")


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


# ----------------------------------------------------------------------------------------------------------------------
# operands
# ----------------------------------------------------------------------------------------------------------------------
def activations(shape: Sequence[int], dist: str, seed: int) -> torch.Tensor:
    """fp32 NHWC values.  "normal": N(0, 1).  "act": what every encoder convolution but the first reads -- relu(N(0.5, 1)),
    non-negative with a non-zero mean, and one channel (index 1 mod C) times 1e3, the outlier."""
    x = torch.randn(tuple(shape), generator=_gen(seed))
    if dist == "act":
        x = torch.relu(x + 0.5)
        x[..., 1 % shape[-1]] *= 1e3
    else:
        assert dist == "normal"
    return x.contiguous()


@dataclass
class ConvCase:
    """Operands of y = act(conv(x, w) * scale + shift (+ residual)) in the project's layouts: x, residual NHWC, w OHWI."""
    x: torch.Tensor
    w: torch.Tensor
    scale: torch.Tensor
    shift: torch.Tensor
    residual: Optional[torch.Tensor]
    stride: int
    pad: int
    dist: str = "normal"

    def out_hw(self) -> Tuple[int, int]:
        k_h, k_w = self.w.shape[1], self.w.shape[2]
        return ((self.x.shape[1] + 2 * self.pad - k_h) // self.stride + 1, (self.x.shape[2] + 2 * self.pad - k_w) // self.stride + 1)


def conv_case(n: int, h: int, w: int, cin: int, cout: int, k: int, stride: int, pad: int, res: bool, dist: str, seed: int) -> ConvCase:
    """Seeded operands: He-scaled weights, BatchNorm scales in +-[0.5, 1.5) (a fifth negative), shifts ~ N(0, 0.3^2), a residual of
    the input's distribution."""
    g = _gen(seed + 1)
    wt = (torch.randn(cout, k, k, cin, generator=g) * (2.0 / (cin * k * k)) ** 0.5).contiguous()
    scale = ((torch.rand(cout, generator=g) + 0.5) * torch.where(torch.rand(cout, generator=g) < 0.2, -1.0, 1.0)).contiguous()
    shift = (torch.randn(cout, generator=g) * 0.3).contiguous()
    case = ConvCase(activations((n, h, w, cin), dist, seed), wt, scale, shift, None, stride, pad, dist)
    if res:
        case.residual = activations((n, *case.out_hw(), cout), dist, seed + 2)
    return case


def more_images(case: ConvCase, n: int, seed: int) -> ConvCase:
    """The same convolution on n fresh images of the same distribution (the reference's extra samples)."""
    dist = case.dist
    _, h, w, cin = case.x.shape
    x = activations((n, h, w, cin), dist, seed)
    r = None if case.residual is None else activations((n, *case.residual.shape[1:]), dist, seed + 2)
    return ConvCase(x, case.w, case.scale, case.shift, r, case.stride, case.pad, dist)


# ----------------------------------------------------------------------------------------------------------------------
# float64 statements
# ----------------------------------------------------------------------------------------------------------------------
def _nchw(t: torch.Tensor) -> torch.Tensor:
    return t.permute(0, 3, 1, 2)


def _nhwc(t: torch.Tensor) -> torch.Tensor:
    return t.permute(0, 2, 3, 1).contiguous()


def conv_direct(case: ConvCase, dtype: torch.dtype) -> torch.Tensor:
    """conv + affine + residual before the activation with torch's convolution in ``dtype`` (NHWC): float64 is z, float32 the CPU
    fp32 statement of the direct routes."""
    y = F.conv2d(_nchw(case.x).to(dtype), _nchw(case.w).to(dtype), None, stride=case.stride, padding=case.pad)
    y = _nhwc(y) * case.scale.to(dtype) + case.shift.to(dtype)
    return y if case.residual is None else y + case.residual.to(dtype)


def conv_exact(case: ConvCase) -> Tuple[torch.Tensor, torch.Tensor]:
    """(z, S) in float64, NHWC, before the activation."""
    z = conv_direct(case, torch.float64)
    s = F.conv2d(_nchw(case.x).double().abs(), _nchw(case.w).double().abs(), None, stride=case.stride, padding=case.pad)
    s = _nhwc(s) * case.scale.double().abs() + case.shift.double().abs()
    return z, (s if case.residual is None else s + case.residual.double().abs())


def stem_exact(x_nchw: torch.Tensor, wt: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(z, S) of conv 7x7 / 2 / pad 3 + BatchNorm affine in float64, NCHW, before ReLU and max-pool."""
    v = lambda t: t.double().view(1, -1, 1, 1)
    z = F.conv2d(x_nchw.double(), wt.double(), None, stride=2, padding=3) * v(scale) + v(shift)
    s = F.conv2d(x_nchw.double().abs(), wt.double().abs(), None, stride=2, padding=3) * v(scale).abs() + v(shift).abs()
    return z, s


def stem_fp32(x_nchw: torch.Tensor, wt: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor) -> torch.Tensor:
    v = lambda t: t.view(1, -1, 1, 1)
    return F.conv2d(x_nchw, wt, None, stride=2, padding=3) * v(scale) + v(shift)


def stem_post(t: torch.Tensor) -> torch.Tensor:
    """ReLU + MaxPool2d(3, 2, 1) of an NCHW tensor, returned NHWC: the monotone map behind the stem's convolution."""
    return _nhwc(F.max_pool2d(torch.relu(t), 3, 2, 1))


def avgpool_exact(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """x [n][hw][c] -> (z, S) = (mean x, mean |x|) in float64."""
    return x.double().mean(1), x.double().abs().mean(1)


def avgpool_ordered(x: torch.Tensor) -> torch.Tensor:
    """global_avgpool_kernel's stated order in x's dtype: the pixels added in ascending order from zero, one division by hw."""
    acc = torch.zeros((x.shape[0], x.shape[2]), dtype=x.dtype)
    for q in range(x.shape[1]):
        acc = acc + x[:, q]
    return acc / float(x.shape[1])


# ----------------------------------------------------------------------------------------------------------------------
# the Winograd algorithm, stated on the CPU
# ----------------------------------------------------------------------------------------------------------------------
def wino43_weights(w_ohwi: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """U [6][cout][3][cin] = G g along the kernel's width, evaluated in float64 and -- for dtype = float32 -- rounded once, as
    wino43_weights_kernel does (float64: not rounded at all)."""
    g = w_ohwi.double()
    g0, g1, g2 = g[:, :, 0, :], g[:, :, 1, :], g[:, :, 2, :]
    u = torch.stack([g0 / 4.0, -(g0 + g1 + g2) / 6.0, -(g0 - g1 + g2) / 6.0, g0 / 24.0 + g1 / 12.0 + g2 / 6.0,
                     g0 / 24.0 - g1 / 12.0 + g2 / 6.0, g2])
    return u if dtype == torch.float64 else u.float().to(dtype)


WINO_DEFECTS = ("edge_position", "drop_top_row_term")


def wino43_conv(x: torch.Tensor, w_ohwi: torch.Tensor, dtype: torch.dtype = torch.float32, defect: Optional[str] = None,
                first_left_tap: Optional[torch.Tensor] = None) -> torch.Tensor:
    """conv 3x3 / 1 / pad 1 of x [n][h][w][cin] as csrc/winograd.hip evaluates it, in ``dtype``: 1-D F(4,3) along the width.
    V = B^T d on 6-pixel windows at stride 4 (zero outside the image), six products summed over (kernel row, channel), y = A^T m;
    B^T d and A^T m in the kernel's own association (stage() and the epilogue's pairs), the sum over the channels left to einsum.
    Planted defects (for the CPU tests only):
      "edge_position"       the last pixel column of each row's last tile takes the neighbouring tile position (2 in place of 3
                            in a whole tile, p - 1 in a ragged one; W % 4 == 1 has no neighbour in the tile and is left alone)
      "drop_top_row_term"   the centre kernel row's term is dropped at the top image row only
      first_left_tap        [cin] values that the padding tap left of pixel (image 0, row 0, column 0) reads where it must read
                            zero (the words in front of x in memory)."""
    assert defect is None or defect in WINO_DEFECTS
    n, h, wd, c = x.shape
    co, tw = w_ohwi.shape[0], (wd + 3) // 4
    u = wino43_weights(w_ohwi, dtype)
    xp = torch.zeros((n, h + 2, 4 * tw + 2, c), dtype=dtype)
    xp[:, 1:h + 1, 1:wd + 1] = x.to(dtype)
    if first_left_tap is not None:
        xp[0, 1, 0] = first_left_tap.to(dtype)
    d = xp.unfold(2, 6, 4)                                              # [n][h + 2][tw][c][6]
    d0, d1, d2, d3, d4, d5 = (d[..., i] for i in range(6))
    s12, q12 = -4.0 * d2 + d4, 4.0 * d1 - d3
    s34, q34 = d4 - d2, 2.0 * d3 - 2.0 * d1
    v = torch.stack([(4.0 * d0 - 5.0 * d2) + d4, s12 - q12, s12 + q12, s34 + q34, s34 - q34, (4.0 * d1 - 5.0 * d3) + d5])
    m = torch.zeros((6, n, h, tw, co), dtype=dtype)
    for kh in range(3):
        term = torch.einsum("xnhtc,xoc->xnhto", v[:, :, kh:kh + h], u[:, :, kh, :])
        if defect == "drop_top_row_term" and kh == 1:
            term[:, :, 0] = 0.0
        m = m + term
    m0, m1, m2, m3, m4, m5 = m
    a12, b12, a34, b34 = m1 + m2, m1 - m2, m3 + m4, m3 - m4
    t = b34 + b34
    y = torch.stack([(m0 + a12) + a34, b12 + t, a12 + 4.0 * a34, (b12 + 4.0 * t) + m5], dim=3)      # [n][h][tw][4][co]
    y = y.reshape(n, h, 4 * tw, co)[:, :, :wd].contiguous()
    if defect == "edge_position" and (wd - 1) % 4 >= 1:
        y[:, :, wd - 1] = y[:, :, wd - 2]
    return y


def conv_wino(case: ConvCase, dtype: torch.dtype = torch.float32, **kw) -> torch.Tensor:
    """The Winograd statement + affine + residual before the activation, NHWC, in ``dtype``."""
    assert case.stride == 1 and case.pad == 1 and tuple(case.w.shape[1:3]) == (3, 3)
    y = wino43_conv(case.x, case.w, dtype, **kw) * case.scale.to(dtype) + case.shift.to(dtype)
    return y if case.residual is None else y + case.residual.to(dtype)


# ----------------------------------------------------------------------------------------------------------------------
# the element-wise check
# ----------------------------------------------------------------------------------------------------------------------
def c_elements(y: torch.Tensor, z: torch.Tensor, S: torch.Tensor, relu: bool = False) -> torch.Tensor:
    """Per element the smallest c with act(z - c u S) <= y <= act(z + c u S).  Without an activation |y - z| / (u S).  With
    ReLU: y > 0 needs |y - z| <= delta (below, only y <= z + delta binds when z - delta < 0: then y - z > 0 anyway), y == 0
    needs z <= delta, y < 0 (and NaN) is never in.  An element with S == 0 is exact by construction: any error is infinite."""
    yd = y.detach().cpu().double()
    if yd.shape != z.shape:
        raise AssertionError(f"shape {tuple(yd.shape)} != reference {tuple(z.shape)}")
    if relu:
        need = torch.where(yd > 0, (yd - z).abs(), z.clamp_min(0.0))
        need = torch.where(yd < 0, torch.full_like(need, math.inf), need)
    else:
        need = (yd - z).abs()
    need = torch.where(torch.isnan(yd), torch.full_like(need, math.inf), need)
    zero = S == 0
    c = need / (U * S.masked_fill(zero, 1.0))
    return torch.where(zero & (need != 0), torch.full_like(c, math.inf), c)


def c_of(y: torch.Tensor, z: torch.Tensor, S: torch.Tensor, relu: bool = False) -> float:
    return float(c_elements(y, z, S, relu).max())


def c_post(y: torch.Tensor, z: torch.Tensor, S: torch.Tensor, post: Callable[[torch.Tensor], torch.Tensor], c_max: float = 64.0) -> float:
    """The smallest c (to 1 %) with post(z - c u S) <= y <= post(z + c u S) on every element, post monotone (the stem's ReLU +
    max-pool): bisection, since the bound does not come apart per element behind a max; inf if c_max is not enough."""
    yd = y.detach().cpu().double()

    def holds(c: float) -> bool:
        d = (c * U) * S
        return bool(((post(z - d) <= yd) & (yd <= post(z + d))).all())
    if not holds(c_max):
        return math.inf
    lo, hi = 0.0, c_max
    while hi - lo > 0.01 * hi:
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if holds(mid) else (mid, hi)
    return hi


def clamped_share(z: torch.Tensor) -> float:
    """Share of the outputs that ReLU sets to exactly zero."""
    return float((z <= 0).double().mean())


def clear_low_bits(y: torch.Tensor, bits: int = 3) -> torch.Tensor:
    """A planted defect: the low mantissa bits of an fp32 tensor cleared."""
    return (y.detach().float().contiguous().view(torch.int32) & ~((1 << bits) - 1)).view(torch.float32).view(y.shape)


@dataclass
class ConvRef:
    """What a convolution case is judged by: z, S of the case itself, and c_ref of the CPU fp32 statement (``kind``: "wino" or
    "direct") measured over the case and as many extra images as make MIN_REF_ELEMS output elements."""
    z: torch.Tensor
    S: torch.Tensor
    c_ref: float
    ref_elems: int


def conv_ref(case: ConvCase, kind: str, seed: int = 9000) -> ConvRef:
    fp32 = {"wino": conv_wino, "direct": conv_direct}[kind]
    z, S = conv_exact(case)
    c_ref, elems = c_of(fp32(case, torch.float32), z, S), z.numel()
    if elems < MIN_REF_ELEMS:
        per_image = z.numel() // z.shape[0]
        extra = more_images(case, -(-(MIN_REF_ELEMS - elems) // per_image), seed)
        ze, Se = conv_exact(extra)
        c_ref, elems = max(c_ref, c_of(fp32(extra, torch.float32), ze, Se)), elems + ze.numel()
    return ConvRef(z, S, c_ref, elems)


# ----------------------------------------------------------------------------------------------------------------------
# the memory harness
# ----------------------------------------------------------------------------------------------------------------------
NAN_BITS = 0x7FC00000            # what the input moats hold: a quiet NaN
PAYLOAD_BITS = 0x7FC5A5A5        # what an output and its moats hold before the launch: a quiet NaN nobody computes


def moat_words(shape: Sequence[int]) -> int:
    """32-bit words of one moat: max(64 KiB, 4 image rows of the tensor), rounded up to 256 bytes so that the tensor between the
    moats keeps the allocation's alignment.  An image row of [..., W, C] is W * C words."""
    row = int(shape[-1]) * (int(shape[-2]) if len(shape) >= 3 else 1)
    return -(-max(64 * 1024 // 4, 4 * row) // 64) * 64


class Moated:
    """One allocation [moat | tensor | moat] of 32-bit words on ``device``.  An input (data given): the moats hold NaN, the tensor
    the data.  An output (data None): moats AND tensor hold PAYLOAD_BITS.  ``t`` is the fp32 tensor in the middle."""

    def __init__(self, shape: Sequence[int], device, data: Optional[torch.Tensor] = None, dtype: torch.dtype = torch.float32):
        assert dtype in (torch.float32, torch.int32)
        self.shape, self.moat = tuple(int(s) for s in shape), moat_words(shape)
        self.numel = math.prod(self.shape)
        self.bits = NAN_BITS if data is not None else PAYLOAD_BITS
        self.raw = torch.full((2 * self.moat + self.numel,), self.bits, dtype=torch.int32, device=device)
        self.t = self.raw[self.moat:self.moat + self.numel].view(dtype).view(self.shape)
        if data is not None:
            assert tuple(data.shape) == self.shape and data.dtype == dtype
            self.t.copy_(data)

    def ptr(self) -> int:
        return self.t.data_ptr()

    def moats_intact(self) -> bool:
        m = self.moat
        return bool((self.raw[:m] == self.bits).all()) and bool((self.raw[m + self.numel:] == self.bits).all())

    def unwritten(self) -> int:
        """Words of the tensor that still hold the payload pattern."""
        return int((self.raw[self.moat:self.moat + self.numel] == PAYLOAD_BITS).sum())

    def words_before(self, k: int) -> torch.Tensor:
        """The k fp32 words in front of the tensor (what a load one pixel too far to the left reads)."""
        return self.raw[self.moat - k:self.moat].view(torch.float32)


def harness_findings(inputs: Sequence[Moated], out: Moated) -> List[str]:
    """What the harness holds against a launch (empty: nothing): a moat that changed, an element of the output never written, a
    non-finite output."""
    found = [f"the moat of input {i} was written" for i, b in enumerate(inputs) if not b.moats_intact()]
    if not out.moats_intact():
        found.append("the output's moat was written")
    if out.unwritten():
        found.append(f"{out.unwritten()} output elements were never written")
    if not bool(torch.isfinite(out.t).all()):
        found.append("the output is not finite")
    return found


# ----------------------------------------------------------------------------------------------------------------------
# launch_conv_wino's route rule, restated
# ----------------------------------------------------------------------------------------------------------------------
ROUTES: Dict[str, Dict[str, int]] = {
    # route              RPG_TUNE_ keys (csrc/winograd.hip launch_conv_wino); ops.tuned puts every key back afterwards
    "wave4":            {"WINOGRAD": 2},
    "wave8_whole":      {"WINOGRAD": 3, "WINO_SPLIT": 0, "WINO_PERSIST": 0},
    "split_launch":     {"WINOGRAD": 3, "WINO_SPLIT": 1, "WINO_PERSIST": 0, "INKERNEL_FIXUP": 0},
    "split_inkernel8":  {"WINOGRAD": 3, "WINO_SPLIT": 1, "WINO_PERSIST": 0, "INKERNEL_FIXUP": 2},
    "split_inkernel32": {"WINOGRAD": 3, "WINO_SPLIT": 1, "WINO_PERSIST": 0, "INKERNEL_FIXUP": 6},
    "persist_whole":    {"WINOGRAD": 3, "WINO_SPLIT": 0, "WINO_PERSIST": 2},
    "persist_split":    {"WINOGRAD": 3, "WINO_SPLIT": 1, "WINO_PERSIST": 2},
}
# The model's constants: the defaults of the four keys wino_taken restates the launcher's rule over (this module needs no library;
# tests/test_encoder_sweep_cpu.py holds each to ops.tuning_default).  Nothing is restored from them.
WINO_MODEL_DEFAULTS = {"WINOGRAD": 1, "WINO_SPLIT": 1, "WINO_PERSIST": 1, "INKERNEL_FIXUP": 0}


def wino_taken(keys: Dict[str, int], n: int, h: int, w: int, cin: int, cout: int, cus: int) -> str:
    """What launch_conv_wino does with this shape under these keys on a device of ``cus`` compute units: "wave4" | "wave8_whole" |
    "wave8_split_launch:P" | "wave8_split_inkernel:P" | "persist_whole" | "persist_split:P" (P parts per tail tile).  The persistent
    kernel combines its parts by the fix-up launch.  Shapes of this sweep are far below the 32-bit offset limits."""
    k = {**WINO_MODEL_DEFAULTS, **keys}
    tw = (w + 3) // 4
    m = n * h * tw
    if k["WINOGRAD"] == 2:
        return "wave4"
    assert k["WINOGRAD"] == 3
    t = -(-m // 128) * -(-cout // 64)
    kpr = -(-cin // 16)
    tail = t % cus
    parts = min(cus // tail, kpr) if (k["WINO_SPLIT"] and tail > 0) else 1        # WINO_SPLIT = 1: at least 3 K steps a part
    if k["WINO_PERSIST"] and cin % 16 == 0 and (t > cus or k["WINO_PERSIST"] == 2) and h >= 2:
        return f"persist_split:{parts}" if parts >= 2 else "persist_whole"
    if parts < 2:
        return "wave8_whole"
    combine_max = 32 if k["INKERNEL_FIXUP"] & 4 else 8
    return f"wave8_split_inkernel:{parts}" if (k["INKERNEL_FIXUP"] & 2 and parts <= combine_max) else f"wave8_split_launch:{parts}"


def wino_pays(n: int, h: int, w: int, cin: int, cout: int, min_blocks: int = 16) -> Tuple[bool, int]:
    """rpg::wino_pays at the default tuning -> (taken, units of 64 tiles x 64 channels); the composite forward asks it per
    3x3 stride-1 convolution.  (The offset limits of the rule are far away at the sizes of this sweep.)"""
    if cin % 4 or cout % 4:
        return False, 0
    blocks = -(-(n * h * ((w + 3) // 4)) // 64) * -(-cout // 64)
    return blocks >= min_blocks, blocks


# ----------------------------------------------------------------------------------------------------------------------
# the case lists (shared with the CPU tests, which check the clamped share and the routes' reach on the reference alone)
# ----------------------------------------------------------------------------------------------------------------------
# (n, h, w, cin, cout, residual, distribution).  W in {1, 2, 3, 4, 5, 7, 8, 9} (Tw = 1, 2, 3, every W mod 4), H in {1, 2, 3, 5},
# Cin in {4, 12, 16, 20, 32, 48, 160}, Cout in {4, 60, 64, 68, 132}; M = n H Tw tiles on and beside the 32-tile wave and the
# 64- / 128-tile workgroup boundaries (with Tw = 2 the neighbours of a boundary are 62 | 66 and 126 | 130).
WINO_SHAPES = (
    # H = 1                               M
    (31, 1, 1, 16, 64, False, "normal"),   # 31
    (33, 1, 2, 32, 64, True, "act"),       # 33
    (63, 1, 3, 48, 4, False, "normal"),    # 63
    (65, 1, 4, 16, 60, True, "act"),       # 65
    (127, 1, 3, 16, 64, True, "normal"),   # 127
    (32, 1, 5, 32, 68, True, "normal"),    # 64
    (31, 1, 5, 20, 64, False, "act"),      # 62
    (33, 1, 7, 48, 132, True, "normal"),   # 66
    (63, 1, 7, 48, 64, False, "act"),      # 126
    (65, 1, 8, 20, 64, True, "normal"),    # 130
    (43, 1, 9, 32, 64, False, "act"),      # 129
    (5, 1, 7, 160, 64, True, "normal"),    # 10, ten channel blocks
    (1, 1, 8, 4, 132, False, "normal"),    # 2, one channel quad
    (3, 1, 2, 12, 60, True, "act"),        # 3
    # H = 2
    (16, 2, 1, 16, 64, True, "normal"),    # 32
    (32, 2, 3, 32, 132, False, "act"),     # 64
    (64, 2, 2, 48, 64, True, "normal"),    # 128
    (16, 2, 4, 16, 68, False, "act"),      # 32
    (7, 2, 9, 32, 64, True, "normal"),     # 42
    (3, 2, 1, 32, 4, False, "normal"),     # 6
    (1, 2, 2, 160, 64, True, "act"),       # 2, ten channel blocks
    (32, 2, 3, 12, 64, True, "normal"),    # 64
    (16, 2, 7, 20, 60, False, "normal"),   # 64
    (8, 2, 8, 48, 68, True, "act"),        # 32
    (31, 2, 5, 32, 64, False, "normal"),   # 124
    # H = 3
    (11, 3, 1, 32, 64, True, "act"),       # 33
    (21, 3, 2, 16, 64, False, "normal"),   # 63
    (43, 3, 4, 48, 60, True, "normal"),    # 129
    (7, 3, 9, 32, 132, False, "act"),      # 63
    (21, 3, 5, 32, 64, True, "normal"),    # 126
    (1, 3, 3, 160, 4, False, "act"),       # 3, ten channel blocks
    (11, 3, 7, 4, 64, True, "act"),        # 66
    (5, 3, 8, 16, 132, False, "normal"),   # 30
    (2, 3, 3, 20, 68, True, "act"),        # 6
    # H = 5
    (13, 5, 1, 32, 64, False, "normal"),   # 65
    (5, 5, 9, 20, 68, True, "act"),        # 75
    (13, 5, 7, 16, 132, True, "normal"),   # 130
    (1, 5, 8, 48, 64, False, "act"),       # 10
    (13, 5, 2, 32, 60, True, "act"),       # 65
    (4, 5, 4, 12, 4, False, "normal"),     # 20
    (3, 5, 5, 160, 68, True, "normal"),    # 30, ten channel blocks
    (2, 5, 3, 48, 132, False, "act"),      # 10
)


def wino_shape_id(shape) -> str:
    n, h, w, cin, cout, res, dist = shape
    return f"n{n}h{h}w{w}c{cin}o{cout}{'r' if res else ''}-{dist}"


def wino_cases(route: str) -> List[tuple]:
    """The shapes a route is asked to run: the split routes need two channel blocks (Cin > 16: a part is at least one block), the
    persistent kernel whole channel blocks.  The persistent list keeps its H = 1 shapes: there the launcher must fall back."""
    if route.startswith("split"):
        return [s for s in WINO_SHAPES if s[3] > 16]
    if route.startswith("persist"):
        return [s for s in WINO_SHAPES if s[3] % 16 == 0]
    return list(WINO_SHAPES)


def wino_expected(route: str, shape, cus: int) -> str:
    """What a (route, shape) of the list is MEANT to take, independent of wino_taken's arithmetic on the tile counts: read off the
    issue's route rules (T tiles below the CU count: the split tail takes min(CUs // T, ceil(Cin / 16)) parts; ten parts are
    above the default combine limit of 8; H = 1 never runs persistently; one channel block cannot be split)."""
    n, h, w, cin, cout, _, _ = shape
    t = -(-(n * h * ((w + 3) // 4)) // 128) * -(-cout // 64)
    assert t < cus, "every shape of this sweep has fewer workgroup tiles than the device has compute units"
    parts = min(cus // t, -(-cin // 16))
    if route == "wave4":
        return "wave4"
    if route == "wave8_whole" or (route.startswith("persist") and h == 1 and (route == "persist_whole" or parts < 2)):
        return "wave8_whole"
    if route.startswith("persist") and h == 1:
        return f"wave8_split_launch:{parts}"
    if route == "persist_whole" or (route == "persist_split" and parts < 2):
        return "persist_whole"
    if route == "persist_split":
        return f"persist_split:{parts}"
    assert parts >= 2, (route, shape)
    if route == "split_launch" or (route == "split_inkernel8" and parts > 8):
        return f"wave8_split_launch:{parts}"
    return f"wave8_split_inkernel:{parts}"


# direct convolutions: (kind, k, stride, pad, cin, cout, relu of the encoder, residual) x input extents
DIRECT_KINDS = {"conv3x3s2": (3, 2, 1, 64, 128, True), "conv1x1s2": (1, 2, 0, 64, 128, False), "conv7x7s2": (7, 2, 3, 4, 64, True)}
DIRECT_EXTENTS = ((1, 1), (2, 2), (7, 7), (13, 14), (14, 13), (1, 14), (2, 7))
DIRECT_IMAGES = 3


def direct_case(kind: str, extent: Tuple[int, int], dist: str = "act") -> ConvCase:
    k, stride, pad, cin, cout, _ = DIRECT_KINDS[kind]
    dist = "normal" if kind == "conv7x7s2" else dist                     # the first convolution reads normalised images
    return conv_case(DIRECT_IMAGES, extent[0], extent[1], cin, cout, k, stride, pad, False, dist, 700 + 13 * extent[0] + extent[1])


STEM_SIZES = ((1, 1), (2, 3), (7, 9), (30, 130), (61, 63))
STEM_IMAGES = 2


def stem_operands(h: int, w: int):
    """(x NCHW, weight OIHW, scale, shift) with test_fused_stem_conv_bn_relu_maxpool's values (some negative gammas)."""
    x = torch.randn(STEM_IMAGES, 3, h, w, generator=_gen(h))
    wt = torch.randn(64, 3, 7, 7, generator=_gen(2)) * (2.0 / 147) ** 0.5
    g = _gen(3)
    scale = (torch.rand(64, generator=g) + 0.5) * torch.where(torch.rand(64, generator=g) < 0.15, -1.0, 1.0)
    shift = torch.randn(64, generator=_gen(4)) * 0.3
    return x, wt, scale, shift


# ----------------------------------------------------------------------------------------------------------------------
# the composite encoder
# ----------------------------------------------------------------------------------------------------------------------
FWD_PLANES, FWD_BLOCKS, FWD_FEAT = (64, 128, 256, 512), (1, 1, 1, 1), 64
# (n, H, W): 17 x 17 -> the layers see 5, 3, 2, 1 pixels; 33 x 47 -> 9 x 12, 5 x 6, 3 x 3, 2 x 2; 40 x 56 -> 10 x 14, 5 x 7, 3 x 4, 2 x 2; the larger n of each
# size makes wino_pays differ between the layers of one forward (layer_plan), n = 1 takes the direct kernels throughout
FWD_CASES = ((1, 17, 17), (128, 17, 17), (1, 33, 47), (48, 33, 47), (1, 40, 56), (32, 40, 56))


def layer_extents(h: int, w: int) -> List[Tuple[int, int]]:
    """(h, w) that layers 1 .. 4 work on: conv 7x7 / 2 / pad 3, max-pool 3 / 2 / pad 1, then three stride-2 blocks."""
    half = lambda v: (v - 1) // 2 + 1
    e = [(half(half(h)), half(half(w)))]
    for _ in range(3):
        e.append((half(e[-1][0]), half(e[-1][1])))
    return e


def layer_plan(n: int, h: int, w: int) -> List[Tuple[bool, int]]:
    """Per layer (Winograd taken by its stride-1 3x3 convolutions, units) at the default tuning."""
    return [wino_pays(n, eh, ew, c, c) for (eh, ew), c in zip(layer_extents(h, w), FWD_PLANES)]


def encoder_module(seed: int = 21):
    """oracle.resnet_module.ResNetCPU at FWD_PLANES / FWD_BLOCKS / FWD_FEAT in eval mode with seeded, non-trivial BatchNorm
    statistics (fp32 parameters)."""
    from oracle.resnet_module import ResNetCPU
    torch.manual_seed(seed)
    m = ResNetCPU(FWD_BLOCKS, FWD_PLANES, FWD_FEAT)
    g = _gen(seed + 1)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.weight.data = torch.rand(mod.num_features, generator=g) + 0.5
            mod.bias.data = torch.randn(mod.num_features, generator=g) * 0.1
            mod.running_mean.data = torch.randn(mod.num_features, generator=g) * 0.1
            mod.running_var.data = torch.rand(mod.num_features, generator=g) + 0.5
    return m.eval()


class _WinoConv(torch.nn.Module):
    """A 3x3 stride-1 convolution evaluated by the Winograd statement in the weight's dtype."""

    def __init__(self, conv: torch.nn.Conv2d):
        super().__init__()
        self.weight = conv.weight

    def forward(self, x):
        w = self.weight.detach()
        return _nchw(wino43_conv(_nhwc(x), w.permute(0, 2, 3, 1).contiguous(), w.dtype))


def encoder_forward(module, x_nchw: torch.Tensor, dtype: torch.dtype, wino: bool = False) -> torch.Tensor:
    """The module's forward in ``dtype`` on the CPU; wino: every 3x3 stride-1 convolution by the Winograd statement."""
    import copy
    m = copy.deepcopy(module).to(dtype).eval()
    if wino:
        for parent in list(m.modules()):
            for name, child in list(parent.named_children()):
                if isinstance(child, torch.nn.Conv2d) and child.kernel_size == (3, 3) and child.stride == (1, 1):
                    setattr(parent, name, _WinoConv(child))
    with torch.no_grad():
        return m(x_nchw.to(dtype))
