"""Helpers shared by tests/test_hip_linear_sweep.py (GPU) and tests/test_linear_sweep_cpu.py: the fp32 Linear engine's operation
(rpg_linear_gather_f32 / rpg_linear_gather_ex_f32: csrc/gemm_f32.hip, csrc/gemm_engine.inc) stated in float64 with its
conditioning sum and in fp32 on the CPU, a plain torch emulation of the engine's arithmetic that can carry planted defects, the
index patterns, and the case lists with the launch route each case is meant to pin.  Test helper (like encoder_sweep_ref.py, whose
element-wise check, value regimes and memory harness it uses): no test lives here, and nothing here needs a GPU.

The operation:   out[r] = act( cat_k( a_k[idx_k[r]][:width_k] ) W^T + bias + res1[i1[r]][:n] + res2[i2[r]][:n] ),  out_relu = max(out, 0)
with every a_k a [rows_k][ld_k] tensor of which the first width_k columns are read (ld_k >= width_k), residual rows of pitch
ldr >= n.  In a LinearCase the columns past a width (and past n in a gathered residual row) hold NaN: a reference that read
them would be NaN, and so is a kernel's output that did.

z, S, u, c(y), c_ref and the bar c_hip <= M c_ref are those of encoder_sweep_ref.py; S = sum |a| |w| + |bias| + |res1| + |res2|.
"""
import math
from dataclasses import dataclass, field, replace
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from encoder_sweep_ref import (CLAMP_CAP, M_START, MIN_REF_ELEMS, U, Moated, activations, c_elements, c_of, clamped_share,  # noqa: F401
                               clear_low_bits, harness_findings)

PATTERNS = ("zero", "last", "reversed", "random", "rows1")
RES_MODES = ("none", "plain", "gathered", "two")
DISTS = ("normal", "act")


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def index_pattern(pattern: str, m: int, rows: int, seed: int) -> torch.Tensor:
    """int64 [m] row ids in [0, rows): every row -> 0 | every row -> rows - 1 | the reversed permutation (rows == m) | random with
    repeats | a source of one row."""
    if pattern == "zero":
        return torch.zeros(m, dtype=torch.int64)
    if pattern == "last":
        return torch.full((m,), rows - 1, dtype=torch.int64)
    if pattern == "reversed":
        assert rows == m
        return torch.arange(m - 1, -1, -1, dtype=torch.int64)
    if pattern == "rows1":
        assert rows == 1
        return torch.zeros(m, dtype=torch.int64)
    assert pattern == "random"
    return torch.randint(0, rows, (m,), generator=_gen(seed), dtype=torch.int64)


def pattern_rows(pattern: str, m: int) -> int:
    """Rows of a gathered tensor under a pattern: never m unless the pattern is a permutation, so that an index used for the wrong
    tensor (or dropped) shows."""
    return {"reversed": m, "rows1": 1}.get(pattern, m // 2 + 3)


def _padded(data: torch.Tensor, ld: int) -> torch.Tensor:
    """[rows][ld] with ``data`` in the first columns and NaN in the others."""
    out = torch.full((data.shape[0], ld), float("nan"))
    out[:, :data.shape[1]] = data
    return out.contiguous()


@dataclass
class Source:
    a: torch.Tensor                       # [rows][ld] fp32, NaN past ``width``
    idx: Optional[torch.Tensor]           # int64 [m] or None (plain: row r)
    width: int

    @property
    def rows(self) -> int:
        return self.a.shape[0]

    @property
    def ld(self) -> int:
        return self.a.shape[1]

    def gathered(self, dtype=torch.float32) -> torch.Tensor:
        rows = self.a if self.idx is None else self.a[self.idx]
        return rows[:, :self.width].to(dtype)


@dataclass
class LinearCase:
    sources: List[Source]
    weight: torch.Tensor                  # [n_out][K]
    bias: Optional[torch.Tensor]
    res_mode: str                         # RES_MODES
    res1: Optional[torch.Tensor]          # plain: [m][n_out]; gathered: [rows][ldr], NaN past n_out
    res_idx: Optional[torch.Tensor]
    res2: Optional[torch.Tensor]
    res2_idx: Optional[torch.Tensor]
    m: int
    relu: bool = False
    want_relu_copy: bool = False
    dist: str = "normal"

    @property
    def n_out(self) -> int:
        return self.weight.shape[0]

    @property
    def k(self) -> int:
        return self.weight.shape[1]

    @property
    def ldr(self) -> int:
        return 0 if self.res1 is None else self.res1.shape[1]

    def a_cat(self, dtype=torch.float32) -> torch.Tensor:
        return torch.cat([s.gathered(dtype) for s in self.sources], 1)

    def residuals(self, dtype=torch.float32) -> List[torch.Tensor]:
        """The residual rows each output row reads, [m][n_out] each."""
        out = []
        for r, i in ((self.res1, self.res_idx), (self.res2, self.res2_idx)):
            if r is not None:
                out.append((r if i is None else r[i])[:, :self.n_out].to(dtype))
        return out


def _values(rows: int, width: int, dist: str, seed: int) -> torch.Tensor:
    return activations((rows, width), dist, seed)


def _weight(n_out: int, widths: Sequence[int], dist: str, seed: int) -> torch.Tensor:
    """N(0, 1 / K).  Under "act" each source's outlier channel (1 mod width, x 1e3) decides the sign of a whole output column:
    its weights are made positive except in every third column, so that ReLU clamps about a third of the columns, not a random
    share of them."""
    k = sum(widths)
    w = torch.randn(n_out, k, generator=_gen(seed)) * k ** -0.5
    if dist == "act":
        sign = torch.where(torch.arange(n_out) % 3 == 2, -1.0, 1.0)
        off = 0
        for wd in widths:
            w[:, off + 1 % wd] = w[:, off + 1 % wd].abs() * sign
            off += wd
    return w.contiguous()


def linear_case(m: int, n_out: int, srcs: Sequence[Tuple[str, int, int, str]], res_mode: str = "none", ldr: int = 0, bias: bool = True,
                relu: bool = False, want_relu_copy: bool = False, dist: str = "normal", seed: int = 0, res_pattern: str = "random",
                bias_heavy: bool = False) -> LinearCase:
    """Seeded operands.  srcs: (kind "plain" | "gather", width, ld, index pattern) per source.  Bias N(0.5, 0.3^2) (the positive
    mean keeps ReLU from clamping most of a small case), or +-30 with ``bias_heavy`` (|z| ~ S: an error of a few ulps of the output
    is an error of a few u S).  Residuals of the sources' distribution; gathered residual rows have pitch ldr > n_out."""
    assert res_mode in RES_MODES and dist in DISTS and 1 <= len(srcs) <= 3
    sources = []
    for i, (kind, width, ld, pattern) in enumerate(srcs):
        assert ld >= width and width % 4 == 0 and ld % 4 == 0
        if kind == "plain":
            sources.append(Source(_padded(_values(m, width, dist, seed + 10 * i), ld), None, width))
        else:
            assert kind == "gather"
            rows = pattern_rows(pattern, m)
            sources.append(Source(_padded(_values(rows, width, dist, seed + 10 * i), ld), index_pattern(pattern, m, rows, seed + 10 * i + 1),
                                  width))
    widths = [s.width for s in sources]
    b = None
    if bias:
        g = _gen(seed + 50)
        b = torch.randn(n_out, generator=g) * 0.3 + 0.5
        if bias_heavy:
            b = torch.where(torch.rand(n_out, generator=g) < 0.5, -30.0, 30.0) + b
    case = LinearCase(sources, _weight(n_out, widths, dist, seed + 40), b, res_mode, None, None, None, None, m, relu, want_relu_copy, dist)
    if res_mode == "plain":
        case.res1 = _values(m, n_out, dist, seed + 60)
    elif res_mode in ("gathered", "two"):
        assert ldr > n_out and ldr % 4 == 0
        rows = pattern_rows(res_pattern, m)
        case.res1 = _padded(_values(rows, n_out, dist, seed + 60), ldr)
        case.res_idx = index_pattern(res_pattern, m, rows, seed + 61)
        if res_mode == "two":
            rows2 = m // 3 + 2
            case.res2 = _padded(_values(rows2, n_out, dist, seed + 70), ldr)
            case.res2_idx = index_pattern("random", m, rows2, seed + 71)
    return case


def more_rows(case: LinearCase, m: int, seed: int) -> LinearCase:
    """The same Linear (weight, bias, residual mode) on m fresh rows of the same distribution, all operands plain: the extra
    samples of the reference."""
    sources = [Source(_values(m, s.width, case.dist, seed + 10 * i), None, s.width) for i, s in enumerate(case.sources)]
    extra = LinearCase(sources, case.weight, case.bias, "none" if case.res1 is None else "plain", None, None, None, None, m, case.relu,
                       case.want_relu_copy, case.dist)
    if case.res1 is not None:
        extra.res1 = _values(m, case.n_out, case.dist, seed + 60)
        if case.res2 is not None:
            extra.res2, extra.res2_idx = _values(m, case.n_out, case.dist, seed + 70), torch.arange(m)
            extra.res_idx = torch.arange(m)
    return extra


# ----------------------------------------------------------------------------------------------------------------------
# the references
# ----------------------------------------------------------------------------------------------------------------------
def linear_exact(case: LinearCase) -> Tuple[torch.Tensor, torch.Tensor]:
    """(z, S) in float64, before the activation."""
    a, w = case.a_cat(torch.float64), case.weight.double()
    z, s = a @ w.t(), a.abs() @ w.abs().t()
    if case.bias is not None:
        z, s = z + case.bias.double(), s + case.bias.double().abs()
    for r in case.residuals(torch.float64):
        z, s = z + r, s + r.abs()
    return z, s


def _finish(y: torch.Tensor, case: LinearCase) -> torch.Tensor:
    """Bias and residuals in the kernels' association, (acc + bias) + (res1 + res2), before the activation."""
    if case.bias is not None:
        y = y + case.bias
    rs = case.residuals()
    if rs:
        y = y + (rs[0] if len(rs) == 1 else rs[0] + rs[1])
    return y


def linear_fp32(case: LinearCase) -> torch.Tensor:
    """F.linear in fp32 on the CPU, + bias and residuals as the kernels associate them, before the activation: what c_ref measures."""
    return _finish(F.linear(case.a_cat(), case.weight), case)


@dataclass
class LinearRef:
    z: torch.Tensor
    S: torch.Tensor
    c_ref: float
    ref_elems: int


def linear_ref(case: LinearCase, seed: int = 9000) -> LinearRef:
    z, S = linear_exact(case)
    c_ref, elems = c_of(linear_fp32(case), z, S), z.numel()
    if elems < MIN_REF_ELEMS:
        extra = more_rows(case, -(-(MIN_REF_ELEMS - elems) // case.n_out), seed)
        c_ref, elems = max(c_ref, c_of(linear_fp32(extra), *linear_exact(extra))), elems + extra.m * case.n_out
    return LinearRef(z, S, c_ref, elems)


# ----------------------------------------------------------------------------------------------------------------------
# the engine's arithmetic in plain torch, with planted defects
# ----------------------------------------------------------------------------------------------------------------------
DEFECTS = ("drop_last_kgroup_partial_m", "segment_off_by_quad", "res2_with_res_idx", "relu_copy_before_residual", "no_bias_on_split",
           "clear_low_bits", "pad_quad", "fold_restart_without_add")


def _raw_quad(src: Source, col: int) -> torch.Tensor:
    """What each output row reads from the four words at column ``col`` of its source row IN MEMORY (past the pitch: the next
    row; past the tensor: the moat's NaN)."""
    flat = torch.cat([src.a.reshape(-1), torch.full((src.ld + 4,), float("nan"))])
    rows = torch.arange(src.a.shape[0]) if src.idx is None else src.idx
    start = rows[:, None] * src.ld + col + torch.arange(4)[None, :]
    return flat[start]


def engine_emulation(case: LinearCase, bm: int = 64, bk: int = 16, fold_k: int = 256, slab_steps: int = 0,
                     defect: Optional[str] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(out, out_relu) as the tile engine computes them, in fp32: K walked in steps of bk across the segments, each step's products
    added to one running accumulator, the accumulator folded into a second one every fold_k of K (fold_steps even, only while two
    more steps follow: tile_mainloop_b), K cut into slabs of slab_steps steps (0: one slab) whose sums are added in ascending k
    (stream-K), then (acc + bias) + (res1 + res2), ReLU if asked, out_relu = max(out, 0).  The sum inside a step is left to
    torch.  Planted defects (for the CPU tests only):
      drop_last_kgroup_partial_m   the last 4-column group of segment 0 is not read for the rows of the last, partial M tile
      segment_off_by_quad          source 1's first quad is read from source 0 (the four words behind its width)
      res2_with_res_idx            residual2's rows are gathered with res_idx
      relu_copy_before_residual    out_relu is taken before the residuals are added
      no_bias_on_split             split (stream-K) tiles lose the bias
      clear_low_bits               the three low mantissa bits of every output are cleared
      pad_quad                     a quad is read one quad too far: from the padding columns behind a source's width
      fold_restart_without_add     at the first fold the accumulator restarts without being added to the second one"""
    assert defect is None or defect in DEFECTS
    a, w = case.a_cat().clone(), case.weight
    m, k = a.shape
    w0 = case.sources[0].width
    if defect == "drop_last_kgroup_partial_m":
        assert m % bm, "needs a partial M tile"
        a[(m // bm) * bm:, w0 - 4:w0] = 0.0
    if defect == "segment_off_by_quad":
        assert len(case.sources) >= 2
        a[:, w0:w0 + 4] = _raw_quad(case.sources[0], w0)
    if defect == "pad_quad":
        off = 0
        for s in case.sources:
            if s.ld > s.width:
                a[:, off + s.width - 4:off + s.width] = _raw_quad(s, s.width)
                break
            off += s.width
        else:
            raise AssertionError("needs a source with ld > width")
    steps = -(-k // bk)
    part = [a[:, s * bk:(s + 1) * bk] @ w[:, s * bk:(s + 1) * bk].t() for s in range(steps)]
    fold_steps = (fold_k // bk) & ~1 if fold_k >= 2 * bk else 1 << 30
    total, first_fold = None, True
    slab_steps = slab_steps or steps
    for ks in range(0, steps, slab_steps):
        ke = min(steps, ks + slab_steps)
        acc, acc2, kt, n = torch.zeros(m, case.n_out), torch.zeros(m, case.n_out), 0, ke - ks
        while kt + 1 < n:
            kstop = min(kt + fold_steps, n)
            while kt + 1 < kstop:
                acc = (acc + part[ks + kt]) + part[ks + kt + 1]
                kt += 2
            if kt + 1 < n:
                if not (defect == "fold_restart_without_add" and first_fold):
                    acc2 = acc2 + acc
                acc, first_fold = torch.zeros_like(acc), False
        if kt < n:
            acc = acc + part[ks + kt]
        slab = acc + acc2
        total = slab if total is None else total + slab
    split = slab_steps < steps
    y = total
    if case.bias is not None and not (defect == "no_bias_on_split" and split):
        y = y + case.bias
    before_res = y
    rs = case.residuals()
    if defect == "res2_with_res_idx" and len(rs) == 2:
        rs[1] = case.res2[case.res_idx % case.res2.shape[0]][:, :case.n_out]
    if rs:
        y = y + (rs[0] if len(rs) == 1 else rs[0] + rs[1])
    if case.relu:
        y = torch.relu(y)
    if defect == "clear_low_bits":
        y = clear_low_bits(y, 3)
    return y, torch.relu(before_res if defect == "relu_copy_before_residual" else y)


# ----------------------------------------------------------------------------------------------------------------------
# the case lists
# ----------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Spec:
    """One case: the builder's arguments, the tuning keys it runs under, the entry point, and the route it claims -- the fields
    of ops.gemm_last_route() that must read so after the launch (``sk``: whether the launch must have split tiles by stream-K)."""
    name: str
    route: str
    m: int
    n_out: int
    srcs: Tuple[Tuple[str, int, int, str], ...]
    res_mode: str = "none"
    ldr: int = 0
    relu: bool = False
    want_relu_copy: bool = False
    dist: str = "normal"
    seed: int = 0
    res_pattern: str = "random"
    bias: bool = True
    bias_heavy: bool = False
    keys: Tuple[Tuple[str, int], ...] = ()
    expect: Tuple[Tuple[str, object], ...] = ()
    sk: bool = False
    entry: str = "ex"

    def build(self) -> LinearCase:
        return linear_case(self.m, self.n_out, self.srcs, self.res_mode, self.ldr, self.bias, self.relu, self.want_relu_copy, self.dist,
                           self.seed, self.res_pattern, self.bias_heavy)

    @property
    def k(self) -> int:
        return sum(s[1] for s in self.srcs)


TILES = {0: (128, 128), 1: (256, 64), 2: (64, 64), 3: (128, 64)}

# route -> (keys, expected record fields, width tuples; the LAST tuple has three segments and serves the mixed arrangement)
TILE_ROUTES: Dict[str, Tuple[Dict[str, int], Dict[str, object], Tuple[Tuple[int, ...], ...]]] = {
    "general_direct": ({"TILE": 2}, {"loader": "general", "epi_lds": 0, "waves": 4, "BK": 16}, ((20, 12), (16, 4, 28), (4, 4, 4))),
    "general_lds": ({"TILE": 2}, {"loader": "general", "epi_lds": 1, "waves": 4, "BK": 16}, ((20, 12), (4, 4, 4), (16, 4, 28))),
    "buffer4_bk16": ({"TILE": 2}, {"loader": "buffer", "epi_lds": 1, "waves": 4, "BK": 16}, ((48, 16), (16, 16, 16))),
    "buffer4_bk32": ({"TILE": 2, "BK": 32}, {"loader": "buffer", "epi_lds": 1, "waves": 4, "BK": 32}, ((32, 96), (32, 32, 64))),
    "buffer4_bk32_128": ({"TILE": 3, "BK": 32, "WAVES8": 0}, {"loader": "buffer", "epi_lds": 1, "waves": 4, "BK": 32}, ((32, 96), (32, 32, 64))),
    "buffer8_t0": ({"TILE": 0, "BK": 32}, {"loader": "buffer", "epi_lds": 1, "waves": 8, "BK": 32}, ((32,), (32, 32), (96, 96, 96))),
    "buffer8_t3": ({"TILE": 3, "BK": 32}, {"loader": "buffer", "epi_lds": 1, "waves": 8, "BK": 32}, ((32,), (32, 32), (96, 96, 96))),
    "tile256": ({"TILE": 1}, {"loader": "buffer", "epi_lds": 1, "waves": 4, "BK": 16}, ((48, 16), (16, 16, 16))),
}
_ARRANGEMENTS = ("gathered", "mixed", "plain", "gathered", "mixed", "gathered", "mixed", "plain")


def _srcs(arrangement: str, widths: Sequence[int], patterns: Sequence[str]) -> Tuple[Tuple[str, int, int, str], ...]:
    """Source tuples of an arrangement; the first source's pitch is one quad wider than its width, the second's two, the third's
    none (ld > width on at least one source of every case; a read one quad too far meets NaN)."""
    kinds = {"plain": ("plain",) * 3, "gathered": ("gather",) * 3, "mixed": ("gather", "plain", "gather")}[arrangement]
    return tuple((kinds[i], wd, wd + (4, 8, 0)[i], patterns[i % len(patterns)]) for i, wd in enumerate(widths))


def tile_route_specs(route: str) -> List[Spec]:
    """Eight cases of a tile-engine route: between them every M in {1, BM - 1, BM, BM + 1, 2 BM + 1} (+ 255 and 257 on the
    256-row tile, which are BM -+ 1), every N in {4, BN - 4, BN, BN + 4} (the direct epilogue: N in {1, 3, 70} and two more that
    are no multiple of 4), the three arrangements (gathered sources through the _ex entry point with their row counts), every
    index pattern on a gathered source, the four residual modes with ldr > n_out, out_relu, ReLU, both value regimes."""
    keys, expect, width_sets = TILE_ROUTES[route]
    bm, bn = TILES[keys["TILE"]]
    ms = (1, bm - 1, bm, bm + 1, 2 * bm + 1)
    ns = (1, 3, 70, bn - 3, bn + 1) if route == "general_direct" else (4, bn - 4, bn, bn + 4)
    specs, gathered_seen = [], 0
    for i, arrangement in enumerate(_ARRANGEMENTS):
        widths = width_sets[-1] if arrangement == "mixed" else width_sets[i % (len(width_sets) - 1)] if len(width_sets) > 1 else width_sets[0]
        if arrangement == "plain":
            patterns = ("random",)
        else:
            patterns = (PATTERNS[gathered_seen % 5], PATTERNS[(gathered_seen + 2) % 5], PATTERNS[(gathered_seen + 3) % 5])
            gathered_seen += 1
        m, n = ms[i % len(ms)], ns[i % len(ns)]
        res_mode = RES_MODES[(i + 1) % 4]
        # ReLU on the cases of at least 256 outputs (a tiny case can clamp any share by chance); out_relu on every other case
        specs.append(Spec(f"{route}-m{m}n{n}-{arrangement}{'+'.join(map(str, widths))}-{'.'.join(patterns)}-{res_mode}", route, m, n,
                          _srcs(arrangement, widths, patterns), res_mode, (n + 7) // 4 * 4 if res_mode in ("gathered", "two") else 0,
                          relu=(i % 3 == 0 and m * n >= 256), want_relu_copy=(i % 2 == 1), dist=DISTS[i % 2], seed=1000 + 37 * i,
                          res_pattern=PATTERNS[(i + 1) % 4], keys=tuple(keys.items()),
                          expect=tuple({"kernel": "tile", "BM": bm, "BN": bn, "combine": "none", **expect}.items())))
    return specs


def streamk_specs(inkernel: bool) -> List[Spec]:
    """M = 333, N = 100 (99 once: the fix-up's scalar form) on few tiles with >= 32 K steps: stream-K splits them; the split tiles
    are combined by the fix-up launch or, with RPG_TUNE_INKERNEL_FIXUP = 1, by the last-arriving workgroup.  K = 512 and 1056 keep
    the buffer loader (every width a multiple of the K step), 516 and 600 take the general one; the 128x64 tile runs K = 1056 at
    K step 32 on eight waves.  Segment ends fall inside, on and beside the boundaries of the 8-step slices."""
    combine = "inkernel" if inkernel else "fixup"
    rows = (
        # tile, n, widths, arrangement, loader, BK, waves
        (2, 100, (256, 128, 128), "mixed", "buffer", 16, 4),
        (2, 100, (256, 260), "gathered", "general", 16, 4),
        (2, 100, (200, 400), "plain", "general", 16, 4),
        (2, 100, (1024, 32), "gathered", "buffer", 16, 4),
        (3, 100, (32, 512, 512), "mixed", "buffer", 32, 8),
        (2, 99, (172, 172, 172), "mixed", "general", 16, 4),
    )
    specs = []
    for i, (tile, n, widths, arrangement, loader, bk, waves) in enumerate(rows):
        bm, bn = TILES[tile]
        res_mode = RES_MODES[(i + 2) % 4]
        patterns = (PATTERNS[i % 5], PATTERNS[(i + 3) % 5], PATTERNS[(i + 1) % 5])
        specs.append(Spec(f"streamk-{combine}-t{tile}-n{n}-{arrangement}{'+'.join(map(str, widths))}-{res_mode}", "streamk_" + combine, 333, n,
                          _srcs(arrangement, widths, patterns), res_mode, 112 if res_mode in ("gathered", "two") else 0,
                          relu=(i % 3 == 1), want_relu_copy=(i % 2 == 0), dist=DISTS[i % 2], seed=3000 + 41 * i,
                          res_pattern=PATTERNS[i % 4], keys=(("TILE", tile), ("INKERNEL_FIXUP", int(inkernel))),
                          expect=(("kernel", "tile"), ("BM", bm), ("BN", bn), ("BK", bk), ("waves", waves), ("loader", loader),
                                  ("epi_lds", int(n % 4 == 0)), ("combine", combine)), sk=True))
    return specs


def linear112_specs(kernel: str, cus: int = 256) -> List[Spec]:
    """The exact-fit kernels: one plain source (a column block of a wider tensor), N = 4096 = 64 tile columns, M = 112 x the tile
    rows that give >= 1.5 tiles per CU (linear112, four waves) or between 1 and 1.5 (linear112k2, eight waves); K in
    {64, 96, 288}; the four residual modes, out_relu, ReLU."""
    tm = -(-3 * cus // 128) if kernel == "linear112" else -(-cus // 64)
    specs = []
    for i, k in enumerate((64, 96, 288, 96)):
        res_mode = RES_MODES[(i + 1) % 4]
        specs.append(Spec(f"{kernel}-m{112 * tm}-k{k}-{res_mode}", kernel, 112 * tm, 4096, (("plain", k, k + 4 * (i % 2 + 1), "random"),), res_mode,
                          4104 if res_mode in ("gathered", "two") else 0, relu=(i == 2), want_relu_copy=(i % 2 == 1), dist=DISTS[i % 2],
                          seed=5000 + 43 * i, res_pattern=PATTERNS[i % 4],
                          expect=(("kernel", kernel), ("BM", 112), ("BN", 64), ("BK", 32), ("waves", 4 if kernel == "linear112" else 8),
                                  ("loader", "buffer"), ("combine", "none"), ("fold_k", 256))))
    return specs


FOLDS = (0, 64, 256)


def fold_specs(cus: int = 256) -> List[Spec]:
    """RPG_TUNE_FOLD_K in {0, 64, 256} x K in {f - BK, f, f + BK, 2 f + BK} (f = the fold length; 256 where folding is off, so that
    the same lengths run as one chain) on the buffer loader's two folding tiles (64x64 on four waves at K step 16, 128x64 on eight
    at K step 32; stream-K off, which would cut these K into slices shorter than a fold) and on linear112 (K step 32, K >= 64)."""
    specs = []
    for fold in FOLDS:
        f = fold or 256
        for route, tile, bk, waves in (("buffer4", 2, 16, 4), ("buffer8", 3, 32, 8), ("linear112", None, 32, 4)):
            for k in (f - bk, f, f + bk, 2 * f + bk):
                if route == "linear112":
                    if k < 64:
                        continue
                    specs.append(Spec(f"fold{fold}-linear112-k{k}", "fold", 112 * -(-3 * cus // 128), 4096, (("plain", k, k + 4, "random"),),
                                      seed=7000 + k + fold, keys=(("FOLD_K", fold),),
                                      expect=(("kernel", "linear112"), ("BK", 32), ("fold_k", fold if fold >= 64 else 0))))
                else:
                    bm, bn = TILES[tile]
                    specs.append(Spec(f"fold{fold}-{route}-k{k}", "fold", bm + 1, bn + 4, (("gather", k, k + 4, "random"),), seed=7000 + k + fold,
                                      keys=(("FOLD_K", fold), ("TILE", tile), ("BK", bk), ("STREAMK", 0)),
                                      expect=(("kernel", "tile"), ("BM", bm), ("BN", bn), ("BK", bk), ("waves", waves), ("loader", "buffer"),
                                              ("combine", "none"), ("fold_k", fold if fold >= 2 * bk else 0))))
    return specs


def long_k_spec(fold: int) -> Spec:
    """K = 4096, M = N = 64 on the 64x64 tile, one sequential chain (fold 0) or folded every 256: the knob's stated purpose."""
    return Spec(f"k4096-fold{fold}", "fold", 64, 64, (("gather", 4096, 4096, "random"),), seed=7777,
                keys=(("FOLD_K", fold), ("TILE", 2), ("STREAMK", 0)),
                expect=(("kernel", "tile"), ("BM", 64), ("BN", 64), ("BK", 16), ("loader", "buffer"), ("combine", "none"), ("fold_k", fold)))


def mantissa_specs() -> List[Spec]:
    """Outputs dominated by one term (a bias of +-30 on top of O(1) sums): |z| ~ S, the cases that weigh mantissa bits, one per
    loader and one on a split tile."""
    base = dict(res_mode="none", dist="normal", bias_heavy=True)
    return [
        Spec("mantissa-general", "mantissa", 65, 68, (("gather", 20, 24, "random"), ("plain", 12, 12, "random")), seed=8100, keys=(("TILE", 2),),
             expect=(("kernel", "tile"), ("loader", "general"), ("epi_lds", 1)), **base),
        Spec("mantissa-buffer", "mantissa", 65, 68, (("gather", 48, 52, "random"), ("plain", 16, 16, "random")), seed=8200, keys=(("TILE", 2),),
             expect=(("kernel", "tile"), ("loader", "buffer"), ("epi_lds", 1)), **base),
        Spec("mantissa-streamk", "mantissa", 130, 68, (("gather", 256, 260, "random"), ("plain", 256, 256, "random")), seed=8300,
             keys=(("TILE", 2),), expect=(("kernel", "tile"), ("loader", "buffer"), ("combine", "fixup")), sk=True, **base),
    ]


def entry_point_spec(entry: str) -> Spec:
    """The same gathered operands through rpg_linear_gather_f32 ("plain": no row counts, so the general loader) and through
    rpg_linear_gather_ex_f32 with rows (the buffer loader)."""
    return Spec(f"entry-{entry}", "entry", 130, 68, (("gather", 48, 48, "random"), ("gather", 16, 16, "reversed")), "plain", seed=8500,
                keys=(("TILE", 2),), expect=(("kernel", "tile"), ("loader", "general" if entry == "plain" else "buffer"), ("epi_lds", 1)),
                entry=entry)


# which list pins which planted defect (test_linear_sweep_cpu.py checks each pair on the CPU; the GPU module runs the same lists)
PINNED_BY = {
    "drop_last_kgroup_partial_m": "buffer4_bk16",
    "segment_off_by_quad": "buffer4_bk16",
    "res2_with_res_idx": "general_lds",
    "relu_copy_before_residual": "buffer8_t3",
    "no_bias_on_split": "streamk_fixup",
    "clear_low_bits": "mantissa",
    "pad_quad": "buffer4_bk32",
    "fold_restart_without_add": "fold",
}


def specs_of(name: str, cus: int = 256) -> List[Spec]:
    if name in TILE_ROUTES:
        return tile_route_specs(name)
    if name in ("streamk_fixup", "streamk_inkernel"):
        return streamk_specs(name == "streamk_inkernel")
    if name in ("linear112", "linear112k2"):
        return linear112_specs(name, cus)
    if name == "fold":
        return fold_specs(cus)
    assert name == "mantissa", name
    return mantissa_specs()


ALL_LISTS = tuple(TILE_ROUTES) + ("streamk_fixup", "streamk_inkernel", "linear112", "linear112k2", "fold", "mantissa")


def emulation_args(spec: Spec) -> Dict[str, int]:
    """bm, bk, fold_k, slab_steps of engine_emulation for a spec: the tile and K step it claims, the fold length of its keys,
    8-step slabs (SK_MIN_ITS) where it claims stream-K."""
    e, k = dict(spec.expect), dict(spec.keys)
    return {"bm": e.get("BM", 112 if "112" in str(e.get("kernel")) else 64), "bk": e.get("BK", 16), "fold_k": k.get("FOLD_K", 256),
            "slab_steps": 8 if spec.sk else 0}
