"""Helpers shared by tests/test_hip_bf16_sweep.py (GPU) and tests/test_bf16_sweep_cpu.py: the memory harness of
encoder_sweep_ref.py for 16-bit tensors, the bf16 dispatcher's rule restated (csrc/conv_bf16.hip launch_conv_bf16, launch_patch,
launch_dma_config, launch_conv_pair_bf16; csrc/block_bf16.inc launch_block64_fused), and the case lists that are ENUMERATED from
that rule.  Test helper (like bf16_rounding.py and encoder_sweep_ref.py): no test lives here, nothing here needs the library or
a GPU.

The bar is bf16_rounding.py's, unchanged: every output element inside [bf16(act(z - c u S)), bf16(act(z + c u S))] with
c = FACTOR c_ref, c_ref measured on the CPU fp32 evaluation over at least MIN_REF_ELEMS outputs (small cases get extra images,
for the reference only), and at most AMBIGUOUS_CAP of the elements with two acceptable answers.
"""
import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

import bf16_rounding as R
import encoder_sweep_ref as E

MIN_REF_ELEMS = E.MIN_REF_ELEMS
Route = Tuple[str, int, int, int, int]            # (family, bm, bn, detail, launches) as rpg_conv_bf16_last_route reports them
NONE: Route = ("none", 0, 0, 0, 0)

# ----------------------------------------------------------------------------------------------------------------------
# the memory harness for 16-bit tensors
# ----------------------------------------------------------------------------------------------------------------------
NAN16_WORD = 0x7FC07FC0          # input moats: a quiet bf16 NaN in both halves of every 32-bit word
PAYLOAD16 = 0x7FA5               # outputs and their moats: a SIGNALLING bf16 NaN (quiet bit clear) -- arithmetic and the
PAYLOAD16_WORD = 0x7FA57FA5      # kernels' rounding only ever produce quiet NaNs, so a half-word nobody wrote shows


def moat_words16(shape: Sequence[int]) -> int:
    """32-bit words of one moat around a 16-bit tensor: max(64 KiB, 4 image rows), rounded up to 256 bytes."""
    row_bytes = 2 * int(shape[-1]) * (int(shape[-2]) if len(shape) >= 3 else 1)
    return -(-max(64 * 1024, 4 * row_bytes) // 256) * 64


class Moated16(E.Moated):
    """encoder_sweep_ref.Moated for a bf16 tensor: one allocation [moat | tensor | moat] of 32-bit words, 256-byte aligned; an
    input's moats hold NaN, an output and its moats PAYLOAD16 in every half-word.  ``t`` is the bf16 tensor in the middle."""

    def __init__(self, shape: Sequence[int], device, data: Optional[torch.Tensor] = None):
        self.shape, self.moat = tuple(int(s) for s in shape), moat_words16(shape)
        self.numel = math.prod(self.shape)
        assert self.numel % 2 == 0, "a 16-bit tensor of whole 32-bit words"
        self.words = self.numel // 2
        self.bits = NAN16_WORD if data is not None else PAYLOAD16_WORD
        self.raw = torch.full((2 * self.moat + self.words,), self.bits, dtype=torch.int32, device=device)
        self.t = self.raw[self.moat:self.moat + self.words].view(torch.bfloat16).view(self.shape)
        if data is not None:
            assert tuple(data.shape) == self.shape and data.dtype == torch.bfloat16
            self.t.copy_(data)

    def moats_intact(self) -> bool:
        m = self.moat
        return bool((self.raw[:m] == self.bits).all()) and bool((self.raw[m + self.words:] == self.bits).all())

    def unwritten(self) -> int:
        """Half-words of the tensor that still hold the payload pattern."""
        return int((self.raw[self.moat:self.moat + self.words].view(torch.int16) == PAYLOAD16).sum())

    def halfwords_before(self, k: int) -> torch.Tensor:
        """The k bf16 values in front of the tensor (what a load one pixel too far to the left reads)."""
        return self.raw[:self.moat].view(torch.bfloat16)[2 * self.moat - k:]


harness_findings = E.harness_findings              # the single check: moats, never-written elements, non-finite output


# ----------------------------------------------------------------------------------------------------------------------
# the dispatcher's rule, restated
# ----------------------------------------------------------------------------------------------------------------------
# defaults of the keys the rule reads (csrc/tuning.h; tests/test_bf16_sweep_cpu.py holds each to ops.tuning_default)
BF16_DEFAULTS = {"BF16_BK": 32, "BF16_FAST": 1, "BF16_TILE": -1, "BF16_DMA": 1, "BF16_PATCH": 1, "BF16_LEAN_EPI": 1,
                 "BF16_PERSIST": 0, "BF16_FUSE_BLOCK": 3, "BF16_TAIL": 1, "BF16_PAIR": 1}
DMA_CONFIGS = {0: (256, 256, 64), 1: (256, 128, 64), 2: (256, 128, 64), 3: (128, 128, 64), 4: (256, 64, 64), 5: (256, 64, 64),
               6: (256, 256, 32), 7: (256, 128, 32), 8: (128, 128, 64), 9: (128, 64, 32)}      # cfg -> (BM, BN, K step)
PATCH_WN = {(256, 128): 2, (512, 128): 2, (256, 256): 4, (160, 256): 8, (128, 128): 2, (512, 64): 1}    # waves along N per tile
LDS_MAX = 160 * 1024


def conv_out(x: int, k: int, s: int, p: int) -> int:
    return (x + 2 * p - k) // s + 1


def _keys(keys: Dict[str, int]) -> Dict[str, int]:
    t = {**BF16_DEFAULTS, **{(k[5:] if k.startswith("TUNE_") else k): v for k, v in keys.items()}}
    t["patch"], t["stages"] = t["BF16_PATCH"] % 10, (3 if t["BF16_PATCH"] >= 10 else 4)
    return t


def patch_plan(bm: int, h: int, w: int) -> Tuple[int, int, int]:
    """launch_patch's LDS patch for a bm-row tile on h x w maps -> (patch rows, slots per row, 1-KiB pieces)."""
    p = (w + 2 + 15) // 16 * 16
    rows, imgs = (bm - 1) // w + 2, (bm - 1) // (h * w) + 2
    pr = rows + 2 * (imgs - 1) + 2
    return pr, p, (pr * p * 64 + 1023) // 1024


def patch_accepts(bm: int, bn: int, ns: int, ps: bool, h: int, w: int, cin: int, cout: int, M: int, lean: bool, cus: int,
                  m_begin: int = 0, m_end: int = 0) -> bool:
    """launch_patch<bm, bn, .., ns, ps> on 3x3 / 1 / 1 with Cin % 64 == 0: the division-exactness limits, the persistent form's
    conditions, the piece and LDS limits, the 32-bit offset limits."""
    if cin % 64:
        return False
    hw = h * w
    if m_end <= 0 or m_end > M:
        m_end = M
    if m_begin < 0 or m_begin >= m_end:
        return False
    pr, _, pieces = patch_plan(bm, h, w)
    imgs = (bm - 1) // hw + 2
    if (hw + bm) * hw >= 1 << 32 or (pr + h + 4) * (h + 2) >= 1 << 32:
        return False
    patch_bytes = pieces * 1024
    slab = 8 * 32 * ((bn // PATCH_WN[(bm, bn)] // 32) * 32 + 4) * 4
    tiles_n = -(-cout // bn)
    n_tiles = -(-(m_end - m_begin) // bm) * tiles_n
    lds = 2 * patch_bytes + ns * bn * 64 + 1024
    if ps:
        if not lean or tiles_n != 1 or n_tiles <= cus or m_begin + (n_tiles + cus) * bm >= 1 << 31:
            return False
        lds = patch_bytes + ns * bn * 64 + 1024 + max(patch_bytes, slab)
    if pieces > 64 or lds > LDS_MAX or lds < slab:
        return False
    return (imgs + 1) * hw * cin * 2 < 1 << 31 and cout * 9 * cin * 2 < 1 << 31


def tail_split(t: Dict[str, int], M: int, cout: int, bm: int, bm_tail: int, cus: int) -> int:
    """Rows of the main launch, or 0: do not split (the lambda of launch_conv_bf16)."""
    if not t["BF16_TAIL"] or cout > 256 or M >= 1 << 30:
        return 0
    tiles = -(-M // bm)
    main_tiles = tiles // cus * cus
    rem = tiles - main_tiles
    if main_tiles == 0 or rem == 0:
        return 0
    tail_rows = M - main_tiles * bm
    return main_tiles * bm if -(-tail_rows // bm_tail) <= cus else 0


def bf16_route(keys: Dict[str, int], n: int, h: int, w: int, cin: int, cout: int, k: int, stride: int, pad: int, res: bool,
               out_f32: bool, cus: int) -> Route:
    """What launch_conv_bf16 launches for this shape under these keys on a device of ``cus`` compute units.  (``res`` does not
    enter the rule: every kernel takes a residual.)"""
    t = _keys(keys)
    ho, wo = conv_out(h, k, stride, pad), conv_out(w, k, stride, pad)
    if min(n, h, w, cin, cout, ho, wo) <= 0 or cin % 8 or cout % 4:
        return NONE
    M, K = n * ho * wo, k * k * cin
    if M >= 1 << 31 or K >= 1 << 24 or h * w * cin >= 1 << 31:
        return NONE
    lean = bool(t["BF16_LEAN_EPI"]) and not out_f32 and 1024 * cout * 2 < 1 << 31
    big_k = t["BF16_BK"] == 64 and K >= 128
    small_w = cout * K * 2 < 1 << 31
    fast = bool(t["BF16_FAST"]) and cin % 64 == 0 and (256 // (ho * wo) + 2) * h * w * cin * 2 < 1 << 31 and small_w
    dma_ok = (1024 // (ho * wo) + 2) * h * w * cin * 2 < 1 << 31 and small_w
    t256 = -(-M // 256) * -(-cout // 256)
    dma_cfg = -1
    if dma_ok and t["BF16_DMA"] == 1 and M >= 8192 and cin % 32 == 0:
        if cout <= 64:
            dma_cfg = 5 if cin % 64 == 0 else -1
        elif cout <= 128 or 4 * t256 < 3 * cus or cin % 64:
            dma_cfg = 7
        else:
            dma_cfg = 0
    elif dma_ok and t["BF16_DMA"] >= 10:
        dma_cfg = t["BF16_DMA"] - 10
    # the patch kernel
    mode, four = t["patch"], t["stages"] != 3
    if mode and k == 3 and stride == 1 and pad == 1 and (mode >= 2 or M >= 8192):
        def p(bm, bn, ns, ps=False, m0=0, m1=0):
            return patch_accepts(bm, bn, ns, ps, h, w, cin, cout, M, lean, cus, m0, m1)

        def first(*cands):
            """The first accepted (bm, bn, ns, ps, m_begin, m_end) of an || chain, or None."""
            return next((c for c in cands if p(*c)), None)

        def rec(main, launches=1) -> Route:
            return ("patch_persistent" if main[3] else "patch", main[0], main[1], main[2], launches)
        big = M >= 65536 or mode >= 2
        if mode == 3:
            got = first((256, 128, 3, False, 0, 0))
            if got:
                return rec(got)
        elif mode == 4 and cout > 128:
            got = first((512, 128, 4, False, 0, 0), (512, 128, 3, False, 0, 0))
            if got:
                return rec(got)
        elif cout > 128 and 4 * t256 >= 3 * cus:
            mm = tail_split(t, M, cout, 256, 160, cus) if (t["BF16_TAIL"] & 2) and cout <= 256 else 0
            got = first(*([(256, 256, 4, False, 0, mm)] if four else []), (256, 256, 3, False, 0, mm))
            if got and not mm:
                return rec(got)
            if got and first((160, 256, 3, False, mm, 0), (256, 256, 3, False, mm, 0)):
                return rec(got, 2)
            # (the main launch ran and no tail tile took the rest: the launcher then runs a second kernel family over ALL rows;
            # no shape of this sweep gets here -- a tail the main tile took is taken by the same tile)
            assert not got, "main launch without a tail launch"
        elif cout > 128:
            got = first((256, 128, 3, False, 0, 0))
            if got:
                return rec(got)
        elif cout > 64 and big:
            tl = t["BF16_TAIL"]
            mm = tail_split(t, M, cout, 512, 128 if tl & 4 else 256, cus) if tl & 1 else 0
            got = first(*([(512, 128, 4, False, 0, mm)] if four else []), (512, 128, 3, False, 0, mm))
            if got and not mm:
                return rec(got)
            if got:
                tails = ([(128, 128, 3, False, mm, 0)] if tl & 4 else []) + [(256, 128, 3, False, mm, 0), (512, 128, 3, False, mm, 0)]
                if first(*tails):
                    return rec(got, 2)
            assert not got, "main launch without a tail launch"
        elif mode >= 2 or big:
            got = first(*([(512, 64, 4, True, 0, 0)] if t["BF16_PERSIST"] and four else []),
                        *([(512, 64, 4, False, 0, 0)] if four else []), (512, 64, 3, False, 0, 0))
            if got:
                return rec(got)
    if dma_cfg in DMA_CONFIGS and cin % DMA_CONFIGS[dma_cfg][2] == 0:
        bm, bn, _ = DMA_CONFIGS[dma_cfg]
        return ("dma", bm, bn, dma_cfg, 1)
    tiles128 = -(-M // 128) * -(-cout // 128)
    if fast and t["BF16_TILE"] >= 0:
        bm, bn = {0: (64, 64), 1: (128, 128), 3: (128, 64)}.get(t["BF16_TILE"], (256, 64))
        return ("interleaved", bm, bn, 64, 1)
    if fast:
        if cout <= 64 and M >= 65536:
            return ("interleaved", 128, 64, 64, 1)
        return ("interleaved", 64, 64, 64, 1) if cout <= 64 or tiles128 < 256 else ("interleaved", 128, 128, 64, 1)
    if cout <= 64 and M >= 65536:
        return ("general", 256, 64, 64 if big_k else 32, 1)
    if cout <= 64 or tiles128 < 256:
        return ("general", 64, 64, 32, 1)
    return ("general", 128, 128, 64 if big_k else 32, 1)


def pair_route(keys: Dict[str, int], n: int, h: int, w: int, cin: int, cout: int, k: int, stride: int, pad: int, cus: int) -> Route:
    """launch_conv_pair_bf16: k x k / stride / pad and 1 x 1 / stride / 0 of one input as one launch, or NONE (refused)."""
    t = _keys(keys)
    if not t["BF16_PAIR"] or t["BF16_DMA"] != 1 or n <= 0 or cin % 32 or cout % 4:
        return NONE
    ho, wo = conv_out(h, k, stride, pad), conv_out(w, k, stride, pad)
    if ho <= 0 or wo <= 0 or ho != conv_out(h, 1, stride, 0) or wo != conv_out(w, 1, stride, 0):
        return NONE
    M, ka = n * ho * wo, k * k * cin
    if M < 8192 or M >= 1 << 31 or ka >= 1 << 24:
        return NONE
    if (1024 // (ho * wo) + 2) * h * w * cin * 2 >= 1 << 31 or cout * ka * 2 >= 1 << 31:
        return NONE
    t256 = -(-M // 256) * -(-cout // 256)
    return ("pair", 256, 128, 7, 1) if cout <= 128 or 4 * t256 < 3 * cus or cin % 64 else ("pair", 256, 256, 0, 1)


def block_plan(n: int, h: int, w: int) -> Optional[Dict[str, int]]:
    """launch_block64_fused's strip search: the whole map if it is at most 63 wide and its patch fits, else two column strips
    with views of ceil(w / 2) + 2, + 3, ... columns -- the first view whose patch fits (<= 72 pieces, the LDS) is taken.
    -> {strips, view, pieces, lds, tiles} or None (refused)."""
    BM2, BM1, NS, C, slab = 512, 640, 4, 64, 8 * 32 * 36 * 4
    if n <= 0 or w < 4 or h < 1:
        return None
    wfull, ws = w, (w + 1) // 2
    wv, first, plan = (ws + 2 if wfull + 1 > 64 else wfull), True, None
    while wv + 1 <= 64 and plan is None:
        two = not (first and wfull + 1 <= 64)
        if two and wv >= wfull:
            break
        nv = 2 * n if two else n
        M, hw = nv * h * wv, h * wv
        if M >= 1 << 30:
            return None
        p = (wv + 2 + 15) // 16 * 16
        rows, imgs = (BM1 - 1) // wv + 2, (BM1 - 1) // hw + 2
        pr = rows + 2 * (imgs - 1) + 2
        pieces = (pr * p * 64 + 1023) // 1024
        if (hw + BM1) * hw >= 1 << 32 or (pr + h + 4) * (h + 2) >= 1 << 32:
            return None
        lds = 2 * pieces * 1024 + NS * C * 64 + 1024
        if pieces <= 72 and slab <= lds <= LDS_MAX:
            plan = {"strips": 2 if two else 1, "view": wv, "pieces": pieces, "lds": lds, "tiles": -(-M // BM2)}
        if (imgs + 1) * h * wfull * C * 2 >= 1 << 31:
            return None
        wv, first = (ws + 2 if first and wfull + 1 <= 64 else wv + 1), False
    if plan is None:
        return None
    if ((BM1 - 1) // (h * plan["view"]) + 3) * h * wfull * C * 2 >= 1 << 31:
        return None
    if plan["strips"] == 2 and n * h * wfull * C * 2 >= 1 << 31:
        return None
    return plan


def block_route(keys: Dict[str, int], n: int, h: int, w: int, cus: int) -> Route:
    """What rpg_basicblock64_bf16 launches (the entry point does not read bit 0 of RPG_TUNE_BF16_FUSE_BLOCK: the composite does)."""
    t, plan = _keys(keys), block_plan(n, h, w)
    if plan is None:
        return NONE
    fb = t["BF16_FUSE_BLOCK"] & 7
    if fb & 4 and plan["lds"] + 64 * 64 <= LDS_MAX:
        return ("block_two_group", 512, 64, 5, 1)
    pgrid = cus & ~7
    if fb & 2 and pgrid >= 8 and plan["tiles"] > pgrid and plan["pieces"] * 1024 >= 8 * 32 * 36 * 4:
        return ("block_persistent", 512, 64, 4, 1)
    return ("block", 512, 64, 4, 1)


def images_in_widest_tile(M: int, hw: int, bm: int) -> int:
    """The largest number of images a bm-row tile of an M-row launch touches."""
    return max((min((t + 1) * bm, M) - 1) // hw - (t * bm) // hw + 1 for t in range(-(-M // bm)))


# ----------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    """One convolution case: the keys it runs under (``route``: a name of PATCH_ROUTES or ANY_ROUTES), its shape, what it is on
    the list for, and the epilogue options."""
    route: str
    n: int
    h: int
    w: int
    cin: int
    cout: int
    k: int
    stride: int
    pad: int
    res: bool
    relu: bool
    lean: int
    out_f32: bool
    why: str

    @property
    def id(self) -> str:
        flags = ("r" if self.res else "") + ("a" if self.relu else "") + ("" if self.lean else "g") + ("f" if self.out_f32 else "")
        return f"{self.route}-{self.why}-n{self.n}h{self.h}w{self.w}c{self.cin}o{self.cout}k{self.k}s{self.stride}{'-' + flags if flags else ''}"

    @property
    def keys(self) -> Dict[str, int]:
        return {**ALL_ROUTES[self.route]["keys"], "BF16_LEAN_EPI": self.lean}

    @property
    def out_hw(self) -> Tuple[int, int]:
        return conv_out(self.h, self.k, self.stride, self.pad), conv_out(self.w, self.k, self.stride, self.pad)

    def expected(self, cus: int) -> Route:
        return bf16_route(self.keys, self.n, self.h, self.w, self.cin, self.cout, self.k, self.stride, self.pad, self.res, self.out_f32, cus)


CUS = 256                        # the lists are enumerated for the MI355X's 256 compute units

# The patch kernel's routes: every (tile, weight stages, form) launch_conv_bf16's table can reach.  want: what the rule must say for an
# accepted shape; rows(cus): the fewest output rows at which the table goes there (more than one tile everywhere; three quarters of
# the CUs in 256 x 256 tiles; more than one round for the persistent form and the tail re-tilings).
PATCH_ROUTES: Dict[str, dict] = {
    "p256x128s3":          {"keys": {"BF16_PATCH": 3}, "cout": 128, "want": ("patch", 256, 128, 3, 1), "rows": lambda cus: 257},
    "p256x128s3_narrow":   {"keys": {"BF16_PATCH": 2}, "cout": 256, "want": ("patch", 256, 128, 3, 1), "rows": lambda cus: 257},
    "p512x128s4":          {"keys": {"BF16_PATCH": 2, "BF16_TAIL": 0}, "cout": 128, "want": ("patch", 512, 128, 4, 1), "rows": lambda cus: 513},
    "p512x128s3":          {"keys": {"BF16_PATCH": 12, "BF16_TAIL": 0}, "cout": 128, "want": ("patch", 512, 128, 3, 1), "rows": lambda cus: 513},
    "p512x128s4_wide":     {"keys": {"BF16_PATCH": 4}, "cout": 256, "want": ("patch", 512, 128, 4, 1), "rows": lambda cus: 513},
    "p512x64s4":           {"keys": {"BF16_PATCH": 2}, "cout": 64, "want": ("patch", 512, 64, 4, 1), "rows": lambda cus: 513},
    "p512x64s3":           {"keys": {"BF16_PATCH": 12}, "cout": 64, "want": ("patch", 512, 64, 3, 1), "rows": lambda cus: 513},
    "p512x64s4_persist":   {"keys": {"BF16_PATCH": 2, "BF16_PERSIST": 1}, "cout": 64, "want": ("patch_persistent", 512, 64, 4, 1),
                            "rows": lambda cus: cus * 512 + 1},
    "p256x256s4":          {"keys": {"BF16_PATCH": 2, "BF16_TAIL": 0}, "cout": 256, "want": ("patch", 256, 256, 4, 1),
                            "rows": lambda cus: (-(-3 * cus // 4) - 1) * 256 + 1},
    "p256x256s3":          {"keys": {"BF16_PATCH": 12, "BF16_TAIL": 0}, "cout": 256, "want": ("patch", 256, 256, 3, 1),
                            "rows": lambda cus: (-(-3 * cus // 4) - 1) * 256 + 1},
    "tail512_256":         {"keys": {"BF16_PATCH": 2, "BF16_TAIL": 1}, "cout": 128, "want": ("patch", 512, 128, 4, 2), "rows": lambda cus: cus * 512 + 1},
    "tail512_128":         {"keys": {"BF16_PATCH": 2, "BF16_TAIL": 5}, "cout": 128, "want": ("patch", 512, 128, 4, 2), "rows": lambda cus: cus * 512 + 1},
    "tail256_160":         {"keys": {"BF16_PATCH": 2, "BF16_TAIL": 2}, "cout": 256, "want": ("patch", 256, 256, 4, 2), "rows": lambda cus: cus * 256 + 1},
    # the same tails behind a three-stage main tile, which accepts maps the four-stage one refuses (one more KiB-piece of LDS)
    "tail512_256_s3":      {"keys": {"BF16_PATCH": 12, "BF16_TAIL": 1}, "cout": 128, "want": ("patch", 512, 128, 3, 2), "rows": lambda cus: cus * 512 + 1},
    "tail512_128_s3":      {"keys": {"BF16_PATCH": 12, "BF16_TAIL": 5}, "cout": 128, "want": ("patch", 512, 128, 3, 2), "rows": lambda cus: cus * 512 + 1},
    "tail256_160_s3":      {"keys": {"BF16_PATCH": 12, "BF16_TAIL": 2}, "cout": 256, "want": ("patch", 256, 256, 3, 2), "rows": lambda cus: cus * 256 + 1},
}
PATCH_CIN = 64
PATCH_MAX_H, PATCH_MAX_W = 16, 62


def _patch_n(name: str, h: int, w: int, cout: int, cus: int) -> Optional[int]:
    """The fewest images of h x w at which the route is reached with a ragged last tile (rows % BM != 0), or None."""
    spec = PATCH_ROUTES[name]
    bm, n0 = spec["want"][1], -(-spec["rows"](cus) // (h * w))
    for n in range(n0, n0 + 3):
        if (n * h * w) % bm and bf16_route(spec["keys"], n, h, w, PATCH_CIN, cout, 3, 1, 1, False, False, cus) == spec["want"]:
            return n
    return None


def patch_accepted(name: str, cus: int = CUS) -> List[Tuple[int, int, int, int]]:
    """Every (h, w, n, pieces) up to PATCH_MAX_H x PATCH_MAX_W that the route accepts."""
    spec, out = PATCH_ROUTES[name], []
    for h in range(1, PATCH_MAX_H + 1):
        for w in range(1, PATCH_MAX_W + 1):
            n = _patch_n(name, h, w, spec["cout"], cus)
            if n is not None:
                out.append((h, w, n, patch_plan(spec["want"][1], h, w)[2]))
    return out


def patch_cases(name: str, cus: int = CUS) -> List[Case]:
    """The route's accepted shapes with the smallest H, the smallest W, the smallest H W, the largest piece count (smallest map
    among them), and the smallest map again with a Cout tail; each with a ragged last tile (by _patch_n), residual / ReLU
    alternating.  Picks that name the same map are one case."""
    spec, acc = PATCH_ROUTES[name], patch_accepted(name, cus)
    assert acc, name
    picks = {"minH": min(acc, key=lambda a: (a[0], a[0] * a[1])), "minW": min(acc, key=lambda a: (a[1], a[0] * a[1])),
             "minHW": min(acc, key=lambda a: (a[0] * a[1], a[0])), "pieces": min(acc, key=lambda a: (-a[3], a[0] * a[1]))}
    cases, seen = [], set()
    for j, (why, (h, w, n, _)) in enumerate(picks.items()):
        if (h, w) in seen:
            continue
        seen.add((h, w))
        cases.append(Case(name, n, h, w, PATCH_CIN, spec["cout"], 3, 1, 1, bool(j & 1), not j & 2, 1, False, why))
    h, w, _, _ = picks["minHW"]
    cout = spec["cout"] - 4                        # Cout % tile != 0, Cout % 4 == 0, the same branch of the table
    n = _patch_n(name, h, w, cout, cus)
    assert n is not None, name
    cases.append(Case(name, n, h, w, PATCH_CIN, cout, 3, 1, 1, True, True, 1, False, "couttail"))
    return cases


# The routes that take any shape: the general kernel on its three tiles at both K steps, the interleaved kernel's forced tiles, the
# forced LDS-DMA configurations.  rows: the fewest output rows at which launch_conv_bf16 goes to the tile (0: any).
ANY_ROUTES: Dict[str, dict] = {
    "general64x64":      {"keys": {"BF16_FAST": 0, "BF16_DMA": 0, "BF16_PATCH": 0}, "cout": 72, "rows": 0, "want": ("general", 64, 64, 32, 1)},
    "general128x128k32": {"keys": {"BF16_FAST": 0, "BF16_DMA": 0, "BF16_PATCH": 0}, "cout": 72, "rows": 255 * 128 + 1, "want": ("general", 128, 128, 32, 1)},
    "general128x128k64": {"keys": {"BF16_FAST": 0, "BF16_DMA": 0, "BF16_PATCH": 0, "BF16_BK": 64}, "cout": 72, "rows": 255 * 128 + 1,
                          "want": ("general", 128, 128, 64, 1)},
    "general256x64k32":  {"keys": {"BF16_FAST": 0, "BF16_DMA": 0, "BF16_PATCH": 0}, "cout": 60, "rows": 65536, "want": ("general", 256, 64, 32, 1)},
    "general256x64k64":  {"keys": {"BF16_FAST": 0, "BF16_DMA": 0, "BF16_PATCH": 0, "BF16_BK": 64}, "cout": 60, "rows": 65536,
                          "want": ("general", 256, 64, 64, 1)},
    **{f"interleaved_tile{i}": {"keys": {"BF16_TILE": i, "BF16_DMA": 0, "BF16_PATCH": 0}, "cout": 72, "rows": 0,
                                "want": ("interleaved", *{0: (64, 64), 1: (128, 128), 2: (256, 64), 3: (128, 64)}[i], 64, 1)} for i in range(4)},
    **{f"dma{c}": {"keys": {"BF16_DMA": 10 + c, "BF16_PATCH": 0}, "cout": 72, "rows": 0, "want": ("dma", DMA_CONFIGS[c][0], DMA_CONFIGS[c][1], c, 1)}
       for c in range(10)},
}
ALL_ROUTES = {**PATCH_ROUTES, **ANY_ROUTES}
ANY_EXTENTS = ((1, 1), (2, 2), (1, 14), (2, 7), (7, 7), (13, 14), (14, 13))
ANY_KINDS = {"c3s1": (3, 1, 1, 64), "c3s2": (3, 2, 1, 64), "c1s2": (1, 2, 0, 64), "c7s2": (7, 2, 3, 8)}     # k, stride, pad, Cin
ANY_IMAGES = 3
# Cin = 8 is outside the interleaved and the LDS-DMA kernels: the rule sends the 7x7 kind to the general 64 x 64 kernel whatever the
# forced tile or configuration, so one route of each family is enough to show the fall-back
C7S2_ROUTES = ("general64x64", "general128x128k32", "general128x128k64", "general256x64k32", "general256x64k64", "interleaved_tile0", "dma0")


def any_cases(name: str) -> List[Case]:
    """The route on every extent under every kind; residual, ReLU, epilogue and fp32 output walk through their combinations
    along the list (every one of the eight bf16 combinations at least twice per route, fp32 output three or four times).  The
    Cin = 8 kind runs on C7S2_ROUTES only."""
    spec, cases = ANY_ROUTES[name], []
    for ki, (kind, (k, stride, pad, cin)) in enumerate(ANY_KINDS.items()):
        if kind == "c7s2" and name not in C7S2_ROUTES:
            continue
        for ei, (h, w) in enumerate(ANY_EXTENTS):
            j = 7 * ki + ei
            ho, wo = conv_out(h, k, stride, pad), conv_out(w, k, stride, pad)
            n = max(ANY_IMAGES, -(-spec["rows"] // (ho * wo)))
            cases.append(Case(name, n, h, w, cin, spec["cout"], k, stride, pad, bool(j & 1), bool(j & 2), (j >> 2) & 1 ^ 1, j % 7 == 3, kind))
    return cases


def any_reaches(case: Case, cus: int = CUS) -> bool:
    """Whether the case is one where its route's own kernel runs (else: a fall-back the rule names -- Cin = 8 is outside the
    interleaved and LDS-DMA kernels, a 64-element K is below the general kernel's K step of 64)."""
    return case.expected(cus) == ANY_ROUTES[case.route]["want"]


def all_cases(cus: int = CUS) -> List[Case]:
    return [c for name in PATCH_ROUTES for c in patch_cases(name, cus)] + [c for name in ANY_ROUTES for c in any_cases(name)]


# ----------------------------------------------------------------------------------------------------------------------
# operands and references
# ----------------------------------------------------------------------------------------------------------------------
@dataclass
class Operands:
    """bf16 operands in the project's layouts (x, residual NHWC, w OHWI), fp32 scale / shift, and the float64 reference."""
    x: torch.Tensor
    w: torch.Tensor
    scale: torch.Tensor
    shift: torch.Tensor
    residual: Optional[torch.Tensor]
    ref: R.Ref = field(repr=False, default=None)
    c_ref: float = 0.0
    ref_elems: int = 0


def _nchw(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if t is None else t.permute(0, 3, 1, 2)


def _images(n: int, h: int, w: int, c: int, seed: int) -> torch.Tensor:
    return torch.randn((n, h, w, c), generator=torch.Generator().manual_seed(seed)).bfloat16()


def conv_operands(n: int, h: int, w: int, cin: int, cout: int, k: int, stride: int, pad: int, res: bool, seed: int = 0) -> Operands:
    """Seeded operands -- N(0, 1) activations and residual, He-scaled weights, bf16_rounding.wide_scales (channels four orders of
    magnitude apart, a fifth negative) -- and their reference; c_ref over at least MIN_REF_ELEMS outputs (extra images of the same
    distribution for the reference only, as encoder_sweep_ref.more_images does)."""
    g = torch.Generator().manual_seed(1000 + seed)
    wt = (torch.randn((cout, k, k, cin), generator=g) * (2.0 / (cin * k * k)) ** 0.5).bfloat16()
    # Shifts of 2 x the channel's scale, a BatchNorm bias of the size of the convolution's own spread (He-scaled weights on
    # N(0, 1) inputs: sigma = 1.4 scale).  With the older tests' 0.1 the outputs crowd around zero, where S / |z| is largest, and
    # the linear, residual-free cases of 32,768 and 65,536 rows -- whose c_ref is a maximum over millions of outputs, 3.4-3.7 --
    # leave 2.1-2.4 % of their elements with two acceptable answers: above the cap.  The interval's width c u S does not shrink.
    scale, shift = R.wide_scales(cout, 3 + cout + seed, shift_scale=2.0)
    ho, wo = conv_out(h, k, stride, pad), conv_out(w, k, stride, pad)
    x = _images(n, h, w, cin, 2000 + seed)
    r = _images(n, ho, wo, cout, 3000 + seed) if res else None
    ref = R.conv_ref(_nchw(x), _nchw(wt), scale, shift, _nchw(r), stride, pad)
    c_ref, elems = ref.c_ref, ref.z.numel()
    if elems < MIN_REF_ELEMS:
        ne = -(-(MIN_REF_ELEMS - elems) // (ho * wo * cout))
        xe, re_ = _images(ne, h, w, cin, 4000 + seed), (_images(ne, ho, wo, cout, 5000 + seed) if res else None)
        extra = R.conv_ref(_nchw(xe), _nchw(wt), scale, shift, _nchw(re_), stride, pad)
        c_ref, elems = max(c_ref, extra.c_ref), elems + extra.z.numel()
    return Operands(x, wt, scale, shift, r, ref, c_ref, elems)


_OPERANDS: Dict[tuple, Operands] = {}


def case_operands(c: Case) -> Operands:
    """A case's operands, shared by every route and epilogue that runs the same convolution (a handful alive at a time)."""
    key = (c.n, c.h, c.w, c.cin, c.cout, c.k, c.stride, c.pad, c.res)
    if key not in _OPERANDS:
        if len(_OPERANDS) >= 8:
            _OPERANDS.pop(next(iter(_OPERANDS)))
        _OPERANDS[key] = conv_operands(*key, seed=c.h * 17 + c.w)
    return _OPERANDS[key]


def conv_cpu(op: Operands, stride: int, pad: int, relu: bool, defect: Optional[str] = None, tile_rows: int = 0) -> torch.Tensor:
    """The op in fp32 on the CPU, rounded ONCE to bf16 (returned as fp32 values, NHWC): what a kernel must be equivalent to.
    Planted defects (for the CPU tests):
      "neighbour_tap"   the padding taps left of column 0 read the last column of the row above (the pixel in front in memory;
                        for row 0 of an image: the last pixel of the image in front) where they must read zero
      "drop_last_row"   the last output row (pixel) of the launch's ragged last tile of ``tile_rows`` rows is never computed (zero)"""
    x, wt = _nchw(op.x).float(), _nchw(op.w).float()
    k = wt.shape[-1]
    v = lambda t: t.view(1, -1, 1, 1)
    if defect == "neighbour_tap":
        n, c, h, w = x.shape
        flat = op.x.float().reshape(-1, c)                                 # pixels in memory order
        xp = F.pad(x, (pad, pad, pad, pad))
        prev = torch.cat([torch.zeros(1, c), flat[:-1]]).view(n, h, w, c)[:, :, 0, :]      # the pixel in front of each row's first
        for j in range(pad):
            xp[:, :, pad:pad + h, pad - 1 - j] = prev.permute(0, 2, 1) if j == 0 else 0.0
        y = F.conv2d(xp, wt, None, stride=stride)
    else:
        y = F.conv2d(x, wt, None, stride=stride, padding=pad)
    y = y * v(op.scale) + v(op.shift)
    if op.residual is not None:
        y = y + _nchw(op.residual).float()
    y = (F.relu(y) if relu else y).permute(0, 2, 3, 1).contiguous()
    if defect == "drop_last_row":
        flat = y.view(-1, y.shape[-1])
        assert tile_rows and flat.shape[0] % tile_rows, "the defect needs a ragged last tile"
        flat[-1] = 0.0
    return R.bf16_rne(y)


# ----------------------------------------------------------------------------------------------------------------------
# pools, re-layout, stem, composite
# ----------------------------------------------------------------------------------------------------------------------
# the fp32 sweep's grid-stride sizes scaled to 8-channel lanes (8192 x 256 lanes of 8 channels are one sweep of the grid)
MAXPOOL_SHAPES = ((5, 129, 131, 1024), (2, 1, 1, 8), (2, 1, 2, 8), (2, 2, 1, 8), (3, 2, 2, 16), (2, 1, 5, 8), (2, 5, 1, 16))
AVGPOOL_SHAPES = ((16385, 3, 1024), (3, 1, 8), (5, 49, 16), (2, 2, 512), (4, 4, 64))
RELAYOUT_SHAPES = ((3, 900, 800), (2, 1, 1), (1, 3, 5), (2, 2, 1), (1, 1, 2))


def avgpool_ordered_bf16(x: torch.Tensor) -> torch.Tensor:
    """global_avgpool_bf16_kernel's order on bf16 x [n][hw][c]: fp32 sum from zero in ascending pixel order, one fp32 division by
    hw, one rounding to bf16."""
    return E.avgpool_ordered(x.float()).bfloat16()


STEM_SIZES = E.STEM_SIZES
STEM_FORMS = {"strip": 1, "strip_half_per_wave": 33, "strip_bands7": 1 + (7 << 8), "strip_half_bands14": 33 + (14 << 8), "tile": 3}
_STEM: Dict[tuple, tuple] = {}


def stem_pool(t: torch.Tensor) -> torch.Tensor:
    """MaxPool2d(3, 2, 1) of an NCHW tensor, returned NHWC (the monotone map behind the stem's convolution and ReLU)."""
    return F.max_pool2d(t, 3, 2, 1).permute(0, 2, 3, 1).contiguous()


def stem_reference(h: int, w: int):
    """(x, weight OIHW, scale, shift, Ref, c_ref): encoder_sweep_ref.stem_operands, the reference on the bf16-rounded image and
    weights (NCHW, before ReLU and pool), c_ref over >= 2^16 outputs of the convolution (extra images for the reference only)."""
    if (h, w) not in _STEM:
        x, wt, scale, shift = E.stem_operands(h, w)
        ref = R.conv_ref(x.bfloat16(), wt.bfloat16(), scale, shift, None, 2, 3, nhwc=False)
        c_ref = ref.c_ref
        if ref.z.numel() < MIN_REF_ELEMS:
            per = ref.z.numel() // ref.z.shape[0]
            xe = torch.randn(-(-(MIN_REF_ELEMS - ref.z.numel()) // per), 3, h, w, generator=torch.Generator().manual_seed(50 + h))
            c_ref = max(c_ref, R.conv_ref(xe.bfloat16(), wt.bfloat16(), scale, shift, None, 2, 3, nhwc=False).c_ref)
        _STEM[(h, w)] = (x, wt, scale, shift, ref, c_ref)
    return _STEM[(h, w)]

PAIR_SHAPES = ((8192, 1, 1), (4096, 2, 3), (168, 13, 14))          # n, h, w of 3x3 / 2 / 1 + 1x1 / 2: 8192, 8192 and 8232 output pixels
PAIR_CHANNELS = ((64, 128), (128, 260))                             # (cin, cout): the 256 x 128 tile; a Cout tail beyond two of them

FWD_BLOCKS, FWD_PLANES, FWD_FEAT = (2, 1, 1, 1), (64, 128, 256, 512), 64
FWD_SIZES = ((17, 17), (33, 47), (40, 56))                          # layers see 5 3 2 1 | 9x12 5x6 3x3 2x2 | 10x14 5x7 3x4 2x2 pixels
FWD_CHUNK = (1 << 12) | 24                                          # RPG_TUNE_BF16_CHUNK: 24 images a group from 1 MB of activations up


def fwd_large_n(h: int, w: int) -> int:
    """The fewest images at which layer 1 has 8192 pixels (the fused block and the patch kernel by shape) AND layer 2's pair
    launch has 8192 output pixels."""
    (h1, w1), (h2, w2) = E.layer_extents(h, w)[:2]
    return max(-(-8192 // (h1 * w1)), -(-8192 // (h2 * w2)))


def fwd_module(seed: int = 23):
    """oracle.resnet_module.ResNetCPU with blocks (2, 1, 1, 1) -- layer 1 is a run of two identity blocks -- and seeded BatchNorm
    statistics, in eval mode."""
    from oracle.resnet_module import ResNetCPU
    torch.manual_seed(seed)
    m = ResNetCPU(FWD_BLOCKS, FWD_PLANES, FWD_FEAT)
    g = torch.Generator().manual_seed(seed + 1)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.weight.data = torch.rand(mod.num_features, generator=g) + 0.5
            mod.bias.data = torch.randn(mod.num_features, generator=g) * 0.1
            mod.running_mean.data = torch.randn(mod.num_features, generator=g) * 0.1
            mod.running_var.data = torch.rand(mod.num_features, generator=g) + 0.5
    return m.eval()
