"""The frame-transform sweep's helper (no tests of its own): the case list with the tile-plan properties every case exists
for, the inputs, variants of the reference with one planted defect each, and a byte-level memory harness.

The reference itself is tests/test_hip_frames.py's numpy restatement of Pillow's 8-bit resampler + ToTensor + Normalize
(ref_table / ref_resize / ref_normalize, which serve any (out_h, out_w)); tests/test_frames_sweep_cpu.py holds it to Pillow
on every case of the list.  This module needs neither the library nor a GPU to import; ``launch`` needs both."""
from __future__ import annotations

import functools
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from test_hip_frames import MEAN, VAR, rand_frames, ref_normalize, ref_resize, ref_table

STD = tuple(np.sqrt(np.asarray(VAR, np.float64)))


# ----------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    in_h: int
    in_w: int
    out_h: int
    out_w: int
    plan: Dict[str, int]          # what ops.frames_plan must say (a subset of its keys, plus last_rows / last_cols / taps_*)
    why: str

    @property
    def id(self) -> str:
        return f"{self.in_h}x{self.in_w}-{self.out_h}x{self.out_w}"

    @property
    def need_h(self) -> bool:
        return self.in_w != self.out_w

    @property
    def need_v(self) -> bool:
        return self.in_h != self.out_h

    @property
    def passes(self) -> str:
        return {(True, True): "both", (True, False): "h", (False, True): "v", (False, False): "none"}[self.need_h, self.need_v]


def taps(n_in: int, n_out: int) -> int:
    """Taps per output index of one axis (the table's row length): 2 * ceil(max(in / out, 1)) + 1, in integers."""
    return 2 * max(-(-n_in // n_out), 1) + 1


def derived(plan: Dict[str, object], case: Case) -> Dict[str, object]:
    """ops.frames_plan's record plus what follows from it and the sizes: the rows / columns of the last tile, whether ``tr`` was
    clamped to out_h, the table row lengths of the passes that run."""
    d = dict(plan)
    d["last_rows"] = case.out_h - (d["tiles_y"] - 1) * d["tr"]
    d["last_cols"] = case.out_w - (d["tiles_x"] - 1) * d["tc"]
    d["taps_h"] = taps(case.in_w, case.out_w) if case.need_h else 0
    d["taps_v"] = taps(case.in_h, case.out_h) if case.need_v else 0
    return d


def _c(ih, iw, oh, ow, why, **plan) -> Case:
    return Case(ih, iw, oh, ow, plan, why)


CASES: List[Case] = [
    # ---- horizontal only: tmp is read as the final image, nrows == th
    _c(256, 640, 256, 341, "horizontal only, full width", need_h=True, need_v=False, tr=8, tiles_x=1, last_rows=8),
    _c(16, 53, 16, 366, "horizontal only, upscale", need_h=True, need_v=False, tr=16, tiles_x=1, taps_h=3),
    _c(3, 1984, 3, 64, "horizontal only at the limit, out_h < 16 (clamped tr)", need_h=True, need_v=False, tr=3, tiles_y=1,
       tiles_x=1, taps_h=63),
    _c(24, 3000, 24, 911, "horizontal only, column tiles 456 + 455", need_h=True, need_v=False, tr=4, tc=456, tiles_x=2,
       last_cols=455),
    _c(21, 53, 21, 100, "horizontal only, short last row tile (nrows == th == 5 under tr = 16)", need_h=True, need_v=False, tr=16,
       last_rows=5),
    _c(300, 5000, 300, 200, "horizontal only, 51 taps, two column tiles", need_h=True, need_v=False, tr=2, tiles_x=2, taps_h=51),
    # ---- vertical only: the vertical pass reads the staged bytes through src_at, no tmp
    _c(480, 341, 256, 341, "vertical only, 32 staged rows", need_h=False, need_v=True, tr=16, tiles_x=1, rows_max=32),
    _c(53, 16, 366, 16, "vertical only, upscale, short last row tile", need_h=False, need_v=True, tr=16, last_rows=14, taps_v=3),
    _c(1984, 3, 64, 3, "vertical only at the limit, W = 3", need_h=False, need_v=True, tr=16, tiles_x=1, rows_max=527, taps_v=63),
    _c(1000, 300, 40, 300, "vertical only with column tiles (c0 != 0 through src_at)", need_h=False, need_v=True, tiles_x=2),
    _c(700, 64, 100, 64, "vertical only, short last row tile", need_h=False, need_v=True, tr=16, last_rows=4),
    # ---- both passes
    _c(248, 248, 8, 8, "both passes at the limit on both axes", need_h=True, need_v=True, tr=2, tc=4, taps_h=63, taps_v=63),
    _c(70, 4000, 33, 500, "both passes, four column tiles, last row tile 1 of 2", need_h=True, need_v=True, tr=2, tiles_x=4,
       last_rows=1),
    _c(600, 1100, 35, 1000, "both passes, 37 vertical taps, 8 column tiles, LDS close to the budget", need_h=True, need_v=True,
       tiles_x=8, taps_v=37, lds_bytes=48864),
    _c(17, 33, 40, 70, "both passes upscaling, last row tile 8 of 16", need_h=True, need_v=True, tr=16, last_rows=8),
    _c(40, 70, 17, 33, "both passes downscaling, last row tile 1 of 16", need_h=True, need_v=True, tr=16, last_rows=1),
    # ---- identity: neither pass, the staged bytes are normalised as they are
    _c(4, 20000, 4, 20000, "identity with column tiles", need_h=False, need_v=False, tr=1, tiles_x=2),
    _c(33, 9000, 33, 9000, "identity, full width at tr = 1", need_h=False, need_v=False, tr=1, tiles_x=1),
    _c(2, 3, 2, 3, "identity, segment shorter than a chunk", need_h=False, need_v=False, tr=2, tiles_x=1, pitch=32),
    _c(1, 1, 1, 1, "identity, one pixel", need_h=False, need_v=False, tr=1, tc=1, pitch=32),
    # ---- 1-pixel axes
    _c(1, 1, 5, 7, "1-pixel source, both passes", need_h=True, need_v=True, tr=5, rows_max=1),
    _c(7, 5, 1, 1, "1-pixel output, both passes", need_h=True, need_v=True, tr=1, tc=1, rows_max=7),
    # ---- the alignment trio
    _c(9, 21, 5, 11, "alignment trio: both passes", need_h=True, need_v=True, tr=5, tiles_x=1, tiles_y=1),
    _c(9, 21, 9, 11, "alignment trio: horizontal only", need_h=True, need_v=False, tr=9, tiles_x=1, tiles_y=1),
    _c(9, 21, 5, 21, "alignment trio: vertical only", need_h=False, need_v=True, tr=5, tiles_x=1, tiles_y=1),
]
TRIO: List[Case] = [c for c in CASES if (c.in_h, c.in_w) == (9, 21)]
TINY_IDENTITY: Case = next(c for c in CASES if (c.in_h, c.in_w) == (2, 3))


def case_by_id(cid: str) -> Case:
    return next(c for c in CASES if c.id == cid)


# ----------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------
CONSTRUCTED = ("all 0", "all 255", "checkerboard")


def constructed_frames(h: int, w: int) -> np.ndarray:
    """[3, h, w, 3]: an all-0 frame and an all-255 frame (the integer weights of an output sum to 2^22 give or take a few
    units, so these decide 254 against 255 and exercise the upper clamp), and a 0 / 255 checkerboard whose phase differs per
    channel (both clamps, the largest tap-to-tap differences)."""
    out = np.zeros((3, h, w, 3), np.uint8)
    out[1] = 255
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for c in range(3):
        out[2, :, :, c] = np.where((yy + xx + c) % 2 == 0, 0, 255)
    return out


@functools.lru_cache(maxsize=None)
def _inputs(h: int, w: int, n_rand: int) -> np.ndarray:
    x = np.concatenate([rand_frames(n_rand, h, w, seed=1000 * h + w), constructed_frames(h, w)])
    x.setflags(write=False)
    return x


def n_rand_of(case: Case) -> int:
    """Random frames per case: 3, or 64 where the output has fewer than 64 pixels (a 1 x 1 output is three numbers per frame,
    too few for a defect that shows only where two roundings happen to disagree, such as the order of the passes)."""
    return 3 if case.out_h * case.out_w >= 64 else 64


def case_inputs(case: Case) -> np.ndarray:
    """uint8 [n_rand_of(case) + 3, in_h, in_w, 3]: ``rand_frames`` frames, then the three constructed ones.  Shared, read-only."""
    return _inputs(case.in_h, case.in_w, n_rand_of(case))


def ref_resize_frames(frames: np.ndarray, oh: int, ow: int) -> np.ndarray:
    """ref_resize one frame at a time (its gather holds taps x the output in int64)."""
    return np.concatenate([ref_resize(frames[i:i + 1], oh, ow) for i in range(len(frames))])


@functools.lru_cache(maxsize=None)
def _want(cid: str) -> Tuple[np.ndarray, torch.Tensor]:
    case = case_by_id(cid)
    img = ref_resize_frames(case_inputs(case), case.out_h, case.out_w)
    img.setflags(write=False)
    return img, torch.from_numpy(ref_normalize(img, MEAN, STD))


def case_resized(case: Case) -> np.ndarray:
    """The reference's uint8 resize of ``case_inputs`` (shared, read-only)."""
    return _want(case.id)[0]


def case_want(case: Case) -> torch.Tensor:
    """The reference's fp32 [n, 3, out_h, out_w] of ``case_inputs`` under (MEAN, STD) (shared: do not write to it)."""
    return _want(case.id)[1]


# ----------------------------------------------------------------------------------------------------------------------
# the reference with one planted defect (to prove that the inputs discriminate; never compared with the kernel)
# ----------------------------------------------------------------------------------------------------------------------
RESIZE_DEFECTS = ("vertical_first", "no_rounding", "one_tap_fewer")
NORM_DEFECTS = ("reciprocal_255", "reciprocal_std")


def _pass(img: np.ndarray, bounds: np.ndarray, weights: np.ndarray, axis: int, rounding: int, drop: int) -> np.ndarray:
    """One 8-bit pass (as test_hip_frames._pass, tap by tap): ``rounding`` is added before the shift, the last ``drop`` taps
    of every output are left out."""
    n_out = bounds.shape[0]
    shape = list(img.shape)
    shape[axis] = n_out
    acc = np.full(shape, rounding, np.int64)
    src = img.astype(np.int64)
    cnt = bounds[:, 1] - drop
    for j in range(weights.shape[1]):
        live = j < cnt
        if not live.any():
            break
        idx = np.where(live, bounds[:, 0] + j, 0)
        w = np.where(live, weights[:, j], 0).astype(np.int64)
        if axis == 2:
            acc += src[:, :, idx, :] * w[None, None, :, None]
        else:
            acc += src[:, idx, :, :] * w[None, :, None, None]
    return np.clip(acc >> 22, 0, 255).astype(np.uint8)


def variant_resize(frames: np.ndarray, oh: int, ow: int, defect: Optional[str] = None) -> np.ndarray:
    """Pillow's resize of uint8 [n, H, W, 3] with ``defect`` planted (None: the resize itself, equal to ref_resize)."""
    assert defect is None or defect in RESIZE_DEFECTS
    n, h, w, _ = frames.shape
    rounding = 0 if defect == "no_rounding" else 1 << 21
    drop = 1 if defect == "one_tap_fewer" else 0
    order = []
    if ow != w:
        order.append((2, ref_table(w, ow)))
    if oh != h:
        order.append((1, ref_table(h, oh)))
    if defect == "vertical_first":
        order.reverse()
    img = frames
    for axis, (b, wt) in order:
        img = _pass(img, b, wt, axis, rounding, drop)
    return img


def defect_applies(defect: str, case: Case) -> bool:
    """Whether ``defect`` can change any output of ``case``, whatever the input.
    - an axis resampled from ONE source sample has one tap of weight exactly 2^22 per output: the pass copies, so neither the
      rounding constant nor the order of the passes can show on it;
    - the order needs two passes that both round;
    - a tap fewer shows on any pass (an output left with no tap at all becomes 0)."""
    rounds_h = case.need_h and case.in_w > 1
    rounds_v = case.need_v and case.in_h > 1
    if defect == "vertical_first":
        return rounds_h and rounds_v
    if defect == "no_rounding":
        return rounds_h or rounds_v
    if defect == "one_tap_fewer":
        return case.need_h or case.need_v
    raise ValueError(defect)


def variant_norm_table(mean: Sequence[float], std: Sequence[float], defect: Optional[str] = None) -> np.ndarray:
    """fp32 [3, 256]: the normalised value of every byte per channel (None: as ref_normalize computes it)."""
    assert defect is None or defect in NORM_DEFECTS
    m = np.asarray(mean, np.float64).astype(np.float32)[:, None]
    s = np.asarray(std, np.float64).astype(np.float32)[:, None]
    u = np.arange(256, dtype=np.float32)[None, :]
    x = u * (np.float32(1) / np.float32(255)) if defect == "reciprocal_255" else u / np.float32(255)
    x = x - m
    return (x * (np.float32(1) / s) if defect == "reciprocal_std" else x / s).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------------------
# byte-level memory harness
# ----------------------------------------------------------------------------------------------------------------------
GUARD = 256                    # guard bytes on either side of a tensor (a multiple of 16: it keeps the alignment asked for)
GUARD_BYTE = 0xA5
NAN16 = 0x7FC1                 # every 16-bit half of an unwritten output: a bf16 NaN, and 0x7FC17FC1 is an fp32 NaN


class GuardedBytes:
    """One uint8 allocation [guard | gap | tensor | guard]: ``t`` is the tensor, ``gap`` (< 16) bytes behind the 16-byte
    boundary the first guard ends at, so ``gap`` is ``t``'s address modulo 16.  The gap holds guard bytes too."""

    def __init__(self, nbytes: int, device, gap: int = 0):
        assert 0 <= gap < 16
        self.nbytes, self.lo = int(nbytes), GUARD + gap
        self.raw = torch.full((self.lo + self.nbytes + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=device)
        assert self.raw.data_ptr() % 16 == 0
        self.t = self.raw[self.lo:self.lo + self.nbytes]
        assert self.t.data_ptr() % 16 == gap

    def guards_changed(self) -> int:
        return int((self.raw[:self.lo] != GUARD_BYTE).sum()) + int((self.raw[self.lo + self.nbytes:] != GUARD_BYTE).sum())


class GuardedFrames(GuardedBytes):
    """uint8 frames [n, H, W, 3] between guards, starting ``gap`` bytes behind a 16-byte boundary."""

    def __init__(self, frames: np.ndarray, device, gap: int = 0):
        super().__init__(frames.size, device, gap)
        self.t = self.t.view(frames.shape)
        self.t.copy_(torch.from_numpy(np.array(frames)).to(device))


class GuardedOut(GuardedBytes):
    """An output [n, 3, oh, ow] of fp32 or bf16 between guards, prefilled with NaNs; ``skip`` elements into its buffer."""

    def __init__(self, shape: Sequence[int], dtype: torch.dtype, device, skip: int = 0):
        assert dtype in (torch.float32, torch.bfloat16)
        size = 4 if dtype == torch.float32 else 2
        numel = int(np.prod(shape))
        super().__init__(numel * size, device, gap=skip * size)
        self.dtype = dtype
        self.t.view(torch.int16).fill_(NAN16)
        self.t = self.t.view(dtype).view(tuple(shape))
        assert bool(torch.isnan(self.t).all())

    def unwritten(self) -> int:
        """Elements that still hold the prefill."""
        if self.dtype == torch.float32:
            return int((self.t.view(torch.int32) == (NAN16 << 16 | NAN16)).sum())
        return int((self.t.view(torch.int16) == NAN16).sum())


@functools.lru_cache(maxsize=None)
def device_tables(in_h: int, in_w: int, out_h: int, out_w: int, device: str):
    """(h_bounds, h_weights, v_bounds, v_weights) of ops.resize_table on ``device``; None for an axis that keeps its size."""
    from relpose_gnn_amd import ops
    hb = hw = vb = vw = None
    if in_w != out_w:
        hb, hw = (t.to(device) for t in ops.resize_table(in_w, out_w))
    if in_h != out_h:
        vb, vw = (t.to(device) for t in ops.resize_table(in_h, out_h))
    return hb, hw, vb, vw


def launch(case: Case, frames: np.ndarray, dtype: torch.dtype, device, mean=MEAN, std=STD, frame_gap: int = 0,
           out_skip: int = 0) -> Tuple[torch.Tensor, List[str]]:
    """ops.frames_u8_to_f32 / _bf16 on ``frames`` inside the harness -> (the output on the CPU, the findings: guard bytes of
    the frames or the output that changed, output elements never written).  Empty findings: nothing to hold against it."""
    from relpose_gnn_amd import ops
    src = GuardedFrames(frames, device, frame_gap)
    dst = GuardedOut((frames.shape[0], 3, case.out_h, case.out_w), dtype, device, out_skip)
    fn = ops.frames_u8_to_bf16 if dtype == torch.bfloat16 else ops.frames_u8_to_f32
    tabs = device_tables(case.in_h, case.in_w, case.out_h, case.out_w, str(device))
    got = fn(src.t, (case.out_h, case.out_w), tabs, mean, std, out=dst.t)
    torch.cuda.synchronize()
    assert got.data_ptr() == dst.t.data_ptr()
    found = []
    if src.guards_changed():
        found.append(f"{src.guards_changed()} guard bytes around the frames changed")
    if dst.guards_changed():
        found.append(f"{dst.guards_changed()} guard bytes around the output changed")
    if dst.unwritten():
        found.append(f"{dst.unwritten()} output elements were never written")
    if not bool(torch.equal(src.t.cpu(), torch.from_numpy(np.array(frames)))):
        found.append("the frames changed")
    return dst.t.cpu(), found
