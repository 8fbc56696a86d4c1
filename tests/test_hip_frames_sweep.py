"""The frame-transform kernel (rpg_frames_u8_to_f32 / _bf16) on every pass combination, tile plan and size limit, bit for bit
against the reference transform (tests/frames_sweep_ref.py: the case list, the inputs and the byte-level memory harness;
tests/test_frames_sweep_cpu.py: the reference against Pillow, the plans the cases take).  Every comparison is exact."""
import numpy as np
import pytest
import torch

import frames_sweep_ref as R
from test_hip_frames import MEAN, rand_frames, ref_normalize, ref_resize, ref_transform

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
DTYPE_IDS = ["f32", "bf16"]
CASE_IDS = [c.id for c in R.CASES]


def _dev():
    return torch.device("cuda:0")


def _same(got: torch.Tensor, want32: torch.Tensor, dtype) -> int:
    """Elements of ``got`` that differ from the fp32 reference (rounded to bf16 for a bf16 output); 0 is a pass."""
    want = want32.to(dtype)
    assert got.shape == want.shape and got.dtype == dtype
    return 0 if torch.equal(got, want) else int((got != want).sum())


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("case", R.CASES, ids=CASE_IDS)
def test_every_case_bit_exact_inside_the_harness(case, dtype):
    frames = R.case_inputs(case)
    got, found = R.launch(case, frames, dtype, _dev())
    assert not found, (case.id, case.why, found)
    assert _same(got, R.case_want(case), dtype) == 0, (case.id, case.why)


@pytest.mark.parametrize("case", R.TRIO, ids=[c.id for c in R.TRIO])
def test_grid_walk_reuses_the_lds_image(case):
    """More tiles than twice the largest grid the launcher starts (8 workgroups per CU): every workgroup walks on to a second
    and a third tile over the LDS image of the one before."""
    from relpose_gnn_amd import ops
    dev = _dev()
    p = ops.frames_plan(case.in_h, case.in_w, case.out_h, case.out_w)
    per_frame = p["tiles_y"] * p["tiles_x"]
    grid_max = 8 * torch.cuda.get_device_properties(dev).multi_processor_count
    n = 2 * grid_max // per_frame + 7
    assert n * per_frame > 2 * grid_max
    frames = np.random.default_rng(case.out_h * 31 + case.out_w).integers(0, 256, (n, case.in_h, case.in_w, 3), dtype=np.uint8)
    want = torch.from_numpy(ref_normalize(ref_resize(frames, case.out_h, case.out_w), MEAN, R.STD))
    for dtype in DTYPES:
        got, found = R.launch(case, frames, dtype, dev)
        assert not found, (case.id, dtype, found)
        assert _same(got, want, dtype) == 0, (case.id, dtype)


ALIGNED = R.TRIO + [R.TINY_IDENTITY]


@pytest.mark.parametrize("case", ALIGNED, ids=[c.id for c in ALIGNED])
def test_every_frame_base_offset_in_a_chunk(case):
    dev = _dev()
    frames, want = R.case_inputs(case), R.case_want(case)
    for gap in range(16):
        for dtype in DTYPES:
            got, found = R.launch(case, frames, dtype, dev, frame_gap=gap)
            assert not found, (case.id, gap, dtype, found)
            assert _same(got, want, dtype) == 0, (case.id, gap, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("case", ALIGNED, ids=[c.id for c in ALIGNED])
def test_out_one_element_into_its_buffer(case, dtype):
    got, found = R.launch(case, R.case_inputs(case), dtype, _dev(), frame_gap=5, out_skip=1)
    assert not found, (case.id, found)
    assert _same(got, R.case_want(case), dtype) == 0, case.id


STATS = {
    "7scenes": (MEAN, R.STD),
    "zero_one": ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
    "negative_std": (MEAN, (-0.25, 0.3, -1.5)),
    "tiny_std": (MEAN, (1e-30, 1e-30, 1e-30)),            # results near 1e30: finite in fp32 and in bf16
    "denormal_std": (MEAN, (1e-39, -1e-39, 1e-39)),       # a denormal divisor: +-inf wherever |u / 255 - mean| > 0.34
    "mean_pm3": ((3.0, -3.0, 3.0), R.STD),
}


@pytest.mark.parametrize("stats", list(STATS), ids=list(STATS))
def test_normalisation_table_every_byte(stats):
    """All 256 byte values in each channel through an identity geometry: the kernel's table against ref_normalize, by bits
    (so -0.0 and the infinities of a denormal std count)."""
    mean, std = STATS[stats]
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16)
    frame = np.stack([ramp, ramp[::-1, ::-1], ramp.T], axis=-1)[None]            # every channel holds every value
    assert all(len(np.unique(frame[0, :, :, c])) == 256 for c in range(3))
    case = R.Case(16, 16, 16, 16, {}, "identity, every byte value")
    with np.errstate(over="ignore", divide="ignore"):
        want = torch.from_numpy(ref_normalize(frame, mean, std))
    assert not bool(torch.isnan(want).any())
    if stats == "denormal_std":
        inf = torch.isinf(want)
        assert bool(inf.any()) and not bool(inf.all()) and bool((want[inf] > 0).any()) and bool((want[inf] < 0).any())
    for dtype, bits in ((torch.float32, torch.int32), (torch.bfloat16, torch.int16)):
        got, found = R.launch(case, frame, dtype, _dev(), mean=mean, std=std)
        assert not found, (stats, dtype, found)
        assert torch.equal(got.view(bits), want.to(dtype).view(bits)), (stats, dtype)


@pytest.mark.parametrize("size", [None, 7, 1000], ids=["none", "7", "1000"])
def test_through_the_public_class(size):
    from relpose_gnn_amd.frames import FrameTransform
    ft = FrameTransform(size, mean=MEAN, std=R.STD)
    frames = rand_frames(2, 40, 70, seed=size or 1)
    if size is None:
        want = torch.from_numpy(ref_normalize(frames, MEAN, R.STD))
    else:
        want = torch.from_numpy(ref_transform(frames, size=size))
    assert tuple(want.shape[2:]) == {None: (40, 70), 7: (7, 12), 1000: (1000, 1750)}[size]
    x = torch.from_numpy(frames).to(_dev())
    for dtype in DTYPES:
        got = ft.apply(x, dtype).cpu()
        assert _same(got, want, dtype) == 0, (size, dtype)


def test_tables_that_do_not_belong_are_refused_before_the_launch():
    """ops.frames_u8_to_* checks its tables against the sizes (the kernel indexes them by the sizes alone): a ValueError that
    names the axis, and nothing launched -- the output keeps its prefill."""
    from relpose_gnn_amd import ops
    dev = _dev()
    h, w, oh, ow = 9, 21, 5, 11
    frames = torch.from_numpy(rand_frames(2, h, w, seed=3)).to(dev)
    hb, hw = (t.to(dev) for t in ops.resize_table(w, ow))
    vb, vw = (t.to(dev) for t in ops.resize_table(h, oh))
    ob, ow_ = (t.to(dev) for t in ops.resize_table(w, ow + 1))                 # another geometry's
    wide = torch.zeros((ow, 2 * hw.shape[1]), dtype=torch.int32, device=dev)
    bad = {
        "horizontal": [(None, hw), (hb, None), (hb.long(), hw), (hb, hw.float()), (hb.cpu(), hw), (hb, hw.cpu()),
                       (ob, hw), (hb, ow_), (hb[:-1], hw), (hb, hw[:, :-1]), (hb, wide[:, ::2]), (hb.reshape(-1), hw)],
        "vertical": [(None, vw), (vb, None), (vb.short(), vw), (vb, vw.cpu()), (hb, vw), (vb, hw), (vb, vw[:-1]), (vb.t(), vw)],
    }
    for dtype, fn in ((torch.float32, ops.frames_u8_to_f32), (torch.bfloat16, ops.frames_u8_to_bf16)):
        out = torch.full((2, 3, oh, ow), float("nan"), dtype=dtype, device=dev)
        for axis, pairs in bad.items():
            for b, wt in pairs:
                tabs = (b, wt, vb, vw) if axis == "horizontal" else (hb, hw, b, wt)
                with pytest.raises(ValueError, match=axis):
                    fn(frames, (oh, ow), tabs, MEAN, R.STD, out=out)
        # an axis that keeps its size takes no tables
        same = torch.full((2, 3, h, ow), float("nan"), dtype=dtype, device=dev)
        with pytest.raises(ValueError, match="vertical"):
            fn(frames, (h, ow), (hb, hw, vb, vw), MEAN, R.STD, out=same)
        with pytest.raises(ValueError, match="horizontal"):
            fn(frames, (oh, w), (hb, hw, vb, vw), MEAN, R.STD, out=torch.full((2, 3, oh, w), float("nan"), dtype=dtype, device=dev))
        with pytest.raises(ValueError, match="vertical"):                         # more than 63 taps
            fn(torch.zeros((1, 1985, 4, 3), dtype=torch.uint8, device=dev), (64, 4), (None, None, vb, vw), MEAN, R.STD)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(same).all())
        fn(frames, (oh, ow), (hb, hw, vb, vw), MEAN, R.STD, out=out)             # the right tables are taken
        torch.cuda.synchronize()
        assert not bool(torch.isnan(out).any())
