"""Host side of the frame-transform sweep (no GPU): the reference against Pillow on every case, the C table builder at the
size limit, the planted defects (the inputs discriminate), every case's tile plan as the launcher records it
(ops.frames_plan), and the planner's invariants over a cross product of axis pairs."""
import numpy as np
import pytest

import frames_sweep_ref as R
from test_hip_frames import MEAN, ref_normalize, ref_table

CASE_IDS = [c.id for c in R.CASES]
LDS_BUDGET = 48 * 1024


@pytest.mark.parametrize("case", R.CASES, ids=CASE_IDS)
def test_reference_equals_pillow(case):
    Image = pytest.importorskip("PIL.Image")
    frames = R.case_inputs(case)
    pil = np.stack([np.asarray(Image.fromarray(f, "RGB").resize((case.out_w, case.out_h), Image.BILINEAR)) for f in frames])
    assert np.array_equal(R.case_resized(case), pil), case.id


@pytest.mark.parametrize("case", R.CASES, ids=CASE_IDS)
def test_defect_free_variant_is_the_reference(case):
    frames = R.case_inputs(case)
    assert np.array_equal(R.variant_resize(frames, case.out_h, case.out_w), R.case_resized(case)), case.id


def test_c_table_builder_at_the_limits():
    from relpose_gnn_amd import ops
    for n_in, n_out in [(1984, 64), (64, 1984), (1, 7), (7, 1), (248, 8)]:
        b, w = ops.resize_table(n_in, n_out)
        rb, rw = ref_table(n_in, n_out)
        assert tuple(w.shape) == (n_out, R.taps(n_in, n_out))
        assert np.array_equal(b.numpy(), rb) and np.array_equal(w.numpy(), rw), (n_in, n_out)
    assert ops.resize_table(1984, 64)[1].shape[1] == 63              # the most taps the kernel takes
    with pytest.raises(ValueError):                                   # 65 taps
        ops.resize_table(1985, 64)
    ops.frames_plan(1984, 10, 64, 10)
    ops.frames_plan(10, 1984, 10, 64)
    with pytest.raises(ValueError):
        ops.frames_plan(1985, 10, 64, 10)
    with pytest.raises(ValueError):
        ops.frames_plan(10, 1985, 10, 64)
    for bad in [(0, 4, 4, 4), (4, 0, 4, 4), (4, 4, 0, 4), (4, 4, 4, 0), (-1, 4, 4, 4)]:
        with pytest.raises(ValueError):
            ops.frames_plan(*bad)


@pytest.mark.parametrize("defect", R.RESIZE_DEFECTS)
def test_resize_defects_are_detected_on_every_case(defect):
    """A planted defect changes at least one output byte on at least one input of every case it can apply to: a kernel with
    that defect cannot pass the sweep on any such case."""
    applied = 0
    for case in R.CASES:
        if not R.defect_applies(defect, case):
            continue
        applied += 1
        frames = R.case_inputs(case)
        changed = int((R.variant_resize(frames, case.out_h, case.out_w, defect) != R.case_resized(case)).sum())
        assert changed > 0, (defect, case.id)
    want = {"vertical_first": sum(c.passes == "both" for c in R.CASES) - 1,          # all but 1x1 -> 5x7
            "no_rounding": sum(c.passes != "none" for c in R.CASES) - 1,
            "one_tap_fewer": sum(c.passes != "none" for c in R.CASES)}[defect]
    assert applied == want, (defect, applied, want)


@pytest.mark.parametrize("defect", R.NORM_DEFECTS)
def test_normalisation_defects_are_detected(defect):
    good, bad = R.variant_norm_table(MEAN, R.STD), R.variant_norm_table(MEAN, R.STD, defect)
    assert int((good.view(np.int32) != bad.view(np.int32)).sum()) > 0, defect
    # the table is what ref_normalize computes for every byte
    ramp = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, None, :, None], (1, 1, 256, 3))
    assert np.array_equal(ref_normalize(ramp, MEAN, R.STD)[0, :, 0, :].view(np.int32), good.view(np.int32))


@pytest.mark.parametrize("case", R.CASES, ids=CASE_IDS)
def test_case_takes_the_plan_it_exists_for(case):
    from relpose_gnn_amd import ops
    got = R.derived(ops.frames_plan(case.in_h, case.in_w, case.out_h, case.out_w), case)
    assert got["need_h"] == case.need_h and got["need_v"] == case.need_v
    assert {k: got[k] for k in case.plan} == case.plan, (case.id, case.why, got)


def test_the_list_covers_every_plan_property():
    from relpose_gnn_amd import ops
    plans = [(c, R.derived(ops.frames_plan(c.in_h, c.in_w, c.out_h, c.out_w), c)) for c in R.CASES]
    assert {p["tr"] for c, p in plans if c.out_h >= p["tr"]} >= {16, 8, 4, 2, 1}
    assert any(p["tr"] == c.out_h < 16 for c, p in plans), "a clamped tr"
    for passes in ("h", "v", "both"):
        assert any(c.passes == passes and p["tiles_y"] > 1 and p["last_rows"] < p["tr"] for c, p in plans), ("short row tile", passes)
    assert any(p["tiles_x"] > 1 and p["last_cols"] < p["tc"] for c, p in plans), "a short last column tile"
    for passes in ("h", "v", "both", "none"):
        assert any(c.passes == passes and p["tiles_x"] > 1 for c, p in plans), ("column tiles", passes)
        assert any(c.passes == passes and p["tiles_x"] == 1 for c, p in plans), ("full width", passes)
    assert any(p["taps_h"] == 63 for c, p in plans) and any(p["taps_v"] == 63 for c, p in plans)
    assert any(p["taps_h"] == 63 and c.passes == "h" for c, p in plans) and any(p["taps_v"] == 63 and c.passes == "v" for c, p in plans)
    assert any(c.in_h == 1 and c.need_v for c, p in plans) and any(c.out_h == 1 and c.need_v for c, p in plans)
    assert any(p["pitch"] == 32 and 3 * c.in_w < 16 for c, p in plans), "a row segment shorter than one chunk"


# about 30 axis pairs: identity, the limits on both sides, 1-pixel axes, large upscales, the cases' own axes
AXES = [(1, 1), (2, 2), (3, 3), (16, 16), (300, 300), (4000, 4000), (20000, 20000),
        (1984, 64), (248, 8), (62, 2), (31, 1), (7, 1), (5000, 200), (3000, 911), (4000, 500), (1920, 455), (1100, 1000),
        (640, 341), (600, 35), (700, 100), (1000, 40), (70, 33), (21, 11), (9, 5), (257, 256),
        (1, 7), (1, 5000), (3, 1000), (64, 1984), (53, 366), (17, 40), (255, 256)]


def _spans(n_in, n_out, tile, tables):
    """Source samples read by each tile of ``tile`` outputs, from ops.resize_table's bounds (the tile itself when the axis
    keeps its size)."""
    o0 = np.arange(0, n_out, tile)
    o1 = np.minimum(o0 + tile, n_out)
    if n_in == n_out:
        return o1 - o0
    b = tables[n_in, n_out]
    return (b[o1 - 1, 0] + b[o1 - 1, 1]) - b[o0, 0]


def test_planner_invariants_over_the_cross_product():
    """Every geometry the size check admits gets a plan whose tiles cover the output, whose staging area holds every tile's
    source rows and row segments (wherever a segment starts inside a 16-byte chunk), and whose LDS image is within 48 KiB.
    The last holds for all of them, as 3072 + 260 + 260 + 63 * 208 + 189 bytes for a 1 x 1 tile at 63 taps on both axes says
    it must, so make_plan's second pass with a 64 KiB budget was dead code: it has been removed."""
    from relpose_gnn_amd import ops
    tables = {(i, o): ops.resize_table(i, o)[0].numpy().astype(np.int64) for i, o in AXES if i != o}
    worst = 0
    for in_h, out_h in AXES:
        for in_w, out_w in AXES:
            p = ops.frames_plan(in_h, in_w, out_h, out_w)            # ValueError: no plan
            geom = (in_h, in_w, out_h, out_w, p)
            assert p["need_h"] == (in_w != out_w) and p["need_v"] == (in_h != out_h), geom
            assert 1 <= p["tr"] <= min(16, out_h) and 1 <= p["tc"] <= out_w, geom
            assert p["tr"] in (16, 8, 4, 2, 1) or p["tr"] == out_h, geom
            assert (p["tiles_y"] - 1) * p["tr"] < out_h <= p["tiles_y"] * p["tr"], geom
            assert (p["tiles_x"] - 1) * p["tc"] < out_w <= p["tiles_x"] * p["tc"], geom
            assert p["rows_max"] >= int(_spans(in_h, out_h, p["tr"], tables).max()), geom
            cols = int(_spans(in_w, out_w, p["tc"], tables).max())
            assert p["pitch"] % 16 == 0 and p["pitch"] >= 16 * -(-(3 * cols + 15) // 16), geom
            assert p["lds_bytes"] >= 3072 + p["rows_max"] * p["pitch"], geom
            assert p["lds_bytes"] <= LDS_BUDGET, geom
            worst = max(worst, p["lds_bytes"])
    assert worst > LDS_BUDGET - 2048                                  # the cross product does come close to the budget
