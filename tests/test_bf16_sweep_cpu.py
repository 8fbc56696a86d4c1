"""The bf16 sweep's own tests (tests/bf16_sweep_ref.py; the kernels are held to it by tests/test_hip_bf16_sweep.py): the restated
dispatcher rule on the shapes the older bf16 tests name, the reach of the enumerated case lists, the 16-bit memory harness against
planted defects, the interval check against defects planted in a CPU statement of the convolution, and per case the conditions
the GPU test relies on -- the fp32 CPU evaluation rounded once passes, at most AMBIGUOUS_CAP of the elements have two acceptable
answers, c_ref is a maximum over at least 2^16 outputs.  No GPU."""
import pytest
import torch

import bf16_rounding as R
import bf16_sweep_ref as B

CUS = 256


def test_model_defaults_are_the_library_s():
    from relpose_gnn_amd import ops
    for key, value in B.BF16_DEFAULTS.items():
        assert ops.tuning_default(key) == value, key


# n, h, w, cin, cout, k, stride, pad of tests/test_hip_bf16_rounding.py's SHAPES, the keys its tests run them under, and the route
# worked out BY HAND from csrc/conv_bf16.hip for 256 CUs (patch rows / pieces / LDS in the comments)
_L1, _L2, _L3, _L4 = (40, 56, 56, 64, 64, 3, 1, 1), (24, 28, 28, 128, 128, 3, 1, 1), (9, 14, 14, 256, 256, 3, 1, 1), (8, 7, 7, 512, 512, 3, 1, 1)
_TINY, _PERSIST = (2, 5, 3, 128, 128, 3, 1, 1), (100, 40, 40, 64, 64, 3, 1, 1)
_EXISTING = [
    ("layer1 default", {}, _L1, ("patch", 512, 64, 4, 1)),                        # 125,440 rows; 15 x 64 slots = 60 pieces, 137 KiB
    ("layer2 default", {}, _L2, ("dma", 256, 128, 7, 1)),                         # 18,816 rows: below 65,536, no patch by shape
    ("layer2 patch=2", {"BF16_PATCH": 2}, _L2, ("patch", 512, 128, 4, 1)),        # 24 x 32 slots = 48 pieces; 37 tiles: no tail
    ("layer2 patch=3", {"BF16_PATCH": 3}, _L2, ("patch", 256, 128, 3, 1)),
    ("layer2 patch=12", {"BF16_PATCH": 12}, _L2, ("patch", 512, 128, 3, 1)),
    ("layer3 patch=2", {"BF16_PATCH": 2}, _L3, ("patch", 256, 128, 3, 1)),        # 7 tiles of 256 x 256 are no three quarters of the CUs
    ("layer4 patch=2", {"BF16_PATCH": 2}, _L4, ("patch", 256, 128, 3, 1)),        # 52 x 16 slots = 52 pieces
    ("layer1 patch=12", {"BF16_PATCH": 12}, _L1, ("patch", 512, 64, 3, 1)),
    # tiny_img: 244 pieces on 512 x 128, 125 on 256 x 128 -- no patch tile takes it; 30 rows are below the LDS-DMA kernel's 8192
    ("tiny_img patch=2", {"BF16_PATCH": 2}, _TINY, ("interleaved", 64, 64, 64, 1)),
    ("tiny_img patch=3", {"BF16_PATCH": 3}, _TINY, ("interleaved", 64, 64, 64, 1)),
    ("tiny_img patch=12", {"BF16_PATCH": 12}, _TINY, ("interleaved", 64, 64, 64, 1)),
    ("persist_ragged", {"BF16_PATCH": 2, "BF16_PERSIST": 1}, _PERSIST, ("patch_persistent", 512, 64, 4, 1)),     # 313 tiles > 256
    ("layer1 persist", {"BF16_PATCH": 2, "BF16_PERSIST": 1}, _L1, ("patch", 512, 64, 4, 1)),                     # 245 tiles: one round
    ("tail_l2", {"BF16_TAIL": 3}, (400, 28, 28, 128, 128, 3, 1, 1), ("patch", 512, 128, 4, 2)),     # 613 tiles: 512 + 201 of 256 rows
    ("tail_l3", {"BF16_TAIL": 3}, (340, 14, 14, 256, 256, 3, 1, 1), ("patch", 256, 256, 4, 2)),     # 261 tiles: 256 + 7 of 160 rows
    ("tail_l3_res", {"BF16_TAIL": 3}, (400, 14, 14, 256, 256, 3, 1, 1), ("patch", 256, 256, 4, 2)),
    ("tail_l2 tail=0", {"BF16_TAIL": 0}, (400, 28, 28, 128, 128, 3, 1, 1), ("patch", 512, 128, 4, 1)),
    ("ragged_s2 dma3", {"BF16_DMA": 13}, (3, 13, 17, 192, 72, 3, 2, 1), ("dma", 128, 128, 3, 1)),
    ("cin96 dma7", {"BF16_DMA": 17}, (5, 9, 11, 96, 40, 3, 1, 1), ("dma", 256, 128, 7, 1)),         # Cin % 32 == 0
    ("cin96 dma0", {"BF16_DMA": 10}, (5, 9, 11, 96, 40, 3, 1, 1), ("general", 64, 64, 32, 1)),      # Cin % 64 != 0: neither DMA nor interleaved
    ("fc", {}, (37, 1, 1, 512, 2048, 1, 1, 0), ("interleaved", 64, 64, 64, 1)),                      # 16 tiles of 128 x 128 < 256
]


@pytest.mark.parametrize("name,keys,shape,want", _EXISTING, ids=[e[0].replace(" ", "_") for e in _EXISTING])
def test_rule_on_the_shapes_of_the_older_tests(name, keys, shape, want):
    assert B.bf16_route(keys, *shape, False, False, CUS) == want


def test_tiny_img_needs_more_pieces_than_any_patch_tile_takes():
    assert B.patch_plan(512, 5, 3)[2] == 244 and B.patch_plan(256, 5, 3)[2] == 125


def test_smallest_maps_of_the_patch_tiles():
    """The enumeration's answer to 'what is the smallest map this tile takes' (smallest H W, then smallest H), per tile."""
    def smallest(bm, bn, ns, cout):
        acc = [(h * w, h, w) for h in range(1, 17) for w in range(1, 63)
               if B.patch_accepts(bm, bn, ns, False, h, w, 64, cout, 100000, True, CUS)]
        return min(acc)[1:]
    assert smallest(256, 128, 3, 128) == (1, 13)
    # the 128-row tail tile alone takes 1 x 7 (20 rows + 2 x 19 image gaps + 2 = 60 patch rows of 16 slots: 60 pieces); a launch
    # reaches it only behind a 512-row main tile, whose smallest map is 4 x 13
    assert smallest(128, 128, 3, 128) == (1, 7)
    assert smallest(160, 256, 3, 256) == (1, 10) and smallest(256, 256, 3, 256) == (2, 10)
    assert smallest(512, 128, 3, 128) == (4, 13) and smallest(512, 64, 4, 64) == (4, 13)
    assert B.block_plan(3, 5, 14) is not None and B.block_plan(3, 4, 14) is None and B.block_plan(3, 5, 13) is None


@pytest.mark.parametrize("name", list(B.PATCH_ROUTES))
def test_patch_route_has_its_cases(name):
    spec, cases = B.PATCH_ROUTES[name], B.patch_cases(name, CUS)
    bm, bn = spec["want"][1], spec["want"][2]
    acc = B.patch_accepted(name, CUS)
    whys = {c.why for c in cases}
    assert "couttail" in whys and ("minHW" in whys or "minH" in whys)
    for c in cases:
        assert c.expected(CUS) == spec["want"], c.id
        assert (c.n * c.h * c.w) % bm, "a ragged last tile"
        assert c.n * c.h * c.w > bm, "more than one workgroup"
    assert min(c.h * c.w for c in cases) == min(h * w for h, w, _, _ in acc)
    assert max(B.patch_plan(bm, c.h, c.w)[2] for c in cases) == max(p for _, _, _, p in acc)
    assert min(c.h for c in cases) == min(a[0] for a in acc) and min(c.w for c in cases) == min(a[1] for a in acc)
    assert any(B.images_in_widest_tile(c.n * c.h * c.w, c.h * c.w, bm) >= 3 for c in cases)
    tail = [c for c in cases if c.why == "couttail"]
    assert tail and all(c.cout % bn and c.cout % 4 == 0 for c in tail)
    # the neighbours the rule refuses: one row or one column less than the smallest map goes elsewhere
    h, w = min(((c.h, c.w) for c in cases), key=lambda e: e[0] * e[1])
    for hh, ww in ((h - 1, w), (h, w - 1)):
        if hh >= 1 and ww >= 1 and (hh, ww) not in {(a[0], a[1]) for a in acc}:
            n = -(-spec["rows"](CUS) // (hh * ww)) + 1
            assert B.bf16_route(spec["keys"], n, hh, ww, 64, spec["cout"], 3, 1, 1, False, False, CUS) != spec["want"]


@pytest.mark.parametrize("name", list(B.ANY_ROUTES))
def test_any_route_has_its_cases(name):
    cases = B.any_cases(name)
    with_c7 = name in B.C7S2_ROUTES
    assert len(cases) == (len(B.ANY_KINDS) - (not with_c7)) * len(B.ANY_EXTENTS)
    reach = [c for c in cases if B.any_reaches(c, CUS)]
    assert {(c.h, c.w) for c in reach if c.why == "c3s1"} == set(B.ANY_EXTENTS)
    assert {(c.h, c.w) for c in reach if c.why == "c3s2"} == set(B.ANY_EXTENTS)
    c7 = [c for c in cases if c.why == "c7s2"]
    assert {(c.h, c.w) for c in c7} == (set(B.ANY_EXTENTS) if with_c7 else set())
    if name.startswith("general"):
        assert all(c in reach for c in c7)                                                   # Cin = 8: the general kernel alone
    else:
        assert all(c.expected(CUS) == ("general", 64, 64, 32, 1) for c in c7)                # the fall-back, once per family
    bf16 = {(c.res, c.relu, c.lean) for c in cases if not c.out_f32}
    assert len(bf16) == 8 and sum(c.out_f32 for c in cases) == (4 if with_c7 else 3)
    assert any(c.h * c.w == 1 and c.pad for c in reach)                                       # a window that is padding but for one tap


def test_dma_k_step_eligibility():
    for cfg, (bm, bn, bk) in B.DMA_CONFIGS.items():
        for cin in (32, 64, 96, 8):
            got = B.bf16_route({"BF16_DMA": 10 + cfg, "BF16_PATCH": 0}, 3, 7, 7, cin, 72, 3, 1, 1, False, False, CUS)
            assert (got == ("dma", bm, bn, cfg, 1)) == (cin % bk == 0), (cfg, cin, got)


def test_pair_and_block_rules():
    for n, h, w in B.PAIR_SHAPES:
        assert B.pair_route({}, n, h, w, 64, 128, 3, 2, 1, CUS) == ("pair", 256, 128, 7, 1)
        assert B.pair_route({}, n, h, w, 128, 260, 3, 2, 1, CUS) == ("pair", 256, 128, 7, 1)          # 33 x 2 tiles of 256 x 256: too few
        assert B.pair_route({"BF16_PAIR": 0}, n, h, w, 64, 128, 3, 2, 1, CUS) == B.NONE
    assert B.pair_route({}, 8191, 1, 1, 64, 128, 3, 2, 1, CUS) == B.NONE and B.pair_route({}, 8192, 1, 1, 48, 128, 3, 2, 1, CUS) == B.NONE
    assert B.pair_route({}, 400, 28, 28, 128, 256, 3, 2, 1, CUS) == ("pair", 256, 256, 0, 1)          # 307 tiles of 256 x 256
    assert B.block_route({"BF16_FUSE_BLOCK": 1}, 3, 5, 14, CUS) == ("block", 512, 64, 4, 1)
    assert B.block_route({"BF16_FUSE_BLOCK": 3}, 3, 5, 14, CUS) == ("block", 512, 64, 4, 1)            # one tile: nothing to walk
    assert B.block_route({"BF16_FUSE_BLOCK": 3}, 96, 56, 56, CUS) == ("block_persistent", 512, 64, 4, 1)
    assert B.block_route({"BF16_FUSE_BLOCK": 5}, 3, 56, 56, CUS) == ("block_two_group", 512, 64, 5, 1)
    assert B.block_route({"BF16_FUSE_BLOCK": 5}, 3, 5, 14, CUS) == ("block_two_group", 512, 64, 5, 1)  # 155 KiB + a fifth stage = 159 KiB
    tight = [(h, w) for h in range(1, 41) for w in range(4, 63) if (B.block_plan(3, h, w) or {"lds": 0})["lds"] + 4096 > B.LDS_MAX]
    assert tight and all(B.block_route({"BF16_FUSE_BLOCK": 5}, 3, h, w, CUS) == ("block", 512, 64, 4, 1) for h, w in tight)
    assert B.block_plan(1, 30, 120)["strips"] == 2 and B.block_plan(1, 30, 121) is None and B.block_plan(1, 30, 3) is None
    # 64 x 86: views of 43 + 2 columns, 48 slots a row; 639 // 45 + 2 = 16 rows + 2 (a second image) + 2 = 20 patch rows: 60 pieces
    assert B.block_plan(2, 64, 86) == {"strips": 2, "view": 45, "pieces": 60, "lds": 140288, "tiles": 23}
    assert B.block_plan(3, 30, 63)["strips"] == 2 and B.block_plan(3, 30, 62)["strips"] == 1


# ----------------------------------------------------------------------------------------------------------------------
# the harness against planted defects
# ----------------------------------------------------------------------------------------------------------------------
def _written(shape=(2, 3, 5, 8)):
    out = B.Moated16(shape, "cpu")
    out.t.copy_(torch.randn(shape).bfloat16())
    return out


def test_harness_layout():
    x = torch.randn(2, 3, 5, 8).bfloat16()
    b = B.Moated16(x.shape, "cpu", x)
    assert b.moat * 4 >= 64 * 1024 and b.moat % 64 == 0 and b.ptr() % 256 == b.raw.data_ptr() % 256
    assert torch.equal(b.t, x) and b.moats_intact() and bool(torch.isnan(b.halfwords_before(8).float()).all())
    wide = B.Moated16((1, 2, 3000, 64), "cpu")
    assert wide.moat * 4 >= 4 * 3000 * 64 * 2
    fresh = B.Moated16((2, 3, 5, 8), "cpu")
    assert fresh.unwritten() == 240 and bool(torch.isnan(fresh.t.float()).all())
    done = _written()
    assert B.harness_findings([b], done) == []


def test_harness_catches_a_halfword_store_into_a_moat():
    for where in (-1, 0):                                  # the half-word in front of the tensor, the one behind it
        out = _written()
        halves = out.raw.view(torch.int16)
        halves[2 * out.moat + (out.numel if where == 0 else -1)] = 0x3F80
        assert B.harness_findings([], out) == ["the output's moat was written"]
    x = B.Moated16((2, 3, 5, 8), "cpu", torch.zeros(2, 3, 5, 8).bfloat16())
    x.raw.view(torch.int16)[7] = 0
    assert B.harness_findings([x], _written()) == ["the moat of input 0 was written"]


def test_harness_catches_a_skipped_halfword():
    out = B.Moated16((2, 3, 5, 8), "cpu")
    y = torch.randn(2, 3, 5, 8).bfloat16()
    out.t.copy_(y)
    out.raw.view(torch.int16)[2 * out.moat + 77] = B.PAYLOAD16            # one half-word of a word keeps the pattern
    found = B.harness_findings([], out)
    assert "1 output elements were never written" in found


def test_harness_catches_a_load_one_pixel_left_of_the_image():
    """A kernel whose left padding tap of (image 0, row 0, column 0) reads the pixel in front of the tensor reads the moat's NaN."""
    op = B.conv_operands(2, 3, 5, 8, 8, 3, 1, 1, False)
    xb = B.Moated16(op.x.shape, "cpu", op.x)
    x = torch.nn.functional.pad(op.x.float().permute(0, 3, 1, 2), (1, 1, 1, 1))
    x[0, :, 1, 0] = xb.halfwords_before(8).float()
    y = torch.nn.functional.conv2d(x, op.w.float().permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    out = B.Moated16(y.shape, "cpu")
    out.t.copy_(y.bfloat16())
    assert B.harness_findings([xb], out) == ["the output is not finite"]


# ----------------------------------------------------------------------------------------------------------------------
# the interval check against defects planted in the CPU statement
# ----------------------------------------------------------------------------------------------------------------------
def _case(route, why):
    return next(c for c in B.patch_cases(route, CUS) if c.why == why)


@pytest.mark.parametrize("route,why", [("p256x128s3", "minH"), ("p512x64s4", "minW"), ("p256x128s3", "pieces")])
def test_interval_catches_a_padding_tap_read_from_the_neighbouring_image(route, why):
    c = _case(route, why)
    op = B.case_operands(c)
    good = R.examine(B.conv_cpu(op, 1, 1, c.relu), op.ref, c.relu, c_ref=op.c_ref)
    bad = R.examine(B.conv_cpu(op, 1, 1, c.relu, defect="neighbour_tap"), op.ref, c.relu, c_ref=op.c_ref)
    assert good["bad"] == 0 and bad["bad"] > 0.2 * bad["n"] / c.w           # every first column (those ReLU does not clamp)


@pytest.mark.parametrize("route,why", [("p256x128s3", "minH"), ("p512x128s3", "pieces"), ("p512x64s4", "couttail")])
def test_interval_catches_a_dropped_last_row_of_a_ragged_tile(route, why):
    c = _case(route, why)
    op = B.case_operands(c)
    bm = B.PATCH_ROUTES[route]["want"][1]
    bad = R.examine(B.conv_cpu(op, 1, 1, False, defect="drop_last_row", tile_rows=bm), op.ref, False, c_ref=op.c_ref)
    assert 0 < bad["bad"] <= c.cout


# ----------------------------------------------------------------------------------------------------------------------
# per case: what the GPU test relies on
# ----------------------------------------------------------------------------------------------------------------------
def _by_operands():
    groups = {}
    for c in B.all_cases(CUS):
        groups.setdefault((c.n, c.h, c.w, c.cin, c.cout, c.k, c.stride, c.pad, c.res), []).append(c)
    return groups


_GROUPS = _by_operands()


@pytest.mark.parametrize("key", list(_GROUPS), ids=lambda k: "n{}h{}w{}c{}o{}k{}s{}p{}r{:d}".format(*k))
def test_case_conditions(key):
    """One convolution of the lists (shared by every route and epilogue that runs it): c_ref over >= 2^16 outputs and above
    zero, and for each ReLU setting a case uses, the fp32 evaluation rounded once is inside the interval everywhere with at most
    AMBIGUOUS_CAP of the elements ambiguous (R.check raises otherwise)."""
    cases = _GROUPS[key]
    op = B.case_operands(cases[0])
    assert op.ref_elems >= B.MIN_REF_ELEMS and op.c_ref > 0.0
    for relu in sorted({c.relu for c in cases}):
        rep = R.check(B.conv_cpu(op, cases[0].stride, cases[0].pad, relu), op.ref, relu, c_ref=op.c_ref, what=cases[0].id)
        assert rep["bad"] == 0 and rep["ambiguous"] <= R.AMBIGUOUS_CAP


@pytest.mark.parametrize("h,w", B.STEM_SIZES)
def test_stem_case_conditions(h, w):
    """The stem cases: the fp32 evaluation, ReLU, max-pool, one rounding -- inside the pooled interval, the cap met."""
    x, wt, scale, shift, ref, c_ref = B.stem_reference(h, w)
    y = R.bf16_rne(B.stem_pool(torch.relu(ref.y32)))
    rep = R.check(y, ref, True, post=B.stem_pool, c_ref=c_ref, what=f"stem {h}x{w}")
    assert rep["bad"] == 0 and rep["ambiguous"] <= R.AMBIGUOUS_CAP and c_ref >= ref.c_ref > 0.0


def test_streaming_statements():
    """The average pool's stated order equals torch's mean up to the fp32 sum's rounding, and is exact on one pixel."""
    x = torch.randn(3, 1, 16).bfloat16()
    assert torch.equal(B.avgpool_ordered_bf16(x), x[:, 0])
    x = torch.randn(5, 49, 16).bfloat16()
    assert float((B.avgpool_ordered_bf16(x).float() - x.float().mean(1)).abs().max()) < 2.0 ** -8
    for h, w in B.FWD_SIZES:
        n = B.fwd_large_n(h, w)
        (h1, w1), (h2, w2) = B.E.layer_extents(h, w)[:2]
        assert n * h1 * w1 >= 8192 and n * h2 * w2 >= 8192 and ((B.block_plan(n, h1, w1) is not None) == ((h, w) != (17, 17)))
