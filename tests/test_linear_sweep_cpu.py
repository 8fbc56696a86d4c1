"""Host-only tests of tests/linear_sweep_ref.py, the yardstick of tests/test_hip_linear_sweep.py: the references agree with each
other, the torch emulation of the engine's arithmetic passes the bar it stands in for, every planted defect is caught -- by the
metric, or by the NaN of a padding column -- on the case list that claims to pin it, ReLU cannot hollow a case out, every c_ref
measures something, and the case lists hold the values the route matrix names.  Nothing here needs a GPU."""
import math

import pytest
import torch

import linear_sweep_ref as R

_REF = {}


def _ref(spec):
    if spec.name in _REF:
        return _REF[spec.name]
    case = spec.build()
    made = (case, R.linear_ref(case))
    if case.m * case.n_out <= 1 << 18:                                    # the 112-row cases are large: not kept
        _REF[spec.name] = made
    return made


def _c(case, ref, out, out_relu):
    """The larger c of the two outputs of a launch (out_relu through the ReLU interval)."""
    c = R.c_of(out, ref.z, ref.S, relu=case.relu)
    return max(c, R.c_of(out_relu, ref.z, ref.S, relu=True)) if case.want_relu_copy else c


@pytest.mark.parametrize("name", R.ALL_LISTS)
def test_references_agree_and_the_emulation_meets_the_bar(name):
    """Per case of every list: the fp32 statement against float64 to 2e-6 in the max norm (the padding columns' NaN reaches
    neither), c_ref finite and non-zero over >= 2^16 outputs, no ReLU case clamps more than CLAMP_CAP of its outputs, and the
    emulation -- another summation order of the same products -- within M_START c_ref, the bar its kernels start at."""
    for spec in R.specs_of(name):
        case, ref = _ref(spec)
        y32 = R.linear_fp32(case)
        assert bool(torch.isfinite(ref.z).all()) and bool(torch.isfinite(y32).all()), spec.name
        assert float((y32.double() - ref.z).abs().max() / ref.z.abs().max()) < 2e-6, spec.name
        assert ref.ref_elems >= R.MIN_REF_ELEMS and math.isfinite(ref.c_ref) and ref.c_ref > 0.0, (spec.name, ref.c_ref)
        if case.relu:
            assert R.clamped_share(ref.z) <= R.CLAMP_CAP, (spec.name, R.clamped_share(ref.z))
        if case.want_relu_copy:
            assert 0.0 < R.clamped_share(ref.z) or case.m * case.n_out < 16, spec.name
        out, out_relu = R.engine_emulation(case, **R.emulation_args(spec))
        c = _c(case, ref, out, out_relu)
        print(f"{spec.name}: c_ref {ref.c_ref:.3f} c_emulation {c:.3f} clamped {R.clamped_share(ref.z):.2f}")
        assert c <= R.M_START * ref.c_ref, (spec.name, ref.c_ref, c)


def _applies(defect, spec, case):
    args = R.emulation_args(spec)
    if defect == "drop_last_kgroup_partial_m":
        return case.m % args["bm"] != 0
    if defect == "segment_off_by_quad":
        return len(case.sources) >= 2
    if defect == "res2_with_res_idx":
        return case.res_mode == "two"
    if defect == "relu_copy_before_residual":
        return case.want_relu_copy and case.res_mode != "none"
    if defect == "no_bias_on_split":
        return spec.sk and case.bias is not None
    if defect == "pad_quad":
        return any(s.ld > s.width for s in case.sources)
    if defect == "fold_restart_without_add":
        steps, fold_steps = case.k // args["bk"], (args["fold_k"] // args["bk"]) & ~1
        return args["fold_k"] >= 2 * args["bk"] and steps > fold_steps + 1
    return True


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_planted_defect_is_caught_on_the_list_that_pins_it(defect):
    """Every case of the pinning list that the defect can touch fails c <= M_START c_ref with the defect planted (a NaN read from a
    padding column or a moat counts: c is infinite, and on the GPU harness_findings reports the non-finite output), and passes
    without it."""
    touched = 0
    for spec in R.specs_of(R.PINNED_BY[defect]):
        case, ref = _ref(spec)
        if not _applies(defect, spec, case):
            continue
        touched += 1
        bar = R.M_START * ref.c_ref
        assert _c(case, ref, *R.engine_emulation(case, **R.emulation_args(spec))) <= bar, spec.name
        c_bad = _c(case, ref, *R.engine_emulation(case, defect=defect, **R.emulation_args(spec)))
        print(f"{defect} on {spec.name}: c {c_bad:.3g} against the bar {bar:.3g}")
        assert c_bad > bar, (defect, spec.name, c_bad, bar)
    assert touched >= 1, f"no case of {R.PINNED_BY[defect]} can show {defect}"


def test_the_old_bar_misses_what_the_new_one_catches():
    """The max-norm rel_err < 1e-5 of the earlier tests passes three cleared mantissa bits and a wrong element of small magnitude;
    the element-wise bar fails both."""
    spec = R.mantissa_specs()[1]
    case, ref = _ref(spec)
    good, _ = R.engine_emulation(case, **R.emulation_args(spec))
    y32 = R.linear_fp32(case)
    rel = lambda y: float((y - y32).abs().max() / y32.abs().max())
    bad = R.clear_low_bits(good, 3)
    assert rel(bad) < 1e-5 and R.c_of(bad, ref.z, ref.S) > R.M_START * ref.c_ref
    plain = R.specs_of("buffer4_bk16")[2]
    case, ref = _ref(plain)
    good, _ = R.engine_emulation(case, **R.emulation_args(plain))
    y32 = R.linear_fp32(case)
    i = int(ref.S.reshape(-1).argmin())
    bad = good.clone().reshape(-1)
    bad[i] += float(ref.S.reshape(-1)[i]) * 3e-6                         # 50 u S on the element with the smallest S
    bad = bad.reshape(good.shape)
    assert rel(bad) < 1e-5 and R.c_of(bad, ref.z, ref.S) > R.M_START * ref.c_ref


def test_index_patterns():
    for pattern in R.PATTERNS:
        rows = R.pattern_rows(pattern, 65)
        idx = R.index_pattern(pattern, 65, rows, 3)
        assert idx.dtype == torch.int64 and idx.shape == (65,) and 0 <= int(idx.min()) and int(idx.max()) < rows
    assert torch.equal(R.index_pattern("reversed", 5, 5, 0), torch.tensor([4, 3, 2, 1, 0]))
    assert int(R.index_pattern("last", 7, 6, 0).min()) == 5 and R.pattern_rows("rows1", 9) == 1
    r = R.index_pattern("random", 65, 35, 3)
    assert r.unique().numel() < 65                                        # repeats


def test_padding_columns_hold_nan_and_the_references_do_not_read_them():
    case = R.specs_of("general_lds")[1].build()
    assert case.res_mode in ("gathered", "two") and case.ldr > case.n_out
    assert bool(torch.isnan(case.res1[:, case.n_out:]).all()) and bool(torch.isfinite(case.res1[:, :case.n_out]).all())
    padded = [s for s in case.sources if s.ld > s.width]
    assert padded and all(bool(torch.isnan(s.a[:, s.width:]).all()) for s in padded)
    z, S = R.linear_exact(case)
    assert bool(torch.isfinite(z).all()) and bool((S > 0).all())


@pytest.mark.parametrize("route", list(R.TILE_ROUTES))
def test_route_lists_hold_the_matrix(route):
    """Every M and N the matrix names, the three arrangements, the five index patterns on gathered sources, the four residual modes
    (the gathered ones with ldr > n_out), out_relu, ReLU, both regimes, ld > width in every case -- on every tile-engine route."""
    specs = R.specs_of(route)
    bm, bn = R.TILES[dict(specs[0].keys)["TILE"]]
    assert {s.m for s in specs} == {1, bm - 1, bm, bm + 1, 2 * bm + 1}
    ns = {s.n_out for s in specs}
    assert ns >= ({1, 3, 70} if route == "general_direct" else {4, bn - 4, bn, bn + 4})
    assert all(n % 4 for n in ns) if route == "general_direct" else not any(n % 4 for n in ns)
    kinds = {tuple(k for k, *_ in s.srcs) for s in specs}
    assert any(set(k) == {"plain"} for k in kinds) and any(set(k) == {"gather"} for k in kinds) and ("gather", "plain", "gather") in kinds
    assert {p for s in specs for kind, _, _, p in s.srcs if kind == "gather"} == set(R.PATTERNS)
    assert {s.res_mode for s in specs} == set(R.RES_MODES) and all(s.ldr > s.n_out for s in specs if s.res_mode in ("gathered", "two"))
    assert any(s.relu for s in specs) and any(s.want_relu_copy for s in specs) and {s.dist for s in specs} == set(R.DISTS)
    assert all(any(ld > wd for _, wd, ld, _ in s.srcs) for s in specs)
    assert {tuple(wd for _, wd, _, _ in s.srcs) for s in specs} >= set(R.TILE_ROUTES[route][2][-2:])
    for s in specs:                                                       # what keeps a case on its loader (direct epilogue: N % 4 alone)
        widths = [wd for _, wd, _, _ in s.srcs]
        bk = dict(s.expect)["BK"]
        if route != "general_direct":
            assert all(wd % bk == 0 for wd in widths) == (dict(s.expect)["loader"] == "buffer")


def test_fold_and_streamk_lists():
    ks = {(dict(s.keys)["FOLD_K"], s.name.split("-")[1], s.k) for s in R.fold_specs()}
    for fold in R.FOLDS:
        f = fold or 256
        assert {(fold, "buffer4", k) for k in (f - 16, f, f + 16, 2 * f + 16)} <= ks
        assert {(fold, "buffer8", k) for k in (f - 32, f, f + 32, 2 * f + 32)} <= ks
        assert {(fold, "linear112", k) for k in (f - 32, f, f + 32, 2 * f + 32) if k >= 64} <= ks
    for inkernel in (False, True):
        specs = R.streamk_specs(inkernel)
        assert {s.k for s in specs} == {512, 516, 600, 1056} and all(s.m == 333 and s.n_out in (99, 100) and s.sk for s in specs)
        assert {dict(s.expect)["loader"] for s in specs} == {"general", "buffer"} and {dict(s.expect)["BK"] for s in specs} == {16, 32}
        assert all(s.k >= 32 * dict(s.expect)["BK"] for s in specs)
        assert {s.res_mode for s in specs} == set(R.RES_MODES)
