"""The fp32 Linear engine -- rpg_linear_gather_f32 / rpg_linear_gather_ex_f32: the tile engine of csrc/gemm_engine.inc on its general
and buffer loaders, four and eight waves, K steps 16 and 32, the direct and the LDS epilogue, stream-K with the fix-up launch and
with the in-kernel combine, and the exact-fit linear112 / linear112k2 kernels of csrc/gemm_f32.hip -- held to float64 per element
inside the memory harness of the encoder sweep (tests/linear_sweep_ref.py; its own tests are test_linear_sweep_cpu.py).

What the suite did not run before.  Gathered sources on the buffer loader (GatherLoaderB with idx != NULL: only the composite GNN
forward got there, because rpg_linear_gather_f32 passes no row counts and the launcher then takes the general loader); gathered
residual rows, a second gathered residual, ldr > n_out and out_relu anywhere but the 112-row kernels -- the tile engine's two
epilogues, the stream-K fix-up kernel, the in-kernel combine, ragged M and N; an A operand that is a column block of a wider
tensor on the tile engine; either side of the 2^31-byte guard that decides between 32-bit offsets and 64-bit pointers; a K at a
fold boundary, a fold length other than the default, and the fold's effect on the error per element.

Every case ASSERTS the route it claims from ops.gemm_last_route(), the launcher's own record of what it did (kernel, tile, K step,
waves, loader, epilogue, stream-K split and combine, fold length): the stream-K decision rests on the occupancy the runtime
reports, so a restatement of the rule in Python would be a guess.  A case that does not reach its route fails.

Every operand lies between two NaN moats in one allocation; the columns past a source's width (ld > width on at least one source of
every case) and past n_out in a gathered residual row hold NaN too, so a read one quad too far poisons an output and
harness_findings reports it.  out and out_relu lie between moats of a NaN pattern nobody computes: an unwritten element and a
stray store both show.  Index arrays are int64 and not moated.

The bar.  c_hip <= M c_ref per case (M = M_LINEAR, and the tighter M_FOLDED wherever the fold is on: below), c as in encoder_sweep_ref.py (|y - z| / (u S) before the activation, the interval
through a ReLU), c_ref that of F.linear in fp32 on the CPU (+ bias and residuals in the kernels' association) over >= 2^16 outputs,
never of a kernel.  A case with ReLU runs once with it and once without, out_relu is checked through the interval AND must be
max(out, 0) bit for bit.  Unmoved beside it: the earlier rel_err < 1e-5 against the fp32 CPU result.  M_LINEAR started at
encoder_sweep_ref.M_START = 4 for the reason given there (32x32x2 / 16x16x4 MFMA blocks, K cut into steps, folds and stream-K
slabs, against oneDNN's blocked sums); ceiling 8.  Every case prints c_ref, c_hip and their ratio and appends them to the file
RPG_SWEEP_RECORD names; profiles/linear_sweep_observed.json holds one such run on an MI355X.

Margins from that run.  One case missed the starting margin: K = 4096 on one 64x64 tile with the fold switched off
(RPG_TUNE_FOLD_K = 0, one sequential chain of 2048 MFMA additions per element): c_hip 3.78 against c_ref 0.51 of oneDNN's blocked
sum, ratio 7.40 -- the noise the fold exists to remove, not a defect (folded every 256 the same case gives c_hip 0.49, ratio 0.95).
Twice that is above the ceiling, so M_LINEAR = 8, and it is what the RPG_TUNE_FOLD_K = 0 cases are held to (their next worst:
2.59, linear112 at K = 544).  Every case that leaves the fold on is held to the tighter M_FOLDED = 4: their worst ratio is 2.00
(linear112 at K = 256; the tile engine's routes <= 1.53, stream-K <= 1.11, linear112k2 <= 0.97), twice that is the starting
value, and 4 is the margin at which test_linear_sweep_cpu.py shows each planted defect caught.  Neither rises without the
arithmetic that justifies it written here: a ratio above the margin is a finding to fix in the kernel or to explain.

What pins what (planted in the torch emulation of linear_sweep_ref.py and caught there by test_linear_sweep_cpu.py on these same
lists; no broken kernel is run on a GPU).  A k-group dropped on the last partial M tile and a segment boundary off by one quad:
"buffer4_bk16" (M = 1, 63, 65, 129; two and three segments; the quad behind source 0's width is NaN).  residual2 gathered with
res_idx: the "two" cases of every list, "general_lds" checked.  out_relu taken before the residual: the out_relu cases with a
residual, "buffer8_t3" checked.  Bias lost on split tiles: "streamk_fixup" / "streamk_inkernel".  Low mantissa bits: "mantissa"
(a bias of +-30, so |z| ~ S; the N(0, 1) cases in general weigh mantissa bits, the "act" cases -- c_ref in the tens to hundreds
with the 1e3 outlier channel -- catch wrong offsets, dropped terms and outside loads).  A quad read from a padding column: every
case (ld > width), "buffer4_bk32" checked.  A fold restarted without its sum: "fold".

Left out: the 112-row kernels' own pitch guard (112 rows x lda x 4 bytes >= 2^31 needs an A operand of more than 8 GiB).
"""
import ctypes as C

import pytest
import torch

import linear_sweep_ref as R
from conftest import rel_err
from relpose_gnn_amd import ops
from test_hip_graph_sweep import _record

pytestmark = pytest.mark.gpu

M_LINEAR = 8.0                # the ceiling: twice the worst ratio of profiles/linear_sweep_observed.json (7.40, K = 4096 as ONE chain) is above it
M_FOLDED = R.M_START          # 4: every case that does not switch the fold off; twice their worst ratio (2.00) is the starting value
assert 2.0 <= M_FOLDED <= M_LINEAR <= 8.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from relpose_gnn_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _opt(buf):
    return None if buf is None else buf.ptr()


class _Operands:
    """A LinearCase in harness buffers on the device."""

    def __init__(self, case, dev):
        self.case = case
        moat = lambda t: None if t is None else R.Moated(t.shape, dev, t)
        self.src = [moat(s.a) for s in case.sources]
        self.idx = [None if s.idx is None else s.idx.to(dev) for s in case.sources]
        self.w, self.bias, self.res1, self.res2 = moat(case.weight), moat(case.bias), moat(case.res1), moat(case.res2)
        self.res_idx = None if case.res_idx is None else case.res_idx.to(dev)
        self.res2_idx = None if case.res2_idx is None else case.res2_idx.to(dev)
        self.inputs = [b for b in (*self.src, self.w, self.bias, self.res1, self.res2) if b is not None]

    def source_arrays(self):
        from relpose_gnn_amd import _lib
        c = self.case
        return (_lib.ptr_array([b.ptr() for b in self.src]), _lib.ptr_array([None if i is None else i.data_ptr() for i in self.idx]),
                _lib.int_array([s.ld for s in c.sources]), _lib.int_array([s.width for s in c.sources]))

    def launch(self, lib, dev, relu, entry="ex", relu_copy=None):
        """One launch into fresh output buffers -> (out, out_relu or None on the CPU, the route record); the harness has looked."""
        from relpose_gnn_amd import ops
        c = self.case
        relu_copy = c.want_relu_copy if relu_copy is None else relu_copy
        out = R.Moated((c.m, c.n_out), dev)
        out_relu = R.Moated((c.m, c.n_out), dev) if relu_copy else None
        if entry == "plain":
            assert c.res_mode in ("none", "plain") and not relu_copy
            rc = lib.rpg_linear_gather_f32(len(self.src), *self.source_arrays(), self.w.ptr(), _opt(self.bias), _opt(self.res1), out.ptr(), c.m,
                                           c.n_out, int(relu), _stream())
        else:
            rows = (C.c_long * len(self.src))(*[0 if s.idx is None else s.rows for s in c.sources])
            rc = lib.rpg_linear_gather_ex_f32(len(self.src), *self.source_arrays(), rows, self.w.ptr(), _opt(self.bias), _opt(self.res1),
                                              None if self.res_idx is None else self.res_idx.data_ptr(), _opt(self.res2),
                                              None if self.res2_idx is None else self.res2_idx.data_ptr(),
                                              c.ldr if c.res_idx is not None else 0, out.ptr(), _opt(out_relu), c.m, c.n_out, int(relu), _stream())
        route = ops.gemm_last_route()
        torch.cuda.synchronize()
        assert rc == 0, (rc, lib.rpg_last_error())
        assert R.harness_findings(self.inputs, out) == []
        if out_relu is not None:
            assert R.harness_findings(self.inputs, out_relu) == []
        return out.t.cpu(), None if out_relu is None else out_relu.t.cpu(), route


def _assert_route(spec, route):
    """The record must read what the case claims; a split case must have split (more stream-K workgroups than split tiles)."""
    got = {k: route[k] for k, _ in spec.expect}
    assert got == dict(spec.expect), (spec.name, route)
    if spec.sk:
        assert route["g_sk"] > route["rem"] > 0 and route["t_dp"] == route["tiles"] - route["rem"] and route["its_per"] >= 1, (spec.name, route)
    elif "combine" in dict(spec.expect):
        assert route["g_sk"] == 0 and route["rem"] == 0 and route["t_dp"] == route["tiles"], (spec.name, route)


_REF = {}


def _ref(spec):
    """(case, LinearRef, fp32 CPU result before the activation), computed once per spec and left unchanged."""
    if spec.name in _REF:
        return _REF[spec.name]
    case = spec.build()
    made = (case, R.linear_ref(case), R.linear_fp32(case))
    if case.m * case.n_out <= 1 << 18:                                    # the 112-row cases are large and run once
        _REF[spec.name] = made
    return made


def _margin(spec):
    """M_LINEAR for a case that runs K as one sequential chain (RPG_TUNE_FOLD_K = 0), the tighter M_FOLDED for every other."""
    return M_LINEAR if dict(spec.keys).get("FOLD_K", ops.tuning_default("FOLD_K")) == 0 else M_FOLDED


def _run(spec, lib, dev, section, repeats=1, assert_bar=True):
    """One spec: launch (without ReLU; with it too if the case has one), assert the route, the harness, both bars.  ``repeats``:
    so many launches without ReLU must be bit-identical.  -> (c_hip of the launch without ReLU, c_ref); with ``assert_bar`` off
    the caller compares them (after it has recorded a second launch)."""
    case, ref, y32 = _ref(spec)
    ops_ = _Operands(case, dev)
    with ops.tuned(dict(spec.keys)):
        out, out_relu, route = ops_.launch(lib, dev, 0, spec.entry)
        _assert_route(spec, route)
        for _ in range(repeats - 1):
            again, again_relu, route2 = ops_.launch(lib, dev, 0, spec.entry)
            assert route2 == route and torch.equal(again, out) and (out_relu is None or torch.equal(again_relu, out_relu)), spec.name
        if case.relu:
            y_act, _, route_act = ops_.launch(lib, dev, 1, spec.entry, relu_copy=False)
            _assert_route(spec, route_act)
    assert rel_err(out, y32) < 1e-5, spec.name
    bar = _margin(spec) * ref.c_ref
    if out_relu is not None:
        assert torch.equal(out_relu, torch.relu(out)), spec.name
        assert R.c_of(out_relu, ref.z, ref.S, relu=True) <= bar, spec.name
    if case.relu:
        assert rel_err(y_act, torch.relu(y32)) < 1e-5, spec.name
        c_act = R.c_of(y_act, ref.z, ref.S, relu=True)
        assert c_act <= bar, (spec.name, ref.c_ref, c_act)
    c_hip = R.c_of(out, ref.z, ref.S)
    assert ref.c_ref > 0.0, "the fp32 CPU reference is exact here: the case measures nothing"
    _record(section, spec.name, {"c_ref": ref.c_ref, "c_hip": c_hip, "ratio": c_hip / ref.c_ref,
                                 "route": "{kernel} {BM}x{BN} bk{BK} w{waves} {loader} epi{epi_lds} sk{g_sk}/{rem} {combine} fold{fold_k}".format(**route)})
    if assert_bar:
        assert c_hip <= bar, (spec.name, ref.c_ref, c_hip, c_hip / ref.c_ref)
    return c_hip, ref.c_ref


# ----------------------------------------------------------------------------------------------------------------------
# the route matrix
# ----------------------------------------------------------------------------------------------------------------------
_TILE_PARAMS = [pytest.param(spec, id=spec.name) for route in R.TILE_ROUTES for spec in R.tile_route_specs(route)]


@pytest.mark.parametrize("spec", _TILE_PARAMS)
def test_tile_engine_route(dev, lib, spec):
    """One case of a tile-engine route (linear_sweep_ref.tile_route_specs): M and N on and beside the tile, plain / gathered / mixed
    sources with every index pattern, the four residual modes with ldr > n_out, out_relu, both value regimes."""
    _run(spec, lib, dev, "tile")


@pytest.mark.parametrize("spec", [pytest.param(s, id=s.name) for s in R.streamk_specs(False)])
def test_streamk_fixup_launch(dev, lib, spec):
    """Split tiles finished by streamk_fixup_kernel (the vector form, and the scalar one at N = 99) with gathered residual rows of
    pitch ldr != n_out on ragged M and N."""
    _run(spec, lib, dev, "streamk_fixup")


@pytest.mark.parametrize("spec", [pytest.param(s, id=s.name) for s in R.streamk_specs(True)])
def test_streamk_inkernel_combine(dev, lib, spec):
    """The same cases finished by their last-arriving workgroup; three runs are bit-identical (the slabs are summed in k order
    whoever arrives last)."""
    _run(spec, lib, dev, "streamk_inkernel", repeats=3)


@pytest.mark.parametrize("i", range(4))
@pytest.mark.parametrize("kernel", ["linear112", "linear112k2"])
def test_linear112(dev, lib, cus, kernel, i):
    """The exact-fit kernels at the tile counts that select them on THIS device (M = 672 / 448 on 256 CUs), K in {64, 96, 288}."""
    _run(R.linear112_specs(kernel, cus)[i], lib, dev, kernel)


@pytest.mark.parametrize("spec", [pytest.param(s, id=s.name) for s in R.mantissa_specs()])
def test_mantissa_cases(dev, lib, spec):
    """|z| ~ S: a few lost mantissa bits of the output are a few u S."""
    _run(spec, lib, dev, "mantissa")


# ----------------------------------------------------------------------------------------------------------------------
# further checks
# ----------------------------------------------------------------------------------------------------------------------
def test_entry_points_take_different_loaders(dev, lib):
    """The same gathered operands: rpg_linear_gather_f32 has no row counts to give, so the launcher cannot bound the 32-bit
    offsets and records the general loader; rpg_linear_gather_ex_f32 with rows records the buffer loader.  Both meet the bar."""
    plain, ex = R.entry_point_spec("plain"), R.entry_point_spec("ex")
    _run(plain, lib, dev, "entry")
    _run(ex, lib, dev, "entry")
    assert torch.equal(_ref(plain)[1].z, _ref(ex)[1].z)


@pytest.mark.parametrize("name", [s.name for s in R.fold_specs()])
def test_fold_boundaries(dev, lib, cus, name):
    """RPG_TUNE_FOLD_K in {0, 64, 256} at K = fold -+ one step, fold, and two folds + one step, on the two folding tiles of the
    buffer loader and on linear112; the record must show the fold length in force."""
    _run({s.name: s for s in R.fold_specs(cus)}[name], lib, dev, "fold")


def test_long_k_chain_and_fold_side_by_side(dev, lib):
    """K = 4096, M = N = 64: c_hip of one sequential chain and of folds every 256, recorded side by side.  Asserted: both meet the
    bar.  Which one is closer to float64 is an observation (profiles/linear_sweep_observed.json)."""
    c = {fold: _run(R.long_k_spec(fold), lib, dev, "long_k", assert_bar=False) for fold in (0, 256)}
    print(f"K = 4096: c_hip {c[0][0]:.3f} as one chain, {c[256][0]:.3f} folded every 256, c_ref {c[0][1]:.3f}")
    assert c[0][1] == c[256][1]                                           # one reference for both
    assert c[0][0] <= M_LINEAR * c[0][1] and c[256][0] <= M_FOLDED * c[256][1], c


@pytest.mark.parametrize("rows,loader", [((1 << 19) - 1, "buffer"), (1 << 19, "general")], ids=["below-buffer", "at-general"])
def test_offset_guard_at_2_31_bytes(dev, lib, rows, loader):
    """One gathered source of pitch 1024: with 2^19 - 1 rows the largest byte offset still fits 32 bits (buffer loader), with 2^19
    rows the tensor is 2^31 bytes and the launcher takes 64-bit pointers.  The tensor is uninitialised memory but for the rows the
    index names -- row 0, the last row and the two rows either side of byte 2^30 -- whose padding columns hold NaN."""
    from relpose_gnn_amd import _lib, ops
    if torch.cuda.get_device_properties(dev).total_memory < 64 << 30:
        pytest.skip("needs 2 GiB for one operand; devices below 64 GiB are not asked to")
    m, n_out, width, ld = 65, 64, 64, 1024
    named = torch.tensor([0, rows - 1, (1 << 18) - 1, 1 << 18])
    spec = R.Spec(f"guard-rows{rows}", "guard", m, n_out, (("gather", width, ld, "random"),), seed=8800)
    case = spec.build()
    src = case.sources[0]
    pick = torch.arange(m) % 4                                            # output row r reads named[r % 4]
    src.a, src.idx = src.a[:4].contiguous(), pick                         # the reference uses only those rows
    ref, y32 = R.linear_ref(case), R.linear_fp32(case)
    big = torch.empty((rows, ld), dtype=torch.float32, device=dev)
    assert big.numel() * 4 == rows * ld * 4 and (big.numel() * 4 >= 1 << 31) == (loader == "general")
    big[named.to(dev)] = src.a.to(dev)
    idx = named[pick].to(dev)
    w, bias, out = R.Moated(case.weight.shape, dev, case.weight), R.Moated(case.bias.shape, dev, case.bias), R.Moated((m, n_out), dev)
    with ops.tuned({"TILE": 2}):
        rc = lib.rpg_linear_gather_ex_f32(1, _lib.ptr_array([big.data_ptr()]), _lib.ptr_array([idx.data_ptr()]), _lib.int_array([ld]),
                                          _lib.int_array([width]), (C.c_long * 1)(rows), w.ptr(), bias.ptr(), None, None, None, None, 0,
                                          out.ptr(), None, m, n_out, 0, _stream())
        route = ops.gemm_last_route()
        torch.cuda.synchronize()
    del big
    torch.cuda.empty_cache()
    assert rc == 0, (rc, lib.rpg_last_error())
    assert (route["kernel"], route["loader"], route["BM"], route["BK"]) == ("tile", loader, 64, 16), route
    assert R.harness_findings([w, bias], out) == []
    got = out.t.cpu()
    assert rel_err(got, y32) < 1e-5
    c_hip = R.c_of(got, ref.z, ref.S)
    _record("guard", spec.name, {"c_ref": ref.c_ref, "c_hip": c_hip, "ratio": c_hip / ref.c_ref, "route": route["loader"]})
    assert c_hip <= M_FOLDED * ref.c_ref, (ref.c_ref, c_hip)
