"""rpg_pose_heads_mc_f32 / rpg_mc_advance on the GPU (ops.pose_heads_mc, csrc/mc_heads.hip) against tests/mc_dropout_ref.py.

Values.  The mask is the numpy helper's, so every sample is a plain Linear of the masked, scaled input, and the yardstick is the
graph sweep's for rpg_pose_heads_f32: graph_sweep_ref.pose_heads_err, max |y - z| / (|z| + sum_k |x_k w_k| + |b|) against float64.
Asserted per case: the kernel's figure <= M_KERNEL (8, tests/test_hip_graph_sweep.py) x the figure of the fp32 CPU statement, for
the samples and -- the mean of S Linears being the Linear of the mean input -- for the mean by the same function.  The standard
deviation: |sqrt(var) - sd64| <= 3 delta + 8 S 2^-24 sd64, delta the largest per-sample deviation the sample bar admits for that
element (samples off by at most delta move the mean by delta, the centred values by 2 delta and the unbiased deviation by at most
2 sqrt(S / (S - 1)) delta <= 3 delta; the second term is the two fp32 passes).  Every case prints c_ref, c_hip and their ratio and
appends them to the file RPG_SWEEP_RECORD names; profiles/mc_heads_observed.json holds one such run on an MI355X.

Shapes.  d = 4: one float4 for 64 lanes; 64; 252: a ragged pass; 2048: the full register tile; 2052: a second tile of one chunk.
R = 1, 5: fewer rows than the workgroup's four waves; 130: a ragged last workgroup.  S = 1, 2: only the one-sample blocks; 5, 7:
a block of four and a tail; 16: blocks only; 300: above 256 samples a workgroup holds one row.
"""
import json
import os

import numpy as np
import pytest
import torch

import graph_sweep_ref as G
import mc_dropout_ref as R

pytestmark = pytest.mark.gpu

M_KERNEL = 8.0                # tests/test_hip_graph_sweep.py
SEED, DRAW, BASE = 0x1234ABCD5678, 3, 1000

# (d, R, S, p, ids): ids "rows" = numbered by the row, "nodes" = explicit node ids, "edges" = (source, target) pairs
CASES = [(4, 1, 1, 0.5, "rows"), (4, 5, 2, 0.1, "nodes"), (4, 130, 16, 0.9, "edges"),
         (64, 1, 16, 0.1, "edges"), (64, 5, 1, 0.9, "rows"), (64, 130, 2, 0.5, "nodes"),
         (2048, 1, 2, 0.9, "nodes"), (2048, 5, 16, 0.5, "edges"), (2048, 130, 1, 0.1, "rows"), (2048, 130, 16, 0.5, "rows"),
         (252, 5, 5, 0.5, "edges"), (2052, 5, 7, 0.1, "nodes"), (64, 5, 300, 0.5, "rows")]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _state(dev, draw=DRAW, base=BASE):
    return torch.tensor([draw, base], dtype=torch.int32, device=dev)


def _inputs(d, r):
    return _rand(r, d, seed=2 + d), _rand(6, d, seed=3, scale=d ** -0.5), _rand(6, seed=4)


def _ids(kind, r, seed=9):
    """-> (what ops.pose_heads_mc takes, a [r], b [r] of the mask before node_base + id_offset)."""
    if kind == "rows":
        return None, np.arange(r), None
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(0, 5000, (r,), generator=g, dtype=torch.int64)
    if kind == "nodes":
        return a, a.numpy(), None
    b = torch.randint(0, 5000, (r,), generator=g, dtype=torch.int64)
    return torch.stack([a, b]), a.numpy(), b.numpy()


def _keep(a, b, off, d, S, p, draw=DRAW):
    r = len(a)
    return R.mask(SEED, draw, a + off, np.full(r, R.NODE_TAG) if b is None else b + off, d, S, p)


def _run(dev, x, w6, b6, p, S, ids, state=None, id_offset=0, want_samples=True):
    from relpose_gnn_amd import ops
    if torch.is_tensor(ids):
        ids = ids.to(dev)
    out = ops.pose_heads_mc(x.to(dev), w6.to(dev), b6.to(dev), p, S, SEED, _state(dev) if state is None else state, ids, id_offset,
                            want_samples=want_samples)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in out)


def _record(case: str, figures: dict) -> None:
    print("pose_heads_mc", case, figures)
    path = os.environ.get("RPG_SWEEP_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"section": "pose_heads_mc", "case": case, **figures}) + "\n")


@pytest.mark.parametrize("d,r,S,p,kind", CASES, ids=lambda v: str(v))
def test_samples_mean_and_spread_against_float64(dev, d, r, S, p, kind):
    x, w6, b6 = _inputs(d, r)
    ids, a, b = _ids(kind, r)
    mean, var, smp = _run(dev, x, w6, b6, p, S, ids)
    assert smp.shape == (S, r, 6) and mean.shape == var.shape == (r, 6)
    assert bool(torch.isfinite(smp).all() and torch.isfinite(mean).all() and torch.isfinite(var).all())
    keep = _keep(a, b, BASE, d, S, p)
    xm = R.masked_input64(x, keep, p)                                   # [S, r, d] float64
    z, mean64, var64 = R.statement64(x, w6, b6, keep, p)
    y32, mean32, _ = R.statement32(x, w6, b6, keep, p)
    flat = xm.reshape(S * r, d)
    c_ref = G.pose_heads_err(y32.reshape(S * r, 6), flat, w6, b6)
    c_hip = G.pose_heads_err(smp.reshape(S * r, 6), flat, w6, b6)
    if c_ref == 0.0:                       # a few products and a bias can round to the float64 value's nearest fp32: half an ulp
        c_ref = 2.0 ** -25                 # of the element's scale then, as tests/test_hip_graph_sweep.py has it for the heads
    m_ref = G.pose_heads_err(mean32, xm.mean(0), w6, b6)
    m_hip = G.pose_heads_err(mean, xm.mean(0), w6, b6)
    if m_ref == 0.0:
        m_ref = 2.0 ** -25
    case = f"d={d} R={r} S={S} p={p} {kind}"
    _record(case, {"c_ref": c_ref, "c_hip": c_hip, "ratio": c_hip / c_ref, "mean_ref": m_ref, "mean_hip": m_hip,
                   "mean_ratio": m_hip / m_ref})
    assert c_hip <= M_KERNEL * c_ref, (case, c_ref, c_hip)
    assert m_hip <= M_KERNEL * m_ref, (case, m_ref, m_hip)
    if S == 1:
        assert torch.equal(var, torch.zeros_like(var))
        return
    scale = z.abs() + xm.abs() @ w6.double().abs().t() + b6.double().abs()          # |z| + s per sample and element
    delta = (M_KERNEL * c_ref * scale).amax(0)
    sd64 = var64.sqrt()
    err = (var.double().sqrt() - sd64).abs()
    bound = 3.0 * delta + 8.0 * S * 2.0 ** -24 * sd64
    _record(case + " sd", {"worst_err_over_bound": float((err / bound).max())})
    assert bool((err <= bound).all()), (case, float((err / bound).max()))


@pytest.mark.parametrize("S,grid", [(1, False), (2, False), (16, True)])
def test_zero_features_give_the_bias(dev, S, grid):
    """x = 0: every sample is b exactly, so the mean is b bit for bit and the variance 0 -- for S = 16 with b on a grid of 2^-10
    (|b| < 8), where the sequential fp32 sum of S copies is exact; for S = 1, 2 with any b (b + b is exact)."""
    d, r = 64, 5
    _, w6, b6 = _inputs(d, r)
    if grid:
        b6 = torch.round(b6 * 1024.0) / 1024.0
    mean, var, smp = _run(dev, torch.zeros(r, d), w6, b6, 0.5, S, None)
    assert torch.equal(smp, b6.expand(S, r, 6)) and torch.equal(mean, b6.expand(r, 6)) and torch.equal(var, torch.zeros(r, 6))


def test_one_sample(dev):
    x, w6, b6 = _inputs(2048, 5)
    mean, var, smp = _run(dev, x, w6, b6, 0.5, 1, None)
    assert torch.equal(var, torch.zeros_like(var)) and torch.equal(mean, smp[0])


@pytest.mark.parametrize("kind", ["nodes", "edges"])
def test_rows_permuted_with_their_ids(dev, kind):
    """A row's result is a function of its features and ids: rows permuted together with their ids give the outputs permuted, bit
    for bit (130 rows: other waves, other workgroups)."""
    d, r, S = 252, 130, 5
    x, w6, b6 = _inputs(d, r)
    ids, _, _ = _ids(kind, r)
    perm = torch.randperm(r, generator=torch.Generator().manual_seed(5))
    mean, var, smp = _run(dev, x, w6, b6, 0.5, S, ids)
    mean_p, var_p, smp_p = _run(dev, x[perm].contiguous(), w6, b6, 0.5, S, (ids[perm] if ids.dim() == 1 else ids[:, perm]).contiguous())
    assert torch.equal(mean_p, mean[perm]) and torch.equal(var_p, var[perm]) and torch.equal(smp_p, smp[:, perm])
    assert not torch.equal(mean_p, mean)


def test_a_slice_of_the_rows_with_its_offset(dev):
    """Rows [a, b) alone with id_offset = a are those rows of the whole call, bit for bit; without the offset they are not."""
    d, r, S, lo, hi = 2048, 130, 3, 37, 102
    x, w6, b6 = _inputs(d, r)
    mean, var, smp = _run(dev, x, w6, b6, 0.5, S, None)
    mean_s, var_s, smp_s = _run(dev, x[lo:hi].contiguous(), w6, b6, 0.5, S, None, id_offset=lo)
    assert torch.equal(mean_s, mean[lo:hi]) and torch.equal(var_s, var[lo:hi]) and torch.equal(smp_s, smp[:, lo:hi])
    mean_0, _, _ = _run(dev, x[lo:hi].contiguous(), w6, b6, 0.5, S, None)
    assert not torch.equal(mean_0, mean[lo:hi])
    # node_base and id_offset add up: the same rows as ids of another base
    mean_b, _, _ = _run(dev, x[lo:hi].contiguous(), w6, b6, 0.5, S, None, state=_state(dev, DRAW, BASE + lo))
    assert torch.equal(mean_b, mean[lo:hi])


def test_advance_is_the_next_draw(dev):
    from relpose_gnn_amd import ops
    d, r, S = 64, 5, 16
    x, w6, b6 = _inputs(d, r)
    state = _state(dev)
    first = _run(dev, x, w6, b6, 0.5, S, None, state=state)
    ops.mc_advance(state)
    after = _run(dev, x, w6, b6, 0.5, S, None, state=state)
    assert state.cpu().tolist() == [DRAW + 1, BASE]
    want = _run(dev, x, w6, b6, 0.5, S, None, state=_state(dev, DRAW + 1))
    assert all(torch.equal(u, v) for u, v in zip(after, want)) and not torch.equal(after[0], first[0])
    keep = _keep(np.arange(r), None, BASE, d, S, 0.5, draw=DRAW + 1)            # and it is the helper's mask of draw + 1
    z, _, _ = R.statement64(x, w6, b6, keep, 0.5)
    assert float((after[2].double() - z).abs().max()) < 1e-4
    wrap = torch.tensor([-1, BASE], dtype=torch.int32, device=dev)               # 0xFFFFFFFF + 1 wraps to 0
    ops.mc_advance(wrap)
    torch.cuda.synchronize()
    assert wrap.cpu().tolist() == [0, BASE]


def test_non_finite_features_follow_the_mask(dev):
    """The mask selects: a NaN / Inf feature poisons the samples that KEEP its column (and the row's mean and variance), and no
    other; in a column every sample drops it changes nothing, bit for bit.  (F.dropout multiplies by 0 and would poison all.)"""
    d, r, S, p = 64, 5, 4, 0.5
    x, w6, b6 = _inputs(d, r)
    keep = _keep(np.arange(r), None, BASE, d, S, p)
    mixed = np.flatnonzero(keep[:, 2, :].any(0) & ~keep[:, 2, :].all(0))
    never = np.flatnonzero(~keep[:, 3, :].any(0))
    assert mixed.size and never.size
    c_mixed, c_never = int(mixed[0]), int(never[0])
    clean = _run(dev, x, w6, b6, p, S, None)
    for bad in (float("nan"), float("inf")):
        xb = x.clone()
        xb[2, c_mixed] = bad
        xb[3, c_never] = bad
        mean, var, smp = _run(dev, xb, w6, b6, p, S, None)
        kept = torch.from_numpy(keep[:, 2, c_mixed])
        assert bool((~torch.isfinite(smp[kept, 2])).all()) and bool(torch.isfinite(smp[~kept, 2]).all())
        assert torch.equal(smp[~kept, 2], clean[2][~kept, 2])
        assert bool((~torch.isfinite(mean[2])).all()) and bool((~torch.isfinite(var[2])).all())
        rest = [0, 1, 3, 4]
        assert torch.equal(mean[rest], clean[0][rest]) and torch.equal(var[rest], clean[1][rest]) and torch.equal(smp[:, rest], clean[2][:, rest])


def test_limits_raise(dev):
    from relpose_gnn_amd import ops
    x, w6, b6 = (t.to(dev) for t in _inputs(64, 5))
    state = _state(dev)
    for p in (0.0, 1.0, -0.5, float("nan")):
        with pytest.raises(ValueError):
            ops.pose_heads_mc(x, w6, b6, p, 4, 0, state)
    for S in (0, 1025):
        with pytest.raises(ValueError):
            ops.pose_heads_mc(x, w6, b6, 0.5, S, 0, state)
    with pytest.raises(ValueError):                                               # d % 4
        ops.pose_heads_mc(x[:, :62].contiguous(), w6[:, :62].contiguous(), b6, 0.5, 4, 0, state)
    wide = torch.zeros(1, 4 * 65536, device=dev)
    with pytest.raises(ValueError):                                               # d / 4 < 65536
        ops.pose_heads_mc(wide, torch.zeros(6, 4 * 65536, device=dev), b6, 0.5, 4, 0, state)
    for off in (-1, 2 ** 31 - 4, 2 ** 31):
        with pytest.raises(ValueError):                                           # node ids stay below 2^31
            ops.pose_heads_mc(x, w6, b6, 0.5, 4, 0, state, id_offset=off)
    with pytest.raises(ValueError):
        ops.pose_heads_mc(x, w6, b6, 0.5, 4, 2 ** 64, state)
    with pytest.raises(ValueError):
        ops.pose_heads_mc(x, w6, b6, 0.5, 4, 0, state, ids=torch.zeros(4, dtype=torch.int64, device=dev))
    with pytest.raises(TypeError):
        ops.pose_heads_mc(x, w6, b6, 0.5, 4, 0, state.float())
    ops.pose_heads_mc(x, w6, b6, 0.5, 1024, 2 ** 64 - 1, state, id_offset=2 ** 31 - 5)          # the limits themselves are served
    torch.cuda.synchronize()
