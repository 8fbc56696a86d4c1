"""The retrieval kernels' sweep (csrc/retrieve.hip): the launchers' rules restated, data on which the order is exact, an integer
oracle, a numpy emulation of the three launches with planted defects, the case lists, and the memory harness of the C ABI.
Test helper (like encoder_sweep_ref.py): no test lives here.  tests/test_retrieval_sweep_cpu.py holds the restatement to
hand-worked values and shows that every planted defect fails a case; tests/test_hip_retrieval_sweep.py runs the cases on the GPU.

THE RESTATED RULE (host side of csrc/retrieve.hip)
    split_plan(m, d)        column slices and 64-column blocks per slice: a function of (m, d) only, part of the summation order
    plan(g, m, d)           + the NQ instantiation launch_dot picks and the 64-query chunks (what rpg_retrieve_plan returns)
    live_digits(lo, hi)     the radix digits (shifts) the select loop histograms for a row range [lo, hi): the four key digits
                            always, a row digit unless (hi - 1) >> shift == 0
    gate_step(row, lo)      (outer step, unroll lane) of a row in the gate sweep: GATE_UNROLL * RS_NT = 4096 rows per outer step
    ws_layout / elect_layout  byte offsets of the plain and the electing call's workspace

DATA ON WHICH THE ORDER IS EXACT
    lattice     rows and queries in {-1, 0, +1}, every database row with the same number w <= 64 of non-zeros: every product and
                partial sum is a small integer, exact in fp32 in ANY order; every row has bit for bit the same inverse norm (the
                same sum w in the same order); so the similarity is a strictly increasing function of the integer dot and equal
                dots are bit-equal.  Half of a row's non-zeros are spaced evenly over d from a row-dependent start, so that every
                64-column block, every offset inside a block and the last float4 of a ragged d carry weight (``coverage``).
    integers    arbitrary small integer rows, d = 8, with ``db_inv_norm`` passed as ones (the ABI takes a caller-cached norm):
                the similarity IS the dot times 1 / |q|, |q| in {0, 1, 2}.  Rows whose cached inverse norm is 2^-126 and whose
                entries are scaled by 2^-30 give products below 2^-150: they round to +0 or -0 by the sign of the dot.  A row with a
                NaN in a column where every query holds 0 is non-finite for every query.
The oracle (``oracle``) is integer numpy: (dot descending, row ascending) over the allowed rows, non-finite rows after every finite
one, ranks clamped and counted as include/relpose_gnn_hip.h states.  It calls neither the GPU nor any entry point.

THE A-PRIORI BOUND OF THE FLOAT CASES (``sim_bound``), u = 2^-24, gamma_n = n u / (1 - n u)
    dot     a product is rounded once (if the matrix pipe rounds it; counting it is the safe side) and then passes through at
            most L_dot - 1 fp32 additions: the wave that owns it adds 64 products per block into one accumulator (16 MFMAs of 4
            products: at most 4 additions of the chain per MFMA whatever order the four are added in) over ceil(bps / 4) blocks,
            the four wave sums take 3 additions, the slices ns - 1.  L_dot = 1 + 64 ceil(bps / 4) + 3 + (ns - 1), and
            |dot32 - dot| <= gamma_{L_dot} sum_i |q_i d_i|  (Higham, Accuracy and Stability, 3.1: any order, chain length L).
    norms   row_inv_norms_kernel: a square is rounded (1), joins its float4's sum (3), the thread's running sum over
            ceil(d / 4 / 256) float4s, the shuffle tree (6), the wave sums (3): L_n = 13 + ceil(d / 1024), all terms positive, so
            ss32 = ss (1 + e), |e| <= gamma_{L_n}; sqrtf and the division are correctly rounded (hipcc's default
            -fhip-fp32-correctly-rounded-divide-sqrt; no fast-math flag in build.py): inv32 = (1 / |x|) (1 + e_n) with
            1 + e_n <= (1 - gamma_{L_n})^(-1/2) (1 + u) / (1 - u).
    sim     sim32 = fl(fl(dot32 q_inv) db_inv): two more roundings.  With rel = (1 + e_n)^2 (1 + u)^2 - 1 and
            A = sum_i |q_i d_i| / (|q| |d|) <= 1:    |sim32 - sim| <= gamma_{L_dot} A (1 + rel) + |sim| rel.
It holds for any order inside an MFMA and inside the launch, so it carries no margin.  The j-th value of the order by sim32 is
within max-bound of the j-th value of the order by sim, and the sim of its row within max-bound of that: 2 x per query.

THE EMULATION (``emulate``) runs the three launches in numpy -- fp32 block products per wave and slice into a flat `part` buffer
of exactly the workspace's size, keys, the radix select digit by digit, the gate sweep by (outer step, lane), the vote -- and takes
``defect=`` one of DEFECTS.  On lattice and integer data every partial sum is exact, so the emulation's bits are the kernels'.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

RT_ROWS, RT_BLK, RT_QCHUNK, RT_WAVES = 16, 64, 64, 4
RS_NT, R_MAX, K_MAX, GATE_UNROLL = 1024, 512, 64, 4
KEY_NONFINITE, KEY_EXCLUDED = 0xFFFFFFFE, 0xFFFFFFFF
ELECT_ALL, ELECT_LOST = 1, 2
U = 2.0 ** -24
FLT_MAX = np.finfo(np.float32).max
TINY_INV = np.float32(2.0 ** -126)          # a cached inverse norm that sends a scaled row's similarity to +-0
TINY_SCALE = np.float32(2.0 ** -30)


def _cdiv(a: int, b: int) -> int:
    return -(-int(a) // int(b))


# ----------------------------------------------------------------------------------------------------------------------
# the rule, restated
# ----------------------------------------------------------------------------------------------------------------------
def split_plan(m: int, d: int) -> Tuple[int, int]:
    """(nsplit, blocks_per_split) of csrc/retrieve.hip split_plan."""
    tiles, nblk = _cdiv(m, RT_ROWS), _cdiv(d, RT_BLK)
    s = max(1, min(_cdiv(1024, tiles), max(1, nblk // 8), 16))
    bps = _cdiv(nblk, s)
    return _cdiv(nblk, bps), bps


def plan(g: int, m: int, d: int) -> Tuple[int, int, int, int]:
    """(nsplit, blocks_per_split, NQ, query chunks): what rpg_retrieve_plan returns."""
    ns, bps = split_plan(m, d)
    tiles = (min(g, RT_QCHUNK) + 15) // 16
    return ns, bps, (1 if tiles <= 1 else 2 if tiles == 2 else 4), _cdiv(g, RT_QCHUNK)


def slice_blocks(m: int, d: int) -> List[Tuple[int, int]]:
    """[b_begin, b_end) of every column slice."""
    ns, bps = split_plan(m, d)
    nblk = _cdiv(d, RT_BLK)
    return [(s * bps, min(s * bps + bps, nblk)) for s in range(ns)]


def live_digits(lo: int, hi: int) -> Tuple[int, ...]:
    """The shifts the radix select histograms over rows [lo, hi), hi >= 1 (the skip reads hi alone)."""
    return tuple(sh for sh in range(56, -1, -8) if not (sh < 32 and ((hi - 1) >> sh) == 0))


def skipped_digits(lo: int, hi: int) -> Tuple[int, ...]:
    return tuple(sh for sh in range(56, -1, -8) if sh not in live_digits(lo, hi))


def gate_step(row: int, lo: int = 0) -> Tuple[int, int]:
    """(outer step, unroll lane) in which the gate sweep of a range that starts at ``lo`` visits ``row``."""
    off = int(row) - int(lo)
    return off // (GATE_UNROLL * RS_NT), (off % (GATE_UNROLL * RS_NT)) // RS_NT


def _round_up(v: int, a: int) -> int:
    return _cdiv(v, a) * a


def ws_layout(g: int, m: int, d: int) -> Dict[str, int]:
    """Byte offsets of rpg_retrieve_workspace_bytes' workspace: q_inv fp32 [g], db_inv fp32 [m], part fp32 [ns][g][m]."""
    ns = split_plan(m, d)[0]
    w = {"q_inv": 0, "db_inv": _round_up(4 * g, 256)}
    w["part"] = w["db_inv"] + _round_up(4 * m, 256)
    w["total"] = w["part"] + _round_up(4 * ns * g * m, 256)
    return w


def elect_layout(g: int, m: int, d: int) -> Dict[str, int]:
    """The electing call's: the plain one, then the vote's keys uint32 [g][m]."""
    w = ws_layout(g, m, d)
    w["vkeys"] = w["total"]
    w["total"] = w["vkeys"] + _round_up(4 * g * m, 256)
    return w


# ----------------------------------------------------------------------------------------------------------------------
# the a-priori bound
# ----------------------------------------------------------------------------------------------------------------------
def gamma(n: int) -> float:
    return n * U / (1.0 - n * U)


def chain_lengths(m: int, d: int) -> Tuple[int, int]:
    """(L_dot, L_n) of the module docstring."""
    ns, bps = split_plan(m, d)
    return 1 + 64 * _cdiv(bps, RT_WAVES) + 3 + (ns - 1), 13 + _cdiv(d, 1024)


def sim_bound(q: np.ndarray, db: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(bound float64 [g, m], sim float64 [g, m]) for finite fp32 inputs; a zero-norm vector gives similarity 0 exactly."""
    import retrieval_ref as R
    m, d = db.shape
    l_dot, l_n = chain_lengths(m, d)
    e_n = (1.0 - gamma(l_n)) ** -0.5 * (1.0 + U) / (1.0 - U) - 1.0
    rel = (1.0 + e_n) ** 2 * (1.0 + U) ** 2 - 1.0
    q64, d64 = np.asarray(q, dtype=np.float64), np.asarray(db, dtype=np.float64)
    qn, dn = np.sqrt((q64 * q64).sum(1)), np.sqrt((d64 * d64).sum(1))
    qn[qn == 0], dn[dn == 0] = 1.0, 1.0
    a = (np.abs(q64) @ np.abs(d64).T) / qn[:, None] / dn[None, :]
    s = R.cosine_f64(q, db)
    return gamma(l_dot) * a * (1.0 + rel) + np.abs(s) * rel, s


# ----------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    id: str
    why: str
    kind: str                                   # "plain" | "gated" | "scoped" | "elect": the entry point it goes through
    q: np.ndarray                               # fp32 [g, d]
    db: np.ndarray                              # fp32 [m, d]
    ranks: np.ndarray                           # int32 [g, k]
    score: Optional[np.ndarray] = None          # int64 [g, m]: the integer the order is by; None: a float case
    nonfinite: Optional[np.ndarray] = None      # bool [g, m]
    sim_scale: Optional[np.ndarray] = None      # fp32 [g]: integer data, similarity == score * sim_scale exactly; None: lattice
    db_inv: Optional[np.ndarray] = None         # fp32 [m] handed in as db_inv_norm
    q_group: Optional[np.ndarray] = None        # int64 [g]
    db_group: Optional[np.ndarray] = None       # int64 [m]
    gate: Optional[dict] = None                 # db_gate f64 [m, 7], prior f64 [g, 7], r2, inside bool [m] (by construction)
    first: Optional[np.ndarray] = None          # int64 [n + 1]
    q_scene: Optional[np.ndarray] = None        # int32 [g] (elect: the array on entry)
    vote_top: int = 0
    mode: int = 0

    @property
    def g(self): return self.q.shape[0]
    @property
    def m(self): return self.db.shape[0]
    @property
    def d(self): return self.db.shape[1]
    @property
    def k(self): return self.ranks.shape[1]
    @property
    def plan(self): return plan(self.g, self.m, self.d)


@dataclass(frozen=True)
class Spec:
    id: str
    why: str
    make: Callable[[], Case] = field(compare=False, hash=False)


_BUILT: Dict[str, Case] = {}


def build(spec: Spec) -> Case:
    """The case of a spec, made once and kept unchanged (nothing writes into a Case's arrays)."""
    if spec.id not in _BUILT:
        c = spec.make()
        c.id, c.why = spec.id, spec.why
        _BUILT[spec.id] = c
    return _BUILT[spec.id]


def spread_ranks(k: int, r: int, must: Sequence[int] = ()) -> np.ndarray:
    """int32 [k], strictly ascending, largest r - 1 (so R = r), holding 0 and every position of ``must`` below r; needs r >= k."""
    assert 1 <= k <= K_MAX and r >= k, (k, r)
    keep = sorted({int(p) for p in must if 0 <= int(p) < r} | {r - 1})[-k:]
    have = set(keep)
    for p in [0] + [int(round(x)) for x in np.linspace(0, r - 1, 4 * k)] + list(range(r)):
        if len(have) >= k:
            break
        have.add(p)
    out = np.array(sorted(have), dtype=np.int32)
    assert out.shape == (k,) and out[-1] == r - 1
    return out


def lattice(m: int, d: int, g: int, w: int = 48, seed: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """(Q int8 [g, d], D int8 [m, d]) of the module docstring."""
    rng = np.random.RandomState(seed)
    w = min(w, d)
    h = max(1, w // 2)
    if w == d:                                                        # every column of every row: nothing to place
        return _lattice_queries(rng, g, d), rng.choice(np.array([-1, 1], dtype=np.int8), (m, d))
    dm = np.zeros((m, d), dtype=np.int8)
    cols = np.arange(d)
    for r in range(m):
        base = (r * 37 + (np.arange(h) * d) // h) % d
        if r % 3 == 0:
            base[0] = d - 1 - (r // 3) % min(4, d)                  # the last float4, each of its four lanes in turn
            base = np.unique(base)
        rest = np.setdiff1d(cols, base)
        pick = np.concatenate([base, rng.choice(rest, w - base.shape[0], replace=False)])
        dm[r, pick] = rng.choice(np.array([-1, 1], dtype=np.int8), w)
    return _lattice_queries(rng, g, d), dm


def _lattice_queries(rng, g: int, d: int) -> np.ndarray:
    qm = rng.randint(-1, 2, (g, d)).astype(np.int8)
    tail = qm[:, -4:]
    tail[tail == 0] = 1                                               # the last float4 always counts
    return qm


def coverage(dm: np.ndarray) -> Dict[str, int]:
    """What of the dot kernel's column geometry no row of ``dm`` puts weight on."""
    d = dm.shape[1]
    used = np.flatnonzero((dm != 0).any(0))
    return {"blocks_missing": _cdiv(d, RT_BLK) - len(set((used // RT_BLK).tolist())),
            "offsets_missing": min(d, RT_BLK) - len(set((used % RT_BLK).tolist())),
            "last_float4_missing": 4 - int((used >= d - 4).sum())}


def _lattice_case(m, d, g, k=None, seed=None, w=48, kind="plain") -> Case:
    qm, dm = lattice(m, d, g, w, seed if seed is not None else 1000 * m + d + g)
    k = min(m, 8) if k is None else k
    r = min(m, R_MAX)
    ranks = np.stack([spread_ranks(k, max(k, r - 3 * (j % 5)), (1, 2)) for j in range(g)])
    score = qm.astype(np.int64) @ dm.astype(np.int64).T
    return Case("", "", kind, qm.astype(np.float32), dm.astype(np.float32), ranks, score, np.zeros((g, m), dtype=bool))


def _hash(r: np.ndarray) -> np.ndarray:
    return (r.astype(np.uint64) * np.uint64(2654435761) >> np.uint64(7)).astype(np.int64)


def int_values(m: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(V int64 [m, 3], tiny bool [m], nan bool [m]): column 0 eleven values -5 .. 5 (lattice load), column 1 a class of 9s from
    300 rows below to 300 rows above row 256 and row 65536 over -(r % 7) (a tie class longer than R_MAX across each boundary;
    six rows from b - 1 on hold 10 and 11, so that R = 2 ends on row b itself),
    column 2 two values.  ``tiny``: rows whose similarity underflows to +-0; ``nan``: non-finite rows, at the boundaries too."""
    r = np.arange(m, dtype=np.int64)
    v = np.stack([_hash(r) % 11 - 5, -(r % 7), (_hash(r + 17) % 3 == 0).astype(np.int64)], axis=1)
    for b, top in ((256, 10), (65536, 11)):
        v[max(0, b - 300):min(m, b + 300), 1] = 9
        v[max(0, b - 1):min(m, b + 5), 1] = top                      # and a small class above it whose second row is row b
    tiny = (r % 13 == 5)
    nan = np.zeros(m, dtype=bool)
    nan[[x for x in (3, 254, 257, 65534, 65537, m - 3) if 0 <= x < m]] = True      # never a boundary row, never the last row
    return v, tiny & ~nan, nan


# queries of the integer form: (value column, factor a); factor 0 is the zero query (every similarity +0: one tie class of m rows)
INT_QUERIES = ((0, 1), (0, -1), (0, 0), (1, 2), (2, 1), (1, -1), (2, -2), (0, 2))


def _int_case(m: int, kind: str, queries: Sequence[Tuple[int, int]], d: int = 8, edit=None) -> Case:
    """q, db, db_inv, score, nonfinite of the integer form; ranks, groups, scopes and gates are the caller's.  ``edit(v, tiny,
    nan)`` changes the values in place first."""
    v, tiny, nan = int_values(m)
    if edit is not None:
        edit(v, tiny, nan)
    g = len(queries)
    db = np.zeros((m, d), dtype=np.float32)
    db[:, :3] = v
    db[tiny, :3] *= TINY_SCALE
    db[nan, 3] = np.nan
    db[:, 5] = 1.0                                                   # a column no query reads: every lane still multiplies
    q = np.zeros((g, d), dtype=np.float32)
    for j, (col, a) in enumerate(queries):
        q[j, col] = a
    # similarity = dot * (1 / |a|) = sign(a) * v exactly: that integer is the score (0 for the zero query and the +-0 rows)
    cls = np.stack([np.where(tiny, 0, int(np.sign(a)) * v[:, col]) for col, a in queries])
    db_inv = np.where(tiny, TINY_INV, np.float32(1.0)).astype(np.float32)
    return Case("", "", kind, q, db, np.zeros((g, 1), dtype=np.int32), cls, np.tile(nan, (g, 1)), np.ones(g, dtype=np.float32),
                db_inv)


# ----------------------------------------------------------------------------------------------------------------------
# the integer oracle
# ----------------------------------------------------------------------------------------------------------------------
def scope_of(first: np.ndarray, n: int, scene: int, m: int) -> Tuple[bool, int, int]:
    if scene < 0 or scene >= n:
        return False, 0, 0
    a = min(max(int(first[scene]), 0), m)
    b = min(max(int(first[scene + 1]), a), m)
    return True, a, b


def vote_int(voters: Sequence[int], first: np.ndarray, m: int) -> Tuple[int, int]:
    """(elected scene, votes): the scene with the most voters, the best-placed voter's among tied ones; -1 without a voter."""
    n = len(first) - 1
    owner = []
    for row in voters:
        own = -1
        for s in range(n):
            ok, a, b = scope_of(first, n, s, m)
            if a <= row < b:
                own = s
        owner.append(own)
    best, votes = -1, 0
    for s in owner:                                                   # by placement: a later scene needs strictly more
        if s >= 0 and owner.count(s) > votes:
            best, votes = s, owner.count(s)
    return best, votes


def order_int(score: np.ndarray, nonfinite: np.ndarray, rows: np.ndarray) -> np.ndarray:
    """``rows`` ordered by (finite first, score descending, row ascending)."""
    key = np.where(nonfinite[rows], 0, -score[rows])                 # a non-finite row's score means nothing
    return rows[np.lexsort((rows, key, nonfinite[rows]))]


def elects(case: Case) -> np.ndarray:
    if case.kind != "elect":
        return np.zeros(case.g, dtype=bool)
    if case.mode == ELECT_ALL:
        return np.ones(case.g, dtype=bool)
    e = np.asarray(case.q_scene) == -1
    if case.gate is not None:
        e |= ~np.isfinite(case.gate["prior"]).all(axis=1)
    return e


@dataclass
class Expect:
    nbrs: np.ndarray
    status: int
    ranked: np.ndarray                          # bool [g]: R > 0
    gate_info: Optional[np.ndarray]
    scene_info: Optional[np.ndarray]
    q_scene: Optional[np.ndarray]
    allowed: List[np.ndarray]                   # per query the rows that were ranked


def clamp_ranks(raw: np.ndarray, n_allowed: int, scene_ok: bool = True) -> Tuple[np.ndarray, int, int]:
    """(clamped ranks, R, the query's count into status) as the select kernel's thread 0 does it."""
    lim = min(int(n_allowed), R_MAX)
    bad, out = 0, []
    for r in raw.tolist():
        if r < 0 or r >= lim:
            bad += 1
            r = max(0, 0 if r < 0 else lim - 1)
        out.append(r)
    if any(b <= a for a, b in zip(raw.tolist(), raw.tolist()[1:])):
        bad += 1
    if not scene_ok:
        bad = 1
    return np.array(out, dtype=np.int64), (max(out) + 1 if lim > 0 else 0), bad


def oracle(case: Case, score: Optional[np.ndarray] = None, nonfinite: Optional[np.ndarray] = None) -> Expect:
    """Integer logic only.  ``score`` / ``nonfinite``: what to order by in place of the case's own (a float case's float64
    similarities, say)."""
    score = case.score if score is None else score
    nonfinite = case.nonfinite if nonfinite is None else nonfinite
    g, k, m = case.g, case.k, case.m
    rows = np.arange(m)
    nbrs = np.zeros((g, k), dtype=np.int64)
    ranked = np.zeros(g, dtype=bool)
    status = 0
    scoped = case.kind in ("scoped", "elect") and case.first is not None
    n = len(case.first) - 1 if scoped else 0
    q_scene = None if not scoped else np.array(case.q_scene, dtype=np.int32)
    scene_info = np.zeros((g, 2), dtype=np.int32) if case.kind == "elect" else None
    gate_info = np.zeros((g, 2), dtype=np.int32) if case.gate is not None else None
    el = elects(case)
    allowed_rows = []
    for j in range(g):
        if case.kind == "elect":
            if el[j]:
                voters = order_int(score[j], nonfinite[j], rows)[:case.vote_top]
                scene_info[j] = vote_int(voters.tolist(), case.first, m)
                q_scene[j] = scene_info[j, 0]
            else:
                scene_info[j] = (q_scene[j], 0)
        ok, lo, hi = (True, 0, m) if not scoped else scope_of(case.first, n, int(q_scene[j]), m)
        allowed = (rows >= lo) & (rows < hi)
        if case.q_group is not None and int(case.q_group[j]) != -1:
            allowed &= np.asarray(case.db_group) != int(case.q_group[j])
        if case.gate is not None:
            if np.isfinite(case.gate["prior"][j]).all():
                both = allowed & case.gate["inside"]
                need = int(case.ranks[j].max()) + 1
                gate_info[j] = (0 if both.sum() >= need else 2, both.sum())
                allowed = both if both.sum() >= need else allowed
            else:
                gate_info[j] = (1, 0)
        ar = rows[allowed]
        allowed_rows.append(ar)
        cl, r, bad = clamp_ranks(case.ranks[j], ar.shape[0], ok)
        status += bad
        ranked[j] = r > 0
        if r > 0:
            nbrs[j] = order_int(score[j], nonfinite[j], ar)[cl]
    return Expect(nbrs, status, ranked, gate_info, scene_info, q_scene if case.kind == "elect" else None, allowed_rows)


# ----------------------------------------------------------------------------------------------------------------------
# the emulation
# ----------------------------------------------------------------------------------------------------------------------
DEFECTS = ("drop_block", "ragged_float4", "last_slice_out", "tail_column_stored", "mislaid_tile", "ties_desc_row",
           "unmasked_skip", "skip_by_length", "ignore_digit16", "neg_zero_key", "nonfinite_first", "sweep_from_0", "gate_lane3",
           "vote_beyond_top")


@dataclass
class Result:
    nbrs: np.ndarray
    sims: np.ndarray
    status: int
    gate_info: Optional[np.ndarray] = None
    scene_info: Optional[np.ndarray] = None
    q_scene: Optional[np.ndarray] = None
    findings: List[str] = field(default_factory=list)


def _inv_norms(x: np.ndarray) -> np.ndarray:
    with np.errstate(all="ignore"):
        ss = (x.astype(np.float32) ** 2).sum(1, dtype=np.float32)
        return np.where(ss == 0, np.float32(0), np.float32(1) / np.sqrt(ss)).astype(np.float32)


def sim_keys(s: np.ndarray, defect: Optional[str] = None) -> np.ndarray:
    """uint32 keys of fp32 similarities (sim_key): larger similarity -> smaller key, -0 and +0 one key, non-finite last."""
    s = np.asarray(s, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        fin = np.abs(s) <= FLT_MAX
    z = s if defect == "neg_zero_key" else s + np.float32(0.0)
    if defect == "nonfinite_first":
        z = np.where(fin, z, np.float32(0.0)).astype(np.float32)
    u = z.view(np.uint32)
    asc = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    key = (~asc).astype(np.uint32)
    if defect != "nonfinite_first":
        key[~fin] = KEY_NONFINITE
    return key


def key_sims(key: np.ndarray) -> np.ndarray:
    key = np.asarray(key, dtype=np.uint32)
    asc = ~key
    bits = np.where(asc & np.uint32(0x80000000), asc & np.uint32(0x7FFFFFFF), ~asc).astype(np.uint32)
    out = bits.view(np.float32).copy()
    out[key >= KEY_NONFINITE] = np.nan
    return out


def radix_select(keys: np.ndarray, lo: int, hi: int, need: int, size: int, defect: Optional[str] = None) -> np.ndarray:
    """The ``need`` smallest (key << 32 | row) of rows [lo, hi) (``keys`` indexed by row), sorted, padded with ~0 to ``size``: the
    select loop digit by digit, the collection, the sort."""
    rows = np.arange(lo, hi, dtype=np.uint64)
    comp = (keys[lo:hi].astype(np.uint64) << np.uint64(32)) | rows
    if defect == "ties_desc_row":                                     # the row digits compared the wrong way round
        order = np.lexsort((-rows.astype(np.int64), keys[lo:hi]))
        got = comp[order][:need]
        return np.concatenate([got, np.full(size - got.shape[0], ~np.uint64(0))])
    prefix, mask = 0, 0
    for sh in range(56, -1, -8):
        last = (hi - lo - 1) if defect == "skip_by_length" else (hi - 1)
        if sh < 32 and (last >> sh) == 0:
            if defect != "unmasked_skip":
                mask |= 0xFF << sh
            continue
        if defect == "ignore_digit16" and sh == 16:
            mask |= 0xFF << sh
            continue
        sel = (comp & np.uint64(mask)) == np.uint64(prefix)
        hist = np.bincount(((comp[sel] >> np.uint64(sh)) & np.uint64(255)).astype(np.int64), minlength=256)
        cum, b = 0, 0
        while b < 255 and cum + int(hist[b]) < need:
            cum += int(hist[b])
            b += 1
        prefix |= b << sh
        mask |= 0xFF << sh
        need -= cum
    got = np.sort(comp[comp <= np.uint64(prefix)][:size])
    return np.concatenate([got, np.full(size - got.shape[0], ~np.uint64(0))])


def emulate(case: Case, defect: Optional[str] = None, fill: float = float("nan")) -> Result:
    """The call of ``case`` in numpy; ``fill``: what the workspace holds on entry."""
    assert defect is None or defect in DEFECTS, defect
    g, k, m, d = case.g, case.k, case.m, case.d
    ns, bps, nq, chunks = case.plan
    findings: List[str] = []
    q, db = case.q, case.db
    q_inv = _inv_norms(q)
    db_inv = case.db_inv if case.db_inv is not None else _inv_norms(db)
    scoped = case.kind in ("scoped", "elect") and case.first is not None
    n = len(case.first) - 1 if scoped else 0
    q_scene = np.array(case.q_scene, dtype=np.int32) if scoped else None
    el = elects(case)
    if case.kind == "elect" and case.mode == ELECT_LOST:
        q_scene[el] = -1                                              # retrieve_mark_lost_kernel
    # ---- the product launch: flat `part` of exactly ns * g * m words, 16 more stand for what lies behind the workspace
    flat = np.full(ns * g * m + RT_ROWS, np.float32(fill), dtype=np.float32)
    flat[ns * g * m:] = np.float32(12345.0)
    part = flat[:ns * g * m].reshape(ns, g, m)
    store = np.ones((g, m), dtype=bool)
    if scoped and not (case.kind == "elect" and case.mode == ELECT_ALL):
        for j in range(g):
            ok, lo, hi = (True, 0, m) if el[j] else scope_of(case.first, n, int(q_scene[j]), m)
            store[j] = (np.arange(m) >= lo) & (np.arange(m) < hi)
    nblk = _cdiv(d, RT_BLK)
    with np.errstate(all="ignore"):
        for s, (b0, b1) in enumerate(slice_blocks(m, d)):
            if defect == "drop_block" and s == ns - 1:
                b1 -= 1
            waves = []
            for w in range(RT_WAVES):
                acc = np.zeros((g, m), dtype=np.float32)
                for b in range(b0 + w, b1, RT_WAVES):
                    c0, c1 = b * RT_BLK, min(b * RT_BLK + RT_BLK, d)
                    if defect == "ragged_float4" and b == nblk - 1 and d % RT_BLK:
                        c1 -= 4
                    acc = acc + (q[:, c0:c1] @ db[:, c0:c1].T).astype(np.float32)
                waves.append(acc)
            dots = ((waves[0] + waves[1]) + waves[2]) + waves[3]
            for j in range(g):
                dst = j - 16 * ((j % RT_QCHUNK) // 16) if defect == "mislaid_tile" else j
                part[s, dst, store[j]] = dots[j, store[j]]
            if defect == "tail_column_stored" and m % RT_ROWS:
                for j in range(g):
                    at = (s * g + j) * m + m
                    flat[at:at + RT_ROWS - m % RT_ROWS] = dots[j, m - 1]
    if not (flat[ns * g * m:] == np.float32(12345.0)).all():
        findings.append("the product launch wrote behind the workspace")

    def similarities(j, lo, hi, out):
        with np.errstate(all="ignore"):
            dot = part[0, j, lo:hi].copy()
            for s in range(1, ns - 1 if defect == "last_slice_out" and ns > 1 else ns):
                dot = dot + part[s, j, lo:hi]
            out[lo:hi] = (dot * q_inv[j]) * db_inv[lo:hi]

    # ---- the vote
    scene_info = np.zeros((g, 2), dtype=np.int32) if case.kind == "elect" else None
    if case.kind == "elect":
        for j in range(g):
            if not (case.mode == ELECT_ALL or q_scene[j] == -1):
                scene_info[j] = (q_scene[j], 0)
                continue
            sim = np.zeros(m, dtype=np.float32)
            similarities(j, 0, m, sim)
            top = min(K_MAX, m) if defect == "vote_beyond_top" else case.vote_top
            lst = radix_select(sim_keys(sim, defect), 0, m, top, K_MAX, defect)
            voters = [min(int(c & np.uint64(0xFFFFFFFF)), m - 1) for c in lst[:top] if c != ~np.uint64(0)]
            scene_info[j] = vote_int(voters, case.first, m)
            q_scene[j] = scene_info[j, 0]
    # ---- the selection
    nbrs = np.zeros((g, k), dtype=np.int64)
    sims = np.full((g, k), np.nan, dtype=np.float32)
    gate_info = np.zeros((g, 2), dtype=np.int32) if case.gate is not None else None
    status = 0
    for j in range(g):
        ok, lo, hi = (True, 0, m) if not scoped else scope_of(case.first, n, int(q_scene[j]), m)
        if defect == "sweep_from_0":
            lo = 0
        rows = np.arange(m)
        by_group = np.ones(m, dtype=bool)
        if case.q_group is not None and int(case.q_group[j]) != -1:
            by_group = np.asarray(case.db_group) != int(case.q_group[j])
        sim = np.zeros(m, dtype=np.float32)
        similarities(j, lo, hi, sim)
        keys = part[0, j].view(np.uint32).copy()                     # slice 0 becomes the keys, in place
        in_range = (rows >= lo) & (rows < hi)
        visited, allowed = in_range, in_range & by_group
        if case.gate is not None:
            state, inside = 1, 0
            if np.isfinite(case.gate["prior"][j]).all():
                lane = ((rows - lo) % (GATE_UNROLL * RS_NT)) // RS_NT
                seen = in_range & ~((lane == 3) if defect == "gate_lane3" else np.zeros(m, dtype=bool))
                both = seen & case.gate["inside"] & by_group
                inside = int(both.sum())
                state = 0 if inside >= int(case.ranks[j].max()) + 1 else 2
                if state == 0:
                    visited, allowed = seen, both
            gate_info[j] = (state, inside)
        keys[visited] = np.where(allowed[visited], sim_keys(sim[visited], defect), np.uint32(KEY_EXCLUDED))
        cl, r, bad = clamp_ranks(case.ranks[j], int(allowed.sum()), ok)
        status += bad
        if r == 0:
            continue
        lst = radix_select(keys, lo, hi, r, R_MAX, defect)
        comp = lst[cl]
        nbrs[j] = np.minimum((comp & np.uint64(0xFFFFFFFF)).astype(np.int64), m - 1)
        sims[j] = key_sims((comp >> np.uint64(32)).astype(np.uint32))
    return Result(nbrs, sims, status, gate_info, scene_info, q_scene if case.kind == "elect" else None, findings)


# ----------------------------------------------------------------------------------------------------------------------
# the checks a result is held to (the GPU's and the emulation's alike)
# ----------------------------------------------------------------------------------------------------------------------
def check_exact(case: Case, res: Result, want: Optional[Expect] = None) -> List[str]:
    """What is wrong with ``res`` on a lattice or integer case (empty: nothing)."""
    want = oracle(case) if want is None else want
    bad = list(res.findings)
    if res.status != want.status:
        bad.append(f"status {res.status}, the oracle counts {want.status}")
    for name in ("gate_info", "scene_info", "q_scene"):
        a, b = getattr(res, name), getattr(want, name)
        if b is not None and (a is None or not np.array_equal(np.asarray(a), b)):
            rows = [] if a is None else np.flatnonzero((np.asarray(a).reshape(case.g, -1) != b.reshape(case.g, -1)).any(1))[:4].tolist()
            bad.append(f"{name} differs from the oracle at queries {rows}")
    if not np.array_equal(res.nbrs, want.nbrs):
        j = int(np.flatnonzero((res.nbrs != want.nbrs).any(1))[0])
        bad.append(f"neighbours differ from the oracle at query {j}: {res.nbrs[j].tolist()} for {want.nbrs[j].tolist()}")
        return bad
    bits = np.asarray(res.sims, dtype=np.float32).view(np.uint32)
    bound = None
    if case.sim_scale is None:
        bound, exact = sim_bound(case.q, case.db)
    for j in range(case.g):
        s = np.asarray(res.sims[j], dtype=np.float32)
        if not want.ranked[j]:
            if not np.isnan(s).all():
                bad.append(f"query {j} ranks nothing and its sims are not NaN")
            continue
        rows = want.nbrs[j]
        nf = case.nonfinite[j, rows]
        if not (np.isnan(s) == nf).all():
            bad.append(f"query {j}: NaN sims do not sit at the non-finite rows")
            continue
        sc = case.score[j, rows]
        for a in range(case.k - 1):
            if nf[a] or nf[a + 1]:
                continue
            if sc[a] == sc[a + 1] and bits[j, a] != bits[j, a + 1]:
                bad.append(f"query {j}: sims of one tie class differ in bits at positions {a}, {a + 1}")
            if sc[a] > sc[a + 1] and not s[a] > s[a + 1]:
                bad.append(f"query {j}: sims do not decrease across classes at positions {a}, {a + 1}")
        fin = ~nf
        if case.sim_scale is not None:
            # similarity == class integer (sign(a) v) for |a| >= 1, and +-0 == 0 for the zero query and the underflowing rows
            wanted = sc[fin].astype(np.float32) * (np.float32(1.0) if np.any(case.q[j] != 0) else np.float32(0.0))
            if not np.array_equal(s[fin], wanted):
                bad.append(f"query {j}: sims are not the integers of the returned rows")
        elif not (np.abs(s[fin].astype(np.float64) - exact[j, rows[fin]]) <= bound[j, rows[fin]]).all():
            bad.append(f"query {j}: a sim is outside the a-priori bound of its row's exact similarity")
    return bad


def check_float(case: Case, res: Result) -> Tuple[List[str], Dict[str, float]]:
    """A float case (plain entry, no groups): -> (what is wrong, the observed error / bound figures)."""
    bound, s64 = sim_bound(case.q, case.db)
    g, m = case.g, case.m
    want = oracle(case, score=s64, nonfinite=np.zeros((g, m), dtype=bool))      # by float64 similarity, descending
    bad = list(res.findings)
    if res.status != want.status:
        bad.append(f"status {res.status}, the oracle counts {want.status}")
    if res.nbrs.min() < 0 or res.nbrs.max() >= m or any(len(set(r)) != len(r) for r in res.nbrs.tolist()):
        bad.append("neighbours outside the map or repeated")
        return bad, {}
    qi = np.arange(g)[:, None]
    err = np.abs(res.sims.astype(np.float64) - s64[qi, res.nbrs])
    r_sim = float((err / bound[qi, res.nbrs]).max())
    gap = np.abs(s64[qi, res.nbrs] - s64[qi, want.nbrs])
    r_pos = float((gap / (2.0 * bound.max(axis=1, keepdims=True))).max())
    if not r_sim <= 1.0:
        bad.append(f"a returned sim is {r_sim:.3f} x its a-priori bound away from the float64 similarity of its row")
    if not r_pos <= 1.0:
        bad.append(f"a returned row's float64 similarity is {r_pos:.3f} x (2 x bound) away from the oracle's row's")
    if not (np.diff(res.sims.astype(np.float64), axis=1) <= 0).all():
        bad.append("returned sims increase along a query's ranks")
    return bad, {"sim_error_over_bound": r_sim, "position_gap_over_2bound": r_pos,
                 "queries_differ": int((res.nbrs != want.nbrs).any(1).sum())}


# ----------------------------------------------------------------------------------------------------------------------
# the case lists
# ----------------------------------------------------------------------------------------------------------------------
PLAN_SHAPES = ((1, 4), (7, 8), (17, 60), (33, 64), (40, 260), (40, 1028), (100, 6340), (17, 8192), (1488, 6340), (1489, 6340))
# hand-worked in tests/test_retrieval_sweep_cpu.py: (nsplit, blocks_per_split)
PLAN_WANT = {(1, 4): (1, 1), (7, 8): (1, 1), (17, 60): (1, 1), (33, 64): (1, 1), (40, 260): (1, 5), (40, 1028): (2, 9),
             (100, 6340): (12, 9), (17, 8192): (16, 8), (1488, 6340): (12, 9), (1489, 6340): (10, 10)}
TILE_M = (15, 16, 17, 31, 32, 33)
QUERY_G = (1, 15, 16, 17, 32, 33, 48, 49, 64, 65, 81, 129)
SELECT_M = (1, 2, 255, 256, 257, 1023, 1024, 1025, 65535, 65536, 65537)
SELECT_R = (1, 2, 511, 512)
GATE_M = (2047, 2049, 3073, 4095, 4097, 8200)
ATLAS_SIZES = (200, 56, 1, 300, 65000, 700)
VOTE_TOPS = (1, 7, 64)


def _plan_g(m: int, d: int) -> int:
    return 3 if m * d > 1 << 20 else 17


PLAN_CASES = [Spec(f"plan_m{m}_d{d}", f"lattice at plan {PLAN_WANT[(m, d)]}", (lambda m=m, d=d: _lattice_case(m, d, _plan_g(m, d))))
              for m, d in PLAN_SHAPES]
TILE_CASES = [Spec(f"tile_m{m}", "16-row tile boundary, ragged d of two blocks", (lambda m=m: _lattice_case(m, 68, 3)))
              for m in TILE_M]
QUERY_CASES = [Spec(f"queries_g{g}", f"NQ {plan(g, 40, 260)[2]}, {plan(g, 40, 260)[3]} chunk(s)",
                    (lambda g=g: _lattice_case(40, 260, g))) for g in QUERY_G]


def _order_positions(case: Case, j: int, rows_allowed: np.ndarray, want_rows: Sequence[int]) -> List[int]:
    order = order_int(case.score[j], case.nonfinite[j], rows_allowed)[:R_MAX]
    pos = {int(r): p for p, r in enumerate(order.tolist())}
    return [pos[r] for r in want_rows if r in pos]


BOUNDARY_ROWS = (255, 256, 65535, 65536)


def _select_case(m: int, r: int) -> Case:
    """No groups; every query's ranks reach R = min(r, m) and hold the positions of the boundary rows its order reaches."""
    c = _int_case(m, "plain", INT_QUERIES)
    r = min(r, m)
    k = min(r, 12)
    rows = np.arange(m)
    c.ranks = np.stack([spread_ranks(k, r, _order_positions(c, j, rows, BOUNDARY_ROWS)) for j in range(c.g)])
    return c


def _select_group_case(m: int, where: str) -> Case:
    """Groups leave S = min(511, m) rows (label 0; every other row label 1): at the map's end, or spread over it with the boundary
    rows and the non-finite rows inside.  Queries 0-3 exclude label 1 with R == |S|, queries 4-5 with R == |S| + 1 (allowed == R - 1:
    one bad rank each), queries 6-7 have group -1."""
    c = _int_case(m, "plain", INT_QUERIES)
    n_s = min(511, m)
    if where == "end":
        s_rows = np.arange(m - n_s, m)
    else:
        _, _, nan = int_values(m)
        must = sorted({x for x in BOUNDARY_ROWS + (0, m - 1) if x < m} | set(np.flatnonzero(nan).tolist()))
        rest = np.setdiff1d(np.arange(m), must)
        take = rest[np.unique(np.linspace(0, len(rest) - 1, n_s - len(must)).astype(np.int64))] if n_s > len(must) else rest[:0]
        s_rows = np.array(sorted(set(must[:n_s]) | set(take.tolist())))
        n_s = len(s_rows)
    c.db_group = np.ones(m, dtype=np.int64)
    c.db_group[s_rows] = 0
    c.q_group = np.array([1, 1, 1, 1, 1, 1, -1, -1], dtype=np.int64)
    k = min(n_s, 12)
    ranks = []
    for j in range(c.g):
        if j < 4:
            ranks.append(spread_ranks(k, n_s, _order_positions(c, j, s_rows, BOUNDARY_ROWS) + [n_s - 7, n_s - 2]))
        elif j < 6:
            ranks.append(spread_ranks(k, n_s + 1, [n_s - 1]) if n_s + 1 <= R_MAX and k >= 2 else spread_ranks(k, n_s))
        else:
            ranks.append(spread_ranks(k, min(m, R_MAX), _order_positions(c, j, np.arange(m), BOUNDARY_ROWS)))
    c.ranks = np.stack(ranks)
    return c


SELECT_CASES = ([Spec(f"select_m{m}_R{r}", f"d = 8 integers, live digits {live_digits(0, m)}", (lambda m=m, r=r: _select_case(m, r)))
                 for m in SELECT_M for r in sorted({min(r, m) for r in SELECT_R})] +
                [Spec(f"select_m{m}_{w}", f"groups leave min(511, m) rows, {w}", (lambda m=m, w=w: _select_group_case(m, w)))
                 for m in SELECT_M for w in ("end", "spread")])


def gate_rows(m: int, lo: int = 0, hi: Optional[int] = None) -> List[int]:
    """Rows inside the gate: two in every (outer step, unroll lane) the range has, its first row and its last."""
    hi = m if hi is None else hi
    out = {lo, hi - 1}
    for base in range(lo, hi, RS_NT):
        out |= {r for r in (base + 3, base + 700) if r < hi}
    return sorted(out)


def _gate_arrays(m: int, g: int, inside_rows: Sequence[int], nan_prior: Sequence[int]) -> dict:
    inside = np.zeros(m, dtype=bool)
    inside[list(inside_rows)] = True
    db_gate = np.zeros((m, 7), dtype=np.float64)
    db_gate[:, 0] = np.where(inside, 0.5, 100.0)
    db_gate[:, 3] = 1.0
    far = np.flatnonzero(~inside)
    db_gate[far[::97], 1] = np.nan                                    # a non-finite gate row is outside whatever else it holds
    prior = np.zeros((g, 7), dtype=np.float64)
    prior[:, 3] = 1.0
    prior[list(nan_prior), 2] = np.nan
    return {"db_gate": db_gate, "prior": prior, "r2": 1.0, "inside": inside}


def _gate_case(m: int, groups: bool) -> Case:
    """Query 0, 1: gated, R == the rows inside (every one of them is returned); 2: no prior; 3: needs one more than are inside, falls
    back; with groups, label 1 takes two inside rows and some outside away from queries 0 and 3."""
    c = _int_case(m, "gated", INT_QUERIES[:4])
    ins = gate_rows(m)
    c.gate = _gate_arrays(m, c.g, ins, [2])
    n_in = len(ins)
    if groups:
        c.db_group = np.zeros(m, dtype=np.int64)
        c.db_group[[ins[1], ins[-1]] + list(range(7, m, 501))] = 1
        c.db_group[ins[2:-1]] = 0
        c.q_group = np.array([1, -1, 1, 1], dtype=np.int64)
    k = n_in - 2
    assert 2 <= k <= K_MAX, (m, k)
    n0 = n_in - 2 if groups else n_in
    c.ranks = np.stack([spread_ranks(k, n0), spread_ranks(k, n_in), spread_ranks(k, min(m, 300)), spread_ranks(k, n0 + 1)])
    return c


GATE_CASES = [Spec(f"gate_m{m}_{'groups' if gr else 'plain'}",
                   f"inside rows in steps {sorted({gate_step(r) for r in gate_rows(m)})[-1]} and below",
                   (lambda m=m, gr=gr: _gate_case(m, gr))) for m in GATE_M for gr in (False, True)]


def atlas_first(sizes=ATLAS_SIZES) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _atlas_values(v: np.ndarray, tiny: np.ndarray, nan: np.ndarray) -> None:
    """Ties across scene boundaries and across 65536 for the votes: column 2 of rows 198 .. 261 gets the largest value 7 (a query on
    column 2 with a > 0 sees them first: 2 rows of scene 0, all 56 of scene 1, scene 2's one, 5 of scene 3) and rows 65533 .. 65559
    the next value 6 (24 of scene 4, 3 of scene 5); the same rows hold column 0's largest value 8, so a query on column 0 with a > 0
    has its first voters on both sides of row 65536; none of them underflows or is non-finite."""
    for (a, b), col, val in (((198, 262), 2, 7), ((65533, 65560), 2, 6), ((65533, 65560), 0, 8)):
        v[a:b, col] = val
        tiny[a:b] = False
        nan[a:b] = False


# (value column, factor) of the atlas queries: 0-5 one per scene, 6 out of range, then more of the large scenes
ATLAS_QUERIES = ((0, 1), (1, 2), (0, -1), (2, 1), (1, 2), (0, 1), (0, 1), (2, 1), (0, 0), (1, -1), (2, 1), (2, -2))
ATLAS_SCENES = (0, 1, 2, 3, 4, 5, 6, 4, 4, 5, 0, -1)


def _atlas_case(kind: str, groups: bool, gated: bool, vote_top: int = 0, mode: int = 0, lattice_form: bool = False) -> Case:
    """``lattice_form``: +-1 in all 8 columns with the rows' own norms (nine tie classes over 66257 rows), which the existing
    oracles -- stated on ops.retrieve, which computes the norms itself -- can rank too."""
    m = int(np.sum(ATLAS_SIZES))
    if lattice_form:
        c = _lattice_case(m, 8, len(ATLAS_QUERIES), k=3, seed=77, w=8, kind=kind)
    else:
        c = _int_case(m, kind, ATLAS_QUERIES, edit=_atlas_values)
    c.first = atlas_first()
    c.q_scene = np.array(ATLAS_SCENES, dtype=np.int32)
    if kind == "elect" and mode == ELECT_ALL:
        c.q_scene = np.full(c.g, -77, dtype=np.int32)                 # an output only
    if kind == "elect" and mode == ELECT_LOST:
        c.q_scene = np.array([-1, 1, -1, -1, 4, -1, 6, -1, -1, 5, -1, -1], dtype=np.int32)
    c.vote_top, c.mode = vote_top, mode
    if groups:
        c.db_group = (np.arange(m) % 5 == 1).astype(np.int64)
        c.q_group = np.array([1, -1, 1, 1, 1, -1, 1, 1, -1, 1, -1, 1], dtype=np.int64)
    if gated:
        ins = sorted(set(gate_rows(m, 557, 65557)) | set(gate_rows(m, 0, 200)[:6]) | set(gate_rows(m, 65557, 66257)) | {256})
        c.gate = _gate_arrays(m, c.g, ins, [3, 9])
    c.ranks = np.stack([spread_ranks(3, r) for r in (200, 56, 3, 300, 512, 511, 3, 130, 512, 4, 5, 3)])
    if gated:
        c.ranks[4] = spread_ranks(3, 100)
        c.ranks[7] = spread_ranks(3, len(gate_rows(m, 557, 65557)))
    return c


SCOPE_CASES = [Spec("scope_plain", "ranges ending at 199 and 255, [256, 257), across 65536, above it, one scene out of range",
                    lambda: _atlas_case("scoped", False, False)),
               Spec("scope_groups_gate", "the same with groups and a gate whose sweep starts at lo = 557",
                    lambda: _atlas_case("scoped", True, True))]
VOTE_CASES = ([Spec(f"vote_all_top{v}", "every query elects over 66257 rows; ties across scene boundaries and 65536",
                    (lambda v=v: _atlas_case("elect", False, False, v, ELECT_ALL))) for v in VOTE_TOPS] +
              [Spec(f"vote_lost_top{v}", "held and electing queries, groups and gate (a lost prior elects)",
                    (lambda v=v: _atlas_case("elect", True, True, v, ELECT_LOST))) for v in VOTE_TOPS])

ATLAS_LATTICE_CASES = [Spec("atlas_lattice_scope", "the atlas on lattice rows: also held to scene_ref.oracle",
                            lambda: _atlas_case("scoped", True, True, lattice_form=True)),
                       Spec("atlas_lattice_vote_all_top7", "also held to scene_vote_ref.oracle",
                            lambda: _atlas_case("elect", False, False, 7, ELECT_ALL, lattice_form=True)),
                       Spec("atlas_lattice_vote_lost_top64", "also held to scene_vote_ref.oracle, groups and gate",
                            lambda: _atlas_case("elect", True, True, 64, ELECT_LOST, lattice_form=True))]


def _float_case(m: int, d: int, kind: str) -> Case:
    rng = np.random.RandomState(m + d + (0 if kind == "iid" else 1))
    g = _plan_g(m, d) if m > 1 else 3
    if kind == "iid":
        q, db = rng.standard_normal((g, d)), rng.standard_normal((m, d))
    else:
        walk = np.cumsum(rng.standard_normal((m, d)) * 0.05, axis=0) + rng.standard_normal(d)
        db = np.maximum(walk, 0)
        q = np.maximum(walk[rng.choice(m, g)] + 0.02 * rng.standard_normal((g, d)), 0)
    k = min(m, 8)
    ranks = np.stack([spread_ranks(k, min(m, R_MAX)) for _ in range(g)])
    return Case("", "", "plain", q.astype(np.float32), db.astype(np.float32), ranks)


FLOAT_CASES = [Spec(f"float_{kind}_m{m}_d{d}", f"{kind} data at plan {PLAN_WANT[(m, d)]}",
                    (lambda m=m, d=d, kind=kind: _float_case(m, d, kind))) for m, d in PLAN_SHAPES for kind in ("iid", "trajectory")]

EXACT_LISTS = {"plan": PLAN_CASES, "tile": TILE_CASES, "queries": QUERY_CASES, "select": SELECT_CASES, "gate": GATE_CASES,
               "scope": SCOPE_CASES, "vote": VOTE_CASES, "atlas_lattice": ATLAS_LATTICE_CASES}
# the lists meant to pin each defect
PINNED_BY = {"drop_block": ("plan",), "ragged_float4": ("plan", "tile"), "last_slice_out": ("plan",),
             "tail_column_stored": ("tile", "plan"), "mislaid_tile": ("queries",), "ties_desc_row": ("select",),
             "skip_by_length": ("scope",), "ignore_digit16": ("select", "scope", "vote"), "neg_zero_key": ("select",),
             "nonfinite_first": ("select",), "sweep_from_0": ("scope",), "gate_lane3": ("gate",), "vote_beyond_top": ("vote",)}
# "a skipped digit not added to the mask" changes nothing: every row of [lo, hi) has digit 0 there and so has the prefix, so
# (comp & mask) == prefix selects the same rows with or without those mask bits.  The emulation carries it to show exactly that;
# the defect next to it that does change results is the skip decided by the range's length, hi - lo - 1, in place of hi - 1.
UNOBSERVABLE = ("unmasked_skip",)


# ----------------------------------------------------------------------------------------------------------------------
# the memory harness of the C ABI
# ----------------------------------------------------------------------------------------------------------------------
MOAT_BYTES = 4096
IN_POISON, OUT_POISON = 0xFF, 0xA5          # 0xFF: NaN as fp32 / fp64, -1 as an integer; 0xA5: no value a launch writes


class Moated:
    """[moat | payload | moat] bytes on the device (the idea of encoder_sweep_ref.Moated for any element type): ``data`` (a numpy
    array) makes an input between 0xFF moats, ``nbytes`` an output that holds 0xA5 all over, ``fill`` (a 32-bit pattern) a
    workspace of exactly ``nbytes`` bytes filled with it."""

    def __init__(self, dev, data: Optional[np.ndarray] = None, nbytes: int = 0, fill: Optional[int] = None):
        import torch
        self.poison = IN_POISON if data is not None else OUT_POISON
        self.data = None if data is None else np.ascontiguousarray(data)
        self.nbytes = int(nbytes) if data is None else self.data.nbytes
        self.raw = torch.full((2 * MOAT_BYTES + self.nbytes,), self.poison, dtype=torch.uint8, device=dev)
        self.payload = self.raw[MOAT_BYTES:MOAT_BYTES + self.nbytes]
        if self.data is not None and self.nbytes:
            self.payload.copy_(torch.from_numpy(self.data.reshape(-1).view(np.uint8)))
        elif fill is not None:
            assert self.nbytes % 4 == 0
            self.payload.view(torch.int32).fill_(fill - (1 << 32) if fill >= 1 << 31 else fill)

    def ptr(self) -> int:
        return self.raw.data_ptr() + MOAT_BYTES

    def intact(self) -> bool:
        return bool((self.raw[:MOAT_BYTES] == self.poison).all()) and bool((self.raw[MOAT_BYTES + self.nbytes:] == self.poison).all())

    def unchanged(self) -> bool:
        import torch
        return bool(torch.equal(self.payload.cpu(), torch.from_numpy(self.data.reshape(-1).view(np.uint8))))

    def numpy(self, dtype, shape) -> np.ndarray:
        return self.payload.cpu().numpy().view(dtype).reshape(shape).copy()


NAN_WORD, ZERO_WORD = 0x7FC00000, 0


def launch(case: Case, dev, fill: int = NAN_WORD) -> Result:
    """``case`` through its entry point of the C ABI, every array inside moats, the workspace exactly the bytes the size function
    returns, pre-filled with ``fill``."""
    import torch
    from relpose_gnn_amd import _lib
    lib = _lib.lib()
    g, k, m, d = case.g, case.k, case.m, case.d
    ins: Dict[str, Moated] = {"q": Moated(dev, case.q), "db": Moated(dev, case.db), "ranks": Moated(dev, case.ranks.astype(np.int32))}
    for name, arr, dt in (("db_inv", case.db_inv, np.float32), ("q_group", case.q_group, np.int64), ("db_group", case.db_group, np.int64),
                          ("first", case.first if case.kind in ("scoped", "elect") else None, np.int64)):
        if arr is not None:
            ins[name] = Moated(dev, np.asarray(arr, dtype=dt))
    if case.gate is not None:
        ins["db_gate"] = Moated(dev, case.gate["db_gate"])
        ins["prior"] = Moated(dev, case.gate["prior"])
    p = lambda name: ins[name].ptr() if name in ins else None
    elect = case.kind == "elect"
    need = int((lib.rpg_retrieve_elect_workspace_bytes if elect else lib.rpg_retrieve_workspace_bytes)(g, m, d))
    outs: Dict[str, Moated] = {"nbrs": Moated(dev, nbytes=8 * g * k), "sims": Moated(dev, nbytes=4 * g * k),
                               "status": Moated(dev, nbytes=4, fill=0), "ws": Moated(dev, nbytes=need, fill=fill)}
    if case.gate is not None:
        outs["gate_info"] = Moated(dev, nbytes=8 * g)
    if elect:
        outs["scene_info"] = Moated(dev, nbytes=8 * g)
    q_scene = None
    if case.kind in ("scoped", "elect") and case.q_scene is not None:
        q_scene = Moated(dev, np.asarray(case.q_scene, dtype=np.int32))          # read by the scoped entry, in / out of the electing
    o = lambda name: outs[name].ptr() if name in outs else None
    gate = (p("db_gate"), p("prior"), float(case.gate["r2"]) if case.gate else 0.0, 0.0, 0, o("gate_info"))
    head = (p("q"), p("db"), p("db_inv"), p("q_group"), p("db_group"), p("ranks"), g, k, m, d)
    tail = (o("nbrs"), o("sims"), o("ws"), need, o("status"), None)
    if case.kind == "plain":
        rc = lib.rpg_retrieve_cosine_f32(*head, *tail)
    elif case.kind == "gated":
        rc = lib.rpg_retrieve_cosine_gated_f32(*head, *gate, *tail)
    elif case.kind == "scoped":
        rc = lib.rpg_retrieve_cosine_scoped_f32(*head, *gate, p("first"), q_scene.ptr(), len(case.first) - 1, *tail)
    else:
        rc = lib.rpg_retrieve_cosine_elect_f32(*head, *gate, p("first"), q_scene.ptr(), len(case.first) - 1, case.vote_top, case.mode,
                                               o("scene_info"), *tail)
    torch.cuda.synchronize()
    findings = [] if rc == 0 else [f"the entry point returned {rc}: {lib.rpg_last_error().decode()}"]
    findings += [f"the moat of {n} was written" for n, b in {**ins, **outs}.items() if not b.intact()]
    findings += [f"the input {n} was written" for n, b in ins.items() if not b.unchanged()]
    if q_scene is not None:
        if not q_scene.intact():
            findings.append("the moat of q_scene was written")
        if not elect and not q_scene.unchanged():
            findings.append("the scoped entry wrote q_scene")
    return Result(outs["nbrs"].numpy(np.int64, (g, k)), outs["sims"].numpy(np.float32, (g, k)),
                  int(outs["status"].numpy(np.int32, (1,))[0]),
                  outs["gate_info"].numpy(np.int32, (g, 2)) if "gate_info" in outs else None,
                  outs["scene_info"].numpy(np.int32, (g, 2)) if elect else None,
                  q_scene.numpy(np.int32, (g,)) if elect else None, findings)
