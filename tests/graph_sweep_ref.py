"""Helpers shared by tests/test_hip_graph_sweep.py (GPU) and tests/test_graph_sweep_cpu.py: a seeded generator of irregular
edge lists, and plain CPU statements -- exact, or in float64 -- of the graph-side operations of csrc/gnn_ops.hip.
Test helper (like bf16_rounding.py and retrieval_ref.py): no test lives here."""
from typing import List, Optional, Sequence, Tuple

import torch

# every boundary of attention_aggregate's 8-wave split (7 | 8 | 9, 15 | 16 | 17), of its 8-row mbar chunk (the same numbers) and
# of scatter_mean's 4-way unroll (remainders 0 .. 3 at one, two and more trips); 40 = five full rounds of the 8 waves
IN_DEGREES = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 40)


# ----------------------------------------------------------------------------------------------------------------------
# graphs
# ----------------------------------------------------------------------------------------------------------------------
def _pick_degrees(a: int, e: Optional[int], classes: Sequence[int], g: torch.Generator) -> List[int]:
    """In-degrees of the ``a`` nodes that may have edges: every class once where a >= len(classes), the rest drawn from the
    classes; with ``e`` given the draws are steered so that the degrees sum to exactly e."""
    classes = sorted(classes)
    must = list(classes) if a >= len(classes) else []
    free = a - len(must)

    def draw(allowed):
        return allowed[int(torch.randint(0, len(allowed), (1,), generator=g))]

    if e is None:
        deg = must + [draw(classes) for _ in range(free)]
    else:
        tail = min(3, free)                                  # the last (up to) three free nodes absorb the remainder exactly
        r = e - sum(must)
        top = classes[-1]
        assert 0 <= r <= top * (free - tail) + (classes[-2] * tail if tail else 0), f"E = {e} is out of reach for {a} nodes"
        deg = list(must)
        for left in range(free - tail, 0, -1):               # `left` steered draws to go, this one included
            lo = r - (top * (left - 1) + classes[-2] * tail)  # what this draw must at least take
            c = draw([c for c in classes if lo <= c <= r])
            deg.append(c)
            r -= c
        small = [c for c in classes if c != top] + [top]
        combos = [[]] if tail == 0 else None
        if tail:                                              # exact remainder over the last nodes (13^3 candidates at the most)
            import itertools
            combos = [list(t) for t in itertools.product(small, repeat=tail) if sum(t) == r]
        assert combos, f"cannot place a remainder of {r} edges on {tail} nodes"
        deg += combos[int(torch.randint(0, len(combos), (1,), generator=g))]
    order = torch.randperm(a, generator=g).tolist()          # which node gets which degree
    return [deg[i] for i in order]


def irregular_edges(n: int, seed: int, e: Optional[int] = None, classes: Sequence[int] = IN_DEGREES, isolated: int = 2,
                    shuffle: bool = True) -> torch.Tensor:
    """Edge list [2, E] int64 over n nodes: per-node in-degrees from ``classes`` (every class occurs where the graph has the
    nodes for it), self-loops, repeated edges, the columns shuffled (neither grouped by target nor by source), and the last
    ``isolated`` nodes without any edge, incoming or outgoing.  ``e``: the exact edge count wanted (None: whatever the draw
    gives).  Deterministic per (n, seed, e, classes, isolated)."""
    a = n - isolated
    assert a >= 1
    g = torch.Generator().manual_seed(1000003 * seed + n)
    deg = _pick_degrees(a, e, classes, g)
    src, dst = [], []
    forced = False
    for v, k in enumerate(deg):
        if k == 0:
            continue
        s = torch.randint(0, a, (k,), generator=g)
        coin = torch.rand(2, generator=g)
        force = k >= 2 and not forced                        # the first node that can hold both: a self-loop AND a repeat
        if coin[0] < 0.25 or force:
            s[0] = v                                         # self-loop
        if k >= 2 and (coin[1] < 0.25 or force):
            s[k - 1] = s[k - 2] if k > 2 else s[0]           # repeated edge (k == 2 with a self-loop: the loop twice)
        forced = forced or force
        src.append(s)
        dst.append(torch.full((k,), v, dtype=torch.int64))
    if not src:
        return torch.zeros((2, 0), dtype=torch.int64)
    ei = torch.stack([torch.cat(src), torch.cat(dst)])
    if shuffle:
        ei = ei[:, torch.randperm(ei.shape[1], generator=g)]
    return ei.contiguous()


# (n, e) of the sweep: N = 1030 crosses graph_prepare's 1024-lane scan chunk; E < 1024 is one pass of its edge loops, E = 1024
# the boundary, E > 2048 more than two passes.  (37 nodes cannot hold 1024 edges with in-degrees of at most 40.)
SWEEP_GRAPHS = ((3, 17), (37, None), (1030, 1000), (1030, 1024), (1030, 2500))


def sweep_graph(n: int, e: Optional[int]) -> torch.Tensor:
    return irregular_edges(n, seed=7, e=e)


def in_degrees(ei: torch.Tensor, n: int) -> torch.Tensor:
    return torch.bincount(ei[1], minlength=n)


def has_repeat(ei: torch.Tensor, n: int) -> bool:
    key = ei[0] * n + ei[1]
    return bool(key.unique().numel() < key.numel())


def csr(ei: torch.Tensor, n: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(rowptr [n + 1], perm [E]) int64: the edges grouped by target, ascending edge id inside a target (stable sort)."""
    perm = torch.sort(ei[1], stable=True).indices
    rowptr = torch.cat([torch.zeros(1, dtype=torch.int64), in_degrees(ei, n).cumsum(0)])
    return rowptr, perm


# the composite forward's batch: graphs of 3, 8, 12, 1 and 9 nodes -- in-degree up to 11 in the 12-node graph (a second round of
# attention_aggregate's 8 waves), 9 in the 9-node one, isolated nodes, self-loops, repeated edges, and a graph without any edge
FORWARD_SIZES = (3, 8, 12, 1, 9)
_FORWARD_CLASSES = {3: ((1, 2, 4), 1), 8: ((0, 1, 2, 3, 5, 7, 8), 1), 12: ((0, 1, 3, 4, 8, 9, 11), 1), 9: ((1, 2, 5, 9), 0)}


def forward_graph_edges(seed: int = 5) -> List[torch.Tensor]:
    """Per graph of FORWARD_SIZES its local edge list [2, E_g] (columns shuffled inside the graph)."""
    out = []
    for n in FORWARD_SIZES:
        if n == 1:
            out.append(torch.zeros((2, 0), dtype=torch.int64))
        else:
            classes, iso = _FORWARD_CLASSES[n]
            out.append(irregular_edges(n, seed, classes=classes, isolated=iso))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# exact references
# ----------------------------------------------------------------------------------------------------------------------
def scatter_mean_ordered(msg: torch.Tensor, ei: torch.Tensor, n: int) -> torch.Tensor:
    """scatter-mean with a STATED order: per target the rows are added in ascending edge id, one IEEE addition each in msg's
    dtype, starting from zero, then one division by the in-degree (isolated nodes: zero).  A loop over the position inside the
    target's segment, vectorised over the nodes; nothing is left to index_add_'s order."""
    rowptr, perm = csr(ei, n)
    deg = rowptr[1:] - rowptr[:-1]
    acc = torch.zeros((n, msg.shape[1]), dtype=msg.dtype)
    for j in range(int(deg.max()) if deg.numel() else 0):
        nodes = (deg > j).nonzero().flatten()
        acc[nodes] = acc[nodes] + msg[perm[rowptr[nodes] + j]]
    return acc / deg.clamp(min=1).to(msg.dtype).unsqueeze(1)


def gather_add2_relu_ref(pq: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    d = pq.shape[1] // 2
    return torch.relu((pq[lo][:, :d] + pq[hi][:, d:]) + bias)


def knn_graph_exact(x: torch.Tensor, k: int, batch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """oracle.knn_graph restated without its per-node Python loop, for INTEGER-valued x: per graph the exact integer matrix of
    squared distances, a stable argsort of each row (ties: lower index first), the first k + 1 columns, the self match
    dropped; row 0 = neighbour, row 1 = query node, grouped by target in node order, nearest first."""
    xi = x.to(torch.int64)
    assert torch.equal(xi.to(x.dtype), x), "knn_graph_exact is for integer-valued features"
    n = x.shape[0]
    batch = torch.zeros(n, dtype=torch.int64) if batch is None else batch
    src, dst = [], []
    sizes = torch.unique_consecutive(batch, return_counts=True)[1].tolist()
    lo = 0
    for m in sizes:
        xg = xi[lo:lo + m]
        sq = (xg * xg).sum(1)
        dist = sq[:, None] + sq[None, :] - 2 * (xg @ xg.t())            # exact in int64
        order = torch.sort(dist, dim=1, stable=True).indices[:, :k + 1]
        tgt = torch.arange(m).unsqueeze(1).expand_as(order)
        keep = order != tgt
        src.append(order[keep] + lo)
        dst.append(tgt[keep] + lo)
        lo += m
    return torch.stack([torch.cat(src), torch.cat(dst)])


def integer_features(n: int, d: int, seed: int) -> torch.Tensor:
    """fp32 [n, d] with integer coordinates in [-4, 4]: a squared distance is an integer of at most 64 d <= 2^17 for d <= 2048,
    far below 2^24, so it is exact in fp32 in any summation order and ties are ties on every side."""
    return torch.randint(-4, 5, (n, d), generator=torch.Generator().manual_seed(seed)).float()


# ----------------------------------------------------------------------------------------------------------------------
# float64 references and the element-wise metric
# ----------------------------------------------------------------------------------------------------------------------
def attention_rows_ref(gtp: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """att.py:20-31 on rows of gtp = [g | theta | phi], evaluated in ``dtype`` on the given (fp32) values: torch's softmax and
    bmm, i.e. with dtype = float32 the CPU fp32 statement of the operation."""
    c = gtp.shape[1] // 3
    t = gtp.to(dtype)
    g, th, ph = t[:, :c], t[:, c:2 * c], t[:, 2 * c:]
    a = torch.softmax(ph.unsqueeze(2) * th.unsqueeze(1), dim=-1)
    return torch.bmm(a, g.unsqueeze(2)).squeeze(2)


def attention_mean_ref(gtp: torch.Tensor, ei: torch.Tensor, n: int, dtype=torch.float64) -> torch.Tensor:
    """ybar of rpg_attention_aggregate_f32: the per-target mean of the attention rows, everything in ``dtype``."""
    return scatter_mean_ordered(attention_rows_ref(gtp, dtype), ei, n)


def rowwise_err(y: torch.Tensor, z: torch.Tensor, rows: Optional[torch.Tensor] = None) -> float:
    """max |y - z| / (|z| + s), s = the float64 root-mean-square of z's row: element-wise, so that a wrong small element of a
    row with large ones still shows.  ``rows``: only those rows (an all-zero row of an isolated node has s = 0)."""
    y, z = y.double(), z.double()
    if rows is not None:
        y, z = y[rows], z[rows]
    s = z.pow(2).mean(1, keepdim=True).sqrt()
    return float(((y - z).abs() / (z.abs() + s)).max())


def pose_heads_err(y: torch.Tensor, x: torch.Tensor, w6: torch.Tensor, b6: torch.Tensor) -> float:
    """max |y - z| / (|z| + s) against z = x W^T + b in float64, s = sum_k |x_k w_k| + |b| of that element."""
    xd, wd, bd = x.double(), w6.double(), b6.double()
    z = xd @ wd.t() + bd
    s = xd.abs() @ wd.abs().t() + bd.abs()
    return float(((y.double() - z).abs() / (z.abs() + s)).max())


REGIMES = ("normal", "large", "tiny")


def attention_inputs(rows: int, c: int, regime: str, seed: int) -> torch.Tensor:
    """gtp [rows, 3c] fp32.  "normal": N(0, 1.5^2), the existing tests' values.  "large": theta and phi rescaled so that
    max |phi| max |theta| = 80 (both signs of phi occur, so both the max-theta and the min-theta shift), row 0's theta all
    equal (max theta == min theta).  "tiny": everything times 1e-20 (every logit is a denormal or zero)."""
    gtp = torch.randn(rows, 3 * c, generator=torch.Generator().manual_seed(seed)) * 1.5
    if regime == "large":
        th, ph = gtp[:, c:2 * c], gtp[:, 2 * c:]
        gtp[0, c:2 * c] = 0.75
        a = (80.0 / float(th.abs().max() * ph.abs().max())) ** 0.5
        th *= a
        ph *= a
    elif regime == "tiny":
        gtp = gtp * 1e-20
    else:
        assert regime == "normal"
    return gtp.contiguous()


# ----------------------------------------------------------------------------------------------------------------------
# the composite forward's batch
# ----------------------------------------------------------------------------------------------------------------------
FWD_D, FWD_H, FWD_W, FWD_PLANES, FWD_BLOCKS = 64, 32, 40, (8, 16, 32, 64), (1, 1, 1, 1)


def forward_batch(seed: int = 5):
    """(images [33, 3*H*W], per-graph local edge lists, grouped edge list [2, E] with node offsets, batch vector [33])."""
    import relpose_gnn_amd.synth as S
    local = forward_graph_edges(seed)
    xs = [S.synth_images(n, FWD_H, FWD_W, seed=400 + i) for i, n in enumerate(FORWARD_SIZES)]
    offs = [sum(FORWARD_SIZES[:i]) for i in range(len(FORWARD_SIZES))]
    ei = torch.cat([e + o for e, o in zip(local, offs)], dim=1)
    batch = torch.cat([torch.full((n,), i, dtype=torch.int64) for i, n in enumerate(FORWARD_SIZES)])
    return torch.cat(xs, 0), local, ei, batch


def forward_state_dict(seed: int = 1):
    import relpose_gnn_amd.synth as S
    return S.synth_state_dict(S.posenet_r2_param_shapes(FWD_D, FWD_D, FWD_D, FWD_PLANES, FWD_BLOCKS), seed=seed)


def oracle_forward(sd, x, ei, dtype=torch.float32, **kw):
    """oracle.posenet_forward with the state dict and the images cast to ``dtype`` -> (abs, rel, edge_index)."""
    from oracle import posenet_ref as O
    sd = {k: (v.to(dtype) if torch.is_floating_point(v) else v) for k, v in sd.items()}
    return O.posenet_forward(sd, x.to(dtype), ei, FWD_H, 2, **kw)


def wave_order_mean(y: torch.Tensor, ei: torch.Tensor, n: int, waves: int = 8) -> torch.Tensor:
    """The per-target mean of the rows y in the order rpg_attention_aggregate_f32 documents for ybar: wave w adds the target's
    edges w, w + 8, ... (ascending edge id) into its partial, the partials are added in wave order, one division by the
    in-degree.  In y's dtype, every step one IEEE operation.  Up to 8 incoming edges this is the ascending-edge-id sum."""
    rowptr, perm = csr(ei, n)
    out = torch.zeros((n, y.shape[1]), dtype=y.dtype)
    for v in range(n):
        ids = perm[rowptr[v]:rowptr[v + 1]]
        if ids.numel() == 0:
            continue
        part = []
        for w in range(waves):
            acc = torch.zeros(y.shape[1], dtype=y.dtype)
            for i in ids[w::waves].tolist():
                acc = acc + y[i]
            part.append(acc)
        tot = part[0]
        for w in range(1, waves):
            tot = tot + part[w]
        out[v] = tot / float(ids.numel())
    return out
