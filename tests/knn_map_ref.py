"""Reference statements for the kNN graph of equal-sized graphs at fixed positions (rpg_knn_graph_uniform_f32), built on
``graph_sweep_ref.knn_graph_exact`` (integer-valued features: every squared distance is exact, ties are ties on every side).

For g graphs of n_per nodes, k' = min(k, n_per - 1).  A node is REGULAR when the reference list gives it exactly k' incoming
edges; then its columns are v k' + [0, k').  An irregular node (its self match is not among its k + 1 nearest by (distance, index):
k + 1 or more lower-numbered nodes of its graph hold a bit-identical row) has k' + 1 edges in the reference; the fixed layout keeps
the first k' of them and counts the node."""
import torch

import graph_sweep_ref as R


def uniform_batch(g: int, n_per: int) -> torch.Tensor:
    return torch.arange(g, dtype=torch.int64).repeat_interleave(n_per)


def reference_in_degrees(x: torch.Tensor, g: int, n_per: int, k: int) -> torch.Tensor:
    ei = R.knn_graph_exact(x, k, uniform_batch(g, n_per))
    return torch.bincount(ei[1], minlength=g * n_per)


def irregular_nodes(x: torch.Tensor, g: int, n_per: int, k: int) -> int:
    """Nodes whose reference in-degree is not k'."""
    return int((reference_in_degrees(x, g, n_per, k) != min(k, n_per - 1)).sum())


def uniform_knn(x: torch.Tensor, g: int, n_per: int, k: int, node_offset: int = 0) -> torch.Tensor:
    """[2, g n_per k'] int64: column v k' + t = (t-th nearest other node of v, v), the first k' reference edges into every node."""
    kp = min(k, n_per - 1)
    ei = R.knn_graph_exact(x, k, uniform_batch(g, n_per))
    deg = torch.bincount(ei[1], minlength=g * n_per)
    assert int(deg.min()) >= kp and int(deg.max()) <= kp + 1
    first = torch.cumsum(deg, 0) - deg                                   # the list is grouped by target in node order
    cols = (first[:, None] + torch.arange(kp)[None, :]).reshape(-1)
    out = ei[:, cols] + node_offset
    assert torch.equal(out[1], torch.arange(g * n_per).repeat_interleave(kp) + node_offset)
    return out


def insertion_knn(x: torch.Tensor, g: int, n_per: int, k: int):
    """The selection rule as ``rpg_knn_graph_f32`` documents it, stated for ANY float features, non-finite ones included: per
    node the candidates of its graph in index order, a candidate enters the sorted list of at most k + 1 only where it is
    strictly nearer than an entry (every comparison with a NaN distance is false: a NaN candidate is appended while the list
    fills and never afterwards, and nothing passes a NaN entry), the self match dropped.  Distances are plain float64 sums, so
    this is for features without near ties (which of them are finite, Inf or NaN does not depend on the summation order).
    -> (the first k' entries of every node's list [2, g n_per k'], the number of nodes whose list has other than k' entries)."""
    kp = min(k, n_per - 1)
    xd = x.double()
    src, dst, irregular = [], [], 0
    for gi in range(g):
        xg = xd[gi * n_per:(gi + 1) * n_per]
        for v in range(n_per):
            dist = ((xg - xg[v]) ** 2).sum(1).tolist()
            best = []                                             # (distance, index), at most k + 1
            for j, dj in enumerate(dist):
                if len(best) < k + 1 or dj < best[-1][0]:
                    p = min(len(best), k)
                    while p > 0 and dj < best[p - 1][0]:
                        p -= 1
                    best.insert(p, (dj, j))
                    del best[k + 1:]
            others = [j for _, j in best if j != v]
            irregular += len(others) != kp
            src += [gi * n_per + j for j in others[:kp]]
            dst += [gi * n_per + v] * kp
    return torch.tensor([src, dst], dtype=torch.int64), irregular


def query_columns(g: int, n_per: int, k: int) -> torch.Tensor:
    """The columns into node 0 of every graph: g n_per k' + [0, k')."""
    kp = min(k, n_per - 1)
    return (torch.arange(g)[:, None] * (n_per * kp) + torch.arange(kp)[None, :]).reshape(-1)


def duplicate_rows_example(d: int = 8) -> torch.Tensor:
    """Eight nodes, rows 1..6 identical, k = 4: node 6 sees five lower-numbered copies of itself at distance 0, so its self match is
    sixth in its list and it keeps five edges -- in-degrees [4, 4, 4, 4, 4, 4, 5, 4], 33 edges."""
    x = R.integer_features(8, d, seed=3)
    x[1:7] = x[1]
    return x


def planted_ties(g: int, n_per: int, d: int, seed: int) -> torch.Tensor:
    """Integer features with exact distance ties (a row at +e0 and one at -e0 of another) and, where the graph is large enough, one
    duplicated row per graph -- too few copies to make a node irregular for k >= 1 when only one copy exists."""
    x = R.integer_features(g * n_per, d, seed)
    for gi in range(g):
        b = gi * n_per
        if n_per >= 3:
            x[b + 1] = x[b]
            x[b + 2] = x[b]
            x[b + 1, 0] += 1
            x[b + 2, 0] -= 1                      # nodes 1 and 2 are equally far from node 0
        if n_per >= 5:
            x[b + 4] = x[b + 3]                   # one duplicate
    return x
