"""What tests/test_gnn_mean_first_cpu.py and tests/test_hip_gnn_mean_first.py share: the three small graphs and the two
formulations of one message-and-aggregate step of simpleConvEdge_upt (my_gnn_layer.py:301,304-307; att.py:20-33), in plain torch
and in whatever dtype the operands come in.

The step starts at h_k = relu(mlp.0(cat[x_src, e_new])) of edge k (the HIP forward's buffer `hid`) and ends at the aggregate:

    reference    msg_k = W2 h_k + b2;  gtp_k = Wg msg_k + bg;  y_k = attention row of gtp_k;  att_k = Wa y_k + ba + msg_k;
                 agg_i = mean over the edges k -> i of att_k               (zeros for a node without incoming edges)
    mean first   gtp_k = (Wg W2) h_k + (Wg b2 + bg);  y_k as above;  hbar_i, ybar_i = means over the edges k -> i of h_k, y_k;
                 agg_i = cat(W2, Wa) [hbar_i ; ybar_i] + res_i,   res_i = ba + b2 where node i has an incoming edge, else zeros
"""
import torch


def fc_edges(n: int) -> torch.Tensor:
    """Every ordered pair (s, t), s != t, of n nodes, grouped by target."""
    return torch.tensor([[s for t in range(n) for s in range(n) if s != t], [t for t in range(n) for s in range(n) if s != t]],
                        dtype=torch.int64)


def ragged_fc_batch(sizes=(8, 5, 8)) -> tuple:
    """Fully connected graphs of the given sizes in one batch -> (edge_index, n)."""
    off, parts = 0, []
    for k in sizes:
        parts.append(fc_edges(k) + off)
        off += k
    return torch.cat(parts, 1).contiguous(), off


IN_DEGREES = (0, 1, 2, 3, 4, 5, 6, 2)          # node 0 has no incoming edge (it is a source of others)
ISOLATED = 0


def knn_like_graph() -> tuple:
    """8 nodes, node i with IN_DEGREES[i] incoming edges from the nodes i + 1, i + 2, ... (mod 8): no self-loop, in-degrees 0 .. 6,
    the columns grouped by target as a kNN build leaves them -> (edge_index, n)."""
    n = len(IN_DEGREES)
    src = [(i + 1 + j) % n for i, k in enumerate(IN_DEGREES) for j in range(k)]
    dst = [i for i, k in enumerate(IN_DEGREES) for _ in range(k)]
    return torch.tensor([src, dst], dtype=torch.int64), n


def duplicated_edges_graph() -> tuple:
    """5 nodes; edge 1 -> 0 three times, 2 -> 3 twice (not adjacent in the list), the rest once; every node has an incoming edge."""
    src = [1, 2, 1, 4, 0, 1, 2, 3, 0, 2]
    dst = [0, 3, 0, 1, 2, 0, 4, 4, 1, 3]
    return torch.tensor([src, dst], dtype=torch.int64), 5


def attention_rows(gtp: torch.Tensor) -> torch.Tensor:
    """att.py:20-31 row-wise on gtp = [g | theta | phi]: y_i = sum_j softmax_j(phi_i theta_j) g_j."""
    c = gtp.shape[1] // 3
    g, th, ph = gtp[:, :c], gtp[:, c:2 * c], gtp[:, 2 * c:]
    a = torch.softmax(ph.unsqueeze(2) * th.unsqueeze(1), dim=-1)
    return torch.bmm(a, g.unsqueeze(2)).squeeze(2)


def scatter_mean(rows: torch.Tensor, dst: torch.Tensor, n: int):
    """(mean of the rows into every target, in-degree): rows added in ascending edge order, zeros for in-degree 0."""
    out = torch.zeros(n, rows.shape[1], dtype=rows.dtype)
    out.index_add_(0, dst, rows)
    cnt = torch.bincount(dst, minlength=n)
    return out / cnt.clamp(min=1).to(rows.dtype).unsqueeze(1), cnt


def step_reference(h, dst, n, w2, b2, wg, bg, wa, ba):
    msg = h @ w2.T + b2
    y = attention_rows(msg @ wg.T + bg)
    return scatter_mean(y @ wa.T + ba + msg, dst, n)[0]


def step_mean_first(h, dst, n, w2, b2, wg, bg, wa, ba, bias_as_residual: bool = True):
    """``bias_as_residual=False`` is the defect the residual row exists to prevent: ba + b2 as the node Linear's bias operand."""
    y = attention_rows(h @ (wg @ w2).T + (wg @ b2 + bg))
    hbar, cnt = scatter_mean(h, dst, n)
    ybar, _ = scatter_mean(y, dst, n)
    bias = ba + b2
    res = torch.where((cnt > 0).unsqueeze(1), bias.unsqueeze(0), torch.zeros_like(bias).unsqueeze(0))
    lin = torch.cat([hbar, ybar], 1) @ torch.cat([w2, wa], 1).T
    return lin + res if bias_as_residual else lin + bias


def step_operands(d: int, e: int, seed: int, dtype=torch.float64):
    """h [e, d] >= 0 as a ReLU leaves it, and the six weights at the scale of a default-initialised Linear (c = d / 8)."""
    g = torch.Generator().manual_seed(seed)
    c = d // 8

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).to(dtype)
    h = rnd(e, d).clamp(min=0)
    return (h, rnd(d, d, scale=d ** -0.5), rnd(d, scale=0.05), rnd(3 * c, d, scale=d ** -0.5), rnd(3 * c, scale=0.05),
            rnd(d, c, scale=c ** -0.5), rnd(d, scale=0.05))
