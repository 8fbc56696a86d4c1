"""The algebra of the mean-first message path, before any kernel runs (no GPU): the two formulations of one message-and-aggregate
step stated in tests/gnn_mean_first_ref.py agree in float64, the isolated node's aggregate is exactly zero, and params.pack_gnn_mean_first
packs the operands the second formulation reads.

Bound.  The formulations differ by the order of float64 sums of at most K = D + D/8 = 2304 terms (2304 * 2^-53 = 2.6e-13 of the sum
of magnitudes each), through three chained stages, one of them a softmax whose arguments are O(10) here: 1e-10 on max|a - b| / max|b|
leaves two orders of magnitude, and a dropped term, a bias counted twice or a bias on the wrong rows is 1e-3 or more.
"""
import pytest
import torch

import gnn_mean_first_ref as R

BOUND = 1e-10

GRAPHS = {"ragged_fc_8_5_8": R.ragged_fc_batch, "knn_like_isolated": R.knn_like_graph, "duplicated_edges": R.duplicated_edges_graph}


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("d", [64, 256])
@pytest.mark.parametrize("graph", list(GRAPHS))
def test_mean_first_equals_reference_in_float64(graph, d):
    ei, n = GRAPHS[graph]()
    dst = ei[1]
    ops = R.step_operands(d, ei.shape[1], seed=d + len(graph))
    ref = R.step_reference(ops[0], dst, n, *ops[1:])
    new = R.step_mean_first(ops[0], dst, n, *ops[1:])
    assert ref.dtype == new.dtype == torch.float64 and ref.shape == new.shape == (n, d)
    assert _rel(new, ref) < BOUND, (graph, d, _rel(new, ref))
    indeg = torch.bincount(dst, minlength=n)
    if graph == "knn_like_isolated":
        assert indeg.tolist() == list(R.IN_DEGREES) and indeg.min() == 0 and indeg.max() == 6
        assert not ref[R.ISOLATED].any() and not new[R.ISOLATED].any()            # exactly zero, as scatter_mean gives it
        # the bias rule: through the Linear's bias operand the isolated row would carry b_att + b_2
        wrong = R.step_mean_first(ops[0], dst, n, *ops[1:], bias_as_residual=False)
        assert torch.equal(wrong[R.ISOLATED], ops[6] + ops[2]) and wrong[R.ISOLATED].abs().max() > 1e-3
        assert _rel(wrong[1:], ref[1:]) < BOUND
    else:
        assert indeg.min() > 0
    if graph == "duplicated_edges":
        pairs = list(zip(*ei.tolist()))
        assert pairs.count((1, 0)) == 3 and pairs.count((2, 3)) == 2


def test_pack_gnn_mean_first():
    """Slots 26..29: the float64 products rounded once, the concatenation along K, the summed biases; 26 tensors in, 4 out."""
    import relpose_gnn_amd.synth as S
    from relpose_gnn_amd.params import pack_gnn, pack_gnn_bf16, pack_gnn_mean_first
    d, c = 64, 8
    sd = S.synth_state_dict(S.posenet_r2_param_shapes(d, d, d, (8, 16, 32, 64), (1, 1, 1, 1)), seed=2)
    t = pack_gnn(sd)
    m = pack_gnn_mean_first(t)
    assert [tuple(v.shape) for v in m] == [(3 * c, d), (3 * c,), (d, d + c), (d,)]
    assert all(v.dtype == torch.float32 and v.is_contiguous() for v in m)
    w2, b2 = sd["gnn1.mlp.2.weight"].double(), sd["gnn1.mlp.2.bias"].double()
    wg = torch.cat([sd[f"gnn1.att.{k}.weight"] for k in ("g", "theta", "phi")]).double()
    bg = torch.cat([sd[f"gnn1.att.{k}.bias"] for k in ("g", "theta", "phi")]).double()
    assert torch.equal(m[0], (wg @ w2).float()) and torch.equal(m[1], (wg @ b2 + bg).float())
    assert torch.equal(m[2][:, :d], sd["gnn1.mlp.2.weight"]) and torch.equal(m[2][:, d:], sd["gnn1.att.W.weight"])
    assert torch.equal(m[3], sd["gnn1.att.W.bias"] + sd["gnn1.mlp.2.bias"])
    # rounded once: the fp32 product of the fp32 factors is a different (noisier) tensor
    assert not torch.equal(m[0], wg.float() @ w2.float())
    assert len(pack_gnn_bf16(t + m)) == len(pack_gnn_bf16(t)) == 10               # the bf16 table ignores the four
    with pytest.raises(ValueError):
        pack_gnn_mean_first(t[:22])
