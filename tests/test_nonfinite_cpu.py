"""The reference's contract on non-finite input (CPU oracle only, no GPU): a bad pixel poisons its own graph and nothing else.

torch's conv, BatchNorm, avg-pool, relu and max_pool2d all propagate NaN, so one non-finite (or huge) pixel in image i makes every
abs-pose row of i's graph and every rel-pose row of that graph's edges non-finite, while the other graphs of the batch are
bit-identical to the clean run.  A NaN in one weight makes every output non-finite.  tests/test_hip_nonfinite.py holds the HIP
kernels and the HIP forward to the same contract."""
import pytest
import torch

D, H, W = 64, 32, 40
PLANES, BLOCKS = (8, 16, 32, 64), (1, 1, 1, 1)
GRAPHS, NODES = 3, 8
BAD_IMAGE = 9                                   # node 1 of graph 1


@pytest.fixture(scope="module")
def model():
    import relpose_gnn_amd.synth as S
    from relpose_gnn_amd.graph import fc_batch
    sd = S.synth_state_dict(S.posenet_r2_param_shapes(D, D, D, PLANES, BLOCKS), seed=1)
    x = S.synth_images(GRAPHS * NODES, H, W, seed=11)
    ei = fc_batch(x, NODES).edge_index
    return sd, x, ei


def _forward(sd, x, ei):
    from oracle import posenet_ref as O
    a, r, _ = O.posenet_forward(sd, x, ei, H, 2)
    return a, r


def _rows(ei, g):
    """abs rows of graph g, rel rows of the edges inside graph g"""
    nodes = torch.zeros(GRAPHS * NODES, dtype=torch.bool)
    nodes[g * NODES:(g + 1) * NODES] = True
    edges = (ei[0] // NODES == g) & (ei[1] // NODES == g)
    return nodes, edges


BAD = {"nan": float("nan"), "-nan": torch.tensor(0xFFC00000, dtype=torch.int64).to(torch.int32).view(torch.float32).item(),
       "+inf": float("inf"), "-inf": float("-inf"), "1e30": 1e30}


@pytest.mark.parametrize("kind", list(BAD))
def test_bad_pixel_poisons_its_graph_only(model, kind):
    sd, x, ei = model
    a0, r0 = _forward(sd, x, ei)
    assert bool(torch.isfinite(a0).all()) and bool(torch.isfinite(r0).all())
    nodes, edges = _rows(ei, BAD_IMAGE // NODES)
    assert int(edges.sum()) == NODES * (NODES - 1)
    for c, y, xx in ((0, 0, 0), (1, H // 2, W // 3), (2, H - 1, W - 1)):      # a corner, an interior pixel, the last element
        xb = x.clone()
        xb[BAD_IMAGE, (c * H + y) * W + xx] = BAD[kind]               # data.x rows are flattened CHW images
        a, r = _forward(sd, xb, ei)
        # every row of the poisoned graph is non-finite (all six pose components need not be: the heads mix them, so any is enough)
        assert bool((~torch.isfinite(a[nodes])).any(dim=1).all()), (kind, c, y, xx)
        assert bool((~torch.isfinite(r[edges])).any(dim=1).all()), (kind, c, y, xx)
        # the other graphs: bit for bit the clean run
        assert torch.equal(a[~nodes], a0[~nodes]) and torch.equal(r[~edges], r0[~edges]), (kind, c, y, xx)


def test_nan_weight_poisons_every_output(model):
    sd, x, ei = model
    sd = dict(sd)
    w = sd["feature_extractor.layer3.0.conv1.weight"].clone()
    w.view(-1)[w.numel() // 3] = float("nan")
    sd["feature_extractor.layer3.0.conv1.weight"] = w
    a, r = _forward(sd, x, ei)
    assert bool(torch.isnan(a).any(dim=1).all()) and bool(torch.isnan(r).any(dim=1).all())
