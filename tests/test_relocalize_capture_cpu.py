"""``relocalize(..., capture=...)`` without a GPU: the argument is refused for a map that is not on one, ``capture=False`` is the
call as it was, and anything but a bool is a TypeError -- all before any work is queued."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from relpose_gnn_amd import evaluate as E
from relpose_gnn_amd.graph import fc_edge_index

G, K, M = 5, 3, 9


class _FakeMapModel:
    """y = [the query's own row; fmap.poses[nb]] per graph, rel = y[dst] - y[src] + 0.01 over the FC list; counts its calls."""
    knn = -1

    def __init__(self):
        self.calls = 0

    def forward_map(self, x, nb, fmap):
        self.calls += 1
        y = torch.cat([x[:, None, :6], fmap.poses[nb]], 1).reshape(-1, 6)
        ei = torch.cat([fc_edge_index(K + 1) + g * (K + 1) for g in range(x.shape[0])], 1)
        return y, y[ei[1]] - y[ei[0]] + 0.01, ei


@pytest.fixture(scope="module")
def case():
    g = torch.Generator().manual_seed(7)
    table = torch.randn(M, 6, generator=g) * 0.3
    targets = torch.randn(G, 6, generator=g) * 0.3
    queries = torch.cat([targets, torch.zeros(G, 6)], 1)
    nb = torch.randint(0, M, (G, K), generator=g)
    fmap = SimpleNamespace(device=torch.device("cpu"), poses=table, features=table, descriptors=None)
    return fmap, queries, nb, targets


def test_capture_needs_a_gpu_map(case):
    fmap, queries, nb, targets = case
    model = _FakeMapModel()
    with pytest.raises(ValueError, match="capture"):
        E.relocalize(model, fmap, queries, nb, micro_batch=2, targets=targets, capture=True)
    assert model.calls == 0                                   # refused before any work


def test_capture_false_is_the_call_without_it(case):
    fmap, queries, nb, targets = case
    kw = dict(micro_batch=2, pose_m=(1.0, 2.0, 3.0), pose_s=(2.0, 2.0, 0.5), targets=targets)
    s0, s1 = {}, {}
    a = E.relocalize(_FakeMapModel(), fmap, queries, nb, stats=s0, **kw)
    b = E.relocalize(_FakeMapModel(), fmap, queries, nb, stats=s1, capture=False, **kw)
    for f in ("pred_poses", "targ_poses", "t_loss", "q_loss", "neighbours"):
        assert np.array_equal(getattr(a, f), getattr(b, f))
    assert set(s0) == set(s1) and "graphs_captured" not in s1
    for mode in ("mean", "median"):
        a = E.relocalize(_FakeMapModel(), fmap, queries, nb, fuse=mode, **kw)
        b = E.relocalize(_FakeMapModel(), fmap, queries, nb, fuse=mode, capture=False, **kw)
        assert np.array_equal(a.pred_poses, b.pred_poses) and np.array_equal(a.q_loss, b.q_loss)


@pytest.mark.parametrize("bad", [1, 0, None, "yes", np.True_])
def test_capture_must_be_a_bool(case, bad):
    fmap, queries, nb, _ = case
    model = _FakeMapModel()
    with pytest.raises(TypeError, match="capture"):
        E.relocalize(model, fmap, queries, nb, capture=bad)
    assert model.calls == 0
