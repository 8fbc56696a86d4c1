"""The micro-batch pipeline without a GPU (relpose_gnn_amd.pipeline): the order of the three-stage driver, the staging-dtype
rule, and ``relocalize`` on the runner's synchronous path against ``evaluate_stream`` over the same graphs."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from relpose_gnn_amd import evaluate as E
from relpose_gnn_amd import pipeline as P
from relpose_gnn_amd.graph import Data, fc_edge_index


@pytest.mark.parametrize("n", [0, 1, 2, 3])
def test_driver_order(n):
    """launch(0); then per micro-batch i: prefetch(i + 1), finish(i - 1), launch(i + 1); then the last finish.  Nothing is
    called for an empty stream, nothing is prefetched after the last chunk, every chunk is built once."""
    log, built = [], []

    def chunk_at(i):
        built.append(i)
        return f"chunk{i}"

    def launch(chunk):
        log.append(("launch", chunk))
        return f"item{chunk[5:]}"
    P.drive(n, chunk_at, launch, lambda chunk: log.append(("prefetch", chunk)), lambda item: log.append(("finish", item)))
    want = [("launch", "chunk0")] if n else []
    for i in range(n):
        if i + 1 < n:
            want.append(("prefetch", f"chunk{i + 1}"))
        if i >= 1:
            want.append(("finish", f"item{i - 1}"))
        if i + 1 < n:
            want.append(("launch", f"chunk{i + 1}"))
    if n:
        want.append(("finish", f"item{n - 1}"))
    assert log == want and built == list(range(n))
    if n == 3:
        assert [f"{a[0]}{b[-1]}" for a, b in log] == ["l0", "p1", "l1", "p2", "f0", "l2", "f1", "f2"]


def test_staging_dtype_rule(monkeypatch):
    """The whole table of the rule both streams stage by; the thread count is injected, not the machine's."""
    u8, f32, bf16 = torch.uint8, torch.float32, torch.bfloat16
    rule = P.staging_dtype
    for pinned in (False, True):
        for accepts in (False, True):
            for flag in (None, False, True):
                for threads in (2, 7, 8, 16):
                    assert rule(True, pinned, accepts, flag, workers=threads) == u8        # uint8 | any | any | any
        for threads in (2, 7, 8, 16):
            for flag in (None, False):                                                      # any | fp32 | None or False | any
                assert rule(False, pinned, False, flag, workers=threads) == f32
            assert rule(False, pinned, True, False, workers=threads) == f32               # the caller refuses the rounding
        for threads in (8, 16):
            for flag in (None, True):                                                       # any | bf16 | None or True | >= 8
                assert rule(False, pinned, True, flag, workers=threads) == bf16
    for threads in (1, 2, 4, 7):
        assert rule(False, True, True, None, workers=threads) == f32                       # pinned fp32 | bf16 | None | < 8
        assert rule(False, False, True, None, workers=threads) == bf16                     # pageable | bf16 | None | < 8
        assert rule(False, True, True, True, workers=threads) == bf16                      # pinned fp32 | bf16 | True | < 8
        assert rule(False, True, False, True, workers=threads) == bf16                     # bf16_input=True forces it for any model
    # the default thread count is the bf16 staging budget of a rank: 16 // local_world (capped by the CPUs it may run on)
    monkeypatch.delenv("RPG_STAGE_WORKERS", raising=False)
    assert rule(False, True, True, None, local_world=8) == f32                             # 2 threads per rank


G, K, M = 5, 3, 9


class _FakeMapModel:
    """forward_map as ``_FakeModel`` of test_eval_io: y = [the query's own row; fmap.poses[nb]] per graph (the query's row is read
    from its "image", the model gets no targets), rel = y[dst] - y[src] + 0.01 over the FC list, or over a ring of its own."""

    def __init__(self, knn=-1):
        self.knn = knn

    def edges(self, n_graphs):
        n = K + 1
        if self.knn <= 0:
            return torch.cat([fc_edge_index(n) + g * n for g in range(n_graphs)], 1)
        tgt = torch.arange(n_graphs * n).repeat_interleave(2)
        base = (tgt // n) * n
        return torch.stack([base + (tgt - base + torch.tensor([1, 3]).repeat(n_graphs * n)) % n, tgt])

    def forward_map(self, x, nb, fmap):
        table = fmap.poses if fmap.poses is not None else fmap.features
        y = torch.cat([x[:, None, :6], table[nb]], 1).reshape(-1, 6)
        ei = self.edges(x.shape[0])
        return y, y[ei[1]] - y[ei[0]] + 0.01, ei

    def __call__(self, batch):                     # the same model over assembled graphs: evaluate_stream's side
        ei = self.edges(batch.x.shape[0] // (K + 1)) if self.knn > 0 else batch.edge_index
        return None, batch.y[ei[1]] - batch.y[ei[0]] + 0.01, ei


@pytest.fixture(scope="module")
def map_case():
    g = torch.Generator().manual_seed(7)
    table = torch.randn(M, 6, generator=g) * 0.3
    targets = torch.randn(G, 6, generator=g) * 0.3
    queries = torch.cat([targets, torch.zeros(G, 6)], 1)            # the "image" of a query carries its row of y
    nb = torch.randint(0, M, (G, K), generator=g)
    fmap = SimpleNamespace(device=torch.device("cpu"), poses=table, features=table, descriptors=None)
    graphs = [Data(x=torch.zeros(K + 1, 12), edge_index=fc_edge_index(K + 1), y=torch.cat([targets[i:i + 1], table[nb[i]]]))
              for i in range(G)]
    return fmap, queries, nb, targets, graphs


def _same(a: E.EvalResult, b: E.EvalResult):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("pred_poses", "targ_poses", "t_loss", "q_loss"))


@pytest.mark.parametrize("knn", [-1, 1])
def test_relocalize_on_the_cpu_equals_evaluate_stream(map_case, knn):
    """G = 5 queries, K = 3, micro-batches of 2 + 2 + 1: with targets the EvalResult is evaluate_stream's over the assembled
    graphs, bit for bit (the same float64 numpy operations on the same fp32 values) -- FC list and a model-built one."""
    fmap, queries, nb, targets, graphs = map_case
    model, stats = _FakeMapModel(knn), {}
    res = E.relocalize(model, fmap, queries, nb, micro_batch=2, pose_m=(1.0, 2.0, 3.0), pose_s=(2.0, 2.0, 0.5), targets=targets,
                       stats=stats)
    ref = E.evaluate_stream(model, graphs, "cpu", micro_batch=2, pose_m=(1.0, 2.0, 3.0), pose_s=(2.0, 2.0, 0.5))
    assert res.pred_poses.shape == (G, 7) and _same(res, ref)
    assert stats["micro_batches"] == 3 and np.array_equal(stats["neighbours"], nb.numpy()) and np.array_equal(res.neighbours, nb.numpy())
    assert stats["h2d_bytes"] == 0 and stats["staging_workers"] == 0 and stats["postprocess"] == "host"
    # without targets: the [5, 7] predictions alone (the source node's pose does not depend on the query's own row)
    pred = E.relocalize(model, fmap, queries, nb, micro_batch=2, pose_m=(1.0, 2.0, 3.0), pose_s=(2.0, 2.0, 0.5))
    assert isinstance(pred, np.ndarray) and pred.shape == (G, 7) and np.array_equal(pred, ref.pred_poses)


def test_relocalize_on_the_cpu_without_map_poses_returns_the_raw_tensors(map_case):
    fmap, queries, nb, _, _ = map_case
    bare = SimpleNamespace(device=fmap.device, poses=None, features=fmap.features, descriptors=None)
    model, stats = _FakeMapModel(), {}
    ab, rel = E.relocalize(model, bare, queries, nb, micro_batch=2, stats=stats)
    want_ab, want_rel, _ = model.forward_map(queries, nb, bare)          # graphs are independent: one forward over all five
    assert torch.equal(ab, want_ab) and torch.equal(rel, want_rel) and ab.shape == (G * (K + 1), 6)
    assert stats["micro_batches"] == 3 and np.array_equal(stats["neighbours"], nb.numpy())
