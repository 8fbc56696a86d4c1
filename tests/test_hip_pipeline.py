"""The micro-batch pipeline on the GPU (relpose_gnn_amd.pipeline) at the smallest shapes at which state shared between its
clients can go wrong: ragged tails, both staging regimes of the bf16 encoder, and evaluate_stream / relocalize / lookahead
taking turns on one model."""
import os

import numpy as np
import pytest
import torch

from test_hip_featmap import _nb, _small

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def test_relocalize_bf16_pinned_queries_in_both_staging_regimes(dev):
    """bf16 encoder, 10 pinned fp32 queries, K = 3, micro-batches of 4 + 4 + 2.  A rank with few staging threads
    (RPG_STAGE_WORKERS = 2) sends the queries as they are: 4 bytes per element, all of them direct.  A rank with >= 8 rounds them
    on the host: 2 bytes per element, all of them staged.  The poses are the same bits, and those of device-resident queries."""
    import relpose_gnn_amd.synth as S
    from relpose_gnn_amd.evaluate import relocalize
    from relpose_gnn_amd.featmap import FeatureMap
    m, _ = _small(dev)
    m.encoder_dtype = "bf16"
    assert m.accepts_bf16_input
    mimgs, queries = S.synth_images(12, 32, 40, seed=71), S.synth_images(10, 32, 40, seed=72)
    fmap = FeatureMap.build(m, mimgs, poses=torch.randn(12, 6, generator=torch.Generator().manual_seed(8)) * 0.3)
    nb, q = _nb(10, 3, 12, 5), queries.pin_memory()
    resident = relocalize(m, fmap, queries.to(dev), nb, micro_batch=4)
    assert resident.shape == (10, 7) and np.isfinite(resident).all()

    def run(workers):
        st, old_env = {}, os.environ.get("RPG_STAGE_WORKERS")
        os.environ["RPG_STAGE_WORKERS"] = workers
        try:
            return relocalize(m, fmap, q, nb, micro_batch=4, stats=st), st
        finally:
            if old_env is None:
                del os.environ["RPG_STAGE_WORKERS"]
            else:
                os.environ["RPG_STAGE_WORKERS"] = old_env
    few, st = run("2")
    assert np.array_equal(few, resident)
    assert (st["h2d_bytes"], st["direct_bytes"], st["staged_bytes"]) == (4 * q.numel(), 4 * q.numel(), 0), st
    assert st["micro_batches"] == 3 and st["staging_workers"] == 2
    if len(os.sched_getaffinity(0)) < 8:
        pytest.skip("fewer than 8 CPUs for this process: the rounding regime (>= 8 staging threads) cannot occur; the direct one passed")
    many, st = run("16")
    assert np.array_equal(many, few)
    assert (st["h2d_bytes"], st["direct_bytes"], st["staged_bytes"]) == (2 * q.numel(), 0, 2 * q.numel()), st


def test_interleaved_clients_of_one_model(dev):
    """evaluate_stream, relocalize, a lookahead loop and evaluate_stream again in one process on ONE model, each with a ragged
    tail (10 graphs or queries, micro-batches of 4): every result equals, bit for bit, the same call made first on a fresh
    model -- no buffer, event or prefetch handle leaks from one client into the next."""
    import relpose_gnn_amd.synth as S
    from relpose_gnn_amd.evaluate import evaluate_stream, relocalize
    from relpose_gnn_amd.featmap import FeatureMap
    from relpose_gnn_amd.graph import Batch, Data, fc_edge_index
    from relpose_gnn_amd.lookahead import lookahead
    imgs = S.synth_images(80, 32, 40, seed=75).reshape(10, 8, -1)
    gen = torch.Generator().manual_seed(9)
    ys, targets = torch.randn(10, 8, 6, generator=gen) * 0.3, torch.randn(10, 6, generator=gen) * 0.3
    graphs = [Data(x=imgs[i], edge_index=fc_edge_index(8), y=ys[i], edge_attr=None) for i in range(10)]
    mimgs, queries, nb = imgs[:2].reshape(16, -1), imgs[:, 0].contiguous().pin_memory(), _nb(10, 3, 16, 4)

    def stream(m):
        r = evaluate_stream(m, graphs, dev, micro_batch=4)
        return [r.pred_poses, r.targ_poses, r.t_loss, r.q_loss]

    def reloc(m):
        fmap = FeatureMap.build(m, mimgs, poses=ys[:2].reshape(16, 6))
        r = relocalize(m, fmap, queries, nb, micro_batch=4, targets=targets)
        return [r.pred_poses, r.targ_poses, r.t_loss, r.q_loss]

    def loop(m):
        loader, wrapped = lookahead([Batch.from_data_list([g]) for g in graphs], m, dev, micro_batch=4)
        out = []
        for data in loader:
            out += [t.cpu().numpy().copy() for t in wrapped(data.to(dev))]
        assert wrapped.forwards == 3 and wrapped.direct_calls == 0
        return out

    shared, _ = _small(dev)
    first = None
    for k, client in enumerate((stream, reloc, loop, stream)):
        fresh, _ = _small(dev)
        want, got = client(fresh), client(shared)
        assert len(want) == len(got) and all(np.array_equal(a, b) for a, b in zip(want, got)), client.__name__
        if k == 0:
            first = got
    assert all(np.array_equal(a, b) for a, b in zip(first, got))              # the second evaluate_stream equals the first
