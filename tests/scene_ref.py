"""Shared by the SceneAtlas tests: the small atlas every retrieval case uses, host-side counts, and the oracle of scene-scoped
retrieval stated on the existing entry points.

The oracle identity (include/relpose_gnn_hip.h, rpg_retrieve_cosine_scoped_f32): query g of scene s and group c gets what the
unscoped entry gives on the same q, db, m, d and ranks when every row outside s is excluded as a row of group c is.  So the
oracle is ``ops.retrieve`` / ``ops.retrieve_gated`` on the whole atlas, once per distinct (scene, group) pair among the queries,
with an emulated ``db_group`` that is 1 where a row is outside the scene or in the query's group and 0 elsewhere, the pair's
queries carrying ``q_group`` 1."""
import numpy as np

SIZES = (37, 91, 16, 5)            # M = 149: every boundary falls inside a 16-row dot tile; the last scene holds exactly 5 rows
RANKS = (0, 2, 4)                  # k = 3, so the 5-row scene is exactly enough


def scene_first(sizes=SIZES):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def scene_of_rows(sizes=SIZES):
    return np.repeat(np.arange(len(sizes), dtype=np.int64), sizes)


def descriptors(d, g, seed, sizes=SIZES):
    """(q fp32 [g, d], db fp32 [M, d]) of unit-variance normals: nothing special about any row."""
    rng = np.random.RandomState(seed)
    m = int(np.sum(sizes))
    return rng.standard_normal((g, d)).astype(np.float32), rng.standard_normal((m, d)).astype(np.float32)


def emulated_groups(sizes, scene, q_group, db_group):
    """int64 [M]: 1 where the row is outside ``scene`` or in the query's group, 0 elsewhere."""
    out = (scene_of_rows(sizes) != scene).astype(np.int64)
    if db_group is not None and q_group != -1:
        out |= (np.asarray(db_group) == q_group).astype(np.int64)
    return out


def n_allowed_ref(sizes, scenes, q_groups=None, db_group=None):
    """numpy count: per query the rows of its scene that are not of its group."""
    sor = scene_of_rows(sizes)
    out = np.empty(len(scenes), dtype=np.int64)
    for i, s in enumerate(scenes):
        keep = sor == s
        if q_groups is not None and db_group is not None and q_groups[i] != -1:
            keep &= np.asarray(db_group) != q_groups[i]
        out[i] = int(keep.sum())
    return out


def pairs_of(scenes, q_groups=None):
    """{(scene, group): indices of its queries}, group -1 without groups."""
    out = {}
    for i, s in enumerate(scenes):
        out.setdefault((int(s), -1 if q_groups is None else int(q_groups[i])), []).append(i)
    return out


def oracle(dev, q, db, ranks, sizes, scenes, q_groups=None, db_group=None, gate=None):
    """-> (neighbours int64 [G, K], sims fp32 [G, K], gate_info int32 [G, 2] or None, status int) on the host, through
    ``ops.retrieve`` / ``ops.retrieve_gated`` as the module docstring says.  ``q``, ``db``, ``ranks`` device tensors; ``gate`` =
    (db_gate, prior, r2, cos_half, rot) with device tensors."""
    import torch
    from relpose_gnn_amd import ops
    g, k = ranks.shape
    nb = torch.zeros((g, k), dtype=torch.int64)
    sims = torch.zeros((g, k), dtype=torch.float32)
    info = None if gate is None else torch.zeros((g, 2), dtype=torch.int32)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    for (scene, grp), idx in pairs_of(scenes, q_groups).items():
        ix = torch.as_tensor(idx, device=dev)
        dg = torch.from_numpy(emulated_groups(sizes, scene, grp, db_group)).to(dev)
        qg = torch.ones(len(idx), dtype=torch.int64, device=dev)
        if gate is None:
            n, s = ops.retrieve(q[ix], db, ranks[ix].contiguous(), q_group=qg, db_group=dg, return_sims=True, status=status)
        else:
            dbg, prior, r2, ch, rot = gate
            n, s, gi = ops.retrieve_gated(q[ix], db, ranks[ix].contiguous(), dbg, prior[ix].contiguous(), r2, ch, rot, q_group=qg,
                                          db_group=dg, return_sims=True, status=status)
            info[idx] = gi.cpu()
        nb[idx], sims[idx] = n.cpu(), s.cpu()
    return nb, sims, info, int(status.item())
