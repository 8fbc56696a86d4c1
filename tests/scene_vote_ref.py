"""Shared by the SceneVote tests: the election stated in integers on the host, descriptors whose elections are known, and the
oracle of the electing retrieval stated on the existing entry points.

The rule (include/relpose_gnn_hip.h, rpg_retrieve_cosine_elect_f32): the voters of a query are the rows at positions 0 .. V-1 of
the order ``ops.retrieve`` defines over the whole atlas without groups; each votes for the scene that owns it; the scene with the
most votes wins, among tied scenes the one of the best-placed voter; the query is then ranked inside that scene exactly as
``scene_ref.oracle`` ranks a query that was told its scene.

``clustered`` margins, measured here on the CPU for seeds 0-19, g = 70, in float64 and in fp32: every query's LEAST similar row
of its own scene is above its MOST similar row of any other scene by at least 0.22 in cosine at d = 64 and by at least 0.70 at
d = 2048 (test_scene_vote_cpu.py asserts both), so all V <= 5 voters (the smallest scene's size) come from the true scene, at V
= 7 at least 5 of 7 do, and no fp32 summation order -- whose effect on a cosine of unit-scale rows is below 1e-5 -- can change
an election."""
import numpy as np

import scene_ref as SR


def vote(voter_rows, scene_first, m=None):
    """(elected scene, its votes) for the voters' rows in order of placement (best first).  Integer logic only.  ``m``: the map's
    row count, to clamp boundaries the way the kernels do (default: the last boundary, i.e. nothing to clamp)."""
    first = np.asarray(scene_first, dtype=np.int64)
    n = first.shape[0] - 1
    m = int(first[-1]) if m is None else int(m)
    c = np.clip(first, 0, m)
    scenes = []
    for row in voter_rows:
        s = int(np.searchsorted(c[:n], int(row), side="right")) - 1
        if s < 0:
            scenes.append(-1)
            continue
        a, b = int(c[s]), max(int(c[s + 1]), int(c[s]))
        scenes.append(s if a <= int(row) < b else -1)
    best = (-1, 0)
    for pos, s in enumerate(scenes):          # in order of placement: a later scene needs strictly more votes to win
        if s >= 0 and scenes.index(s) == pos:
            votes = scenes.count(s)
            if votes > best[1]:
                best = (s, votes)
    return best


def clustered(d, g, seed, sizes=SR.SIZES):
    """(q fp32 [g, d], db fp32 [M, d]): four cluster centres N(0, 1)^d; a database row is its scene's centre + 0.5 noise, query i
    the centre of scene i % len(sizes) + 0.5 noise."""
    rng = np.random.RandomState(seed)
    n = len(sizes)
    centres = rng.standard_normal((n, d))
    db = centres[SR.scene_of_rows(sizes)] + 0.5 * rng.standard_normal((int(np.sum(sizes)), d))
    q = centres[np.arange(g) % n] + 0.5 * rng.standard_normal((g, d))
    return q.astype(np.float32), db.astype(np.float32)


def cosines(q, db, dtype):
    q, db = q.astype(dtype), db.astype(dtype)
    return (q / np.linalg.norm(q, axis=1, keepdims=True)) @ (db / np.linalg.norm(db, axis=1, keepdims=True)).T


def voters_ref(sim, top):
    """numpy: per query the rows at positions 0 .. top-1 by (similarity descending, row ascending)."""
    return np.stack([np.lexsort((np.arange(sim.shape[1]), -sim[i]))[:top] for i in range(sim.shape[0])])


def oracle(dev, q, db, ranks, sizes, top, q_groups=None, db_group=None, gate=None, held=None, first=None):
    """-> (neighbours, sims, gate_info or None, status, scenes int32 [G], scene_info int32 [G, 2]) on the host.  The voters come
    from ``ops.retrieve(ranks=arange(top))`` without groups, ``vote`` runs here, ``scene_ref.oracle`` ranks every query in its
    elected scene.  ``held`` [G] (RPG_ELECT_LOST): query g elects when ``held[g] == -1`` or its prior is not finite and stays in
    ``held[g]`` otherwise.  ``first``: raw boundaries to vote by (clamped to the map) in place of ``sizes``' own; ``sizes`` must
    then be the clamped scenes.  A query whose scene does not exist -- elected -1, or held out of range -- is what the scoped
    entry makes of it: row 0, NaN, one count in status, gate state 1 / 2 with no row inside."""
    import torch
    from relpose_gnn_amd import ops
    g, k = ranks.shape
    m = db.shape[0]
    first = SR.scene_first(sizes) if first is None else np.asarray(first, dtype=np.int64)
    elects = np.ones(g, dtype=bool)
    if held is not None:
        held = np.asarray(held, dtype=np.int64)
        elects = held == -1
        if gate is not None:
            elects |= ~np.isfinite(gate[1].cpu().numpy()).all(axis=1)
    vr = torch.arange(top, dtype=torch.int32, device=dev).repeat(g, 1)
    voters = ops.retrieve(q, db, vr).cpu().numpy()
    scenes = np.empty(g, dtype=np.int64)
    info = np.zeros((g, 2), dtype=np.int32)
    for i in range(g):
        if elects[i]:
            info[i] = vote(voters[i], first, m)
            scenes[i] = info[i, 0]
        else:
            scenes[i], info[i] = held[i], (held[i], 0)
    ok = np.flatnonzero((scenes >= 0) & (scenes < len(sizes)))
    nb = torch.zeros((g, k), dtype=torch.int64)
    sims = torch.full((g, k), float("nan"), dtype=torch.float32)
    ginfo = None
    if gate is not None:
        finite = np.isfinite(gate[1].cpu().numpy()).all(axis=1)
        ginfo = torch.from_numpy(np.stack([np.where(finite, 2, 1), np.zeros(g)], axis=1).astype(np.int32))
    status = g - len(ok)
    if len(ok):
        ix = torch.as_tensor(ok, device=dev)
        sub_gate = None if gate is None else (gate[0], gate[1][ix].contiguous(), *gate[2:])
        n, s, gi, st = SR.oracle(dev, q[ix].contiguous(), db, ranks[ix].contiguous(), sizes, scenes[ok].tolist(),
                                 None if q_groups is None else [q_groups[i] for i in ok], db_group, sub_gate)
        nb[ok], sims[ok] = n, s
        if gi is not None:
            ginfo[ok] = gi
        status += st
    return nb, sims, ginfo, status, torch.from_numpy(scenes.astype(np.int32)), torch.from_numpy(info)
