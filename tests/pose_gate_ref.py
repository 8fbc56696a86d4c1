"""Reference statements for pose-gated retrieval and the tracking loop's update rule (csrc/pose_gate.h, csrc/retrieve.hip,
csrc/track.hip), none of which runs project code: numpy float64, every product and sum rounded on its own, in the order the
header states.

    gate_mask(db_gate, prior, r2, cos_half)     bool [M]: the rows inside the gate of ONE finite prior
    gate_decision(mask, allowed, need)          (state, rows_inside, the bool [M] row set that is ranked)
    gated_rows(...)                             the two for every query of a call
    track_update_ref(...)                       the accept rule of one frame, for S cameras
"""
import numpy as np

INT32_MAX = 2 ** 31 - 1


def finite7(p):
    """Whether all seven of ``p`` [..., 7] are finite."""
    return np.all(np.isfinite(np.asarray(p, dtype=np.float64)), axis=-1)


def gate_mask(db_gate, prior, r2, cos_half=None):
    """bool [M]: row r of ``db_gate`` float64 [M, 7] is inside the gate around ``prior`` [7] (finite): all its entries finite,
    ``((dx*dx + dy*dy) + dz*dz) <= r2`` and, with ``cos_half`` (None: no rotation gate), ``|((w1*w2 + x1*x2) + y1*y2) + z1*z2| >=
    cos_half``."""
    db = np.asarray(db_gate, dtype=np.float64).reshape(-1, 7)
    p = np.asarray(prior, dtype=np.float64).reshape(7)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = db[:, 0] - p[0], db[:, 1] - p[1], db[:, 2] - p[2]
        d2 = (dx * dx + dy * dy) + dz * dz
        inside = finite7(db) & (d2 <= np.float64(r2))
        if cos_half is not None:
            dot = ((db[:, 3] * p[3] + db[:, 4] * p[4]) + db[:, 5] * p[5]) + db[:, 6] * p[6]
            inside &= np.abs(dot) >= np.float64(cos_half)
    return inside


def gate_decision(mask, allowed, need):
    """``mask``: ``gate_mask`` of the query, or None when its prior is not finite; ``allowed`` bool [M]: the group filter;
    ``need``: the query's largest rank + 1.  -> (state, rows_inside, the rows that are ranked): state 1 without a prior (rows
    inside 0), 0 = gated when the allowed rows inside cover ``need``, 2 = fallback to the group filter otherwise."""
    allowed = np.asarray(allowed, dtype=bool)
    if mask is None:
        return 1, 0, allowed.copy()
    both = np.asarray(mask, dtype=bool) & allowed
    inside = int(both.sum())
    return (0, inside, both) if inside >= int(need) else (2, inside, allowed.copy())


def gated_rows(db_gate, priors, r2, cos_half, ranks, q_group=None, db_group=None):
    """Per query of a call: -> (gate_info int32 [G, 2], used bool [G, M])."""
    db = np.asarray(db_gate, dtype=np.float64).reshape(-1, 7)
    priors = np.asarray(priors, dtype=np.float64).reshape(-1, 7)
    ranks = np.asarray(ranks).reshape(priors.shape[0], -1)
    info = np.zeros((priors.shape[0], 2), dtype=np.int32)
    used = np.zeros((priors.shape[0], db.shape[0]), dtype=bool)
    for g in range(priors.shape[0]):
        allowed = np.ones(db.shape[0], dtype=bool)
        if q_group is not None and int(q_group[g]) != -1:
            allowed = np.asarray(db_group) != int(q_group[g])
        mask = gate_mask(db, priors[g], r2, cos_half) if finite7(priors[g]) else None
        info[g, 0], info[g, 1], used[g] = gate_decision(mask, allowed, int(ranks[g].max()) + 1)
    return info, used


def track_update_ref(poses, inliers, used, prior, lost, min_inliers, min_ratio, max_lost):
    """One frame of S cameras: ``poses`` float64 [S, 7], ``inliers`` / ``used`` int [S], the state ``prior`` float64 [S, 7] and
    ``lost`` int [S] -> (prior, lost, accepted), new arrays.  Accepted: the pose is finite, ``inliers >= min_inliers`` and
    ``float(inliers) >= min_ratio * float(used)``; the pose then is the prior and ``lost`` 0.  Otherwise ``lost`` counts one more
    (saturating at INT32_MAX) and past ``max_lost`` the prior is NaN."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 7)
    prior = np.array(prior, dtype=np.float64).reshape(-1, 7)
    lost = np.array(lost, dtype=np.int64).reshape(-1)
    accepted = np.zeros(poses.shape[0], dtype=np.int32)
    for s in range(poses.shape[0]):
        i, u = int(inliers[s]), int(used[s])
        if bool(finite7(poses[s])) and i >= int(min_inliers) and np.float64(i) >= np.float64(min_ratio) * np.float64(u):
            prior[s], lost[s], accepted[s] = poses[s], 0, 1
        else:
            lost[s] = min(int(lost[s]) + 1, INT32_MAX)
            if lost[s] > int(max_lost):
                prior[s] = np.nan
    return prior, lost.astype(np.int32), accepted


def quat_about_z(deg):
    """Unit quaternion (w, x, y, z) of a rotation by ``deg`` degrees about z."""
    h = np.deg2rad(np.float64(deg) / 2.0)
    return np.array([np.cos(h), 0.0, 0.0, np.sin(h)], dtype=np.float64)


def bits(x) -> str:
    """The 16 hex digits of a double's bits (what tests/pose_gate_check.cpp reads and prints)."""
    return format(int(np.asarray(x, dtype=np.float64).reshape(1).view(np.uint64)[0]), "016x")
