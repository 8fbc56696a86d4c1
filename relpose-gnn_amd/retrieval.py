"""``RetrievalRule``: which positions of a query's ranked database rows become its graph's database images.

The reference picks a test graph's database frames by image retrieval (dataset_7Scenes_multi.py:238-264, the same tail in
dataset_Cambridge_multi.py:126-136): cosine similarity of the query descriptor against every database descriptor, a ranking, an
exclusion filter, a random half-drop, a strided pick of ``K = seq_len - 1`` rows.  The half-drop mask (:256-257) and the start
(:259-260) are drawn over *positions of the filtered sorted list*, so which positions survive depends on the draw and on the
number of allowed rows only, never on the similarities: they are computed here, on the host, as ``ranks`` int32 [G, K], and the
kernel (``ops.retrieve`` / ``rpg_retrieve_cosine_f32``) does everything that touches descriptors.

    RetrievalRule(k=7)                                    plain top-K (ranks 0..K-1): the default for live relocalisation
    RetrievalRule(k=7, sampling_period=5)                 positions 0, 5, 10, ...
    RetrievalRule.reference(k=7, sampling_period=5, seed=3)
        the reference's draws bit for bit for ``np.random.seed(3)``: per query, in query order, ``random(n_g) < 0.5``, then
        ``randint(0, sampling_period, 1)[0]``, then ``kept[start::sampling_period][:K]`` -- from a ``RandomState(seed)``, the
        stream of the legacy global generator, which runs on from call to call as the global one does.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

K_MAX = 64


def max_rank() -> int:
    """``R_MAX`` of the built library: ranks must stay below it (a compile-time limit of the selection kernel)."""
    from . import _lib as L
    return int(L.lib().rpg_retrieve_max_rank())


class RetrievalRule:
    def __init__(self, k: int = 7, sampling_period: int = 1, drop: float = 0.0, seed: Optional[int] = None,
                 random_start: bool = False):
        if not 1 <= int(k) <= K_MAX:
            raise ValueError(f"RetrievalRule: k must be in [1, {K_MAX}], got {k}")
        if int(sampling_period) < 1:
            raise ValueError(f"RetrievalRule: sampling_period must be >= 1, got {sampling_period}")
        if not 0.0 <= float(drop) < 1.0:
            raise ValueError(f"RetrievalRule: drop must be in [0, 1), got {drop}")
        self.k, self.sampling_period, self.drop = int(k), int(sampling_period), float(drop)
        self.random_start, self.seed = bool(random_start), seed
        self._rng = np.random.RandomState(seed) if self.random else None
        self._dev_ranks: Dict[tuple, torch.Tensor] = {}

    @classmethod
    def reference(cls, k: int = 7, sampling_period: int = 5, seed: Optional[int] = None) -> "RetrievalRule":
        """The reference's rule (dataset_7Scenes_multi.py:255-264): half of the positions dropped, a random start below the
        sampling period; ``seed`` as ``np.random.seed(seed)``."""
        return cls(k=k, sampling_period=sampling_period, drop=0.5, seed=seed, random_start=True)

    @property
    def random(self) -> bool:
        return self.drop > 0.0 or self.random_start

    def __repr__(self) -> str:
        return (f"RetrievalRule(k={self.k}, sampling_period={self.sampling_period}, drop={self.drop}, seed={self.seed!r}, "
                f"random_start={self.random_start})")

    def ranks(self, n_allowed: Sequence[int], limit: Optional[int] = None) -> np.ndarray:
        """int32 [G, K]: per query the positions, strictly ascending, of its picks in the order (similarity descending, row
        ascending) of its ``n_allowed[g]`` allowed rows.  Raises ValueError, naming the query, where the reference would return
        fewer than K rows, and where a position reaches ``limit`` (default: the kernel's ``R_MAX``)."""
        n_allowed = np.asarray(n_allowed, dtype=np.int64).reshape(-1)
        limit = max_rank() if limit is None else int(limit)
        out = np.empty((n_allowed.shape[0], self.k), dtype=np.int32)
        sp = self.sampling_period
        for g, n in enumerate(n_allowed):
            n = int(n)
            if n < 0:
                raise ValueError(f"RetrievalRule.ranks: query {g} has a negative number of allowed rows ({n})")
            if self.drop > 0.0:                                                   # :256-257 (the reference: < 0.5)
                kept = np.flatnonzero(self._rng.random_sample(n) < 1.0 - self.drop)
            else:
                kept = None
            start = int(self._rng.randint(0, sp, 1)[0]) if self.random_start else 0   # :259
            if kept is None:
                pick = np.arange(start, min(n, start + sp * self.k), sp)           # :260, :264 without the mask
            else:
                pick = kept[start::sp][:self.k]                                    # :260, :264
            if pick.shape[0] < self.k:
                raise ValueError(f"retrieval: query {g} gets {pick.shape[0]} database rows, the rule needs {self.k} "
                                 f"({n} allowed rows, sampling_period {sp}, drop {self.drop})")
            if int(pick[-1]) >= limit:
                raise ValueError(f"retrieval: query {g} needs the row at position {int(pick[-1])} of its ranking; the kernel "
                                 f"serves positions below R_MAX = {limit}")
            out[g] = pick
        return out

    def device_ranks(self, n_allowed: Sequence[int], device) -> torch.Tensor:
        """``ranks`` as an int32 tensor on ``device``, sent from pinned memory on the current stream without blocking.  A rule
        without random draws gives the same ranks for every call of the same size: those are kept on the device."""
        key = None
        if not self.random:
            n_allowed = np.asarray(n_allowed, dtype=np.int64).reshape(-1)
            # the ranks depend on n_allowed only through the error checks, which the smallest count decides
            need = (self.k - 1) * self.sampling_period + 1
            key = (n_allowed.shape[0], bool(n_allowed.size) and int(n_allowed.min()) >= need and need <= max_rank(), str(device))
            if key[1] and key in self._dev_ranks:
                return self._dev_ranks[key]
        r = torch.from_numpy(self.ranks(n_allowed)).pin_memory().to(device, non_blocking=True)
        if key is not None and key[1]:
            if len(self._dev_ranks) >= 16:
                self._dev_ranks.clear()
            self._dev_ranks[key] = r
        return r


class PoseGate:
    """Restricts retrieval to the map rows near a prior pose (``FeatureMap.retrieve(prior=, gate=)``, ``forward_map(prior=,
    gate=)``, ``tracking.Tracker``): a row is inside when its translation lies within ``radius`` of the prior's and -- with
    ``max_deg`` -- its rotation within ``max_deg`` degrees.  ``radius`` is in the unit of the UN-normalised translation (``t *
    pose_s + pose_m``, what ``relocalize`` returns), finite and >= 0; ``max_deg`` in [0, 360] or None for no rotation test
    (ValueError otherwise).  ``pose_m`` / ``pose_s``: the translation mean / std the map's poses are normalised by, as the pose
    rule takes them.  ``r2`` and ``cos_half`` (cos of ``max_deg / 2``: the kernel compares ``|<q1, q2>|`` with it) are computed
    once, here, as Python floats -- the numbers the kernel gets."""

    def __init__(self, radius: float, max_deg: Optional[float] = None, pose_m=(0.0, 0.0, 0.0), pose_s=(1.0, 1.0, 1.0)):
        radius = float(radius)
        if not np.isfinite(radius) or radius < 0.0:
            raise ValueError(f"PoseGate: radius must be finite and >= 0, got {radius}")
        if max_deg is not None:
            max_deg = float(max_deg)
            if not 0.0 <= max_deg <= 360.0:                   # (a NaN fails both comparisons)
                raise ValueError(f"PoseGate: max_deg must be in [0, 360] (or None: no rotation gate), got {max_deg}")
        self.pose_m = tuple(float(v) for v in np.asarray(pose_m, dtype=np.float64).reshape(3))
        self.pose_s = tuple(float(v) for v in np.asarray(pose_s, dtype=np.float64).reshape(3))
        self.radius, self.max_deg = radius, max_deg
        self.r2 = radius * radius
        self.cos_half = 0.0 if max_deg is None else float(np.cos(np.deg2rad(max_deg / 2.0)))

    @property
    def rot(self) -> bool:
        return self.max_deg is not None

    @property
    def key(self) -> tuple:
        """What a captured step is keyed by: two gates with the same key are the same gate."""
        return (self.r2, self.cos_half, self.rot, self.pose_m, self.pose_s)

    def __repr__(self) -> str:
        return f"PoseGate(radius={self.radius}, max_deg={self.max_deg}, pose_m={self.pose_m}, pose_s={self.pose_s})"


ELECT_ALL, ELECT_LOST = 1, 2                                  # RPG_ELECT_ALL, RPG_ELECT_LOST


class SceneVote:
    """Goes where ``scenes=`` goes on a ``featmap.SceneAtlas``, in place of the indices: the queries are not told their scene,
    they elect it on the GPU (``ops.retrieve_elect`` / rpg_retrieve_cosine_elect_f32).  The ``top`` most similar rows of the
    WHOLE atlas (no group filter, no gate) vote for the scene that owns them; the scene with the most votes -- among tied ones
    the scene of the best-placed voter -- is the one the query is then ranked in, exactly as if it had been given.  ``top`` in
    [1, 64] (ValueError otherwise; above the atlas's row count is refused where the atlas is known).
    ``lost_only``: only the queries whose static scene is -1, or whose prior is not finite, elect; the others stay in the scene
    they hold -- for a step whose scenes live on the device between calls (``GraphedForwardMap`` with a gate,
    ``tracking.Tracker``, which always works this way); anywhere else it is a ValueError."""

    def __init__(self, top: int = 16, lost_only: bool = False):
        if isinstance(top, bool) or int(top) != top or not 1 <= int(top) <= K_MAX:
            raise ValueError(f"SceneVote: top must be an integer in [1, {K_MAX}], got {top!r}")
        if not isinstance(lost_only, bool):
            raise ValueError(f"SceneVote: lost_only must be a bool, got {type(lost_only).__name__}")
        self.top, self.lost_only = int(top), lost_only

    @property
    def mode(self) -> int:
        return ELECT_LOST if self.lost_only else ELECT_ALL

    @property
    def key(self) -> tuple:
        """What a captured step is keyed by: two votes with the same key are the same vote."""
        return ("vote", self.top, self.lost_only)

    def __repr__(self) -> str:
        return f"SceneVote(top={self.top}, lost_only={self.lost_only})"
