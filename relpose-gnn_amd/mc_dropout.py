"""Monte-Carlo sampling of the reference's always-on dropout in front of the pose heads (posenet.py:1073-1086).

The reference applies ``F.dropout`` at evaluation time, so with ``droprate > 0`` every pose it returns is one sample of a random
estimator.  With

    model.mc_dropout = McDropout(samples=16, seed=0)

``forward``, ``forward_map`` (and with them ``evaluate_stream``, ``relocalize`` and the look-ahead client) return the MEAN over
``samples`` masks in place of ``abs_pose`` / ``rel_pose`` -- same signatures, same shapes -- and ``model.mc_dropout.last`` holds the
variances of the most recent call, row for row.  One kernel per head reads every feature row once for all the samples
(``ops.pose_heads_mc``, csrc/mc_heads.hip).

The masks are a pure function of (seed, draw, node ids, column, sample) (csrc/philox.h): they do not depend on how a batch was cut
into stream slots or micro-batches, on the edge order, or on the ``outputs`` mode of ``forward_map``.  ``draw`` counts the forwards
(a one-thread kernel behind every forward adds 1, on the device, so a captured step draws new masks at every replay);
``reset(draw)`` sets it, which makes a run repeatable.  ``node_base`` is the global id of the call's first node: ``relocalize`` and
``evaluate_stream`` set it per micro-batch to the number of nodes that went before and hold ONE draw for all their micro-batches
(the counter moves on by one per call of theirs), so a query's masks do not depend on ``micro_batch``.  Like
``model.frame_transform`` this is a plain attribute: not a module, parameter or buffer.  ``use_AP=False`` is not served
(NotImplementedError), and ``mc_dropout`` on a model with ``droprate == 0`` raises ValueError.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Optional

import torch

# variances of the most recent call: the rows of the abs_pose / rel_pose it returned
McSpread = namedtuple("McSpread", "abs_var rel_var")

_RING = 64      # pinned word pairs a setter call copies from, reused in turn (each behind the event of its previous copy)


class McDropout:
    def __init__(self, samples: int = 16, seed: int = 0):
        samples, seed = int(samples), int(seed)
        if not 1 <= samples <= 1024:
            raise ValueError(f"McDropout: samples must be in 1..1024, got {samples}")
        if not 0 <= seed < 2 ** 64:
            raise ValueError("McDropout: seed must fit 64 bits")
        self.samples, self.seed = samples, seed
        self.last: Optional[McSpread] = None
        self._state: Optional[torch.Tensor] = None      # device int32 [2] = (draw, node_base), read by the kernels
        self._init = [0, 0]                             # what a state tensor made later starts from
        self._pinned: Optional[torch.Tensor] = None
        self._events = [None] * _RING
        self._next = 0

    def state(self, device) -> torch.Tensor:
        """The device state, made on first use on the model's device (and again on another device)."""
        device = torch.device(device)
        if self._state is None or self._state.device != device:
            self._state = torch.tensor(self._init, dtype=torch.int32, device=device)
            self._pinned = torch.zeros((_RING, 2), dtype=torch.int32).pin_memory()
            self._events = [None] * _RING
        return self._state

    @staticmethod
    def _word(v: int) -> int:
        v = int(v) & 0xFFFFFFFF                         # 32 bits, wrapping; stored in an int32 tensor
        return v - (1 << 32) if v >= (1 << 31) else v

    def _send(self, first: int, values) -> None:
        """Words ``first ...`` of the state := values: the host's copy now, the device's by an asynchronous copy from pinned memory
        on the current stream."""
        for j, v in enumerate(values):
            self._init[first + j] = self._word(v)
        if self._state is None:
            return
        i, self._next = self._next, (self._next + 1) % _RING
        if self._events[i] is not None:
            self._events[i].synchronize()               # the copy that last read these pinned words (64 copies ago) has run
        n = len(values)
        self._pinned[i, :n] = torch.tensor(self._init[first:first + n], dtype=torch.int32)
        with torch.cuda.device(self._state.device):
            self._state[first:first + n].copy_(self._pinned[i, :n], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
        self._events[i] = ev

    @property
    def draw(self) -> int:
        """The draw counter as the host has followed it: what ``reset`` set, plus one per forward (or replay) queued since."""
        return self._init[0] & 0xFFFFFFFF

    def reset(self, draw: int = 0) -> None:
        """Set the draw counter (asynchronously, on the current stream): the next forward draws the masks of ``draw``."""
        self._send(0, [draw])

    def place(self, draw: int, node_base: int) -> None:
        """Both words in one copy: what a stream of micro-batches does ahead of every forward -- the draw of the whole stream, held
        while it runs, and the number of nodes that went before -- so that a graph's masks do not depend on ``micro_batch``."""
        if not 0 <= int(node_base) < 2 ** 31:
            raise ValueError(f"McDropout: node_base must be in [0, 2^31), got {node_base}")
        self._send(0, [draw, node_base])

    def advance(self, device) -> None:
        """draw += 1 on the device, by a one-thread kernel on the current stream (rpg_mc_advance): queued once behind every
        forward's heads.  Inside a stream capture only the kernel is recorded; the host's count follows the replays
        (``advanced``)."""
        from . import ops
        ops.mc_advance(self.state(device))
        if not torch.cuda.is_current_stream_capturing():
            self.advanced()

    def advanced(self) -> None:
        """The host's count of a draw the device has been told to make (a replayed step's own advance)."""
        self._init[0] = self._word(self._init[0] + 1)

    @property
    def node_base(self) -> int:
        """The global id of the next call's first node, as last set from the host."""
        return self._init[1] & 0xFFFFFFFF

    @node_base.setter
    def node_base(self, value: int) -> None:
        if not 0 <= int(value) < 2 ** 31:
            raise ValueError(f"McDropout: node_base must be in [0, 2^31), got {value}")
        self._send(1, [value])
