"""``DeferredCounters``: error counters that kernels bump on the device and the host looks at without blocking.

A kernel that meets something it cannot process (an edge with a node id out of range, a graph without its reference edge) counts
it in an int32 word on the device, clamps, and goes on: nothing reads out of bounds and nothing waits.  The counts travel to a
pinned host mirror with an asynchronous copy behind every call, and an event marks the copy.  The owner (``PoseNetX_R2``: 16
counters, ``QueryPose``: one) decides when to look and builds the exception from the host counts.  A non-zero count is reported
ONCE (device and mirror are cleared before the exception is raised), and nothing copies or blocks while the stream is capturing.
Nothing is allocated at construction: the buffers are made on first use, for the device of that call.
"""
from __future__ import annotations

from typing import Callable, Optional

import torch


class DeferredCounters:
    def __init__(self, n: int, error: Callable[[torch.Tensor], Exception]):
        """``n`` int32 counters; ``error(counts)`` turns the host copy of non-zero counters (int32 [n]) into the exception."""
        self.n, self._error = n, error
        self.counters: Optional[torch.Tensor] = None        # device int32 [n]; None until tensor() has been called
        self._host: Optional[torch.Tensor] = None           # pinned mirror
        self._event: Optional[torch.cuda.Event] = None
        self._pending = False

    def tensor(self, dev) -> torch.Tensor:
        """The device counters on ``dev`` (created on first use, and again when the device changes)."""
        if self.counters is None or self.counters.device != dev:
            self.counters = torch.zeros(self.n, dtype=torch.int32, device=dev)
            self._host = torch.zeros(self.n, dtype=torch.int32).pin_memory()
            self._event = torch.cuda.Event()
            self._pending = False
        return self.counters

    def _report(self, counts: torch.Tensor) -> None:
        if not int(counts.sum()):
            return
        exc = self._error(counts)
        self.counters.zero_()                     # (stream-ordered: after every call issued so far)
        self._host.zero_()                        # the mirror too, or a look without waiting would report it again
        self._pending = False
        raise exc

    def publish(self, sync: bool = False) -> None:
        """Enqueue the counters' copy to pinned memory behind the current stream's work; ``sync``: read them back now instead
        (one device synchronisation) and report."""
        if self.counters is None or torch.cuda.is_current_stream_capturing():
            return                                # a captured call is validated by its eager warm-up / a publish behind the replay
        if sync:
            self._report(self.counters.cpu())
            return
        self._host.copy_(self.counters, non_blocking=True)
        self._event.record()
        self._pending = True

    def poll(self, block: bool = False) -> None:
        """Report the counters of the call(s) published so far if their copy has landed (or wait for it when ``block``)."""
        if not self._pending or torch.cuda.is_current_stream_capturing():
            return
        if block:
            self._event.synchronize()
        elif not self._event.query():
            return
        self._pending = False
        self._report(self._host)

    def check(self, wait: bool = True) -> None:
        """``wait``: block until every call published so far has reported.  Otherwise only look at what has already arrived in
        the mirror (the counters accumulate on the device, so a report that is not in yet is seen by the next look)."""
        if wait:
            self.poll(block=True)
        elif self._host is not None and int(self._host.sum()):
            self._event.synchronize()
            self._report(self._host)
