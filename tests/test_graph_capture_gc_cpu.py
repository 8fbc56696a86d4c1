"""graphed._capturing without a GPU: dead reference cycles are collected AHEAD of a capture and Python's cycle collector is off
while it lasts.  A cycle may hold captured graphs (a model and the steps in its ``_map_captures``), and on ROCm the destructor of
a ``torch.cuda.CUDAGraph`` synchronises the device, which must not happen while a stream is capturing."""
import contextlib
import gc
import weakref

import pytest
import torch


class _Node:
    pass


def _dead_cycle():
    a, b = _Node(), _Node()
    a.other, b.other = b, a
    return weakref.ref(a)


@pytest.mark.parametrize("enabled_before", [True, False])
def test_collector_is_held_off_during_a_capture(monkeypatch, enabled_before):
    from relpose_gnn_amd import graphed
    seen = {}

    @contextlib.contextmanager
    def fake_graph(graph, stream=None):
        seen["entered"] = (graph, stream, gc.isenabled(), ref() is None)
        yield
        seen["left_enabled"] = gc.isenabled()
    monkeypatch.setattr(torch.cuda, "graph", fake_graph)
    was = gc.isenabled()
    try:
        gc.disable()                                          # so that only _capturing's own collection can clear the cycle
        ref = _dead_cycle()
        assert ref() is not None
        if enabled_before:
            gc.enable()
        with graphed._capturing("g", "s"):
            assert not gc.isenabled()
            inside = _dead_cycle()                            # garbage made during the capture stays until it is over
            for _ in range(5000):
                _Node()
            assert inside() is not None
        assert seen["entered"] == ("g", "s", False, True)    # collected before torch.cuda.graph was entered, collector off
        assert seen["left_enabled"] is False and gc.isenabled() is enabled_before
        # an exception inside the capture restores the collector, too
        with pytest.raises(KeyError):
            with graphed._capturing("g", "s"):
                raise KeyError("x")
        assert gc.isenabled() is enabled_before
    finally:
        gc.enable() if was else gc.disable()
