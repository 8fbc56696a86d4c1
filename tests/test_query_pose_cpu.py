"""Host side of the device pose rule (ops.query_pose, query_pose.QueryPose, postprocess= of the two streams): every argument
error is raised before the library is touched, so none of this needs a GPU or a built library."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def no_library(monkeypatch):
    """Any use of the shared library fails the test."""
    from relpose_gnn_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", refuse)


def _targets_args(g=3, n_per=4):
    e = g * n_per * (n_per - 1)
    return dict(rel_pose=torch.zeros(e, 6), edge_index=torch.zeros((2, e), dtype=torch.int64),
                node_first=torch.arange(g + 1) * n_per, node_targets=torch.zeros(g * n_per, 6),
                edge_first=torch.arange(g + 1) * n_per * (n_per - 1))


def _map_args(g=3, k=3, m=10):
    e = g * (k + 1) * k
    return dict(rel_pose=torch.zeros(e, 6), edge_index=torch.zeros((2, e), dtype=torch.int64), map_poses=torch.zeros(m, 6),
                neighbours=torch.zeros((g, k), dtype=torch.int64), query_targets=torch.zeros(g, 6))


@pytest.mark.parametrize("form", ["targets", "map"])
def test_ops_query_pose_refuses_bad_arguments(no_library, form):
    from relpose_gnn_amd import ops
    good = _targets_args() if form == "targets" else _map_args()

    def call(**change):
        kw = dict(good)
        kw.update(change)
        rel, ei = kw.pop("rel_pose"), kw.pop("edge_index")
        return ops.query_pose(rel, ei, **kw)

    # wrong type / dtype: TypeError
    with pytest.raises(TypeError):
        call(rel_pose=good["rel_pose"].double())
    with pytest.raises(TypeError):
        call(edge_index=good["edge_index"].int())
    with pytest.raises(TypeError):
        call(rel_pose=good["rel_pose"].numpy())
    with pytest.raises(TypeError):
        call(ref_node=1.0)
    with pytest.raises(TypeError):
        call(status=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(TypeError):
        call(out=torch.zeros((3, 16), dtype=torch.float32))
    if form == "targets":
        with pytest.raises(TypeError):
            call(node_first=good["node_first"].int())
        with pytest.raises(TypeError):
            call(node_targets=good["node_targets"].double())
        with pytest.raises(TypeError):
            call(edge_first=good["edge_first"].float())
    else:
        with pytest.raises(TypeError):
            call(neighbours=good["neighbours"].int())
        with pytest.raises(TypeError):
            call(map_poses=good["map_poses"].half())
        with pytest.raises(TypeError):
            call(query_targets=good["query_targets"].double())
    # shapes that do not match G / N / E, bad scalars: ValueError
    with pytest.raises(ValueError):
        call(rel_pose=torch.zeros(good["rel_pose"].shape[0], 7))
    with pytest.raises(ValueError):
        call(edge_index=good["edge_index"][:, :-1])
    with pytest.raises(ValueError):
        call(rel_pose=torch.zeros(0, 6), edge_index=torch.zeros((2, 0), dtype=torch.int64))
    with pytest.raises(ValueError):
        call(ref_node=-1)
    with pytest.raises(ValueError):
        call(pose_m=(0.0, 1.0))
    with pytest.raises(ValueError):
        call(out=torch.zeros((2, 16), dtype=torch.float64))
    if form == "targets":
        with pytest.raises(ValueError):
            call(edge_first=good["edge_first"][:-1])
        with pytest.raises(ValueError):
            call(node_targets=torch.zeros(12, 5))
        with pytest.raises(ValueError):
            call(node_first=torch.zeros(1, dtype=torch.int64))              # no graphs
        with pytest.raises(ValueError):
            call(node_first=None)
        with pytest.raises(ValueError):
            call(neighbours=torch.zeros((3, 3), dtype=torch.int64))        # both forms at once
        with pytest.raises(ValueError):
            call(map_poses=torch.zeros(10, 6))
    else:
        with pytest.raises(ValueError):
            call(query_targets=torch.zeros(2, 6))
        with pytest.raises(ValueError):
            call(neighbours=torch.zeros(3, dtype=torch.int64))
        with pytest.raises(ValueError):
            call(neighbours=torch.zeros((3, 0), dtype=torch.int64))
        with pytest.raises(ValueError):
            call(map_poses=torch.zeros(10, 7))
        with pytest.raises(ValueError):
            call(map_poses=None)                                           # neither form
        with pytest.raises(ValueError):
            call(node_first=torch.arange(4))
    # everything right, but on the host: wrong device
    with pytest.raises(ValueError, match="GPU"):
        call()


def test_query_pose_object_refuses_bad_arguments(no_library):
    from relpose_gnn_amd.query_pose import QueryPose
    with pytest.raises(ValueError):
        QueryPose(pose_m=(1.0, 2.0))
    with pytest.raises(TypeError):
        QueryPose(ref_node="0")
    with pytest.raises(ValueError):
        QueryPose(ref_node=-2)
    qp = QueryPose((1.0, 2.0, 3.0), np.array([1.0, 1.0, 2.0]), ref_node=1)
    assert qp.pose_m == (1.0, 2.0, 3.0) and qp.pose_s == (1.0, 1.0, 2.0) and qp.ref_node == 1
    qp.check()                                                             # nothing issued: nothing to report, nothing to wait for
    qp.check(wait=False)
    t = _targets_args()
    with pytest.raises(ValueError, match="GPU"):
        qp.from_targets(t["rel_pose"], t["edge_index"], t["node_first"], t["node_targets"], edge_first=t["edge_first"])
    with pytest.raises(TypeError):
        qp.from_targets(t["rel_pose"], t["edge_index"], t["node_first"].float(), t["node_targets"])
    with pytest.raises(ValueError):
        qp.from_targets(t["rel_pose"], t["edge_index"], t["node_first"], t["node_targets"][:, :5])

    class Map:
        poses = None
    m = _map_args()
    with pytest.raises(ValueError, match="no poses"):
        qp.from_map(m["rel_pose"], m["edge_index"], Map(), m["neighbours"])
    Map.poses = m["map_poses"]
    with pytest.raises(ValueError, match="GPU"):
        qp.from_map(m["rel_pose"], m["edge_index"], Map(), m["neighbours"], query_targets=m["query_targets"])
    with pytest.raises(ValueError):
        qp.from_map(m["rel_pose"], m["edge_index"], Map(), m["neighbours"], query_targets=torch.zeros(4, 6))


def test_postprocess_takes_two_values(no_library):
    from relpose_gnn_amd.evaluate import evaluate_stream, relocalize

    class Map:
        device = torch.device("cpu")
        poses = None
    for bad in ("gpu", "Device", None, True):
        with pytest.raises(ValueError, match="postprocess"):
            evaluate_stream(None, [], "cpu", postprocess=bad)
        with pytest.raises(ValueError, match="postprocess"):
            relocalize(None, Map(), torch.zeros(2, 4), torch.zeros((2, 1), dtype=torch.int64), postprocess=bad)
    # "device" needs the GPU: refused for a host stream before anything runs
    with pytest.raises(ValueError, match="postprocess"):
        evaluate_stream(None, [], "cpu", postprocess="device")
    with pytest.raises(ValueError, match="postprocess"):
        relocalize(None, Map(), torch.zeros(2, 4), torch.zeros((2, 1), dtype=torch.int64), postprocess="device")
    # "host" is the default and an empty stream still evaluates to an empty result
    res = evaluate_stream(None, [], "cpu", postprocess="host")
    assert res.pred_poses.shape == (0, 7)


def test_entry_point_is_declared_bound_and_built():
    from relpose_gnn_amd import _lib, build
    with open(os.path.join(ROOT, "include", "relpose_gnn_hip.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+rpg_query_pose_f64\s*\(", header)
    assert "rpg_query_pose_f64" in _lib.SYMBOLS
    assert "query_pose.hip" in build.SOURCES
    with open(os.path.join(ROOT, "relpose-gnn_amd", "csrc", "query_pose.hip")) as f:
        src = f.read()
    assert re.search(r'extern\s+"C"\s+int\s+rpg_query_pose_f64\s*\(', src)
    # the binding passes as many arguments as the declaration names
    decl = re.search(r"\bint\s+rpg_query_pose_f64\s*\(([^)]*)\)", header).group(1)
    n_args = len([a for a in decl.split(",") if a.strip()])

    class Fake:
        def __getattr__(self, name):
            holder = type("F", (), {})()
            setattr(self, name, holder)
            return holder
    fake = Fake()
    _lib._declare(fake)
    assert len(fake.rpg_query_pose_f64.argtypes) == n_args == 24
