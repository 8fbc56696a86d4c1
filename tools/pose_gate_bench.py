#!/usr/bin/env python3
"""Pose-gated retrieval and the tracking loop on the GPU (opt-in; bench.py does not call it).  One JSON document, written to
``--out`` (default profiles/pose_gate_bench.json), three legs:

  * ``ungated_vs_parent`` (only with ``--parent-lib``, a build of the PARENT commit's library): rpg_retrieve_cosine_f32 of this
    build against the parent build's, called the same way (ctypes, cached inverse norms, a caller's workspace, the same buffers),
    at M in {1000, 100000} rows, Dd = 2048, G in {1, 64} queries, plain top-7.  The ungated path gained only null-pointer
    branches, so the expectation is "within the run-to-run spread"; both numbers and the spread are written down, and the two
    builds' neighbours and similarities are compared bit for bit.
  * ``gated_vs_ungated``: ops.retrieve_gated (every query with a finite prior whose gate holds enough rows: the counting pass
    runs for all of them) against ops.retrieve at the same sizes -- the cost of the counting pass.
  * ``tracker``: ``Tracker.step`` at one stream, captured and eager, against the single-query ``GraphedForwardMap`` replay with the
    same retrieval rule and pose rule and NO gate -- the parent's serving call, which this build issues with the same launches
    -- in frames/s: the cost of the gate plus the update launch.  ResNet-34, 224 x 224, fp32, D = 2048, a map of 4000 rows, K = 7,
    ``outputs="query"``, consensus pose rule.

Timing: every figure is the median of ``--runs`` windows of at least ``--window`` seconds of back-to-back calls on one stream,
ended by a device synchronise; the two sides of a comparison alternate window by window, and ``spread`` is (max - min) / median
over a side's windows.  The device's clock state (rocm-smi's current sclk / mclk, read only) is noted before and after.

    usage: tools/pose_gate_bench.py [--parent-lib PATH] [--runs 3] [--window 0.4]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import relpose_gnn_amd.synth as S  # noqa: E402
from relpose_gnn_amd import _lib, ops  # noqa: E402
from relpose_gnn_amd.featmap import FeatureMap  # noqa: E402
from relpose_gnn_amd.graphed import GraphedForwardMap  # noqa: E402
from relpose_gnn_amd.posenet import PoseNetX_R2  # noqa: E402
from relpose_gnn_amd.query_pose import QueryPose  # noqa: E402
from relpose_gnn_amd.resnet import resnet34  # noqa: E402
from relpose_gnn_amd.retrieval import PoseGate, RetrievalRule  # noqa: E402
from relpose_gnn_amd.tracking import Tracker  # noqa: E402

D, K = 2048, 7
SIZES = [(m, g) for m in (1000, 100000) for g in (1, 64)]


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=20).stdout
        return [ln.strip() for ln in out.splitlines() if "sclk" in ln or "mclk" in ln][:2]
    except Exception as e:                                   # the tool is optional: the numbers stand without it
        return [f"unavailable: {type(e).__name__}"]


def window_us(fn, n):
    """Microseconds per call over ``n`` back-to-back calls, host clock, ended by a synchronise."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / n


def alternate(sides: dict, runs: int, window: float) -> dict:
    """``sides``: name -> callable.  Warm-up and calibration per side, then ``runs`` windows per side, alternating."""
    count = {}
    for name, fn in sides.items():
        for _ in range(3):
            fn()
        per = window_us(fn, 10)
        count[name] = max(10, int(np.ceil(window * 1.1e6 / per)))
    got = {name: [] for name in sides}
    for _ in range(runs):
        for name, fn in sides.items():
            got[name].append(window_us(fn, count[name]))
    out = {}
    for name, v in got.items():
        med = float(np.median(v))
        out[name] = {"us": [round(x, 2) for x in v], "median_us": round(med, 2), "spread": round((max(v) - min(v)) / med, 4),
                     "calls_per_window": count[name]}
    return out


def _retrieval_inputs(dev, m, g, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    db = torch.randn((m, D), device=dev, generator=gen)
    q = torch.randn((g, D), device=dev, generator=gen)
    ranks = torch.arange(K, dtype=torch.int32, device=dev).repeat(g, 1)
    lib = _lib.lib()
    ws = torch.empty(int(lib.rpg_retrieve_workspace_bytes(g, m, D)), dtype=torch.uint8, device=dev)
    return db, q, ranks, ops.row_inv_norms(db), ws


def parent_leg(dev, parent_path, runs, window):
    parent = C.CDLL(parent_path)
    parent.rpg_retrieve_cosine_f32.argtypes = _lib.lib().rpg_retrieve_cosine_f32.argtypes
    rows = []
    for m, g in SIZES:
        db, q, ranks, inv, ws = _retrieval_inputs(dev, m, g, 1)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        outs = {}

        def call(lib, name):
            nb = outs.setdefault(name, (torch.empty((g, K), dtype=torch.int64, device=dev),
                                        torch.empty((g, K), dtype=torch.float32, device=dev)))
            stream = torch.cuda.current_stream().cuda_stream

            def fn():
                rc = lib.rpg_retrieve_cosine_f32(q.data_ptr(), db.data_ptr(), inv.data_ptr(), None, None, ranks.data_ptr(), g, K, m, D,
                                                 nb[0].data_ptr(), nb[1].data_ptr(), ws.data_ptr(), ws.numel(), status.data_ptr(),
                                                 stream)
                assert rc == 0, rc
            return fn
        res = alternate({"this": call(_lib.lib(), "this"), "parent": call(parent, "parent")}, runs, window)
        torch.cuda.synchronize()
        same = bool(torch.equal(outs["this"][0], outs["parent"][0])
                    and torch.equal(outs["this"][1].view(torch.int32), outs["parent"][1].view(torch.int32)))
        ratio = res["this"]["median_us"] / res["parent"]["median_us"]
        spread = max(res["this"]["spread"], res["parent"]["spread"])
        rows.append({"M": m, "D": D, "G": g, "this": res["this"], "parent": res["parent"], "this_over_parent": round(ratio, 4),
                     "larger_spread": spread, "within_spread": bool(abs(ratio - 1.0) <= spread), "results_bit_identical": same,
                     "bad_ranks": int(status.item())})
        print(rows[-1], flush=True)
        del db, q, ws
        torch.cuda.empty_cache()
    return rows


def gated_leg(dev, runs, window):
    rows = []
    for m, g in SIZES:
        db, q, ranks, inv, ws = _retrieval_inputs(dev, m, g, 2)
        gen = torch.Generator(device=dev).manual_seed(3)
        gate_rows = torch.cat([torch.rand((m, 3), device=dev, generator=gen, dtype=torch.float64) * 10.0,
                               torch.nn.functional.normalize(torch.randn((m, 4), device=dev, generator=gen, dtype=torch.float64), dim=1)], 1)
        prior = gate_rows[torch.arange(g, device=dev) * 7 % m].clone()
        gate = PoseGate(4.0, 120.0)                          # about a quarter of the box, a third of the rotations: far above K rows
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        out = torch.empty((g, K), dtype=torch.int64, device=dev)
        info = torch.empty((g, 2), dtype=torch.int32, device=dev)

        def ungated():
            ops.retrieve(q, db, ranks, db_inv_norm=inv, status=status, workspace=ws, out=out)

        def gated():
            ops.retrieve_gated(q, db, ranks, gate_rows, prior, gate.r2, gate.cos_half, gate.rot, db_inv_norm=inv, status=status,
                               workspace=ws, out=out, gate_info=info)
        res = alternate({"ungated": ungated, "gated": gated}, runs, window)
        h = info.cpu().numpy()
        rows.append({"M": m, "D": D, "G": g, "ungated": res["ungated"], "gated": res["gated"],
                     "gated_over_ungated": round(res["gated"]["median_us"] / res["ungated"]["median_us"], 4),
                     "extra_us": round(res["gated"]["median_us"] - res["ungated"]["median_us"], 2),
                     "queries_gated": int((h[:, 0] == 0).sum()), "median_rows_inside": float(np.median(h[:, 1])),
                     "bad_ranks": int(status.item())})
        print(rows[-1], flush=True)
        del db, q, ws, gate_rows
        torch.cuda.empty_cache()
    return rows


def tracker_leg(dev, runs, window):
    m_rows = 4000
    model = PoseNetX_R2(resnet34(), droprate=0.0, pretrained=False, feat_dim=D, edge_feat_dim=D, node_dim=D, input_img_height=224,
                        use_gnn=True, knn=-1, use_AP=True, gnn_recursion=2)
    model.load_state_dict(S.synth_state_dict(S.posenet_r2_param_shapes(D, D, D), seed=1))
    model = model.to(dev).eval()
    gen = torch.Generator(device=dev).manual_seed(1)
    poses = torch.randn((m_rows, 6), device=dev, generator=gen) * 0.1
    fmap = FeatureMap(torch.randn((m_rows, D), device=dev, generator=gen).relu_(), FeatureMap.model_meta(model), poses)
    frame = torch.randn((1, 3 * 224 * 224), device=dev, generator=gen)
    # wide enough that the accepted pose of the synthetic weights keeps K rows inside: the frames after the first are GATED (state 0:
    # the counting sweep and the gated key-writing sweep both run), which the last frame's gate_info below records
    rule, gate = RetrievalRule(k=K), PoseGate(1e3, 180.0)
    mk_pose = lambda: QueryPose(fuse="consensus", inlier_t=1e6, inlier_deg=360.0)    # every frame accepted: the gated path runs
    ungated = GraphedForwardMap(model, fmap, frame, rule=rule, pose=mk_pose(), outputs="query")
    captured = Tracker(model, fmap, rule, gate, mk_pose(), capture=True, example=frame)
    eager = Tracker(model, fmap, rule, gate, mk_pose(), capture=False)
    res = alternate({"ungated_replay": lambda: ungated(frame), "tracker_captured": lambda: captured.step(frame),
                     "tracker_eager": lambda: eager.step(frame)}, runs, window)
    states = {"captured": captured.step(frame).gate_info.cpu().numpy().tolist(), "eager": eager.step(frame).gate_info.cpu().numpy().tolist()}
    model.check_edge_index()
    for v in res.values():
        v["frames_per_s"] = round(1e6 / v["median_us"], 1)
    return {"map_rows": m_rows, "geometry": "224x224", "precision": "f32", "D": D, "K": K, "streams": 1, "outputs": "query",
            "sides": res, "gate_info_last_frame": states,
            "captured_over_ungated_replay": round(res["tracker_captured"]["median_us"] / res["ungated_replay"]["median_us"], 4),
            "captured_over_eager": round(res["tracker_captured"]["median_us"] / res["tracker_eager"]["median_us"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="a build of the parent commit's library (leg 1 is skipped without)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.4)
    ap.add_argument("--legs", default="parent,gated,tracker")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_gate_bench.json"))
    args = ap.parse_args()
    if args.runs < 3 or args.window < 0.4:
        raise SystemExit("at least 3 runs per side, in windows of at least 0.4 s")
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    legs = set(args.legs.split(","))
    doc = {"metric": "pose_gate", "device": torch.cuda.get_device_name(0), "runs": args.runs, "window_s": args.window,
           "clocks_before": clocks()}
    if "parent" in legs:
        doc["ungated_vs_parent"] = (parent_leg(dev, args.parent_lib, args.runs, args.window) if args.parent_lib
                                    else "not measured: no --parent-lib given")
    if "gated" in legs:
        doc["gated_vs_ungated"] = gated_leg(dev, args.runs, args.window)
    if "tracker" in legs:
        doc["tracker"] = tracker_leg(dev, args.runs, args.window)
    doc["clocks_after"] = clocks()
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in doc.items() if k == "tracker"}))


if __name__ == "__main__":
    main()
