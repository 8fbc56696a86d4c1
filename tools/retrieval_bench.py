#!/usr/bin/env python3
"""Retrieval against a map on the GPU (opt-in; bench.py does not call it).  One JSON document, written to ``--out``
(default profiles/retrieval_bench.json):

  * ``kernel``: rpg_retrieve_cosine_f32 (ops.retrieve with cached inverse norms and a caller's workspace) at M = 4000 rows,
    D in {2048, 32768}, G in {1, 8, 64, 256} queries, ranks of the reference rule (K = 7, period 5, half dropped); next to it, in
    the same run, the same result composed from torch (normalize, matmul, topk(R_MAX)) as an independent yardstick; and the two
    floors that can be derived: 4 M D bytes at 5.3 TB/s (the streaming-read rate this project has measured,
    other_kernels.scatter_isolated) and 2 G M D flop at the 157.3 TFLOP/s f32 matrix peak.  ``frac_of_floor`` = the larger floor
    over the measured time.
  * ``relocalize``: graphs/s of ``relocalize`` with retrieval (plain top-7 on the map's own 2048-d features) against
    ``relocalize`` with the same neighbours given: 256 graphs, 224 x 224, fp32, micro_batch 64, queries in pinned host memory.

Timing: ``--warmup`` untimed calls, then events around ``--steps`` back-to-back calls on one stream; the device's clock state
(rocm-smi's current sclk / mclk, read only) is noted before and after.   usage: tools/retrieval_bench.py [--steps 50] [--warmup 5]"""
import argparse
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
from relpose_gnn_amd.evaluate import relocalize  # noqa: E402
from relpose_gnn_amd.featmap import FeatureMap  # noqa: E402
from relpose_gnn_amd.posenet import PoseNetX_R2  # noqa: E402
from relpose_gnn_amd.resnet import resnet34  # noqa: E402
from relpose_gnn_amd.retrieval import RetrievalRule  # noqa: E402

M = 4000
STREAM_TBS, F32_MATRIX_TFLOPS = 5.3, 157.3


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=20).stdout
        return [ln.strip() for ln in out.splitlines() if "sclk" in ln or "mclk" in ln][:2]
    except Exception as e:                                   # the tool is optional: the numbers stand without it
        return [f"unavailable: {type(e).__name__}"]


def event_us(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def kernel_leg(dev, steps, warmup):
    r_max = int(_lib.lib().rpg_retrieve_max_rank())
    rows = []
    gen = torch.Generator(device=dev).manual_seed(0)
    for d in (2048, 32768):
        db = torch.randn((M, d), device=dev, generator=gen)
        inv = ops.row_inv_norms(db)
        for g in (1, 8, 64, 256):
            q = torch.randn((g, d), device=dev, generator=gen)
            ranks = torch.from_numpy(RetrievalRule.reference(k=7, sampling_period=5, seed=g).ranks([M] * g)).to(dev)
            ws = torch.empty(int(_lib.lib().rpg_retrieve_workspace_bytes(g, M, d)), dtype=torch.uint8, device=dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            out = torch.empty((g, 7), dtype=torch.int64, device=dev)
            dbn = torch.nn.functional.normalize(db, dim=1)    # the yardstick caches its normalised map as the kernel its norms

            def hip():
                ops.retrieve(q, db, ranks, db_inv_norm=inv, status=status, workspace=ws, out=out)

            def composed():
                s = torch.nn.functional.normalize(q, dim=1) @ dbn.T
                return torch.gather(torch.topk(s, r_max, dim=1).indices, 1, ranks.long())
            n = steps if d == 2048 else max(5, steps // 5)
            t_hip, t_torch = event_us(hip, n, warmup), event_us(composed, n, warmup)
            agree = float((out == composed()).all(1).float().mean())
            floor_bw = 4.0 * M * d / (STREAM_TBS * 1e12) * 1e6
            floor_fl = 2.0 * g * M * d / (F32_MATRIX_TFLOPS * 1e12) * 1e6
            rows.append({"M": M, "D": d, "G": g, "hip_us": round(t_hip, 2), "torch_us": round(t_torch, 2),
                         "floor_bytes_us": round(floor_bw, 2), "floor_flop_us": round(floor_fl, 2),
                         "frac_of_floor": round(max(floor_bw, floor_fl) / t_hip, 3), "hip_over_torch": round(t_hip / t_torch, 3),
                         "queries_equal_to_torch": agree, "repetitions": n})
            print(rows[-1], flush=True)
            del dbn
        del db
        torch.cuda.empty_cache()
    return rows


def relocalize_leg(dev, repeats):
    d, g = 2048, 256
    m = PoseNetX_R2(resnet34(), droprate=0.0, pretrained=False, feat_dim=d, edge_feat_dim=d, node_dim=d, input_img_height=224,
                    use_gnn=True, knn=-1, use_AP=True, gnn_recursion=2)
    m.load_state_dict(S.synth_state_dict(S.posenet_r2_param_shapes(d, d, d), seed=1))
    m = m.to(dev).eval()
    gen = torch.Generator(device=dev).manual_seed(1)
    fmap = FeatureMap(torch.randn((M, d), device=dev, generator=gen).relu_(), FeatureMap.model_meta(m),
                      torch.randn((M, 6), device=dev, generator=gen) * 0.1)
    q = torch.randn((g, 3 * 224 * 224)).pin_memory()
    rule = RetrievalRule(k=7)
    st = {}
    relocalize(m, fmap, q, rule=rule, micro_batch=64, stats=st)
    nb = torch.from_numpy(st["neighbours"])

    def run(**kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        relocalize(m, fmap, q, micro_batch=64, **kw)
        torch.cuda.synchronize()
        return g / (time.perf_counter() - t0)
    with_rule, given = [], []
    for _ in range(repeats + 1):                              # alternating, first pair is the warm-up
        with_rule.append(run(rule=rule))
        given.append(run(neighbours=nb))
    a, b = float(np.median(with_rule[1:])), float(np.median(given[1:]))
    return {"graphs": g, "map_rows": M, "geometry": "224x224", "precision": "f32", "micro_batch": 64, "repeats": repeats,
            "graphs_per_s_with_retrieval": round(a, 1), "graphs_per_s_neighbours_given": round(b, 1), "ratio": round(a / b, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retrieval_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    doc = {"metric": "retrieval", "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
           "assumed_stream_TBps": STREAM_TBS, "assumed_f32_matrix_TFLOPs": F32_MATRIX_TFLOPS, "clocks_before": clocks()}
    doc["kernel"] = kernel_leg(dev, args.steps, args.warmup)
    doc["relocalize"] = relocalize_leg(dev, args.repeats)
    doc["clocks_after"] = clocks()
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["relocalize"]))


if __name__ == "__main__":
    main()
