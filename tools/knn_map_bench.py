#!/usr/bin/env python3
"""The kNN map step at fixed positions (``model.static_knn``) against the general kNN build (opt-in; bench.py does not call it).
One JSON line.  Model: ResNet34, D = 2048, ``knn = 4``, K = 7 database images per query from a 256-row FeatureMap.

  * ``forward_map``: graphs/s at 224x224 and 256x341, 1 / 32 / 64 / 256 graphs per call, fp32 and bf16, in three modes --
    ``general`` (``static_knn`` off: the waiting path, whose code ``static_knn`` does not touch), ``static_all`` and
    ``static_query`` (``outputs="query"``);
  * ``relocalize`` over queries in pinned host memory with the device pose rule (micro-batches of 64): general against static
    all / query / query + capture;
  * one captured query (``GraphedForwardMap``, G = 1, ``outputs="query"``): median latency, next to the eager modes';
  * ``schedule`` (at 32 and 64 graphs): the static step on ONE stream (``hip_streams = 1``) and the fully-connected step
    (``knn = -1`` on the same weights) on one and two streams, beside the three modes above -- what the stream schedule alone
    is worth at a shape, apart from the kNN build;
  * the kernel alone: ``ops.knn_graph_uniform`` against ``ops.knn_graph_launch`` at 2048 rows (256 graphs of 8), D = 2048, by device
    events around ``--kernel-reps`` launches.

The modes of one configuration are ALTERNATED, ``--rounds`` times over; every figure is the median of its rounds with (min, max)
beside it, so a difference can be held against the run-to-run spread on the same box.  Timing: ``--warmup`` untimed calls, then
one window of at least ``--min-seconds`` between two host synchronisations (``--steps`` calls, more where they take less);
``relocalize`` is called over all its queries again and again until the window is that long.   usage: tools/knn_map_bench.py [--rounds 3] [--steps 10] [--out F]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import relpose_gnn_amd.synth as S  # noqa: E402
from relpose_gnn_amd import ops  # noqa: E402
from relpose_gnn_amd.evaluate import relocalize  # noqa: E402
from relpose_gnn_amd.featmap import FeatureMap  # noqa: E402
from relpose_gnn_amd.graphed import GraphedForwardMap  # noqa: E402
from relpose_gnn_amd.posenet import PoseNetX_R2  # noqa: E402
from relpose_gnn_amd.resnet import resnet34  # noqa: E402

D, K, KNN, MAP_ROWS = 2048, 7, 4, 256
GEOMS = ((224, 224), (256, 341))
GRAPHS = (1, 32, 64, 256)
MODES = {"general": (False, {}), "static_all": (True, {}), "static_query": (True, {"outputs": "query"})}


def spread(vals, digits=1):
    return {"median": round(statistics.median(vals), digits), "min": round(min(vals), digits), "max": round(max(vals), digits)}


def throughput(fn, graphs, steps, warmup, min_seconds):
    """graphs/s over ONE window of at least ``min_seconds``: ``steps`` calls are timed first, and if that window was shorter the
    call count is scaled up (with a margin) and the window taken again."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    while True:
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= min_seconds:
            return graphs * steps / dt
        steps = int(steps * min_seconds / dt * 1.2) + 1


def latency_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(max(steps, 30)):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def kernel_alone(dev, rounds, reps):
    g, n_per = 256, K + 1
    x = torch.randn((g * n_per, D), device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    batch = torch.arange(g, device=dev).repeat_interleave(n_per)
    out = torch.empty((2, g * n_per * KNN), dtype=torch.int64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    fns = {"general_us": lambda: ops.knn_graph_launch(x, KNN, batch),          # its own four allocations included, as the model pays them
           "uniform_us": lambda: ops.knn_graph_uniform(x, g, n_per, KNN, out=out, irregular=cnt)}
    res = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            for _ in range(10):
                fn()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            res[name].append(a.elapsed_time(b) * 1e3 / reps)
    assert int(cnt.item()) == 0
    return {"rows": g * n_per, "d": D, "k": KNN, "reps": reps, **{name: spread(v, 2) for name, v in res.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.4, help="shortest timed window of a throughput figure")
    ap.add_argument("--relocalize-queries", type=int, default=1024)
    ap.add_argument("--kernel-reps", type=int, default=200)
    ap.add_argument("--legs", default="kernel,forward_map,schedule,latency,relocalize", help="comma-separated parts to run")
    ap.add_argument("--precisions", default="f32,bf16")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    legs = set(args.legs.split(","))
    dev = torch.device("cuda:0")
    m = PoseNetX_R2(resnet34(), droprate=0.0, pretrained=False, feat_dim=D, edge_feat_dim=D, node_dim=D, input_img_height=224,
                    use_gnn=True, knn=KNN, use_AP=True, gnn_recursion=2)
    m.load_state_dict(S.synth_state_dict(S.posenet_r2_param_shapes(D, D, D), seed=1))
    m = m.to(dev).eval()
    gen = torch.Generator(device=dev).manual_seed(0)
    out = {"metric": "knn_map_step", "K": K, "knn": KNN, "map_rows": MAP_ROWS, "rounds": args.rounds, "steps": args.steps,
           "warmup": args.warmup, "min_seconds": args.min_seconds, "forward_map": {}, "schedule": {}, "latency_ms": {}, "relocalize": {}}
    if "kernel" in legs:
        out["kernel_alone"] = kernel_alone(dev, args.rounds, args.kernel_reps)

    def run(mode, fn):
        m.static_knn = MODES[mode][0]
        try:
            return fn(MODES[mode][1])
        finally:
            m.static_knn = False

    for prec in args.precisions.split(","):
        m.encoder_dtype, m.gnn_dtype = prec, prec
        for h, w in GEOMS:
            m.input_img_height = h
            key = f"{h}x{w}_{prec}"
            fmap = FeatureMap.build(m, torch.randn((MAP_ROWS, 3 * h * w), device=dev, generator=gen))
            for g in GRAPHS if legs & {"forward_map", "latency", "schedule"} else ():
                print(f"[knn_map_bench] {key} {g} graphs", file=sys.stderr, flush=True)
                q = torch.randn((g, 3 * h * w), device=dev, generator=gen)
                # distinct map rows per query (retrieval never names a row twice): no duplicate feature rows, no irregular graph
                nb = torch.stack([torch.randperm(MAP_ROWS, device=dev, generator=gen)[:K] for _ in range(g)])
                if "forward_map" in legs:
                    res = {mode: [] for mode in MODES}
                    for _ in range(args.rounds):
                        for mode in MODES:
                            res[mode].append(run(mode, lambda kw: throughput(lambda: m.forward_map(q, nb, fmap, **kw), g, args.steps,
                                                                             args.warmup, args.min_seconds)))
                    m.check_edge_index()
                    out["forward_map"].setdefault(key, {})[str(g)] = {mode: spread(v) for mode, v in res.items()}
                if "schedule" in legs and g in (32, 64):
                    # (static_knn, knn, hip_streams): the kNN build and the stream schedule varied one at a time
                    sched = {"general": (False, KNN, 2), "static_all": (True, KNN, 2), "static_all_1stream": (True, KNN, 1),
                             "fc_2streams": (False, -1, 2), "fc_1stream": (False, -1, 1)}
                    res = {name: [] for name in sched}
                    for _ in range(args.rounds):
                        for name, (static, knn, streams) in sched.items():
                            m.static_knn, m.knn, m.hip_streams = static, knn, streams
                            try:
                                res[name].append(throughput(lambda: m.forward_map(q, nb, fmap), g, args.steps, args.warmup, args.min_seconds))
                            finally:
                                m.static_knn, m.knn, m.hip_streams = False, KNN, 2
                    m.check_edge_index()
                    out["schedule"].setdefault(key, {})[str(g)] = {name: spread(v) for name, v in res.items()}
                if g == 1 and "latency" in legs:
                    m.static_knn = True
                    step = GraphedForwardMap(m, fmap, q, K, outputs="query")
                    m.static_knn = False
                    fns = {mode: (lambda mode=mode: run(mode, lambda kw: m.forward_map(q, nb, fmap, **kw))) for mode in MODES}
                    fns["static_query_captured"] = lambda: step(q, nb)
                    res = {name: [] for name in fns}
                    for _ in range(args.rounds):
                        for name, fn in fns.items():
                            m.static_knn = name == "static_query_captured"          # the step compares the flag it was captured with
                            res[name].append(latency_ms(fn, args.steps, args.warmup))
                            m.static_knn = False
                    m.check_edge_index()
                    out["latency_ms"][key] = {name: spread(v, 3) for name, v in res.items()}
                    del step
                del q, nb
            if "relocalize" in legs:
                n = args.relocalize_queries
                print(f"[knn_map_bench] {key} relocalize", file=sys.stderr, flush=True)
                qh = torch.randn((n, 3 * h * w), generator=torch.Generator().manual_seed(1)).pin_memory()
                nbh = torch.stack([torch.randperm(MAP_ROWS, generator=torch.Generator().manual_seed(10 + i))[:K] for i in range(n)])
                fmap.poses = torch.zeros((MAP_ROWS, 6), device=dev)
                rmodes = {"general": ("general", {}), "static_all": ("static_all", {}), "static_query": ("static_query", {}),
                          "static_query_capture": ("static_query", {"capture": True})}
                res = {name: [] for name in rmodes}
                irregular = 0
                for name, (mode, ckw) in rmodes.items():                          # warm-up: pipeline buffers, workspaces, captures
                    run(mode, lambda kw: relocalize(m, fmap, qh[:128], nbh[:128], micro_batch=64, postprocess="device", **kw, **ckw))
                for _ in range(args.rounds):
                    for name, (mode, ckw) in rmodes.items():
                        calls, t0 = 0, time.perf_counter()
                        while calls == 0 or time.perf_counter() - t0 < args.min_seconds:
                            st = {}
                            run(mode, lambda kw: relocalize(m, fmap, qh, nbh, micro_batch=64, postprocess="device", stats=st, **kw, **ckw))
                            irregular += st.get("knn_irregular_batches", 0)
                            calls += 1
                        res[name].append(n * calls / (time.perf_counter() - t0))
                out["relocalize"][key] = {"queries": n, "knn_irregular_batches": irregular, **{name: spread(v) for name, v in res.items()}}
                del qh
            del fmap
            torch.cuda.empty_cache()
    m.encoder_dtype, m.gnn_dtype = "f32", "f32"
    out["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
