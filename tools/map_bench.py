#!/usr/bin/env python3
"""The map path against the plain forward (opt-in; bench.py does not call it).  One JSON line:

  * graphs/s of ``forward`` (all K + 1 = 8 images of every graph through the encoder) and of ``forward_map`` (the query alone;
    its 7 database images assembled from a 256-row FeatureMap) at 224x224 and 256x341, 1 / 32 / 64 / 256 graphs per call, fp32
    and bf16 (bf16 encoder + bf16 GNN, BASELINE configs[4]); ``speedup`` = forward_map / forward;
  * the latency of one query with K = 7 (``forward_map`` of one graph, host synchronisation after each call; median), next to
    the one-graph ``forward``;
  * ``relocalize`` graphs/s over queries in pinned host memory (micro-batches of 64; the query images are the only H2D bytes).

``--outputs query`` measures ``forward_map`` / ``relocalize`` in the query-only output mode (``outputs="query"``: only what the pose
rule reads, the GNN's last recursion pruned to it), ``--outputs both`` the two modes side by side, alternated per configuration;
the result then holds ``forward_map_query`` / ``relocalize_query`` and ``query_speedup`` = query / all.  For an A/B against another
checkout of the package (a baseline commit built in its own directory) ``--tree DIR`` imports the package from there; ``--legs``
picks the parts to run (the plain ``forward`` legs are the expensive ones; ``timing`` adds the per-kernel-class times of
``ops.timing_read()`` at 32 and 256 graphs), ``--postprocess`` / ``--capture`` are ``relocalize``'s.

Timing: ``--warmup`` untimed calls, then ``--steps`` calls between two host synchronisations (throughput legs); inputs are random
device tensors (the kernels' work does not depend on the values).   usage: tools/map_bench.py [--steps 10] [--warmup 3] [--out F]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

_TREE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _i, _a in enumerate(sys.argv):                  # --tree DIR: before the package is imported
    if _a == "--tree" and _i + 1 < len(sys.argv):
        _TREE = os.path.abspath(sys.argv[_i + 1])
sys.path.insert(0, _TREE)
import relpose_gnn_amd.synth as S  # noqa: E402
from relpose_gnn_amd.evaluate import relocalize  # noqa: E402
from relpose_gnn_amd.featmap import FeatureMap  # noqa: E402
from relpose_gnn_amd.graph import fc_batch  # noqa: E402
from relpose_gnn_amd.posenet import PoseNetX_R2  # noqa: E402
from relpose_gnn_amd.resnet import resnet34  # noqa: E402

D, K, MAP_ROWS = 2048, 7, 256
GEOMS = ((224, 224), (256, 341))
GRAPHS = (1, 32, 64, 256)


def throughput(fn, graphs, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return graphs * steps / (time.perf_counter() - t0)


def latency_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(max(steps, 20)):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--relocalize-queries", type=int, default=1024)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--outputs", choices=("all", "query", "both"), default="all", help="forward_map's output mode(s) to measure")
    ap.add_argument("--tree", default=None, help="import relpose_gnn_amd from this checkout instead of the script's own")
    ap.add_argument("--legs", default="forward,forward_map,latency,relocalize", help="comma-separated parts to run")
    ap.add_argument("--postprocess", choices=("host", "device"), default="host", help="relocalize's pose rule")
    ap.add_argument("--capture", choices=("off", "on", "both"), default="off", help="relocalize(capture=True), or both ways")
    args = ap.parse_args()
    legs = set(args.legs.split(","))
    modes = ("all", "query") if args.outputs == "both" else (args.outputs,)
    okw = {"all": {}, "query": {"outputs": "query"}}          # "all" passes nothing: a baseline checkout has no such argument
    dev = torch.device("cuda:0")
    m = PoseNetX_R2(resnet34(), droprate=0.0, pretrained=False, feat_dim=D, edge_feat_dim=D, node_dim=D, input_img_height=224,
                    use_gnn=True, knn=-1, use_AP=True, gnn_recursion=2)
    m.load_state_dict(S.synth_state_dict(S.posenet_r2_param_shapes(D, D, D), seed=1))
    m = m.to(dev).eval()
    gen = torch.Generator(device=dev).manual_seed(0)
    out = {"metric": "map_path", "K": K, "map_rows": MAP_ROWS, "steps": args.steps, "warmup": args.warmup,
           "forward": {}, "forward_map": {}, "speedup": {}, "latency_ms": {}, "relocalize": {}, "outputs": args.outputs,
           "tree": _TREE, "postprocess": args.postprocess, "capture": args.capture}
    if "query" in modes:
        out.update(forward_map_query={}, relocalize_query={}, query_speedup={})
    for prec in ("f32", "bf16"):
        m.encoder_dtype, m.gnn_dtype = prec, prec
        for h, w in GEOMS:
            m.input_img_height = h
            key = f"{h}x{w}_{prec}"
            fmap = FeatureMap.build(m, torch.randn((MAP_ROWS, 3 * h * w), device=dev, generator=gen))
            fwd, fmp = {}, {mode: {} for mode in modes}
            lat = {}
            for g in GRAPHS:
                x = torch.randn((g * (K + 1), 3 * h * w), device=dev, generator=gen)
                data = fc_batch(x, K + 1)
                q = x[::K + 1].contiguous()
                nb = torch.randint(0, MAP_ROWS, (g, K), device=dev, generator=gen)
                if "forward" in legs:
                    fwd[str(g)] = round(throughput(lambda: m(data), g, args.steps, args.warmup), 1)
                for mode in modes if "forward_map" in legs else ():
                    fmp[mode][str(g)] = round(throughput(lambda: m.forward_map(q, nb, fmap, **okw[mode]), g, args.steps, args.warmup), 1)
                if g == 1 and "latency" in legs:
                    if "forward" in legs:
                        lat["forward_1graph"] = round(latency_ms(lambda: m(data), args.steps, args.warmup), 3)
                    for mode in modes:
                        name = "forward_map_1query" + ("" if mode == "all" else "_query")
                        lat[name] = round(latency_ms(lambda: m.forward_map(q, nb, fmap, **okw[mode]), args.steps, args.warmup), 3)
                    out["latency_ms"][key] = lat
                if "timing" in legs and g in (32, 256):
                    # per kernel class (ops.timing_read): ms per forward_map call, summed over both streams' launches
                    from relpose_gnn_amd import ops
                    for mode in modes:
                        m.forward_map(q, nb, fmap, **okw[mode])
                        torch.cuda.synchronize()
                        ops.timing_enable(True)
                        ops.timing_read()
                        for _ in range(5):
                            m.forward_map(q, nb, fmap, **okw[mode])
                        t = ops.timing_read()
                        ops.timing_enable(False)
                        out.setdefault("kernel_ms_per_call", {}).setdefault(key, {}).setdefault(mode, {})[str(g)] = {
                            name: {"ms": round(v["ms"] / 5, 4), "launches": v["launches"] // 5} for name, v in t.items() if v["launches"]}
                del x, data, q, nb
            if "forward" in legs:
                out["forward"][key] = fwd
            if "forward_map" in legs:
                for mode in modes:
                    out["forward_map" if mode == "all" else "forward_map_query"][key] = fmp[mode]
                if "forward" in legs and "all" in modes:
                    out["speedup"][key] = {g: round(fmp["all"][g] / fwd[g], 2) for g in fwd}
                if len(modes) == 2:
                    out["query_speedup"][key] = {g: round(fmp["query"][g] / fmp["all"][g], 3) for g in fmp["all"]}
            if "relocalize" not in legs:
                del fmap
                torch.cuda.empty_cache()
                continue
            # relocalize from pinned host queries (the evaluation stream of the map path)
            n = args.relocalize_queries
            qh = torch.randn((n, 3 * h * w), generator=torch.Generator().manual_seed(1)).pin_memory()
            nbh = torch.randint(0, MAP_ROWS, (n, K), generator=torch.Generator().manual_seed(2))
            fmap.poses = torch.zeros((MAP_ROWS, 6), device=dev)
            rkw = dict(micro_batch=64)
            if args.postprocess != "host":
                rkw["postprocess"] = args.postprocess
            for mode, cap in [(mode, cap) for cap in {"off": (False,), "on": (True,), "both": (False, True)}[args.capture] for mode in modes]:
                ckw = {"capture": True} if cap else {}
                relocalize(m, fmap, qh[:128], nbh[:128], **rkw, **ckw, **okw[mode])   # warm-up (pipeline buffers, workspaces, captures)
                st = {}
                t0 = time.perf_counter()
                relocalize(m, fmap, qh, nbh, stats=st, **rkw, **ckw, **okw[mode])
                name = "relocalize" + ("" if mode == "all" else "_query") + ("_capture" if cap else "")
                out.setdefault(name, {})[key] = {
                    "queries": n, "graphs_per_s": round(n / (time.perf_counter() - t0), 1), "h2d_bytes": st["h2d_bytes"],
                    "direct_bytes": st["direct_bytes"], "d2h_bytes": st.get("d2h_bytes")}
            del qh, fmap
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
