#!/usr/bin/env python3
"""The evaluation streams with the pose rule on the host against the pose rule on the device (opt-in; bench.py does not call it).

  * ``relocalize`` over 1024 queries in pinned host memory against a 256-row map, K = 7, micro-batches of 64, at
    {224x224, 256x341} x {fp32, bf16 encoder + GNN} x postprocess {"host", "device"};
  * ``evaluate_stream`` over 8-node graphs at 256x341 bf16, the same two modes.

Every leg: one warm-up call, then ``--reps`` timed calls (wall clock around the call, which ends with everything on the host);
reported are the rates, their median and the spread (max - min) / median.  ``--baseline-root DIR`` also measures ``relocalize``
as ANOTHER checkout of this package has it (the parent commit's tree, with its own built library), in a child process, called
without the ``postprocess`` argument: the baseline the device mode is held against -- "not slower beyond the run-to-run spread".
``--fuse mean,median`` adds, per mode, a row ``MODE+FUSE`` with the streams' ``fuse=`` argument (every edge into the query
combined, not one: the fused kernel behind the forward for "device", the numpy rule for "host"), held against the same baseline;
``--legs`` keeps only the named ``relocalize`` legs (and drops the ``evaluate_stream`` one).
``--capture`` adds, per mode, a row ``MODE+capture`` with ``relocalize(..., capture=True)`` (the micro-batch step replayed from a
captured HIP graph), measures the baseline checkout's ``device`` mode next to its default one -- the row ``device+capture`` is
held against -- and adds ``latency_g1``: one query per call, the median of 200 synchronised calls of ``GraphedForwardMap``
against eager ``forward_map`` (here and in the baseline checkout).
``--only LEG`` runs one leg in one mode in a loop, for a profiler (``rocprofv3 --kernel-trace --stats -- python
tools/postprocess_bench.py --only 256x341_bf16:device``), and prints the wall time of the timed loop to relate kernel time to.

``--against MODE`` (with ``--baseline-root DIR`` and ONE mode in ``--modes``, both written as rows are named, e.g. ``--modes
device+consensus --against device+median``) holds a new mode of this checkout against another mode of the baseline checkout:
``--rounds`` times in turn a child process measures MODE there and a child process measures the mode here, so that both see the
same box in the same minutes; reported are every round's rates, the median and spread over all of a side's timed calls, and
whether this side is slower by more than the larger of 3 % and the observed spread.

``--mc-samples S`` builds the model with ``droprate = 0.5`` and ``model.mc_dropout = McDropout(S, seed 0)`` (the fused Monte-Carlo
heads) on both sides; a mode ending in ``+var`` (``device+mean+var``, ``host+consensus+var``) then runs the fused rule with
``weights="variance"``, which reads the variances those heads leave.  ``--modes device+mean+var --against device+mean --mc-samples
16`` holds the weighted rule against the baseline checkout's unweighted ``"mean"`` under the same sampler.

usage: tools/postprocess_bench.py [--reps 3] [--baseline-root DIR] [--out profiles/query_pose_bench.json]
       tools/postprocess_bench.py --fuse mean,median --baseline-root DIR --out profiles/query_pose_fused_bench.json
       tools/postprocess_bench.py --capture --baseline-root DIR --out profiles/relocalize_capture_bench.json
       tools/postprocess_bench.py --modes device+consensus --against device+median --baseline-root DIR --legs 224x224_f32,224x224_bf16 \
                                  --out profiles/consensus_pose_bench.json
       tools/postprocess_bench.py --modes device+mean+var --against device+mean --mc-samples 16 --baseline-root DIR \
                                  --legs 224x224_f32,224x224_bf16 --out profiles/weighted_pose_bench.json"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))

D, K, MAP_ROWS = 2048, 7, 256
GEOMS = ((224, 224), (256, 341))


def _arg_root():
    for i, a in enumerate(sys.argv):
        if a == "--root" and i + 1 < len(sys.argv):
            return os.path.abspath(sys.argv[i + 1])
    return os.path.dirname(HERE)


ROOT = _arg_root()
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def rates(fn, n, reps):
    fn()                                                   # warm-up: pipeline buffers, workspaces, pinned blocks
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        out.append(n / (time.perf_counter() - t0))
    med = statistics.median(out)
    return {"graphs_per_s": [round(r, 1) for r in out], "median": round(med, 1), "spread": round((max(out) - min(out)) / med, 4)}


def latency_ms(fn, calls=200):
    """Median wall time of ``calls`` synchronised calls, in ms, and the spread (p90 - p10) / median."""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    med = statistics.median(ts)
    return {"median_ms": round(med, 4), "spread": round((ts[int(0.9 * len(ts))] - ts[int(0.1 * len(ts))]) / med, 4)}


def alternate(args):
    """``--against``: the baseline checkout's mode and this checkout's mode in alternating child processes."""
    here_mode = args.modes
    if not args.baseline_root or "," in here_mode or here_mode in ("host,device", ""):
        raise SystemExit("--against needs --baseline-root and exactly one mode in --modes (e.g. --modes device+consensus)")
    sides = {"baseline": (os.path.abspath(args.baseline_root), args.against), "here": (ROOT, here_mode)}
    rounds, info = [], {}
    for _ in range(args.rounds):
        row = {}
        for side, (root, mode) in sides.items():
            cmd = [sys.executable, os.path.abspath(__file__), "--root", root, "--modes", mode, "--reps", str(args.reps), "--queries",
                   str(args.queries), "--legs", args.legs or ",".join(f"{h}x{w}_{p}" for p in ("f32", "bf16") for h, w in GEOMS),
                   "--mc-samples", str(args.mc_samples)]
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=900)
            if res.returncode != 0:
                raise SystemExit(f"the {side} run failed with exit status {res.returncode}")
            doc = json.loads(res.stdout.strip().splitlines()[-1])
            info[side] = {"mode": mode, "library_digest": doc["library_digest"]}
            info.update({k: doc[k] for k in ("K", "map_rows", "queries", "micro_batch", "reps", "device", "host", "cpus", "mc_samples")})
            row[side] = {key: leg[mode] for key, leg in doc["relocalize"].items()}
            print(f"round {len(rounds)} {side} {mode}: " + ", ".join(f"{k} {v['median']}" for k, v in row[side].items()),
                  file=sys.stderr, flush=True)
        rounds.append(row)
    out = {"metric": "query_pose_mode_against_baseline_mode", **info, "rounds": rounds, "legs": {}}
    for key in rounds[0]["here"]:
        leg = {}
        for side in sides:
            calls = [r for row in rounds for r in row[side][key]["graphs_per_s"]]
            med = statistics.median(calls)
            leg[side] = {"graphs_per_s": calls, "median": round(med, 1), "spread": round((max(calls) - min(calls)) / med, 4)}
        spread = max(leg["baseline"]["spread"], leg["here"]["spread"])
        ratio = leg["here"]["median"] / leg["baseline"]["median"]
        leg.update(here_over_baseline=round(ratio, 4), spread=spread, allowed=round(max(0.03, spread), 4),
                   slower_beyond_allowed=bool(ratio < 1.0 - max(0.03, spread)))
        out["legs"][key] = leg
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--stream-graphs", type=int, default=256)
    ap.add_argument("--root", default=None, help="the checkout whose package is measured (default: this one)")
    ap.add_argument("--modes", default="host,device", help="comma list of host, device, baseline (= no postprocess argument)")
    ap.add_argument("--baseline-root", default=None, help="another checkout (the parent commit, built) to measure as the baseline")
    ap.add_argument("--fuse", default="", help="comma list of mean, median: also measure every mode with fuse= (rows MODE+FUSE)")
    ap.add_argument("--capture", action="store_true", help="also measure every mode with capture=True (rows MODE+capture) and "
                    "the one-query latency of GraphedForwardMap")
    ap.add_argument("--g1", action="store_true", help="measure the one-query latency of eager forward_map (the baseline child "
                    "of --capture)")
    ap.add_argument("--legs", default=None, help="comma list of relocalize legs to keep, e.g. 256x341_bf16 (default: all four)")
    ap.add_argument("--only", default=None, help="LEG:MODE, e.g. 256x341_bf16:device -- that leg alone, for a profiler")
    ap.add_argument("--out", default=None, help="also write the JSON document to this file")
    ap.add_argument("--against", default=None, help="a mode of the --baseline-root checkout (e.g. device+median) to hold the one "
                    "mode of --modes against, in alternating child processes")
    ap.add_argument("--rounds", type=int, default=3, help="--against: how often each side is run")
    ap.add_argument("--mc-samples", type=int, default=0, help="S > 0: droprate = 0.5 and model.mc_dropout = McDropout(S, 0); the "
                    "+var modes need S >= 2")
    args = ap.parse_args()
    if args.against:
        return alternate(args)

    import relpose_gnn_amd.synth as S
    from relpose_gnn_amd import build as B
    from relpose_gnn_amd.evaluate import evaluate_stream, relocalize
    from relpose_gnn_amd.featmap import FeatureMap
    from relpose_gnn_amd.graph import Data, fc_edge_index
    from relpose_gnn_amd.posenet import PoseNetX_R2
    from relpose_gnn_amd.resnet import resnet34

    modes = [m for m in args.modes.split(",") if m]
    modes += [f"{m}+{f}" for f in args.fuse.split(",") if f for m in modes if m != "baseline"]
    if args.capture:
        modes += [f"{m}+capture" for m in modes if m != "baseline"]
    legs = args.legs.split(",") if args.legs else None
    only_leg, only_mode = (args.only.split(":") + [None])[:2] if args.only else (None, None)
    if only_mode:
        modes = [only_mode]
    if any(mo.endswith("+var") for mo in modes) and args.mc_samples < 2:
        raise SystemExit("a +var mode weights by the Monte-Carlo variances: give --mc-samples S >= 2")
    dev = torch.device("cuda:0")
    m = PoseNetX_R2(resnet34(), droprate=0.5 if args.mc_samples else 0.0, pretrained=False, feat_dim=D, edge_feat_dim=D, node_dim=D, input_img_height=224,
                    use_gnn=True, knn=-1, use_AP=True, gnn_recursion=2)
    m.load_state_dict(S.synth_state_dict(S.posenet_r2_param_shapes(D, D, D), seed=1))
    m = m.to(dev).eval()
    if args.mc_samples:
        from relpose_gnn_amd.mc_dropout import McDropout
        m.mc_dropout = McDropout(args.mc_samples, 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    doc = {"metric": "query_pose_postprocess", "K": K, "map_rows": MAP_ROWS, "queries": args.queries, "micro_batch": 64,
           "reps": args.reps, "mc_samples": args.mc_samples, "root": "this checkout" if args.root is None else "another checkout",
           "library_digest": B.source_digest(), "device": torch.cuda.get_device_name(0), "host": os.uname().nodename,
           "cpus": len(os.sched_getaffinity(0)), "relocalize": {}, "evaluate_stream": {}}

    def kw_of(mode):
        if mode == "baseline":
            return {}
        mode, *extra = mode.split("+")
        kw = {"postprocess": mode}
        for e in extra:                                    # "capture", "var" (the weighted rule), or the fuse mode
            kw.update({"capture": True} if e == "capture" else {"weights": "variance"} if e == "var" else {"fuse": e})
        return kw

    n = args.queries
    for prec in ("f32", "bf16"):
        m.encoder_dtype, m.gnn_dtype = prec, prec
        for h, w in GEOMS:
            key = f"{h}x{w}_{prec}"
            if (only_leg and only_leg != key) or (legs and key not in legs):
                continue
            m.input_img_height = h
            fmap = FeatureMap.build(m, torch.randn((MAP_ROWS, 3 * h * w), device=dev, generator=gen),
                                    poses=torch.randn((MAP_ROWS, 6), generator=torch.Generator().manual_seed(3)) * 0.3)
            qh = torch.randn((n, 3 * h * w), generator=torch.Generator().manual_seed(1)).pin_memory()
            nbh = torch.randint(0, MAP_ROWS, (n, K), generator=torch.Generator().manual_seed(2))
            tg = torch.randn((n, 6), generator=torch.Generator().manual_seed(4)) * 0.3
            leg = {}
            for mode in modes:
                st = {}
                fn = lambda: relocalize(m, fmap, qh, nbh, micro_batch=64, targets=tg, stats=st, **kw_of(mode))  # noqa: E731
                if only_mode:
                    fn()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(10):
                        fn()
                    wall = time.perf_counter() - t0
                    print(json.dumps({"only": args.only, "calls": 10, "wall_s": round(wall, 4),
                                      "graphs_per_s": round(10 * n / wall, 1)}), flush=True)
                    return
                leg[mode] = rates(fn, n, args.reps)
                leg[mode]["d2h_bytes"] = st.get("d2h_bytes")
            doc["relocalize"][key] = leg
            if args.capture or args.g1:
                # one query per call, everything on the device: a camera that sends one frame at a time
                q1, nb1 = qh[:1].to(dev), nbh[:1].to(dev)
                lat = {"eager": latency_ms(lambda: m.forward_map(q1, nb1, fmap))}
                if args.capture:
                    from relpose_gnn_amd.graphed import GraphedForwardMap
                    step = GraphedForwardMap(m, fmap, q1, K)
                    lat["captured"] = latency_ms(lambda: step(q1, nb1))
                    del step
                m.check_edge_index()
                doc.setdefault("latency_g1", {})[key] = lat
            del qh, fmap
            torch.cuda.empty_cache()

    # evaluate_stream: all 8 images of a graph cross the host link (pinned, as the reference's loader delivers them)
    if not only_leg and not legs and "baseline" not in modes:
        h, w = 256, 341
        m.input_img_height = h
        g_n = args.stream_graphs
        ei = fc_edge_index(K + 1)
        xs = torch.randn((g_n, K + 1, 3 * h * w), generator=torch.Generator().manual_seed(5)).pin_memory()
        ys = torch.randn((g_n, K + 1, 6), generator=torch.Generator().manual_seed(6)) * 0.3
        graphs = [Data(x=xs[i], edge_index=ei, y=ys[i]) for i in range(g_n)]
        leg = {}
        for mode in (mo for mo in modes if "capture" not in mo):       # capture is relocalize's alone
            st = {}
            leg[mode] = rates(lambda: evaluate_stream(m, graphs, dev, micro_batch=64, stats=st, **kw_of(mode)), g_n, args.reps)
            leg[mode]["d2h_bytes"] = st.get("d2h_bytes")
        doc["evaluate_stream"][f"{h}x{w}_bf16"] = leg
        del xs, graphs
    m.encoder_dtype, m.gnn_dtype = "f32", "f32"

    if args.baseline_root:
        # the parent commit's relocalize, on this box, in this visit: a fresh child process on the other checkout
        cmd = [sys.executable, os.path.abspath(__file__), "--root", os.path.abspath(args.baseline_root), "--modes",
               "baseline,device" if args.capture else "baseline", "--reps", str(args.reps), "--queries", str(args.queries)]
        cmd += (["--legs", args.legs] if args.legs else []) + (["--g1"] if args.capture else [])
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=600)
        if res.returncode != 0:
            raise SystemExit(f"baseline run failed with exit status {res.returncode}")
        base = json.loads(res.stdout.strip().splitlines()[-1])
        doc["baseline_library_digest"] = base["library_digest"]
        verdict = {}
        for key, leg in doc["relocalize"].items():
            b = base["relocalize"][key]["baseline"]
            leg["baseline"] = b
            if "device" in leg:
                d = leg["device"]
                spread = max(b["spread"], d["spread"])
                verdict[key] = {"device_over_baseline": round(d["median"] / b["median"], 3), "spread": spread,
                                "not_slower": bool(d["median"] >= b["median"] * (1.0 - spread))}
            for mode, d in leg.items():                    # the fused rows: against the same baseline and against plain "device"
                if mode.startswith("device+"):
                    spread = max(b["spread"], d["spread"])
                    v = {"over_baseline": round(d["median"] / b["median"], 3), "spread": spread,
                         "not_slower": bool(d["median"] >= b["median"] * (1.0 - spread))}
                    if "device" in leg:
                        v["over_device"] = round(d["median"] / leg["device"]["median"], 3)
                    verdict[f"{key}:{mode}"] = v
            if "device+capture" in leg and "device" in base["relocalize"][key]:
                # the captured step against the BASELINE checkout's device mode; a gain only beyond both rows' spreads
                bd, d = base["relocalize"][key]["device"], leg["device+capture"]
                leg["baseline_device"] = bd
                spread = max(bd["spread"], d["spread"])
                ratio = d["median"] / bd["median"]
                verdict[f"{key}:device+capture"] = {"over_baseline_device": round(ratio, 3), "spread": spread,
                                                    "gain": bool(ratio - 1.0 > spread), "not_slower": bool(ratio >= 1.0 - spread)}
            if key in doc.get("latency_g1", {}) and key in base.get("latency_g1", {}):
                lat = doc["latency_g1"][key]
                lat["baseline_eager"] = base["latency_g1"][key]["eager"]
                if "captured" in lat:
                    lat["captured_over_baseline_eager"] = round(lat["baseline_eager"]["median_ms"] / lat["captured"]["median_ms"], 3)
        doc["device_vs_baseline"] = verdict
    line = json.dumps(doc)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
