#!/usr/bin/env python3
"""The Monte-Carlo pose heads, measured (opt-in; bench.py does not call it).

  * kernel: ``ops.pose_heads_mc`` (one launch: S masked evaluations, mean and variance) against what the parent commit offers for
    the same S samples, S x (``F.dropout`` + ``ops.pose_heads``), at R = 1792 and 256 rows, d = 2048, S = 1, 8, 32.  Both sides
    run ``--inner`` calls between two device events, ``--rounds`` times in turn (A, B, A, B, ...); reported per side: every
    round's microseconds per call, median, minimum and spread (max - min) / median, and the ratio of the medians.  Next to them
    what the fused kernel's time means: the feature bytes it reads once (R d 4) per second, and Philox calls (S R d / 4) per second.
  * serving: ``relocalize`` over ``--queries`` queries in pinned host memory against a 256-row map, K = 7, 224 x 224, micro-batches
    of 64, pose rule on the device, fp32 and bf16 -- with ``droprate = 0.5`` and ``model.mc_dropout`` (S = 16), eager and
    ``capture=True``; with ``droprate = 0.5`` and torch's masks (eager: what the parent commit serves; it refuses the capture); and
    with ``droprate = 0``, eager and captured: what the always-on dropout costs in serving.  Wall clock around the call, one
    warm-up call, ``--reps`` timed ones.

usage: tools/mc_heads_bench.py [--out profiles/mc_heads_bench.json] [--rounds 7] [--inner 200] [--reps 5] [--queries 2048]
       tools/mc_heads_bench.py --skip-serving"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

D, K, MAP_ROWS, P = 2048, 7, 256, 0.5


def _summary(us):
    med = statistics.median(us)
    return {"us_per_call": [round(v, 2) for v in us], "median_us": round(med, 2), "min_us": round(min(us), 2),
            "spread": round((max(us) - min(us)) / med, 4)}


def kernel_legs(dev, rounds, inner):
    from relpose_gnn_amd import ops
    gen = torch.Generator(device=dev).manual_seed(0)
    w6 = torch.randn((6, D), device=dev, generator=gen) * D ** -0.5
    b6 = torch.randn((6,), device=dev, generator=gen)
    state = torch.zeros(2, dtype=torch.int32, device=dev)
    out = {}
    for r in (1792, 256):
        x = torch.randn((r, D), device=dev, generator=gen)
        mean, var, y = (torch.empty((r, 6), device=dev) for _ in range(3))
        for s in (1, 8, 32):
            def fused():
                ops.pose_heads_mc(x, w6, b6, P, s, 1, state, out=(mean, var))

            def composed():
                for _ in range(s):
                    ops.pose_heads(F.dropout(x, p=P), w6, b6, out=y)

            def timed(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(inner):
                    fn()
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) * 1e3 / inner
            for fn in (fused, composed):                   # warm-up: code objects, the allocator's blocks
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            a, b = [], []
            for _ in range(rounds):
                a.append(timed(fused))
                b.append(timed(composed))
            fa, fb = _summary(a), _summary(b)
            spread = max(fa["spread"], fb["spread"])
            ratio = fb["median_us"] / fa["median_us"]
            out[f"R{r}_S{s}"] = {
                "fused": fa, "composed": fb, "composed_over_fused": round(ratio, 3), "spread": spread,
                "fused_faster_beyond_spread": bool(ratio - 1.0 > spread),
                "fused_feature_GB_per_s": round(r * D * 4 / (fa["median_us"] * 1e-6) / 1e9, 1),
                "fused_philox_calls_per_s": round(s * r * (D // 4) / (fa["median_us"] * 1e-6), 0)}
            print(f"kernel R={r} S={s}: fused {fa['median_us']} us, composed {fb['median_us']} us, x{ratio:.2f}", file=sys.stderr, flush=True)
    return out


def serving_legs(dev, queries, reps):
    import relpose_gnn_amd.synth as S
    from relpose_gnn_amd.evaluate import relocalize
    from relpose_gnn_amd.featmap import FeatureMap
    from relpose_gnn_amd.mc_dropout import McDropout
    from relpose_gnn_amd.posenet import PoseNetX_R2
    from relpose_gnn_amd.resnet import resnet34
    h = w = 224
    m = PoseNetX_R2(resnet34(), droprate=P, pretrained=False, feat_dim=D, edge_feat_dim=D, node_dim=D, input_img_height=h,
                    use_gnn=True, knn=-1, use_AP=True, gnn_recursion=2)
    m.load_state_dict(S.synth_state_dict(S.posenet_r2_param_shapes(D, D, D), seed=1))
    m = m.to(dev).eval()
    gen = torch.Generator(device=dev).manual_seed(0)
    mc = McDropout(samples=16, seed=1)
    configs = (("mc16", P, mc, False), ("mc16+capture", P, mc, True), ("torch_masks", P, None, False),
               ("droprate0", 0.0, None, False), ("droprate0+capture", 0.0, None, True))
    out = {}
    for prec in ("f32", "bf16"):
        m.encoder_dtype, m.gnn_dtype = prec, prec
        fmap = FeatureMap.build(m, torch.randn((MAP_ROWS, 3 * h * w), device=dev, generator=gen),
                                poses=torch.randn((MAP_ROWS, 6), generator=torch.Generator().manual_seed(3)) * 0.3)
        qh = torch.randn((queries, 3 * h * w), generator=torch.Generator().manual_seed(1)).pin_memory()
        nbh = torch.randint(0, MAP_ROWS, (queries, K), generator=torch.Generator().manual_seed(2))
        tg = torch.randn((queries, 6), generator=torch.Generator().manual_seed(4)) * 0.3
        leg = {}
        for name, rate, sampler, capture in configs:
            m.droprate, m.mc_dropout = rate, sampler

            def call():
                return relocalize(m, fmap, qh, nbh, micro_batch=64, targets=tg, postprocess="device", capture=capture)
            call()                                         # warm-up: pipeline buffers, workspaces, the captured steps
            rates = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                rates.append(queries / (time.perf_counter() - t0))
            med = statistics.median(rates)
            leg[name] = {"queries_per_s": [round(v, 1) for v in rates], "median": round(med, 1),
                         "spread": round((max(rates) - min(rates)) / med, 4)}
            print(f"serving {prec} {name}: {leg[name]['median']} queries/s", file=sys.stderr, flush=True)
        for name in ("mc16", "mc16+capture", "torch_masks"):
            leg[name]["over_droprate0"] = round(leg[name]["median"] / leg["droprate0"]["median"], 3)
        leg["mc16+capture"]["over_mc16"] = round(leg["mc16+capture"]["median"] / leg["mc16"]["median"], 3)
        out[f"{h}x{w}_{prec}"] = leg
        del fmap, qh
        torch.cuda.empty_cache()
    m.droprate, m.mc_dropout = P, None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--skip-serving", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON document to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU (there is no fallback)"
    from relpose_gnn_amd import build as B
    dev = torch.device("cuda:0")
    doc = {"metric": "mc_heads", "d": D, "p": P, "rounds": args.rounds, "inner": args.inner, "library_digest": B.source_digest(),
           "device": torch.cuda.get_device_name(0), "cpus": len(os.sched_getaffinity(0)), "kernel": kernel_legs(dev, args.rounds, args.inner)}
    if not args.skip_serving:
        doc.update(K=K, map_rows=MAP_ROWS, queries=args.queries, micro_batch=64, reps=args.reps, samples=16,
                   serving=serving_legs(dev, args.queries, args.reps))
    print(json.dumps(doc), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
