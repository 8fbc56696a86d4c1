#!/usr/bin/env python3
"""Several scenes in one map on the GPU (opt-in; bench.py does not call it).  One JSON document, written to ``--out`` (default
profiles/scene_atlas_bench.json), three legs -- no value is fixed in advance, every figure is written down as measured:

  * ``relocalize`` (a): ``relocalize`` over 1024 pinned queries spread evenly over 7 synthetic scenes of 4000 rows (K = 7, 224 x
    224, ResNet-34, D = 2048, fp32 and bf16, ``postprocess="device"``, ``outputs="query"``, micro-batches of 64), eager and
    captured: ONE call on the ``SceneAtlas`` with ``scenes=`` against the way without an atlas -- seven calls on the seven
    scenes' own maps, each with its partial last micro-batch.  Both sides return the same rows (checked: the neighbours of the
    atlas call, minus each scene's offset, equal the per-scene calls').
  * ``one_camera`` (b): the captured one-camera step (``GraphedForwardMap``, consensus pose rule, ``outputs="query"``) on the atlas
    against the same step on that scene's own 4000-row map and against an UNSCOPED retrieval over all 28 000 rows (the atlas's
    storage as one plain ``FeatureMap``: what concatenating by hand would rank); and the retrieval call alone at G = 1 the same
    three ways.  The expectation is that the first two agree within spread and the third is slower: the early exit of the dot
    workgroups and the scoped sweeps of the selection are there for exactly that.
  * ``unscoped_vs_parent`` (c) (only with ``--parent-lib``, a build of the PARENT commit's library): rpg_retrieve_cosine_f32 and
    rpg_frames_u8_to_f32 of this build against the parent build's, called the same way through ctypes on the same buffers, at M
    in {1000, 100000} rows (G in {1, 64}) and on 64 frames of 480 x 640.  The unscoped paths gained a template argument and an
    empty struct, so the expectation is "within the run-to-run spread"; results are compared bit for bit.

Timing as tools/pose_gate_bench.py: medians of ``--runs`` windows of at least ``--window`` seconds of back-to-back calls, the
sides of a comparison alternating window by window, ``spread`` = (max - min) / median over a side's windows; a relocalize call
is its own window (wall clock around the call, after ``--warmup-calls`` calls per side: the first calls of a process load the
kernels of every micro-batch shape they meet).  A run of some ``--legs`` only keeps the other legs of an existing ``--out`` file.

    usage: tools/scene_bench.py [--parent-lib PATH] [--runs 3] [--window 0.4] [--legs relocalize,one_camera,parent]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import relpose_gnn_amd.synth as S  # noqa: E402
from pose_gate_bench import alternate, clocks  # noqa: E402
from relpose_gnn_amd import _lib, ops  # noqa: E402
from relpose_gnn_amd.evaluate import relocalize  # noqa: E402
from relpose_gnn_amd.featmap import FeatureMap, SceneAtlas  # noqa: E402
from relpose_gnn_amd.frames import FrameTransform  # noqa: E402
from relpose_gnn_amd.graphed import GraphedForwardMap  # noqa: E402
from relpose_gnn_amd.posenet import PoseNetX_R2  # noqa: E402
from relpose_gnn_amd.query_pose import QueryPose  # noqa: E402
from relpose_gnn_amd.resnet import resnet34  # noqa: E402
from relpose_gnn_amd.retrieval import RetrievalRule  # noqa: E402

D, K, N_SCENES, SCENE_ROWS, QUERIES, MB = 2048, 7, 7, 4000, 1024, 64
H = W = 224


def _model(dev):
    m = PoseNetX_R2(resnet34(), droprate=0.0, pretrained=False, feat_dim=D, edge_feat_dim=D, node_dim=D, input_img_height=H,
                    use_gnn=True, knn=-1, use_AP=True, gnn_recursion=2)
    m.load_state_dict(S.synth_state_dict(S.posenet_r2_param_shapes(D, D, D), seed=1))
    return m.to(dev).eval()


def _scene_maps(model, dev, seed=1):
    gen = torch.Generator(device=dev).manual_seed(seed)
    meta = FeatureMap.model_meta(model)
    return [FeatureMap(torch.randn((SCENE_ROWS, D), device=dev, generator=gen).relu_(), meta,
                       torch.randn((SCENE_ROWS, 6), device=dev, generator=gen) * 0.1) for _ in range(N_SCENES)]


def _summary(v):
    med = float(np.median(v))
    return {"s": [round(x, 4) for x in v], "median_s": round(med, 4), "spread": round((max(v) - min(v)) / med, 4),
            "queries_per_s": round(QUERIES / med, 1)}


def relocalize_leg(dev, runs, warmup_calls):
    model = _model(dev)
    rule = RetrievalRule(k=K)
    scenes = np.arange(QUERIES) % N_SCENES
    qh = torch.randn((QUERIES, 3 * H * W), generator=torch.Generator().manual_seed(2)).pin_memory()
    by_scene = [torch.from_numpy(np.flatnonzero(scenes == s)) for s in range(N_SCENES)]
    q_of = [qh[idx].pin_memory() for idx in by_scene]          # the per-scene loop's own pinned query blocks, made ahead of the clock
    rows = []
    for prec in ("f32", "bf16"):
        model.encoder_dtype, model.gnn_dtype = prec, prec
        maps = _scene_maps(model, dev)
        atlas = SceneAtlas.concat(maps)
        for capture in (False, True):
            kw = dict(micro_batch=MB, postprocess="device", outputs="query", rule=rule, capture=capture)

            def one_call(stats=None):
                return relocalize(model, atlas, qh, scenes=scenes, stats=stats, **kw)

            def seven_calls(stats=None):
                out = []
                for s in range(N_SCENES):
                    st = {}
                    out.append(relocalize(model, maps[s], q_of[s], stats=st, **kw))
                    if stats is not None:
                        stats.setdefault("neighbours", []).append(st["neighbours"])
                return out
            sa, sb = {}, {}
            pa, pb = one_call(sa), seven_calls(sb)               # warm-up: pipeline buffers, workspaces, captures -- and the check
            for _ in range(warmup_calls - 1):
                one_call()
                seven_calls()
            same_rows = all(np.array_equal(sa["neighbours"][by_scene[s].numpy()] - int(atlas.scene_first_host[s]), sb["neighbours"][s])
                            for s in range(N_SCENES))
            same_poses = all(np.array_equal(pa[by_scene[s].numpy()], pb[s]) for s in range(N_SCENES))
            t = {"atlas_one_call": [], "seven_maps_seven_calls": []}
            for _ in range(runs):
                for name, fn in (("atlas_one_call", one_call), ("seven_maps_seven_calls", seven_calls)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    t[name].append(time.perf_counter() - t0)
            res = {name: _summary(v) for name, v in t.items()}
            if capture:                                          # how many steps a call captured anew, after all the calls above
                st = {}
                one_call(st)
                res["atlas_one_call"]["graphs_captured_per_call"] = st["graphs_captured"]
                n = 0
                for s in range(N_SCENES):
                    st = {}
                    relocalize(model, maps[s], q_of[s], stats=st, **kw)
                    n += st["graphs_captured"]
                res["seven_maps_seven_calls"]["graphs_captured_per_call"] = n
            ratio = res["atlas_one_call"]["median_s"] / res["seven_maps_seven_calls"]["median_s"]
            rows.append({"precision": prec, "capture": capture, "queries": QUERIES, "scenes": N_SCENES, "rows_per_scene": SCENE_ROWS,
                         "micro_batch": MB, "warmup_calls": warmup_calls, **res, "atlas_over_seven_calls": round(ratio, 4),
                         "same_neighbours": bool(same_rows), "same_poses_bit_for_bit": bool(same_poses)})
            print(rows[-1], flush=True)
            model.check_edge_index()
        del maps, atlas
        torch.cuda.empty_cache()
    model.encoder_dtype, model.gnn_dtype = "f32", "f32"
    return rows


def one_camera_leg(dev, runs, window):
    model = _model(dev)
    maps = _scene_maps(model, dev)
    atlas = SceneAtlas.concat(maps)
    scene = 3
    own = atlas.scene(scene)
    whole = FeatureMap(atlas.features, atlas.meta, atlas.poses)          # every row ranked: what a hand-made concatenation does
    rule = RetrievalRule(k=K)
    gen = torch.Generator(device=dev).manual_seed(5)
    frame = torch.randn((1, 3 * H * W), device=dev, generator=gen)
    mk_pose = lambda: QueryPose(fuse="consensus", inlier_t=1e6, inlier_deg=360.0)
    steps = {"atlas_scoped": GraphedForwardMap(model, atlas, frame, rule=rule, pose=mk_pose(), outputs="query", scenes=[scene]),
             "own_map": GraphedForwardMap(model, own, frame, rule=rule, pose=mk_pose(), outputs="query"),
             "all_rows_unscoped": GraphedForwardMap(model, whole, frame, rule=rule, pose=mk_pose(), outputs="query")}
    res = alternate({name: (lambda st=st: st(frame)) for name, st in steps.items()}, runs, window)
    for v in res.values():
        v["frames_per_s"] = round(1e6 / v["median_us"], 1)
    a = steps["atlas_scoped"](frame).neighbours.clone()
    b = steps["own_map"](frame).neighbours.clone()
    step_doc = {"sides": res, "atlas_over_own_map": round(res["atlas_scoped"]["median_us"] / res["own_map"]["median_us"], 4),
                "all_rows_over_atlas": round(res["all_rows_unscoped"]["median_us"] / res["atlas_scoped"]["median_us"], 4),
                "same_neighbours_as_own_map": bool(torch.equal(a - int(atlas.scene_first_host[scene]), b))}
    # the retrieval call alone, one query
    q = torch.randn((1, D), device=dev, generator=gen)
    ranks = torch.arange(K, dtype=torch.int32, device=dev).repeat(1, 1)
    qs = torch.tensor([scene], dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.empty((1, K), dtype=torch.int64, device=dev)
    m_all = len(atlas)
    ws = torch.empty(int(_lib.lib().rpg_retrieve_workspace_bytes(1, m_all, D)), dtype=torch.uint8, device=dev)
    inv_all, inv_own = atlas.inv_norms(), own.inv_norms()
    calls = {"atlas_scoped": lambda: ops.retrieve_scoped(q, atlas.features, ranks, atlas.scene_first, qs, db_inv_norm=inv_all,
                                                         status=status, workspace=ws, out=out),
             "own_map": lambda: ops.retrieve(q, own.features, ranks, db_inv_norm=inv_own, status=status, workspace=ws, out=out),
             "all_rows_unscoped": lambda: ops.retrieve(q, atlas.features, ranks, db_inv_norm=inv_all, status=status, workspace=ws, out=out)}
    rres = alternate(calls, runs, window)
    model.check_edge_index()
    return {"geometry": f"{H}x{W}", "precision": "f32", "D": D, "K": K, "scenes": N_SCENES, "rows_per_scene": SCENE_ROWS,
            "atlas_rows": m_all, "camera_scene": scene, "captured_step": step_doc,
            "retrieval_alone_G1": {"sides": rres,
                                   "atlas_over_own_map": round(rres["atlas_scoped"]["median_us"] / rres["own_map"]["median_us"], 4),
                                   "all_rows_over_atlas": round(rres["all_rows_unscoped"]["median_us"] / rres["atlas_scoped"]["median_us"], 4),
                                   "bad_ranks": int(status.item())}}


def parent_leg(dev, parent_path, runs, window):
    this, parent = _lib.lib(), C.CDLL(parent_path)
    parent.rpg_retrieve_cosine_f32.argtypes = this.rpg_retrieve_cosine_f32.argtypes
    parent.rpg_frames_u8_to_f32.argtypes = this.rpg_frames_u8_to_f32.argtypes
    rows = []

    def compare(what, make, outs_equal):
        res = alternate({"this": make(this, "this"), "parent": make(parent, "parent")}, runs, window)
        torch.cuda.synchronize()
        ratio = res["this"]["median_us"] / res["parent"]["median_us"]
        spread = max(res["this"]["spread"], res["parent"]["spread"])
        rows.append({**what, "this": res["this"], "parent": res["parent"], "this_over_parent": round(ratio, 4), "larger_spread": spread,
                     "within_spread": bool(abs(ratio - 1.0) <= spread), "results_bit_identical": bool(outs_equal())})
        print(rows[-1], flush=True)

    for m in (1000, 100000):
        for g in (1, 64):
            gen = torch.Generator(device=dev).manual_seed(1)
            db = torch.randn((m, D), device=dev, generator=gen)
            q = torch.randn((g, D), device=dev, generator=gen)
            ranks = torch.arange(K, dtype=torch.int32, device=dev).repeat(g, 1)
            ws = torch.empty(int(this.rpg_retrieve_workspace_bytes(g, m, D)), dtype=torch.uint8, device=dev)
            inv = ops.row_inv_norms(db)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            outs = {}

            def make(lib, name):
                nb = outs.setdefault(name, (torch.empty((g, K), dtype=torch.int64, device=dev),
                                            torch.empty((g, K), dtype=torch.float32, device=dev)))
                stream = torch.cuda.current_stream().cuda_stream

                def fn():
                    rc = lib.rpg_retrieve_cosine_f32(q.data_ptr(), db.data_ptr(), inv.data_ptr(), None, None, ranks.data_ptr(), g, K, m, D,
                                                     nb[0].data_ptr(), nb[1].data_ptr(), ws.data_ptr(), ws.numel(), status.data_ptr(),
                                                     stream)
                    assert rc == 0, rc
                return fn
            compare({"entry": "rpg_retrieve_cosine_f32", "M": m, "D": D, "G": g}, make,
                    lambda: torch.equal(outs["this"][0], outs["parent"][0])
                    and torch.equal(outs["this"][1].view(torch.int32), outs["parent"][1].view(torch.int32)))
            del db, q, ws
            torch.cuda.empty_cache()

    n, fh, fw = 64, 480, 640
    ft = FrameTransform(256, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
    frames = torch.randint(0, 256, (n, fh, fw, 3), dtype=torch.uint8, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    (oh, ow), (hb, hw, vb, vw) = ft.tables(fh, fw, dev)
    outs = {}

    def make_frames(lib, name):
        out = outs.setdefault(name, torch.empty((n, 3, oh, ow), dtype=torch.float32, device=dev))
        stream = torch.cuda.current_stream().cuda_stream
        p = lambda t: None if t is None else t.data_ptr()

        def fn():
            rc = lib.rpg_frames_u8_to_f32(frames.data_ptr(), n, fh, fw, oh, ow, p(hb), p(hw), p(vb), p(vw), *ft.mean, *ft.std,
                                          out.data_ptr(), None, 0, stream)
            assert rc == 0, rc
        return fn
    compare({"entry": "rpg_frames_u8_to_f32", "frames": n, "geometry": f"{fh}x{fw}->{oh}x{ow}"}, make_frames,
            lambda: torch.equal(outs["this"].view(torch.int32), outs["parent"].view(torch.int32)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="a build of the parent commit's library (leg c is skipped without)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.4)
    ap.add_argument("--legs", default="relocalize,one_camera,parent")
    ap.add_argument("--warmup-calls", type=int, default=2, help="relocalize calls per side ahead of the clock (leg a)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_atlas_bench.json"))
    args = ap.parse_args()
    if args.runs < 3 or args.window < 0.4 or args.warmup_calls < 1:
        raise SystemExit("at least 3 runs per side, in windows of at least 0.4 s, after at least one warm-up call")
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    legs = set(args.legs.split(","))
    doc = {}
    if legs != {"relocalize", "one_camera", "parent"} and os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)                     # the legs not measured now stay as they were measured
    doc.update({"metric": "scene_atlas", "device": torch.cuda.get_device_name(0), "runs": args.runs, "window_s": args.window,
                "clocks_before": clocks()})
    if "parent" in legs:
        doc["unscoped_vs_parent"] = (parent_leg(dev, args.parent_lib, args.runs, args.window) if args.parent_lib
                                     else "not measured: no --parent-lib given")
    if "one_camera" in legs:
        doc["one_camera"] = one_camera_leg(dev, args.runs, args.window)
    if "relocalize" in legs:
        doc["relocalize"] = relocalize_leg(dev, args.runs, args.warmup_calls)
    doc["clocks_after"] = clocks()
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in doc.items() if k in ("one_camera",)}))


if __name__ == "__main__":
    main()
