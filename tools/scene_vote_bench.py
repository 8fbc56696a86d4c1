#!/usr/bin/env python3
"""Finding each query's scene on the GPU (opt-in; bench.py does not call it).  One JSON document, written to ``--out`` (default
profiles/scene_vote_bench.json), three legs on the atlas of tools/scene_bench.py (7 synthetic scenes of 4000 rows, D = 2048) -- no
value is fixed in advance, every figure is written down as measured:

  * ``unchanged_entries`` (a) (only with ``--parent-lib``, a build of the PARENT commit's library): rpg_retrieve_cosine_f32,
    rpg_retrieve_cosine_gated_f32 and rpg_retrieve_cosine_scoped_f32 of this build against the parent build's, called the same
    way through ctypes on the same buffers, at M in {1000, 100000} rows and G in {1, 64}.  Their kernels gained a defaulted
    template argument and their launcher was cut in two, so the expectation is "within the run-to-run spread"; the results are
    compared bit for bit.
  * ``electing_call`` (b): ``ops.retrieve_elect`` (every query elects, ``top`` = 16), G = 1 and G = 64, against two yardsticks on
    the same atlas: the UNSCOPED call over all 28 000 rows -- the cost of looking everywhere, which a vote cannot avoid -- and the
    SCOPED call -- what a told scene costs.  Both ratios are reported; there is no target.
  * ``one_camera`` (c): the captured one-camera ``tracking.Tracker`` (consensus pose rule, ``outputs="query"``), frames per
    second: told its scene (``scenes=[s]``); with ``scenes=SceneVote`` while the camera is tracked (held in the scene it
    elected: expected at the told figure within spread); and with ``SceneVote`` when EVERY frame elects (``reset()`` ahead of
    each frame, whose four small fills are inside the window).

Timing as tools/scene_bench.py: medians of ``--runs`` windows of at least ``--window`` seconds of back-to-back calls, the sides of
a comparison alternating window by window, ``spread`` = (max - min) / median over a side's windows.  A run of some ``--legs``
only keeps the other legs of an existing ``--out`` file.

    usage: tools/scene_vote_bench.py [--parent-lib PATH] [--runs 3] [--window 0.4] [--legs parent,call,camera]"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pose_gate_bench import alternate, clocks  # noqa: E402
from relpose_gnn_amd import _lib, ops  # noqa: E402
from relpose_gnn_amd.featmap import SceneAtlas  # noqa: E402
from relpose_gnn_amd.query_pose import QueryPose  # noqa: E402
from relpose_gnn_amd.retrieval import PoseGate, RetrievalRule, SceneVote  # noqa: E402
from relpose_gnn_amd.tracking import Tracker  # noqa: E402
from scene_bench import D, H, K, N_SCENES, SCENE_ROWS, W, _model, _scene_maps  # noqa: E402

TOP = 16


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def parent_leg(dev, parent_path, runs, window):
    this, parent = _lib.lib(), C.CDLL(parent_path)
    entries = ("rpg_retrieve_cosine_f32", "rpg_retrieve_cosine_gated_f32", "rpg_retrieve_cosine_scoped_f32")
    for name in entries:
        getattr(parent, name).argtypes = getattr(this, name).argtypes
    rows = []
    for m in (1000, 100000):
        for g in (1, 64):
            gen = torch.Generator(device=dev).manual_seed(1)
            db = torch.randn((m, D), device=dev, generator=gen)
            q = torch.randn((g, D), device=dev, generator=gen)
            ranks = torch.arange(K, dtype=torch.int32, device=dev).repeat(g, 1)
            ws = torch.empty(int(this.rpg_retrieve_workspace_bytes(g, m, D)), dtype=torch.uint8, device=dev)
            inv = ops.row_inv_norms(db)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            # the gate: map rows ~ N(0, 1)^3 with unit quaternions, a prior at the origin (about half the rows inside radius 1.5)
            dbg = torch.randn((m, 7), device=dev, generator=gen, dtype=torch.float64)
            dbg[:, 3:] /= dbg[:, 3:].norm(dim=1, keepdim=True)
            prior = torch.zeros((g, 7), dtype=torch.float64, device=dev)
            prior[:, 3] = 1.0
            first = (torch.arange(N_SCENES + 1, dtype=torch.int64, device=dev) * m) // N_SCENES
            qs = (torch.arange(g, dtype=torch.int32, device=dev) % N_SCENES).contiguous()
            for entry in entries:
                outs = {}

                def make(lib, name, entry=entry, outs=outs):
                    nb, sims, info = outs.setdefault(name, (torch.empty((g, K), dtype=torch.int64, device=dev),
                                                            torch.empty((g, K), dtype=torch.float32, device=dev),
                                                            torch.zeros((g, 2), dtype=torch.int32, device=dev)))
                    stream = torch.cuda.current_stream().cuda_stream
                    head = (q.data_ptr(), db.data_ptr(), inv.data_ptr(), None, None, ranks.data_ptr(), g, K, m, D)
                    gate = (dbg.data_ptr(), prior.data_ptr(), 2.25, 0.0, 0, info.data_ptr())
                    tail = (nb.data_ptr(), sims.data_ptr(), ws.data_ptr(), ws.numel(), status.data_ptr(), stream)
                    args = head + {"rpg_retrieve_cosine_f32": (), "rpg_retrieve_cosine_gated_f32": gate,
                                   "rpg_retrieve_cosine_scoped_f32": gate + (first.data_ptr(), qs.data_ptr(), N_SCENES)}[entry] + tail
                    fn_c = getattr(lib, entry)

                    def fn():
                        rc = fn_c(*args)
                        assert rc == 0, rc
                    return fn
                res = alternate({"this": make(this, "this"), "parent": make(parent, "parent")}, runs, window)
                torch.cuda.synchronize()
                ratio = res["this"]["median_us"] / res["parent"]["median_us"]
                spread = max(res["this"]["spread"], res["parent"]["spread"])
                same = all(torch.equal(_bits(a), _bits(b)) for a, b in zip(outs["this"], outs["parent"]))
                rows.append({"entry": entry, "M": m, "D": D, "G": g, "this": res["this"], "parent": res["parent"],
                             "this_over_parent": round(ratio, 4), "larger_spread": spread,
                             "within_spread": bool(abs(ratio - 1.0) <= spread), "results_bit_identical": bool(same)})
                print(rows[-1], flush=True)
            del db, q, ws, dbg
            torch.cuda.empty_cache()
    return rows


def call_leg(dev, model, atlas, runs, window):
    lib = _lib.lib()
    m_all, inv = len(atlas), atlas.inv_norms()
    rows = []
    for g in (1, 64):
        gen = torch.Generator(device=dev).manual_seed(5 + g)
        # a query is a map row with noise on it.  The synthetic rows are independent draws -- a scene is a row range and
        # nothing else --, so only that one row ties a query to a scene and the other voters fall where chance puts them:
        # what is checked below is that the election is the recount of those voters, not that it finds the source's scene
        src = torch.randint(0, m_all, (g,), device=dev, generator=gen)
        q = (atlas.features[src] + 0.5 * torch.randn((g, D), device=dev, generator=gen)).contiguous()
        truth = (torch.bucketize(src, atlas.scene_first, right=True) - 1).to(torch.int32)
        ranks = torch.arange(K, dtype=torch.int32, device=dev).repeat(g, 1)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        out = torch.empty((g, K), dtype=torch.int64, device=dev)
        ws = torch.empty(int(lib.rpg_retrieve_elect_workspace_bytes(g, m_all, D)), dtype=torch.uint8, device=dev)
        qs, info = torch.empty(g, dtype=torch.int32, device=dev), torch.empty((g, 2), dtype=torch.int32, device=dev)
        kw = dict(db_inv_norm=inv, status=status, workspace=ws, out=out)
        calls = {"elect": lambda: ops.retrieve_elect(q, atlas.features, ranks, atlas.scene_first, TOP, q_scene=qs, scene_info=info, **kw),
                 "all_rows_unscoped": lambda: ops.retrieve(q, atlas.features, ranks, **kw),
                 "scoped_told": lambda: ops.retrieve_scoped(q, atlas.features, ranks, atlas.scene_first, truth, **kw)}
        res = alternate(calls, runs, window)
        calls["elect"]()
        elected, votes, nb_elect = qs.clone(), info[:, 1].clone(), out.clone()
        # the recount on the host: the voters from the unscoped entry, the scene with the most of them, the best-placed on a tie
        voters = ops.retrieve(q, atlas.features, torch.arange(TOP, dtype=torch.int32, device=dev).repeat(g, 1), db_inv_norm=inv)
        recount = []
        for row in (torch.bucketize(voters, atlas.scene_first, right=True) - 1).tolist():
            recount.append(max(((row.count(s), -row.index(s), s) for s in set(row)))[::2])
        ops.retrieve_scoped(q, atlas.features, ranks, atlas.scene_first, elected, **kw)
        rows.append({"G": g, "top": TOP, "atlas_rows": m_all, "D": D, "K": K, "sides": res,
                     "elect_over_all_rows": round(res["elect"]["median_us"] / res["all_rows_unscoped"]["median_us"], 4),
                     "elect_over_scoped": round(res["elect"]["median_us"] / res["scoped_told"]["median_us"], 4),
                     "elections_equal_the_host_recount": [list(r) for r in recount] == [[int(v), int(s)] for s, v in
                                                                                          zip(elected.tolist(), votes.tolist())],
                     "same_neighbours_as_scoped_by_the_elected_scenes": bool(torch.equal(nb_elect, out)),
                     "elected_the_source_rows_scene": f"{int((elected == truth).sum().item())} of {g} (chance level: see the tool)",
                     "bad_ranks": int(status.item())})
        print(rows[-1], flush=True)
    return rows


def camera_leg(dev, model, atlas, runs, window):
    rule, gate = RetrievalRule(k=K), PoseGate(1.0)
    mk_pose = lambda: QueryPose(fuse="consensus", inlier_t=1e6, inlier_deg=360.0)
    gen = torch.Generator(device=dev).manual_seed(5)
    frame = torch.randn((1, 3 * H * W), device=dev, generator=gen)
    voting = Tracker(model, atlas, rule, gate, mk_pose(), streams=1, capture=True, example=frame, scenes=SceneVote(TOP))
    first = voting.step(frame)
    scene, votes = first.scene_info[0].tolist()
    told = Tracker(model, atlas, rule, gate, mk_pose(), streams=1, capture=True, example=frame, scenes=[scene])
    told.step(frame)
    every = Tracker(model, atlas, rule, gate, mk_pose(), streams=1, capture=True, example=frame, scenes=SceneVote(TOP))

    def every_frame_elects():
        every.reset()
        every.step(frame)
    res = alternate({"told_scene": lambda: told.step(frame), "vote_held": lambda: voting.step(frame),
                     "vote_every_frame": every_frame_elects}, runs, window)
    for v in res.values():
        v["frames_per_s"] = round(1e6 / v["median_us"], 1)
    a, b = told.step(frame), voting.step(frame)
    held = b.scene_info[0].tolist()
    every_frame_elects()
    model.check_edge_index()
    return {"geometry": f"{H}x{W}", "precision": "f32", "D": D, "K": K, "scenes": N_SCENES, "rows_per_scene": SCENE_ROWS, "top": TOP,
            "elected_scene": scene, "votes": votes, "sides": res,
            "held_over_told": round(res["vote_held"]["median_us"] / res["told_scene"]["median_us"], 4),
            "every_frame_over_told": round(res["vote_every_frame"]["median_us"] / res["told_scene"]["median_us"], 4),
            "tracked_camera_is_held": held == [scene, 0], "accepted": bool(b.accepted[0].item()),
            "held_same_neighbours_as_told": bool(torch.equal(a.neighbours, b.neighbours)),
            "every_frame_scene_info": every.scene_info[0].tolist()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="a build of the parent commit's library (leg a is skipped without)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.4)
    ap.add_argument("--legs", default="parent,call,camera")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_vote_bench.json"))
    args = ap.parse_args()
    if args.runs < 3 or args.window < 0.4:
        raise SystemExit("at least 3 runs per side, in windows of at least 0.4 s")
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    legs = set(args.legs.split(","))
    doc = {}
    if legs != {"parent", "call", "camera"} and os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)                     # the legs not measured now stay as they were measured
    doc.update({"metric": "scene_vote", "device": torch.cuda.get_device_name(0), "runs": args.runs, "window_s": args.window,
                "clocks_before": clocks()})
    if "parent" in legs:
        doc["unchanged_entries"] = (parent_leg(dev, args.parent_lib, args.runs, args.window) if args.parent_lib
                                    else "not measured: no --parent-lib given")
    if legs & {"call", "camera"}:
        model = _model(dev)
        atlas = SceneAtlas.concat(_scene_maps(model, dev))
        if "call" in legs:
            doc["electing_call"] = call_leg(dev, model, atlas, args.runs, args.window)
        if "camera" in legs:
            doc["one_camera"] = camera_leg(dev, model, atlas, args.runs, args.window)
    doc["clocks_after"] = clocks()
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in doc.items() if k in ("electing_call", "one_camera")}))


if __name__ == "__main__":
    main()
