"""``Tracker``: the closed loop of a camera that sends one frame at a time -- the pose a frame is accepted with gates the next
frame's retrieval, with no host decision between frames.

``relocalize`` and ``GraphedForwardMap`` treat every frame as if the camera could be anywhere in the scene.  A tracker keeps,
per camera (``streams`` of them, one query per camera per step), a prior pose ON THE DEVICE:

    1. the map step, its retrieval gated by the prior (``forward_map(prior=, gate=)``: ``retrieval.PoseGate``; a NaN prior ranks
       the whole map, a gate that holds too few rows falls back to it),
    2. the pose rule (``QueryPose(fuse="consensus")``: a pose and (inliers, used) per camera),
    3. one launch (``ops.track_update`` / rpg_track_update_f64) that accepts the pose -- finite, ``inliers >= min_inliers``,
       ``inliers >= min_ratio * used`` -- and makes it the prior, or counts the frame as lost and, past ``max_lost`` lost frames
       in a row, forgets the prior so that the next frame is relocalised against the whole map.

With ``capture=True`` the three are ONE captured HIP graph (the update launch is captured with the ``GraphedForwardMap`` step): a
frame is one H2D copy and one replay.

    tracker = Tracker(model, fmap, RetrievalRule(k=7), PoseGate(radius=1.0, max_deg=60), QueryPose(fuse="consensus"),
                      example=frames0)
    out = tracker.step(frames)        # TrackStep of device tensors; nothing blocks
    tracker.state()                   # host copies of prior / lost / accepted, for logging
"""
from __future__ import annotations

from collections import namedtuple
from typing import Optional

import torch

from . import ops

# what a step returns, all on the device (with capture=True: the step's static tensors, overwritten by the next step): the pose
# rule's rows float64 [S, 16], its (inliers, used) int32 [S, 2], accepted int32 [S], the gate's (state, rows inside) int32 [S, 2]
# and the retrieved map rows int64 [S, K]; with scenes=SceneVote the vote's (elected scene, its votes) int32 [S, 2] -- (held
# scene, 0) for a camera that stayed in its room --, None otherwise
TrackStep = namedtuple("TrackStep", "rows inliers accepted gate_info neighbours scene_info", defaults=(None,))


class Tracker:
    def __init__(self, model, fmap, rule, gate, pose, streams: int = 1, min_inliers: int = 2, min_ratio: float = 0.5,
                 max_lost: int = 3, capture: bool = True, outputs: str = "query", example: Optional[torch.Tensor] = None,
                 query_descriptors: Optional[torch.Tensor] = None, scenes=None):
        """``pose``: a ``QueryPose(fuse="consensus", ...)`` -- the accept rule reads its integers (anything else: ValueError).
        ``gate``: a ``retrieval.PoseGate``; ``rule``: a ``RetrievalRule`` without random draws.  ``example``: frames [streams,
        ...] as ``forward_map`` takes them (fp32, or bf16 for the bf16 encoder), on the map's GPU: the shape every step has
        (required with ``capture=True``, where it is the capture's example).  ``query_descriptors``: an example [streams, Dd] for a
        map that holds its own retrieval descriptors.  ``mc_dropout`` / ``static_knn`` models: as ``GraphedForwardMap`` takes
        them.  ``scenes`` [streams] (a ``featmap.SceneAtlas`` only, where it is required): the scene every camera stands in;
        ``self.scenes`` -- int32 [streams] on the device, static -- scopes every step's retrieval, and ``move`` rewrites it.
        A ``retrieval.SceneVote`` in its place: the tracker finds the rooms itself.  It is treated as ``lost_only``: a camera
        elects its scene from the whole atlas on its first frame, again once the update launch has forgotten its prior (past
        ``max_lost`` lost frames), and again after ``reset(streams)`` -- which in this mode also writes -1 ("elect") into those
        cameras' scenes; while it is tracked it stays in its room, at the cost of that room's rows.  ``TrackStep.scene_info`` holds
        (elected scene, votes) per camera, (held scene, 0) for one that did not elect; ``move`` raises ValueError.  With
        ``capture=True`` the vote is part of the captured graph: a frame stays one H2D copy and one replay."""
        if getattr(pose, "fuse", None) != "consensus":
            raise ValueError("Tracker: pose must be a QueryPose(fuse='consensus', ...): the accept rule reads its (inliers, used)")
        if gate is None or rule is None:
            raise ValueError("Tracker: needs a retrieval rule and a PoseGate")
        fmap.check_gate("Tracker", rule, True, gate)                    # (the prior is the tracker's own)
        if fmap.poses is None:
            raise ValueError("Tracker: the feature map holds no poses: neither the pose rule nor the gate can work without")
        streams, min_inliers, max_lost = int(streams), int(min_inliers), int(max_lost)
        min_ratio = float(min_ratio)
        if streams < 1:
            raise ValueError(f"Tracker: streams must be >= 1, got {streams}")
        if min_inliers < 0 or max_lost < 0 or not 0.0 <= min_ratio <= 1.0:
            raise ValueError(f"Tracker: needs min_inliers >= 0, max_lost >= 0 and 0 <= min_ratio <= 1 (got {min_inliers}, "
                             f"{max_lost}, {min_ratio})")
        if not isinstance(capture, bool):
            raise TypeError(f"Tracker: capture must be a bool, got {type(capture).__name__}")
        if capture and example is None:
            raise ValueError("Tracker: capture=True needs example frames [streams, ...] to capture the step with")
        if example is not None and (not torch.is_tensor(example) or example.shape[0] != streams):
            raise ValueError(f"Tracker: example must be a tensor of {streams} frame(s), one per stream")
        self.model, self.fmap, self.rule, self.gate, self.pose = model, fmap, rule, gate, pose
        self.streams, self.min_inliers, self.min_ratio, self.max_lost = streams, min_inliers, min_ratio, max_lost
        self.capture, self.outputs = capture, outputs
        dev = fmap.device
        self.lost = torch.zeros(streams, dtype=torch.int32, device=dev)
        self.accepted = torch.zeros(streams, dtype=torch.int32, device=dev)
        self._step = None
        scope = fmap._scope(scenes, streams, rule, "Tracker", lost_ok=True)  # None for one scene's map (which takes no scenes)
        self.vote = self.scene_info = None
        if scope is not None and len(scope) == 3:
            from .retrieval import SceneVote
            self.vote = SceneVote(scope[2].top, lost_only=True)
            self.scenes = torch.full((streams,), -1, dtype=torch.int32, device=dev)
            self.scene_info = torch.zeros((streams, 2), dtype=torch.int32, device=dev)
        else:
            self.scenes = None if scope is None else scope[1].clone()
        if capture:
            from .graphed import GraphedForwardMap
            # the update launch goes behind the pose rule of every step the class issues: warm-up, capture -- and so every replay
            self._step = GraphedForwardMap(model, fmap, example, rule=rule, query_descriptors=query_descriptors, pose=pose,
                                           outputs=outputs, gate=gate, _after=self._update,
                                           **({} if self.scenes is None else
                                              {"scenes": self.scenes if self.vote is None else self.vote}))
            self.prior = self._step.prior
            self.scenes = self._step.scenes       # the captured step's static tensor: what every replay reads
            self.scene_info = self._step.scene_info
        else:
            model._check_outputs(outputs, None)
            self.prior = torch.full((streams, 7), float("nan"), dtype=torch.float64, device=dev)
            self._rows, self._ints, _, self._sigma = pose.output_block(streams, dev)
            if self._sigma is not None and getattr(model, "mc_dropout", None) is None:
                raise ValueError("Tracker: a weighted pose rule reads the Monte-Carlo variances: set model.mc_dropout")
            kp = model._static_columns(None, rule.k) if getattr(model, "knn", -1) > 0 else 0
            per_node = kp or rule.k
            self._edge_first = torch.arange(streams + 1, dtype=torch.int64, device=dev) * (
                per_node if outputs == "query" else per_node * (rule.k + 1))
        self.reset()                              # (the warm-up steps of a capture have counted frames)

    def _update(self, step, out) -> None:
        """Part 3, behind a step's pose rule: the prior of the next frame.  ``step``: the ``GraphedForwardMap`` that issues it (in
        its warm-up, in its capture -- and so in every replay), or None for the eager loop."""
        prior, ints = (self.prior, self._ints) if step is None else (step.prior, step.inliers)
        ops.track_update(out.rows, ints, prior, self.lost, self.accepted, self.min_inliers, self.min_ratio, self.max_lost)

    @torch.no_grad()
    def step(self, frames: torch.Tensor, query_descriptors: Optional[torch.Tensor] = None) -> TrackStep:
        """One frame per camera, ``frames`` [streams, ...] on the map's GPU -> ``TrackStep``.  Nothing blocks and no value
        crosses to the host."""
        if not torch.is_tensor(frames) or frames.shape[0] != self.streams:
            raise ValueError(f"Tracker.step: frames must be a tensor of {self.streams} frame(s), one per stream")
        if self._step is not None:
            out = self._step(frames, query_descriptors=query_descriptors)        # prior=None: the device's own
            return TrackStep(out.rows, self._step.inliers, self.accepted, self._step.gate_info, out.neighbours, self.scene_info)
        m = self.model
        ab, rel, ei, nb = m.forward_map(frames, None, self.fmap, rule=self.rule, query_descriptors=query_descriptors,
                                        outputs=self.outputs, prior=self.prior, gate=self.gate,
                                        **({} if self.scenes is None else {"scenes": self.scenes} if self.vote is None else
                                           {"scenes": self.vote, "_vote": (self.scenes, self.scene_info)}))
        info = m.gate_info
        var = None if self._sigma is None else m.mc_dropout.last.rel_var
        rows = self.pose.from_map(rel, ei, self.fmap, nb, edge_first=self._edge_first, out=self._rows, inliers=self._ints,
                                  rel_var=var, spread=self._sigma)
        out = TrackStep(rows, self._ints, self.accepted, info, nb, self.scene_info)
        self._update(None, out)
        return out

    def reset(self, streams=None) -> None:
        """Forget the prior of every camera (or of the cameras ``streams``, indices): their next frame is relocalised against
        the whole map, and their ``lost`` count starts at 0.  With a ``SceneVote`` their scenes are forgotten too (-1): the
        next frame elects them."""
        if streams is None:
            self.prior.fill_(float("nan"))
            if self.vote is not None:
                self.scenes.fill_(-1)
            self.lost.zero_()
            self.accepted.zero_()
            return
        idx = torch.as_tensor(streams, dtype=torch.int64).reshape(-1)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= self.streams):
            raise IndexError(f"Tracker.reset: stream index outside [0, {self.streams})")
        idx = idx.to(self.prior.device)
        self.prior[idx] = float("nan")
        if self.vote is not None:
            self.scenes[idx] = -1
        self.lost[idx] = 0
        self.accepted[idx] = 0

    def move(self, stream: int, scene: int) -> None:
        """Camera ``stream`` now stands in ``scene`` (an index of the atlas): written into the static scenes, so the next step
        ranks its frame there with no new capture -- and its prior and ``lost`` count are forgotten, because a prior from
        another room must not gate."""
        if self.scenes is None:
            raise ValueError("Tracker.move: the tracker's map is one scene's FeatureMap (scenes belong to a SceneAtlas)")
        if self.vote is not None:
            raise ValueError("Tracker.move: this tracker finds the rooms itself (scenes=SceneVote): reset(streams) makes a camera "
                             "elect its scene again")
        stream, scene = int(stream), int(scene)
        if not 0 <= stream < self.streams:
            raise IndexError(f"Tracker.move: stream index outside [0, {self.streams})")
        if not 0 <= scene < self.fmap.n_scenes:
            raise IndexError(f"Tracker.move: scene outside [0, {self.fmap.n_scenes})")
        self.scenes[stream] = scene
        self.reset([stream])

    def state(self) -> dict:
        """Host copies of ``prior`` [S, 7], ``lost`` [S] and ``accepted`` [S] (numpy; this waits for the device)."""
        return {"prior": self.prior.cpu().numpy(), "lost": self.lost.cpu().numpy(), "accepted": self.accepted.cpu().numpy()}
