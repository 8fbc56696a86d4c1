"""``FeatureMap``: encoder features of a scene's database images, computed once and reused by every query.

The reference's test graphs are one query followed by ``seq_len - 1`` database frames picked by image retrieval from the scene's
training split (dataset_7Scenes_multi.py:333-345, ``x = torch.cat((query, db_batch))``), and the same database frames come back
in graph after graph.  The encoder is per image (eval-mode BatchNorm), so a database image's feature is a function of its pixels
and the encoder weights only: ``PoseNetX_R2.forward_map`` takes the query images and, per query, the indices of its database
images in a map built here, and runs the encoder on the queries alone.

A map holds raw encoder output (``PoseNetX_R2.encode``: before the optional model-level AttentionBlock, which runs per node
after assembly, posenet.py:1040-1041), so one map serves ``use_attention`` True and False alike.  Its metadata binds it to the
encoder that made it: ``feat_dim``, the encoder precision (``"f32"`` / ``"bf16"``) and a digest of the encoder weights.
``check(model)`` -- called by every ``forward_map`` -- raises ``ValueError`` when they do not match the model, so a stale map
never gives poses silently.
"""
from __future__ import annotations

from typing import Iterable, Optional, Union

import torch

FORMAT = "relpose_gnn_amd.FeatureMap/1"

ImageSource = Union[torch.Tensor, Iterable[torch.Tensor]]


def _chunks(images: ImageSource, chunk: int):
    """Chunks of at most ``chunk`` images from a tensor, or the caller's own chunks (each cut further if larger)."""
    if chunk < 1:
        raise ValueError(f"chunk must be >= 1, got {chunk}")
    parts = [images] if torch.is_tensor(images) else images
    for part in parts:
        if not torch.is_tensor(part):
            raise TypeError(f"images: expected a tensor or an iterable of tensors, got {type(part).__name__}")
        for i in range(0, part.shape[0], chunk):
            yield part[i:i + chunk]


def _poses_tensor(poses, n: int, device) -> torch.Tensor:
    p = torch.as_tensor(poses)
    if p.dim() != 2 or p.shape[1] != 6 or p.shape[0] != n:
        raise ValueError(f"poses must be [{n}, 6] (the database images' targets, [t, log q]), got {tuple(p.shape)}")
    return p.to(device=device, dtype=torch.float32).contiguous()


class FeatureMap:
    """``features`` fp32 [M, feat_dim] on the device; optional ``poses`` fp32 [M, 6] (the database images' ``y``, in the
    reference's ``[t, log q]`` target layout); ``meta`` = {"feat_dim", "precision", "encoder_digest"}."""

    def __init__(self, features: torch.Tensor, meta: dict, poses: Optional[torch.Tensor] = None):
        if not torch.is_tensor(features) or features.dim() != 2 or features.dtype != torch.float32:
            raise ValueError("features must be an fp32 tensor [M, feat_dim]")
        for key in ("feat_dim", "precision", "encoder_digest"):
            if key not in meta:
                raise ValueError(f"FeatureMap metadata lacks {key!r}")
        if int(meta["feat_dim"]) != features.shape[1]:
            raise ValueError(f"features have {features.shape[1]} columns, metadata says feat_dim = {meta['feat_dim']}")
        if poses is not None:
            poses = _poses_tensor(poses, features.shape[0], features.device)
        self.features = features.contiguous()
        self.poses = poses
        self.meta = {"feat_dim": int(meta["feat_dim"]), "precision": str(meta["precision"]),
                     "encoder_digest": str(meta["encoder_digest"])}

    def __len__(self) -> int:
        return int(self.features.shape[0])

    @property
    def feat_dim(self) -> int:
        return self.meta["feat_dim"]

    @property
    def device(self) -> torch.device:
        return self.features.device

    def __repr__(self) -> str:
        return (f"FeatureMap(rows={len(self)}, feat_dim={self.feat_dim}, precision={self.meta['precision']!r}, "
                f"poses={'yes' if self.poses is not None else 'no'}, device={self.device})")

    # ---- building --------------------------------------------------------------------------------------------------
    @staticmethod
    def model_meta(model) -> dict:
        return {"feat_dim": int(model.feature_extractor.fc.out_features), "precision": model.encoder_dtype,
                "encoder_digest": model.encoder_digest()}

    @staticmethod
    def _encode(model, images: ImageSource, chunk: int, device) -> torch.Tensor:
        feats = []
        for part in _chunks(images, chunk):
            if part.shape[0] == 0:
                continue
            if part.device != device:
                # host chunks go over one at a time: the whole database never sits on the GPU as pixels
                part = part.to(device, non_blocking=part.is_pinned())
            feats.append(model.encode(part))
        d = int(model.feature_extractor.fc.out_features)
        return torch.cat(feats) if feats else torch.empty((0, d), dtype=torch.float32, device=device)

    @classmethod
    def build(cls, model, images: ImageSource, poses=None, chunk: int = 256) -> "FeatureMap":
        """Encode ``images`` through ``model``'s encoder in chunks of ``chunk`` images.  ``images``: fp32 (or bf16, for the bf16
        encoder) processed images [n, 3*H*W] / [n, 3, H, W], or uint8 frames [n, H, W, 3] through ``model.frame_transform``;
        a host or device tensor, or an iterable of such chunks."""
        device = cls._model_device(model)
        meta = cls.model_meta(model)
        feats = cls._encode(model, images, chunk, device)
        if feats.shape[0] == 0:
            raise ValueError("FeatureMap.build: no images")
        return cls(feats, meta, None if poses is None else _poses_tensor(poses, feats.shape[0], device))

    def extend(self, model, images: ImageSource, poses=None, chunk: int = 256) -> "FeatureMap":
        """Append the features of more database images (same encoder; poses given iff the map has poses).  Returns self."""
        self.check(model)
        if (poses is None) != (self.poses is None):
            raise ValueError("extend: poses must be given exactly when the map holds poses (every row has one or none has)")
        feats = self._encode(model, images, chunk, self.device)
        if poses is not None:
            self.poses = torch.cat([self.poses, _poses_tensor(poses, feats.shape[0], self.device)])
        self.features = torch.cat([self.features, feats])
        return self

    @staticmethod
    def _model_device(model) -> torch.device:
        p = next(model.feature_extractor.parameters())
        if p.device.type != "cuda":
            raise RuntimeError("FeatureMap.build: the model must be on the GPU (the encoder runs there only)")
        return p.device

    # ---- validity ----------------------------------------------------------------------------------------------------
    def check(self, model) -> None:
        """Raise ValueError unless this map was made by ``model``'s encoder as it is now (weights, precision, feat_dim)."""
        want = self.model_meta(model)
        if want["feat_dim"] != self.meta["feat_dim"]:
            raise ValueError(f"FeatureMap has feat_dim {self.meta['feat_dim']}, the model's encoder gives {want['feat_dim']}")
        if want["precision"] != self.meta["precision"]:
            raise ValueError(f"FeatureMap was encoded with the {self.meta['precision']!r} encoder, the model's encoder_dtype is "
                             f"{want['precision']!r}: rebuild the map")
        if want["encoder_digest"] != self.meta["encoder_digest"]:
            raise ValueError("FeatureMap was encoded with other encoder weights than the model's (digest "
                             f"{self.meta['encoder_digest'][:12]} != {want['encoder_digest'][:12]}): rebuild the map")

    # ---- persistence ------------------------------------------------------------------------------------------------
    def save(self, path) -> None:
        """Plain tensors plus metadata (str / int): ``torch.load(weights_only=True)`` reads it back."""
        obj = {"format": FORMAT, "meta": dict(self.meta), "features": self.features.detach().cpu()}
        if self.poses is not None:
            obj["poses"] = self.poses.detach().cpu()
        torch.save(obj, path)

    @classmethod
    def load(cls, path, device) -> "FeatureMap":
        obj = torch.load(path, map_location="cpu", weights_only=True)
        if not isinstance(obj, dict) or obj.get("format") != FORMAT:
            raise ValueError(f"{path}: not a saved FeatureMap (format {FORMAT!r})")
        poses = obj.get("poses")
        return cls(obj["features"].to(device), obj["meta"], None if poses is None else poses.to(device))
