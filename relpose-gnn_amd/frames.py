"""uint8 camera frames in, the encoder's normalised input out: the reference's image transform on the GPU.

The reference runs every node image through a CPU transform before the model sees it
(/root/reference/python/niantic/datasets/dataset_7Scenes_multi.py:290-298; images from torchvision's ``default_loader``,
i.e. uint8 RGB): ``Resize(256)`` (torchvision 0.9.1 on a PIL image = Pillow ``Image.resize(..., BILINEAR)``), ``ToTensor``,
``Normalize(mean=stats[0], std=sqrt(stats[1]))``.  ``FrameTransform`` does the same on the device in one HIP launch
(``rpg_frames_u8_to_f32`` / ``_bf16``) and is bit-identical to it, so a loader can hand over the frames it holds -- a quarter
of the fp32 bytes on the host link -- instead of running the transform::

    ft = FrameTransform.from_stats_file(".../seq-01/stats.txt")
    model.frame_transform = ft                      # PoseNetX_R2 then accepts uint8 data.x [n, H, W, 3] on the GPU
    x = ft.apply(frames_u8_cuda)                    # or directly: fp32 [n, 3, 256, W'] (dtype=torch.bfloat16 for the bf16 encoder)
"""
from __future__ import annotations

import math
from typing import Dict, Sequence, Tuple

import numpy as np
import torch

from . import ops


def output_size(h: int, w: int, size: int = 256) -> Tuple[int, int]:
    """torchvision 0.9.1 ``Resize(int)`` on a PIL image (functional_pil.resize): no resize when the short side already equals
    ``size``; otherwise the short side becomes ``size`` and the long side ``int(size * long / short)``.  -> (out_h, out_w)."""
    h, w, size = int(h), int(w), int(size)
    if (w <= h and w == size) or (h <= w and h == size):
        return h, w
    if w < h:
        return int(size * h / w), size
    return size, int(size * w / h)


class FrameTransform:
    """``Resize(resize)`` + ``ToTensor`` + ``Normalize(mean, std)`` of uint8 RGB frames ``[n, H, W, 3]`` on the GPU.

    ``mean`` / ``std``: three numbers each, taken as torchvision takes them (rounded to fp32).  ``resize=None``: no resize
    (pure normalisation).  The coefficient tables of a frame geometry are built on the host once and cached per device."""

    def __init__(self, resize=256, mean: Sequence[float] = (0.0, 0.0, 0.0), std: Sequence[float] = (1.0, 1.0, 1.0)):
        if len(mean) != 3 or len(std) != 3:
            raise ValueError("mean and std need three values (R, G, B)")
        self.resize = None if resize is None else int(resize)
        if self.resize is not None and self.resize <= 0:
            raise ValueError("resize must be positive")
        self.mean = tuple(float(np.float32(v)) for v in mean)
        self.std = tuple(float(np.float32(v)) for v in std)
        if any(s == 0.0 or not math.isfinite(s) for s in self.std) or not all(math.isfinite(m) for m in self.mean):
            raise ValueError("std must be finite and non-zero, mean finite")
        self._tables: Dict[tuple, tuple] = {}

    @classmethod
    def from_stats_file(cls, path, resize=256) -> "FrameTransform":
        """The reference's per-sequence ``stats.txt`` (two rows: per-channel mean and variance): ``std = sqrt(var)`` in
        float64, as ``np.sqrt(stats[1])`` in dataset_7Scenes_multi.py:297."""
        stats = np.loadtxt(path)
        return cls(resize, mean=stats[0], std=np.sqrt(stats[1]))

    def __repr__(self) -> str:
        return f"FrameTransform(resize={self.resize}, mean={self.mean}, std={self.std})"

    def output_size(self, h: int, w: int) -> Tuple[int, int]:
        return (int(h), int(w)) if self.resize is None else output_size(h, w, self.resize)

    def tables(self, h: int, w: int, device) -> tuple:
        """((out_h, out_w), (h_bounds, h_weights, v_bounds, v_weights)) on ``device``; None for an axis that is not resized."""
        device = torch.device(device)
        key = (device, int(h), int(w))
        hit = self._tables.get(key)
        if hit is None:
            oh, ow = self.output_size(h, w)
            hb = hw = vb = vw = None
            if ow != w:
                hb, hw = (t.to(device) for t in ops.resize_table(w, ow))
            if oh != h:
                vb, vw = (t.to(device) for t in ops.resize_table(h, oh))
            hit = self._tables[key] = ((oh, ow), (hb, hw, vb, vw))
        return hit

    def apply(self, frames: torch.Tensor, dtype=torch.float32, out=None) -> torch.Tensor:
        """uint8 ``[n, H, W, 3]`` on the GPU -> ``dtype`` (fp32 or bf16) ``[n, 3, out_h, out_w]`` on the current stream."""
        if not torch.is_tensor(frames) or frames.dim() != 4 or frames.shape[3] != 3:
            raise ValueError("frames must be a uint8 tensor [n, H, W, 3] (RGB, HWC)")
        if not frames.is_cuda:
            raise RuntimeError(f"frames must be on the GPU (the transform is a HIP kernel; no CPU fallback), got {frames.device}")
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("dtype must be torch.float32 or torch.bfloat16")
        hw, tabs = self.tables(frames.shape[1], frames.shape[2], frames.device)
        fn = ops.frames_u8_to_bf16 if dtype == torch.bfloat16 else ops.frames_u8_to_f32
        return fn(frames, hw, tabs, self.mean, self.std, out=out)
