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


def scenes_to_device(scenes, n: int, device, who: str):
    """``scenes`` [n], one scene index per query / frame -> (host int64 numpy [n], or None for a device tensor; int32 tensor [n]
    on ``device``).  Host integers are staged through pinned memory without blocking; an int32 tensor on ``device`` is used in
    place (a captured step reads its current contents at every replay)."""
    device = torch.device(device)
    if torch.is_tensor(scenes) and scenes.is_cuda:
        if scenes.dtype != torch.int32 or tuple(scenes.shape) != (n,) or scenes.device != device:
            raise ValueError(f"{who}: scenes on the GPU must be int32 [{n}] on {device}, got {scenes.dtype} {tuple(scenes.shape)} "
                             f"on {scenes.device}")
        return None, scenes.contiguous()
    host = torch.as_tensor(scenes)
    if host.dim() != 1 or host.shape[0] != n or host.dtype.is_floating_point or host.dtype == torch.bool:
        raise ValueError(f"{who}: scenes must be integers [{n}] (one scene index per query), got {tuple(host.shape)} {host.dtype}")
    host = host.to(dtype=torch.int32).contiguous()
    if device.type != "cuda":
        return host.numpy().astype(np.int64), host.to(device)
    dev = (host if host.is_pinned() else host.pin_memory()).to(device, non_blocking=True)
    return host.numpy().astype(np.int64), dev


class SceneFrameTransform:
    """``FrameTransform`` with the statistics per scene, for batches whose frames come from several scenes (the reference reads
    one ``stats.txt`` per sequence, dataset_7Scenes_multi.py:290-298): ``means`` / ``stds`` [S, 3], rounded to fp32 as
    ``FrameTransform`` rounds them.  ``apply(frames, scenes)`` transforms frame i with the statistics of ``scenes[i]`` in one
    launch (``rpg_frames_u8_to_*_scenes``), bit-identical to ``scene(scenes[i]).apply`` on that frame.  The statistics live on the
    device, where the launch cannot check them without a wait, so they are checked here: ``std`` finite and non-zero, ``mean``
    finite (ValueError otherwise)."""

    def __init__(self, resize=256, means=((0.0, 0.0, 0.0),), stds=((1.0, 1.0, 1.0),)):
        means, stds = np.asarray(means, dtype=np.float64), np.asarray(stds, dtype=np.float64)
        if means.ndim != 2 or means.shape[1] != 3 or means.shape[0] < 1 or stds.shape != means.shape:
            raise ValueError(f"means and stds must both be [S >= 1, 3] (R, G, B per scene), got {means.shape} and {stds.shape}")
        self.resize = None if resize is None else int(resize)
        if self.resize is not None and self.resize <= 0:
            raise ValueError("resize must be positive")
        with np.errstate(over="ignore"):
            self.means, self.stds = means.astype(np.float32), stds.astype(np.float32)
        if not np.isfinite(self.stds).all() or (self.stds == 0.0).any() or not np.isfinite(self.means).all():
            raise ValueError("std must be finite and non-zero, mean finite (every scene)")
        self._geometry = FrameTransform(self.resize)          # sizes and coefficient tables do not depend on the statistics
        self._stats: Dict[torch.device, torch.Tensor] = {}

    @classmethod
    def from_stats_files(cls, paths, resize=256) -> "SceneFrameTransform":
        """One ``stats.txt`` per scene, in scene order (see ``FrameTransform.from_stats_file``)."""
        stats = [np.loadtxt(p) for p in paths]
        return cls(resize, means=[s[0] for s in stats], stds=[np.sqrt(s[1]) for s in stats])

    def __len__(self) -> int:
        return int(self.means.shape[0])

    def __repr__(self) -> str:
        return f"SceneFrameTransform(resize={self.resize}, scenes={len(self)})"

    def scene(self, i: int) -> FrameTransform:
        """The plain ``FrameTransform`` of scene ``i``."""
        i = int(i)
        if not 0 <= i < len(self):
            raise IndexError(f"scene {i} outside [0, {len(self)})")
        return FrameTransform(self.resize, mean=self.means[i], std=self.stds[i])

    def output_size(self, h: int, w: int) -> Tuple[int, int]:
        return self._geometry.output_size(h, w)

    def tables(self, h: int, w: int, device) -> tuple:
        return self._geometry.tables(h, w, device)

    def stats(self, device) -> torch.Tensor:
        """fp32 [S, 6] = mean[3], std[3] on ``device`` (made once per device)."""
        device = torch.device(device)
        hit = self._stats.get(device)
        if hit is None:
            hit = self._stats[device] = torch.from_numpy(np.concatenate([self.means, self.stds], axis=1)).to(device)
        return hit

    def apply(self, frames: torch.Tensor, scenes, dtype=torch.float32, out=None, status=None) -> torch.Tensor:
        """uint8 ``[n, H, W, 3]`` on the GPU -> ``dtype`` (fp32 or bf16) ``[n, 3, out_h, out_w]`` on the current stream, frame i
        with the statistics of ``scenes[i]``.  ``scenes`` [n]: host integers (checked here, staged without blocking), or an int32
        tensor on the frames' GPU, whose entries outside [0, S) are counted into ``status`` (``ops.frames_u8_to_f32_scenes``)."""
        if not torch.is_tensor(frames) or frames.dim() != 4 or frames.shape[3] != 3:
            raise ValueError("frames must be a uint8 tensor [n, H, W, 3] (RGB, HWC)")
        if not frames.is_cuda:
            raise RuntimeError(f"frames must be on the GPU (the transform is a HIP kernel; no CPU fallback), got {frames.device}")
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("dtype must be torch.float32 or torch.bfloat16")
        if scenes is None:
            raise ValueError("SceneFrameTransform.apply: scenes [n] (one scene index per frame) is required")
        host, dev = scenes_to_device(scenes, frames.shape[0], frames.device, "SceneFrameTransform.apply")
        if host is not None:
            if host.size and (host.min() < 0 or host.max() >= len(self)):
                raise IndexError(f"SceneFrameTransform.apply: scenes has entries outside [0, {len(self)})")
            if status is None:                    # checked on the host: nothing to read back
                status = self._sink(frames.device)
        hw, tabs = self.tables(frames.shape[1], frames.shape[2], frames.device)
        fn = ops.frames_u8_to_bf16_scenes if dtype == torch.bfloat16 else ops.frames_u8_to_f32_scenes
        return fn(frames, hw, tabs, self.stats(frames.device), dev, status=status, out=out)

    def _sink(self, device) -> torch.Tensor:
        """The counter of the calls whose scenes were checked on the host (it stays 0)."""
        key = ("sink", torch.device(device))
        hit = self._stats.get(key)
        if hit is None:
            hit = self._stats[key] = torch.zeros(1, dtype=torch.int32, device=device)
        return hit
