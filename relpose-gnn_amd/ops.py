"""Tensor-level wrappers over the C ABI (one Python function per ``rpg_*`` entry point).

PyTorch is used for device memory and the current stream only: every function takes CUDA (ROCm) fp32
tensors, allocates its output with ``torch.empty`` and launches the HIP kernel on
``torch.cuda.current_stream()``.  CPU tensors are rejected: there is no fallback path.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import numbers
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import _lib as L


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _req(t: torch.Tensor, name: str, dtype=torch.float32) -> torch.Tensor:
    if not torch.is_tensor(t):
        raise TypeError(f"{name}: expected a tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a tensor on the GPU (the HIP kernels are the only compute path), got {t.device}")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _opt(t: Optional[torch.Tensor], name: str, dtype=torch.float32) -> Optional[torch.Tensor]:
    return None if t is None else _req(t, name, dtype)


def _out(out: Optional[torch.Tensor], shape, dtype, dev, what: str) -> torch.Tensor:
    """The ``out`` argument of ``what``: checked when given, allocated otherwise."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"{what}: out must be a contiguous {dtype} {list(shape)} tensor on the inputs' GPU")
    return out


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _status_arg(status: Optional[torch.Tensor], dev, what: str, bad_dtype=ValueError) -> Tuple[torch.Tensor, bool]:
    """The ``status`` argument of ``what``: a given tensor must be int32 (``bad_dtype`` otherwise) and hold a counter on ``dev``
    (ValueError otherwise); None becomes a zeroed counter of this call's own.  -> (status, whether it is this call's own)."""
    if status is None:
        return torch.zeros(1, dtype=torch.int32, device=dev), True
    if not torch.is_tensor(status) or status.dtype != torch.int32:
        raise bad_dtype(f"{what}: status must be an int32 tensor on the inputs' GPU")
    if status.numel() < 1 or status.device != dev:
        raise ValueError(f"{what}: status must be an int32 tensor holding one counter on the inputs' GPU, got "
                         f"{status.numel()} element(s) on {status.device}")
    return status, False


def _own_count(status: torch.Tensor, own: bool) -> int:
    """What a call without a ``status`` argument counted (read back here: one synchronisation); 0 for the caller's counter,
    which the caller reads."""
    return int(status.item()) if own else 0


def nchw3_to_nhwc4(x: torch.Tensor) -> torch.Tensor:
    x = _req(x, "x")
    n, c, h, w = x.shape
    if c != 3:
        raise ValueError("expected [N,3,H,W]")
    y = torch.empty((n, h, w, 4), dtype=torch.float32, device=x.device)
    L.check(L.lib().rpg_nchw3_to_nhwc4_f32(_p(x), _p(y), n, h, w, _stream()), "nchw3_to_nhwc4")
    return y


def conv2d_bn_act_nhwc(x: torch.Tensor, w_ohwi: torch.Tensor, scale: Optional[torch.Tensor], shift: Optional[torch.Tensor],
                       residual: Optional[torch.Tensor] = None, stride: int = 1, pad: int = 0, relu: bool = False) -> torch.Tensor:
    x, w_ohwi = _req(x, "x"), _req(w_ohwi, "w_ohwi")
    n, h, w, cin = x.shape
    cout, kh, kw, cin_w = w_ohwi.shape
    if cin_w != cin:
        raise ValueError(f"channel mismatch: x has {cin}, weight has {cin_w}")
    ho, wo = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
    y = torch.empty((n, ho, wo, cout), dtype=torch.float32, device=x.device)
    scale = _opt(scale, "scale")
    shift = _opt(shift, "shift")
    residual = _opt(residual, "residual")
    if residual is not None and residual.shape != y.shape:
        raise ValueError("residual shape mismatch")
    L.check(L.lib().rpg_conv2d_bn_act_nhwc_f32(_p(x), _p(w_ohwi), _p(scale), _p(shift), _p(residual), _p(y), n, h, w, cin,
                                                cout, kh, kw, stride, pad, int(relu), _stream()), "conv2d_bn_act_nhwc")
    return y


def wino43_transform_weights(w_ohwi: torch.Tensor) -> torch.Tensor:
    """[Cout][3][3][Cin] -> Winograd F(4,3) weights U [6][Cout][3][Cin] (once per weight load), as one flat buffer of
    rpg_wino43_weights_floats(Cout, Cin) floats (18 Cout Cin; a probe build with the nested 2-D kernel appends its image)."""
    w_ohwi = _req(w_ohwi, "w_ohwi")
    cout, kh, kw, cin = w_ohwi.shape
    if (kh, kw) != (3, 3):
        raise ValueError("Winograd F(4,3) path is for 3x3 kernels")
    floats = int(L.lib().rpg_wino43_weights_floats(cout, cin))
    # [6][Cout][3][Cin] in the product build; a flat buffer when a probe build appends the nested 2-D image behind it
    shape = (6, cout, 3, cin) if floats == 18 * cout * cin else (floats,)
    u = torch.empty(shape, dtype=torch.float32, device=w_ohwi.device)
    L.check(L.lib().rpg_wino43_transform_weights_f32(_p(w_ohwi), _p(u), cout, cin, _stream()), "wino43_transform_weights")
    return u


def conv3x3_wino43_bn_act_nhwc(x: torch.Tensor, u: torch.Tensor, scale: Optional[torch.Tensor], shift: Optional[torch.Tensor],
                               residual: Optional[torch.Tensor] = None, relu: bool = False) -> torch.Tensor:
    x, u = _req(x, "x"), _req(u, "u")
    n, h, w, cin = x.shape
    per = int(L.lib().rpg_wino43_weights_floats(1, 1))            # 18 (42 in a probe build with the nested kernel)
    if u.dim() not in (1, 4) or u.numel() == 0 or u.numel() % (per * cin) or (u.dim() == 4 and tuple(u.shape[::2]) != (6, 3)):
        raise ValueError("u must come from wino43_transform_weights: [6][Cout][3][Cin]")
    if u.dim() == 4:
        if u.shape[3] != cin:
            raise ValueError(f"channel mismatch: x has {cin} channels, u was built for {u.shape[3]}")
        cout = u.shape[1]
    else:                                                          # flat buffer of a probe build: Cout from its size
        cout = u.numel() // (per * cin)
    y = torch.empty((n, h, w, cout), dtype=torch.float32, device=x.device)
    scale = _opt(scale, "scale")
    shift = _opt(shift, "shift")
    residual = _opt(residual, "residual")
    for name, t in (("scale", scale), ("shift", shift)):
        if t is not None and t.numel() != cout:
            raise ValueError(f"{name} must have Cout = {cout} elements, got {t.numel()}")
    if residual is not None and tuple(residual.shape) != (n, h, w, cout):
        raise ValueError("residual shape mismatch")
    L.check(L.lib().rpg_conv3x3_wino43_bn_act_nhwc_f32(_p(x), _p(u), _p(scale), _p(shift), _p(residual), _p(y), n, h, w, cin,
                                                        cout, int(relu), _stream()), "conv3x3_wino43_bn_act_nhwc")
    return y


def conv2d_bn_act_nhwc_bf16(x: torch.Tensor, w_ohwi: torch.Tensor, scale: Optional[torch.Tensor], shift: Optional[torch.Tensor],
                            residual: Optional[torch.Tensor] = None, stride: int = 1, pad: int = 0, relu: bool = False,
                            out_f32: bool = False) -> torch.Tensor:
    """bf16 twin of conv2d_bn_act_nhwc: x / w_ohwi / residual bf16, scale / shift fp32, fp32 accumulation."""
    x, w_ohwi = _req(x, "x", torch.bfloat16), _req(w_ohwi, "w_ohwi", torch.bfloat16)
    n, h, w, cin = x.shape
    cout, kh, kw, cin_w = w_ohwi.shape
    if cin_w != cin:
        raise ValueError(f"channel mismatch: x has {cin}, weight has {cin_w}")
    ho, wo = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
    y = torch.empty((n, ho, wo, cout), dtype=torch.float32 if out_f32 else torch.bfloat16, device=x.device)
    scale = _opt(scale, "scale")
    shift = _opt(shift, "shift")
    residual = _opt(residual, "residual", torch.bfloat16)
    L.check(L.lib().rpg_conv2d_bn_act_nhwc_bf16(_p(x), _p(w_ohwi), _p(scale), _p(shift), _p(residual), _p(y), n, h, w, cin,
                                                 cout, kh, kw, stride, pad, int(relu), int(out_f32), _stream()),
            "conv2d_bn_act_nhwc_bf16")
    return y


def basicblock64_bf16(x: torch.Tensor, w1_ohwi: torch.Tensor, scale1: torch.Tensor, shift1: torch.Tensor, w2_ohwi: torch.Tensor,
                      scale2: torch.Tensor, shift2: torch.Tensor) -> torch.Tensor:
    """relu(bn2(conv2(relu(bn1(conv1(x))))) + x) for a 64-channel identity BasicBlock in ONE kernel (the intermediate stays in
    LDS): x bf16 NHWC [n,h,w,64], weights bf16 [64,3,3,64], folded BN scale / shift fp32 [64].  Bit-identical to two
    conv2d_bn_act_nhwc_bf16 calls."""
    x = _req(x, "x", torch.bfloat16)
    w1_ohwi, w2_ohwi = _req(w1_ohwi, "w1_ohwi", torch.bfloat16), _req(w2_ohwi, "w2_ohwi", torch.bfloat16)
    n, h, w, c = x.shape
    if c != 64 or tuple(w1_ohwi.shape) != (64, 3, 3, 64) or tuple(w2_ohwi.shape) != (64, 3, 3, 64):
        raise ValueError("basicblock64_bf16: x [n,h,w,64], weights [64,3,3,64]")
    ps = [_req(t, nm) for t, nm in ((scale1, "scale1"), (shift1, "shift1"), (scale2, "scale2"), (shift2, "shift2"))]
    if any(t.numel() != 64 for t in ps):
        raise ValueError("basicblock64_bf16: scale / shift must have 64 elements")
    y = torch.empty_like(x)
    L.check(L.lib().rpg_basicblock64_bf16(_p(x), _p(w1_ohwi), _p(ps[0]), _p(ps[1]), _p(w2_ohwi), _p(ps[2]), _p(ps[3]), _p(y), n, h, w,
                                          _stream()), "basicblock64_bf16")
    return y


def probe_mfma_bf16(data: str = "relu_like", iters: int = 20000, workgroups: int = 0, device=None) -> float:
    """PFLOP/s that a chip-wide, registers-only stream of v_mfma_f32_32x32x16_bf16 sustains on this device with `data` operands
    ("zeros" | "random" | "relu_like": half zeros, half uniform): the matrix pipe's own ceiling under the power cap
    (rpg_probe_mfma_bf16; measurement aid of bench.py's bf16 roofline).  Timed with events on the current stream."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    g = torch.Generator(device=dev).manual_seed(17)
    n = 65536 * 8
    if data == "zeros":
        v = torch.zeros(n, device=dev)
    elif data == "random":
        v = (torch.rand(n, generator=g, device=dev) - 0.5) * 2e-3
    elif data == "relu_like":
        v = torch.rand(n, generator=g, device=dev) * 2e-3 * (torch.rand(n, generator=g, device=dev) < 0.5)
    else:
        raise ValueError("data: zeros | random | relu_like")
    src = v.bfloat16().contiguous()
    sink = torch.zeros(1, device=dev)
    wgs = workgroups or 2 * torch.cuda.get_device_properties(dev).multi_processor_count
    lib = L.lib()
    L.check(lib.rpg_probe_mfma_bf16(_p(src), max(1, iters // 10), wgs, _p(sink), _stream()), "probe_mfma_bf16")      # warm (clock ramp)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    L.check(lib.rpg_probe_mfma_bf16(_p(src), iters, wgs, _p(sink), _stream()), "probe_mfma_bf16")
    e1.record()
    e1.synchronize()
    return wgs * 8 * iters * 16 * 32768.0 / (e0.elapsed_time(e1) * 1e-3) / 1e15


def f32_to_bf16(x: torch.Tensor, out: Optional[torch.Tensor] = None, col_off: int = 0) -> torch.Tensor:
    """bf16 image of the fp32 matrix x [rows][cols] (written at column col_off of `out` when given)."""
    x = _req(x, "x")
    rows, cols = x.shape
    if out is None:
        out = torch.empty((rows, cols), dtype=torch.bfloat16, device=x.device)
    out = _req(out, "out", torch.bfloat16)
    L.check(L.lib().rpg_f32_to_bf16(_p(x), cols, _p(out), out.shape[1], col_off, rows, cols, _stream()), "f32_to_bf16")
    return out


def _frames_axis_tables(axis: str, n_in: int, n_out: int, bounds, weights, dev) -> None:
    """The tables of one axis of a frame launch are ``resize_table(n_in, n_out)``'s, on ``dev``, in shape and type; None where
    the size does not change.  The kernel indexes them by the sizes alone, so anything else is refused here (ValueError)."""
    if n_in == n_out:
        if bounds is not None or weights is not None:
            raise ValueError(f"frames: the {axis} size does not change ({n_in}), so its tables must be None")
        return
    ks = L.lib().rpg_resize_table_ksize(int(n_in), int(n_out))
    if ks <= 0:
        raise ValueError(f"frames: unsupported {axis} sizes {n_in} -> {n_out}")
    for name, t, shape in (("bounds", bounds, (n_out, 2)), ("weights", weights, (n_out, ks))):
        if (not torch.is_tensor(t) or t.dtype != torch.int32 or tuple(t.shape) != shape or not t.is_contiguous()
                or t.device != dev):
            got = f"{t.dtype} {list(t.shape)} on {t.device}" if torch.is_tensor(t) else type(t).__name__
            raise ValueError(f"frames: the {axis} {name} of {n_in} -> {n_out} must be a contiguous int32 {list(shape)} tensor "
                             f"on the frames' GPU (resize_table), got {got}")


def _frames(frames: torch.Tensor, out_hw: Tuple[int, int], tables, mean: Sequence[float], std: Sequence[float],
            dtype, out: Optional[torch.Tensor]) -> torch.Tensor:
    frames = _req(frames, "frames", torch.uint8)
    if frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError(f"frames: expected uint8 [n, H, W, 3] (RGB, HWC), got {tuple(frames.shape)}")
    n, h, w, _ = frames.shape
    oh, ow = int(out_hw[0]), int(out_hw[1])
    hb, hw, vb, vw = tables
    _frames_axis_tables("horizontal", w, ow, hb, hw, frames.device)
    _frames_axis_tables("vertical", h, oh, vb, vw, frames.device)
    out = _out(out, (n, 3, oh, ow), dtype, frames.device, "frames")
    fn = L.lib().rpg_frames_u8_to_bf16 if dtype == torch.bfloat16 else L.lib().rpg_frames_u8_to_f32
    L.check(fn(_p(frames), n, h, w, oh, ow, _p(hb), _p(hw), _p(vb), _p(vw), *[float(v) for v in mean], *[float(v) for v in std],
               _p(out), None, 0, _stream()), "frames_u8")
    return out


def frames_u8_to_f32(frames: torch.Tensor, out_hw: Tuple[int, int], tables, mean: Sequence[float], std: Sequence[float],
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 RGB frames [n, H, W, 3] -> fp32 [n, 3, out_h, out_w]: Pillow's bilinear resize + ToTensor + Normalize, bit for bit.
    ``tables`` = (h_bounds, h_weights, v_bounds, v_weights) int32 device tensors of ``resize_table`` (None for an axis whose size
    does not change); ``mean`` / ``std`` three floats each (frames.FrameTransform builds and caches all of it)."""
    return _frames(frames, out_hw, tables, mean, std, torch.float32, out)


def frames_u8_to_bf16(frames: torch.Tensor, out_hw: Tuple[int, int], tables, mean: Sequence[float], std: Sequence[float],
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """As ``frames_u8_to_f32``, rounded to bf16 (nearest even): the bf16 encoder's rounding of the fp32 result."""
    return _frames(frames, out_hw, tables, mean, std, torch.bfloat16, out)


def _frames_scenes(frames, out_hw, tables, scene_stats, frame_scene, dtype, status, out) -> torch.Tensor:
    frames = _req(frames, "frames", torch.uint8)
    if frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError(f"frames: expected uint8 [n, H, W, 3] (RGB, HWC), got {tuple(frames.shape)}")
    n, h, w, _ = frames.shape
    oh, ow = int(out_hw[0]), int(out_hw[1])
    hb, hw, vb, vw = tables
    _frames_axis_tables("horizontal", w, ow, hb, hw, frames.device)
    _frames_axis_tables("vertical", h, oh, vb, vw, frames.device)
    stats, scene = _req(scene_stats, "scene_stats"), _req(frame_scene, "frame_scene", torch.int32)
    if stats.dim() != 2 or stats.shape[0] < 1 or stats.shape[1] != 6 or stats.device != frames.device:
        raise ValueError(f"frames: scene_stats must be fp32 [S >= 1, 6] (mean[3], std[3]) on the frames' GPU, got {tuple(stats.shape)}")
    if tuple(scene.shape) != (n,) or scene.device != frames.device:
        raise ValueError(f"frames: frame_scene must be int32 [{n}] on the frames' GPU, got {tuple(scene.shape)}")
    out = _out(out, (n, 3, oh, ow), dtype, frames.device, "frames")
    status, own = _status_arg(status, frames.device, "frames")
    fn = L.lib().rpg_frames_u8_to_bf16_scenes if dtype == torch.bfloat16 else L.lib().rpg_frames_u8_to_f32_scenes
    L.check(fn(_p(frames), n, h, w, oh, ow, _p(hb), _p(hw), _p(vb), _p(vw), _p(stats), _p(scene), stats.shape[0], status.data_ptr(),
               _p(out), None, 0, _stream()), "frames_u8_scenes")
    bad = _own_count(status, own)
    if bad:
        raise IndexError(f"frame_scene has {bad} entry(ies) outside the statistics' scenes [0, {stats.shape[0]})")
    return out


def frames_u8_to_f32_scenes(frames: torch.Tensor, out_hw: Tuple[int, int], tables, scene_stats: torch.Tensor,
                            frame_scene: torch.Tensor, status: Optional[torch.Tensor] = None,
                            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``frames_u8_to_f32`` with the statistics per frame (rpg_frames_u8_to_f32_scenes): ``scene_stats`` fp32 [S, 6] = mean[3],
    std[3] per scene and ``frame_scene`` int32 [n], both on the frames' GPU.  A scene outside [0, S) is counted into ``status``
    (int32 device tensor, accumulates; the frame takes scene 0's statistics) -- with ``status=None`` the count is read back
    here (one synchronisation) and a non-zero count raises IndexError."""
    return _frames_scenes(frames, out_hw, tables, scene_stats, frame_scene, torch.float32, status, out)


def frames_u8_to_bf16_scenes(frames: torch.Tensor, out_hw: Tuple[int, int], tables, scene_stats: torch.Tensor,
                             frame_scene: torch.Tensor, status: Optional[torch.Tensor] = None,
                             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """As ``frames_u8_to_f32_scenes``, rounded to bf16 (nearest even)."""
    return _frames_scenes(frames, out_hw, tables, scene_stats, frame_scene, torch.bfloat16, status, out)


def resize_table(n_in: int, n_out: int):
    """HOST: Pillow's 8-bit bilinear table of one axis -> (bounds int32 [n_out, 2], weights int32 [n_out, ksize])."""
    lib = L.lib()
    ks = lib.rpg_resize_table_ksize(int(n_in), int(n_out))
    if ks <= 0:
        raise ValueError(f"resize_table: unsupported sizes {n_in} -> {n_out}")
    bounds = torch.empty((n_out, 2), dtype=torch.int32)
    weights = torch.empty((n_out, ks), dtype=torch.int32)
    rc = lib.rpg_resize_table_bilinear(int(n_in), int(n_out), bounds.data_ptr(), weights.data_ptr())
    if rc != ks:
        raise ValueError(f"resize_table: unsupported sizes {n_in} -> {n_out}")
    return bounds, weights


PLAN_FIELDS = ("tr", "tc", "tiles_y", "tiles_x", "rows_max", "pitch", "lds_bytes")


def frames_plan(in_h: int, in_w: int, out_h: int, out_w: int) -> Dict[str, object]:
    """HOST: the tile plan frames_u8_to_* launches this geometry with (rpg_frames_plan: the launcher's own planner): tile rows
    ``tr`` x columns ``tc``, ``tiles_y`` x ``tiles_x`` tiles per frame, ``rows_max`` staged source rows, ``pitch`` LDS bytes per
    staged row, ``lds_bytes`` per workgroup, and which passes run (``need_h``, ``need_v``).  ValueError for sizes the launch
    refuses."""
    raw = (C.c_int32 * 8)()
    if L.lib().rpg_frames_plan(int(in_h), int(in_w), int(out_h), int(out_w), raw) != 0:
        raise ValueError(f"frames_plan: unsupported sizes {in_h} x {in_w} -> {out_h} x {out_w}")
    plan: Dict[str, object] = {k: int(raw[i]) for i, k in enumerate(PLAN_FIELDS)}
    plan["need_h"], plan["need_v"] = bool(raw[7] & 1), bool(raw[7] & 2)
    return plan


def _linear_bf16_args(a, weight, bias, residual, res_idx, residual2, res2_idx, strided: bool = False):
    """The checked operands of linear_bf16 / linear_bf16_ex -> (a, weight, bias, residual, res_idx, residual2, res2_idx, m, k,
    n_out, the residuals' row pitch).  ``strided``: the optional tensors are taken as they are (dtype and device checked, never
    copied), so that ``residual2`` may be a view of ``residual``'s storage; the row pitch is then their stride."""
    a, weight = _req(a, "a", torch.bfloat16), _req(weight, "weight", torch.bfloat16)
    m, k = a.shape
    if weight.shape[1] != k:
        raise ValueError("a.shape[1] != weight.shape[1]")
    opt = ((bias, "bias", torch.float32), (residual, "residual", torch.float32), (residual2, "residual2", torch.float32),
           (res_idx, "res_idx", torch.int64), (res2_idx, "res2_idx", torch.int64))
    if strided:
        for t, nm, dt in opt:
            if t is not None and (t.dtype != dt or not t.is_cuda):
                raise TypeError(f"{nm}: expected {dt} on the GPU")
    else:
        bias, residual, residual2, res_idx, res2_idx = (_opt(t, nm, dt) for t, nm, dt in opt)
    pitch = (lambda t: t.stride(0)) if strided else (lambda t: t.shape[1])
    if residual2 is not None and (residual is None or pitch(residual2) != pitch(residual)):
        raise ValueError("residual2 needs residual with the same row pitch")
    return (a, weight, bias, residual, res_idx, residual2, res2_idx, m, k, weight.shape[0],
            0 if residual is None else pitch(residual))


def linear_bf16(a: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
                residual: Optional[torch.Tensor] = None, res_idx: Optional[torch.Tensor] = None,
                residual2: Optional[torch.Tensor] = None, res2_idx: Optional[torch.Tensor] = None, relu: bool = False) -> torch.Tensor:
    """out (fp32) = act(a (bf16) @ weight.T (bf16) + bias + residual[res_idx or arange] + residual2[res2_idx]); the
    residual matrices are fp32 with a common row pitch."""
    a, weight, bias, residual, res_idx, residual2, res2_idx, m, k, n_out, ldr = _linear_bf16_args(
        a, weight, bias, residual, res_idx, residual2, res2_idx)
    out = torch.empty((m, n_out), dtype=torch.float32, device=a.device)
    L.check(L.lib().rpg_linear_bf16(_p(a), _p(weight), _p(bias), _p(residual), _p(res_idx), _p(residual2), _p(res2_idx), ldr,
                                    _p(out), m, k, n_out, int(relu), _stream()), "linear_bf16")
    return out


def linear_bf16_ex(a: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
                   residual: Optional[torch.Tensor] = None, res_idx: Optional[torch.Tensor] = None,
                   residual2: Optional[torch.Tensor] = None, res2_idx: Optional[torch.Tensor] = None, relu: bool = False,
                   out_dtype: Optional[torch.dtype] = torch.float32, out2: bool = False, relu2: bool = False
                   ) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """linear_bf16 in its general form (rpg_linear_bf16_ex): primary output fp32 / bf16 / none (``out_dtype``), and with ``out2`` a
    second bf16 output = bf16(relu2 ? max(y, 0) : y), y taken before the primary's ReLU.  ``residual2`` may be a column-offset view
    of ``residual``'s storage (common row pitch)."""
    if out_dtype not in (torch.float32, torch.bfloat16, None) or (out_dtype is None and not out2):
        raise ValueError("out_dtype: float32 | bfloat16 | None (then out2 must be set)")
    a, weight, bias, residual, res_idx, residual2, res2_idx, m, k, n_out, ldr = _linear_bf16_args(
        a, weight, bias, residual, res_idx, residual2, res2_idx, strided=True)
    y = None if out_dtype is None else torch.empty((m, n_out), dtype=out_dtype, device=a.device)
    y2 = torch.empty((m, n_out), dtype=torch.bfloat16, device=a.device) if out2 else None
    L.check(L.lib().rpg_linear_bf16_ex(_p(a), k, _p(weight), _p(bias), _p(residual), _p(res_idx), _p(residual2), _p(res2_idx), ldr,
                                       _p(y), int(out_dtype == torch.float32), _p(y2), n_out if out2 else 0, int(relu2), m, k, n_out,
                                       int(relu), _stream()), "linear_bf16_ex")
    return y, y2


def conv_pair_bf16(x: torch.Tensor, wa_ohwi: torch.Tensor, scale_a: torch.Tensor, shift_a: torch.Tensor, wb_ohwi: torch.Tensor,
                   scale_b: torch.Tensor, shift_b: torch.Tensor, stride: int = 2, pad: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """(relu(bn_a(conv k x k / stride / pad (x))), bn_b(conv 1 x 1 / stride (x))) of a down-sampling BasicBlock in one launch
    (rpg_conv_pair_bf16); ValueError where the pair is not eligible."""
    x, wa_ohwi, wb_ohwi = _req(x, "x", torch.bfloat16), _req(wa_ohwi, "wa_ohwi", torch.bfloat16), _req(wb_ohwi, "wb_ohwi", torch.bfloat16)
    n, h, w, cin = x.shape
    cout, k, kw, cin_a = wa_ohwi.shape
    if k != kw or cin_a != cin or tuple(wb_ohwi.shape) != (cout, 1, 1, cin):
        raise ValueError("conv_pair_bf16: wa [cout,k,k,cin], wb [cout,1,1,cin]")
    ps = [_req(t, nm) for t, nm in ((scale_a, "scale_a"), (shift_a, "shift_a"), (scale_b, "scale_b"), (shift_b, "shift_b"))]
    if any(t.numel() != cout for t in ps):
        raise ValueError("conv_pair_bf16: scale / shift must have cout elements")
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    ya = torch.empty((n, ho, wo, cout), dtype=torch.bfloat16, device=x.device)
    yb = torch.empty_like(ya)
    L.check(L.lib().rpg_conv_pair_bf16(_p(x), _p(wa_ohwi), _p(ps[0]), _p(ps[1]), _p(ya), _p(wb_ohwi), _p(ps[2]), _p(ps[3]), _p(yb),
                                       n, h, w, cin, cout, k, stride, pad, _stream()), "conv_pair_bf16")
    return ya, yb


def stem_conv_bn_relu_maxpool(x_nchw: torch.Tensor, wpack: torch.Tensor, shift: torch.Tensor) -> torch.Tensor:
    """conv7x7/2 (3 -> 64) + BN + ReLU + maxpool3x3/2 in one kernel: [N,3,H,W] -> pooled NHWC [N,Hp,Wp,64]; wpack from
    params.pack_stem_pairs (BatchNorm scale folded in), shift [64]."""
    x, wpack, shift = _req(x_nchw, "x_nchw"), _req(wpack, "wpack"), _req(shift, "shift")
    n, c, h, w = x.shape
    if c != 3 or wpack.numel() != (74 + 75) * 2 * 64 or shift.numel() != 64:
        raise ValueError("expected x [N,3,H,W], wpack from params.pack_stem_pairs (19,072 floats), shift [64]")
    hc, wc = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    y = torch.empty((n, (hc - 1) // 2 + 1, (wc - 1) // 2 + 1, 64), dtype=torch.float32, device=x.device)
    L.check(L.lib().rpg_stem_conv7x7s2_bn_relu_maxpool_f32(_p(x), _p(wpack), _p(shift), _p(y), n, h, w, _stream()),
            "stem_conv_bn_relu_maxpool")
    return y


def stem_conv_bn_relu_maxpool_bf16(x_nchw: torch.Tensor, wpack_bf16: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor) -> torch.Tensor:
    """The bf16 encoder's stem in one kernel: fp32 [N,3,H,W] -> bf16 [N,Hp,Wp,64] (wpack_bf16 from params.pack_stem_bf16)."""
    xbf = x_nchw.dtype == torch.bfloat16
    x_nchw, scale, shift = _req(x_nchw, "x_nchw", torch.bfloat16 if xbf else torch.float32), _req(scale, "scale"), _req(shift, "shift")
    wpack_bf16 = _req(wpack_bf16, "wpack_bf16", torch.bfloat16)
    n, c, h, w = x_nchw.shape
    if c != 3 or wpack_bf16.numel() != (11 * 2 + 2 * 3 * 4) * 64 * 8 or scale.numel() != 64 or shift.numel() != 64:
        raise ValueError("expected x [N,3,H,W], wpack_bf16 from params.pack_stem_bf16 (23,552 bf16), scale / shift [64]")
    hc, wc = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    hp, wp = (hc - 1) // 2 + 1, (wc - 1) // 2 + 1
    y = torch.empty((n, hp, wp, 64), dtype=torch.bfloat16, device=x_nchw.device)
    fn = L.lib().rpg_stem_conv7x7s2_bn_relu_maxpool_bf16_xbf16 if xbf else L.lib().rpg_stem_conv7x7s2_bn_relu_maxpool_bf16
    L.check(fn(_p(x_nchw), _p(wpack_bf16), _p(scale), _p(shift), _p(y), n, h, w, _stream()), "stem_conv_bn_relu_maxpool_bf16")
    return y


def maxpool3x3s2_nhwc(x: torch.Tensor) -> torch.Tensor:
    x = _req(x, "x")
    n, h, w, c = x.shape
    y = torch.empty((n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c), dtype=torch.float32, device=x.device)
    L.check(L.lib().rpg_maxpool3x3s2_nhwc_f32(_p(x), _p(y), n, h, w, c, _stream()), "maxpool3x3s2_nhwc")
    return y


def global_avgpool_nhwc(x: torch.Tensor) -> torch.Tensor:
    x = _req(x, "x")
    n, h, w, c = x.shape
    y = torch.empty((n, c), dtype=torch.float32, device=x.device)
    L.check(L.lib().rpg_global_avgpool_nhwc_f32(_p(x), _p(y), n, h * w, c, _stream()), "global_avgpool_nhwc")
    return y


def graph_prepare(edge_index: torch.Tensor, n: int) -> Dict[str, torch.Tensor]:
    ei = _req(edge_index, "edge_index", torch.int64)
    if ei.dim() != 2 or ei.shape[0] != 2:
        raise ValueError("edge_index must be [2, E]")
    e = ei.shape[1]
    dev = ei.device
    ends = torch.empty((4, e), dtype=torch.int64, device=dev)
    rowptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
    cursor = torch.empty(n, dtype=torch.int32, device=dev)
    perm = torch.empty(e, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    L.check(L.lib().rpg_graph_prepare(ei.data_ptr(), ei.data_ptr() + 8 * e, 0, e, n, _p(ends), _p(rowptr), _p(cursor), _p(perm),
                                      _p(status), _stream()), "graph_prepare")
    return {"ends": ends, "rowptr": rowptr, "perm": perm, "status": status}


def knn_graph_launch(x: torch.Tensor, k: int, batch: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Enqueue the kNN graph build on the current stream WITHOUT synchronising: returns (edge buffer [2, n*(k+1)] int64,
    meta int32 [2] = (E, graphs-too-large flag), both on the device).  The first E columns of the buffer are the edges once
    the stream has run; knn_graph() below reads E right away, PoseNetX_R2's multi-stream path reads it behind an event."""
    x = _req(x, "x")
    n, d = x.shape
    batch = _opt(batch, "batch", torch.int64)
    cap = n * (k + 1)
    ei = torch.empty((2, cap), dtype=torch.int64, device=x.device)
    cand = torch.empty((n, k + 1), dtype=torch.int32, device=x.device)
    cnt = torch.empty(n, dtype=torch.int32, device=x.device)
    meta = torch.zeros(2, dtype=torch.int32, device=x.device)
    L.check(L.lib().rpg_knn_graph_f32(_p(x), _p(batch), n, d, k, _p(ei), _p(cand), _p(cnt), meta.data_ptr(),
                                      meta.data_ptr() + 4, _stream()), "knn_graph")
    return ei, meta


def knn_graph(x: torch.Tensor, k: int, batch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """torch_cluster.knn_graph(x, k, batch, loop=False): [2, E] int64, row 0 = neighbour, row 1 = query node.
    Synchronises once to learn E (E = n*k unless a graph has fewer than k+1 nodes or duplicate rows)."""
    ei, meta = knn_graph_launch(x, k, batch)
    total, bad = (int(v) for v in meta.tolist())
    if bad:
        raise ValueError("knn_graph: a graph has more than 2048 nodes (unsupported)")
    return ei[:, :total].contiguous()


def _edge_rows(out, cols: int, dev, what: str):
    """``out`` of knn_graph_uniform: None (allocated, [2, cols]), an int64 [2, cols] tensor, or a pair of int64 [cols] tensors
    (two row slices of a larger list) -- every row contiguous, on ``dev``.  -> (what to return, source row, target row)."""
    if out is None:
        out = torch.empty((2, cols), dtype=torch.int64, device=dev)
    if len(out) != 2:
        raise ValueError(f"{what} must be an int64 [2, {cols}] tensor or a pair of int64 [{cols}] tensors")
    for row in (out[0], out[1]):
        if (not torch.is_tensor(row) or row.dtype != torch.int64 or row.device != dev or tuple(row.shape) != (cols,)
                or not row.is_contiguous()):
            raise ValueError(f"{what} must be an int64 [2, {cols}] tensor or a pair of int64 [{cols}] tensors, rows contiguous, on "
                             f"the inputs' GPU")
    return out, out[0], out[1]


def knn_graph_uniform(x: torch.Tensor, g: int, n_per: int, k: int, node_offset: int = 0, out=None, q_out=None,
                      irregular: Optional[torch.Tensor] = None):
    """knn_graph over ``g`` graphs of ``n_per`` nodes each (x [g * n_per, d]) with every column at a fixed position
    (rpg_knn_graph_uniform_f32): k' = min(k, n_per - 1), column v k' + t = (t-th nearest other node of v, v), both plus
    ``node_offset`` -- knn_graph's neighbours in knn_graph's order, but nothing for the host to wait for.  ``out``: where the list
    goes (int64 [2, g n_per k'] or a pair of rows; allocated if None); ``q_out``: likewise [2, g k'] for the columns into node 0 of
    every graph, ``True`` allocates them, None leaves them out; ``irregular``: int32 counter, += the nodes whose reference
    in-degree is k' + 1 (their list here is its first k' entries; see the header), a zeroed one of this call's own if None.
    -> (out, q_out or None, irregular); nothing synchronises."""
    x = _req(x, "x")
    g, n_per, k = int(g), int(n_per), int(k)
    if x.dim() != 2 or g < 1 or n_per < 2 or k < 1 or x.shape[0] != g * n_per:
        raise ValueError(f"knn_graph_uniform: x must be [g * n_per, d] with g >= 1 graphs of n_per >= 2 nodes and k >= 1, got "
                         f"{tuple(x.shape)} for g = {g}, n_per = {n_per}, k = {k}")
    kp = min(k, n_per - 1)
    dev = x.device
    out, src, dst = _edge_rows(out, g * n_per * kp, dev, "knn_graph_uniform: out")
    q_src = q_dst = None
    if q_out is not None:
        q_out, q_src, q_dst = _edge_rows(None if q_out is True else q_out, g * kp, dev, "knn_graph_uniform: q_out")
    irregular, _ = _status_arg(irregular, dev, "knn_graph_uniform")
    L.check(L.lib().rpg_knn_graph_uniform_f32(_p(x), g, n_per, x.shape[1], k, int(node_offset), _p(src), _p(dst), _p(q_src),
                                              _p(q_dst), _p(irregular), _stream()), "knn_graph_uniform")
    return out, q_out, irregular


def edge_concat_gather(x: torch.Tensor, edge_index: torch.Tensor) -> torch.Tensor:
    x, ei = _req(x, "x"), _req(edge_index, "edge_index", torch.int64)
    e, d = ei.shape[1], x.shape[1]
    out = torch.empty((e, 2 * d), dtype=torch.float32, device=x.device)
    L.check(L.lib().rpg_edge_concat_gather_f32(_p(x), _p(ei), e, d, _p(out), _stream()), "edge_concat_gather")
    return out


def gather_add2_relu(pq: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """relu((pq[lo][:, :d] + pq[hi][:, d:]) + bias) (rpg_gather_add2_relu_f32; proj_edge on per-node products): pq [rows, 2d],
    lo / hi int64 [E] row ids (checked here against ``rows``: one synchronisation), bias [d] -> [E, d]."""
    pq, bias = _req(pq, "pq"), _req(bias, "bias")
    lo, hi = _req(lo, "lo", torch.int64), _req(hi, "hi", torch.int64)
    if pq.dim() != 2 or pq.shape[1] % 8 or lo.dim() != 1 or lo.shape != hi.shape or bias.shape != (pq.shape[1] // 2,):
        raise ValueError(f"gather_add2_relu: needs pq [rows, 2d] with d % 4 == 0, lo / hi [E] and bias [d], got "
                         f"{tuple(pq.shape)}, {tuple(lo.shape)}, {tuple(hi.shape)}, {tuple(bias.shape)}")
    rows, e, d = pq.shape[0], lo.shape[0], pq.shape[1] // 2
    if e and (int(torch.minimum(lo.min(), hi.min())) < 0 or int(torch.maximum(lo.max(), hi.max())) >= rows):
        raise IndexError(f"gather_add2_relu: lo / hi hold a row id outside [0, {rows})")
    out = torch.empty((e, d), dtype=torch.float32, device=pq.device)
    L.check(L.lib().rpg_gather_add2_relu_f32(_p(pq), _p(lo), _p(hi), _p(bias), e, d, _p(out), _stream()), "gather_add2_relu")
    return out


def gather_graph_nodes(query_feat: torch.Tensor, map_feat: torch.Tensor, neighbours: torch.Tensor,
                       out: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Node features of G graphs, each its query followed by K map rows (rpg_gather_graph_nodes_f32): query_feat [G, d],
    map_feat [M, d], neighbours int64 [G, K] -> [G*(K+1), d].  A neighbour outside [0, M) is counted into ``status`` (int32
    device tensor, accumulates; its row is clamped) -- with ``status=None`` the count is read back here (one synchronisation)
    and a non-zero count raises IndexError."""
    q, mp, nb = _req(query_feat, "query_feat"), _req(map_feat, "map_feat"), _req(neighbours, "neighbours", torch.int64)
    if q.dim() != 2 or mp.dim() != 2 or nb.dim() != 2:
        raise ValueError("gather_graph_nodes: query_feat [G, d], map_feat [M, d] and neighbours [G, K] must be 2-D")
    (g, d), (m, dm), (gn, k) = q.shape, mp.shape, nb.shape
    if dm != d or gn != g:
        raise ValueError(f"gather_graph_nodes: shapes do not agree: query_feat {tuple(q.shape)}, map_feat {tuple(mp.shape)}, "
                         f"neighbours {tuple(nb.shape)}")
    if g == 0 or k == 0 or m == 0 or d % 4:
        raise ValueError(f"gather_graph_nodes: needs G >= 1, K >= 1, M >= 1 and d % 4 == 0 (G={g}, K={k}, M={m}, d={d})")
    if mp.device != q.device or nb.device != q.device:
        raise RuntimeError("gather_graph_nodes: query_feat, map_feat and neighbours must be on the same GPU")
    out = _out(out, (g * (k + 1), d), torch.float32, q.device, "gather_graph_nodes")
    status, own = _status_arg(status, q.device, "gather_graph_nodes")
    L.check(L.lib().rpg_gather_graph_nodes_f32(_p(q), _p(mp), _p(nb), g, k, m, d, _p(out), status.data_ptr(), _stream()),
            "gather_graph_nodes")
    bad = _own_count(status, own)
    if bad:
        raise IndexError(f"neighbours has {bad} index(es) outside the map's rows [0, {m})")
    return out


def row_inv_norms(x: torch.Tensor) -> torch.Tensor:
    """1 / |x_r| per row of x [M, d] (rpg_row_inv_norms_f32; 0 for a zero row): what ``retrieve`` takes as ``db_inv_norm``."""
    x = _req(x, "x")
    if x.dim() != 2 or x.shape[0] == 0 or x.shape[1] == 0 or x.shape[1] % 4:
        raise ValueError(f"row_inv_norms: needs x [M >= 1, d] with d % 4 == 0, got {tuple(x.shape)}")
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    L.check(L.lib().rpg_row_inv_norms_f32(_p(x), x.shape[0], x.shape[1], _p(out), _stream()), "row_inv_norms")
    return out


def retrieve(q: torch.Tensor, db: torch.Tensor, ranks, db_inv_norm: Optional[torch.Tensor] = None,
             q_group: Optional[torch.Tensor] = None, db_group: Optional[torch.Tensor] = None, return_sims: bool = False,
             status: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
             out: Optional[torch.Tensor] = None):
    """Per query the database rows at positions ``ranks[g]`` of its ranking (rpg_retrieve_cosine_f32): q [G, d], db [M, d] fp32,
    ranks int32 [G, K] (a tensor on the GPU, or host integers), strictly ascending per query -> neighbours int64 [G, K] (and
    their similarities [G, K] with ``return_sims``).  Row m is skipped for query g when ``db_group[m] == q_group[g]`` (int64
    [M] / [G]; both or neither; ``q_group[g] == -1`` skips nothing).  A rank outside query g's allowed rows or the kernel's
    ``R_MAX``, or a row of ranks that does not ascend, is counted into ``status`` (int32 device tensor, accumulates; the rank
    is clamped) -- with ``status=None`` the count is read back here (one synchronisation) and a non-zero count raises
    IndexError.  ``workspace``: a uint8 device tensor to use instead of allocating one; ``out``: the neighbours' tensor."""
    return _retrieve(q, db, ranks, db_inv_norm, q_group, db_group, return_sims, status, workspace, out, None)


def retrieve_gated(q: torch.Tensor, db: torch.Tensor, ranks, db_gate: torch.Tensor, prior: torch.Tensor, r2: float,
                   cos_half: float = 0.0, rot_gate: bool = False, db_inv_norm: Optional[torch.Tensor] = None,
                   q_group: Optional[torch.Tensor] = None, db_group: Optional[torch.Tensor] = None, return_sims: bool = False,
                   status: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None, gate_info: Optional[torch.Tensor] = None):
    """``retrieve`` restricted to the map rows near a prior pose (rpg_retrieve_cosine_gated_f32): ``db_gate`` float64 [M, 7] and
    ``prior`` float64 [G, 7] hold (t[3], q[4]), the un-normalised translation and the unit quaternion.  Per query: a non-finite
    prior ranks as ``retrieve`` does (state 1); otherwise the allowed rows with squared distance <= ``r2`` (and, with
    ``rot_gate``, ``|<q_row, q_prior>| >= cos_half``) are the only ones ranked (state 0) when they cover the query's largest
    rank, and all allowed rows are (state 2) when they do not.  -> (neighbours [, sims], gate_info int32 [G, 2] = (state, allowed
    rows inside)); ``gate_info``: the tensor to write them to.  Everything else as ``retrieve``."""
    dbg, pr = _req(db_gate, "db_gate", torch.float64), _req(prior, "prior", torch.float64)
    if not torch.is_tensor(q) or not torch.is_tensor(db) or q.dim() != 2 or db.dim() != 2:
        raise ValueError("retrieve_gated: q [G, d] and db [M, d] must be 2-D tensors")
    g, m = q.shape[0], db.shape[0]
    if tuple(dbg.shape) != (m, 7) or tuple(pr.shape) != (g, 7) or dbg.device != q.device or pr.device != q.device:
        raise ValueError(f"retrieve_gated: db_gate must be float64 [{m}, 7] and prior float64 [{g}, 7] on the inputs' GPU, got "
                         f"{tuple(dbg.shape)} and {tuple(pr.shape)}")
    r2, cos_half = float(r2), float(cos_half)
    if not r2 >= 0.0 or cos_half != cos_half:
        raise ValueError(f"retrieve_gated: r2 must be >= 0 and cos_half a number, got {r2} and {cos_half}")
    info = _out(gate_info, (g, 2), torch.int32, q.device, "retrieve_gated")
    res = _retrieve(q, db, ranks, db_inv_norm, q_group, db_group, return_sims, status, workspace, out,
                    (dbg, pr, r2, cos_half, int(bool(rot_gate)), info))
    return (*res, info) if return_sims else (res, info)


def retrieve_scoped(q: torch.Tensor, db: torch.Tensor, ranks, scene_first: Optional[torch.Tensor],
                    q_scene: Optional[torch.Tensor], db_gate: Optional[torch.Tensor] = None,
                    prior: Optional[torch.Tensor] = None, r2: float = 0.0, cos_half: float = 0.0, rot_gate: bool = False,
                    db_inv_norm: Optional[torch.Tensor] = None, q_group: Optional[torch.Tensor] = None,
                    db_group: Optional[torch.Tensor] = None, return_sims: bool = False, status: Optional[torch.Tensor] = None,
                    workspace: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                    gate_info: Optional[torch.Tensor] = None):
    """``retrieve`` / ``retrieve_gated`` on a map of several scenes (rpg_retrieve_cosine_scoped_f32): ``scene_first`` int64
    [S + 1] (scene s owns rows [scene_first[s], scene_first[s + 1])) and ``q_scene`` int32 [G], on the inputs' GPU; query g ranks
    its scene's rows only, exactly as if the rows outside were of its group.  A ``q_scene`` outside [0, S) counts 1 into
    ``status`` and ranks nothing (row 0).  Both None: the gated entry itself.  ``db_gate`` and ``prior`` (both or neither)
    gate as ``retrieve_gated`` does; then -> (neighbours [, sims], gate_info), otherwise neighbours [, sims]."""
    if (scene_first is None) != (q_scene is None):
        raise ValueError("retrieve_scoped: scene_first and q_scene go together (both or neither)")
    if (db_gate is None) != (prior is None):
        raise ValueError("retrieve_scoped: db_gate and prior go together (both or neither)")
    if not torch.is_tensor(q) or not torch.is_tensor(db) or q.dim() != 2 or db.dim() != 2:
        raise ValueError("retrieve_scoped: q [G, d] and db [M, d] must be 2-D tensors")
    g, m = q.shape[0], db.shape[0]
    scope = None
    if scene_first is not None:
        first, qs = _req(scene_first, "scene_first", torch.int64), _req(q_scene, "q_scene", torch.int32)
        if first.dim() != 1 or first.shape[0] < 2 or tuple(qs.shape) != (g,) or first.device != q.device or qs.device != q.device:
            raise ValueError(f"retrieve_scoped: scene_first must be int64 [S + 1 >= 2] and q_scene int32 [{g}] on the inputs' GPU, "
                             f"got {tuple(first.shape)} and {tuple(qs.shape)}")
        scope = (first, qs, first.shape[0] - 1)
    gate = None
    if db_gate is not None:
        dbg, pr = _req(db_gate, "db_gate", torch.float64), _req(prior, "prior", torch.float64)
        if tuple(dbg.shape) != (m, 7) or tuple(pr.shape) != (g, 7) or dbg.device != q.device or pr.device != q.device:
            raise ValueError(f"retrieve_scoped: db_gate must be float64 [{m}, 7] and prior float64 [{g}, 7] on the inputs' GPU, got "
                             f"{tuple(dbg.shape)} and {tuple(pr.shape)}")
        r2, cos_half = float(r2), float(cos_half)
        if not r2 >= 0.0 or cos_half != cos_half:
            raise ValueError(f"retrieve_scoped: r2 must be >= 0 and cos_half a number, got {r2} and {cos_half}")
        gate = (dbg, pr, r2, cos_half, int(bool(rot_gate)), _out(gate_info, (g, 2), torch.int32, q.device, "retrieve_scoped"))
    elif gate_info is not None:
        raise ValueError("retrieve_scoped: gate_info is an output of gated retrieval: pass db_gate and prior")
    res = _retrieve(q, db, ranks, db_inv_norm, q_group, db_group, return_sims, status, workspace, out, gate, scope, True)
    if gate is None:
        return res
    return (*res, gate[5]) if return_sims else (res, gate[5])


def retrieve_elect(q: torch.Tensor, db: torch.Tensor, ranks, scene_first: torch.Tensor, top: int = 16,
                   q_scene: Optional[torch.Tensor] = None, lost_only: bool = False, db_gate: Optional[torch.Tensor] = None,
                   prior: Optional[torch.Tensor] = None, r2: float = 0.0, cos_half: float = 0.0, rot_gate: bool = False,
                   db_inv_norm: Optional[torch.Tensor] = None, q_group: Optional[torch.Tensor] = None,
                   db_group: Optional[torch.Tensor] = None, return_sims: bool = False, status: Optional[torch.Tensor] = None,
                   workspace: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                   gate_info: Optional[torch.Tensor] = None, scene_info: Optional[torch.Tensor] = None):
    """``retrieve_scoped`` for queries that are not told their scene (rpg_retrieve_cosine_elect_f32): the ``top`` (1 .. 64, at
    most M) most similar rows of the whole map -- ``retrieve(q, db, ranks=arange(top))`` without groups -- vote for the scene
    that owns them, the scene with the most votes (among tied ones the best-placed voter's) is elected, and the query is ranked
    inside it bit for bit as ``retrieve_scoped`` ranks it there.  ``lost_only=False``: every query elects; ``q_scene`` int32 [G]
    (made here when None) is an output.  ``lost_only=True``: ``q_scene`` is required, in and out: query g elects when
    ``q_scene[g] == -1`` or, with a gate, when ``prior[g]`` is not finite, and is otherwise held in ``q_scene[g]``; elected entries
    are overwritten.  -> (neighbours [, sims] [, gate_info], q_scene, scene_info), ``scene_info`` int32 [G, 2] = (elected scene,
    its votes), (held scene, 0) for a held query, -1 when no row voted.  ``workspace``: at least
    rpg_retrieve_elect_workspace_bytes(G, M, d) bytes.  Everything else as ``retrieve_scoped``."""
    if (db_gate is None) != (prior is None):
        raise ValueError("retrieve_elect: db_gate and prior go together (both or neither)")
    if not torch.is_tensor(q) or not torch.is_tensor(db) or q.dim() != 2 or db.dim() != 2:
        raise ValueError("retrieve_elect: q [G, d] and db [M, d] must be 2-D tensors")
    g, m = q.shape[0], db.shape[0]
    top = int(top)
    if not 1 <= top <= 64 or top > m:
        raise ValueError(f"retrieve_elect: top must be in [1, 64] and at most the map's {m} rows, got {top}")
    first = _req(scene_first, "scene_first", torch.int64)
    if first.dim() != 1 or first.shape[0] < 2 or first.device != q.device:
        raise ValueError(f"retrieve_elect: scene_first must be int64 [S + 1 >= 2] on the inputs' GPU, got {tuple(first.shape)}")
    if q_scene is None:
        if lost_only:
            raise ValueError("retrieve_elect: lost_only reads q_scene (-1: elect): pass it")
        q_scene = torch.empty(g, dtype=torch.int32, device=q.device)
    qs = _req(q_scene, "q_scene", torch.int32)
    if tuple(qs.shape) != (g,) or qs.device != q.device or qs is not q_scene:       # (written in place: no contiguous copy)
        raise ValueError(f"retrieve_elect: q_scene must be a contiguous int32 [{g}] on the inputs' GPU, got {tuple(qs.shape)}")
    gate = None
    if db_gate is not None:
        dbg, pr = _req(db_gate, "db_gate", torch.float64), _req(prior, "prior", torch.float64)
        if tuple(dbg.shape) != (m, 7) or tuple(pr.shape) != (g, 7) or dbg.device != q.device or pr.device != q.device:
            raise ValueError(f"retrieve_elect: db_gate must be float64 [{m}, 7] and prior float64 [{g}, 7] on the inputs' GPU, got "
                             f"{tuple(dbg.shape)} and {tuple(pr.shape)}")
        r2, cos_half = float(r2), float(cos_half)
        if not r2 >= 0.0 or cos_half != cos_half:
            raise ValueError(f"retrieve_elect: r2 must be >= 0 and cos_half a number, got {r2} and {cos_half}")
        gate = (dbg, pr, r2, cos_half, int(bool(rot_gate)), _out(gate_info, (g, 2), torch.int32, q.device, "retrieve_elect"))
    elif gate_info is not None:
        raise ValueError("retrieve_elect: gate_info is an output of gated retrieval: pass db_gate and prior")
    info = _out(scene_info, (g, 2), torch.int32, q.device, "retrieve_elect")
    res = _retrieve(q, db, ranks, db_inv_norm, q_group, db_group, return_sims, status, workspace, out, gate,
                    (first, qs, first.shape[0] - 1), True, (top, 2 if lost_only else 1, info))
    res = res if return_sims else (res,)
    return (*res, qs, info) if gate is None else (*res, gate[5], qs, info)


def _retrieve(q, db, ranks, db_inv_norm, q_group, db_group, return_sims, status, workspace, out, gate, scope=None, scoped=False,
              elect=None):
    """``retrieve`` / ``retrieve_gated`` / ``retrieve_scoped`` / ``retrieve_elect``: ``gate`` = None, or (db_gate, prior, r2,
    cos_half, rot_gate, gate_info) checked; ``scope`` = None, or (scene_first, q_scene, n_scenes) checked; ``scoped``: through the
    scoped entry; ``elect`` = None, or (top, mode, scene_info) checked: through the electing entry (with a scope)."""
    q, db = _req(q, "q"), _req(db, "db")
    if q.dim() != 2 or db.dim() != 2:
        raise ValueError("retrieve: q [G, d] and db [M, d] must be 2-D")
    (g, d), (m, dm) = q.shape, db.shape
    if dm != d:
        raise ValueError(f"retrieve: shapes do not agree: q {tuple(q.shape)}, db {tuple(db.shape)}")
    if db.device != q.device:
        raise RuntimeError("retrieve: q and db must be on the same GPU")
    if not torch.is_tensor(ranks):
        ranks = torch.as_tensor(ranks, dtype=torch.int32).to(q.device)
    ranks = _req(ranks, "ranks", torch.int32)
    if ranks.dim() != 2 or ranks.shape[0] != g or ranks.device != q.device:
        raise ValueError(f"retrieve: ranks must be int32 [G = {g}, K] on the inputs' GPU, got {tuple(ranks.shape)}")
    k = ranks.shape[1]
    if g == 0 or not 1 <= k <= 64 or m < k or m >= 1 << 31 or d == 0 or d % 4:
        raise ValueError(f"retrieve: needs G >= 1, 1 <= K <= 64, K <= M < 2^31 and d % 4 == 0 (G={g}, K={k}, M={m}, d={d})")
    if (q_group is None) != (db_group is None):
        raise ValueError("retrieve: q_group and db_group go together (both or neither)")
    if q_group is not None:
        q_group, db_group = _req(q_group, "q_group", torch.int64), _req(db_group, "db_group", torch.int64)
        if q_group.shape != (g,) or db_group.shape != (m,) or q_group.device != q.device or db_group.device != q.device:
            raise ValueError(f"retrieve: q_group must be int64 [{g}] and db_group int64 [{m}] on the inputs' GPU")
    if db_inv_norm is not None:
        db_inv_norm = _req(db_inv_norm, "db_inv_norm")
        if db_inv_norm.shape != (m,) or db_inv_norm.device != q.device:
            raise ValueError(f"retrieve: db_inv_norm must be fp32 [{m}] on the inputs' GPU")
    lib = L.lib()
    need = int((lib.rpg_retrieve_workspace_bytes if elect is None else lib.rpg_retrieve_elect_workspace_bytes)(g, m, d))
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=q.device)
    elif workspace.dtype != torch.uint8 or workspace.device != q.device or not workspace.is_contiguous():
        raise ValueError("retrieve: workspace must be a contiguous uint8 tensor on the inputs' GPU")
    nbrs = _out(out, (g, k), torch.int64, q.device, "retrieve")
    sims = torch.empty((g, k), dtype=torch.float32, device=q.device) if return_sims else None
    status, own = _status_arg(status, q.device, "retrieve")
    if elect is not None:
        dbg, pr, r2, cos_half, rot, info = gate if gate is not None else (None, None, 0.0, 0.0, 0, None)
        first, qs, ns = scope
        L.check(lib.rpg_retrieve_cosine_elect_f32(_p(q), _p(db), _p(db_inv_norm), _p(q_group), _p(db_group), _p(ranks), g, k, m, d,
                                                  _p(dbg), _p(pr), r2, cos_half, rot, _p(info), _p(first), _p(qs), ns, elect[0],
                                                  elect[1], _p(elect[2]), _p(nbrs), _p(sims), workspace.data_ptr(),
                                                  workspace.numel(), status.data_ptr(), _stream()), "retrieve_elect")
    elif scoped:
        dbg, pr, r2, cos_half, rot, info = gate if gate is not None else (None, None, 0.0, 0.0, 0, None)
        first, qs, ns = scope if scope is not None else (None, None, 0)
        L.check(lib.rpg_retrieve_cosine_scoped_f32(_p(q), _p(db), _p(db_inv_norm), _p(q_group), _p(db_group), _p(ranks), g, k, m, d,
                                                   _p(dbg), _p(pr), r2, cos_half, rot, _p(info), _p(first), _p(qs), ns, _p(nbrs),
                                                   _p(sims), workspace.data_ptr(), workspace.numel(), status.data_ptr(), _stream()),
                "retrieve_scoped")
    elif gate is None:
        L.check(lib.rpg_retrieve_cosine_f32(_p(q), _p(db), _p(db_inv_norm), _p(q_group), _p(db_group), _p(ranks), g, k, m, d,
                                            _p(nbrs), _p(sims), workspace.data_ptr(), workspace.numel(), status.data_ptr(),
                                            _stream()), "retrieve")
    else:
        dbg, pr, r2, cos_half, rot, info = gate
        L.check(lib.rpg_retrieve_cosine_gated_f32(_p(q), _p(db), _p(db_inv_norm), _p(q_group), _p(db_group), _p(ranks), g, k, m, d,
                                                  _p(dbg), _p(pr), r2, cos_half, rot, _p(info), _p(nbrs), _p(sims),
                                                  workspace.data_ptr(), workspace.numel(), status.data_ptr(), _stream()),
                "retrieve_gated")
    bad = _own_count(status, own)
    if bad:
        raise IndexError(f"ranks has {bad} entry(ies) outside a query's allowed rows / the kernel's R_MAX, or rows that do "
                         "not ascend" + (", or q_scene has entries outside the scenes" if scope is not None else ""))
    return (nbrs, sims) if return_sims else nbrs


def _qp_tensor(t, name: str, dtype, shape, who: str = "query_pose") -> torch.Tensor:
    """Host-side check of one ``query_pose`` / ``query_pose_fused`` argument: TypeError for a non-tensor / wrong dtype, ValueError
    for a wrong shape (``shape``: ints, or None for an axis that is free)."""
    if not torch.is_tensor(t):
        raise TypeError(f"{who}: {name} must be a tensor, got {type(t).__name__}")
    if t.dtype != dtype:
        raise TypeError(f"{who}: {name} must be {dtype}, got {t.dtype}")
    if t.dim() != len(shape) or any(s is not None and int(d) != s for d, s in zip(t.shape, shape)):
        want = ", ".join("*" if s is None else str(s) for s in shape)
        raise ValueError(f"{who}: {name} must be [{want}], got {tuple(t.shape)}")
    return t


def _qp_ref_node(v) -> int:
    if isinstance(v, bool) or not isinstance(v, numbers.Integral):
        raise TypeError(f"query_pose: ref_node must be an int, got {type(v).__name__}")
    if v < 0:
        raise ValueError(f"query_pose: ref_node must be >= 0, got {v}")
    return int(v)


def _qp_triple(v, name: str) -> Tuple[float, float, float]:
    try:
        out = tuple(float(x) for x in v)
    except TypeError:
        raise TypeError(f"query_pose: {name} must be three numbers") from None
    if len(out) != 3:
        raise ValueError(f"query_pose: {name} must be three numbers, got {len(out)}")
    return out


def query_pose(rel_pose: torch.Tensor, edge_index: torch.Tensor, *, node_first: Optional[torch.Tensor] = None,
               node_targets: Optional[torch.Tensor] = None, map_poses: Optional[torch.Tensor] = None,
               neighbours: Optional[torch.Tensor] = None, query_targets: Optional[torch.Tensor] = None,
               edge_first: Optional[torch.Tensor] = None, pose_m=(0.0, 0.0, 0.0), pose_s=(1.0, 1.0, 1.0), ref_node: int = 0,
               status: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per graph of one forward's output the query's pose and errors (rpg_query_pose_f64; evaluate.query_pose + evaluate.errors
    on the device): rel_pose fp32 [E, 6] and edge_index int64 [2, E] as the forward returned them -> float64 [G, 16] =
    pred (t, q) [7], targ (t, q) [7], translation error, rotation error in degrees.

    The graphs come in one of two forms.  Targets: ``node_first`` int64 [G + 1] (graph g owns nodes node_first[g] ..
    node_first[g + 1]) and ``node_targets`` fp32 [N, 6], the collated ``data.y``.  Map: ``map_poses`` fp32 [M, 6] and
    ``neighbours`` int64 [G, K] (graph g is a query followed by those map rows; an index outside [0, M) is clamped), with
    ``query_targets`` fp32 [G, 6] or None (zeros).  ``edge_first`` int64 [G + 1]: the columns of graph g when the edge list is
    cut contiguously; None for a model-built list (a column then belongs to the graph whose nodes hold its target).

    A graph without a ``ref_node``-th edge into its first node, or whose reference edge starts outside the graph, gets a row of
    NaN and one count in ``status`` (int32 device tensor, accumulates) -- with ``status=None`` the count is read back here (one
    synchronisation) and a non-zero count raises the ValueError of ``evaluate.reference_edge``.  Every argument is checked on
    the host before anything is launched: TypeError for a wrong type or dtype, ValueError for a wrong shape or device."""
    graphs = _qp_graphs("query_pose", rel_pose, edge_index, node_first, node_targets, map_poses, neighbours, query_targets,
                        edge_first, status, out)
    pm, ps = _qp_triple(pose_m, "pose_m"), _qp_triple(pose_s, "pose_s")
    return _qp_launch("rpg_query_pose_f64", "query_pose", graphs, pm, ps, (_qp_ref_node(ref_node),), (),
                      "lack the reference edge, or its source lies outside the graph")


def _qp_graphs(who, rel_pose, edge_index, node_first, node_targets, map_poses, neighbours, query_targets, edge_first, status, out):
    """The checks ``query_pose`` and ``query_pose_fused`` share: the forward's output, the two forms of the graphs, ``out`` and
    ``status``.  -> (rel, ei, E, G, (N, M, K), the form's tensors by
    name -- still as given --, out, status, whether the status word is this call's own)."""
    rel = _qp_tensor(rel_pose, "rel_pose", torch.float32, (None, 6), who)
    e = int(rel.shape[0])
    ei = _qp_tensor(edge_index, "edge_index", torch.int64, (2, e), who)
    if e < 1:
        raise ValueError(f"{who}: needs at least one edge")
    if (node_targets is None) == (map_poses is None):
        raise ValueError(f"{who}: give node_first + node_targets (the collated targets) or map_poses + neighbours (the map "
                         "form): exactly one of the two")
    n = m = k = 0
    if node_targets is not None:
        if neighbours is not None or query_targets is not None:
            raise ValueError(f"{who}: neighbours / query_targets belong to the map form (map_poses)")
        if node_first is None:
            raise ValueError(f"{who}: node_targets needs node_first [G + 1]")
        nf = _qp_tensor(node_first, "node_first", torch.int64, (None,), who)
        g = int(nf.shape[0]) - 1
        nt = _qp_tensor(node_targets, "node_targets", torch.float32, (None, 6), who)
        n = int(nt.shape[0])
        if n < 1:
            raise ValueError(f"{who}: node_targets is empty")
        parts = [("node_first", nf), ("node_targets", nt)]
    else:
        if node_first is not None:
            raise ValueError(f"{who}: node_first belongs to the targets form (graph g of the map form owns nodes g (K + 1) ..)")
        if neighbours is None:
            raise ValueError(f"{who}: map_poses needs neighbours [G, K]")
        nb = _qp_tensor(neighbours, "neighbours", torch.int64, (None, None), who)
        g, k = int(nb.shape[0]), int(nb.shape[1])
        mp = _qp_tensor(map_poses, "map_poses", torch.float32, (None, 6), who)
        m = int(mp.shape[0])
        if k < 1 or m < 1:
            raise ValueError(f"{who}: needs K >= 1 neighbours per query and M >= 1 map rows (K={k}, M={m})")
        parts = [("map_poses", mp), ("neighbours", nb)]
        if query_targets is not None:
            parts.append(("query_targets", _qp_tensor(query_targets, "query_targets", torch.float32, (g, 6), who)))
    if g < 1:
        raise ValueError(f"{who}: no graphs")
    if edge_first is not None:
        parts.append(("edge_first", _qp_tensor(edge_first, "edge_first", torch.int64, (g + 1,), who)))
    if out is not None:
        _qp_tensor(out, "out", torch.float64, (g, 16), who)
        if not out.is_contiguous():
            raise ValueError(f"{who}: out must be contiguous")
    status, own = _status_arg(status, rel.device, who, bad_dtype=TypeError)
    return rel, ei, e, g, (n, m, k), dict(parts), out, status, own


def _qp_launch(entry: str, who: str, graphs, pm, ps, head, outputs, lack: str) -> torch.Tensor:
    """One launch of a pose rule's C entry point over the result of ``_qp_graphs``: everything on rel_pose's GPU and contiguous,
    ``out`` made if it was not given, then the call -- the arguments all four entry points share, up to the six pose_m / pose_s
    doubles, then ``head``, ``out``, the optional ``outputs`` [(name, tensor | None)], the status word and the stream.  A status
    word that is this call's own is read back and a non-zero count raises the ValueError of ``evaluate.reference_edge`` ("...
    graph(s) of this call ``lack``").  -> out."""
    rel, ei, e, g, (n, m, k), by_name, out, status, own = graphs
    dev = rel.device
    if dev.type != "cuda":
        raise ValueError(f"{who}: rel_pose must be on the GPU (the HIP kernel is the only compute path), got {dev}")
    for name, t in [("edge_index", ei)] + list(by_name.items()) + [("out", out)] + list(outputs):
        if t is not None and t.device != dev:
            raise ValueError(f"{who}: {name} is on {t.device}, rel_pose on {dev}: everything must be on the same GPU")
    rel, ei = rel.contiguous(), ei.contiguous()
    by_name = {name: t.contiguous() for name, t in by_name.items()}
    ptr = {name: _p(t) for name, t in by_name.items()}
    if out is None:
        out = torch.empty((g, 16), dtype=torch.float64, device=dev)
    L.check(getattr(L.lib(), entry)(_p(rel), ei.data_ptr(), ei.data_ptr() + 8 * e, e, ptr.get("node_first"), ptr.get("edge_first"), g,
                                    ptr.get("node_targets"), n, ptr.get("map_poses"), m, ptr.get("neighbours"), k,
                                    ptr.get("query_targets"), *pm, *ps, *head, _p(out), *(_p(t) for _, t in outputs),
                                    status.data_ptr(), _stream()), who)
    bad = _own_count(status, own)
    if bad:
        raise ValueError(f"graph has no edge into node 0: cannot derive the query pose ({bad} graph(s) of this call {lack})")
    return out


FUSE_MODES = ("mean", "median", "consensus")   # the first two: the C entry point's `fuse` is the index; the third has its own
# the consensus rule's thresholds: API defaults, not measured optima.  Both belong to the scene's scale; INLIER_T is in the unit of
# the un-normalised translation (it is compared after `* pose_s + pose_m`), INLIER_DEG in degrees.  These three and _qp_thresholds
# are the host rule's too: evaluate.py imports them (this module needs no built library until a kernel is called)
INLIER_T, INLIER_DEG = 0.25, 5.0


def _qp_fuse(fuse, max_edges, who: str = "query_pose_fused"):
    if fuse not in FUSE_MODES:
        raise ValueError(f"{who}: fuse must be 'mean', 'median' or 'consensus', got {fuse!r}")
    if isinstance(max_edges, bool) or not isinstance(max_edges, numbers.Integral):
        raise TypeError(f"{who}: max_edges must be an int, got {type(max_edges).__name__}")
    if not 1 <= max_edges <= 64:
        raise ValueError(f"{who}: max_edges must be in 1..64 (one candidate per lane of a wave), got {max_edges}")
    return FUSE_MODES.index(fuse), int(max_edges)


def _qp_thresholds(inlier_t, inlier_deg, who: str = "query_pose_fused") -> Tuple[float, float]:
    """The consensus rule's two thresholds as floats: both finite, inlier_t >= 0, 0 <= inlier_deg <= 360 (ValueError otherwise)."""
    out = []
    for name, v in (("inlier_t", inlier_t), ("inlier_deg", inlier_deg)):
        if isinstance(v, bool) or not isinstance(v, numbers.Real):
            raise ValueError(f"{who}: {name} must be a finite number, got {v!r}")
        out.append(float(v))
    t, deg = out
    if not (t >= 0.0 and t != float("inf")):                 # (written so that NaN fails too)
        raise ValueError(f"{who}: inlier_t must be finite and >= 0, got {inlier_t!r}")
    if not 0.0 <= deg <= 360.0:
        raise ValueError(f"{who}: inlier_deg must be in 0..360 degrees, got {inlier_deg!r}")
    return t, deg


# the weighted rules' floor under every variance: an API default like the thresholds above, not a tuned value.  It only has to keep
# 1 / (v + floor) finite for a variance of exactly 0 (McDropout(samples=1), a dead feature row); it is in the unit of the variances,
# i.e. of the NORMALISED pose squared.  _qp_weights is the host rule's check too (evaluate.py imports it)
VAR_FLOOR = 1e-12
WEIGHT_MODES = ("variance",)


def _qp_weights(weights, fuse, var_floor, who: str = "query_pose_fused") -> Tuple[Optional[str], float]:
    """The weighting of a fused rule and its floor, checked (ValueError): ``weights`` None or ``"variance"``, the latter with
    ``fuse="mean"`` or ``"consensus"`` only (there is no weighted single edge, median or medoid); ``var_floor`` a finite number
    >= 1e-30, checked always and read with weights only."""
    if isinstance(var_floor, bool) or not isinstance(var_floor, numbers.Real):
        raise ValueError(f"{who}: var_floor must be a finite number >= 1e-30, got {var_floor!r}")
    floor = float(var_floor)
    if not (floor >= 1e-30 and floor != float("inf")):       # (written so that NaN fails too)
        raise ValueError(f"{who}: var_floor must be finite and >= 1e-30, got {var_floor!r}")
    if weights is None:
        return None, floor
    if weights not in WEIGHT_MODES:
        raise ValueError(f"{who}: weights must be None or 'variance', got {weights!r}")
    if fuse not in ("mean", "consensus"):
        raise ValueError(f"{who}: weights={weights!r} weights the mean of fuse='mean' or 'consensus', got fuse={fuse!r}")
    return weights, floor


def query_pose_fused(rel_pose: torch.Tensor, edge_index: torch.Tensor, *, fuse: str, max_edges: int = 64,
                     node_first: Optional[torch.Tensor] = None, node_targets: Optional[torch.Tensor] = None,
                     map_poses: Optional[torch.Tensor] = None, neighbours: Optional[torch.Tensor] = None,
                     query_targets: Optional[torch.Tensor] = None, edge_first: Optional[torch.Tensor] = None,
                     pose_m=(0.0, 0.0, 0.0), pose_s=(1.0, 1.0, 1.0), status: Optional[torch.Tensor] = None,
                     out: Optional[torch.Tensor] = None, candidates: Optional[torch.Tensor] = None,
                     counts: Optional[torch.Tensor] = None, inlier_t: float = INLIER_T, inlier_deg: float = INLIER_DEG,
                     inliers: Optional[torch.Tensor] = None, weights: Optional[str] = None,
                     rel_var: Optional[torch.Tensor] = None, var_floor: float = VAR_FLOOR,
                     spread: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``query_pose`` over ALL the edges into every graph's query node (rpg_query_pose_fused_f64; evaluate.fused_query_pose on
    the device): each such edge whose source is not the query itself is one estimate of the query's pose, the first
    ``max_edges`` (1..64) of them in column order are combined by ``fuse`` -- ``"mean"`` (mean translation, sign-aligned
    normalised quaternion sum) or ``"median"`` (component-wise median translation, medoid quaternion) -- and the row's errors are
    those of the fused pose.  The graphs' two forms, ``edge_first``, ``status``, ``out`` and the row layout are ``query_pose``'s.

    ``fuse="consensus"`` (rpg_query_pose_consensus_f64; ``evaluate.consensus_query_row`` in numpy): the candidates vote.  Two
    finite candidates support each other when their translations lie within ``inlier_t`` AND their rotations within
    ``inlier_deg`` degrees; the candidate of largest support wins (the lowest slot among equals) and the row holds the ``"mean"``
    of its supporters alone.  A non-finite candidate is an outlier, it voids nothing; when every used candidate is non-finite the
    pose and both errors are NaN (not a bad graph).  ``inliers`` int32 [G, 2] (optional output, this mode only): per graph
    (supporters of the winner, candidates used) -- their ratio is the caller's confidence; (0, used) for a bad graph.  The
    defaults 0.25 / 5.0 are API defaults, not measured optima: both belong to the scene's scale, and ``inlier_t`` is in the unit
    of the UN-NORMALISED translation (compared after ``* pose_s + pose_m``).  Both must be finite, ``inlier_t >= 0`` and
    ``0 <= inlier_deg <= 360`` (ValueError); with the other modes they are checked and not used.

    ``candidates`` float64 [G, max_edges, 16] (optional output): used candidate c as a full row, NaN past the graph's count;
    ``counts`` int32 [G] (optional output): the usable edges found before the cut at ``max_edges``.  A graph without a usable
    edge, or with a used edge whose source lies outside the graph, gets a NaN row and one count in ``status``.

    ``weights="variance"`` (rpg_query_pose_weighted_f64; ``evaluate.weighted_query_row`` in numpy; with ``fuse="mean"`` or
    ``"consensus"`` only, ValueError otherwise): the mean of those two rules weights every candidate by the inverse of its
    Monte-Carlo variance.  ``rel_var`` fp32 [E, 6], row for row with ``rel_pose`` (``McSpread.rel_var``: the variance of ONE
    dropout sample), is required exactly then.  Translation component j of candidate c weighs ``1 / (v_c[j] + var_floor)``, its
    quaternion ``1 / (v_c[3] + v_c[4] + v_c[5] + var_floor)``; the voting of ``"consensus"`` stays unweighted.  A variance that
    is NaN, negative or +inf counts wherever a non-finite candidate does.  ``var_floor`` (finite, >= 1e-30, ValueError; 1e-12 is
    an API default, not a tuned value) is checked always.  ``spread`` float64 [G, 2] (optional output, this mode only): per graph
    the predicted standard deviation of the fused translation, in the un-normalised unit, and of the fused rotation in
    log-quaternion units (``2 * sigma_q`` radians ~ the rotation angle's deviation); NaN where the pose is.  They are the
    deviations of one dropout sample's prediction, not of the S-sample mean."""
    who = "query_pose_fused"
    graphs = _qp_graphs(who, rel_pose, edge_index, node_first, node_targets, map_poses, neighbours, query_targets, edge_first,
                        status, out)
    g = graphs[3]
    pm, ps = _qp_triple(pose_m, "pose_m"), _qp_triple(pose_s, "pose_s")
    mode, max_edges = _qp_fuse(fuse, max_edges)
    inlier_t, inlier_deg = _qp_thresholds(inlier_t, inlier_deg)
    weights, var_floor = _qp_weights(weights, fuse, var_floor)
    consensus = fuse == "consensus"
    if inliers is not None and not consensus:
        raise ValueError(f"{who}: inliers is an output of fuse='consensus', got fuse={fuse!r}")
    if weights is None and (rel_var is not None or spread is not None):
        raise ValueError(f"{who}: rel_var / spread belong to weights='variance', got weights=None")
    if weights is not None:
        if rel_var is None:
            raise ValueError(f"{who}: weights={weights!r} needs rel_var fp32 [E, 6], the variances of rel_pose's rows")
        _qp_tensor(rel_var, "rel_var", torch.float32, (graphs[2], 6), who)
        if rel_var.device != graphs[0].device:
            raise ValueError(f"{who}: rel_var is on {rel_var.device}, rel_pose on {graphs[0].device}: everything must be on the "
                             "same GPU")
    outputs = [("candidates", candidates), ("counts", counts)] + ([("inliers", inliers)] if consensus or weights else [])
    outputs += [("spread", spread)] if weights else []
    shapes = {"candidates": (torch.float64, (g, max_edges, 16)), "counts": (torch.int32, (g,)), "inliers": (torch.int32, (g, 2)),
              "spread": (torch.float64, (g, 2))}
    for name, t in outputs:
        if t is not None:
            _qp_tensor(t, name, *shapes[name], who)
    for name, t in outputs:
        if t is not None and not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be contiguous")
    lack = "have no usable edge into their query node, or a used edge's source lies outside the graph"
    if weights:                                      # (rel_var is kept alive by the caller's own reference until the launch returns)
        var = rel_var.contiguous()
        return _qp_launch("rpg_query_pose_weighted_f64", who, graphs, pm, ps,
                          (max_edges, inlier_t, inlier_deg, _p(var), var_floor, int(consensus)), outputs, lack)
    if consensus:
        return _qp_launch("rpg_query_pose_consensus_f64", who, graphs, pm, ps, (max_edges, inlier_t, inlier_deg), outputs, lack)
    return _qp_launch("rpg_query_pose_fused_f64", who, graphs, pm, ps, (mode, max_edges), outputs, lack)


def _gather_sources(sources, weight: torch.Tensor, widths: Optional[Sequence[int]] = None):
    """The checked A operands of linear_gather / linear_gather_ex, and their C arrays: sources = [(a_k, idx_k or None), ...],
    ``widths[k]`` columns of a_k are read (all of them by default) and together they are weight's columns.
    -> (the tensors kept alive, (pointers, index pointers, row pitches, widths) as the C entry points take them)."""
    keep = [(_req(a, f"a{i}"), _opt(ix, f"idx{i}", torch.int64)) for i, (a, ix) in enumerate(sources)]
    wd_l = [a.shape[1] for a, _ in keep] if widths is None else [int(v) for v in widths]
    if len(wd_l) != len(keep) or any(w <= 0 or w > a.shape[1] for w, (a, _) in zip(wd_l, keep)):
        raise ValueError("widths: one positive entry per source, at most the source's row pitch")
    if sum(wd_l) != weight.shape[1]:
        raise ValueError("sum of source widths != weight.shape[1]")
    return keep, (L.ptr_array([a.data_ptr() for a, _ in keep]), L.ptr_array([_p(ix) for _, ix in keep]),
                  L.int_array([a.shape[1] for a, _ in keep]), L.int_array(wd_l))


def linear_gather(sources: Sequence[Tuple[torch.Tensor, Optional[torch.Tensor]]], weight: torch.Tensor,
                  bias: Optional[torch.Tensor], m: int, residual: Optional[torch.Tensor] = None, relu: bool = False) -> torch.Tensor:
    """out[m] = act(cat_k(a_k[idx_k[m]]) @ weight.T + bias (+ residual)); sources = [(a_k, idx_k or None), ...]."""
    weight, bias, residual = _req(weight, "weight"), _opt(bias, "bias"), _opt(residual, "residual")
    keep, arrays = _gather_sources(sources, weight)
    n_out = weight.shape[0]
    out = torch.empty((m, n_out), dtype=torch.float32, device=weight.device)
    L.check(L.lib().rpg_linear_gather_f32(len(keep), *arrays, _p(weight), _p(bias), _p(residual), _p(out), m, n_out,
                                           int(relu), _stream()), "linear_gather")
    return out


def linear_gather_ex(sources: Sequence[Tuple[torch.Tensor, Optional[torch.Tensor]]], weight: torch.Tensor, bias: Optional[torch.Tensor],
                     m: int, residual: Optional[torch.Tensor] = None, res_idx: Optional[torch.Tensor] = None,
                     residual2: Optional[torch.Tensor] = None, res2_idx: Optional[torch.Tensor] = None, relu: bool = False,
                     want_relu_copy: bool = False, widths: Optional[Sequence[int]] = None):
    """rpg_linear_gather_ex_f32: linear_gather with gathered residual rows, an optional max(out, 0) copy and A operands that are
    column blocks of wider tensors (``widths[k]`` < a_k.shape[1]: row pitch a_k.shape[1], the first widths[k] columns are read).
    -> out, or (out, out_relu) with ``want_relu_copy``."""
    weight, bias = _req(weight, "weight"), _opt(bias, "bias")
    residual, residual2 = _opt(residual, "residual"), _opt(residual2, "residual2")
    res_idx, res2_idx = _opt(res_idx, "res_idx", torch.int64), _opt(res2_idx, "res2_idx", torch.int64)
    keep, arrays = _gather_sources(sources, weight, widths)
    n_out = weight.shape[0]
    for r_, i_ in ((residual, res_idx), (residual2, res2_idx)):
        if r_ is not None and (r_.shape[1] < n_out or (i_ is None and r_.shape[0] != m) or (i_ is not None and i_.numel() != m)):
            raise ValueError("residual: [rows][>= n_out] with one (gathered) row per output row")
    if residual is not None and residual2 is not None and residual.shape[1] != residual2.shape[1]:
        raise ValueError("residual and residual2 share one row pitch")
    out = torch.empty((m, n_out), dtype=torch.float32, device=weight.device)
    out_relu = torch.empty_like(out) if want_relu_copy else None
    rows = (C.c_long * len(keep))(*[a.shape[0] if ix is not None else 0 for a, ix in keep])
    L.check(L.lib().rpg_linear_gather_ex_f32(len(keep), *arrays, rows, _p(weight), _p(bias), _p(residual), _p(res_idx), _p(residual2),
                                              _p(res2_idx), 0 if residual is None else residual.shape[1], _p(out), _p(out_relu), m, n_out,
                                              int(relu), _stream()), "linear_gather_ex")
    return (out, out_relu) if want_relu_copy else out


ROUTE_FIELDS = ("kernel", "BM", "BN", "BK", "waves", "loader", "epi_lds", "occ", "tiles", "t_dp", "g_sk", "rem", "its_per", "combine",
                "fold_k")
ROUTE_KERNELS = ("none", "tile", "linear112", "linear112k2")
ROUTE_LOADERS = ("general", "buffer", "tap")
ROUTE_COMBINES = ("none", "fixup", "inkernel")


def gemm_last_route() -> Dict[str, object]:
    """What the launcher did with this thread's last fp32 GEMM (rpg_gemm_last_route): kernel "tile" | "linear112" | "linear112k2"
    ("none" before the first launch), BM / BN / BK, waves, loader "general" | "buffer" | "tap", epi_lds, occ, tiles, t_dp, g_sk,
    rem, its_per, combine "none" | "fixup" | "inkernel", fold_k."""
    raw = (C.c_int * len(ROUTE_FIELDS))()
    n = L.lib().rpg_gemm_last_route(raw, len(ROUTE_FIELDS))
    if n != len(ROUTE_FIELDS):
        raise L.RpgError(f"gemm_last_route: the library records {n} fields, this binding knows {len(ROUTE_FIELDS)}")
    rec: Dict[str, object] = dict(zip(ROUTE_FIELDS, (int(v) for v in raw)))
    rec["kernel"], rec["loader"], rec["combine"] = ROUTE_KERNELS[raw[0]], ROUTE_LOADERS[raw[5]], ROUTE_COMBINES[raw[13]]
    return rec


BF16_ROUTE_FAMILIES = ("none", "general", "interleaved", "dma", "patch", "patch_persistent", "pair", "block", "block_persistent",
                       "block_two_group")


def conv_bf16_last_route() -> Dict[str, object]:
    """What the launchers did with this thread's last bf16 convolution / paired launch / fused block / bf16 Linear
    (rpg_conv_bf16_last_route): family (one of BF16_ROUTE_FAMILIES; "none": the shape was refused), bm, bn (the tile of the first
    kernel launched), detail (K step | LDS-DMA configuration | weight stages), launches (2: the tail re-tiling split the rows)."""
    v = [C.c_int() for _ in range(5)]
    L.check(L.lib().rpg_conv_bf16_last_route(*[C.byref(f) for f in v]), "conv_bf16_last_route")
    fam, bm, bn, detail, launches = (int(f.value) for f in v)
    return {"family": BF16_ROUTE_FAMILIES[fam], "bm": bm, "bn": bn, "detail": detail, "launches": launches}


def attention_rows(gtp: torch.Tensor) -> torch.Tensor:
    gtp = _req(gtp, "gtp")
    r, c3 = gtp.shape
    c = c3 // 3
    y = torch.empty((r, c), dtype=torch.float32, device=gtp.device)
    L.check(L.lib().rpg_attention_rows_f32(_p(gtp), r, c, _p(y), _stream()), "attention_rows")
    return y


def scatter_mean(msg: torch.Tensor, rowptr: torch.Tensor, perm: torch.Tensor, n: int) -> torch.Tensor:
    msg = _req(msg, "msg")
    rowptr, perm = _req(rowptr, "rowptr", torch.int32), _req(perm, "perm", torch.int32)
    e, d = msg.shape
    out = torch.empty((n, d), dtype=torch.float32, device=msg.device)
    L.check(L.lib().rpg_scatter_mean_f32(_p(msg), _p(rowptr), _p(perm), n, e, d, _p(out), _stream()), "scatter_mean")
    return out


def attention_aggregate(gtp: torch.Tensor, msg: torch.Tensor, rowptr: torch.Tensor, perm: torch.Tensor, n: int,
                        bias: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(ybar [n, c], mbar [n, d]): per-node means of the attention rows of gtp [e, 3c] and of msg [e, d] (+ bias on nodes
    with incoming edges), ascending edge order; see rpg_attention_aggregate_f32."""
    gtp, msg = _req(gtp, "gtp"), _req(msg, "msg")
    rowptr, perm = _req(rowptr, "rowptr", torch.int32), _req(perm, "perm", torch.int32)
    bias = _opt(bias, "bias")
    e, c3 = gtp.shape
    c, d = c3 // 3, msg.shape[1]
    ybar = torch.empty((n, c), dtype=torch.float32, device=gtp.device)
    mbar = torch.empty((n, d), dtype=torch.float32, device=gtp.device)
    L.check(L.lib().rpg_attention_aggregate_f32(_p(gtp), _p(msg), _p(rowptr), _p(perm), _p(bias), n, e, c, d, _p(ybar), _p(mbar),
                                                _stream()), "attention_aggregate")
    return ybar, mbar


def attention_aggregate_hidden(gtp: torch.Tensor, hid: torch.Tensor, rowptr: torch.Tensor, perm: torch.Tensor, n: int,
                               bias: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(ybar [n, c], hbar [n, d], res [n, d]): attention_aggregate on the message MLP's hidden rows, with the bias kept apart as the
    residual rows of the node-level Linear behind it (bias on nodes with incoming edges, zeros on the others); see
    rpg_attention_aggregate_hidden_f32."""
    gtp, hid, bias = _req(gtp, "gtp"), _req(hid, "hid"), _req(bias, "bias")
    rowptr, perm = _req(rowptr, "rowptr", torch.int32), _req(perm, "perm", torch.int32)
    e, c3 = gtp.shape
    c, d = c3 // 3, hid.shape[1]
    if bias.numel() != d or hid.shape[0] != e:
        raise ValueError("attention_aggregate_hidden: gtp [e, 3c], hid [e, d], bias [d]")
    ybar = torch.empty((n, c), dtype=torch.float32, device=gtp.device)
    hbar = torch.empty((n, d), dtype=torch.float32, device=gtp.device)
    res = torch.empty((n, d), dtype=torch.float32, device=gtp.device)
    L.check(L.lib().rpg_attention_aggregate_hidden_f32(_p(gtp), _p(hid), _p(rowptr), _p(perm), _p(bias), n, e, c, d, _p(ybar), _p(hbar),
                                                       _p(res), _stream()), "attention_aggregate_hidden")
    return ybar, hbar, res


def pose_heads(x: torch.Tensor, w6: torch.Tensor, b6: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    x, w6, b6 = _req(x, "x"), _req(w6, "w6"), _req(b6, "b6")
    r, d = x.shape
    out = _out(out, (r, 6), torch.float32, x.device, "pose_heads")
    L.check(L.lib().rpg_pose_heads_f32(_p(x), _p(w6), _p(b6), r, d, _p(out), _stream()), "pose_heads")
    return out


def _mc_ids(ids, r: int, dev):
    """``pose_heads_mc``'s ``ids``: None (node rows, numbered by their row), int64 [r] (node rows with their ids), int64 [2, r] or a
    pair of int64 [r] (edge rows: the ids of source and target).  -> (id_a, id_b), each None or a contiguous int64 [r]."""
    if ids is None:
        return None, None
    if torch.is_tensor(ids):
        if ids.dim() == 1:
            ids = (ids,)
        elif ids.dim() == 2 and ids.shape[0] == 2:
            ids = (ids[0], ids[1])
        else:
            raise ValueError(f"pose_heads_mc: ids must be int64 [r] (nodes) or [2, r] (edges), got {tuple(ids.shape)}")
    if not isinstance(ids, (tuple, list)) or len(ids) not in (1, 2):
        raise TypeError("pose_heads_mc: ids must be None, an int64 tensor [r] / [2, r] or a pair of int64 tensors [r]")
    out = tuple(_req(t, "ids", torch.int64) for t in ids)
    if any(t.dim() != 1 or t.numel() != r or t.device != dev for t in out):
        raise ValueError(f"pose_heads_mc: every id vector must be int64 [{r}] on the inputs' GPU")
    return out[0], (out[1] if len(out) == 2 else None)


def pose_heads_mc(x: torch.Tensor, w6: torch.Tensor, b6: torch.Tensor, p: float, samples: int, seed: int, state: torch.Tensor,
                  ids=None, id_offset: int = 0, want_samples: bool = False, out=None):
    """The heads under ``samples`` dropout masks of rate ``p`` from one read of x [r, d] (rpg_pose_heads_mc_f32): -> (mean [r, 6],
    var [r, 6]) over the samples, and with ``want_samples`` the samples themselves [samples, r, 6] as a third element.  ``state``:
    device int32 / uint32 [2] = (draw, node_base), read by the kernel; ``seed``: 64 bits.  The masks are a function of (seed, draw,
    ids, column, sample) only: ``ids`` None numbers node rows by node_base + id_offset + row, an int64 [r] gives their ids, an int64
    [2, r] (or a pair of [r]) the ids of an edge row's source and target, all offset by node_base + id_offset.  ``out``: (mean, var)
    to write into.  ValueError for p outside (0, 1), samples outside 1..1024, d % 4, d / 4 >= 65536, ids beyond 2^31."""
    x, w6, b6 = _req(x, "x"), _req(w6, "w6"), _req(b6, "b6")
    if not torch.is_tensor(state) or not state.is_cuda or state.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):
        raise TypeError("pose_heads_mc: state must be a 32-bit integer tensor [2] = (draw, node_base) on the GPU")
    if state.numel() != 2 or not state.is_contiguous() or state.device != x.device:
        raise ValueError("pose_heads_mc: state must hold (draw, node_base), contiguous, on the inputs' GPU")
    if x.dim() != 2 or w6.dim() != 2 or tuple(w6.shape) != (6, x.shape[1]) or b6.numel() != 6:
        raise ValueError(f"pose_heads_mc: x [r, d], w6 [6, d] and b6 [6], got {tuple(x.shape)}, {tuple(w6.shape)}, {tuple(b6.shape)}")
    r, d = x.shape
    samples, seed, id_offset = int(samples), int(seed), int(id_offset)
    if not 0 <= seed < 2 ** 64:
        raise ValueError("pose_heads_mc: seed must fit 64 bits")
    id_a, id_b = _mc_ids(ids, r, x.device)
    mean_out, var_out = (None, None) if out is None else out
    mean = _out(mean_out, (r, 6), torch.float32, x.device, "pose_heads_mc")
    var = _out(var_out, (r, 6), torch.float32, x.device, "pose_heads_mc")
    smp = torch.empty((max(samples, 0), r, 6), dtype=torch.float32, device=x.device) if want_samples else None
    L.check(L.lib().rpg_pose_heads_mc_f32(_p(x), _p(w6), _p(b6), r, d, float(p), samples, seed, _p(state), _p(id_a), _p(id_b),
                                          id_offset, _p(mean), _p(var), _p(smp), _stream()), "pose_heads_mc")
    return (mean, var, smp) if want_samples else (mean, var)


def mc_advance(state: torch.Tensor) -> None:
    """draw += 1 in ``state`` (see ``pose_heads_mc``) on the current stream (rpg_mc_advance)."""
    if not torch.is_tensor(state) or not state.is_cuda or state.numel() != 2 or state.element_size() != 4:
        raise TypeError("mc_advance: state must be a 32-bit integer tensor [2] on the GPU")
    L.check(L.lib().rpg_mc_advance(_p(state), _stream()), "mc_advance")


def gnn_forward_query(tensors: Sequence[torch.Tensor], feat: torch.Tensor, edge_index: torch.Tensor, sel: torch.Tensor,
                      qnodes: torch.Tensor, gnn_recursion: int = 2, weights_bf16: Optional[Sequence[torch.Tensor]] = None,
                      node_offset: int = 0, want_features: bool = False, status: Optional[torch.Tensor] = None,
                      workspace: Optional[torch.Tensor] = None):
    """The GNN and its heads in the query-only output mode (rpg_gnn_forward_query_f32, or _bf16 with ``weights_bf16`` from
    params.pack_gnn_bf16): ``tensors`` from params.pack_gnn (22 or 26, or 30 with params.pack_gnn_mean_first's behind them), feat [n, d], edge_index int64 [2, e], ``sel`` int64
    [e_sel] -- ascending, exactly the valid columns whose target is in ``qnodes`` (graph.query_edge_columns) -- and ``qnodes``
    int64 [q], ascending node ids -> (abs_pose [q, 6] of qnodes, rel_pose [e_sel, 6] of the sel columns), and with
    ``want_features`` also (node_out [q, d], edge_out [e_sel, d]), the heads' inputs.  Every row is what the full forward gives
    there; the last recursion only runs on the selected columns and the query rows.

    A selection that breaks the contract (a column outside [0, e), one graph_prepare leaves out, one whose target is no query
    node, columns that do not ascend, a count other than the edges into the query nodes, qnodes not ascending / distinct / in
    range) and a bad edge are counted into ``status`` (int32 device tensor, accumulates; everything is clamped) -- with
    ``status=None`` the count is read back here (one synchronisation) and a non-zero count raises IndexError.  ``workspace``: a
    uint8 device tensor to use instead of allocating one."""
    feat, ei = _req(feat, "feat"), _req(edge_index, "edge_index", torch.int64)
    sel, qnodes = _req(sel, "sel", torch.int64), _req(qnodes, "qnodes", torch.int64)
    if feat.dim() != 2 or ei.dim() != 2 or ei.shape[0] != 2 or sel.dim() != 1 or qnodes.dim() != 1:
        raise ValueError("gnn_forward_query: feat [n, d], edge_index [2, e], sel [e_sel] and qnodes [q]")
    (n, d), e, es, q = feat.shape, ei.shape[1], sel.numel(), qnodes.numel()
    if not (1 <= es <= e and 1 <= q <= n) or d % 32:
        raise ValueError(f"gnn_forward_query: needs 1 <= e_sel <= e, 1 <= q <= n and d % 32 == 0 (e_sel={es}, e={e}, q={q}, n={n}, d={d})")
    dev = feat.device
    if any(t.device != dev for t in (ei, sel, qnodes)):
        raise RuntimeError("gnn_forward_query: feat, edge_index, sel and qnodes must be on the same GPU")
    keep = [_req(t, f"tensors[{i}]") for i, t in enumerate(tensors)]
    lib = L.lib()
    need = int(lib.rpg_gnn_query_workspace_bytes(n, e, d, es, q))
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    elif workspace.dtype != torch.uint8 or workspace.device != dev or not workspace.is_contiguous():
        raise ValueError("gnn_forward_query: workspace must be a contiguous uint8 tensor on the inputs' GPU")
    abs_pose = torch.empty((q, 6), dtype=torch.float32, device=dev)
    rel_pose = torch.empty((es, 6), dtype=torch.float32, device=dev)
    node_out = torch.empty((q, d), dtype=torch.float32, device=dev) if want_features else None
    edge_out = torch.empty((es, d), dtype=torch.float32, device=dev) if want_features else None
    status, own = _status_arg(status, dev, "gnn_forward_query")
    weights = (L.ptr_array([t.data_ptr() for t in keep]), len(keep))
    fn = lib.rpg_gnn_forward_query_f32
    if weights_bf16 is not None:
        keep_bf = [_req(t, f"weights_bf16[{i}]", torch.bfloat16) for i, t in enumerate(weights_bf16)]
        weights += (L.ptr_array([t.data_ptr() for t in keep_bf]), len(keep_bf))
        fn = lib.rpg_gnn_forward_query_bf16
    L.check(fn(*weights, _p(feat), ei.data_ptr(), ei.data_ptr() + 8 * e, int(node_offset), n, e, d, int(gnn_recursion), _p(sel), es,
               _p(qnodes), q, _p(abs_pose), _p(rel_pose), _p(node_out), _p(edge_out), status.data_ptr(), workspace.data_ptr(),
               workspace.numel(), _stream()), "gnn_forward_query")
    bad = _own_count(status, own)
    if bad:
        raise IndexError(f"gnn_forward_query: {bad} violation(s) of the index contract: an edge with a node id outside [0, n), or a "
                         "selection that is not exactly the ascending valid columns into the ascending, distinct query nodes")
    return (abs_pose, rel_pose, node_out, edge_out) if want_features else (abs_pose, rel_pose)


def timing_enable(on: bool) -> None:
    L.check(L.lib().rpg_timing_enable(int(on)), "timing_enable")


def timing_read() -> Dict[str, Dict[str, float]]:
    n = len(L.TIMER_NAMES)
    ms, cnt, work, ex = (C.c_double * n)(), (C.c_longlong * n)(), (C.c_double * n)(), (C.c_double * n)()
    L.check(L.lib().rpg_timing_read_ex(ms, cnt, work, ex), "timing_read")
    return {name: {"ms": ms[i], "launches": int(cnt[i]), "work": work[i], "executed": ex[i]}
            for i, name in enumerate(L.TIMER_NAMES)}


def release_scratch() -> None:
    """Free the library-owned split-K scratch pool of the fine-grained entry points (synchronises)."""
    L.check(L.lib().rpg_release_scratch(), "release_scratch")


# The tuning keys in key order: TUNE_<name> = the header's RPG_TUNE_<name> (tests/test_host.py checks them against it).  The header
# documents each key's values; csrc/tuning.h holds their defaults, accepted values and decoding.
TUNING_KEYS = (
    "TILE", "BK", "EPILOGUE", "STREAMK", "WINOGRAD", "GNN_SPLIT", "BF16_BK", "FAST_LOADER", "WINO_SPLIT", "BF16_FAST", "FUSED_STEM",
    "WAVES8", "WINO_SHORT", "GNN_FUSE_AGG", "WINO_PERSIST", "BF16_TILE", "BF16_DMA", "BF16_PATCH", "BF16_WS64", "SK_MIN_ITS",
    "INKERNEL_FIXUP", "BF16_CHUNK", "WINO2D", "BF16_LEAN_EPI", "BF16_LINEAR_DMA", "BF16_PERSIST", "FOLD_K", "BF16_FUSE_BLOCK",
    "BF16_TAIL", "LIN112", "FIXUP_PRIO", "BF16_PAIR",
)
globals().update({"TUNE_" + _name: _key for _key, _name in enumerate(TUNING_KEYS)})


def _tuning_key(key) -> int:
    """A key given as its number, its name ("FOLD_K") or its constant's name ("TUNE_FOLD_K")."""
    if isinstance(key, str):
        return TUNING_KEYS.index(key[5:] if key.startswith("TUNE_") else key)
    return int(key)


def set_tuning(key: int, value: int) -> None:
    L.check(L.lib().rpg_set_tuning(key, value), "set_tuning")


def get_tuning(key) -> int:
    """The value last accepted for the key, as it was passed in (its default before any set)."""
    value = C.c_int()
    L.check(L.lib().rpg_get_tuning(_tuning_key(key), C.byref(value), None), "get_tuning")
    return value.value


def tuning_default(key) -> int:
    value = C.c_int()
    L.check(L.lib().rpg_get_tuning(_tuning_key(key), None, C.byref(value)), "tuning_default")
    return value.value


def reset_tuning() -> None:
    """Every key back to its default."""
    for key in range(len(TUNING_KEYS)):
        set_tuning(key, tuning_default(key))


@contextlib.contextmanager
def tuned(keys):
    """with tuned({key or name: value, ...}): the keys set for the block, EVERY key back at its default afterwards -- also when a
    set is refused half-way or the block raises.  Blocks do not nest (the inner one's exit resets the outer one's keys): name
    every key of a launch in one block."""
    try:
        for key, value in keys.items():
            set_tuning(_tuning_key(key), value)
        yield
    finally:
        reset_tuning()


def track_update(rows: torch.Tensor, inliers: torch.Tensor, prior: torch.Tensor, lost: torch.Tensor, accepted: torch.Tensor,
                 min_inliers: int, min_ratio: float, max_lost: int) -> torch.Tensor:
    """The update launch of a tracking loop (rpg_track_update_f64), in place: per camera s, the pose in ``rows[s, :7]`` (float64
    [S, 16], the pose rule's rows) is accepted when it is finite, ``inliers[s, 0] >= min_inliers`` and ``inliers[s, 0] >=
    min_ratio * inliers[s, 1]`` (int32 [S, 2], the consensus rule's (inliers, used)); then ``prior[s]`` (float64 [S, 7]) becomes
    that pose, ``lost[s] = 0`` and ``accepted[s] = 1``; otherwise ``accepted[s] = 0``, ``lost[s]`` counts one more frame and past
    ``max_lost`` the prior becomes NaN.  ``lost`` / ``accepted``: int32 [S].  Returns ``accepted``."""
    rows, inliers = _req(rows, "rows", torch.float64), _req(inliers, "inliers", torch.int32)
    s = rows.shape[0]
    if rows.dim() != 2 or rows.shape[1] != 16 or s < 1 or tuple(inliers.shape) != (s, 2):
        raise ValueError(f"track_update: rows must be float64 [S >= 1, 16] and inliers int32 [S, 2], got {tuple(rows.shape)} and "
                         f"{tuple(inliers.shape)}")
    for t, name, dtype, shape in ((prior, "prior", torch.float64, (s, 7)), (lost, "lost", torch.int32, (s,)),
                                  (accepted, "accepted", torch.int32, (s,))):
        if (not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous()
                or t.device != rows.device):
            raise ValueError(f"track_update: {name} must be a contiguous {dtype} {list(shape)} tensor on the rows' GPU (it is "
                             "written in place)")
    min_ratio = float(min_ratio)
    if min_ratio != min_ratio:
        raise ValueError("track_update: min_ratio is NaN")
    L.check(L.lib().rpg_track_update_f64(_p(rows), _p(inliers), s, int(min_inliers), min_ratio, int(max_lost), _p(prior), _p(lost),
                                         _p(accepted), _stream()), "track_update")
    return accepted
