"""uint8 frames -> the encoder's input on the GPU (rpg_frames_u8_to_f32 / _bf16, frames.FrameTransform, PoseNetX_R2.frame_transform,
evaluate_stream with uint8 graphs), checked bit for bit against the reference's CPU transform: torchvision 0.9.1 Resize(256) on a
PIL RGB image (Pillow Image.resize(BILINEAR)), ToTensor, Normalize(mean, sqrt(var)) -- dataset_7Scenes_multi.py:290-298.

Pillow need not be installed where these tests run, so the reference is a numpy restatement of Pillow's 8-bit resampler kept
here (ref_table / ref_transform); tests/test_frames_cpu.py proves it equal to Pillow itself.  Where PIL imports, the kernel is
compared with Pillow directly as well."""
import math

import numpy as np
import pytest
import torch

# a 7-Scenes-like statistics pair (mean, variance per channel)
MEAN = (0.4, 0.45, 0.5)
VAR = (0.07, 0.065, 0.08)


# ---- numpy restatement of the reference transform ------------------------------------------------------------------------
def ref_output_size(h, w, size=256):
    """torchvision 0.9.1 functional_pil.resize with an int size."""
    if (w <= h and w == size) or (h <= w and h == size):
        return h, w
    if w < h:
        return int(size * h / w), size
    return size, int(size * w / h)


def ref_table(n_in, n_out):
    """Pillow Resample.c precompute_coeffs (bilinear, support 1) + normalize_coeffs_8bpc: (bounds [out, 2], weights [out, ksize])."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fs
    ss = 1.0 / fs
    ks = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((n_out, 2), np.int32)
    weights = np.zeros((n_out, ks), np.int32)
    for o in range(n_out):
        center = (o + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        cnt = min(int(center + support + 0.5), n_in) - xmin
        k = []
        for x in range(cnt):
            t = abs((x + xmin - center + 0.5) * ss)
            k.append(1.0 - t if t < 1.0 else 0.0)
        ww = 0.0
        for v in k:
            ww += v
        for x, v in enumerate(k):
            v = v / ww if ww != 0.0 else v
            weights[o, x] = int(0.5 + v * (1 << 22)) if v >= 0 else int(-0.5 + v * (1 << 22))
        bounds[o] = (xmin, cnt)
    return bounds, weights


def _pass(img, bounds, weights, axis):
    """One 8-bit pass over axis 1 (rows) or 2 (columns) of uint8 [n, H, W, 3]: clamp((2^21 + sum src * w) >> 22, 0, 255)."""
    ks = weights.shape[1]
    j = np.arange(ks)[None, :]
    valid = j < bounds[:, 1:2]
    idx = np.where(valid, bounds[:, 0:1] + j, 0)
    w = np.where(valid, weights, 0).astype(np.int64)
    src = img.astype(np.int64)
    if axis == 2:
        taps = src[:, :, idx, :]                                   # [n, H, out, ks, 3]
        acc = (taps * w[None, None, :, :, None]).sum(axis=3)
    else:
        taps = src[:, idx, :, :]                                   # [n, out, ks, W, 3]
        acc = (taps * w[None, :, :, None, None]).sum(axis=2)
    return np.clip((acc + (1 << 21)) >> 22, 0, 255).astype(np.uint8)


def ref_resize(frames, oh, ow):
    """Pillow Image.resize((ow, oh), BILINEAR) of uint8 RGB frames [n, H, W, 3]."""
    n, h, w, _ = frames.shape
    img = frames
    vb, vw = ref_table(h, oh) if oh != h else (None, None)
    if ow != w:
        if oh != h:                                                # horizontal pass over the rows the vertical pass reads
            first, last = int(vb[0, 0]), int(vb[-1, 0] + vb[-1, 1])
            img = img[:, first:last]
            vb = vb.copy()
            vb[:, 0] -= first
        hb, hw = ref_table(w, ow)
        img = _pass(img, hb, hw, 2)
    if oh != h:
        img = _pass(img, vb, vw, 1)
    return img


def ref_normalize(img, mean, std):
    """ToTensor + Normalize on the CPU: ((float)u / 255 - mean_c) / std_c in fp32, both divisions correctly rounded."""
    m = np.asarray(mean, np.float64).astype(np.float32)
    s = np.asarray(std, np.float64).astype(np.float32)
    x = img.astype(np.float32) / np.float32(255)
    x = (x - m) / s
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2))


def ref_transform(frames, mean=MEAN, std=None, size=256):
    std = np.sqrt(np.asarray(VAR, np.float64)) if std is None else std
    n, h, w, _ = frames.shape
    oh, ow = ref_output_size(h, w, size)
    return ref_normalize(ref_resize(frames, oh, ow), mean, std)


def rand_frames(n, h, w, seed):
    """Camera-like frames: smooth gradients + noise (exercises the whole 0..255 range and the clamps)."""
    g = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    out = np.empty((n, h, w, 3), np.uint8)
    for i in range(n):
        base = 127.5 + 127.5 * np.sin(2 * np.pi * (g.uniform(0.5, 3) * yy[..., None] + g.uniform(0.5, 3) * xx[..., None]
                                                   + g.uniform(0, 1, 3)))
        out[i] = np.clip(base + g.normal(0, 40, (h, w, 3)), 0, 255).astype(np.uint8)
    out[0, 0, :4] = 0
    out[0, -1, -4:] = 255
    return out


def _pil_transform(frames, mean, std):
    from PIL import Image
    n, h, w, _ = frames.shape
    oh, ow = ref_output_size(h, w)
    imgs = np.stack([np.asarray(Image.fromarray(f, "RGB").resize((ow, oh), Image.BILINEAR)) for f in frames])
    return ref_normalize(imgs, mean, std)


def _have_pil():
    try:
        import PIL  # noqa: F401
        return True
    except ImportError:
        return False


# ---- GPU tests ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ft():
    from relpose_gnn_amd.frames import FrameTransform
    return FrameTransform(256, mean=MEAN, std=np.sqrt(np.asarray(VAR)))


GEOMS = [(480, 640), (1080, 1920), (256, 341), (100, 80), (37, 53)]


@pytest.mark.gpu
@pytest.mark.parametrize("hw", GEOMS, ids=[f"{h}x{w}" for h, w in GEOMS])
def test_kernel_bit_exact_against_reference_transform(ft, hw):
    h, w = hw
    base = rand_frames(8, h, w, seed=h * 7 + w)
    want8 = torch.from_numpy(ref_transform(base))
    if _have_pil():
        assert torch.equal(torch.from_numpy(_pil_transform(base[:2], ft.mean, ft.std)), want8[:2])
    dev = torch.device("cuda:0")
    for n in (1, 8, 64):
        frames = np.concatenate([base] * ((n + 7) // 8))[:n]
        want = torch.cat([want8] * ((n + 7) // 8))[:n]
        x = torch.from_numpy(frames).to(dev)
        y32 = ft.apply(x)
        yb = ft.apply(x, torch.bfloat16)
        torch.cuda.synchronize()
        assert y32.shape == want.shape and y32.dtype == torch.float32
        assert torch.equal(y32.cpu(), want), (hw, n, int((y32.cpu() != want).sum()))
        assert torch.equal(yb.cpu(), want.to(torch.bfloat16)), (hw, n)


@pytest.mark.gpu
def test_unaligned_frame_tensors(ft):
    dev = torch.device("cuda:0")
    for h, w in ((480, 640), (37, 53), (256, 341)):
        frames = torch.from_numpy(rand_frames(3, h, w, seed=5))
        want = torch.from_numpy(ref_transform(frames.numpy()))
        nb = frames.numel()
        for off in (1, 2, 3):
            buf = torch.full((nb + 64,), 77, dtype=torch.uint8, device=dev)
            view = buf[off:off + nb].view(3, h, w, 3)
            view.copy_(frames.to(dev))
            assert view.data_ptr() % 4 == off % 4
            assert torch.equal(ft.apply(view).cpu(), want), (h, w, off)
            assert torch.equal(ft.apply(view, torch.bfloat16).cpu(), want.to(torch.bfloat16)), (h, w, off)


@pytest.mark.gpu
def test_big_launch_past_2gib_matches_pieces_and_ignores_poison(ft):
    dev = torch.device("cuda:0")
    n, h, w = 2100, 256, 341
    assert n * 3 * h * w * 4 > 2 ** 31
    frames = torch.from_numpy(rand_frames(16, h, w, seed=9)).to(dev).repeat(n // 16 + 1, 1, 1, 1)[:n].contiguous()
    frames[-1] = torch.arange(h * w * 3, device=dev).view(h, w, 3).to(torch.uint8)       # the last frame differs from the others
    big = torch.full((n, 3, h, w), float("nan"), dtype=torch.float32, device=dev)
    ft.apply(frames, out=big)
    piece = torch.full((64, 3, h, w), float("nan"), dtype=torch.float32, device=dev)
    for i0 in range(0, n, 64):
        i1 = min(n, i0 + 64)
        ref = ft.apply(frames[i0:i1], out=piece[: i1 - i0])
        assert torch.equal(big[i0:i1], ref), i0
    assert torch.equal(big[-1].cpu(), torch.from_numpy(ref_transform(frames[-1:].cpu().numpy()))[0])
    from relpose_gnn_amd import _lib
    assert _lib.lib().rpg_frames_workspace_bytes(n, 480, 640, 256, 341) == 0       # the intermediate stays in LDS
    del big, piece
    torch.cuda.empty_cache()


def _model(dev, enc):
    import relpose_gnn_amd.synth as S
    from relpose_gnn_amd.posenet import PoseNetX_R2
    from relpose_gnn_amd.resnet import resnet34
    D = 256
    m = PoseNetX_R2(resnet34(), droprate=0.0, pretrained=False, feat_dim=D, edge_feat_dim=D, node_dim=D, input_img_height=256,
                    use_gnn=True, knn=-1, use_AP=True, gnn_recursion=2)
    m.load_state_dict(S.synth_state_dict(S.posenet_r2_param_shapes(D, D, D), seed=3))
    m = m.to(dev).eval()
    m.encoder_dtype = enc
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("enc", ["f32", "bf16"])
def test_model_on_frames_equals_model_on_reference_images(ft, enc):
    from relpose_gnn_amd.graph import fc_batch
    dev = torch.device("cuda:0")
    m = _model(dev, enc)
    base = rand_frames(16, 480, 640, seed=21)
    ref = torch.from_numpy(ref_transform(base)).reshape(16, -1)
    for graphs in (1, 32):
        n = 8 * graphs
        idx = np.arange(n) % 16
        fr = torch.from_numpy(base[idx]).to(dev)
        x32 = ref[idx].contiguous().to(dev)
        m.frame_transform = None
        a0, r0, _ = m(fc_batch(x32, 8))
        m.frame_transform = ft
        a1, r1, _ = m(fc_batch(fr, 8))
        torch.cuda.synchronize()
        assert torch.equal(a0, a1) and torch.equal(r0, r1), (enc, graphs)
    m.frame_transform = None


@pytest.mark.gpu
def test_evaluate_stream_uint8_frames(ft):
    from relpose_gnn_amd.evaluate import evaluate_stream
    from relpose_gnn_amd.graph import Data, fc_edge_index
    dev = torch.device("cuda:0")
    m = _model(dev, "bf16")
    G, h, w = 12, 300, 400
    base = rand_frames(8, h, w, seed=33)
    ref = torch.from_numpy(ref_transform(base)).reshape(8, -1)
    g = torch.Generator().manual_seed(4)
    ys = [torch.randn(8, 6, generator=g) for _ in range(G)]
    ei = fc_edge_index(8)
    perm = [np.roll(np.arange(8), k) for k in range(G)]
    f32 = [Data(x=ref[p].contiguous().pin_memory(), edge_index=ei, y=y) for p, y in zip(perm, ys)]
    pinned = [Data(x=torch.from_numpy(base[p]).pin_memory(), edge_index=ei, y=y) for p, y in zip(perm, ys)]
    pageable = [Data(x=torch.from_numpy(base[p]).clone(), edge_index=ei, y=y) for p, y in zip(perm, ys)]
    r0 = evaluate_stream(m, f32, dev, micro_batch=8)
    m.frame_transform = ft
    frame_bytes = 8 * h * w * 3
    for src, kind in ((pinned, "direct_bytes"), (pageable, "staged_bytes")):
        st = {}
        r = evaluate_stream(m, src, dev, micro_batch=8, stats=st)
        assert np.array_equal(r.pred_poses, r0.pred_poses) and np.array_equal(r.t_loss, r0.t_loss), kind
        assert np.array_equal(r.q_loss, r0.q_loss)
        assert st["h2d_bytes"] == G * frame_bytes and st[kind] == G * frame_bytes, st
    m.frame_transform = None


@pytest.mark.gpu
def test_frame_errors(ft):
    from relpose_gnn_amd.graph import Batch, Data, fc_batch, fc_edge_index
    from relpose_gnn_amd.evaluate import evaluate_stream
    dev = torch.device("cuda:0")
    m = _model(dev, "f32")
    fr = torch.from_numpy(rand_frames(8, 480, 640, seed=1))
    with pytest.raises(TypeError):                                  # no transform: exactly today's error
        m(fc_batch(fr.to(dev), 8))
    m.frame_transform = ft
    from relpose_gnn_amd.frames import FrameTransform
    m.frame_transform = FrameTransform(320, ft.mean, ft.std)       # 480 x 640 -> 320 x 426, but input_img_height is 256
    with pytest.raises(ValueError):
        m(fc_batch(fr.to(dev), 8))
    m.frame_transform = ft
    ei = fc_edge_index(8)
    mixed = [Data(x=fr, edge_index=ei, y=torch.zeros(8, 6)),
             Data(x=torch.zeros((8, 300, 400, 3), dtype=torch.uint8), edge_index=ei, y=torch.zeros(8, 6))]
    with pytest.raises(ValueError):
        Batch.from_data_list(mixed)
    with pytest.raises(ValueError):
        evaluate_stream(m, mixed, dev, micro_batch=8)
    with pytest.raises(RuntimeError):                               # frames on the CPU
        m(fc_batch(fr, 8))
    with pytest.raises(RuntimeError):
        ft.apply(fr)
    m.frame_transform = None
