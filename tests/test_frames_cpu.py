"""Host side of the uint8 frame transform (no GPU): the C table builder, the numpy restatement the GPU tests compare against
(proved equal to Pillow here), torchvision's size rule, the stats-file reader, the exact inverse of processed samples and the
model's state_dict with a transform set."""
import numpy as np
import pytest
import torch

from test_hip_frames import MEAN, VAR, rand_frames, ref_output_size, ref_resize, ref_table, ref_transform

GEOMS = [(480, 640, 256, 341), (1080, 1920, 256, 455), (100, 80, 320, 256), (257, 341, 256, 339), (37, 53, 256, 366),
         (256, 400, 256, 400)]


def test_c_table_builder_equals_restatement():
    from relpose_gnn_amd import ops
    for n_in, n_out in [(640, 341), (480, 256), (1920, 455), (1080, 256), (80, 256), (100, 320), (53, 366), (37, 256),
                        (341, 339), (257, 256), (400, 400), (5000, 256)]:
        b, w = ops.resize_table(n_in, n_out)
        rb, rw = ref_table(n_in, n_out)
        assert np.array_equal(b.numpy(), rb) and np.array_equal(w.numpy(), rw), (n_in, n_out)
    with pytest.raises(ValueError):
        ops.resize_table(0, 4)


def test_torchvision_size_rule():
    from relpose_gnn_amd.frames import FrameTransform, output_size
    for h, w, oh, ow in GEOMS:
        assert output_size(h, w) == ref_output_size(h, w), (h, w)
    assert output_size(480, 640) == (256, 341)
    assert output_size(1080, 1920) == (256, 455)
    assert output_size(100, 80) == (320, 256)
    assert output_size(256, 341) == (256, 341)            # short side already 256: no resize
    assert output_size(400, 256) == (400, 256)
    assert output_size(300, 300) == (256, 256)
    assert FrameTransform(None).output_size(37, 53) == (37, 53)


@pytest.mark.parametrize("geom", GEOMS, ids=[f"{g[0]}x{g[1]}" for g in GEOMS])
def test_restatement_equals_pillow(geom):
    Image = pytest.importorskip("PIL.Image")
    h, w, oh, ow = geom
    assert ref_output_size(h, w) == (oh, ow)
    frames = rand_frames(2, h, w, seed=h + w)
    mine = ref_resize(frames, oh, ow)
    pil = np.stack([np.asarray(Image.fromarray(f, "RGB").resize((ow, oh), Image.BILINEAR)) for f in frames])
    assert np.array_equal(mine, pil), geom


def test_stats_file_reader(tmp_path):
    from relpose_gnn_amd.frames import FrameTransform
    p = tmp_path / "stats.txt"
    stats = np.array([[0.5164, 0.4437, 0.4443], [0.0773, 0.0808, 0.0647]])
    np.savetxt(p, stats)
    ft = FrameTransform.from_stats_file(str(p))
    loaded = np.loadtxt(p)
    # what torchvision's Normalize uses: torch.as_tensor(mean / np.sqrt(var), dtype=float32)
    assert ft.mean == tuple(float(v) for v in torch.as_tensor(loaded[0], dtype=torch.float32))
    assert ft.std == tuple(float(v) for v in torch.as_tensor(np.sqrt(loaded[1]), dtype=torch.float32))
    assert ft.resize == 256
    with pytest.raises(ValueError):
        FrameTransform(256, mean=(0, 0, 0), std=(1, 0, 1))


def test_frames_from_normalized_round_trip_is_exact():
    from relpose_gnn_amd.io import frames_from_normalized
    std = np.sqrt(np.asarray(VAR))
    frames = rand_frames(3, 256, 341, seed=2)
    frames[0, 0, 0] = (0, 128, 255)
    x = torch.from_numpy(ref_transform(frames)).reshape(3, -1)            # a processed sample: [n, 3*H*W]
    back = frames_from_normalized(x, MEAN, std)
    assert back.dtype == torch.uint8 and tuple(back.shape) == (3, 256, 341, 3)
    assert np.array_equal(back.numpy(), frames)
    bad = x.clone()
    bad[1, 12345] = torch.nextafter(bad[1, 12345], torch.tensor(10.0))
    with pytest.raises(ValueError):
        frames_from_normalized(bad, MEAN, std)


def test_state_dict_unchanged_with_a_transform():
    import relpose_gnn_amd.synth as S
    from relpose_gnn_amd.frames import FrameTransform
    from relpose_gnn_amd.posenet import PoseNetX_R2
    from relpose_gnn_amd.resnet import resnet34
    m = PoseNetX_R2(resnet34(), droprate=0.0, pretrained=False, feat_dim=64, edge_feat_dim=64, node_dim=64, use_gnn=True)
    keys = list(m.state_dict().keys())
    assert m.frame_transform is None
    m.frame_transform = FrameTransform(256, MEAN, np.sqrt(VAR))
    assert list(m.state_dict().keys()) == keys and len(keys) == 248
    assert not any(isinstance(v, FrameTransform) for v in m.modules())
    m.load_state_dict(S.synth_state_dict(S.posenet_r2_param_shapes(64, 64, 64), seed=1))
    assert m.frame_transform is not None
