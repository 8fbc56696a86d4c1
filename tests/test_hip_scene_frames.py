"""Per-frame image statistics on the GPU (rpg_frames_u8_to_*_scenes / frames.SceneFrameTransform) against the existing launch:
the frames of scene s, transformed by ``FrameTransform`` with scene s's six floats, must be EQUAL bit for bit, in fp32 and bf16."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MEANS = ((0.485, 0.456, 0.406), (0.1, 0.7, 0.3), (0.52, 0.5, 0.9))
STDS = ((0.229, 0.224, 0.225), (0.5, 0.05, 1.75), (0.3, 0.31, 0.07))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _frames(dev, n, h, w, seed):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, (n, h, w, 3)).astype(np.uint8)).to(dev)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _per_scene(sft, frames, scenes, dtype):
    """The existing launch, once per scene, on that scene's frames."""
    oh, ow = sft.output_size(frames.shape[1], frames.shape[2])
    out = torch.empty((frames.shape[0], 3, oh, ow), dtype=dtype, device=frames.device)
    sc = np.asarray(scenes)
    for s in np.unique(sc):
        idx = torch.as_tensor(np.flatnonzero(sc == s), device=frames.device)
        out[idx] = sft.scene(int(s)).apply(frames[idx].contiguous(), dtype=dtype)
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", ["five", "many", "crossing", "noresize"])
def test_equals_the_launch_per_scene(dev, dtype, shape):
    """"many": 2048 one-tile frames with scenes i % 3 (a launcher that takes 8 workgroups per CU gives each of them one tile on
    a 256-CU device, so this case alone crosses nothing there).  "crossing": one-tile frames, three times and a few more than the largest grid the launcher takes (8 workgroups per CU, as
    ``ops.frames_plan`` and the device's CU count say), with scenes drawn at random: a workgroup walks tiles wi, wi + grid,
    wi + 2 grid (and a few a fourth), whose scenes differ for most workgroups -- the table is rebuilt after it has been used."""
    from relpose_gnn_amd.frames import SceneFrameTransform
    if shape == "five":
        sft, frames, scenes = SceneFrameTransform(24, MEANS, STDS), _frames(dev, 5, 30, 40, 1), [2, 0, 0, 1, 2]
    elif shape == "many":
        sft, frames = SceneFrameTransform(8, MEANS, STDS), _frames(dev, 2048, 12, 16, 2)
        scenes = [i % 3 for i in range(2048)]
    elif shape == "crossing":
        from relpose_gnn_amd import ops
        plan = ops.frames_plan(12, 16, 8, 10)
        assert plan["tiles_y"] == plan["tiles_x"] == 1
        grid = 8 * torch.cuda.get_device_properties(dev).multi_processor_count     # the launcher's cap: at most 8 workgroups per CU
        n = 3 * grid + 37
        sft, frames = SceneFrameTransform(8, MEANS, STDS), _frames(dev, n, 12, 16, 2)
        scenes = np.random.RandomState(9).randint(0, 3, n).tolist()
        walks = np.asarray(scenes[:3 * grid]).reshape(3, grid)                      # row j: the scene of every workgroup's j-th tile
        assert ((walks[0] != walks[1]) | (walks[1] != walks[2])).mean() > 0.8       # most workgroups change scene on their way
    else:
        sft, frames, scenes = SceneFrameTransform(None, MEANS, STDS), _frames(dev, 7, 9, 13, 3), [1, 1, 2, 0, 2, 0, 1]
    got = sft.apply(frames, scenes, dtype=dtype)
    want = _per_scene(sft, frames, scenes, dtype)
    assert got.dtype == dtype and got.shape == want.shape
    assert torch.equal(_bits(got), _bits(want))
    # the int32 device form of the scenes gives the same
    dev_scenes = torch.as_tensor(scenes, dtype=torch.int32).to(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    assert torch.equal(_bits(sft.apply(frames, dev_scenes, dtype=dtype, status=status)), _bits(want))
    assert int(status.item()) == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_scene_out_of_range_is_counted_and_takes_scene_0(dev, dtype):
    from relpose_gnn_amd.frames import SceneFrameTransform
    sft, frames = SceneFrameTransform(24, MEANS, STDS), _frames(dev, 6, 30, 40, 4)
    scenes = torch.tensor([1, -1, 3, 2, 0, 7], dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    got = sft.apply(frames, scenes, dtype=dtype, status=status)
    assert int(status.item()) == 3
    assert torch.equal(_bits(got), _bits(_per_scene(sft, frames, [1, 0, 0, 2, 0, 0], dtype)))
    with pytest.raises(IndexError):               # without a counter of the caller's the count is read back and raised
        sft.apply(frames, scenes, dtype=dtype)
    with pytest.raises(IndexError):               # host scenes are checked before the launch
        sft.apply(frames, [1, -1, 3, 2, 0, 7], dtype=dtype)
