"""Time the uint8 frame transform (rpg_frames_u8_to_f32 / _bf16) on one GPU: 512 frames (one 64-graph micro-batch) per launch.

    python tools/frames_bench.py [--reps 50]

Prints one JSON line per case: median launch time (HIP events around each launch, after warm-up) and the algorithmic bytes
(frames read once + output written once) per second as a share of the 8 TB/s HBM spec.  For kernel-only times run it under
`rocprofv3 --kernel-trace --stats -- python tools/frames_bench.py`."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from relpose_gnn_amd.frames import FrameTransform  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--frames", type=int, default=512)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ft = FrameTransform(256, mean=(0.5, 0.45, 0.44), std=(0.28, 0.28, 0.25))
    g = torch.Generator(device=dev).manual_seed(0)
    for (h, w), dtype in (((480, 640), torch.bfloat16), ((480, 640), torch.float32), ((256, 341), torch.bfloat16),
                          ((256, 341), torch.float32), ((1080, 1920), torch.bfloat16)):
        n = args.frames if h * w <= 480 * 640 else args.frames // 4
        x = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device=dev, generator=g)
        oh, ow = ft.output_size(h, w)
        out = torch.empty((n, 3, oh, ow), dtype=dtype, device=dev)
        for _ in range(5):
            ft.apply(x, dtype, out=out)
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ft.apply(x, dtype, out=out)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        ts.sort()
        us = ts[len(ts) // 2]
        nbytes = x.numel() + out.numel() * out.element_size()
        print(json.dumps({"in": f"{h}x{w}", "out": f"{oh}x{ow}", "dtype": str(dtype).split(".")[-1], "frames": n,
                          "median_us": round(us, 1), "min_us": round(ts[0], 1), "alg_MB": round(nbytes / 1e6, 1),
                          "TB_s": round(nbytes / us / 1e6, 2), "share_of_8TBs": round(nbytes / us / 1e6 / 8.0, 3)}), flush=True)


if __name__ == "__main__":
    main()
