#!/usr/bin/env python3
"""Times the sensor-frame front end on the HIP device - scene_utils.undistort (gsr_frame_undistort) and scene_utils.build_pyramid
(gsr_frame_pyramid, 3 levels) - at 640 x 480 and 1920 x 1080: HIP events around each call, warm-up, medians.  Beside each, the
same work composed from torch ops on the same device: F.grid_sample over a precomputed sampling grid (bilinear colour, nearest
depth, a mask from the grid) and F.avg_pool2d per level (colour, mask; the depth rule has no torch one-liner, avg_pool2d stands in).
Bytes moved are what the algorithm needs - every input pixel read once, every output written once - computed from the shapes;
bytes / time is printed beside the 8 TB/s HBM specification.  The times include the output allocations of each call.
    python tools/frames_bench.py [--out profiles/frames_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-slam_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from scene_utils import undistort, build_pyramid  # noqa: E402

HBM_SPEC_TBPS = 8.0
DIST = (-0.28, 0.07, 1e-3, -5e-4, 0.0)
LEVELS = 3


def median_ms(fn, warmup=5, reps=31):
    ts = []
    for i in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def sampling_grid(K, W, H, dev):
    """The undistortion map as a grid_sample grid (align_corners=True: -1 .. 1 spans pixel centres 0 .. S - 1), built once."""
    fx, fy, cx, cy = K
    k1, k2, p1, p2, k3 = DIST
    v, u = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32),
                          indexing="ij")
    x, y = (u - cx) / fx, (v - cy) / fy
    r2 = x * x + y * y
    rho = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
    xd = x * rho + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * rho + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    us, vs = fx * xd + cx, fy * yd + cy
    return torch.stack([2 * us / (W - 1) - 1, 2 * vs / (H - 1) - 1], -1)[None].contiguous()


def torch_undistort(img, depth, grid):
    col = F.grid_sample(img[None], grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0]
    dep = F.grid_sample(depth[None, None], grid, mode="nearest", padding_mode="zeros", align_corners=True)[0, 0]
    mask = ((grid.abs() <= 1).all(-1)[0]).float()
    return col * mask, dep * mask, mask


def torch_pyramid(img, depth, mask):
    out = []
    for _ in range(LEVELS):
        img, depth = F.avg_pool2d(img[None], 2)[0], F.avg_pool2d(depth[None, None], 2)[0, 0]
        mask = (F.avg_pool2d(mask[None, None], 2)[0, 0] == 1).float()
        out.append((img, depth, mask))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frames_bench needs the HIP device: nothing is measured without it")
    dev = "cuda"
    res = dict(device=torch.cuda.get_device_name(0), hbm_spec_TBps=HBM_SPEC_TBPS, rows=[])
    for W, H in ((640, 480), (1920, 1080)):
        g = torch.Generator(device=dev).manual_seed(1)
        img = torch.rand(3, H, W, device=dev, generator=g)
        depth = 1.0 + 3.0 * torch.rand(H, W, device=dev, generator=g)
        depth[torch.rand(H, W, device=dev, generator=g) < 0.2] = 0.0
        K = (0.9 * W, 0.9 * W, (W - 1) / 2 + 3.2, (H - 1) / 2 - 2.1)
        n = W * H
        # undistort: 3 colour planes + depth read, 3 colour planes + depth + mask written, 4 bytes each
        und_bytes = n * 4 * (4 + 5)
        grid = sampling_grid(K, W, H, dev)
        rows = [("undistort", "hip", lambda: undistort(img, depth, K, DIST), und_bytes),
                ("undistort", "torch grid_sample (grid precomputed)", lambda: torch_undistort(img, depth, grid), und_bytes)]
        col, dep, mask = undistort(img, depth, K, DIST)
        a = torch_undistort(img, depth, grid)
        inside = (mask == 1) & (a[2] == 1)
        diff = float((col - a[0]).abs()[:, inside].max())
        # pyramid: level 0 (5 planes) read once, levels 1 .. 3 written
        pyr_bytes = sum(5 * 4 * (W >> l) * (H >> l) for l in range(LEVELS + 1))
        rows += [("pyramid L=3", "hip", lambda: build_pyramid(col, dep, mask, LEVELS), pyr_bytes),
                 ("pyramid L=3", "torch avg_pool2d per level", lambda: torch_pyramid(col, dep, mask), pyr_bytes)]
        for what, how, fn, nbytes in rows:
            med, lo, hi = median_ms(fn)
            row = dict(W=W, H=H, what=what, how=how, median_ms=med, min_ms=lo, max_ms=hi, bytes=nbytes,
                       TBps=nbytes / (med * 1e-3) / 1e12, share_of_hbm_spec=nbytes / (med * 1e-3) / 1e12 / HBM_SPEC_TBPS)
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
        print(json.dumps(dict(W=W, H=H, what="undistort colour, hip vs grid_sample where both masks are 1", max_abs_diff=diff)),
              flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
