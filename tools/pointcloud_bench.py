#!/usr/bin/env python3
"""Times the point-cloud conditioning stage on the HIP device: simple_knn.knn_k at k = 3, 8, 19 (mean distance only, what the
outlier filter asks for) beside the existing knn_dist2, scene_utils.voxel_down_sample and condition_point_cloud (voxel grid, then
the statistical outlier filter at nb_neighbors = 20).  HIP events around each call, 5 warm-up calls, median of 30.  Point sets: a
synthetic depth frame back-projected by the library (640 x 480 = 307 200 points; ~1 M at 1344 x 744) and the uniform box, at
307 200 and 1 000 000 points.  A second, separately run pass with the library's per-kernel event timing on
(gsr_profile_enable) says where a call's time goes: sort, box build, query sweep, voxel reduction, statistics.
The Python calls include their allocations and, for voxel_down_sample / condition_point_cloud, the read-back of the count.
    python tools/pointcloud_bench.py [--out profiles/pointcloud_bench.json] [--sizes 307200,1000000]"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-slam_amd"))
import torch  # noqa: E402
from diff_gaussian_rasterization import _C  # noqa: E402
from scene_utils import condition_point_cloud, fibonacci_cameras, unproject_rgbd, voxel_down_sample  # noqa: E402
from simple_knn import knn_dist2, knn_k  # noqa: E402

WARMUP, REPS = 5, 30
VOXEL = 0.05


def median_ms(fn):
    ts = []
    for i in range(WARMUP + REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= WARMUP:
            ts.append(a.elapsed_time(b))
    ts.sort()
    return dict(median_ms=ts[len(ts) // 2], min_ms=ts[0], max_ms=ts[-1])


def kernel_split(fn):
    """one profiled call: ms per kernel (events around every launch: not the end-to-end time)"""
    lib = _C.lib()
    fn()
    torch.cuda.synchronize()
    lib.gsr_profile_reset()
    lib.gsr_profile_enable(1)
    fn()
    torch.cuda.synchronize()
    lib.gsr_profile_enable(0)
    prof = _C.profile_read()
    groups = {}
    for name, (ms, _) in prof.items():
        key = "sort" if name.startswith("radix") else "scan" if name.startswith("scan") else name
        groups[key] = groups.get(key, 0.0) + ms
    return {k: round(v, 5) for k, v in sorted(groups.items())}


def uniform_box(P, box=1.3):
    g = torch.Generator().manual_seed(0)
    return (torch.rand(P, 3, generator=g) * (2 * box) - box).cuda()


def depth_frame(P):
    """a smooth depth image with sensor noise, back-projected: 640 x 480 for 307 200 points, 4:3 otherwise"""
    W = 640 if P == 307200 else int(math.sqrt(P * 4 / 3)) + 1
    H = (P + W - 1) // W
    y, x = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32),
                          indexing="ij")
    g = torch.Generator(device="cuda").manual_seed(1)
    depth = 2.0 + 0.6 * torch.sin(x / W * 5.0 + 1.0) * torch.cos(y / H * 4.0 + 2.0) + 0.02 * torch.randn(H, W, device="cuda", generator=g)
    cam = fibonacci_cameras(2, W, H, seed=3, device="cuda")[0]
    xyz, _ = unproject_rgbd(cam, torch.zeros(3, H, W, device="cuda"), depth)
    return xyz[:P].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointcloud_bench.json"))
    ap.add_argument("--sizes", default="307200,1000000")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pointcloud_bench needs the HIP device: nothing is measured without it")
    res = dict(device=torch.cuda.get_device_name(0), warmup=WARMUP, reps=REPS, voxel_size=VOXEL, nb_neighbors=20, std_ratio=2.0,
               rows=[])
    for P in [int(s) for s in args.sizes.split(",")]:
        for name, make in (("depth_frame", depth_frame), ("uniform_box", uniform_box)):
            pts = make(P)
            cols = torch.rand(P, 3, device="cuda")
            row = dict(points=P, set=name)
            row["knn_dist2"] = dict(**median_ms(lambda: knn_dist2(pts)), kernels=kernel_split(lambda: knn_dist2(pts)))
            for k in (3, 8, 19):
                def call():
                    return knn_k(pts, k, return_dist2=False, return_mean=True)
                row[f"knn_k_{k}"] = dict(**median_ms(call), kernels=kernel_split(call))
            q3 = row["knn_k_3"]["kernels"].get("knn_query_k4", 0.0)
            q19 = row["knn_k_19"]["kernels"].get("knn_query_k32", 0.0)
            row["k19_over_k3"] = dict(call=row["knn_k_19"]["median_ms"] / row["knn_k_3"]["median_ms"],
                                      query_kernel=q19 / q3 if q3 else None, linear_in_k=19 / 3)
            vox = voxel_down_sample(pts, cols, VOXEL)[0]
            row["voxel_down_sample"] = dict(**median_ms(lambda: voxel_down_sample(pts, cols, VOXEL)), voxels=int(vox.shape[0]),
                                            kernels=kernel_split(lambda: voxel_down_sample(pts, cols, VOXEL)))
            out = condition_point_cloud(pts, cols, VOXEL, 20, 2.0)[0]
            row["condition_point_cloud"] = dict(**median_ms(lambda: condition_point_cloud(pts, cols, VOXEL, 20, 2.0)),
                                                kept=int(out.shape[0]),
                                                kernels=kernel_split(lambda: condition_point_cloud(pts, cols, VOXEL, 20, 2.0)))
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
            del pts, cols
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
