#!/usr/bin/env python3
"""Times simple_knn.distCUDA2 (gsr_knn_dist2) and scene_utils.unproject_rgbd on the HIP device: HIP events around each call,
warm-up, medians.  Point sets: the uniform box of make_gaussians and a depth sheet (a smooth synthetic depth image
back-projected by the library itself) at 100 k / 1 M / 5 M points; unproject_rgbd at 1080p.  Beside it, what a user has without the
module: a chunked torch.cdist + topk brute force on the same device at 100 k.  A second, separately run pass with the library's
per-kernel event timing on (gsr_profile_enable) attributes the time to the sort, the box build and the query sweep and derives
the achieved bytes/s of the first two from the bytes the algorithm moves.
    python tools/knn_bench.py [--out profiles/knn_bench.json] [--sizes 100000,1000000,5000000]"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-slam_amd"))
import torch  # noqa: E402
from diff_gaussian_rasterization import _C  # noqa: E402
from scene_utils import fibonacci_cameras, unproject_rgbd  # noqa: E402
from simple_knn._C import distCUDA2  # noqa: E402

BOX, SUPER = 64, 64


def median_ms(fn, warmup=3, reps=11):
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


def uniform_box(P, seed=0, box=1.3):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(P, 3, generator=g) * (2 * box) - box).cuda()


def depth_image(H, W, dev="cuda"):
    y, x = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32),
                          indexing="ij")
    g = torch.Generator(device=dev).manual_seed(1)
    return 2.0 + 0.6 * torch.sin(x / W * 5.0 + 1.0) * torch.cos(y / H * 4.0 + 2.0) + 0.02 * torch.randn(H, W, device=dev, generator=g)


def depth_sheet(P):
    W = int(math.sqrt(P * 16 / 9)) + 1
    H = (P + W - 1) // W
    cam = fibonacci_cameras(2, W, H, seed=3, device="cuda")[0]
    xyz, _ = unproject_rgbd(cam, torch.zeros(3, H, W, device="cuda"), depth_image(H, W))
    return xyz[:P].contiguous()


def brute_force(points, chunk=4096):
    out = torch.empty(points.shape[0], device=points.device)
    for s in range(0, points.shape[0], chunk):
        d = torch.cdist(points[s:s + chunk], points) ** 2
        out[s:s + chunk] = torch.topk(d, 4, dim=1, largest=False).values[:, 1:].mean(1)      # [0] is the point itself
    return out


def kernel_split(points):
    """One profiled call: ms per kernel group (events around every launch: not the end-to-end time)."""
    lib = _C.lib()
    distCUDA2(points)
    torch.cuda.synchronize()
    lib.gsr_profile_reset()
    lib.gsr_profile_enable(1)
    distCUDA2(points)
    torch.cuda.synchronize()
    lib.gsr_profile_enable(0)
    prof = _C.profile_read()
    sort = sum(v[0] for k, v in prof.items() if k.startswith("radix"))
    return dict(sort_ms=sort, boxes_ms=prof.get("knn_boxes", (0, 0))[0], query_ms=prof.get("knn_query", (0, 0))[0],
                other_ms=sum(v[0] for k, v in prof.items() if k.startswith("knn_") and k not in ("knn_boxes", "knn_query")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_bench.json"))
    ap.add_argument("--sizes", default="100000,1000000,5000000")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("knn_bench needs the HIP device: nothing is measured without it")
    res = dict(device=torch.cuda.get_device_name(0), box=BOX, super_box=SUPER, knn=[], unproject=None, brute_force=None)
    for P in [int(s) for s in args.sizes.split(",")]:
        for name, make in (("uniform_box", uniform_box), ("depth_sheet", depth_sheet)):
            pts = make(P)
            med, lo, hi = median_ms(lambda: distCUDA2(pts))
            split = kernel_split(pts)
            nbox = (P + BOX - 1) // BOX
            row = dict(points=P, set=name, median_ms=med, min_ms=lo, max_ms=hi, **split,
                       # 30-bit keys: 4 passes, each reads and writes key + value (16 B), + one histogram read of the keys
                       sort_bytes=P * (4 * 16 + 4), boxes_bytes=P * (4 + 12 + 16),
                       super_box_tests_per_query=(nbox + SUPER - 1) // SUPER)
            row["sort_GBps"] = row["sort_bytes"] / (split["sort_ms"] * 1e6) if split["sort_ms"] else None
            row["boxes_GBps"] = row["boxes_bytes"] / (split["boxes_ms"] * 1e6) if split["boxes_ms"] else None
            res["knn"].append(row)
            print(json.dumps(row), flush=True)
            del pts
    pts = uniform_box(100000)
    med, lo, hi = median_ms(lambda: brute_force(pts), warmup=1, reps=5)
    ours = distCUDA2(pts)
    ref = brute_force(pts)
    res["brute_force"] = dict(points=100000, what="chunked torch.cdist + topk", median_ms=med, min_ms=lo, max_ms=hi,
                              max_rel_diff_to_hip=float(((ours - ref).abs() / ref.clamp_min(1e-30)).max()))
    print(json.dumps(res["brute_force"]), flush=True)
    W, H = 1920, 1080
    cam = fibonacci_cameras(2, W, H, seed=3, device="cuda")[0]
    depth, img = depth_image(H, W), torch.rand(3, H, W, device="cuda")
    alpha, z = torch.rand(H, W, device="cuda"), depth * torch.rand(H, W, device="cuda")
    for label, kw in (("all valid pixels", {}), ("alpha + rendered_z rule", dict(alpha=alpha, rendered_z=z))):
        med, lo, hi = median_ms(lambda: unproject_rgbd(cam, img, depth, **kw))
        n = int(unproject_rgbd(cam, img, depth, **kw)[0].shape[0])
        row = dict(what=label, W=W, H=H, selected=n, median_ms=med, min_ms=lo, max_ms=hi,
                   note="includes the host read-back of the count and the allocation of the outputs")
        res["unproject"] = (res["unproject"] or []) + [row]
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
