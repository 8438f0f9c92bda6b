"""Times the TSDF kernels (csrc/tsdf.hip) at 640 x 480, a 1 cm voxel and a 4 cm truncation: touch, integrate, extract points,
extract triangles - recorded, not gated (the output is kept as profiles/tsdf.txt).

The scene is analytic: a sphere of radius 0.8 m seen from 2.2 m by cameras on a Fibonacci sphere.  Per stage the wall time of the
Python call between two device synchronisations (median of --repeat calls), and for integrate the bytes a block moves - tsdf,
weight and colour of 512 voxels read and written, 20 KiB - against the 6.29 TB/s an MI355X was measured to copy at.

    python tools/tsdf_bench.py [--views 8] [--repeat 20]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-slam_amd"))

HBM_MEASURED = 6.29e12        # B/s, float4 copy
BLOCK_BYTES = 512 * (4 + 4 + 12) * 2


def sphere_depth(cam, radius, dev):
    """z-depth and colour of a sphere at the origin through `cam`, on the device"""
    import scene_utils as S
    fx, fy, cx, cy = S.camera_intrinsics(cam)
    H, W = cam.image_height, cam.image_width
    v, u = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64),
                          indexing="ij")
    w2c = cam.world_view_transform.T.double()
    R, t = w2c[:3, :3], w2c[:3, 3]
    dirs = torch.stack(((u - cx) / fx, (v - cy) / fy, torch.ones_like(u)), dim=-1) @ R
    o = -R.T @ t
    a, b = (dirs * dirs).sum(-1), dirs @ o
    disc = b * b - a * (o @ o - radius * radius)
    lam = (-b - disc.clamp_min(0).sqrt()) / a
    hit = disc > 0
    nrm = (o + lam[..., None] * dirs) / radius
    image = torch.where(hit[..., None], 0.5 + 0.5 * nrm, torch.zeros_like(nrm)).permute(2, 0, 1).float().contiguous()
    return image, torch.where(hit, lam, torch.zeros_like(lam)).float().contiguous()


def timed(fn, repeat):
    ms = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--voxel", type=float, default=0.01)
    ap.add_argument("--trunc", type=float, default=0.04)
    args = ap.parse_args()
    import scene_utils as S
    dev = torch.device("cuda:0")
    cams = S.fibonacci_cameras(args.views, 640, 480, radius=2.2, seed=1, device=dev)
    frames = [sphere_depth(c, 0.8, dev) + (c,) for c in cams]
    vol = S.TSDFVolume(args.voxel, args.trunc, depth_trunc=5.0, device=dev)
    for image, depth, cam in frames:
        vol.integrate(image, depth, cam)
    image, depth, cam = frames[0]
    touched = int(vol.touch(depth, cam).shape[0])
    print(f"640 x 480, voxel {args.voxel} m, truncation {args.trunc} m, {args.views} views: {vol.num_blocks} blocks "
          f"({vol.num_blocks * 512 * 20 / 2 ** 20:.0f} MiB), {touched} touched by one frame")
    med, best = timed(lambda: vol.touch(depth, cam), args.repeat)
    print(f"touch (kernel + unique of 27 x 307200 keys)   median {med:8.3f} ms   best {best:8.3f} ms")
    med, best = timed(lambda: vol.integrate(image, depth, cam), args.repeat)
    t_touch = timed(lambda: vol.touch(depth, cam), args.repeat)[1]
    moved = touched * BLOCK_BYTES
    print(f"integrate (touch + merge + kernel)            median {med:8.3f} ms   best {best:8.3f} ms")
    print(f"  integrate without touch (merge and launch included), best: {best - t_touch:.3f} ms for {moved / 2 ** 20:.1f} MiB of block rows "
          f"({BLOCK_BYTES} B per block) = {moved / max(best - t_touch, 1e-6) / 1e6:.1f} GB/s, "
          f"{100 * moved / max(best - t_touch, 1e-6) * 1e3 / HBM_MEASURED:.1f} % of the measured 6.29 TB/s")
    med, best = timed(lambda: vol.extract_point_cloud(), args.repeat)
    n = int(vol.extract_point_cloud()[0].shape[0])
    print(f"extract_point_cloud ({n} points)          median {med:8.3f} ms   best {best:8.3f} ms")
    med, best = timed(lambda: vol.extract_triangle_mesh(weld=False), args.repeat)
    n = int(vol.extract_triangle_mesh(weld=False)[0].shape[0])
    print(f"extract_triangle_mesh, soup ({n} triangles) median {med:8.3f} ms   best {best:8.3f} ms")
    med, best = timed(lambda: vol.extract_triangle_mesh(), max(3, args.repeat // 4))
    print(f"extract_triangle_mesh, welded                 median {med:8.3f} ms   best {best:8.3f} ms")
    from diff_gaussian_rasterization import _C
    _C.lib().gsr_profile_enable(1)
    _C.lib().gsr_profile_reset()
    for _ in range(args.repeat):
        vol.integrate(image, depth, cam)
        vol.extract_point_cloud()
        vol.extract_triangle_mesh(weld=False)
    torch.cuda.synchronize()
    for name, (ms, calls) in sorted(_C.profile_read().items()):
        if name.startswith("tsdf"):
            print(f"  kernel {name:22s} {ms / max(calls, 1):8.4f} ms per launch ({calls} launches)")
            if name == "tsdf_integrate":
                rate = moved / (ms / calls * 1e-3)
                print(f"    = {rate / 1e12:.2f} TB/s of block rows, {100 * rate / HBM_MEASURED:.0f} % of the measured 6.29 TB/s "
                      f"(a volume of this size stays in the 256 MiB Infinity Cache)")
    _C.lib().gsr_profile_enable(0)


if __name__ == "__main__":
    main()
