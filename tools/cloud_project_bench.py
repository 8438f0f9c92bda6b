#!/usr/bin/env python3
"""Times scene_utils.project_cloud (project + resolve, with colours) and scene_utils.densify_depth (radius 4) on the HIP device
for 120 000 and 1 000 000 points into 1280 x 720: HIP events around each call, warm-up, medians, and - from a separate profiled
call - the library's kernels alone.  Each row carries the bytes its kernels have to move, computed from the shapes (project:
the two per-pixel buffers cleared, 12 B; a row read, 12 B, its z and pixel written and read again, 16 B, its occlusion word and
visible byte, 5 B; the buffers read and depth and index written, 20 B per pixel; 72 B per visible row for the colour: the row
again, four taps of three planes, the colour out.  densify: depth in, dense and valid out, 12 B per pixel; atomics and LDS
traffic are not bytes that must move), the share of the 6.0 TB/s plain-stream figure of DESIGN.md section 8 item 4 that implies,
and the same work written with PyTorch ops on the same device: scatter_reduce(amin) per footprint offset and for the winner,
grid_sample for the colours; max_pool and unfold-ed window sums for the fill.
One GPU process at a time: the parent starts one child per step under `timeout` and stops at the first that fails.
    python tools/cloud_project_bench.py [--out profiles/cloud_project_bench.json]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-slam_amd"))

STREAM_TBPS = 6.0
W, H = 1280, 720
K = (900.0, 900.0, 639.5, 359.5)
SIZES = (120000, 1000000)
FOOTPRINT, OCCLUSION, RADIUS, BAND = 2, 0.05, 4, 0.05
STEP_SECONDS = 60


def median_ms(fn, warmup=5, reps=31):
    import torch
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


def kernels_ms(fn, prefixes):
    import torch
    from diff_gaussian_rasterization import _C
    lib = _C.lib()
    fn()
    torch.cuda.synchronize()
    lib.gsr_profile_reset()
    lib.gsr_profile_enable(1)
    fn()
    torch.cuda.synchronize()
    lib.gsr_profile_enable(0)
    return {k: v[0] for k, v in _C.profile_read().items() if k.startswith(prefixes)}


def scene(N):
    """a wall at 8 m behind a slab at 3 m across the middle of the image, sampled at random pixel positions: points, image, camera"""
    import torch
    from scene_utils import camera_from_intrinsics
    g = torch.Generator(device="cuda").manual_seed(N)
    u = torch.rand(N, device="cuda", generator=g) * (W + 40) - 20
    v = torch.rand(N, device="cuda", generator=g) * (H + 40) - 20
    slab = ((v > 0.3 * H) & (v < 0.7 * H) & (torch.rand(N, device="cuda", generator=g) < 0.7))
    z = torch.where(slab, 3.0, 8.0) * (1.0 + 0.01 * torch.rand(N, device="cuda", generator=g))
    pts = torch.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], dim=1).contiguous()
    image = torch.rand((3, H, W), device="cuda", generator=g)
    return pts, image, camera_from_intrinsics(*K, W, H)


def torch_project(pts, image, r, scale, z_near, z_far):
    """the same outputs from PyTorch ops (identity pose)"""
    import torch
    import torch.nn.functional as F
    N = pts.shape[0]
    q = pts.double().float()
    z = q[:, 2]
    part = torch.isfinite(q).all(dim=1) & (z >= z_near) & (z <= z_far)
    px, py = K[0] * (q[:, 0] / z) + K[2], K[1] * (q[:, 1] / z) + K[3]
    u = torch.floor(px + 0.5).clamp(-(r + 1), W + r).long()
    v = torch.floor(py + 0.5).clamp(-(r + 1), H + r).long()
    zb = z.view(torch.int32)
    big = torch.iinfo(torch.int32).max
    zocc = torch.full((W * H,), big, dtype=torch.int32, device=pts.device)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            x, y = u + dx, v + dy
            m = part & (x >= 0) & (x < W) & (y >= 0) & (y < H)
            zocc.scatter_reduce_(0, (y * W + x)[m], zb[m], reduce="amin")
    cand = part & (u >= 0) & (u < W) & (v >= 0) & (v < H)
    pixel = torch.where(cand, v * W + u, -1)
    key = (zb.long() << 32) | torch.arange(N, device=pts.device)
    win = torch.full((W * H,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=pts.device)
    win.scatter_reduce_(0, pixel[cand], key[cand], reduce="amin")
    limit = zocc.view(torch.float32)[pixel.clamp_min(0)] * scale
    visible = cand & (z <= limit)
    wz = (win >> 32).int().view(torch.float32)
    seen = (win != torch.iinfo(torch.int64).max) & (wz <= zocc.view(torch.float32) * scale)
    depth = torch.where(seen, wz, 0.0).view(H, W)
    index = torch.where(seen, (win & 0xFFFFFFFF).int(), -1).view(H, W)
    grid = torch.stack([2 * px / (W - 1) - 1, 2 * py / (H - 1) - 1], dim=1).view(1, 1, N, 2)
    col = F.grid_sample(image[None], grid, mode="bilinear", padding_mode="border", align_corners=True)[0, :, 0].t()
    colors = torch.where(visible[:, None], col, 0.0)
    return depth, index, pixel, visible, colors


def torch_densify(depth, R, band_scale, k):
    import torch
    import torch.nn.functional as F
    inf = float("inf")
    zn = -F.max_pool2d(-torch.where(depth > 0, depth, inf)[None, None], 2 * R + 1, 1, R)[0, 0]
    win = F.unfold(depth[None, None], 2 * R + 1, padding=R)[0]                     # [(2R+1)^2, H W]
    off = torch.arange(-R, R + 1, device=depth.device, dtype=torch.float32)
    d2 = (off[:, None] ** 2 + off[None, :] ** 2).reshape(-1, 1)
    w = torch.where(d2 > 0, 1.0 / d2.clamp_min(1.0), 0.0)
    m = (win > 0) & (win <= (zn.reshape(1, -1) * band_scale))
    sw, swz, cnt = (w * m).sum(0), (w * m * win).sum(0), m.sum(0)
    fill = (cnt >= k) & torch.isfinite(zn.reshape(-1))
    dense = torch.where(depth.reshape(-1) > 0, depth.reshape(-1), torch.where(fill, swz / sw.clamp_min(1e-30), 0.0))
    return dense.view_as(depth), ((depth.reshape(-1) > 0) | fill).float().view_as(depth)


def step(name, N):
    """one measured step, in its own process: prints a JSON row"""
    import numpy as np
    import torch
    from scene_utils import project_cloud, densify_depth
    if not torch.cuda.is_available():
        raise SystemExit("cloud_project_bench needs the HIP device: nothing is measured without it")
    pts, image, cam = scene(N)
    npix = W * H
    opts = dict(footprint=FOOTPRINT, occlusion=OCCLUSION, z_near=0.05, z_far=100.0)
    proj = project_cloud(pts, cam, image=image, **opts)
    scale = float(np.float32(1.0 + OCCLUSION))
    if name == "project":
        nbytes = 32 * npix + 33 * N + 72 * proj.n_visible
        fn = lambda: project_cloud(pts, cam, image=image, **opts)                  # noqa: E731
        base = lambda: torch_project(pts, image, FOOTPRINT, scale, 0.05, 100.0)    # noqa: E731
        td, ti, _, tv, _ = base()
        agree = dict(depth_equal=bool(torch.equal(td, proj.depth)), visible_equal=bool(torch.equal(tv, proj.visible)))
        prefixes = ("cloud_project",)
    else:
        nbytes = 12 * npix
        fn = lambda: densify_depth(proj.depth, RADIUS, BAND, 2)                    # noqa: E731
        base = lambda: torch_densify(proj.depth, RADIUS, scale, 2)                 # noqa: E731
        agree = dict(max_abs_difference=float((base()[0] - fn()[0]).abs().max()))
        prefixes = ("depth_densify",)
    med, lo, hi = median_ms(fn)
    ker = kernels_ms(fn, prefixes)
    ksum = sum(ker.values())
    bmed, blo, bhi = median_ms(base, warmup=2, reps=9)
    row = dict(what=name, N=N, W=W, H=H, n_visible=proj.n_visible, n_candidates=proj.n_candidates,
               coverage=float((proj.depth > 0).float().mean()), bytes=nbytes, median_ms=med, min_ms=lo, max_ms=hi,
               kernels_ms=ker, kernels_sum_ms=ksum, kernels_GBps=nbytes / (ksum * 1e6),
               kernels_share_of_stream=nbytes / (ksum * 1e-3) / (STREAM_TBPS * 1e12),
               torch_median_ms=bmed, torch_min_ms=blo, torch_max_ms=bhi, torch_over_kernels=bmed / ksum, torch_over_call=bmed / med,
               agreement_with_torch=agree, device=torch.cuda.get_device_name(0))
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_project_bench.json"))
    ap.add_argument("--step", default=None, help="(internal) project:N or densify:N - one measured step in this process")
    args = ap.parse_args()
    if args.step:
        name, n = args.step.split(":")
        return step(name, int(n))
    res = dict(stream_TBps=STREAM_TBPS, footprint=FOOTPRINT, occlusion=OCCLUSION, radius=RADIUS, depth_band=BAND, rows=[],
               note="median_ms: the whole Python call (wrapper, allocations, launches, the read-back of the two counts); kernels_ms: "
                    "the library's kernels alone, from a separate profiled call; torch_*: the same work in PyTorch ops")
    for n in SIZES:
        for name in ("project", "densify"):
            cmd = ["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--step", f"{name}:{n}"]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(p.stdout)
            if p.returncode != 0:      # a failed or timed-out step: nothing more is started on the device
                raise SystemExit(f"step {name}:{n} ended with status {p.returncode}; stopping")
            res["rows"] += [json.loads(l[4:]) for l in p.stdout.splitlines() if l.startswith("ROW ")]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
