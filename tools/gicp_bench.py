#!/usr/bin/env python3
"""Times generalized ICP on the HIP device beside the point-to-plane path, on the same build and clouds, at 100 000 and 1 000 000
rows.
  1. estimate_covariances beside estimate_normals (uniform box, max_nn = 20, the radius at which about half the rows are
     radius-limited: the median 19th-neighbour distance, taken from knn_k), and regularize_covariances of the result.
  2. one generalized update beside one point-to-plane update (Ps = Pt, the same correspondences), with the bytes a row moves -
     streamed: 12 point + 24 covariance + 4 index; gathered through the index: 12 point + 24 covariance (76 in all; the plane
     update's 12 + 4 + 12 + 12 = 40) - turned into GB/s of the median.  The ratio is reported, nothing is asserted.
  3. a full registration of a three-plane scene (normals_bench's: three tilted patches, the source other samples of them moved by
     a motion that slides along them), covariances or normals estimated inside the call, the default stopping rule:
     registration_generalized_icp beside registration_icp(estimation="point_to_plane"), with the iterations each took.
HIP events around each call, 5 warm-up calls, median of 30.  The Python calls include their allocations.  Each measurement runs
in a process of its own under `timeout`, so that one that hangs ends alone.
    python tools/gicp_bench.py [--out profiles/gicp_bench.json] [--sizes 100000,1000000]"""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-slam_amd"))

from normals_bench import BOX, REPS, STEP_LIMIT_S, WARMUP, box, median_ms, patches      # noqa: E402

GICP_BYTES_PER_ROW = 12 + 24 + 4 + 12 + 24
PLANE_BYTES_PER_ROW = 12 + 4 + 12 + 12


def step_covariances(P):
    import torch
    from scene_utils import estimate_covariances, estimate_normals, regularize_covariances
    from simple_knn import knn_k
    pts = box(P)
    radius = float(torch.sqrt(knn_k(pts, 19)[:, 18].median()))
    cov, count = estimate_covariances(pts, radius, 20, return_count=True)
    row = dict(points=P, max_nn=20, radius=radius, radius_limited_share=float((count < 20).float().mean()))
    row["estimate_normals"] = median_ms(lambda: estimate_normals(pts, radius, 20))
    row["estimate_covariances"] = median_ms(lambda: estimate_covariances(pts, radius, 20))
    row["regularize_covariances"] = median_ms(lambda: regularize_covariances(cov))
    row["covariances_over_normals"] = row["estimate_covariances"]["median_ms"] / row["estimate_normals"]["median_ms"]
    return row


def step_update(P):
    import torch
    from scene_utils import NeighborIndex, estimate_covariances, estimate_normals, gicp_update, icp_update
    tgt = box(P)
    src = (tgt[torch.randperm(P, generator=torch.Generator().manual_seed(1)).cuda()] + 0.002).contiguous()
    h = ((2 * BOX) ** 3 / P) ** (1.0 / 3.0)
    idx, _ = NeighborIndex(tgt).query(src, None, 5 * h)
    nrm = estimate_normals(tgt, 3 * h, 20)
    tcov = estimate_covariances(tgt, 3 * h, 20)
    scov = estimate_covariances(src, 3 * h, 20)
    row = dict(points=P, gicp_bytes_per_row=GICP_BYTES_PER_ROW, plane_bytes_per_row=PLANE_BYTES_PER_ROW)
    row["icp_update_plane"] = median_ms(lambda: icp_update(src, tgt, idx, None, target_normals=nrm))
    row["gicp_update"] = median_ms(lambda: gicp_update(src, scov, tgt, tcov, idx, None))
    row["generalized_over_plane"] = row["gicp_update"]["median_ms"] / row["icp_update_plane"]["median_ms"]
    row["gicp_update_gb_per_s"] = P * GICP_BYTES_PER_ROW / (row["gicp_update"]["median_ms"] * 1e-3) / 1e9
    row["icp_update_plane_gb_per_s"] = P * PLANE_BYTES_PER_ROW / (row["icp_update_plane"]["median_ms"] * 1e-3) / 1e9
    return row


def step_registration(P):
    import torch
    from scene_utils import registration_generalized_icp, registration_icp
    h = 0.02
    m = P // 3
    tgt = patches(m, 1, h)
    src = patches(m, 2, h)
    a = math.radians(1.0)
    T = torch.eye(4, dtype=torch.float64)
    T[0, 0], T[0, 1], T[1, 0], T[1, 1] = math.cos(a), -math.sin(a), math.sin(a), math.cos(a)
    T[:3, 3] = torch.tensor([1.2, -0.9, 0.8], dtype=torch.float64) * h
    src = ((src - T[:3, 3]) @ T[:3, :3]).float().cuda().contiguous()
    tgt = tgt.float().cuda().contiguous()
    md = 4 * h
    row = dict(source_points=int(src.shape[0]), target_points=int(tgt.shape[0]))
    runs = (("point_to_plane", lambda: registration_icp(src, tgt, md, estimation="point_to_plane", normal_radius=2.5 * h,
                                                        normal_max_nn=20)),
            ("generalized", lambda: registration_generalized_icp(src, tgt, md, covariance_radius=2.5 * h, covariance_max_nn=20)))
    for name, fn in runs:
        res = fn()
        row[name] = dict(iterations=res.iterations, converged=res.converged, fitness=res.fitness, inlier_rmse=res.inlier_rmse,
                         **median_ms(fn))
    row["generalized_over_plane"] = row["generalized"]["median_ms"] / row["point_to_plane"]["median_ms"]
    return row


STEPS = {"covariances": step_covariances, "update": step_update, "registration": step_registration}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gicp_bench.json"))
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)      # one measurement, in this process: "name:size"
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gicp_bench needs the HIP device: nothing is measured without it")
    if args.step:
        name, size = args.step.split(":")
        print("RESULT " + json.dumps(STEPS[name](int(size))), flush=True)
        return
    res = dict(device=torch.cuda.get_device_name(0), warmup=WARMUP, reps=REPS, covariances=[], update=[], registration=[])
    plan = [(name, int(s)) for name in STEPS for s in args.sizes.split(",")]
    for name, size in plan:
        p = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step",
                            f"{name}:{size}"], capture_output=True, text=True)
        if p.returncode != 0:      # a step that failed, faulted or hung: nothing more is started on the device
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit(f"gicp_bench: step {name}:{size} ended with status {p.returncode}")
        row = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        res[name].append(row)
        print(json.dumps({name: row}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
