#!/usr/bin/env python3
"""Times normal estimation and the point-to-plane update on the HIP device.
  1. estimate_normals at P = 307 200 and 1 000 000 (uniform box, max_nn = 30, the radius at which about half the rows are
     radius-limited: the median 29th-neighbour distance, taken from knn_k) beside simple_knn.knn_k(k = 29) on the same cloud -
     the kernel that does the same first sweep; the ratio is reported, nothing is asserted.
  2. one point-to-plane update beside one point-to-point update (Ps = Pt = 307 200).
  3. a three-plane scene (three tilted patches, the source other samples of them moved by a motion that slides along them):
     the number of updates after which each estimator's transformation has the RMSE the point-to-point run stops at (one pass,
     the RMSE read back every iteration), and the milliseconds of a registration of that many iterations.
HIP events around each call, 5 warm-up calls, median of 30.  The Python calls include their allocations.  Each measurement runs
in a process of its own under `timeout`, so that one that hangs ends alone.
    python tools/normals_bench.py [--out profiles/normals_bench.json] [--sizes 307200,1000000]"""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-slam_amd"))

WARMUP, REPS = 5, 30
BOX = 1.3
STEP_LIMIT_S = 240


def median_ms(fn):
    import torch
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


def box(P, seed=0):
    import torch
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(P, 3, generator=g) * (2 * BOX) - BOX).cuda().contiguous()


def step_normals(P):
    import torch
    from scene_utils import estimate_normals
    from simple_knn import knn_k
    pts = box(P)
    d29 = knn_k(pts, 29)[:, 28]
    radius = float(torch.sqrt(d29.median()))
    _, count, _ = estimate_normals(pts, radius, 30, return_stats=True)
    row = dict(points=P, max_nn=30, radius=radius, radius_limited_share=float((count < 30).float().mean()))
    row["knn_k_29"] = median_ms(lambda: knn_k(pts, 29))
    row["estimate_normals"] = median_ms(lambda: estimate_normals(pts, radius, 30))
    row["estimate_normals_count_limited"] = median_ms(lambda: estimate_normals(pts, math.inf, 30))
    row["normals_over_knn_k_29"] = row["estimate_normals"]["median_ms"] / row["knn_k_29"]["median_ms"]
    return row


def step_update(P):
    import torch
    from scene_utils import NeighborIndex, estimate_normals, icp_update
    tgt = box(P)
    src = (tgt[torch.randperm(P, generator=torch.Generator().manual_seed(1)).cuda()] + 0.002).contiguous()
    h = ((2 * BOX) ** 3 / P) ** (1.0 / 3.0)
    idx, _ = NeighborIndex(tgt).query(src, None, 5 * h)
    nrm = estimate_normals(tgt, 3 * h, 30)
    row = dict(points=P)
    row["icp_update_point"] = median_ms(lambda: icp_update(src, tgt, idx, None))
    row["icp_update_plane"] = median_ms(lambda: icp_update(src, tgt, idx, None, target_normals=nrm))
    row["plane_over_point"] = row["icp_update_plane"]["median_ms"] / row["icp_update_point"]["median_ms"]
    return row


def patches(m, seed, h):
    """three tilted square patches of m jittered grid rows each, apart from each other"""
    import torch
    g = torch.Generator().manual_seed(seed)
    side = int(math.ceil(math.sqrt(m)))
    ij = torch.stack(torch.meshgrid(torch.arange(side), torch.arange(side), indexing="ij"), dim=-1).reshape(-1, 2)[:m].double()
    out = []
    for o, n in (([0.0, 0.0, 0.0], [0.1, 0.15, 1.0]), ([-0.3, 0.1, 0.3], [1.0, 0.2, -0.1]), ([0.1, -0.3, 0.4], [-0.15, 1.0, 0.2])):
        n = torch.tensor(n, dtype=torch.float64)
        n = n / n.norm()
        a = torch.linalg.cross(n, torch.tensor([1.0, 0.0, 0.0] if abs(float(n[0])) < 0.9 else [0.0, 1.0, 0.0], dtype=torch.float64))
        a = a / a.norm()
        b = torch.linalg.cross(n, a)
        uv = (ij + torch.rand(m, 2, generator=g, dtype=torch.float64) * 0.6 - 0.3) * h
        out.append(torch.tensor(o, dtype=torch.float64) * (side * h / 0.8) + uv[:, :1] * a + uv[:, 1:] * b)
    return torch.cat(out)


def step_scene(m):
    import torch
    from scene_utils import NeighborIndex, estimate_normals, icp_update, registration_icp
    h = 0.02
    tgt = patches(m, 1, h)
    src = patches(m, 2, h)
    a = math.radians(1.0)
    T = torch.eye(4, dtype=torch.float64)
    T[0, 0], T[0, 1], T[1, 0], T[1, 1] = math.cos(a), -math.sin(a), math.sin(a), math.cos(a)
    T[:3, 3] = torch.tensor([1.2, -0.9, 0.8], dtype=torch.float64) * h
    src = ((src - T[:3, 3]) @ T[:3, :3]).float().cuda().contiguous()
    tgt = tgt.float().cuda().contiguous()
    md = 4 * h
    index = NeighborIndex(tgt)
    nrm = estimate_normals(tgt, 2.5 * h, 30)
    point = registration_icp(src, None, md, max_iteration=200, index=index)
    goal = point.inlier_rmse
    row = dict(source_points=int(src.shape[0]), target_points=int(tgt.shape[0]), goal_rmse=goal,
               point_to_point_stopped_after=point.iterations)
    for name, normals in (("point_to_point", None), ("point_to_plane", nrm)):
        # one pass of at most 200 iterations, the RMSE of every incoming T read back: the first T that is at the goal
        T = torch.eye(4, dtype=torch.float64, device="cuda")
        need, rmse = None, float("nan")
        for it in range(201):
            idx, _ = index.query(src, T, md)
            T, stats = icp_update(src, tgt, idx, T, target_normals=normals)
            rmse = float(stats[2])
            if rmse <= goal * (1 + 1e-9):
                need = it
                break
        kw = {} if normals is None else dict(estimation="point_to_plane", target_normals=normals)
        iters = max(need or 200, 1)
        t = median_ms(lambda: registration_icp(src, None, md, relative_fitness=0.0, relative_rmse=0.0, max_iteration=iters,
                                               check_every=0, index=index, **kw))
        row[name] = dict(iterations_to_goal=need, inlier_rmse=rmse, **t)
    return row


STEPS = {"normals": step_normals, "update": step_update, "scene": step_scene}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals_bench.json"))
    ap.add_argument("--sizes", default="307200,1000000")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)      # one measurement, in this process: "name:size"
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("normals_bench needs the HIP device: nothing is measured without it")
    if args.step:
        name, size = args.step.split(":")
        print("RESULT " + json.dumps(STEPS[name](int(size))), flush=True)
        return
    res = dict(device=torch.cuda.get_device_name(0), warmup=WARMUP, reps=REPS, normals=[], update=[], scene=[])
    plan = [("normals", int(s)) for s in args.sizes.split(",")] + [("update", 307200), ("scene", 40000)]
    for name, size in plan:
        p = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step",
                            f"{name}:{size}"], capture_output=True, text=True)
        if p.returncode != 0:      # a step that failed, faulted or hung: nothing more is started on the device
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit(f"normals_bench: step {name}:{size} ended with status {p.returncode}")
        row = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        res[name].append(row)
        print(json.dumps({name: row}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
