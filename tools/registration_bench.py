#!/usr/bin/env python3
"""Times the registration stage on the HIP device: the target index build, one neighbour search (with and without the Morton
`order` of the queries), one ICP update, and a 30-iteration registration with check_every = 1 and 0, at Ps = 307 200 source
points against Pt = 307 200 and 1 000 000 target points.  Beside them simple_knn.knn_k at k = 1 on the target alone (P = Pt): one
sweep over the same structure, the nearest existing yardstick; the ratio is reported, nothing is asserted.
HIP events around each call, 5 warm-up calls, median of 30.  Clouds: the uniform box; the source is a rigid copy of a sample of
the target (2 degrees, a shift of 0.3 mean spacings) so that a registration has something to do; relative_fitness =
relative_rmse = 0 keeps the check_every = 1 loop at its 30 iterations.  The Python calls include their allocations.
    python tools/registration_bench.py [--out profiles/registration_bench.json] [--targets 307200,1000000]"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-slam_amd"))
import torch  # noqa: E402
from scene_utils import NeighborIndex, icp_update, registration_icp  # noqa: E402
from simple_knn import knn_k  # noqa: E402

WARMUP, REPS = 5, 30
PS = 307200
BOX = 1.3


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


def clouds(Pt):
    g = torch.Generator().manual_seed(0)
    tgt = torch.rand(Pt, 3, generator=g) * (2 * BOX) - BOX
    h = ((2 * BOX) ** 3 / Pt) ** (1.0 / 3.0)
    a = math.radians(2.0)
    T = torch.eye(4, dtype=torch.float64)
    T[0, 0], T[0, 1], T[1, 0], T[1, 1] = math.cos(a), -math.sin(a), math.sin(a), math.cos(a)
    T[:3, 3] = torch.tensor([0.18, -0.19, 0.14], dtype=torch.float64) * h
    pick = torch.randperm(Pt, generator=g)[:PS] if Pt >= PS else torch.randint(0, Pt, (PS,), generator=g)
    src = ((tgt[pick].double() - T[:3, 3]) @ T[:3, :3]).float()      # T src = the sampled target rows
    return src.cuda().contiguous(), tgt.cuda().contiguous(), h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "registration_bench.json"))
    ap.add_argument("--targets", default="307200,1000000")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("registration_bench needs the HIP device: nothing is measured without it")
    res = dict(device=torch.cuda.get_device_name(0), warmup=WARMUP, reps=REPS, source_points=PS, rows=[])
    for Pt in [int(s) for s in args.targets.split(",")]:
        src, tgt, h = clouds(Pt)
        md = 5.0 * h
        row = dict(target_points=Pt, source_points=PS, max_correspondence_distance=md)
        row["index_build"] = median_ms(lambda: NeighborIndex(tgt))
        index = NeighborIndex(tgt)
        order = index.query_order(src)
        row["query_order"] = median_ms(lambda: index.query_order(src))
        row["search_plain"] = median_ms(lambda: index.query(src, None, md))
        row["search_ordered"] = median_ms(lambda: index.query(src, None, md, order=order))
        row["search_unbounded_ordered"] = median_ms(lambda: index.query(src, None, math.inf, order=order))
        row["order_speedup"] = row["search_plain"]["median_ms"] / row["search_ordered"]["median_ms"]
        idx, _ = index.query(src, None, md, order=order)
        row["icp_update"] = median_ms(lambda: icp_update(src, tgt, idx, None))
        row["knn_k_1_on_target"] = median_ms(lambda: knn_k(tgt, 1))
        # per query: the cross search answers Ps rows, knn_k answers Pt (and sorts the cloud first)
        row["search_over_knn_k_1_per_query"] = (row["search_ordered"]["median_ms"] / PS) / (row["knn_k_1_on_target"]["median_ms"] / Pt)
        for ce in (1, 0):
            def call():
                return registration_icp(src, None, md, relative_fitness=0.0, relative_rmse=0.0, max_iteration=30, check_every=ce,
                                        index=index)
            r = call()
            row[f"icp_30_check_every_{ce}"] = dict(**median_ms(call), iterations=r.iterations, fitness=r.fitness,
                                                    inlier_rmse=r.inlier_rmse)
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        del src, tgt, index
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
