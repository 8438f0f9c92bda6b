#!/usr/bin/env python3
"""Times the two scan-context kernels on the HIP device at the default geometry (20 rings x 60 sectors):
  1. scan_context of one 100 000-point scan, from one origin and from three (the memset, the binning launch, the norms launch and
     the Python call's two allocations);
  2. ScanDatabase.distances of that context, one variant and three, against 10 000 stored descriptors of random heights (every
     column takes part: the most work a row can be).
HIP events around each call, 10 warm-up calls, median / min / max of 50.  Recorded in profiles/README.md; nothing is asserted.
    python tools/scancontext_bench.py [--out profiles/scancontext_bench.json] [--points 100000] [--rows 10000]"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-slam_amd"))

WARMUP, REPS = 10, 50


def timed(fn):
    import torch
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--rows", type=int, default=10000)
    args = ap.parse_args()
    import torch
    from scene_utils import ScanDatabase, ScanEntry, scan_context
    g = torch.Generator().manual_seed(1)
    rho = 80.0 * torch.sqrt(torch.rand(args.points, generator=g))
    theta = 2.0 * math.pi * torch.rand(args.points, generator=g)
    pts = torch.stack([rho * torch.cos(theta), rho * torch.sin(theta), 9.0 * torch.rand(args.points, generator=g) - 3.0], dim=1).cuda()
    lanes = [[0.0, 0.0, 0.0], [0.0, -2.0, 0.0], [0.0, 2.0, 0.0]]
    out = dict(points=args.points, rows=args.rows, rings=20, sectors=60, warmup=WARMUP, reps=REPS)
    db = ScanDatabase("cuda")
    d = (8.0 * torch.rand(args.rows, 20, 60, generator=g)).cuda()
    db._desc, db._norms = d, torch.sqrt((d * d).sum(dim=1))      # (filled in place: 10 000 add() calls are not what is timed)
    db._entries = [ScanEntry(i, None, None) for i in range(args.rows)]
    for B in (1, 3):
        out[f"scan_context_B{B}"] = timed(lambda: scan_context(pts, origins=lanes[:B]))
        ctx = scan_context(pts, origins=lanes[:B])
        out[f"distances_B{B}"] = timed(lambda: db.distances(ctx))
    print(json.dumps(out, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
