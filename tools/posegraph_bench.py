"""Times PoseGraph.optimize (one launch of one workgroup, csrc/posegraph.hip) on a ring of N nodes with 2 loop edges per 16
nodes, started from the truth moved by 5 cm / 2 degrees per node (drift chained over hundreds of nodes would saturate every loop
edge at mu and leave the optimiser nothing to do): `python tools/posegraph_bench.py [N ...]` prints one line per size; run each size as its own process under `timeout`.
Warm-up launches first, then HIP events around the launch alone (the topology and the stacked edges are built before); the
median of the repeats and the spread are printed.  Nothing is gated on these figures."""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gaussian-splatting-slam_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import posegraph_reference as PR      # noqa: E402
import scene_utils as S               # noqa: E402


def ring(n, seed=0):
    rng = np.random.default_rng(seed)
    truth = PR.ring_truth(n, radius=n / 8.0)
    g = S.PoseGraph()
    g.add_node(truth[0], fixed=True)
    for i in range(1, n):
        g.add_node(PR._noise(rng, 0.05, 2.0) @ truth[i])
    for i in range(n - 1):      # odometry with 1 cm / 0.5 degree noise
        g.add_edge(i, i + 1, PR.relative(truth[i + 1], truth[i]) @ PR._noise(rng, 0.01, 0.5), PR.INFO)
    for b in range(0, n, 16):
        for a, c in ((b, (b + n // 2) % n), (b + 5, (b + 5 + n // 3) % n)):
            if a != c and (a, c) not in g._pairs and (c, a) not in g._pairs:
                g.add_edge(a, c, PR.relative(truth[c], truth[a]) @ PR._noise(rng, 0.01, 0.5), PR.INFO, uncertain=True)
    return g


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [64, 512, 4096]
    for n in sizes:
        g = ring(n)
        X0 = g.poses.clone()
        times, res = [], None
        warm, reps = (3, 10) if n <= 512 else (1, 3)      # (the largest ring runs for seconds)
        for rep in range(warm + reps):
            g._X = X0.clone()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            res = g.optimize(line_process_weight=0.25)
            b.record()
            torch.cuda.synchronize()
            if rep >= warm:
                times.append(a.elapsed_time(b))
        per = statistics.median(times) / max(res.cg_iterations, 1)
        print(f"posegraph ring N={n} E={len(g.edges)}: optimize median {statistics.median(times):.3f} ms (min {min(times):.3f}, max "
              f"{max(times):.3f}, {reps} repeats after {warm} warm-ups; includes the read-back of the 16 statistics), status {res.status}, "
              f"{res.iterations} solves, {res.accepted} accepted, {res.cg_iterations} PCG products ({1e3 * per:.1f} us of the whole "
              f"launch per product), F {res.residual_start:.4g} -> {res.residual_end:.4g}", flush=True)


if __name__ == "__main__":
    main()
