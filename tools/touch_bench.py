#!/usr/bin/env python3
"""Cost of the per-Gaussian visibility counts (render(..., n_touched=True)) at BASELINE configs[3]
(1 M Gaussians, 1080p), one view, forward-only render under torch.no_grad():
   (a) plain;  (b) n_touched at touched_T_min = 0.5;  (c) n_touched at touched_T_min = 0 (every blended pair is counted).
The three are INTERLEAVED (a, b, c, a, b, c, ...) so that clock and thermal drift hits them alike; medians of --iters timed
repetitions of the whole forward (HIP events around the call), then, in a second interleaved pass with the library's per-kernel
profiling on, the mean time of the compositing kernel alone (`render_fwd`).  Prints one JSON line and writes it, with a short
header, to profiles/n_touched_c3.txt.
    python tools/touch_bench.py [--iters N] [--out PATH]   (GPU box, repo root)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-slam_amd"))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "n_touched_c3.txt"))
    a = ap.parse_args()
    from scene_utils import make_config, GaussianModel
    from gaussian_renderer import render, PipelineParams
    from diff_gaussian_rasterization import _C
    dev = "cuda"
    raw, cams, cfg = make_config(3, views=2)
    cam = cams[0].to(dev)
    pipe, bg = PipelineParams(), torch.zeros(3, device=dev)
    model = GaussianModel.from_raw(raw.to(dev), requires_grad=False)
    variants = [("plain", {}), ("n_touched_T0.5", dict(n_touched=True, touched_T_min=0.5)),
                ("n_touched_T0", dict(n_touched=True, touched_T_min=0.0))]

    def run(kw):
        with torch.no_grad():
            return render(cam, model, pipe, bg, **kw)

    for _ in range(a.warmup):
        for _, kw in variants:
            run(kw)
    torch.cuda.synchronize()
    ts = {name: [] for name, _ in variants}
    for _ in range(a.iters):
        for name, kw in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(kw)
            e1.record()
            e1.synchronize()
            ts[name].append(e0.elapsed_time(e1))
    out = {"config": 3, "P": cfg["P"], "W": cfg["W"], "H": cfg["H"], "iters": a.iters}
    for name, v in ts.items():
        v.sort()
        out[f"forward_ms_{name}"] = round(v[len(v) // 2], 4)
        out[f"forward_ms_{name}_min_max"] = [round(v[0], 4), round(v[-1], 4)]
    # the compositing kernel alone: the library's per-kernel events, one variant at a time between resets, still interleaved
    lib = _C.lib()
    lib.gsr_profile_enable(1)
    kt = {name: [0.0, 0] for name, _ in variants}
    for _ in range(a.iters):
        for name, kw in variants:
            lib.gsr_profile_reset()
            run(kw)
            torch.cuda.synchronize()
            ms, calls = _C.profile_read().get("render_fwd", (0.0, 0))
            kt[name][0] += ms
            kt[name][1] += calls
    lib.gsr_profile_enable(0)
    for name, (ms, calls) in kt.items():
        out[f"render_fwd_kernel_ms_{name}"] = round(ms / max(calls, 1), 4)
    n5 = run(variants[1][1])
    n0 = run(variants[2][1])
    out["radii_gt0"] = int((n5["radii"] > 0).sum())
    out["touched_rows_T0.5"] = int((n5["n_touched"] > 0).sum())
    out["touched_rows_T0"] = int((n0["n_touched"] > 0).sum())
    out["counted_pairs_T0.5"] = int(n5["n_touched"].sum(dtype=torch.int64))
    out["counted_pairs_T0"] = int(n0["n_touched"].sum(dtype=torch.int64))
    line = json.dumps(out)
    print(line)
    with open(a.out, "w") as f:
        f.write("# tools/touch_bench.py: forward-only render at configs[3] with and without n_touched, interleaved, medians (ms)\n")
        f.write(line + "\n")


if __name__ == "__main__":
    main()
