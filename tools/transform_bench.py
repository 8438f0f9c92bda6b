"""Times gsr_transform_gaussians (csrc/transform.hip) at map size against a device-to-device copy of the bytes it must move.

    python tools/transform_bench.py [--P 1000000] [--reps 30] [--out profiles/transform.txt]

Per case (K = 1 without anchors, K = 64 with random anchors; with and without the eight moment pointers): HIP-event time of the
call through the C ABI, median and min..max over `reps` after a warm-up, and in the same process the same statistics for
torch.clone of the four tensors the call reads and writes (xyz, rotation, scaling, features_rest: the same bytes in, the same
bytes out) plus, with moments, zero_() of the eight moment tensors (the same bytes written)."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-slam_amd"))

from diff_gaussian_rasterization import _C  # noqa: E402
from scene_utils import make_gaussians  # noqa: E402


def timed(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms = np.array(ms)
    return float(np.median(ms)), float(ms.min()), float(ms.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    P, lib = a.P, _C.lib()
    raw = make_gaussians(P, 3, seed=1).to("cuda")
    params = [raw.xyz.contiguous(), raw.rotation.contiguous(), raw.scaling.contiguous(), raw.features_rest.contiguous()]
    moments = [torch.rand_like(p) for p in params for _ in range(2)]
    row_bytes = sum(p.numel() * 4 for p in params) // P
    lines = [f"gsr_transform_gaussians, P = {P}, SH degree 3 ({row_bytes} B of a row are read and written; f_dc and opacity are not touched)",
             f"device: {torch.cuda.get_device_name(0)}; HIP events, median (min..max) of {a.reps} after 5 warm-up calls", ""]
    rng = np.random.default_rng(0)
    for K in (1, 64):
        T = np.tile(np.eye(4), (K, 1, 1))
        for k in range(K):                                   # rotations only: repeated calls keep the values bounded
            ax = rng.normal(size=3)
            ax /= np.linalg.norm(ax)
            Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
            T[k, :3, :3] = np.eye(3) + np.sin(1.0) * Kx + (1 - np.cos(1.0)) * (Kx @ Kx)
        Td = torch.tensor(T).cuda()
        anchor = None if K == 1 else torch.randint(0, K, (P,), dtype=torch.int32, device="cuda")
        ws = torch.empty(lib.gsr_transform_workspace_bytes(K), dtype=torch.uint8, device="cuda")
        for with_m in (False, True):
            mom8 = (C.c_void_p * 8)(*[m.data_ptr() for m in moments]) if with_m else None

            def call():
                _C.check(lib.gsr_transform_gaussians(P, _C.ptr(anchor), K, _C.ptr(Td), _C.ptr(ws), ws.numel(), _C.ptr(params[0]),
                                                     _C.ptr(params[1]), _C.ptr(params[2]), _C.ptr(params[3]), 15, mom8,
                                                     _C._stream()))

            def copy():
                for p in params:
                    p.clone()
                if with_m:
                    for m in moments:
                        m.zero_()
            nbytes = P * row_bytes * 2 + (P * 4 if K > 1 else 0) + (P * row_bytes * 2 if with_m else 0)
            k_med, k_lo, k_hi = timed(call, a.reps)
            c_med, c_lo, c_hi = timed(copy, a.reps)
            lines.append(f"K = {K:2d} {'anchors' if K > 1 else 'all rows'}, moments {'reset' if with_m else 'kept '}: "
                         f"{nbytes / 1e6:7.1f} MB  kernel {k_med:.3f} ms ({k_lo:.3f}..{k_hi:.3f}) = {nbytes / k_med / 1e6:6.0f} GB/s | "
                         f"copy {c_med:.3f} ms ({c_lo:.3f}..{c_hi:.3f}) = {nbytes / c_med / 1e6:6.0f} GB/s | "
                         f"kernel / copy rate = {c_med / k_med:.2f}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
