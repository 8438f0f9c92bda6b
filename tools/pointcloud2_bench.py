#!/usr/bin/env python3
"""Times the PointCloud2 decode on the HIP device: gsr_pc2_decode (count pass, scan of the chunk counts, scatter pass) on 307 200
points - a 640 x 480 depth frame - in layout (a) (x / y / z / rgb FLOAT32, point_step 20) and layout (c) (point_step 19, fields at
1 / 5 / 9 / 13: unaligned in offset and stride), on buffers allocated once.  Each layout is timed on the LDS-staged path and on
the direct path (gsr_debug_pc2_force_direct), with everything kept (decode only) and with the reference's stages on (skip_nans,
height and range crop, pose).  Beside them, in the same run, a device-to-device copy of the same number of bytes: the yardstick
of a bandwidth-bound pass; the ratio is reported, nothing is asserted.  All of that twice: on ONE buffer, which stays in cache
from call to call, and "cold", on 96 copies taken in turn (0.59 GB: the copy a call reads was last touched 0.58 GB ago, twice
what the Infinity Cache holds).  Also scene_utils.decode_pointcloud2 as a user calls it, from host bytes (upload, allocations and
the read-back included) and from a device tensor.  Last, both paths with all stages on 2^24 points (a buffer larger than the
Infinity Cache), where the pass is bound by throughput and not by its launches.
HIP events around each call, 5 warm-up calls, median of 30.
    python tools/pointcloud2_bench.py [--out profiles/pointcloud2_bench.json]"""
import argparse
import ctypes as C
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-slam_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from diff_gaussian_rasterization import _C  # noqa: E402
from scene_utils import PointCloud2, decode_pointcloud2  # noqa: E402

WARMUP, REPS = 5, 30
N = 307200
COLD_COPIES = 96
LARGE_N = 1 << 24            # 16.8 M points: 336 / 319 MB of message, more than the Infinity Cache holds
LAYOUTS = {"a": (20, (0, 4, 8, 16), 7), "c": (19, (1, 5, 9, 13), 6)}      # point_step, offsets of x y z rgb, colour datatype


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


def message(name, N=N):
    """a depth camera's cloud: points in front of the sensor, 3 % invalid returns (NaN), colours in the low 24 bits"""
    step, offs, cdt = LAYOUTS[name]
    rng = np.random.default_rng(0)
    xyz = (rng.normal(0, 1.5, size=(N, 3)) + np.array([0.0, 0.5, 3.0])).astype(np.float32)
    xyz[rng.random(N) < 0.03] = np.nan
    rec = np.dtype({"names": ["x", "y", "z", "rgb"], "formats": ["<f4", "<f4", "<f4", "<u4"], "offsets": list(offs), "itemsize": step})
    buf = np.zeros(N, dtype=rec)
    buf["x"], buf["y"], buf["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    buf["rgb"] = rng.integers(0, 1 << 24, size=N).astype(np.uint32)
    fields = [(n, o, 7 if n != "rgb" else cdt, 1) for n, o in zip(("x", "y", "z", "rgb"), offs)]
    return PointCloud2(1, N, fields, False, step, N * step, buf.tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointcloud2_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pointcloud2_bench needs the HIP device: nothing is measured without it")
    lib = _C.lib()
    dev = torch.device("cuda", 0)
    res = dict(device=torch.cuda.get_device_name(0), warmup=WARMUP, reps=REPS, points=N, rows=[])
    T = torch.eye(4, dtype=torch.float64)
    T[0, 0], T[0, 2], T[2, 0], T[2, 2] = math.cos(0.3), math.sin(0.3), -math.sin(0.3), math.cos(0.3)
    T[:3, 3] = torch.tensor([1.0, 0.2, -0.5], dtype=torch.float64)
    Td = T.to(dev)
    out_p = torch.empty(N, 3, device=dev)
    out_c = torch.empty(N, 3, device=dev)
    out_i = torch.empty(N, dtype=torch.int32, device=dev)
    count = torch.zeros(2, dtype=torch.int64, device=dev)
    ws = torch.empty(lib.gsr_pc2_decode_workspace_bytes(N), dtype=torch.uint8, device=dev)
    for name, (step, offs, cdt) in LAYOUTS.items():
        msg = message(name)
        data = torch.from_numpy(np.frombuffer(msg.data, dtype=np.uint8).copy()).to(dev)
        copy_dst = torch.empty_like(data)
        L = _C.gsr_pc2_layout(N, 1, step, N * step, 0, (C.c_int32 * 3)(*offs[:3]), (C.c_int32 * 3)(7, 7, 7), offs[3], cdt)
        row = dict(layout=name, point_step=step, bytes=int(data.numel()))
        row["d2d_copy_same_bytes"] = median_ms(lambda: copy_dst.copy_(data))

        def decode(full, src=None):
            src = data if src is None else src
            _C.check(lib.gsr_pc2_decode(C.byref(L), _C.ptr(src), src.numel(), _C.ptr(Td) if full else None,
                                        -0.1 if full else -math.inf, 16.0 if full else math.inf, 1 if full else 0, _C.ptr(out_p),
                                        _C.ptr(out_c), _C.ptr(out_i), N, _C.ptr(count), _C.ptr(ws), ws.numel(), _C._stream()))
        for path, force in (("staged", 0), ("direct", 1)):
            lib.gsr_debug_pc2_force_direct(force)
            for stages, full in (("decode_only", False), ("nan_crop_pose", True)):
                row[f"{path}_{stages}"] = median_ms(lambda: decode(full))
                row[f"{path}_{stages}"]["kept"] = int(count.tolist()[0])
                row[f"{path}_{stages}_over_copy"] = row[f"{path}_{stages}"]["median_ms"] / row["d2d_copy_same_bytes"]["median_ms"]
        # cold: COLD_COPIES copies of the message, 0.59 GB together - twice the 256 MB Infinity Cache -, taken in turn, so that
        # every call reads bytes no cache holds any more
        ring = [data.clone() for _ in range(COLD_COPIES)]
        turn = [0]

        def cold(fn):
            turn[0] = (turn[0] + 1) % COLD_COPIES
            fn(ring[turn[0]])
        row["cold_bytes_in_rotation"] = COLD_COPIES * int(data.numel())
        row["cold_d2d_copy_same_bytes"] = median_ms(lambda: cold(lambda src: copy_dst.copy_(src)))
        for path, force in (("staged", 0), ("direct", 1)):
            lib.gsr_debug_pc2_force_direct(force)
            for stages, full in (("decode_only", False), ("nan_crop_pose", True)):
                key = f"cold_{path}_{stages}"
                row[key] = median_ms(lambda: cold(lambda src: decode(full, src)))
                row[key + "_over_copy"] = row[key]["median_ms"] / row["cold_d2d_copy_same_bytes"]["median_ms"]
        lib.gsr_debug_pc2_force_direct(0)
        row["cold_staged_over_direct_decode_only"] = row["cold_staged_decode_only"]["median_ms"] / row["cold_direct_decode_only"]["median_ms"]
        row["cold_staged_over_direct_nan_crop_pose"] = row["cold_staged_nan_crop_pose"]["median_ms"] / row["cold_direct_nan_crop_pose"]["median_ms"]
        del ring
        dev_msg = PointCloud2(1, N, msg.fields, False, step, N * step, data)
        row["python_from_host_bytes"] = median_ms(lambda: decode_pointcloud2(msg, transform=T, min_y=-0.1, max_range=4.0))
        row["python_from_device_tensor"] = median_ms(lambda: decode_pointcloud2(dev_msg, transform=T, min_y=-0.1, max_range=4.0))
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    del out_p, out_c, out_i, ws
    # where the pass is bound by throughput, not by its launches: LARGE_N points, a buffer larger than the Infinity Cache
    res["large"] = []
    for name, (step, offs, cdt) in LAYOUTS.items():
        msg = message(name, LARGE_N)
        data = torch.from_numpy(np.frombuffer(msg.data, dtype=np.uint8)).to(dev)
        del msg
        copy_dst = torch.empty_like(data)
        big_p, big_c = torch.empty(LARGE_N, 3, device=dev), torch.empty(LARGE_N, 3, device=dev)
        big_i = torch.empty(LARGE_N, dtype=torch.int32, device=dev)
        big_ws = torch.empty(lib.gsr_pc2_decode_workspace_bytes(LARGE_N), dtype=torch.uint8, device=dev)
        L = _C.gsr_pc2_layout(LARGE_N, 1, step, LARGE_N * step, 0, (C.c_int32 * 3)(*offs[:3]), (C.c_int32 * 3)(7, 7, 7), offs[3], cdt)

        def decode_large():
            _C.check(lib.gsr_pc2_decode(C.byref(L), _C.ptr(data), data.numel(), _C.ptr(Td), -0.1, 16.0, 1, _C.ptr(big_p),
                                        _C.ptr(big_c), _C.ptr(big_i), LARGE_N, _C.ptr(count), _C.ptr(big_ws), big_ws.numel(),
                                        _C._stream()))
        row = dict(layout=name, point_step=step, points=LARGE_N, bytes=int(data.numel()))
        row["d2d_copy_same_bytes"] = median_ms(lambda: copy_dst.copy_(data))
        for path, force in (("staged", 0), ("direct", 1)):
            lib.gsr_debug_pc2_force_direct(force)
            row[f"{path}_nan_crop_pose"] = median_ms(decode_large)
            row[f"{path}_nan_crop_pose"]["kept"] = int(count.tolist()[0])
            row[f"{path}_nan_crop_pose_over_copy"] = row[f"{path}_nan_crop_pose"]["median_ms"] / row["d2d_copy_same_bytes"]["median_ms"]
        lib.gsr_debug_pc2_force_direct(0)
        row["staged_over_direct"] = row["staged_nan_crop_pose"]["median_ms"] / row["direct_nan_crop_pose"]["median_ms"]
        res["large"].append(row)
        print(json.dumps(row), flush=True)
        del data, copy_dst, big_p, big_c, big_i, big_ws
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
