#!/usr/bin/env python3
"""Times scene_utils.decode_image (rgb8, bayer_rggb8, 16UC1) and scene_utils.register_depth on the HIP device at 640 x 480 and
1920 x 1080: HIP events around each call, warm-up, medians.  Each is reported as a time and as achieved bytes per second - the
bytes the operation has to move (message bytes read + float32 planes written; for the registration the depth read, and the
colour-sized integer buffer written, read and written out again), computed from the shapes - beside the equivalent chain of
PyTorch ops on the same device (uint8 view -> reshape -> permute -> float -> divide) and beside the 6.0 TB/s plain-stream
figure of DESIGN.md section 8 item 4.  The end-to-end call includes the Python wrapper and the allocation of the output; a
second, separately run pass with the library's per-kernel event timing on (gsr_profile_enable) gives the kernels alone.
    python tools/image_decode_bench.py [--out profiles/image_decode_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-slam_amd"))
import torch  # noqa: E402
from diff_gaussian_rasterization import _C  # noqa: E402
from scene_utils import decode_image, register_depth  # noqa: E402
from scene_utils.messages import Image  # noqa: E402

STREAM_TBPS = 6.0      # a plain stream on this device
SIZES = [(640, 480), (1920, 1080)]


def median_ms(fn, warmup=5, reps=41):
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


def kernels_ms(fn):
    """one profiled call: the sum of the library's kernels (events around every launch: not the end-to-end time)"""
    lib = _C.lib()
    fn()
    torch.cuda.synchronize()
    lib.gsr_profile_reset()
    lib.gsr_profile_enable(1)
    fn()
    torch.cuda.synchronize()
    lib.gsr_profile_enable(0)
    return {k: v[0] for k, v in _C.profile_read().items() if k.startswith(("image_", "depth_register"))}


def message(encoding, W, H, bpp, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if encoding == "16UC1":      # 0.3 .. 6 m in millimetres, little-endian
        mm = torch.randint(300, 6000, (H, W), device="cuda", generator=g, dtype=torch.int32).to(torch.int16)
        data = mm.view(torch.uint8).reshape(-1)
    else:
        data = torch.randint(0, 256, (H * W * bpp,), device="cuda", generator=g, dtype=torch.uint8)
    return Image(H, W, encoding, False, W * bpp, data)


def torch_rgb8(msg):
    return (msg.data.view(msg.height, msg.width, 3).permute(2, 0, 1).float() / 255.0).contiguous()


def torch_depth16(msg):
    return msg.data.view(torch.int16).view(msg.height, msg.width).float() * 0.001


def row(what, W, H, nbytes, fn, baseline=None):
    med, lo, hi = median_ms(fn)
    ker = kernels_ms(fn)
    ksum = sum(ker.values())
    r = dict(what=what, W=W, H=H, bytes=nbytes, median_ms=med, min_ms=lo, max_ms=hi, GBps=nbytes / (med * 1e6),
             kernels_ms=ker, kernels_GBps=(nbytes / (ksum * 1e6) if ksum else None),
             kernels_share_of_stream=(nbytes / (ksum * 1e-3) / (STREAM_TBPS * 1e12) if ksum else None))
    if baseline is not None:
        bmed, blo, bhi = median_ms(baseline)
        r.update(torch_median_ms=bmed, torch_min_ms=blo, torch_max_ms=bhi, torch_GBps=nbytes / (bmed * 1e6))
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_decode_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_decode_bench needs the HIP device: nothing is measured without it")
    res = dict(device=torch.cuda.get_device_name(0), stream_TBps=STREAM_TBPS, rows=[],
               note="median_ms: the whole Python call (wrapper, output allocation, launch); kernels_ms: the library's kernels alone, "
                    "from a separate profiled call; torch_*: the chain of PyTorch ops on the same message")
    empty = torch.empty(0, device="cuda")
    res["empty_launch_ms"] = median_ms(lambda: empty.zero_())[0]      # what one (empty) PyTorch launch costs between two events
    for W, H in SIZES:
        n = W * H
        rgb, bayer, d16 = message("rgb8", W, H, 3, 1), message("bayer_rggb8", W, H, 1, 2), message("16UC1", W, H, 2, 3)
        res["rows"].append(row("decode_image rgb8", W, H, n * (3 + 12), lambda: decode_image(rgb), lambda: torch_rgb8(rgb)))
        res["rows"].append(row("decode_image bayer_rggb8", W, H, n * (1 + 12), lambda: decode_image(bayer)))
        res["rows"].append(row("decode_image 16UC1", W, H, n * (2 + 4), lambda: decode_image(d16), lambda: torch_depth16(d16)))
        depth = decode_image(d16)
        Kd, Kc = (0.66 * W, 0.66 * W, 0.5 * W - 0.7, 0.5 * H + 0.4), (0.96 * W, 0.96 * W, 0.5 * W + 1.1, 0.5 * H - 0.6)
        T = torch.eye(4, dtype=torch.float64)
        T[0, 3] = 0.015
        # depth read (4) + buffer cleared (4), read and written out (8); the atomics touch every colour pixel ~2 times more
        res["rows"].append(row("register_depth", W, H, n * (4 + 4 + 8), lambda: register_depth(depth, Kd, Kc, T)))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
