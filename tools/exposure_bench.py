"""Forward + backward of the per-view exposure affine (scene_utils.apply_exposure, csrc/exposure.hip) against the torch expression
render() ran before it, on the same tensors: HIP events, both forms alternating in one process, then the device launches of each
in a profiler pass of its own.  `python tools/exposure_bench.py [--out FILE]` -> profiles/exposure.txt."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gaussian-splatting-slam_amd")):
    sys.path.insert(0, p)
import torch
from scene_utils import apply_exposure

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the lines to this file (rewritten after every line)")
OUT = ap.parse_args().out
if OUT and os.path.dirname(OUT):
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    if OUT:
        with open(OUT, "w") as f:
            f.write("\n".join(lines) + "\n")


def torch_form(img, E):
    return torch.matmul(img.permute(1, 2, 0), E[:3, :3]).permute(2, 0, 1) + E[:3, 3, None, None]


def hip_form(img, E):
    return apply_exposure(img, E)


def one(fn, img, E, g):
    img.grad = None
    E.grad = None
    fn(img, E).backward(g)


def timed(fn, img, E, g, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        one(fn, img, E, g)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters     # us per forward + backward


assert torch.cuda.is_available()
say(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
gen = torch.Generator().manual_seed(3)
E0 = torch.eye(3, 4) + 0.3 * torch.randn(3, 4, generator=gen)
for (W, H) in ((1920, 1080), (640, 480)):
    img = torch.rand(3, H, W, generator=gen).cuda().requires_grad_(True)
    g = torch.randn(3, H, W, generator=gen).cuda()
    E = E0.cuda().requires_grad_(True)
    # same results first (the two forms on the same tensors)
    one(torch_form, img, E, g)
    ref = (torch_form(img, E).detach().clone(), img.grad.clone(), E.grad.clone())
    one(hip_form, img, E, g)
    got = (hip_form(img, E).detach().clone(), img.grad.clone(), E.grad.clone())
    say(f"{W}x{H}: max |hip - torch| forward {(got[0] - ref[0]).abs().max().item():.2e}, dL/dimage "
        f"{(got[1] - ref[1]).abs().max().item():.2e}, dL/dexposure rel {((got[2] - ref[2]).abs().max() / ref[2].abs().max()).item():.2e}")
    iters = 300
    for fn in (torch_form, hip_form):
        timed(fn, img, E, g, 50)                  # warm-up of both forms at this shape
    rounds = {"torch": [], "hip": []}
    for r in range(9):
        for name, fn in (("torch", torch_form), ("hip", hip_form)) if r % 2 == 0 else (("hip", hip_form), ("torch", torch_form)):
            rounds[name].append(timed(fn, img, E, g, iters))
    for name in ("torch", "hip"):
        v = rounds[name]
        say(f"{W}x{H} {name:5s} forward+backward, us per call over {iters} calls x {len(v)} alternating rounds (host enqueue "
            f"included): median {statistics.median(v):.1f}  min {min(v):.1f}  max {max(v):.1f}")
    say(f"{W}x{H} ratio torch / hip (medians): {statistics.median(rounds['torch']) / statistics.median(rounds['hip']):.2f}")
    # bytes the HIP form moves: forward 3 planes in + 3 out, backward 6 in + 3 out
    n = W * H
    say(f"{W}x{H} algorithmic bytes: forward {24 * n / 1e6:.1f} MB, backward {36 * n / 1e6:.1f} MB")

# launch counts, in a pass of their own (the profiler slows the host)
try:
    from torch.profiler import profile, ProfilerActivity
    img = torch.rand(3, 480, 640, generator=gen).cuda().requires_grad_(True)
    g = torch.randn(3, 480, 640, generator=gen).cuda()
    E = E0.cuda().requires_grad_(True)
    for name, fn in (("torch", torch_form), ("hip", hip_form)):
        one(fn, img, E, g)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            img.grad = None
            E.grad = None
            out = fn(img, E)
            torch.cuda.synchronize()
            out.backward(g)
            torch.cuda.synchronize()
        kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        names = [e.name for e in kernels]
        say(f"{name}: {len(names)} device launches per forward + backward: " + "; ".join(n[:60] for n in names))
except Exception as ex:       # noqa: BLE001
    say(f"launch counts: not measured ({type(ex).__name__}: {ex})")
say("done")
