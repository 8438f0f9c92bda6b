"""Measurements behind profiles/colored_icp.txt: gsr_color_gradient against gsr_estimate_normals and gsr_icp_update_colored against
gsr_icp_update_plane, interleaved rounds in one process (device events), and the end-to-end plane scene of
tests/colored_reference.py under every estimator (wall time around a synchronise).
    python tools/colored_icp_bench.py [OUTPUT.txt]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: F401,E402  (paths)
import colored_reference as CR  # noqa: E402
import normals_reference as NR  # noqa: E402
import scene_utils as S  # noqa: E402

out = open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def timed(fns, rounds=20, warm=3):
    """interleaved rounds; per function the list of device-event milliseconds"""
    for _ in range(warm):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(rounds):
        for k, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return [(float(np.median(m)), float(np.min(m))) for m in ms]


dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
say("device", torch.cuda.get_device_name(0))

# 1. colour gradient against normals at 307 200 rows (a 640 x 480 jittered surface with gentle relief, spacing 0.01)
rng = np.random.default_rng(1)
h = 0.01
gy, gx = np.mgrid[0:480, 0:640]
uv = (np.stack([gx.ravel(), gy.ravel()], axis=1) + rng.uniform(-0.3, 0.3, size=(307200, 2))) * h
pts = np.concatenate([uv, (0.05 * np.sin(uv[:, :1] * 3) * np.cos(uv[:, 1:] * 2))], axis=1).astype(np.float32)
pts = pts[rng.permutation(307200)]
cols = CR.texture(pts, 12 * h)
P = pts.shape[0]
p, c = dev(pts), dev(cols)
for radius, nn in ((2.5 * h, 30), (float("inf"), 30), (2.5 * h, 9)):
    nrm = S.estimate_normals(p, radius, max(nn, 4))
    (n_med, n_min), (g_med, g_min) = timed([lambda: S.estimate_normals(p, radius, nn),
                                            lambda: S.estimate_color_gradients(p, c, nrm, radius, nn)])
    _, count, status = S.estimate_color_gradients(p, c, nrm, radius, nn, return_stats=True)
    say(f"P={P} radius={radius / h:.3g} spacings max_nn={nn}: estimate_normals {n_med:.3f} ms (min {n_min:.3f}), "
        f"estimate_color_gradients {g_med:.3f} ms (min {g_min:.3f}), ratio {g_med / n_med:.3f}; mean count "
        f"{float(count.float().mean()):.1f}, status {torch.bincount(status.int(), minlength=4).tolist()}")

# 2. the coloured update against the plane update at the same Ps
radius, nn = 2.5 * h, 30
nrm = S.estimate_normals(p, radius, nn)
grd = S.estimate_color_gradients(p, c, nrm, radius, nn)
T0 = torch.from_numpy(CR.RR.rigid_about([3.2, 2.4, 0], [0.1, 0.2, 1.0], 0.002, [0.3 * h, -0.2 * h, 0.1 * h]))
for Ps in (307200, 65536, 4096):
    s = p[:Ps].contiguous()
    sc = c[:Ps].contiguous()
    idx, _ = S.NeighborIndex(p).query(s, T0, 3 * h)
    from scene_utils.registration import _Updater
    Td = T0.cuda()
    st = torch.zeros(8, dtype=torch.float64, device="cuda")
    up, uc = _Updater(s, p, nrm), _Updater(s, p, nrm, (sc, c, grd, 0.968))
    (p_med, p_min), (c_med, c_min) = timed([lambda: up(idx, Td.clone(), st), lambda: uc(idx, Td.clone(), st)], rounds=50)
    say(f"Ps={Ps}: gsr_icp_update_plane {p_med * 1e3:.1f} us (min {p_min * 1e3:.1f}), gsr_icp_update_colored {c_med * 1e3:.1f} us "
        f"(min {c_min * 1e3:.1f}), ratio {c_med / p_med:.3f}  (each with one 128-byte clone of T)")

# 3. the end-to-end scene: iterations and wall time
src, scol, tgt, tcol, T_true, md = CR.plane_scene()
a, ac, b, bc = dev(src), dev(scol), dev(tgt), dev(tcol)
nrm = S.estimate_normals(b, CR.PLANE_RADIUS, 30)
grd = S.estimate_color_gradients(b, bc, nrm, CR.PLANE_RADIUS, 30)
runs = {"coloured (normals and gradients given)": lambda: S.registration_colored_icp(a, ac, b, bc, md, target_normals=nrm, target_gradients=grd),
        "coloured (normals and gradients estimated)": lambda: S.registration_colored_icp(a, ac, b, bc, md, normal_radius=CR.PLANE_RADIUS, gradient_radius=CR.PLANE_RADIUS),
        "point-to-plane (normals given)": lambda: S.registration_icp(a, b, md, estimation="point_to_plane", target_normals=nrm),
        "point-to-point": lambda: S.registration_icp(a, b, md)}
for name, f in runs.items():
    f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(10):
        t0 = time.perf_counter()
        res = f()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    err = NR.displacement(res.transformation.cpu().numpy(), T_true, src) / NR.SPACING
    say(f"plane scene ({src.shape[0]} -> {tgt.shape[0]} rows), {name}: {res.iterations} iterations, wall median {np.median(ts):.2f} ms "
        f"(min {np.min(ts):.2f}), {err:.3g} spacings from the truth")
