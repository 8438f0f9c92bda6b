"""numpy restatement of dense RGB-D odometry (csrc/odometry.hip, include/gsr.h: gsr_odometry_prepare, gsr_odometry_update) and of
scene_utils.odometry.rgbd_odometry over the pyramid reference of tests/frames_reference.py.  `prepare` is float32 in the header's
order of operations (numpy rounds every elementwise operation on its own and never contracts): it reproduces the kernel's bits.
`update` is float64 in the header's order: the association (steps 1 - 8) reproduces the kernel's decisions exactly, so n is exact;
the sums are formed in another order, the solve is the same LDL^T.  Also the analytic scene and the cases the CPU and GPU tests
share."""
import functools
import math

import numpy as np

import frames_reference as FR

PIVOT_MIN = 1e-12
LAMBDA = 0.968


# ---- prepare ------------------------------------------------------------------------------------------------------------------------
def sobel(P):
    """(d/dx, d/dy) of a float32 plane: the 3 x 3 Sobel operator times 0.125 in the header's order; NaN on the border."""
    f = np.float32
    P = np.asarray(P, dtype=f)
    H, W = P.shape
    gx, gy = np.full((H, W), np.nan, dtype=f), np.full((H, W), np.nan, dtype=f)
    if H < 3 or W < 3:
        return gx, gy
    a, b, c = P[:-2, :-2], P[:-2, 1:-1], P[:-2, 2:]
    d, e = P[1:-1, :-2], P[1:-1, 2:]
    p, q, r = P[2:, :-2], P[2:, 1:-1], P[2:, 2:]
    with np.errstate(invalid="ignore", over="ignore"):
        gx[1:-1, 1:-1] = (((c - a) + f(2) * (e - d)) + (r - p)) * f(0.125)
        gy[1:-1, 1:-1] = (((p - a) + f(2) * (q - b)) + (r - c)) * f(0.125)
    return gx, gy


def prepare(color, depth, mask, depth_min=0.0, depth_max=4.0, gradients=True):
    """-> (intensity [H,W], depth [H,W], grad [4,H,W] or None), float32"""
    f = np.float32
    color, depth = np.asarray(color, dtype=f), np.asarray(depth, dtype=f)
    seen = np.ones(depth.shape, dtype=bool) if mask is None else (np.asarray(mask, dtype=f) == f(1))
    with np.errstate(invalid="ignore", over="ignore"):
        I = np.where(seen, ((color[0] + color[1]) + color[2]) / f(3), f(np.nan)).astype(f)
        ok = seen & np.isfinite(depth) & (depth > f(depth_min)) & (depth <= f(depth_max))
    D = np.where(ok, depth, f(np.nan)).astype(f)
    if not gradients:
        return I, D, None
    return I, D, np.stack(sobel(I) + sobel(D)).astype(f)


# ---- update -------------------------------------------------------------------------------------------------------------------------
def associate(K, w, h, src_I, src_D, tgt_I, tgt_D, tgt_grad, T, depth_diff_max):
    """steps 1 - 8 -> dict(ok [h,w] bool: the participants, Q [3,h,w], j = (vi, ui) integer arrays (0 where not ok), rD, why: the
    step at which every other pixel dropped out, 0 for participants)"""
    fx, fy, cx, cy = (float(v) for v in K)
    T = np.asarray(T, dtype=np.float64)
    d, Is = np.asarray(src_D, dtype=np.float32).astype(np.float64), np.asarray(src_I, dtype=np.float32).astype(np.float64)
    x = np.broadcast_to(np.arange(w, dtype=np.float64)[None, :], (h, w))
    y = np.broadcast_to(np.arange(h, dtype=np.float64)[:, None], (h, w))
    why = np.zeros((h, w), dtype=np.int32)

    def drop(ok, cond, step):
        why[ok & ~cond] = step
        return ok & cond
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        ok = drop(np.ones((h, w), dtype=bool), np.isfinite(d) & np.isfinite(Is), 1)
        P = [d * ((x - cx) / fx), d * ((y - cy) / fy), d]
        Q = [((T[k, 0] * P[0] + T[k, 1] * P[1]) + T[k, 2] * P[2]) + T[k, 3] for k in range(3)]
        ok = drop(ok, np.isfinite(Q[2]) & (Q[2] > 0), 4)
        u, v = fx * (Q[0] / Q[2]) + cx, fy * (Q[1] / Q[2]) + cy
        ui, vi = np.floor(u + 0.5), np.floor(v + 0.5)
        ok = drop(ok, (ui >= 0) & (ui <= w - 1) & (vi >= 0) & (vi <= h - 1), 6)
        uj, vj = np.where(ok, ui, 0).astype(np.int64), np.where(ok, vi, 0).astype(np.int64)
        dt = np.asarray(tgt_D, dtype=np.float32).astype(np.float64)[vj, uj]
        It = np.asarray(tgt_I, dtype=np.float32).astype(np.float64)[vj, uj]
        g = np.asarray(tgt_grad, dtype=np.float32).astype(np.float64)[:, vj, uj]
        ok = drop(ok, np.isfinite(dt) & np.isfinite(It) & np.isfinite(g).all(axis=0), 7)
        rD = dt - Q[2]
        ok = drop(ok, np.abs(rD) <= depth_diff_max, 8)
    return dict(ok=ok, Q=np.stack(Q), vj=vj, uj=uj, dt=dt, It=It, Is=Is, g=g, rD=rD, why=why)


def ldlt_solve(A, g):
    """A x = g by LDL^T with the kernel's pivot rule -> x, or None (a rejected pivot, or a solution that is not finite)"""
    A, g = np.asarray(A, dtype=np.float64), np.asarray(g, dtype=np.float64)
    n = A.shape[0]
    L, D = np.zeros((n, n)), np.zeros(n)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for j in range(n):
            d = A[j, j]
            for k in range(j):
                d -= L[j, k] * L[j, k] * D[k]
            if not (abs(d) < np.inf) or not (d > PIVOT_MIN * A[j, j]):
                return None
            D[j] = d
            L[j, j] = 1.0
            for i in range(j + 1, n):
                v = A[i, j]
                for k in range(j):
                    v -= L[i, k] * L[j, k] * D[k]
                L[i, j] = v / d
        x = np.zeros(n)
        for i in range(n):
            v = g[i]
            for k in range(i):
                v -= L[i, k] * x[k]
            x[i] = v
        x /= D
        for i in range(n - 1, -1, -1):
            v = x[i]
            for k in range(i + 1, n):
                v -= L[k, i] * x[k]
            x[i] = v
    return x if abs(x.sum()) < np.inf else None


def vector_to_matrix(x):
    """[Rz(gamma) Ry(beta) Rx(alpha), t] as a 4 x 4"""
    sa, ca, sb, cb, sg, cg = math.sin(x[0]), math.cos(x[0]), math.sin(x[1]), math.cos(x[1]), math.sin(x[2]), math.cos(x[2])
    M = np.eye(4)
    M[:3, :3] = [[cb * cg, sa * sb * cg - ca * sg, ca * sb * cg + sa * sg],
                 [cb * sg, sa * sb * sg + ca * cg, ca * sb * sg - sa * cg],
                 [-sb, sa * cb, ca * cb]]
    M[:3, 3] = x[3:6]
    return M


def update(K, w, h, src_I, src_D, tgt_I, tgt_D, tgt_grad, T, lambda_geometric=LAMBDA, depth_diff_max=0.03, apply=True):
    """One step -> dict(n, fitness, rmse, status, sum_rD2, sum_rI2, T (the new one, or the old one), JtJ, Jtr, cond, ok, why)"""
    fx, fy = float(K[0]), float(K[1])
    T = np.asarray(T, dtype=np.float64)
    a = associate(K, w, h, src_I, src_D, tgt_I, tgt_D, tgt_grad, T, depth_diff_max)
    ok = a["ok"]
    Q = a["Q"][:, ok]
    g, rD, rI = a["g"][:, ok], a["rD"][ok], (a["It"] - a["Is"])[ok]
    n = int(ok.sum())
    sd, si = math.sqrt(lambda_geometric), math.sqrt(1.0 - lambda_geometric)
    fa, fb = fx / Q[2], fy / Q[2]

    def rows(gx, gy, minus_one, weight):
        c0, c1 = gx * fa, gy * fb
        c2 = -((c0 * Q[0] + c1 * Q[1]) / Q[2]) - (1.0 if minus_one else 0.0)
        return weight * np.stack([Q[1] * c2 - Q[2] * c1, Q[2] * c0 - Q[0] * c2, Q[0] * c1 - Q[1] * c0, c0, c1, c2])
    JD, JI = rows(g[2], g[3], True, sd), rows(g[0], g[1], False, si)
    JtJ = JD @ JD.T + JI @ JI.T
    Jtr = JD @ (sd * rD) + JI @ (si * rI)
    sum_rD2 = float(np.sum(rD * rD)) if sd > 0 else 0.0
    sum_rI2 = float(np.sum(rI * rI)) if si > 0 else 0.0
    out = dict(n=n, fitness=n / (w * h), rmse=math.sqrt(sum_rD2 / n) if n else 0.0, sum_rD2=sum_rD2, sum_rI2=sum_rI2, JtJ=JtJ,
               Jtr=Jtr, ok=ok, why=a["why"], T=T.copy(), cond=float("inf"))
    if n < 6:
        out["status"] = 1
        return out
    x = ldlt_solve(JtJ, -Jtr)
    if x is None:
        out["status"] = 2
        return out
    out["status"] = 0
    out["cond"] = float(np.linalg.cond(JtJ))
    if apply:
        Tn = vector_to_matrix(x) @ T
        Tn[3] = [0.0, 0.0, 0.0, 1.0]
        out["T"] = Tn
    return out


# ---- the driver ---------------------------------------------------------------------------------------------------------------------
def pyramid(color, depth, mask, K, levels):
    """[(color, depth, mask, K, w, h)] for levels 0 .. `levels`: tests/frames_reference.py's pyramid and intrinsics"""
    h, w = depth.shape
    out = [(color, depth, mask, tuple(float(v) for v in K), w, h)]
    for l, (c, d, m) in enumerate(FR.pyramid_reference(color, depth, mask, levels), start=1):
        fx, fy, cx, cy, wl, hl = FR.scaled_intrinsics(*K, w, h, l)
        out.append((c, d, m, (fx, fy, cx, cy), wl, hl))
    return out


def rgbd_odometry(source, target, K, init=None, max_iterations=(20, 10, 5), lambda_geometric=LAMBDA, depth_min=0.0, depth_max=4.0,
                  depth_diff_max=0.03):
    """source, target: (color [3,h,w], depth [h,w], mask or None), float32.  check_every = 0: every level runs its count.
    -> dict(T, fitness, rmse, status, iterations, first: per level (coarse to fine) dict(level, T0 = the transformation the level
    started from, step = update()'s result of its first iteration, planes = (K, w, h, and the five planes of the level)))"""
    levels = len(max_iterations) - 1
    ps, pt = pyramid(*source, K, levels), pyramid(*target, K, levels)
    T = np.eye(4) if init is None else np.asarray(init, dtype=np.float64).copy()
    first, iterations = [], 0
    planes = None
    for level, n in zip(range(levels, -1, -1), max_iterations):
        cs, ds, ms, Kl, w, h = ps[level]
        ct, dt, mt = pt[level][:3]
        sI, sD, _ = prepare(cs, ds, ms, depth_min, depth_max, gradients=False)
        tI, tD, tg = prepare(ct, dt, mt, depth_min, depth_max)
        planes = (Kl, w, h, sI, sD, tI, tD, tg)
        for k in range(n):
            step = update(*planes, T, lambda_geometric, depth_diff_max)
            if k == 0:
                first.append(dict(level=level, T0=T.copy(), step=step, planes=planes))
            T = step["T"]
            iterations += 1
    closing = update(*planes, T, lambda_geometric, depth_diff_max, apply=False)
    return dict(T=T, fitness=closing["fitness"], rmse=closing["rmse"], status=closing["status"], iterations=iterations, first=first)


# ---- the analytic scene -------------------------------------------------------------------------------------------------------------
def rigid(axis, degrees, t):
    """4 x 4 of a rotation by `degrees` about `axis` through the origin, then the translation t"""
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.linalg.norm(k)
    th = math.radians(degrees)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * (Kx @ Kx)
    M[:3, 3] = t
    return M


def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    """world-to-camera 4 x 4 of a camera (x right, y down, z forward) at `eye` looking at `target`"""
    eye = np.asarray(eye, dtype=np.float64)
    f = np.asarray(target, dtype=np.float64) - eye
    f /= np.linalg.norm(f)
    r = np.cross(f, np.asarray(up, dtype=np.float64))
    r /= np.linalg.norm(r)
    d = np.cross(f, r)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = r, d, f, eye
    return np.linalg.inv(c2w)


TEXTURE = (  # per channel: (amplitude, wave vector [1/m], phase) of three sinusoids of the world position
    ((0.16, (5.0, 2.0, -3.0), 0.3), (0.12, (-2.5, 6.0, 1.5), 1.1), (0.08, (1.0, -3.0, 7.0), 2.0)),
    ((0.15, (-4.0, 3.0, 2.0), 0.7), (0.11, (3.0, 5.5, -2.0), 2.9), (0.09, (6.5, -1.0, 2.5), 0.2)),
    ((0.14, (2.0, -5.0, 4.0), 1.9), (0.13, (-6.0, -2.0, 1.0), 0.5), (0.07, (1.5, 4.0, 6.0), 3.3)),
)


def corner_scene(w, h, K, w2c, texture=True):
    """The inside of a box corner - the planes x = 0, y = 0, z = 0 of the world, seen from the positive octant - as a camera with
    intrinsics K and world-to-camera `w2c` sees it: for every pixel's ray the nearest positive hit.  -> (color [3,h,w] float32:
    0.5 + a smooth sum of sinusoids of the hit's world position, depth [h,w] float32: the exact view-space z; 0 and colour 0.5
    where the ray hits nothing)."""
    fx, fy, cx, cy = (float(v) for v in K)
    w2c = np.asarray(w2c, dtype=np.float64)
    R, eye = w2c[:3, :3].T, -w2c[:3, :3].T @ w2c[:3, 3]
    x = np.broadcast_to(np.arange(w, dtype=np.float64)[None, :], (h, w))
    y = np.broadcast_to(np.arange(h, dtype=np.float64)[:, None], (h, w))
    dc = np.stack([(x - cx) / fx, (y - cy) / fy, np.ones((h, w))])           # camera-space direction with z = 1: t is the z-depth
    dw = np.einsum("ij,jhw->ihw", R, dc)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.stack([np.where(dw[k] < 0, -eye[k] / dw[k], np.inf) for k in range(3)])
    t = np.where(t > 0, t, np.inf).min(axis=0)
    hit = np.isfinite(t)
    t = np.where(hit, t, 0.0)
    X = eye[:, None, None] + dw * t
    color = np.full((3, h, w), 0.5)
    if texture:
        for ch in range(3):
            for amp, k, ph in TEXTURE[ch]:
                color[ch] += np.where(hit, amp * np.sin(k[0] * X[0] + k[1] * X[1] + k[2] * X[2] + ph), 0.0)
    return color.astype(np.float32), t.astype(np.float32)


def unproject(depth, K):
    """[n,3] float64 camera-space points of the valid (finite, > 0) pixels of a depth plane"""
    fx, fy, cx, cy = (float(v) for v in K)
    d = np.asarray(depth, dtype=np.float64)
    h, w = d.shape
    x = np.broadcast_to(np.arange(w, dtype=np.float64)[None, :], (h, w))
    y = np.broadcast_to(np.arange(h, dtype=np.float64)[:, None], (h, w))
    ok = np.isfinite(d) & (d > 0)
    return np.stack([d * (x - cx) / fx, d * (y - cy) / fy, d], axis=-1)[ok]


def displacement(Ta, Tb, points):
    """the largest distance between Ta p and Tb p over the rows of `points`"""
    p = np.asarray(points, dtype=np.float64)
    D = (np.asarray(Ta, dtype=np.float64) - np.asarray(Tb, dtype=np.float64))
    return float(np.linalg.norm(p @ D[:3, :3].T + D[:3, 3], axis=1).max())


# ---- the end-to-end case (tests/test_odometry_cpu.py, tests/test_odometry_gpu.py) -----------------------------------------------------
E2E_W, E2E_H = 160, 120
E2E_K = (140.0, 140.0, 80.3, 59.1)
E2E_EYE = (1.5, 1.3, 1.4)
E2E_MOTION = rigid((0.3, -0.8, 0.5), 1.5, (0.03, -0.02, 0.025))      # source-camera to target-camera coordinates
E2E_ITERATIONS = (20, 10, 5)


@functools.lru_cache(maxsize=None)
def e2e():
    """-> dict(source, target: (color, depth, None), K, T_true, points: the source's unprojected pixels, ref: rgbd_odometry's
    result from the identity, error: E_ref)"""
    w2c_t = look_at(E2E_EYE)
    w2c_s = np.linalg.inv(E2E_MOTION) @ w2c_t
    tc, td = corner_scene(E2E_W, E2E_H, E2E_K, w2c_t)
    sc, sd = corner_scene(E2E_W, E2E_H, E2E_K, w2c_s)
    source, target = (sc, sd, None), (tc, td, None)
    ref = rgbd_odometry(source, target, E2E_K, max_iterations=E2E_ITERATIONS)
    points = unproject(np.where(sd <= 4.0, sd, 0.0), E2E_K)
    return dict(source=source, target=target, K=E2E_K, T_true=E2E_MOTION, points=points, ref=ref,
                error=displacement(ref["T"], E2E_MOTION, points), start=displacement(np.eye(4), E2E_MOTION, points))


# ---- the update cases (tests/test_odometry_cpu.py checks on the reference alone that each has what it is there for;
# tests/test_odometry_update_gpu.py runs them on the device) -----------------------------------------------------------------------
# (257 x 255 is one pixel short of 256 workgroups x 256 threads: every thread takes at most one; 257 x 257 takes the stride loop)
UPDATE_SIZES = ((4, 3), (20, 13), (64, 64), (257, 255), (257, 257))
UPDATE_LAMBDAS = (0.968, 0.5, 0.0, 1.0)
EDGE_DIFF = 0.03125                       # a depth_diff_max that float32 depths can meet exactly


def size_K(w, h):
    return (0.875 * w, 0.875 * w, (w - 1) / 2 + 0.011 * w, (h - 1) / 2 - 0.017 * h)


def _planes(w, h, motion, texture=True):
    K = size_K(w, h)
    w2c_t = look_at(E2E_EYE)
    tc, td = corner_scene(w, h, K, w2c_t, texture)
    sc, sd = corner_scene(w, h, K, np.linalg.inv(motion) @ w2c_t, texture)
    sI, sD, _ = prepare(sc, sd, None, gradients=False)
    tI, tD, tg = prepare(tc, td, None)
    return dict(K=K, w=w, h=h, src_I=sI, src_D=sD, tgt_I=tI, tgt_D=tD, tgt_grad=tg)


SMALL_MOTION = rigid((0.3, -0.8, 0.5), 0.4, (0.008, -0.006, 0.007))


@functools.lru_cache(maxsize=None)
def update_case(name):
    """name -> dict(K, w, h, the five planes, T: the incoming transformation, depth_diff_max, status: what the update must report,
    lambdas: the weights the case is run with).  The arrays are shared: do not write to them."""
    lam_all = UPDATE_LAMBDAS
    if name.startswith("size_"):                     # the corner scene at every size, from the identity
        w, h = (int(v) for v in name[5:].split("x"))
        c = _planes(w, h, SMALL_MOTION)
        c.update(T=np.eye(4), depth_diff_max=0.03, status=1 if (w, h) == (4, 3) else 0, lambdas=lam_all)
    elif name == "outside":                          # a start a quarter of the image off: a band of pixels projects outside
        c = _planes(64, 64, SMALL_MOTION)
        c.update(T=rigid((0, 1, 0), 14.0, (0.0, 0.0, 0.0)) , depth_diff_max=0.5, status=0, lambdas=(LAMBDA,))
    elif name == "behind":                           # negative and zero source depths handed in directly: Qz <= 0
        c = _planes(64, 64, SMALL_MOTION)
        d = c["src_D"].copy()
        d[10:14, 20:40] = -d[10:14, 20:40]
        d[30, 5:25] = 0.0
        c.update(src_D=d, T=np.eye(4), depth_diff_max=0.03, status=0, lambdas=(LAMBDA,))
    elif name == "edge":                             # |d_t - Qz| exactly at depth_diff_max, and one float32 step beyond
        c = _planes(64, 64, np.eye(4))               # (the same view twice: under the identity every pixel maps to itself)
        sD, tD = c["src_D"].copy(), c["tgt_D"].copy()
        f = np.float32
        for row, (x0, sign) in enumerate(((8, 1.0), (24, -1.0))):
            for k in range(8):
                y, x = 20 + row, x0 + k
                sD[y, x] = f(2.0)
                at = f(2.0 + sign * EDGE_DIFF)
                tD[y, x] = at if k % 2 == 0 else np.nextafter(at, f(sign * np.inf), dtype=f)
        c.update(src_D=sD, tgt_D=tD, T=np.eye(4), depth_diff_max=EDGE_DIFF, status=0, lambdas=(LAMBDA,))
    elif name == "nan_planes":                       # NaN and inf sprinkled over every plane
        c = _planes(64, 64, SMALL_MOTION)
        rng = np.random.default_rng(7)
        for key in ("src_I", "src_D", "tgt_I", "tgt_D", "tgt_grad"):
            a = c[key].copy()
            hit = rng.random(a.shape) < 0.03
            a[hit] = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), size=int(hit.sum()))
            c[key] = a
        c.update(T=np.eye(4), depth_diff_max=0.03, status=0, lambdas=(LAMBDA,))
    elif name == "all_invalid":                      # no source depth at all: n = 0
        c = _planes(20, 13, SMALL_MOTION)
        c.update(src_D=np.full_like(c["src_D"], np.nan), T=np.eye(4), depth_diff_max=0.03, status=1, lambdas=(LAMBDA,))
    elif name == "wall":                             # a fronto-parallel one-colour plane: three unknowns are not fixed
        w, h = 64, 64
        color, depth = np.full((3, h, w), 0.5, dtype=np.float32), np.full((h, w), 2.0, dtype=np.float32)
        I, D, g = prepare(color, depth, None)
        c = dict(K=size_K(w, h), w=w, h=h, src_I=I, src_D=D, tgt_I=I, tgt_D=(D + np.float32(0.015625)).astype(np.float32), tgt_grad=g,
                 T=np.eye(4), depth_diff_max=0.03, status=2, lambdas=(LAMBDA, 1.0))
    else:
        raise KeyError(name)
    return c


UPDATE_CASES = tuple(f"size_{w}x{h}" for w, h in UPDATE_SIZES) + ("outside", "behind", "edge", "nan_planes", "all_invalid", "wall")


def run_update(case, lam, apply=True):
    return update(case["K"], case["w"], case["h"], case["src_I"], case["src_D"], case["tgt_I"], case["tgt_D"], case["tgt_grad"],
                  case["T"], lam, case["depth_diff_max"], apply)


def extent(case):
    """the largest side of the bounding box of the source's unprojected pixels"""
    p = unproject(case["src_D"], case["K"])
    return float(np.ptp(p, axis=0).max()) if len(p) else 0.0
