"""numpy restatement of the sensor-frame front end (csrc/frames.hip, include/gsr.h: gsr_frame_undistort, gsr_frame_pyramid) and of
scene_utils.cameras.scaled_camera's intrinsics.  Every function takes `dtype`: np.float64 is the reference; np.float32 follows the
kernels' stated operation order step by step (numpy rounds every elementwise operation on its own and never contracts), so for the
pyramid it reproduces the kernel's bits.  Also the seeded scenes the CPU and GPU tests share."""
import numpy as np


# ---- undistortion ------------------------------------------------------------------------------------------------------------------
def undistort_map(K_src, dist, K_dst, W, H, dtype=np.float64):
    """Source coordinates (us, vs) [H,W] of every target pixel, in `dtype`, in the header's order of operations."""
    f = dtype
    fx, fy, cx, cy = (f(v) for v in K_src)
    fxt, fyt, cxt, cyt = (f(v) for v in K_dst)
    k1, k2, p1, p2, k3 = (f(v) for v in dist)
    identity = all(float(v) == 0.0 for v in dist) and all(f(a) == f(b) for a, b in zip(K_src, K_dst))
    u = np.broadcast_to(np.arange(W, dtype=f)[None, :], (H, W))
    v = np.broadcast_to(np.arange(H, dtype=f)[:, None], (H, W))
    if identity:
        return u.copy(), v.copy()
    x, y = (u - cxt) / fxt, (v - cyt) / fyt
    x2, y2, xy = x * x, y * y, x * y
    r2 = x2 + y2
    rho = f(1) + r2 * (k1 + r2 * (k2 + r2 * k3))
    xd = (x * rho + (f(2) * p1) * xy) + p2 * (r2 + f(2) * x2)
    yd = (y * rho + p1 * (r2 + f(2) * y2)) + (f(2) * p2) * xy
    return fx * xd + cx, fy * yd + cy


def undistort_reference(color, depth, K_src, dist, K_dst, W, H, dtype=np.float64):
    """-> dict(color [3,H,W], depth [H,W] or None, mask [H,W], us, vs) in `dtype`: bilinear colour over the taps floor / ceil of
    the source coordinate, nearest depth (halves rounded up), mask = all taps inside; 0 outside."""
    f = dtype
    color = np.asarray(color, dtype=f)
    Hs, Ws = color.shape[1:]
    us, vs = undistort_map(K_src, dist, K_dst, W, H, f)
    inside = (us >= 0) & (us <= Ws - 1) & (vs >= 0) & (vs <= Hs - 1)
    uc, vc = np.where(inside, us, f(0)), np.where(inside, vs, f(0))
    x0f, y0f = np.floor(uc), np.floor(vc)
    ax, ay = uc - x0f, vc - y0f
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    x1, y1 = x0 + (ax > 0), y0 + (ay > 0)
    out = np.zeros((3, H, W), dtype=f)
    for ch in range(3):
        s = color[ch]
        c00, c01, c10, c11 = s[y0, x0], s[y0, x1], s[y1, x0], s[y1, x1]
        top = c00 + ax * (c01 - c00)
        bot = c10 + ax * (c11 - c10)
        out[ch] = np.where(inside, top + ay * (bot - top), f(0))
    d = None
    if depth is not None:
        xn, yn = np.floor(uc + f(0.5)).astype(np.int64), np.floor(vc + f(0.5)).astype(np.int64)
        d = np.where(inside, np.asarray(depth, dtype=f)[yn, xn], f(0))
    return dict(color=out, depth=d, mask=inside.astype(f), us=us, vs=vs)


def undistort_scene(seed=5):
    """The undistort tests' scene: an 80 x 60 source - a smooth colour image (three low-frequency sinusoids per channel: bounded
    gradient), a piecewise-constant depth with a step edge and a hole of zeros - distortion D, and a 72 x 56 target with its own K
    whose field of view is wider than the source's, so that a border of the target falls outside it."""
    rng = np.random.default_rng(seed)
    Ws, Hs, W, H = 80, 60, 72, 56
    yy, xx = np.meshgrid(np.arange(Hs, dtype=np.float64), np.arange(Ws, dtype=np.float64), indexing="ij")
    color = np.zeros((3, Hs, Ws))
    for ch in range(3):
        for _ in range(3):
            kx, ky = rng.uniform(-0.12, 0.12, size=2)         # at most ~1.5 periods across the image
            color[ch] += rng.uniform(0.05, 0.16) * np.sin(kx * xx + ky * yy + rng.uniform(0, 2 * np.pi))
        color[ch] += 0.5
    depth = np.where(xx < 37, 2.0, 3.5)
    depth[20:31, 50:63] = 0.0
    return dict(color=color.astype(np.float32), depth=depth.astype(np.float32), K=(70.0, 68.0, 40.2, 28.7),
                D=(-0.28, 0.07, 1e-3, -5e-4, 0.0), new_K=(45.0, 44.0, 35.1, 27.3), W=W, H=H, Ws=Ws, Hs=Hs)


def near_half_integer(us, vs, tol=1e-3):
    """Target pixels whose source coordinate lies within `tol` px of a half-integer in x or y (nearest-pixel ties)."""
    fx, fy = np.abs((us - 0.5) - np.round(us - 0.5)), np.abs((vs - 0.5) - np.round(vs - 0.5))
    return (fx <= tol) | (fy <= tol)


def near_border(us, vs, Ws, Hs, tol=1e-3):
    """Target pixels with a tap within `tol` px of the source border (the mask may flip there between float32 and float64)."""
    return (np.abs(us) <= tol) | (np.abs(us - (Ws - 1)) <= tol) | (np.abs(vs) <= tol) | (np.abs(vs - (Hs - 1)) <= tol)


# ---- pyramid -----------------------------------------------------------------------------------------------------------------------
def _quads(p):
    H2, W2 = p.shape[-2] // 2, p.shape[-1] // 2
    p = p[..., :2 * H2, :2 * W2]
    return p[..., 0::2, 0::2], p[..., 0::2, 1::2], p[..., 1::2, 0::2], p[..., 1::2, 1::2]      # a, b, c, d


def pyramid_level(color, depth, mask, band=0.05, dtype=np.float32):
    """One halving: colour ((a + b) + (c + d)) 0.25; depth the mean, in the order a, b, c, d, of the valid (> 0) readings
    <= m (1 + band), m the smallest valid one, 0 without any; mask 1 iff all four are 1."""
    f = dtype
    a, b, c, d = _quads(np.asarray(color, dtype=f))
    col = ((a + b) + (c + d)) * f(0.25)
    dep = msk = None
    if depth is not None:
        q = _quads(np.asarray(depth, dtype=f))
        big = f(np.inf)
        m = np.minimum(np.minimum(np.where(q[0] > 0, q[0], big), np.where(q[1] > 0, q[1], big)),
                       np.minimum(np.where(q[2] > 0, q[2], big), np.where(q[3] > 0, q[3], big)))
        lim = m * (f(1) + f(band))
        total, n = np.zeros_like(m), np.zeros_like(m)
        for r in q:
            take = (r > 0) & (r <= lim)
            total = np.where(take, total + r, total)
            n = n + take.astype(f)
        with np.errstate(invalid="ignore", divide="ignore"):
            dep = np.where(n > 0, total / np.where(n > 0, n, f(1)), f(0)).astype(f)
    if mask is not None:
        q = _quads(np.asarray(mask, dtype=f))
        msk = ((q[0] == 1) & (q[1] == 1) & (q[2] == 1) & (q[3] == 1)).astype(f)
    return col.astype(f), dep, msk


def pyramid_reference(color, depth, mask, levels, band=0.05, dtype=np.float32):
    """-> [(color, depth, mask)] for levels 1 .. `levels`."""
    out = []
    for _ in range(levels):
        color, depth, mask = pyramid_level(color, depth, mask, band, dtype)
        out.append((color, depth, mask))
    return out


def pyramid_scene(W, H, seed=0):
    """Colour noise; a depth with a vertical edge whose sides (2.0 and 3.0, each with 1 % ripple) differ by far more than the 5 %
    band, holes of zeros sprinkled over it (quads with 0 .. 4 valid readings) and one all-zero block; a mask with dropouts."""
    rng = np.random.default_rng(seed)
    color = rng.random((3, H, W), dtype=np.float32)
    xx = np.broadcast_to(np.arange(W)[None, :], (H, W))
    depth = np.where(xx < (W // 2) | 1, 2.0, 3.0) * (1.0 + 0.01 * rng.standard_normal((H, W)))       # (an odd column: inside quads)
    depth[rng.random((H, W)) < 0.45] = 0.0
    depth[: min(H, 9), : min(W, 9)] = 0.0
    mask = (rng.random((H, W)) < 0.9).astype(np.float32)
    mask[H // 2:, : W // 2] = 1.0
    return color, depth.astype(np.float32), mask


# ---- cameras -----------------------------------------------------------------------------------------------------------------------
def scaled_intrinsics(fx, fy, cx, cy, W, H, level):
    """(fx, fy, cx, cy, W, H) of pyramid level `level`."""
    s = float(2 ** level)
    return fx / s, fy / s, (cx + 0.5) / s - 0.5, (cy + 0.5) / s - 0.5, W >> level, H >> level
