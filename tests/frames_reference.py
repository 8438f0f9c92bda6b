"""numpy restatement of the sensor-frame front end (csrc/frames.hip, include/gsr.h: gsr_frame_undistort, gsr_frame_pyramid) and of
scene_utils.cameras.scaled_camera's intrinsics.  Every function takes `dtype`: np.float64 is the reference; np.float32 follows the
kernels' stated operation order step by step (numpy rounds every elementwise operation on its own and never contracts), so it
reproduces both kernels' bits.  Also the seeded scenes and cases the CPU and GPU tests share."""
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
    with np.errstate(over="ignore", invalid="ignore"):          # (coefficients may be large enough to overflow: inf / NaN = outside)
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
        with np.errstate(over="ignore", invalid="ignore"):      # (NaN and inf in the source propagate as IEEE 754 says)
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


def differing(got, want):
    """Elements of `got` whose float32 bits differ from `want`'s, [bool array]; where `want` is NaN any NaN is equal (the payload
    and sign of a NaN that arithmetic produced are not part of the rule)."""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    return (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))


# the bit tests' cases (tests/test_frames_bits_gpu.py runs them on the device, tests/test_frames_cpu.py checks on the reference
# alone that each has what it is there for).  Every case is a dict with undistort_scene's keys; `depth` may be None.
BARREL = (-0.22, 0.06, 1.2e-3, -7e-4, -0.015)           # k1 < 0: the target's corners are pulled into the source
PINCUSHION = (0.18, 0.05, -9e-4, 6e-4, 0.02)
EDGE_W, EDGE_H = (1, 63, 64, 65, 129), (1, 3, 4, 5, 9)   # around the 64 x 4 workgroup
TINY_SOURCES = ((1, 1), (2, 1), (1, 2))


def distinct_depth(Ws, Hs):
    """A depth plane with a different, exactly representable value on every pixel: 1 + index / 4096 (up to 2^19 pixels)."""
    return (1.0 + np.arange(Ws * Hs, dtype=np.float64).reshape(Hs, Ws) / 4096.0).astype(np.float32)


def undistort_case(Ws, Hs, W, H, dist, seed=0, depth=True, spread=1.25, K=None, new_K=None):
    """A seeded Ws x Hs source (colour noise, distinct_depth) and a W x H target whose K is placed relative to the TARGET's size:
    the principal point 1.1 % / 1.7 % of the size off its centre, the focal lengths such that the target's pixel centres span
    `spread` times the angle the source's do - so the outermost target pixels fall outside the source at any size (with a fixed
    target K a small target lies wholly inside or wholly outside).  `K` / `new_K` override either."""
    rng = np.random.default_rng([seed, Ws, Hs, W, H])
    color = rng.random((3, Hs, Ws), dtype=np.float32)
    if K is None:
        K = (0.875 * max(Ws, 8), 0.85 * max(Ws, 8), (Ws - 1) / 2 + 0.0125 * Ws, (Hs - 1) / 2 - 0.02 * Hs)
    if new_K is None:
        new_K = (K[0] * max(W - 1, 1) / max(Ws - 1, 1) / spread, K[1] * max(H - 1, 1) / max(Hs - 1, 1) / spread,
                 (W - 1) / 2 + 0.011 * W, (H - 1) / 2 - 0.017 * H)
    return dict(color=color, depth=distinct_depth(Ws, Hs) if depth else None, K=tuple(float(v) for v in K),
                D=tuple(float(v) for v in dist), new_K=tuple(float(v) for v in new_K), W=W, H=H, Ws=Ws, Hs=Hs)


def undistort_tiny_source_case(Ws, Hs):
    """A 1 x 1, 2 x 1 or 1 x 2 source under a 9 x 9 target, radial distortion only.  The source's principal point is the centre of
    its pixels, the target's the pixel (4, 4), and a target pixel is 0.2 source pixels wide: x = 0 gives xd = 0 and us = cx exactly
    (p1 = p2 = 0), so the target's row 4 / column 4 lies exactly on the only row / column a one-pixel-high / -wide source has.
    Inside: the pixel (4, 4) alone for 1 x 1 (us = vs = 0), the five pixels |u - 4| <= 2 of row 4 for 2 x 1 (us = 0.5 + 0.2 (u - 4)
    rho), the five of column 4 for 1 x 2.  -> (case, the number of inside pixels)"""
    assert (Ws, Hs) in TINY_SOURCES
    case = undistort_case(Ws, Hs, 9, 9, (-0.2, 0.05, 0.0, 0.0, 0.01), K=(8.0, 8.0, (Ws - 1) / 2, (Hs - 1) / 2),
                          new_K=(40.0, 40.0, 4.0, 4.0))
    return case, 1 if (Ws, Hs) == (1, 1) else 5


# name -> (dx, dy, W, H): us = u + dx, vs = v + dy EXACTLY on a 16 x 12 source, from a change of the principal point alone
EXACT_SHIFTS = {
    "half_x": (0.5, 0.0, 16, 12),             # every us a nearest-pixel tie, ax = 0.5; vs = v: the first row on vs = 0, ay = 0
    "half_y": (0.0, 0.5, 16, 12),             # the same vertically; the first column on us = 0
    "half_xy": (0.5, 0.5, 16, 12),
    "one_x": (1.0, 0.0, 16, 12),              # ax = ay = 0: the taps coincide, the source pixel is copied
    "one_y": (0.0, 1.0, 16, 12),
    "minus_one": (-1.0, -1.0, 16, 12),        # the first column and row outside, the second exactly on 0
    "last_col": (4.0, 0.5, 12, 12),           # the last target column exactly on us = 15 = src_w - 1: inside
    "last_row": (0.5, 3.0, 16, 9),            # the last target row exactly on vs = 11 = src_h - 1: inside
    "last_both": (4.0, 3.0, 12, 9),
}


def undistort_exact_case(name):
    """No distortion, fx' = fx = fy' = fy = 64 (a power of two: (u - cx') / 64 * 64 is exact), principal points on multiples of
    0.5: the source coordinate of the target pixel (u, v) is (u + dx, v + dy) without any rounding."""
    dx, dy, W, H = EXACT_SHIFTS[name]
    K = (64.0, 64.0, 7.5, 5.5)
    return undistort_case(16, 12, W, H, (0.0,) * 5, K=K, new_K=(64.0, 64.0, K[2] - dx, K[3] - dy))


def undistort_overflow_case():
    """k3 = 3e38 (finite: the entry point takes it) over a 65 x 33 target with |x|, |y| up to 1.19 / 1.14: r2 k3 overflows to +inf
    where r2 > 1.134, so rho = inf there and the coordinate is inf - or NaN, on the column x = 0 (0 inf).  The source's focal
    length is 1e-37, so that where rho stays finite (up to 3e38) the coordinate fx x rho + cx is an ordinary one: a large part of
    the target is inside."""
    return undistort_case(80, 60, 65, 33, (0.0, 0.0, 0.0, 0.0, 3e38), K=(1e-37, 1e-37, 39.5, 29.5), new_K=(27.0, 14.0, 32.0, 16.0))


def undistort_special_case():
    """The 80 x 60 -> 72 x 56 barrel case with NaN, +inf and -inf in source colour pixels and +inf, -inf, negative and -0.0 depth
    readings, all well inside the part of the source that the target samples."""
    case = undistort_case(80, 60, 72, 56, BARREL, seed=3)
    c, d = case["color"], case["depth"]
    c[0, 30, 40], c[1, 30, 40], c[2, 31, 41] = np.nan, np.inf, -np.inf
    c[0, 20, 25:27] = np.inf                   # two neighbours: inf - inf between the taps
    c[1, 35, 50], c[1, 36, 50] = np.inf, -np.inf
    c[2, 10:12, 60] = np.nan
    # (2 x 2 blocks: a target pixel is about 1.4 source pixels wide, the nearest-pixel rule may step over a single one)
    for (y, x), val in (((30, 40), np.inf), ((40, 20), -np.inf), ((20, 25), -1.5), ((35, 50), -0.0), ((12, 12), np.nan)):
        d[y:y + 2, x:x + 2] = val
    return case


def undistort_named_cases():
    """name -> case: every small case but the edge sizes (EDGE_W x EDGE_H, built by the tests from undistort_case)."""
    cases = {f"source_{w}x{h}": undistort_tiny_source_case(w, h)[0] for w, h in TINY_SOURCES}
    cases["source_80x60"] = undistort_case(80, 60, 72, 56, BARREL)
    cases["source_80x60_pincushion"] = undistort_case(80, 60, 72, 56, PINCUSHION)
    cases.update({f"exact_{k}": undistort_exact_case(k) for k in EXACT_SHIFTS})
    cases["overflow"] = undistort_overflow_case()
    cases["upsample"] = undistort_case(20, 15, 131, 67, BARREL)
    cases["downsample"] = undistort_case(131, 67, 20, 15, PINCUSHION)
    cases["special_values"] = undistort_special_case()
    return cases


def undistort_full_frame_case():
    """640 x 480 with a calibration of the size a RealSense colour stream reports, onto the same K and size."""
    K = (615.3, 615.8, 318.2, 241.7)
    return undistort_case(640, 480, 640, 480, (0.14, -0.42, -8e-4, 5e-4, 0.38), seed=7, K=K, new_K=K)


# ---- pyramid -----------------------------------------------------------------------------------------------------------------------
PYR_W, PYR_H = (2, 3, 31, 32, 33, 34, 63, 64, 65, 66), (2, 3, 32, 33, 65)      # around the 32-px block and its halvings


def max_levels(W, H, cap=3):
    """The largest `levels` <= cap that leaves a W x H image a pixel."""
    n = 0
    while n < cap and (W >> (n + 1)) >= 1 and (H >> (n + 1)) >= 1:
        n += 1
    return n


def depth_class_quads(band):
    """name -> the four readings (a, b, c, d) of a hand-built quad, float32.  `edge` is float32(m float32(1 + band)) for m = 2:
    the largest reading inside the band."""
    f = np.float32
    inf, nan = f(np.inf), f(np.nan)
    with np.errstate(over="ignore"):           # (a band wide enough to overflow: edge = above = inf, which is never valid)
        edge = f(f(2.0) * (f(1) + f(band)))
    above = np.nextafter(edge, inf, dtype=f)
    tiny = f(1e-40)                            # a denormal
    assert 0 < tiny < np.finfo(f).tiny
    q = {
        "valid0": (0, 0, 0, 0), "valid1": (0, 0, 2.0, 0), "valid2": (0, 2.0, 2.01, 0), "valid3": (2.04, 2.0, 0, 2.02),
        "valid4": (2.0, 2.02, 2.04, 2.06),
        "inf_alone": (inf, inf, inf, inf), "inf_and_holes": (0, inf, 0, 0), "inf_beside_finite": (inf, 2.0, 0, inf),
        "inf_beside_three": (2.0, inf, 2.05, 3.5),
        "nan": (nan, 2.0, 2.01, 0), "nan_alone": (nan, nan, nan, nan), "negative": (-1.0, 2.0, 2.02, -3.0),
        "negative_alone": (-1.0, -2.0, 0, -0.5), "minus_zero": (-0.0, 2.0, 0, 2.03), "minus_zero_alone": (-0.0, -0.0, -0.0, -0.0),
        "denormal_alone": (tiny, 0, 0, 0), "denormals": (tiny, f(1.02e-40), 0, f(2e-40)), "denormal_beside_finite": (2.0, tiny, 2.0, 0),
        "equal4": (2.5, 2.5, 2.5, 2.5),
        "at_edge": (2.0, edge, 0, 0), "above_edge": (2.0, above, 0, 0), "edge_both": (above, edge, 2.0, edge),
        "far": (2.0, 3.5, 2.0, 3.5),
    }
    return {k: tuple(f(x) for x in v) for k, v in q.items()}


def depth_class_scene(band, level, seed=0):
    """A scene whose level-(`level` - 1) depth holds depth_class_quads(band), one quad per 2 x 2 cell, 6 cells per row: every reading
    fills a 2^(level-1) square of level 0 (the mean of equal readings is the reading: r + r + r + r and / 4 are exact), except that
    a square of a reading that is not valid (inf, NaN, <= 0) reduces to 0 on the way - at level 1 the quads are the readings
    themselves.  Colour noise; a mask with 1, 0, 0.5, 2 and NaN.  -> (color, depth, mask, {name: (row, col) at `level`})"""
    quads = depth_class_quads(band)
    s = 1 << (level - 1)
    cols = 6
    rows = -(-len(quads) // cols)
    W, H = cols * 2 * s, rows * 2 * s
    depth = np.zeros((H, W), dtype=np.float32)
    where = {}
    for i, (name, (a, b, c, d)) in enumerate(quads.items()):
        r, cc = divmod(i, cols)
        y, x = r * 2 * s, cc * 2 * s
        depth[y:y + s, x:x + s], depth[y:y + s, x + s:x + 2 * s] = a, b
        depth[y + s:y + 2 * s, x:x + s], depth[y + s:y + 2 * s, x + s:x + 2 * s] = c, d
        where[name] = (r, cc)
    rng = np.random.default_rng([seed, level])
    color = rng.random((3, H, W), dtype=np.float32)
    mask = rng.choice(np.array([1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0.5, 2, np.nan], dtype=np.float32), size=(H, W))
    mask[:2 * s, :4 * s] = 1.0                 # (two cells whose mask is 1 for certain)
    return color, depth, mask, where


def _quads(p):
    H2, W2 = p.shape[-2] // 2, p.shape[-1] // 2
    p = p[..., :2 * H2, :2 * W2]
    return p[..., 0::2, 0::2], p[..., 0::2, 1::2], p[..., 1::2, 0::2], p[..., 1::2, 1::2]      # a, b, c, d


def pyramid_level(color, depth, mask, band=0.05, dtype=np.float32):
    """One halving: colour ((a + b) + (c + d)) 0.25; depth the mean, in the order a, b, c, d, of the valid (> 0 and < +inf) readings
    <= m (1 + band), m the smallest valid one, 0 without any (+inf is never valid: a quad of +inf alone gives 0, and no band, however
    wide, lets +inf into a mean); mask 1 iff all four are 1."""
    f = dtype
    a, b, c, d = _quads(np.asarray(color, dtype=f))
    with np.errstate(invalid="ignore", over="ignore"):
        col = ((a + b) + (c + d)) * f(0.25)
    dep = msk = None
    if depth is not None:
        q = _quads(np.asarray(depth, dtype=f))
        big = f(np.inf)
        valid = [(r > 0) & (r < big) for r in q]
        m = np.minimum(np.minimum(np.where(valid[0], q[0], big), np.where(valid[1], q[1], big)),
                       np.minimum(np.where(valid[2], q[2], big), np.where(valid[3], q[3], big)))
        total, n = np.zeros_like(m), np.zeros_like(m)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            lim = m * (f(1) + f(band))
            for r, ok in zip(q, valid):
                take = ok & (r <= lim)
                total = np.where(take, total + r, total)
                n = n + take.astype(f)
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
