"""The three rules of csrc/cloud_image.hip - PROJECT, RESOLVE, DENSIFY of include/gsr.h - restated in numpy, operation by
operation in float32 with the point transform in float64, the way image_reference.py restates register_depth.  Needs no device.
The tests compare the kernels' outputs with these bit for bit.

Error bound of the bilinear colour (used by test_cloud_image_cpu.py): on an image that is linear in the pixel coordinates,
I(x, y) = a x + b y + c, the taps are float32 roundings of exact values of magnitude <= M, and the sample is built from 3 lerps of
3 operations each on top of tx = px - floor(px) and ty (exact: Sterbenz, or a difference of a float and an integer below it with
no more bits than the float).  In exact arithmetic on exact taps the three lerps give I(px, py) itself (away from the image's
edge, where the taps are clamped).  Each of the 9 operations rounds a value of magnitude <= 2 M (a difference of two taps is
the largest intermediate) to within 2 M eps, eps = 2^-24, and reaches the result through operations whose derivative with
respect to it is at most 1 in magnitude (tx, ty in [0, 1]); a tap's rounding, <= M eps, passes through two lerps with a weight of
at most 1 in each and is counted as 2 M eps.  |sample - I(px, py)| <= (9 * 2 + 4 * 2) M eps = 26 M eps = BILINEAR_OPS_BOUND M eps."""
from collections import namedtuple

import numpy as np

F32 = np.float32
UNTOUCHED = np.uint32(0xFFFFFFFF)
NO_WINNER = np.uint64(0xFFFFFFFFFFFFFFFF)
MAX_FOOTPRINT = 4
MAX_RADIUS = 8
BILINEAR_OPS_BOUND = 26.0
EPS = 2.0 ** -24

Projection = namedtuple("Projection", "depth index pixel z visible colors n_visible n_candidates px py takes_part zocc")


def occlusion_scale(occlusion):
    """float32(1 + relative margin), the sum in float64: what the host forms"""
    return F32(1.0 + float(occlusion))


def transform(points, T):
    """q = T p: products and sums in float64 in the order ((T0 x + T1 y) + T2 z) + T3, one rounding to float32"""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    T = np.asarray(T, dtype=np.float64)[:3]
    with np.errstate(all="ignore"):
        return [(((T[i, 0] * p[:, 0] + T[i, 1] * p[:, 1]) + T[i, 2] * p[:, 2]) + T[i, 3]).astype(F32) for i in range(3)]


def project(points, W, H, K, T, footprint=2, scale=F32(1.05), z_near=0.05, z_far=100.0, image=None, mask=None, colors=None):
    """points [N,3], K = (fx, fy, cx, cy), T = [3,4] or [4,4] float64 cloud frame -> camera, scale = occlusion_scale(...).
    `colors`: the array the visible rows are painted into (a copy; None with an image: zeros).  -> Projection."""
    points = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    N, r = points.shape[0], int(footprint)
    fx, fy, cx, cy = (F32(v) for v in K)
    zn, zf, scale, half = F32(z_near), F32(z_far), F32(scale), F32(0.5)
    qx, qy, qz = transform(points, T)
    with np.errstate(all="ignore"):
        part = np.isfinite(qx) & np.isfinite(qy) & np.isfinite(qz) & (qz >= zn) & (qz <= zf)
        px = fx * (qx / qz) + cx
        py = fy * (qy / qz) + cy
        u = np.clip(np.floor(px + half), F32(-(r + 1)), F32(W + r))
        v = np.clip(np.floor(py + half), F32(-(r + 1)), F32(H + r))
    u = np.where(part, u, F32(-(r + 1))).astype(np.int64)
    v = np.where(part, v, F32(-(r + 1))).astype(np.int64)
    zb = qz.view(np.uint32)
    zocc = np.full(W * H, UNTOUCHED, dtype=np.uint32)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            x, y = u + dx, v + dy
            m = part & (x >= 0) & (x < W) & (y >= 0) & (y < H)
            if m.any():
                np.minimum.at(zocc, y[m] * W + x[m], zb[m])
    cand = part & (u >= 0) & (u < W) & (v >= 0) & (v < H)
    at = np.where(cand, v * W + u, 0)
    if mask is not None:
        cand &= np.asarray(mask, dtype=np.float32).reshape(-1)[at] != 0
    pixel = np.where(cand, at, -1).astype(np.int32)
    win = np.full(W * H, NO_WINNER, dtype=np.uint64)
    rows = np.arange(N, dtype=np.uint64)
    key = (zb.astype(np.uint64) << np.uint64(32)) | rows
    np.minimum.at(win, pixel[cand], key[cand])
    z = np.where(part, qz, F32(0)).astype(F32)
    # resolve
    limit = np.zeros(N, dtype=F32)
    with np.errstate(all="ignore"):
        limit[cand] = zocc[pixel[cand]].view(F32) * scale
    visible = cand & (z <= limit)
    has = win != NO_WINNER
    wz = (win >> np.uint64(32)).astype(np.uint32).view(F32)
    wi = (win & np.uint64(0xFFFFFFFF)).astype(np.int64)
    with np.errstate(all="ignore"):
        seen = has & (wz <= zocc.view(F32) * scale)
    depth = np.where(seen, wz, F32(0)).astype(F32).reshape(H, W)
    index = np.where(seen, wi, -1).astype(np.int32).reshape(H, W)
    out_colors = None
    if image is not None:
        out_colors = np.zeros((N, 3), dtype=F32) if colors is None else np.array(colors, dtype=F32).reshape(N, 3).copy()
        out_colors[visible] = bilinear(image, px[visible], py[visible])
    return Projection(depth, index, pixel, z, visible, out_colors, int(visible.sum()), int(cand.sum()), px, py, part,
                      zocc.reshape(H, W))


def bilinear(image, px, py):
    """[3,H,W] sampled at float32 (px, py) -> [n,3]: taps clamped to the image, horizontal lerps first, then the vertical one,
    each a + t * (b - a) in float32"""
    image = np.asarray(image, dtype=np.float32)
    _, H, W = image.shape
    px, py = np.asarray(px, dtype=F32), np.asarray(py, dtype=F32)
    x0f, y0f = np.floor(px), np.floor(py)
    tx, ty = px - x0f, py - y0f
    xl, yl = x0f.astype(np.int64), y0f.astype(np.int64)
    xa, xb = np.clip(xl, 0, W - 1), np.clip(xl + 1, 0, W - 1)
    ya, yb = np.clip(yl, 0, H - 1), np.clip(yl + 1, 0, H - 1)
    out = np.empty((px.shape[0], 3), dtype=F32)
    for c in range(3):
        a, b, cc, d = image[c, ya, xa], image[c, ya, xb], image[c, yb, xa], image[c, yb, xb]
        top = a + tx * (b - a)
        bot = cc + tx * (d - cc)
        out[:, c] = top + ty * (bot - top)
    return out


def densify(depth, radius=4, band_scale=F32(1.05), min_neighbors=2, details=False):
    """[H,W] -> (dense, valid): see DENSIFY in include/gsr.h.  details=True also returns (zn, band_lo, band_hi, count): per pixel
    the nearest reading of its window and the smallest / largest in-band reading and their number (holes only; inf / 0
    elsewhere)."""
    depth = np.asarray(depth, dtype=np.float32)
    H, W = depth.shape
    R, band_scale = int(radius), F32(band_scale)
    pad = np.zeros((H + 2 * R, W + 2 * R), dtype=F32)
    pad[R:R + H, R:R + W] = depth
    inf = F32(np.inf)
    zn = np.full((H, W), inf, dtype=F32)
    shifts = [(dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1)]      # row-major window order
    for dy, dx in shifts:
        z = pad[R + dy:R + dy + H, R + dx:R + dx + W]
        zn = np.where((z > 0) & (z < zn), z, zn)
    with np.errstate(all="ignore"):
        band = zn * band_scale
    sw, swz = np.zeros((H, W), dtype=F32), np.zeros((H, W), dtype=F32)
    cnt = np.zeros((H, W), dtype=np.int64)
    lo, hi = np.full((H, W), inf, dtype=F32), np.zeros((H, W), dtype=F32)
    for dy, dx in shifts:
        if dy == 0 and dx == 0:
            continue                                  # (the centre of a hole holds no reading)
        z = pad[R + dy:R + dy + H, R + dx:R + dx + W]
        m = (z > 0) & (z <= band)
        w = F32(1.0) / F32(dx * dx + dy * dy)
        sw = np.where(m, sw + w, sw)
        swz = np.where(m, swz + w * z, swz)
        cnt += m
        lo, hi = np.where(m, np.minimum(lo, z), lo), np.where(m, np.maximum(hi, z), hi)
    hole = ~(depth > 0)
    fill = hole & (zn < inf) & (cnt >= int(min_neighbors))
    with np.errstate(all="ignore"):
        dense = np.where(hole, np.where(fill, swz / sw, F32(0)), depth).astype(F32)
    valid = np.where(hole, fill, True).astype(F32)
    if details:
        return dense, valid, (np.where(hole, zn, inf), np.where(hole, lo, inf), np.where(hole, hi, F32(0)), np.where(hole, cnt, 0))
    return dense, valid


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def wall_and_box(W, H, K, wall_z=6.0, box_z=2.0, box=(0.35, 0.65, 0.3, 0.7), wall_step=1.0, box_step=2.0):
    """A wall at wall_z sampled every wall_step pixels and, in front of it, a box at box_z covering the image rectangle `box`
    (fractions x0, x1, y0, y1) sampled every box_step pixels, both on pixel centres of the camera K with the identity pose.
    -> (points [N,3] float32, is_box [N], behind [N]: wall rows whose pixel lies inside the box's rectangle, at least one box
    sample spacing from its edge)"""
    fx, fy, cx, cy = K

    def sheet(us, vs, z):
        uu, vv = np.meshgrid(us, vs)
        uu, vv = uu.reshape(-1), vv.reshape(-1)
        return np.stack([(uu - cx) / fx * z, (vv - cy) / fy * z, np.full(uu.shape, z)], axis=1), uu, vv
    wall, wu, wv = sheet(np.arange(0, W, wall_step), np.arange(0, H, wall_step), wall_z)
    bx0, bx1, by0, by1 = box[0] * W, box[1] * W, box[2] * H, box[3] * H
    bus = np.arange(np.ceil(bx0), bx1, box_step)
    bvs = np.arange(np.ceil(by0), by1, box_step)
    boxp, _, _ = sheet(bus, bvs, box_z)
    behind = (wu >= bus[0]) & (wu <= bus[-1]) & (wv >= bvs[0]) & (wv <= bvs[-1])
    points = np.concatenate([wall, boxp]).astype(np.float32)
    is_box = np.concatenate([np.zeros(len(wall), bool), np.ones(len(boxp), bool)])
    return points, is_box, np.concatenate([behind, np.zeros(len(boxp), bool)])


def scan_rings(W, H, K, beams=32, per_ring=360, wall_z=6.0, box_z=2.0, box_half=(0.5, 0.4), seed=0):
    """A spinning-LiDAR style sample of a wall (z = wall_z) with a box (|x| <= box_half[0], |y| <= box_half[1] at z = box_z) in
    front, seen from the camera's origin: `beams` elevation rings, `per_ring` azimuth steps across a field a little wider than
    the camera's, each ray cut at the nearer surface.  -> points [N,3] float32 in the camera frame (x right, y down, z ahead)."""
    fx, fy, cx, cy = K
    rng = np.random.default_rng(seed)
    half_x, half_y = np.arctan(0.55 * W / fx), np.arctan(0.55 * H / fy)
    az = np.linspace(-half_x, half_x, per_ring)
    el = np.linspace(-half_y, half_y, beams)
    aa, ee = np.meshgrid(az, el)
    dx, dy = np.tan(aa).reshape(-1), (np.tan(ee) / np.cos(aa)).reshape(-1)
    hits_box = (np.abs(dx * box_z) <= box_half[0]) & (np.abs(dy * box_z) <= box_half[1])
    z = np.where(hits_box, box_z, wall_z) * (1.0 + 0.002 * rng.standard_normal(dx.shape))
    return np.stack([dx * z, dy * z, z], axis=1).astype(np.float32)
