"""numpy reference of the sparse-feature kernels (csrc/orb.hip), written from the rules of include/gsr.h - integers and float64,
no look at the kernels - and the images the tests run on: a seeded blocky texture, planted corners, and a textured plane seen
from known poses with exact depth."""
import ctypes

import numpy as np

BORDER, CELL, BINS, RADIUS, NONE = 17, 32, 30, 15, 257
CIRCLE = ((0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1),
          (-2, -2), (-1, -3))


# ---- the rules ---------------------------------------------------------------------------------------------------------------------
def intensity(image):
    image = np.asarray(image, dtype=np.float32)
    if image.ndim == 2:
        return image
    with np.errstate(invalid="ignore", over="ignore"):      # (the tests feed inf and 3e38 on purpose)
        return ((image[0] + image[1]) + image[2]) / np.float32(3.0)


def prepare_ref(image):
    """-> (u8 [H,W] uint8, box [H,W] uint16)"""
    I = intensity(image)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.floor((255.0 * I.astype(np.float64) + 0.5).astype(np.float32))
    v = np.where(np.isnan(v), np.float32(0), v)
    u8 = np.clip(v, 0, 255).astype(np.uint8)
    p = np.pad(u8.astype(np.int64), 2, mode="edge")
    H, W = u8.shape
    box = sum(p[dy:dy + H, dx:dx + W] for dy in range(5) for dx in range(5))
    return u8, box.astype(np.uint16)


def fast_score_at(u8, x, y):
    p = int(u8[y, x])
    c = [int(u8[y + dy, x + dx]) for dx, dy in CIRCLE]
    best = -255
    for s in range(16):
        arc = [c[(s + k) % 16] for k in range(9)]
        best = max(best, min(v - p for v in arc), min(p - v for v in arc))
    return best


def corner_scores(u8, threshold, mask=None):
    """S [H,W] int: the score of every corner, 0 elsewhere"""
    H, W = u8.shape
    S = np.zeros((H, W), dtype=np.int64)
    if H < 2 * BORDER + 1 or W < 2 * BORDER + 1:
        return S
    a = u8.astype(np.int64)
    ys, xs = slice(BORDER, H - BORDER), slice(BORDER, W - BORDER)
    p = a[ys, xs]
    d = np.stack([a[BORDER + dy:H - BORDER + dy, BORDER + dx:W - BORDER + dx] - p for dx, dy in CIRCLE])
    best = np.full(p.shape, -255, dtype=np.int64)
    for s in range(16):
        arc = d[[(s + k) % 16 for k in range(9)]]
        best = np.maximum(best, np.maximum(arc.min(axis=0), (-arc).min(axis=0)))
    ok = best > threshold
    if mask is not None:
        ok &= np.asarray(mask)[ys, xs] > 0
    S[ys, xs] = np.where(ok, best, 0)
    return S


def nms(S):
    """bool [H,W]: the corners that survive the 3 x 3 suppression"""
    H, W = S.shape
    P = np.pad(S, 1)
    keep = S > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx == 0 and dy == 0:
                continue
            q = P[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
            later = (dy, dx) > (0, 0)      # the neighbour comes after the pixel in raster order
            keep &= (S >= q) if later else (S > q)
    return keep


def detect_ref(u8, threshold, per_cell, mask=None):
    """-> slots int32 [cells, per_cell, 3]"""
    H, W = u8.shape
    S = corner_scores(u8, threshold, mask)
    keep = nms(S)
    gx, gy = -(-W // CELL), -(-H // CELL)
    slots = np.zeros((gx * gy, per_cell, 3), dtype=np.int32)
    for cy in range(gy):
        for cx in range(gx):
            ys, xs = np.nonzero(keep[cy * CELL:(cy + 1) * CELL, cx * CELL:(cx + 1) * CELL])
            found = sorted((-int(S[cy * CELL + y, cx * CELL + x]), int(y), int(x)) for y, x in zip(ys, xs))[:per_cell]
            for r, (ns, y, x) in enumerate(found):
                slots[cy * gx + cx, r] = (cx * CELL + x, cy * CELL + y, -ns)
    return slots


def library_pattern():
    """int8 [30,256,4] as gsr_orb_pattern hands it out"""
    from diff_gaussian_rasterization import _C
    buf = (ctypes.c_int8 * (BINS * 256 * 4))()
    _C.check(_C.lib().gsr_orb_pattern(ctypes.cast(buf, ctypes.c_void_p)))
    return np.frombuffer(buf, dtype=np.int8).reshape(BINS, 256, 4).copy()


_DISC = [(dx, dy) for dy in range(-RADIUS, RADIUS + 1) for dx in range(-RADIUS, RADIUS + 1) if dx * dx + dy * dy <= RADIUS * RADIUS]


def describe_ref(u8, box, keypoints, pattern):
    """keypoints int [M,3] -> dict(bin [M], moments [M,2], desc int32 [M,8], margin [M]: the float64 angle's distance in radians
    from the nearest bin boundary; -1 / 0 / 0 / inf for a skipped row)"""
    H, W = u8.shape
    M = len(keypoints)
    out = dict(bin=np.full(M, -1, np.int32), moments=np.zeros((M, 2), np.int32), desc=np.zeros((M, 8), np.uint32),
               margin=np.full(M, np.inf))
    a, b = u8.astype(np.int64), box.astype(np.int64)
    dxs, dys = np.array([d[0] for d in _DISC]), np.array([d[1] for d in _DISC])
    step = 2.0 * np.pi / BINS
    for k, (x, y, s) in enumerate(np.asarray(keypoints).tolist()):
        if s <= 0 or not (BORDER <= x < W - BORDER and BORDER <= y < H - BORDER):
            continue
        v = a[y + dys, x + dxs]
        m10, m01 = int((dxs * v).sum()), int((dys * v).sum())
        t = np.arctan2(float(m01), float(m10)) / step
        bin_ = int(np.floor(t + 0.5)) % BINS
        out["bin"][k], out["moments"][k] = bin_, (m10, m01)
        out["margin"][k] = abs((t + 0.5) - np.round(t + 0.5)) * step
        pt = pattern[bin_].astype(np.int64)
        bits = b[y + pt[:, 1], x + pt[:, 0]] < b[y + pt[:, 3], x + pt[:, 2]]
        out["desc"][k] = [sum(int(bits[32 * w + i]) << i for i in range(32)) for w in range(8)]
    out["desc"] = out["desc"].view(np.int32)
    return out


_POPCOUNT = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint8)


def hamming_matrix(q, db):
    """int [Q,N] distances between int32 [Q,8] and [N,8]: a byte-wise popcount table over the xor"""
    qb = np.ascontiguousarray(q, dtype=np.int32).view(np.uint8).reshape(len(q), 32)
    tb = np.ascontiguousarray(db, dtype=np.int32).view(np.uint8).reshape(len(db), 32)
    return _POPCOUNT[qb[:, None, :] ^ tb[None, :, :]].sum(axis=2, dtype=np.int64)


def hamming_ref(q, db):
    """-> (idx, best, second) int32 [Q]"""
    D = hamming_matrix(q, db)
    Q, N = D.shape
    idx, best, second = np.full(Q, -1, np.int32), np.full(Q, NONE, np.int32), np.full(Q, NONE, np.int32)
    if N:
        idx = D.argmin(axis=1).astype(np.int32)      # (the first of equal minima)
        best = D[np.arange(Q), idx].astype(np.int32)
    if N > 1:
        second = np.sort(D, axis=1)[:, 1].astype(np.int32)
    return idx, best, second


def vote_ref(q, db, segments, max_distance, ratio):
    votes = np.zeros(len(segments) - 1, dtype=np.int32)
    for k in range(len(votes)):
        _, best, second = hamming_ref(q, db[segments[k]:segments[k + 1]])
        if segments[k + 1] > segments[k]:
            ok = (best <= max_distance) & (best.astype(np.float32) < np.float32(ratio) * second.astype(np.float32))
            votes[k] = int(ok.sum())
    return votes


def horn_fit(src, dst):
    """the rigid T (float64 [4,4]) with dst ~ R src + t, least squares (SVD form)"""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    cs, cd = src.mean(axis=0), dst.mean(axis=0)
    U, _, Vt = np.linalg.svd((dst - cd).T @ (src - cs))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    T = np.eye(4)
    T[:3, :3] = U @ D @ Vt
    T[:3, 3] = cd - T[:3, :3] @ cs
    return T


# ---- images ------------------------------------------------------------------------------------------------------------------------
def blocky_texture(h, w, seed, block=5, levels=6):
    """float32 [h,w] in [0.1, 0.9]: random grey levels on blocks of `block` pixels - corners at the block junctions"""
    rng = np.random.RandomState(seed)
    g = rng.randint(0, levels, size=(-(-h // block), -(-w // block))).astype(np.float32)
    img = np.kron(g, np.ones((block, block), dtype=np.float32))[:h, :w]
    return (0.1 + 0.8 * img / (levels - 1)).astype(np.float32)


def plant_corner(img, x, y, value=0.9, size=6):
    """a bright quadrant with its tip at (x, y) on whatever the image holds: a FAST corner at the tip"""
    img[y:y + size, x:x + size] = value
    return img


def pose_w2c(rx, ry, rz, t):
    """world-to-camera [4,4] float64 from small rotations about x, y, z (radians) and a translation"""
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = t
    return T


def plane_view(h, w, K, w2c, seed, plane_z=2.0, block=0.045, levels=6, table=64):
    """A plane z = plane_z of the world, painted with random grey blocks of side `block` (a seeded table, repeated every `table`
    blocks), seen by the pinhole camera K = (fx, fy, cx, cy) at `w2c`.  The texture is evaluated at the ray-plane hit of every
    pixel centre and the depth (camera z) is exact.  -> (image float32 [3,h,w], depth float32 [h,w])"""
    fx, fy, cx, cy = K
    rng = np.random.RandomState(seed)
    tab = rng.randint(0, levels, size=(table, table))
    R, t = w2c[:3, :3], w2c[:3, 3]
    o = -R.T @ t
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], axis=-1) @ R      # R^T d, row form
    s = (plane_z - o[2]) / d[..., 2]
    X = o + s[..., None] * d
    ia = np.floor(X[..., 0] / block).astype(np.int64) % table
    ib = np.floor(X[..., 1] / block).astype(np.int64) % table
    grey = (0.1 + 0.8 * tab[ib, ia] / (levels - 1)).astype(np.float32)
    return np.stack([grey, grey, grey]), s.astype(np.float32)
