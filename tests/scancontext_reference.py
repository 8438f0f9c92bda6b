"""A numpy float64 restatement of the two rules of csrc/scancontext.hip (include/gsr.h: gsr_scan_context,
gsr_scan_context_distance), a cloud generator whose points lie strictly inside their polar cells, and the fixtures the CPU and
GPU tests share.

The generator draws a ring and a sector per point and places the point at a ring fraction and a sector fraction from [0.1, 0.9],
its range below 0.99 max_range: no ring, sector or range decision lies within float32 rounding of a boundary, so a float32
evaluation of the rule MUST find the bins this file finds, and tests may demand equal bins.  Without a frame and with the origin
at 0 the height is one float32 add, which this file performs in float32: such descriptors must agree bit for bit."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
TWO_PI = 2.0 * math.pi


# ---- the rules ------------------------------------------------------------------------------------------------------------------------
def bins(points, rings, sectors, max_range, frame=None, origin=None):
    """-> (p float64 [N,3] in the levelled frame about the origin, ring int [N], sector int [N]); ring = -1 for a skipped row"""
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.asarray(points, dtype=F32).astype(F64).reshape(-1, 3)
        if frame is not None:
            F = np.asarray(frame, dtype=F32).astype(F64).reshape(-1, 4)[:3]
            p = p @ F[:, :3].T + F[:, 3]
        if origin is not None:
            p = p - np.asarray(origin, dtype=F32).astype(F64)
        rho2 = p[:, 0] ** 2 + p[:, 1] ** 2
        ok = np.isfinite(p).all(axis=1) & (rho2 > 0) & (rho2 < float(max_range) ** 2)
        rho = np.sqrt(np.where(ok, rho2, 1.0))
        ring = np.minimum(rings - 1, np.floor(rho * rings / max_range)).astype(np.int64)
        theta = np.arctan2(np.where(ok, p[:, 1], 0.0), np.where(ok, p[:, 0], 1.0))
        theta = np.where(theta < 0, theta + TWO_PI, theta)
        sector = np.minimum(sectors - 1, np.floor(theta * sectors / TWO_PI)).astype(np.int64)
    return p, np.where(ok, ring, -1), np.where(ok, sector, -1)


def descriptor(points, rings, sectors, max_range, height_offset, frame=None, origin=None):
    """float64 [R,S]: the largest max(0, z + height_offset) per cell, 0 where a cell is empty"""
    p, ring, sector = bins(points, rings, sectors, max_range, frame, origin)
    if frame is None and origin is None:      # one float32 add: the kernel's bits
        h = (np.asarray(points, dtype=F32).reshape(-1, 3)[:, 2] + F32(height_offset)).astype(F64)
    else:
        h = p[:, 2] + float(F32(height_offset))
    ok = ring >= 0
    h = np.maximum(np.where(ok, h, 0.0), 0.0)
    desc = np.zeros((rings, sectors), dtype=F64)
    np.maximum.at(desc, (ring[ok], sector[ok]), h[ok])
    return desc


def norms(desc):
    """float64 [..., S]: the Euclidean norm of every column of [..., R, S]"""
    return np.sqrt((np.asarray(desc, dtype=F64) ** 2).sum(axis=-2))


def distance_table(query, database_row):
    """float64 [B,S]: d(b, s) of the query variants [B,R,S] against one database descriptor [R,S]"""
    q, d = np.asarray(query, dtype=F64), np.asarray(database_row, dtype=F64)
    B, R, S = q.shape
    nq, nd = norms(q), norms(d)
    table = np.ones((B, S), dtype=F64)
    for b in range(B):
        for s in range(S):
            acc, n = 0.0, 0
            for c in range(S):
                j = (c + s) % S
                if nq[b, j] != 0 and nd[c] != 0:
                    acc += float(q[b, :, j] @ d[:, c]) / (nq[b, j] * nd[c])
                    n += 1
            if n:
                table[b, s] = 1.0 - acc / n
    return table


def best_of(table):
    """(distance, shift, variant, margin): the smallest entry, ties to the smallest variant, then the smallest shift; margin = the
    second smallest entry minus the smallest (inf for a single entry)"""
    flat = table.reshape(-1)
    i = int(np.argmin(flat))      # (the first of equal entries: variants major, shifts minor)
    rest = np.delete(flat, i)
    return float(flat[i]), i % table.shape[1], i // table.shape[1], float(rest.min() - flat[i]) if rest.size else math.inf


def distance(query, database):
    """the rule against K descriptors [K,R,S] -> (dist float64 [K], shift int [K], variant int [K], margin float64 [K])"""
    out = [best_of(distance_table(query, row)) for row in database]
    return tuple(np.array([o[i] for o in out], dtype=t) for i, t in enumerate((F64, np.int64, np.int64, F64)))


# ---- clouds strictly inside their cells ---------------------------------------------------------------------------------------------
def polar_draw(rng, n, rings, sectors, z_lo=-3.0, z_hi=6.0):
    """n points as (ring, ring fraction, sector, sector fraction, z); fractions from [0.1, 0.9], the range below 0.99 max_range"""
    ring = rng.integers(0, rings, n)
    hi = np.minimum(0.9, 0.99 * rings - ring - 0.01)
    return dict(ring=ring, fr=0.1 + rng.random(n) * (hi - 0.1), sector=rng.integers(0, sectors, n),
                fs=0.1 + 0.8 * rng.random(n), z=z_lo + (z_hi - z_lo) * rng.random(n))


def polar_points(draw, rings, sectors, max_range, shift=0):
    """float32 [n,3] of a draw, every point moved on by `shift` sectors (a rotation by shift 2 pi / S about z)"""
    rho = (draw["ring"] + draw["fr"]) * (max_range / rings)
    theta = (((draw["sector"] + shift) % sectors) + draw["fs"]) * (TWO_PI / sectors)
    return np.stack([rho * np.cos(theta), rho * np.sin(theta), draw["z"]], axis=1).astype(F32)


def make_cloud(seed, n, rings, sectors, max_range, shift=0, **z):
    return polar_points(polar_draw(np.random.default_rng(seed), n, rings, sectors, **z), rings, sectors, max_range, shift)


def to_cloud_frame(points_levelled, frame):
    """float32 [n,3]: the points whose image under `frame` ([3,4], cloud -> levelled) is `points_levelled` (float64 inverse)"""
    F = np.asarray(frame, dtype=F32).astype(F64).reshape(3, 4)
    return ((np.asarray(points_levelled, dtype=F64) - F[:, 3]) @ np.linalg.inv(F[:, :3]).T).astype(F32)


def tilted_frame():
    """a [3,4] float32 frame: a sensor pitched by 7 and rolled by -4 degrees, mounted 0.3 m off the axis and 1.7 m up"""
    a, b = math.radians(7.0), math.radians(-4.0)
    Ry = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    return np.concatenate([Ry @ Rx, np.array([[0.3], [-0.1], [1.7]])], axis=1).astype(F32)


# ---- fixtures of the distance tests -------------------------------------------------------------------------------------------------------
DISTANCE_CASES = [(20, 60, 65, 2), (20, 60, 2, 1), (20, 60, 1, 3), (3, 7, 2, 2), (40, 120, 2, 2), (1, 1, 1, 1)]      # R, S, K, B
MAX_RANGE, HEIGHT_OFFSET = 80.0, 2.0


def distance_fixture(rings, sectors, K, B, seed=5):
    """(query float32 [B,R,S], database float32 [K,R,S], shifts int [K], variants int [K]): the query variants are descriptors of
    B generated clouds; database row k is the cloud of variant k mod B turned BACK by shifts[k] sectors with three tenths of its
    points dropped, another three tenths for every row - so every row has one clear best (variant, shift)"""
    n = 6 * rings * sectors
    draws = [polar_draw(np.random.default_rng(1000 * seed + b), n, rings, sectors) for b in range(B)]
    q = [descriptor(polar_points(d, rings, sectors, MAX_RANGE), rings, sectors, MAX_RANGE, HEIGHT_OFFSET) for d in draws]
    shifts = np.array([(7 * k + 3) % sectors for k in range(K)], dtype=np.int64)
    variants = np.arange(K, dtype=np.int64) % B
    db = np.zeros((K, rings, sectors), dtype=F64)
    for k in range(K):
        keep = np.random.default_rng(2000 * seed + k).random(n) >= 0.3
        pts = polar_points(draws[variants[k]], rings, sectors, MAX_RANGE, shift=-int(shifts[k]))[keep]
        db[k] = descriptor(pts, rings, sectors, MAX_RANGE, HEIGHT_OFFSET)
    return np.stack(q).astype(F32), db.astype(F32), shifts, variants


def one_hot_columns(rings, sectors, period):
    """float32 [R,S]: column c holds the single height 2^(c mod period) in ring c mod period - every cosine between two such
    columns is exactly 0 or 1 in any precision, so a descriptor periodic in its columns ties exactly"""
    d = np.zeros((rings, sectors), dtype=F32)
    for c in range(sectors):
        d[(c % period) % rings, c] = 2.0 ** (c % period)
    return d


# ---- a synthetic levelled scene for the end-to-end test: walls, boxes, poles, ground ---------------------------------------------------
SENSOR_HEIGHT = 1.8
PLACES = [(35.0 * i, 35.0 * j) for j in range(2) for i in range(4)]      # eight places, 35 m apart


def make_scene(seed=11):
    """float64 [M,3] world points (z = 0 is the road): samples of 110 walls, 70 boxes, 90 poles and the ground"""
    rng = np.random.default_rng(seed)
    lo, hi = np.array([-55.0, -55.0]), np.array([160.0, 90.0])
    parts = []
    for _ in range(110):      # a wall: a vertical rectangle
        a = lo + rng.random(2) * (hi - lo)
        ang, length, height = rng.random() * math.pi, 5.0 + 15.0 * rng.random(), 2.0 + 5.0 * rng.random()
        t, z = rng.random(1400), rng.random(1400)
        xy = a + np.outer(t * length, [math.cos(ang), math.sin(ang)])
        parts.append(np.column_stack([xy, np.sqrt(z) * height]))      # (denser towards the top edge, as a scan's upper beams are)
    for _ in range(70):       # a box: four sides and the top
        c = lo + rng.random(2) * (hi - lo)
        sx, sy, sz = 1.5 + 3.0 * rng.random(), 1.5 + 3.0 * rng.random(), 1.0 + 2.0 * rng.random()
        u, v, f = rng.random(500), rng.random(500), rng.integers(0, 5, 500)
        x = np.where(f == 0, 0.0, np.where(f == 1, 1.0, u))
        y = np.where(f == 2, 0.0, np.where(f == 3, 1.0, np.where(f < 2, u, v)))
        z = np.where(f == 4, 1.0, v)
        parts.append(np.column_stack([c[0] + (x - 0.5) * sx, c[1] + (y - 0.5) * sy, z * sz]))
    for _ in range(90):       # a pole
        c = lo + rng.random(2) * (hi - lo)
        ang, z = rng.random(120) * TWO_PI, rng.random(120) * (4.0 + 4.0 * rng.random())
        parts.append(np.column_stack([c[0] + 0.15 * np.cos(ang), c[1] + 0.15 * np.sin(ang), z]))
    g = lo + rng.random((40000, 2)) * (hi - lo)
    parts.append(np.column_stack([g, np.zeros(len(g))]))
    return np.concatenate(parts)


def sensor_pose(place, yaw=0.0, sideways=0.0):
    """float64 [4,4] sensor -> world: the levelled sensor at PLACES[place], SENSOR_HEIGHT up, turned by `yaw`, then moved
    `sideways` along its own y axis"""
    c, s = math.cos(yaw), math.sin(yaw)
    X = np.eye(4)
    X[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    X[:3, 3] = [PLACES[place][0], PLACES[place][1], SENSOR_HEIGHT]
    X[:3, 3] += X[:3, 1] * sideways
    return X


def take_scan(scene, pose, seed, n=4000, max_range=40.0):
    """float32 [n,3] in the sensor frame: n of the scene's points within max_range of the sensor, drawn with `seed`"""
    p = (scene - pose[:3, 3]) @ pose[:3, :3]      # (R^T (x - t), row form)
    near = p[(p[:, 0] ** 2 + p[:, 1] ** 2) < (0.98 * max_range) ** 2]
    pick = np.random.default_rng(seed).permutation(len(near))[:n]
    return near[np.sort(pick)].astype(F32)
