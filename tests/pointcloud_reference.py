"""CPU restatements for the point-cloud conditioning tests (numpy / torch on the host; nothing of the product is imported).

knn_k_reference: float64 brute force on the float32 inputs.
voxel_cells_f32: the lattice in float32 numpy, one rounding per operation - what the kernel must reproduce bit for bit;
voxel_cells_f64: the same lattice in float64, independent of the float32 one (they agree away from cell faces).
voxel_down_sample_reference: membership from the float32 lattice, means in float64.
statistical_outlier_reference: Open3D's remove_statistical_outlier as recalled (the search returns the query itself, so the mean
runs over nb_neighbors values of which one is 0; sample standard deviation; keep iff 0 < mean < mu + ratio sigma)."""
import numpy as np
import torch

VOXEL_INDEX_LIMIT = 1 << 20


def finite_rows(points):
    return np.isfinite(np.asarray(points, dtype=np.float64)).all(axis=1)


def knn_k_reference(points, k):
    """-> (dist2 [P,k] float64 ascending with a +inf tail, mean [P] float64).  k_eff = min(k, P - 1); mean = sum of the square
    roots of the finite ones among the first k_eff / (k_eff + 1).  Rows with a non-finite coordinate are nobody's neighbour and
    get +inf / NaN themselves."""
    x = torch.as_tensor(np.asarray(points, dtype=np.float32)).double()
    P = x.shape[0]
    ok = torch.isfinite(x).all(dim=1)
    xs = torch.where(ok[:, None], x, torch.zeros_like(x))
    out = torch.full((P, k), float("inf"), dtype=torch.float64)
    kk = min(k, P)
    for i in range(0, P, 1024):
        d2 = ((xs[i:i + 1024, None, :] - xs[None, :, :]) ** 2).sum(-1)
        d2[:, ~ok] = float("inf")
        r = torch.arange(d2.shape[0])
        d2[r, r + i] = float("inf")
        out[i:i + 1024, :kk] = torch.topk(d2, kk, dim=1, largest=False, sorted=True).values
    out[~ok, :] = float("inf")
    return out.numpy(), knn_mean_from_dist2(out.numpy(), k, ok.numpy())


def knn_mean_from_dist2(dist2, k, ok=None):
    """the mean distance of knn_k_reference from its (or a wider) dist2 table: the first k columns"""
    P = dist2.shape[0]
    keff = min(k, P - 1)
    head = dist2[:, :keff]
    with np.errstate(invalid="ignore"):
        mean = np.where(np.isfinite(head), np.sqrt(head), 0.0).sum(axis=1) / (keff + 1)
    if ok is not None:
        mean[~ok] = np.nan
    return mean


def voxel_origin_f32(points, voxel_size, origin=None):
    """the lattice origin as float32: the caller's, or per axis (smallest finite coordinate) - 0.5 voxel_size"""
    if origin is not None:
        return np.asarray(origin, dtype=np.float32)
    p = np.asarray(points, dtype=np.float32)
    lo = np.array([p[np.isfinite(p[:, a]), a].min() if np.isfinite(p[:, a]).any() else np.inf for a in range(3)], dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (lo - np.float32(0.5) * np.float32(voxel_size)).astype(np.float32)


def voxel_cells_f32(points, voxel_size, origin=None):
    """-> (cells int64 [P,3], kept bool [P]): floor((p - o) / v) with every operation a float32 operation."""
    p = np.asarray(points, dtype=np.float32)
    v = np.float32(voxel_size)
    kept = np.isfinite(p).all(axis=1)
    o = voxel_origin_f32(p, voxel_size, origin)
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor(((p - o[None, :]).astype(np.float32) / v).astype(np.float32))
    cells = np.zeros(p.shape, dtype=np.int64)
    cells[kept] = f[kept].astype(np.int64)
    return cells, kept


def voxel_cells_f64(points, voxel_size, origin):
    p = np.asarray(points, dtype=np.float64)
    return np.floor((p - np.asarray(origin, dtype=np.float64)[None, :]) / float(voxel_size)).astype(np.int64)


def voxel_in_range(cells, kept):
    c = cells[kept]
    return bool(((c >= -VOXEL_INDEX_LIMIT) & (c < VOXEL_INDEX_LIMIT)).all())


def voxel_down_sample_reference(points, colors, voxel_size, origin=None):
    """-> dict(points float64 [V,3], colors float64 [V,3] or None, counts int64 [V], cells int64 [V,3]) in ascending
    (i_z, i_y, i_x); the membership is the float32 lattice's."""
    cells, kept = voxel_cells_f32(points, voxel_size, origin)
    p = np.asarray(points, dtype=np.float32).astype(np.float64)[kept]
    c = cells[kept]
    if p.shape[0] == 0:
        return dict(points=np.zeros((0, 3)), colors=None if colors is None else np.zeros((0, 3)), counts=np.zeros(0, np.int64),
                    cells=np.zeros((0, 3), np.int64))
    uniq, inv, counts = np.unique(c[:, ::-1], axis=0, return_inverse=True, return_counts=True)      # rows sorted by (z, y, x)
    inv = inv.reshape(-1)
    V = uniq.shape[0]
    mean = np.zeros((V, 3))
    np.add.at(mean, inv, p)
    mean /= counts[:, None]
    col = None
    if colors is not None:
        col = np.zeros((V, 3))
        np.add.at(col, inv, np.asarray(colors, dtype=np.float32).astype(np.float64)[kept])
        col /= counts[:, None]
    return dict(points=mean, colors=col, counts=counts.astype(np.int64), cells=uniq[:, ::-1].copy())


def statistical_outlier_reference(points, nb_neighbors=20, std_ratio=2.0):
    """-> dict(dbar [P], n_valid, mu, sigma, threshold, keep bool [P]) in float64."""
    _, dbar = knn_k_reference(points, nb_neighbors - 1)
    ok = np.isfinite(dbar)
    n = int(ok.sum())
    mu = float(dbar[ok].mean()) if n else 0.0
    sigma = float(np.sqrt(((dbar[ok] - mu) ** 2).sum() / (n - 1))) if n >= 2 else 0.0
    thr = mu + std_ratio * sigma
    with np.errstate(invalid="ignore"):
        keep = ok & (dbar > 0) & (dbar < thr)
    return dict(dbar=dbar, n_valid=n, mu=mu, sigma=sigma, threshold=thr, keep=keep)


def condition_reference(points, colors, voxel_size, nb_neighbors, std_ratio, origin=None):
    """down-sample (float64 means rounded to float32, as the product hands them on), then filter -> (points f32, colors f32,
    the filter's reference on the down-sampled cloud)"""
    vox = voxel_down_sample_reference(points, colors, voxel_size, origin)
    p32 = vox["points"].astype(np.float32)
    so = statistical_outlier_reference(p32, nb_neighbors, std_ratio)
    return p32, None if vox["colors"] is None else vox["colors"].astype(np.float32), so


# ---- clouds -----------------------------------------------------------------------------------------------------------------------
def uniform_cloud(P, seed):
    return (np.random.default_rng(seed).uniform(-1.3, 1.3, size=(P, 3))).astype(np.float32)


def clustered_cloud(P, seed, offset=1000.0):
    rng = np.random.default_rng(seed)
    centres = rng.uniform(0, 4, size=(12, 3))
    return (offset + centres[rng.integers(0, 12, size=P)] + 0.02 * rng.standard_normal((P, 3))).astype(np.float32)


def duplicate_cloud(P, seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1, 1, size=(P, 3)).astype(np.float32)
    if P >= 4:
        n = max(1, P // 10)
        p[P - n:] = p[rng.integers(0, P - n, size=n)]
        m = min(P, 40)
        p[:m] = p[0]
    return p[rng.permutation(P)]


def surface_with_outliers(seed, n_surface=3000, n_far=30):
    """a gently curved patch of ~1 x 1 (jittered grid: no two points coincide) + points planted far off it"""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n_surface)))
    gy, gx = np.mgrid[0:side, 0:side]
    uv = (np.stack([gx.ravel(), gy.ravel()], axis=1)[:n_surface] + rng.uniform(-0.35, 0.35, size=(n_surface, 2))) / side
    z = 0.1 * np.sin(3 * uv[:, 0]) * np.cos(2 * uv[:, 1]) + 0.002 * rng.standard_normal(n_surface)
    surf = np.concatenate([uv, z[:, None]], axis=1)
    far = np.concatenate([rng.uniform(0, 1, size=(n_far, 2)), rng.uniform(0.6, 1.5, size=(n_far, 1)) *
                          rng.choice([-1.0, 1.0], size=(n_far, 1))], axis=1)
    pts = np.concatenate([surf, far]).astype(np.float32)
    planted = np.zeros(pts.shape[0], dtype=bool)
    planted[n_surface:] = True
    perm = rng.permutation(pts.shape[0])
    return pts[perm], planted[perm]
