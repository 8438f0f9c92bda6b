"""CPU restatements for the registration tests (float64 on the host; nothing of the product is imported).

apply_transform: q = (float32)(R s + t) in the order include/gsr.h documents - ((T[i,0] x + T[i,1] y) + T[i,2] z) + T[i,3],
  every numpy float64 operation rounded on its own, one rounding to float32.  The device must give the same bits.
nearest: chunked brute force, distances in float64 from the float32 coordinates (exact differences), the tie rule (d2, row): the
  first minimum in row order; also the second-best distance, for the preconditions of the end-to-end inputs.  (The chunked
  differences run on torch's float64 CPU tensors - the same IEEE operations as numpy's, on several threads.)
kabsch: the rigid dT that minimises sum |dT q - p|^2 by numpy.linalg.svd with the determinant fix.
icp: the loop of scene_utils.registration_icp with the same stopping rule, and a record of every iteration."""
import numpy as np
import torch

INF = float("inf")


def apply_transform(T, points):
    """-> float32 [P,3]; T None = the identity (same formula: x * 1 + y * 0 ...)."""
    T = np.eye(4) if T is None else np.asarray(T, dtype=np.float64)
    p = np.asarray(points, dtype=np.float32).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        q = [((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3] for i in range(3)]
        return np.stack(q, axis=1).astype(np.float32)


def max_dist2(max_distance):
    """the threshold as the product compares it: the float32 square of the float32 distance"""
    d = np.float32(max_distance)
    with np.errstate(over="ignore"):
        return float(np.float32(d * d))


def finite_rows(points):
    return np.isfinite(np.asarray(points, dtype=np.float64)).all(axis=1)


def nearest(q, target, max_distance=INF, chunk=1024):
    """q float32 [P,3] (already transformed), target float32 [Pt,3] -> dict(idx int64 [P] (-1: none), d2 float64 [P] of the
    nearest finite target row (+inf: none; NOT cut at max_distance), second float64 [P], valid bool [P] = d2 <= max_dist2)."""
    qt = torch.from_numpy(np.asarray(q, dtype=np.float32)).double()
    tt = torch.from_numpy(np.asarray(target, dtype=np.float32)).double()
    okt = torch.isfinite(tt).all(dim=1)
    okq = torch.isfinite(qt).all(dim=1)
    tt = torch.where(okt[:, None], tt, torch.zeros_like(tt))
    qt = torch.where(okq[:, None], qt, torch.zeros_like(qt))
    P = qt.shape[0]
    idx = torch.full((P,), -1, dtype=torch.int64)
    d2 = torch.full((P,), INF, dtype=torch.float64)
    second = torch.full((P,), INF, dtype=torch.float64)
    for i in range(0, P, chunk):
        e = qt[i:i + chunk, None, :] - tt[None, :, :]
        d = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
        d[:, ~okt] = INF
        best = torch.argmin(d, dim=1)                     # the first minimum: the smallest row among equal distances
        r = torch.arange(d.shape[0])
        d2[i:i + chunk] = d[r, best]
        idx[i:i + chunk] = best
        if d.shape[1] > 1:
            d[r, best] = INF
            second[i:i + chunk] = d.min(dim=1).values
    none = ~okq | ~torch.isfinite(d2)
    idx[none] = -1
    d2[none] = INF
    second[none] = INF
    d2, second, idx = d2.numpy(), second.numpy(), idx.numpy()
    valid = (idx >= 0) & (d2 <= max_dist2(max_distance))
    return dict(idx=idx, d2=d2, second=second, valid=valid)


def correspondences(near):
    """int32 [P]: the row, -1 where the correspondence is not valid - what the product returns"""
    return np.where(near["valid"], near["idx"], -1).astype(np.int32)


def margins(near, max_distance):
    """The two conditions under which float32 distances must select what float64 selects, over the rows that matter:
    (smallest relative gap between best and second-best among rows whose best is valid, smallest relative distance of a best d2
    from the threshold)."""
    d2, second = near["d2"], near["second"]
    has = near["idx"] >= 0
    thr = max_dist2(max_distance)
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = np.where(has & near["valid"] & np.isfinite(second), (second - d2) / np.maximum(second, 1e-300), INF)
        band = np.where(has, np.abs(d2 - thr) / thr, INF) if np.isfinite(thr) else np.full(d2.shape, INF)
    return float(gap.min()) if gap.size else INF, float(band.min()) if band.size else INF


def kabsch(q, p):
    """rigid dT [4,4] float64 minimising sum |dT q - p|^2 (rows of q onto rows of p); a proper rotation always"""
    q, p = np.asarray(q, dtype=np.float64), np.asarray(p, dtype=np.float64)
    qb, pb = q.mean(axis=0), p.mean(axis=0)
    H = (q - qb).T @ (p - pb)
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0])
    R = Vt.T @ D @ U.T
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, pb - R @ qb
    return T


def update(source, target, corr, T):
    """One ICP update from given correspondences (-1 = none) -> dict(T new [4,4], n, fitness, rmse, sum_d2, status): the sums
    over the valid rows with q = apply_transform(T, source), in float64; fitness and rmse describe the incoming T.  n < 3: T
    stays and status = 1."""
    T = np.eye(4) if T is None else np.asarray(T, dtype=np.float64)
    corr = np.asarray(corr)
    q = apply_transform(T, source).astype(np.float64)
    use = corr >= 0
    q, p = q[use], np.asarray(target, dtype=np.float32).astype(np.float64)[corr[use]]
    n = int(use.sum())
    sum_d2 = float(((q - p) ** 2).sum())
    out = dict(n=n, fitness=n / corr.shape[0], rmse=float(np.sqrt(sum_d2 / n)) if n else 0.0, sum_d2=sum_d2)
    if n < 3:
        return dict(out, T=T.copy(), status=1)
    return dict(out, T=kabsch(q, p) @ T, status=0)


def icp(source, target, max_distance, init=None, relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30):
    """-> dict(T final, iterations, converged, fitness, rmse, corr (of the final T), history: per iteration k the incoming T_k, its
    correspondences, fitness_k, rmse_k and margins).  Iteration k: neighbours under T_k, T_{k+1} = dT T_k; stop after it when
    k >= 1 and |fitness_k - fitness_{k-1}| < relative_fitness and |rmse_k - rmse_{k-1}| < relative_rmse."""
    T = np.eye(4) if init is None else np.asarray(init, dtype=np.float64).copy()
    history, converged = [], False
    for k in range(max_iteration):
        near = nearest(apply_transform(T, source), target, max_distance)
        corr = correspondences(near)
        u = update(source, target, corr, T)
        history.append(dict(T=T, corr=corr, fitness=u["fitness"], rmse=u["rmse"], margins=margins(near, max_distance)))
        T = u["T"]
        if k >= 1 and abs(history[k]["fitness"] - history[k - 1]["fitness"]) < relative_fitness and \
                abs(history[k]["rmse"] - history[k - 1]["rmse"]) < relative_rmse:
            converged = True
            break
    near = nearest(apply_transform(T, source), target, max_distance)
    corr = correspondences(near)
    u = update(source, target, corr, T)
    return dict(T=T, iterations=len(history), converged=converged, fitness=u["fitness"], rmse=u["rmse"], corr=corr,
                history=history, final_margins=margins(near, max_distance))


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def rotation(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def rigid_about(centre, axis, angle, shift):
    """[4,4]: rotation about `centre`, then `shift`"""
    R = rotation(axis, angle)
    c = np.asarray(centre, dtype=np.float64)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, c - R @ c + np.asarray(shift, dtype=np.float64)
    return T


def mean_spacing(P, extent):
    """edge of the cube one of P uniformly spread points has to itself in a box of the given extent"""
    return float((np.prod(np.asarray(extent, dtype=np.float64)) / P) ** (1.0 / 3.0))


# the end-to-end inputs: seeds for which tests/test_registration_cpu.py shows the preconditions at every reference iteration
E2E_SEED = 3
E2E_OVERLAP_SEED = 4
E2E_P = 5000
E2E_EXTENT = 2.6


def e2e_full(seed=None):
    """source: 5000 uniform points in a 2.6 cube; target: its float32 rigid copy (5 degrees about the centre, shift of 0.3 mean
    spacings), rows shuffled -> (source, target, T_true, max_distance)"""
    seed = E2E_SEED if seed is None else seed
    rng = np.random.default_rng(seed)
    src = rng.uniform(-1.3, 1.3, size=(E2E_P, 3)).astype(np.float32)
    h = mean_spacing(E2E_P, [E2E_EXTENT] * 3)
    shift = 0.3 * h * np.array([0.6, -0.64, 0.48])
    T = rigid_about([0, 0, 0], [0.3, -0.5, 0.8], np.deg2rad(5.0), shift)
    tgt = apply_transform(T, src)[rng.permutation(E2E_P)]
    return src, tgt, T, 3.0 * h


def e2e_overlap(seed=None):
    """one 5000-point cloud cut into two slabs along x that share 40 % of the source's extent; the target slab moved as in
    e2e_full -> (source, target, T_true, max_distance)"""
    seed = E2E_OVERLAP_SEED if seed is None else seed
    rng = np.random.default_rng(seed + 100)
    cloud = rng.uniform(-1.3, 1.3, size=(2 * E2E_P, 3)).astype(np.float32)
    x = cloud[:, 0]
    src = cloud[x < 0.26][:E2E_P]                       # x in [-1.3, 0.26): 1.56 wide
    keep = cloud[x >= 0.26 - 0.4 * 1.56][:E2E_P]      # shares the last 40 % of it
    h = mean_spacing(2 * E2E_P, [E2E_EXTENT] * 3)
    T = rigid_about([0, 0, 0], [0.3, -0.5, 0.8], np.deg2rad(2.0), 0.3 * h * np.array([0.6, -0.64, 0.48]))
    tgt = apply_transform(T, keep)[rng.permutation(keep.shape[0])]
    return src, tgt, T, 0.5 * h
