"""CPU restatements for the generalized-ICP tests (float64 on the host; nothing of the product is imported).  The three rules of
include/gsr.h, "generalized ICP":

covariances: the neighbourhood and the normal of normals_reference.analyse (brute force, numpy.linalg.eigh), Sigma = I - (1 -
  epsilon) n n^T; I where the neighbourhood has fewer than three rows, NaN for a non-finite row.
regularize: numpy.linalg.eigh of a given symmetric matrix, the eigenvector of the smallest eigenvalue, the same Sigma; I where the
  three eigenvalues are equal, NaN for a non-finite row.
generalized_update: one update about the shift the product documents (the target point of the first row whose q and p are finite),
  M = Sigma_t + R Sigma_s R^T, W = adj(M) / det M by the header's formula, the header's validity rule, J^T W J and J^T W d in
  float64, numpy.linalg.solve, dT = Tr(c) [Rz Ry Rx, t] Tr(-c).
icp_generalized: the loop of registration_icp with the same stopping rule, a per-iteration history like normals_reference.icp_plane.

A covariance is six values per row: xx, xy, xz, yy, yz, zz."""
import numpy as np

import normals_reference as NR
import registration_reference as RR

INF = float("inf")
EPSILON = 1e-3
SIX = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def full(c6):
    """[P,6] -> symmetric [P,3,3]"""
    c6 = np.asarray(c6, dtype=np.float64)
    m = np.empty(c6.shape[:-1] + (3, 3))
    for k, (a, b) in enumerate(SIX):
        m[..., a, b] = m[..., b, a] = c6[..., k]
    return m


def six(m):
    """symmetric [P,3,3] -> [P,6]"""
    m = np.asarray(m, dtype=np.float64)
    return np.stack([m[..., a, b] for a, b in SIX], axis=-1)


def from_normals(normals, epsilon=EPSILON):
    """I - (1 - epsilon) n n^T as [P,6] (NaN where n is)"""
    n = np.asarray(normals, dtype=np.float64)
    return six(np.eye(3)[None] - (1.0 - epsilon) * n[:, :, None] * n[:, None, :])


def covariances(points, radius, max_nn, epsilon=EPSILON, analysis=None):
    """-> dict(cov float64 [P,6], count int64 [P], gap float64 [P] = (l1 - l0) / l2 of the sample covariance, NaN where it does
    not exist).  analysis: the entry of NR.analyse for (radius, max_nn), where the caller has it."""
    a = NR.analyse(points, [(radius, max_nn)])[0] if analysis is None else analysis
    cov = from_normals(a["normal"], epsilon)
    cov[a["finite"] & (a["count"] < 3)] = six(np.eye(3))
    cov[~a["finite"]] = np.nan
    return dict(cov=cov, count=a["count"], gap=a["gap"])


def sample_covariances(points, radius, max_nn, chunk=256):
    """the neighbourhood's covariance C = S2 / n - (S1 / n)(S1 / n)^T itself, [P,3,3] (brute force; the rule of NR.analyse
    restated with numpy) and its count"""
    p = np.asarray(points, dtype=np.float32)
    P = p.shape[0]
    ok = np.isfinite(p).all(axis=1)
    ps = np.where(ok[:, None], p, np.float32(0))
    r2 = NR.radius2(radius)
    C, count = np.zeros((P, 3, 3)), np.zeros(P, np.int64)
    for i in range(0, P, chunk):
        delta = (ps[None, :, :] - ps[i:i + chunk, None, :]).astype(np.float64)
        d2 = (delta[..., 0] * delta[..., 0] + delta[..., 1] * delta[..., 1]) + delta[..., 2] * delta[..., 2]
        c = d2.shape[0]
        other = np.repeat(ok[None, :], c, axis=0)
        other[np.arange(c), np.arange(c) + i] = False
        d2o = np.where(other, d2, INF)
        k = max_nn - 1
        dk = np.sort(d2o, axis=1)[:, k - 1] if P >= k else np.full(c, INF)
        member = other & (d2 <= np.minimum(dk, r2)[:, None])
        n = 1.0 + member.sum(axis=1)
        S1 = np.einsum("cp,cpk->ck", member.astype(np.float64), delta)
        S2 = np.einsum("cp,cpk,cpl->ckl", member.astype(np.float64), delta, delta)
        mean = S1 / n[:, None]
        C[i:i + c] = S2 / n[:, None, None] - mean[:, :, None] * mean[:, None, :]
        count[i:i + c] = n
    count[~ok] = 0
    return C, count


def regularize(cov6, epsilon=EPSILON):
    """-> dict(cov float64 [P,6], gap float64 [P] = (l1 - l0) / l2 of the given matrices, NaN where it does not exist)"""
    c = np.asarray(cov6, dtype=np.float64)
    ok = np.isfinite(c).all(axis=1)
    w, v = np.linalg.eigh(full(np.where(ok[:, None], c, 0.0)))
    out = from_normals(v[:, :, 0], epsilon)
    out[(w[:, 0] == w[:, 1]) & (w[:, 1] == w[:, 2])] = six(np.eye(3))
    out[~ok] = np.nan
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = np.where(ok & (w[:, 2] > 0), (w[:, 1] - w[:, 0]) / w[:, 2], np.nan)
    return dict(cov=out, gap=gap)


def adjugate_inverse(M):
    """-> (W [n,3,3], det [n]) by the formula of include/gsr.h, M symmetric [n,3,3]"""
    m0, m1, m2, m3, m4, m5 = M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2]
    k00, k01, k02 = m3 * m5 - m4 * m4, m2 * m4 - m1 * m5, m1 * m4 - m2 * m3
    k11, k12, k22 = m0 * m5 - m2 * m2, m1 * m2 - m0 * m4, m0 * m3 - m1 * m1
    det = (m0 * k00 + m1 * k01) + m2 * k02
    with np.errstate(invalid="ignore", divide="ignore"):
        W = full(np.stack([k00, k01, k02, k11, k12, k22], axis=1) / det[:, None])
    return W, det


def generalized_system(source, source_cov, target, target_cov, corr, T):
    """-> dict(use bool [Ps], c, M [n,3,3], W [n,3,3], JTWJ, JTWd, n, sum_d2, sum_w) about the documented shift"""
    T = np.eye(4) if T is None else np.asarray(T, dtype=np.float64)
    corr = np.asarray(corr)
    tgt = np.asarray(target, dtype=np.float32).astype(np.float64)
    scov = np.asarray(source_cov, dtype=np.float32).astype(np.float64)
    tcov = np.asarray(target_cov, dtype=np.float32).astype(np.float64)
    q = RR.apply_transform(T, source).astype(np.float64)
    has = (corr >= 0) & (corr < tgt.shape[0])
    safe = np.where(has, corr, 0)
    p = tgt[safe]
    pair = has & np.isfinite(q).all(axis=1) & np.isfinite(p).all(axis=1)
    c = p[np.flatnonzero(pair)[0]] if pair.any() else np.zeros(3)
    finite = pair & np.isfinite(scov).all(axis=1) & np.isfinite(tcov[safe]).all(axis=1)
    R = T[:3, :3]
    with np.errstate(invalid="ignore", over="ignore"):
        M = full(np.where(finite[:, None], tcov[safe], 0.0)) + R[None] @ full(np.where(finite[:, None], scov, 0.0)) @ R.T[None]
        M = 0.5 * (M + M.transpose(0, 2, 1))
        W, det = adjugate_inverse(M)
        use = finite & np.isfinite(det) & (det > 0)
    q, p, M, W = q[use], p[use], M[use], W[use]
    d = q - p
    qs = q - c
    J = np.zeros((q.shape[0], 3, 6))
    J[:, 0, 1], J[:, 0, 2] = qs[:, 2], -qs[:, 1]
    J[:, 1, 0], J[:, 1, 2] = -qs[:, 2], qs[:, 0]
    J[:, 2, 0], J[:, 2, 1] = qs[:, 1], -qs[:, 0]
    J[:, :, 3:] = np.eye(3)[None]
    WJ = W @ J
    Wd = np.einsum("nab,nb->na", W, d)
    return dict(use=use, c=c, M=M, W=W, JTWJ=np.einsum("nra,nrb->ab", J, WJ), JTWd=np.einsum("nra,nr->a", J, Wd), n=int(use.sum()),
                sum_d2=float((d * d).sum()), sum_w=float((d * Wd).sum()))


def generalized_update(source, source_cov, target, target_cov, corr, T):
    """-> dict(T new, dT, n, fitness, rmse, sum_d2, sum_w, status, cond, cond_M): status 1 (T kept) with n < 6"""
    T = np.eye(4) if T is None else np.asarray(T, dtype=np.float64)
    s = generalized_system(source, source_cov, target, target_cov, corr, T)
    n = s["n"]
    out = dict(n=n, fitness=n / np.asarray(corr).shape[0], rmse=float(np.sqrt(s["sum_d2"] / n)) if n else 0.0,
               sum_d2=s["sum_d2"], sum_w=s["sum_w"], cond_M=float(np.linalg.cond(s["M"]).max()) if n else 0.0)
    if n < 6:
        return dict(out, T=T.copy(), dT=np.eye(4), status=1, cond=INF)
    x = np.linalg.solve(s["JTWJ"], -s["JTWd"])
    dT = np.eye(4)
    dT[:3, :3] = NR.rot_zyx(x[0], x[1], x[2])
    dT[:3, 3] = x[3:] + s["c"] - dT[:3, :3] @ s["c"]
    return dict(out, T=dT @ T, dT=dT, status=0, cond=float(np.linalg.cond(s["JTWJ"])))


def icp_generalized(source, source_cov, target, target_cov, max_distance, init=None, relative_fitness=1e-6, relative_rmse=1e-6,
                    max_iteration=30):
    """registration_reference.icp with the generalized update; every history entry also carries `cond` and `cond_M`"""
    T = np.eye(4) if init is None else np.asarray(init, dtype=np.float64).copy()
    history, converged = [], False
    for k in range(max_iteration):
        near = RR.nearest(RR.apply_transform(T, source), target, max_distance)
        corr = RR.correspondences(near)
        u = generalized_update(source, source_cov, target, target_cov, corr, T)
        history.append(dict(T=T, corr=corr, n=u["n"], fitness=u["fitness"], rmse=u["rmse"], cond=u["cond"], cond_M=u["cond_M"],
                            margins=RR.margins(near, max_distance)))
        T = u["T"]
        if k >= 1 and abs(history[k]["fitness"] - history[k - 1]["fitness"]) < relative_fitness and \
                abs(history[k]["rmse"] - history[k - 1]["rmse"]) < relative_rmse:
            converged = True
            break
    near = RR.nearest(RR.apply_transform(T, source), target, max_distance)
    corr = RR.correspondences(near)
    u = generalized_update(source, source_cov, target, target_cov, corr, T)
    return dict(T=T, iterations=len(history), converged=converged, fitness=u["fitness"], rmse=u["rmse"], corr=corr,
                history=history, final_margins=RR.margins(near, max_distance))


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
UPDATE_SIZES = [6, 256, 257, 65537]
UPDATE_OFFSETS = [0.0, 1000.0]
COVARIANCE_RADIUS = NR.E2E_NORMAL_RADIUS      # 2.5 spacings, about 20 grid rows: max_nn = 20 cuts some neighbourhoods and not others


def update_case(Ps, offset):
    """NR.update_case with covariances from the reference: the target's from its (perturbed) normals, the source's from the normals
    of the target rows it was drawn next to, turned by T0^-1 - flat on both sides, tilted against each other by the perturbation
    -> (source, source_cov float32, target, target_cov float32, corr, T0): the arguments of
    generalized_update"""
    src, tgt, nrm, T0, corr = NR.update_case(Ps, offset)
    near = RR.correspondences(RR.nearest(RR.apply_transform(T0, src), tgt))
    rng = np.random.default_rng(900 + Ps + int(offset))
    ns = nrm[near].astype(np.float64) + 0.02 * rng.standard_normal((Ps, 3))
    ns /= np.linalg.norm(ns, axis=1, keepdims=True)
    ns = ns @ T0[:3, :3]                                         # R0^T n: the normal in the source's own frame
    return src, from_normals(ns).astype(np.float32), tgt, from_normals(nrm).astype(np.float32), corr, T0


def single_plane_case():
    """the scene of test_update_status_two_on_a_single_exact_plane (tests/test_icp_plane_gpu.py): one exact plane, the source 1/8
    above it; the target's covariances flat along z, the source's isotropic -> (source, source_cov, target, target_cov, corr, T0)"""
    rng = np.random.default_rng(3)
    tgt = np.concatenate([rng.integers(-128, 128, size=(500, 2)) / 64.0, np.full((500, 1), 0.25)], axis=1).astype(np.float32)
    nrm = np.tile(np.float32([0, 0, 1]), (500, 1))
    src = (tgt[rng.integers(0, 500, size=300)] + np.float32([0.0, 0.0, 0.125])).astype(np.float32)
    T0 = RR.rigid_about([0, 0, 0.25], [0, 0, 1], 0.0, [0.0, 0.0, 0.0])
    corr = RR.correspondences(RR.nearest(src, tgt))
    scov = np.tile(np.float32([1, 0, 0, 1, 0, 1]), (300, 1))
    return src, scov, tgt, from_normals(nrm).astype(np.float32), corr, T0


# The fixed point of generalized ICP is not the true motion exactly: across a plane every pair still pulls as a point-to-point
# pair does, with weight 1 / 2 against 1 / (2 epsilon) along the normal, and nearest-neighbour pairs of two samplings of a patch
# do not cancel (their RMS is a third of a spacing, 7e-3).  The float64 loop above settles 6.0e-6 from the truth at epsilon = 1e-3 and
# 6.2e-7 at 1e-4 (tests/test_gicp_reference_cpu.py): the end-to-end tests, which ask for 1e-6, run at 1e-4.
E2E_EPSILON = 1e-4


def e2e_case():
    """NR.e2e_planes with the reference's covariances of both clouds at E2E_EPSILON (float32, as the device returns them) ->
    (source, source_cov, target, target_cov, T_true, max_distance)"""
    src, tgt, T, md = NR.e2e_planes()
    scov = covariances(src, COVARIANCE_RADIUS, 20, E2E_EPSILON)["cov"].astype(np.float32)
    tcov = covariances(tgt, COVARIANCE_RADIUS, 20, E2E_EPSILON)["cov"].astype(np.float32)
    return src, scov, tgt, tcov, T, md


def map_gaussians(target):
    """the e2e target as a Gaussian map: per patch a rotation whose LAST column is the patch's normal (NR._basis) as a unit
    quaternion (w, x, y, z), scales (s, s, s / 50) -> (quaternions float32 [Pt,4], scales float32 [Pt,3], patch of every row).
    The patch of a row is the one plane it lies on (the patches are exact: float32 rounding only)"""
    tgt = np.asarray(target, dtype=np.float64)
    off = np.stack([np.abs((tgt - np.asarray(o)) @ NR._basis(n)[2]) for o, n in zip(NR.SCENE_ORIGINS, NR.SCENE_NORMALS)], axis=1)
    patch = off.argmin(axis=1)
    assert (np.sort(off, axis=1)[:, 0] < 1e-6).all() and (np.sort(off, axis=1)[:, 1] > 1e-5).all()
    quats = []
    for n in NR.SCENE_NORMALS:
        a, b, c = NR._basis(n)
        quats.append(_quaternion(np.stack([a, b, c], axis=1)))
    q = np.asarray(quats)[patch].astype(np.float32)
    s = np.tile(np.float32([NR.SPACING, NR.SPACING, NR.SPACING / 50]), (tgt.shape[0], 1))
    return q, s, patch


def _quaternion(R):
    """unit quaternion (w, x, y, z) of a proper rotation whose trace is > -1"""
    if np.linalg.det(R) < 0:
        raise ValueError("not a proper rotation")
    w = 0.5 * np.sqrt(max(1.0 + np.trace(R), 0.0))
    if w < 1e-3:
        raise ValueError("a half turn: pick another basis")
    return np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])


def gaussian_covariances(quaternions, scales):
    """R diag(s^2) R^T of every row, [P,6] float64 (what GaussianModel.get_covariance forms in float32)"""
    q = np.asarray(quaternions, dtype=np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], axis=1),
                  np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], axis=1),
                  np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1)], axis=1)
    L = R * np.asarray(scales, dtype=np.float64)[:, None, :]
    return six(L @ L.transpose(0, 2, 1))


def random_spd(P, seed):
    """P symmetric positive definite matrices of random orientation and of sizes over four decades, eigenvalues l2 (a, b, 1) with
    b - a >= 5e-3 -> float32 [P,6]"""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((P, 3, 3)))
    b = rng.uniform(0.05, 1.0, size=P)
    lam = (10.0 ** rng.uniform(-4, 0, size=P))[:, None] * np.stack([b * rng.uniform(0.0, 0.9, size=P), b, np.ones(P)], axis=1)
    return six(Q @ (lam[:, :, None] * Q.transpose(0, 2, 1))).astype(np.float32)
