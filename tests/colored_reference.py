"""CPU restatements for the coloured-ICP tests (float64 on the host; nothing of the product is imported).

intensity: I = ((r + g) + b) / 3 from the float32 colours, promoted.
gradient: the colour gradient of every row (include/gsr.h gsr_color_gradient).  Membership comes from normals_reference.analyse -
  a row whose point, colour or normal is not finite is given a NaN point first, so it is nobody's neighbour - through its
  `inc_max`: the members of row i are the other finite rows with d2 <= the largest included d2, d2 formed exactly as analyse
  forms it, so float32 ties are decided identically.  M = sum u u^T + (n_i - 1)^2 n n^T, v = sum u (I_j - I_i),
  numpy.linalg.solve; status by the LDL^T pivot rule (a pivot <= 1e-12 x its diagonal entry), with the smallest pivot ratio of every
  row so that a test can show its rows are far from that threshold; cond(M) for the error bound.
colored_system / colored_update: one joint update about the documented shift (the target point of the first row whose q and p are
  finite): both residuals, both Jacobians, J^T J and J^T r in float64, numpy.linalg.solve, dT = Tr(c) [Rz Ry Rx, t] Tr(-c).
icp_colored: the loop of registration_icp with the same stopping rule.
Scene builders: a smooth texture for the clouds of normals_reference, and the flat textured plane of the end-to-end tests."""
import functools

import numpy as np

import normals_reference as NR
import registration_reference as RR

INF = float("inf")
PIVOT_MIN = 1e-12
LAMBDA = 0.968


def intensity(colors):
    c = np.asarray(colors, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return ((c[:, 0] + c[:, 1]) + c[:, 2]) / 3.0


def masked_points(points, colors, normals):
    """-> (float32 [P,3] with NaN rows where point, colour or normal is not finite, ok bool [P])"""
    p = np.asarray(points, dtype=np.float32).copy()
    ok = np.isfinite(p).all(axis=1) & np.isfinite(np.asarray(colors, dtype=np.float32)).all(axis=1) & \
        np.isfinite(np.asarray(normals, dtype=np.float32)).all(axis=1)
    p[~ok] = np.nan
    return p, ok


def _ldl_pivot_ratio(M):
    """smallest pivot / its diagonal entry over the three pivots of LDL^T of every M [R,3,3] (nan where a diagonal entry is 0 or a
    pivot is not finite: the rule rejects those)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        d0 = M[:, 0, 0]
        l10, l20 = M[:, 0, 1] / d0, M[:, 0, 2] / d0
        d1 = M[:, 1, 1] - l10 * l10 * d0
        l21 = (M[:, 1, 2] - l20 * l10 * d0) / d1
        d2 = (M[:, 2, 2] - l20 * l20 * d0) - l21 * l21 * d1
        ratios = np.stack([d0 / M[:, 0, 0], d1 / M[:, 1, 1], d2 / M[:, 2, 2]], axis=1)
    ratios[~np.isfinite(np.stack([d0, d1, d2], axis=1))] = np.nan
    return np.where(np.isnan(ratios).any(axis=1), np.nan, np.nanmin(np.nan_to_num(ratios, nan=INF), axis=1))


def gradient(points, colors, normals, radius, max_nn, chunk=256):
    """-> dict(gradient float64 [P,3], count int64 [P], status int64 [P], cond float64 [P] (inf where not solved), pivot float64 [P]
    (the smallest pivot ratio; nan where rejected outright or not formed), analysis: the dict of NR.analyse)"""
    pm, ok = masked_points(points, colors, normals)
    a = NR.analyse(pm, [(radius, max_nn)])[0]
    P = pm.shape[0]
    ps = np.where(ok[:, None], pm, np.float32(0))
    n64 = np.asarray(normals, dtype=np.float32).astype(np.float64)
    I = intensity(colors)
    g = np.zeros((P, 3))
    cond = np.full(P, INF)
    pivot = np.full(P, np.nan)
    status = np.zeros(P, np.int64)
    count = a["count"].copy()
    for i in range(0, P, chunk):
        c = min(chunk, P - i)
        delta = (ps[None, :, :] - ps[i:i + c, None, :]).astype(np.float64)          # float32 differences, promoted
        d2 = (delta[..., 0] * delta[..., 0] + delta[..., 1] * delta[..., 1]) + delta[..., 2] * delta[..., 2]
        other = np.repeat(ok[None, :], c, axis=0)
        other[np.arange(c), np.arange(c) + i] = False
        member = other & (d2 <= a["inc_max"][i:i + c, None])
        assert np.array_equal(1 + member.sum(axis=1), np.where(ok[i:i + c], count[i:i + c], 1 + member.sum(axis=1)))
        nn = np.where(ok[i:i + c, None], n64[i:i + c], 0.0)                          # (a masked row's sums are never used)
        along = (delta * nn[:, None, :]).sum(axis=2)
        u = (delta - along[..., None] * nn[:, None, :]) * member[..., None]
        b = np.where(member, np.nan_to_num(I)[None, :] - np.nan_to_num(I[i:i + c])[:, None], 0.0)
        w = (member.sum(axis=1)).astype(np.float64)                                 # n_i - 1
        M = np.einsum("cpk,cpl->ckl", u, u) + (w * w)[:, None, None] * nn[:, :, None] * nn[:, None, :]
        v = np.einsum("cpk,cp->ck", u, b)
        full = ok[i:i + c] & (count[i:i + c] >= 4)
        ratio = _ldl_pivot_ratio(M)
        with np.errstate(invalid="ignore"):
            solved = full & (ratio > PIVOT_MIN)
        pivot[i:i + c] = np.where(full, ratio, np.nan)
        rows = np.flatnonzero(solved)
        if rows.size:
            g[i + rows] = np.linalg.solve(M[rows], v[rows][..., None])[..., 0]
            cond[i + rows] = np.linalg.cond(M[rows])
        status[i:i + c] = np.where(~ok[i:i + c], 3, np.where(count[i:i + c] < 4, 1, np.where(solved, 0, 2)))
    g[~ok] = np.nan
    return dict(gradient=g, count=count, status=status, cond=cond, pivot=pivot, analysis=a)


# ---- the joint update -------------------------------------------------------------------------------------------------------------
def colored_system(source, source_colors, target, normals, target_colors, gradients, corr, T, lam=LAMBDA):
    """-> dict(use bool [Ps], c, q, p, n, d (the rows that take part), Is, It, rG, rI (unweighted), JG, JI (weighted), JTJ, JTr, n_rows,
    sum_d2, sum_rg2, sum_ri2)"""
    T = np.eye(4) if T is None else np.asarray(T, dtype=np.float64)
    corr = np.asarray(corr)
    tgt = np.asarray(target, dtype=np.float32).astype(np.float64)
    nrm = np.asarray(normals, dtype=np.float32).astype(np.float64)
    grd = np.asarray(gradients, dtype=np.float32).astype(np.float64)
    q = RR.apply_transform(T, source).astype(np.float64)
    has = (corr >= 0) & (corr < tgt.shape[0])
    safe = np.where(has, corr, 0)
    p, nv, dv = tgt[safe], nrm[safe], grd[safe]
    Is, It = intensity(source_colors), intensity(target_colors)[safe]
    pair = has & np.isfinite(q).all(axis=1) & np.isfinite(p).all(axis=1)
    use = pair & np.isfinite(nv).all(axis=1) & np.isfinite(dv).all(axis=1) & np.isfinite(Is) & np.isfinite(It)
    c = p[np.flatnonzero(pair)[0]] if pair.any() else np.zeros(3)
    q, p, nv, dv, Is, It = q[use], p[use], nv[use], dv[use], Is[use], It[use]
    sg, si = np.sqrt(lam), np.sqrt(1.0 - lam)
    e = q - p
    en = (e * nv).sum(axis=1)
    w = e - en[:, None] * nv                                      # q_proj - p
    rI = Is - (It + (dv * w).sum(axis=1))
    m = (dv * nv).sum(axis=1)[:, None] * nv - dv                  # -(I - n n^T) d
    JG = sg * np.concatenate([np.cross(q - c, nv), nv], axis=1)
    JI = si * np.concatenate([np.cross(q - c, m), m], axis=1)
    JTJ = JG.T @ JG + JI.T @ JI
    JTr = JG.T @ (sg * en) + JI.T @ (si * rI)
    return dict(use=use, c=c, q=q, p=p, n=nv, d=dv, Is=Is, It=It, rG=en, rI=rI, JG=JG, JI=JI, JTJ=JTJ, JTr=JTr, n_rows=int(use.sum()),
                sum_d2=float((e * e).sum()), sum_rg2=float((en * en).sum()) if lam > 0 else 0.0,
                sum_ri2=float((rI * rI).sum()) if lam < 1 else 0.0)


def delta_transform(x, c):
    dT = np.eye(4)
    dT[:3, :3] = NR.rot_zyx(x[0], x[1], x[2])
    dT[:3, 3] = np.asarray(x[3:]) + c - dT[:3, :3] @ c
    return dT


def residuals_at(s, x, lam=LAMBDA):
    """the weighted residuals (r_G, r_I) of the rows of a colored_system `s` after its q are moved by dT(x) about s["c"]"""
    dT = delta_transform(np.asarray(x, dtype=np.float64), s["c"])
    q = s["q"] @ dT[:3, :3].T + dT[:3, 3]
    e = q - s["p"]
    en = (e * s["n"]).sum(axis=1)
    w = e - en[:, None] * s["n"]
    rI = s["Is"] - (s["It"] + (s["d"] * w).sum(axis=1))
    return np.sqrt(lam) * en, np.sqrt(1.0 - lam) * rI


def colored_update(source, source_colors, target, normals, target_colors, gradients, corr, T, lam=LAMBDA):
    """-> dict(T new, dT, n, fitness, rmse, sum_d2, sum_rg2, sum_ri2, status, cond): status 1 (T kept) with n < 6, 2 (T kept) when
    LDL^T of J^T J rejects a pivot"""
    T = np.eye(4) if T is None else np.asarray(T, dtype=np.float64)
    s = colored_system(source, source_colors, target, normals, target_colors, gradients, corr, T, lam)
    n = s["n_rows"]
    out = dict(n=n, fitness=n / np.asarray(corr).shape[0], rmse=float(np.sqrt(s["sum_d2"] / n)) if n else 0.0,
               sum_d2=s["sum_d2"], sum_rg2=s["sum_rg2"], sum_ri2=s["sum_ri2"])
    if n < 6:
        return dict(out, T=T.copy(), dT=np.eye(4), status=1, cond=INF)
    A = s["JTJ"]
    L, D = np.eye(6), np.zeros(6)
    for j in range(6):
        d = A[j, j] - (L[j, :j] ** 2 * D[:j]).sum()
        if not np.isfinite(d) or not d > PIVOT_MIN * A[j, j]:
            return dict(out, T=T.copy(), dT=np.eye(4), status=2, cond=INF)
        D[j] = d
        for i in range(j + 1, 6):
            L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j] * D[:j]).sum()) / d
    x = np.linalg.solve(A, -s["JTr"])
    dT = delta_transform(x, s["c"])
    return dict(out, T=dT @ T, dT=dT, status=0, cond=float(np.linalg.cond(A)))


def icp_colored(source, source_colors, target, normals, target_colors, gradients, max_distance, lam=LAMBDA, init=None,
                relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=50):
    """registration_reference.icp with the coloured update"""
    T = np.eye(4) if init is None else np.asarray(init, dtype=np.float64).copy()
    history, converged = [], False

    def step(T):
        near = RR.nearest(RR.apply_transform(T, source), target, max_distance)
        corr = RR.correspondences(near)
        return corr, colored_update(source, source_colors, target, normals, target_colors, gradients, corr, T, lam)

    for k in range(max_iteration):
        corr, u = step(T)
        history.append(dict(T=T, corr=corr, n=u["n"], fitness=u["fitness"], rmse=u["rmse"], status=u["status"]))
        T = u["T"]
        if k >= 1 and abs(history[k]["fitness"] - history[k - 1]["fitness"]) < relative_fitness and \
                abs(history[k]["rmse"] - history[k - 1]["rmse"]) < relative_rmse:
            converged = True
            break
    corr, u = step(T)
    return dict(T=T, iterations=len(history), converged=converged, fitness=u["fitness"], rmse=u["rmse"], corr=corr, history=history)


# ---- textures and scenes -----------------------------------------------------------------------------------------------------------
def texture(points, wavelength=12 * NR.SPACING):
    """float32 [P,3] in [0.1, 0.9]: three smooth channels of different direction and phase about the cloud's finite mean; rows that
    are not finite get 0.5"""
    p = np.asarray(points, dtype=np.float64)
    ok = np.isfinite(p).all(axis=1)
    x = np.where(ok[:, None], p - p[ok].mean(axis=0), 0.0) * (2 * np.pi / wavelength)
    dirs = np.array([[0.8, 0.5, 0.33], [-0.4, 0.9, 0.2], [0.3, -0.3, 0.9]])
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    cols = [0.5 + 0.4 * np.sin(x @ dirs[k] + 0.7 * k) * np.cos(0.37 * (x @ dirs[(k + 1) % 3])) for k in range(3)]
    return np.stack(cols, axis=1).astype(np.float32)


# the gradient cases: P per family (257 .. 4097: one block and a row, several blocks, more than one super-box), and per case the
# (radius, max_nn) pairs - max_nn 4 and 5 (K = 4), 30 and 33 (K = 32); the radius binds at 30 / 33 on most rows and on the
# planted rows everywhere, and does not bind (inf) elsewhere
GRADIENT_SIZES = {"plane": 4097, "sphere": 1500, "clusters": 3000, "lattice": 1024, "duplicates": 257}
KAPPA_MAX = 1e8
LEFT_OUT_MAX = 0.02


def gradient_combos(kind):
    r = NR.LATTICE_RADIUS if kind == "lattice" else NR.RADIUS
    return [(INF, 4), (r, 5), (r, 30), (INF, 33)]


def gradient_cloud(kind):
    """-> (points float32 [P,3], colors float32 [P,3], normals float32 [P,3]): a cloud of normals_reference with a smooth texture
    and the reference's own normals of (inf, 30)"""
    pts = NR.cloud(kind, GRADIENT_SIZES[kind])
    wavelength = 2.0 if kind == "lattice" else 12 * NR.SPACING      # (the lattice's step is 1 / 8)
    nrm = NR.estimate(pts, INF, 30)[0].astype(np.float32)
    return pts, texture(pts, wavelength), nrm


PLANE_SIDE = 60
PLANE_Z = 0.25
PLANE_SEED = 11
PLANE_TURN = np.deg2rad(2.0)
PLANE_MAX_DISTANCE = 3 * NR.SPACING
PLANE_RADIUS = 2.5 * NR.SPACING


def plane_texture(points, h=NR.SPACING):
    """two smooth frequencies with wavelengths of about 12 spacings, different per channel"""
    p = np.asarray(points, dtype=np.float64)
    a = 2 * np.pi / (12 * h)
    b = 2 * np.pi / (11 * h)
    u, v = p[:, 0], p[:, 1]
    f1 = np.sin(a * u) * np.cos(a * 0.9 * v)
    f2 = np.sin(b * (0.6 * u + 0.8 * v) + 0.5)
    f3 = np.cos(b * (0.8 * u - 0.6 * v))
    return np.stack([0.5 + 0.25 * f1 + 0.15 * f2, 0.5 + 0.2 * f2 + 0.2 * f3, 0.5 + 0.25 * f3 - 0.15 * f1], axis=1).astype(np.float32)


def plane_scene(seed=PLANE_SEED, side=PLANE_SIDE):
    """target: side x side jittered samples of the plane z = 0.25 with the texture; source: OTHER samples of the inner part of the
    same surface, moved back by a motion IN the plane (1.5 spacings, a turn about the normal through the centre) -> (source,
    source_colors, target, target_colors, T_true, max_distance).  The plane's normals alone fix three of the six unknowns."""
    h = NR.SPACING
    rng = np.random.default_rng(seed)

    def samples(n, lo):
        gy, gx = np.mgrid[0:n, 0:n]
        uv = (np.stack([gx.ravel(), gy.ravel()], axis=1) + lo + rng.uniform(-0.3, 0.3, size=(n * n, 2))) * h
        return np.concatenate([uv, np.full((n * n, 1), PLANE_Z)], axis=1)

    tgt = samples(side, 0.0)
    inner = samples(side - 12, 6.4)                                  # six spacings off every rim, on a lattice half a step aside
    tcol, scol = plane_texture(tgt), plane_texture(inner)
    centre = np.array([0.5 * side * h, 0.5 * side * h, PLANE_Z])
    T = RR.rigid_about(centre, [0, 0, 1], PLANE_TURN, np.array([1.2, -0.9, 0.0]) * h)
    inv = np.linalg.inv(T)
    src = (inner @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    ps, pt = rng.permutation(src.shape[0]), rng.permutation(tgt.shape[0])
    return src[ps], scol[ps], tgt.astype(np.float32)[pt], tcol[pt], T, PLANE_MAX_DISTANCE


MULTISCALE_VOXELS = (2 * NR.SPACING, NR.SPACING)
MULTISCALE_ITERATIONS = (30, 20)


@functools.lru_cache(maxsize=None)
def update_case(Ps, offset):
    """NR.update_case with colours: the target's texture, a gradient per target row from the reference, source colours = the
    texture at the source's true place plus noise -> (src, scol, tgt, nrm, tcol, grd, T0, corr)"""
    src, tgt, nrm, T0, corr = NR.update_case(Ps, offset)
    rng = np.random.default_rng(900 + Ps + int(offset))
    tcol = texture(tgt)
    grd = gradient(tgt, tcol, nrm, 2.5 * NR.SPACING, 30)["gradient"].astype(np.float32)
    near = RR.correspondences(RR.nearest(RR.apply_transform(T0, src), tgt))
    scol = (tcol[np.maximum(near, 0)] + 0.02 * rng.standard_normal((Ps, 3))).astype(np.float32)
    return src, scol, tgt, nrm, tcol, grd, T0, corr
