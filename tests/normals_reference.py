"""CPU restatements for the normal-estimation and point-to-plane tests (float64 on the host; nothing of the product is imported).

neighbourhoods / normals: brute force.  delta_ij = p_j - p_i per component in float32 (exact when promoted), d2 = |delta|^2 in
  float64; k = max_nn - 1, d_k the k-th smallest d2 to the other finite rows (+inf with fewer), bound = min(r2, d_k) with r2 the
  float32 square of the float32 radius; members = the point itself and every other finite row with d2 <= bound (ties at the bound
  all belong).  C = S2 / n - (S1 / n)(S1 / n)^T from the members' delta, numpy.linalg.eigh, the eigenvector of the smallest
  eigenvalue.  Besides the answer, the quantities the preconditions are stated on: per row the largest included and the smallest
  excluded d2, and (lambda1 - lambda0) / lambda2.
orient: the two sign rules.
plane_update: one point-to-plane update about the shift the product documents (the target point of the first row whose q and p
  are finite), J^T J and J^T r in float64, numpy.linalg.solve, dT = Tr(c) [Rz Ry Rx, t] Tr(-c).
icp_plane: the loop of registration_icp with the same stopping rule."""
import numpy as np
import torch

import registration_reference as RR

INF = float("inf")


def radius2(radius):
    r = np.float32(radius)
    with np.errstate(over="ignore"):
        return float(np.float32(r * r))


def analyse(points, combos, chunk=512):
    """points float32 [P,3]; combos: list of (radius, max_nn) -> list of dict(count int64 [P], normal float64 [P,3] (sign as
    eigh left it; (0,0,1) where count < 3, NaN for a non-finite row), eig float64 [P,3] ascending, gap float64 [P] =
    (l1 - l0) / l2 (NaN where count < 3 or l2 == 0), inc_max, exc_min float64 [P] (largest included / smallest excluded d2 among
    the other rows; -inf / +inf without one), r2)."""
    p32 = torch.from_numpy(np.ascontiguousarray(np.asarray(points, dtype=np.float32)))
    P = p32.shape[0]
    ok = torch.isfinite(p32).all(dim=1)
    ps = torch.where(ok[:, None], p32, torch.zeros_like(p32))
    kmax = max(nn for _, nn in combos) - 1
    out = [dict(count=np.zeros(P, np.int64), S1=np.zeros((P, 3)), S2=np.zeros((P, 3, 3)), inc_max=np.full(P, -INF),
                exc_min=np.full(P, INF), r2=radius2(r)) for r, _ in combos]
    for i in range(0, P, chunk):
        delta = (ps[None, :, :] - ps[i:i + chunk, None, :]).double()          # float32 differences, promoted
        d2 = (delta[..., 0] * delta[..., 0] + delta[..., 1] * delta[..., 1]) + delta[..., 2] * delta[..., 2]
        c = d2.shape[0]
        other = ok[None, :].repeat(c, 1)
        other[torch.arange(c), torch.arange(c) + i] = False
        d2o = torch.where(other, d2, torch.full_like(d2, INF))
        kk = min(kmax, P)
        small = torch.topk(d2o, kk, dim=1, largest=False, sorted=True).values if kk else d2o[:, :0]
        small = torch.cat([small, torch.full((c, kmax - kk + 1), INF, dtype=torch.float64)], dim=1)
        for o, (_, nn) in zip(out, combos):
            bound = torch.clamp(small[:, nn - 2], max=o["r2"])
            member = other & (d2 <= bound[:, None])
            m = member.double()
            o["count"][i:i + c] = 1 + member.sum(dim=1).numpy()
            o["S1"][i:i + c] = torch.einsum("cp,cpk->ck", m, delta).numpy()
            o["S2"][i:i + c] = torch.einsum("cp,cpk,cpl->ckl", m, delta, delta).numpy()
            o["inc_max"][i:i + c] = torch.where(member, d2, torch.full_like(d2, -INF)).max(dim=1).values.numpy()
            o["exc_min"][i:i + c] = torch.where(other & ~member, d2, torch.full_like(d2, INF)).min(dim=1).values.numpy()
    okn = ok.numpy()
    res = []
    for o in out:
        n = o["count"].astype(np.float64)
        mean = o["S1"] / n[:, None]
        C = o["S2"] / n[:, None, None] - mean[:, :, None] * mean[:, None, :]
        w, v = np.linalg.eigh(C)
        normal = v[:, :, 0].copy()
        few = o["count"] < 3
        normal[few] = [0.0, 0.0, 1.0]
        w[few] = 0.0
        with np.errstate(invalid="ignore", divide="ignore"):
            gap = np.where(few | (w[:, 2] <= 0), np.nan, (w[:, 1] - w[:, 0]) / w[:, 2])
        count = o["count"].copy()
        count[~okn] = 0
        normal[~okn] = np.nan
        w[~okn] = np.nan
        gap[~okn] = np.nan
        res.append(dict(count=count, normal=normal, eig=w, gap=gap, inc_max=o["inc_max"], exc_min=o["exc_min"], r2=o["r2"],
                        finite=okn))
    return res


def set_margin(a):
    """smallest relative distance, over the finite rows, between what decides membership: the largest included d2 against the
    smallest excluded one and against r2, and the smallest excluded one against r2 (a row without an included or an excluded
    row has nothing to confuse there)"""
    inc, exc, r2, okn = a["inc_max"], a["exc_min"], a["r2"], a["finite"]
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.where(np.isfinite(inc) & np.isfinite(exc), (exc - inc) / exc, INF)
        if np.isfinite(r2):
            # a tie AT the bound is a member whatever the arithmetic only if it is exact; r2 must stay clear of both sides
            m = np.minimum(m, np.where(np.isfinite(inc), np.abs(r2 - inc) / r2, INF))
            m = np.minimum(m, np.where(np.isfinite(exc), np.abs(exc - r2) / r2, INF))
    return float(m[okn].min()) if okn.any() else INF


def orient(normals, points, viewpoint=None):
    """-> (oriented float64 [P,3], decider float64 [P]): towards the viewpoint (decider = n.(v - p)), or the component of largest
    magnitude, the first on ties, positive (decider: see below).  Rows with count < 3 are the caller's to restore."""
    n = np.asarray(normals, dtype=np.float64)
    if viewpoint is not None:
        d = (n * (np.asarray(viewpoint, dtype=np.float32).astype(np.float64)[None, :] -
                  np.asarray(points, dtype=np.float32).astype(np.float64))).sum(axis=1)
    else:
        # two quantities decide here: the leading component's distance from zero, and - where a second component of the
        # OPPOSITE sign comes within reach of it - by how much the leading one leads (quantised clouds give normals such as
        # (1, -1, 0) / sqrt 2, whose leader only rounding picks); the decider is the smaller of the two
        m = np.abs(np.nan_to_num(n))
        lead = np.argmax(m, axis=1)
        rows = np.arange(n.shape[0])
        d = n[rows, lead]
        rival = np.where(np.sign(np.nan_to_num(n)) == -np.sign(d)[:, None], m, 0.0).max(axis=1)
        d = np.sign(d) * np.minimum(np.abs(d), np.abs(d) - rival)
    with np.errstate(invalid="ignore"):
        return np.where((d < 0)[:, None], -n, n), d


def estimate(points, radius, max_nn, viewpoint=None):
    """what the product returns, in float64: (normals, count, eigenvalues)"""
    a = analyse(points, [(radius, max_nn)])[0]
    n, _ = orient(a["normal"], points, viewpoint)
    n[a["finite"] & (a["count"] < 3)] = [0.0, 0.0, 1.0]
    return n, a["count"], a["eig"]


# ---- point-to-plane ---------------------------------------------------------------------------------------------------------------
def rot_zyx(alpha, beta, gamma):
    ca, sa, cb, sb, cg, sg = np.cos(alpha), np.sin(alpha), np.cos(beta), np.sin(beta), np.cos(gamma), np.sin(gamma)
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    Rz = np.array([[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def plane_system(source, target, normals, corr, T):
    """-> dict(use bool [Ps], c, JTJ, JTr, n, sum_d2, sum_r2) about the documented shift; None for c without a valid pair"""
    T = np.eye(4) if T is None else np.asarray(T, dtype=np.float64)
    corr = np.asarray(corr)
    tgt = np.asarray(target, dtype=np.float32).astype(np.float64)
    nrm = np.asarray(normals, dtype=np.float32).astype(np.float64)
    q = RR.apply_transform(T, source).astype(np.float64)
    has = (corr >= 0) & (corr < tgt.shape[0])
    safe = np.where(has, corr, 0)
    p, nv = tgt[safe], nrm[safe]
    pair = has & np.isfinite(q).all(axis=1) & np.isfinite(p).all(axis=1)
    use = pair & np.isfinite(nv).all(axis=1)
    c = p[np.flatnonzero(pair)[0]] if pair.any() else np.zeros(3)
    q, p, nv = q[use], p[use], nv[use]
    e = q - p
    r = (e * nv).sum(axis=1)
    J = np.concatenate([np.cross(q - c, nv), nv], axis=1)
    return dict(use=use, c=c, JTJ=J.T @ J, JTr=J.T @ r, n=int(use.sum()), sum_d2=float((e * e).sum()), sum_r2=float((r * r).sum()))


def plane_update(source, target, normals, corr, T):
    """-> dict(T new, dT, n, fitness, rmse, sum_d2, sum_r2, status, cond): status 1 (T kept) with n < 6"""
    T = np.eye(4) if T is None else np.asarray(T, dtype=np.float64)
    s = plane_system(source, target, normals, corr, T)
    n = s["n"]
    out = dict(n=n, fitness=n / np.asarray(corr).shape[0], rmse=float(np.sqrt(s["sum_d2"] / n)) if n else 0.0,
               sum_d2=s["sum_d2"], sum_r2=s["sum_r2"])
    if n < 6:
        return dict(out, T=T.copy(), dT=np.eye(4), status=1, cond=INF)
    x = np.linalg.solve(s["JTJ"], -s["JTr"])
    dT = np.eye(4)
    dT[:3, :3] = rot_zyx(x[0], x[1], x[2])
    dT[:3, 3] = x[3:] + s["c"] - dT[:3, :3] @ s["c"]
    return dict(out, T=dT @ T, dT=dT, status=0, cond=float(np.linalg.cond(s["JTJ"])))


def icp_plane(source, target, normals, max_distance, init=None, relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30):
    """registration_reference.icp with the point-to-plane update; every history entry also carries `cond`"""
    T = np.eye(4) if init is None else np.asarray(init, dtype=np.float64).copy()
    history, converged = [], False
    for k in range(max_iteration):
        near = RR.nearest(RR.apply_transform(T, source), target, max_distance)
        corr = RR.correspondences(near)
        u = plane_update(source, target, normals, corr, T)
        history.append(dict(T=T, corr=corr, n=u["n"], fitness=u["fitness"], rmse=u["rmse"], cond=u["cond"],
                            margins=RR.margins(near, max_distance)))
        T = u["T"]
        if k >= 1 and abs(history[k]["fitness"] - history[k - 1]["fitness"]) < relative_fitness and \
                abs(history[k]["rmse"] - history[k - 1]["rmse"]) < relative_rmse:
            converged = True
            break
    near = RR.nearest(RR.apply_transform(T, source), target, max_distance)
    corr = RR.correspondences(near)
    u = plane_update(source, target, normals, corr, T)
    return dict(T=T, iterations=len(history), converged=converged, fitness=u["fitness"], rmse=u["rmse"], corr=corr,
                history=history, final_margins=RR.margins(near, max_distance))


def displacement(T_a, T_b, source):
    s = np.asarray(source, dtype=np.float64)
    a = s @ np.asarray(T_a)[:3, :3].T + np.asarray(T_a)[:3, 3]
    b = s @ np.asarray(T_b)[:3, :3].T + np.asarray(T_b)[:3, 3]
    return float(np.linalg.norm(a - b, axis=1).max())


# ---- clouds -------------------------------------------------------------------------------------------------------------------------
# Bodies are JITTERED GRIDS on surfaces, not uniform samples: the number of rows inside a radius then varies within a band, and the
# neighbourhoods of the test radius hold enough rows to be well shaped.  The rows whose neighbourhood the radius cuts below three,
# or to exactly three, are PLANTED five spacings off the body: singles (count 1), pairs (count 2) and near-equilateral triangles
# (count 3, l1 / l2 near 1) - a random cloud's three-row neighbourhoods are triangles of any thinness, and no seed avoids the
# thin ones at 5000 rows.  Coordinates are multiples of QUANTUM = 2^-10 (a twentieth of the spacing): every difference and every
# squared distance a neighbourhood can reach (< 0.2) is then exact in float32 as in float64, equal distances are exact ties, and
# unequal ones differ by at least 2^-20 - more than 1e-5 relative of any of them.  That is what makes the membership
# precondition hold on EVERY row rather than on lucky seeds.
SIZES = [1, 2, 3, 63, 64, 65, 4096, 4097, 5000]
SPACING = 0.02
QUANTUM = 2.0 ** -10


def _basis(normal):
    n = np.asarray(normal, dtype=np.float64)
    n = n / np.linalg.norm(n)
    a = np.cross(n, [1.0, 0.0, 0.0] if abs(n[0]) < 0.9 else [0.0, 1.0, 0.0])
    a /= np.linalg.norm(a)
    return a, np.cross(n, a), n


def _patch(rng, m, origin, normal, noise, h=SPACING):
    """m rows of a jittered square grid of spacing h in the plane through `origin`, plus `noise` along the normal"""
    side = int(np.ceil(np.sqrt(max(m, 1))))
    gy, gx = np.mgrid[0:side, 0:side]
    uv = (np.stack([gx.ravel(), gy.ravel()], axis=1)[:m] + rng.uniform(-0.3, 0.3, size=(m, 2))) * h
    a, b, n = _basis(normal)
    return np.asarray(origin)[None, :] + uv[:, :1] * a + uv[:, 1:] * b + noise * rng.standard_normal((m, 1)) * n


def _planted(rng, P, frames, h=SPACING):
    """min(P // 32, 24) rows in groups - triangle, pair, single in turn - one per frame (centre, a, b: a tangent basis); the
    frames lie five spacings off the body and six apart"""
    want = min(P // 32, 24)
    groups, rows, g = [], 0, 0
    while rows < want:
        kind = (3, 2, 1)[g % 3]
        centre, a, b = frames(g)
        ang = rng.uniform(0, 2 * np.pi) + 2 * np.pi * np.arange(kind) / 3
        groups.append(centre[None, :] + 0.6 * h * (np.cos(ang)[:, None] * a + np.sin(ang)[:, None] * b) +
                      rng.uniform(-0.03, 0.03, size=(kind, 3)) * h)
        rows += kind
        g += 1
    return np.concatenate(groups)[:want] if groups else np.zeros((0, 3))


def _finish(rng, body, P, frames):
    extra = _planted(rng, P, frames)
    pts = np.concatenate([body[:P - extra.shape[0]], extra])
    assert pts.shape[0] == P
    return (np.round(pts / QUANTUM) * QUANTUM).astype(np.float32)[rng.permutation(P)]


def _edge_frames(origin, normal, h=SPACING):
    a, b, _ = _basis(normal)
    return lambda g: (np.asarray(origin, dtype=np.float64) - 5 * h * a + (1 + 6 * g) * h * b, a, b)


def plane_cloud(P, seed, twice=0):
    """`twice`: that many body rows are stored a second time (the duplicates cloud)"""
    rng = np.random.default_rng(seed)
    origin, normal = [0.3, -0.2, 0.1], [0.3, -0.5, 0.8]
    body = _patch(rng, P, origin, normal, 0.05 * SPACING)
    if twice:
        nb = P - min(P // 32, 24)
        src = rng.choice(nb, size=2 * twice, replace=False)
        body[src[:twice]] = body[src[twice:]]
    return _finish(rng, body, P, _edge_frames(origin, normal))


def sphere_radius(P):
    """the radius at which P rows cover the WHOLE shell at the grid's density (at least 3 spacings)"""
    return max(SPACING * np.sqrt(P / (4 * np.pi)), 3 * SPACING)


def _fibonacci(i, n):
    z = 1 - 2 * (i + 0.5) / n
    phi = (i + 0.5) * np.pi * (3 - np.sqrt(5))
    return np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], axis=-1)


def sphere_cloud(P, seed):
    """a whole shell about (0.5, 0.5, 0.5): a jittered Fibonacci lattice of the body's rows at the grid's density, noise along the
    radius; the planted groups float five spacings above it, in the directions of a 12-point lattice of their own"""
    rng = np.random.default_rng(seed)
    nb = P - min(P // 32, 24)
    R = sphere_radius(nb)
    d = _fibonacci(np.arange(nb, dtype=np.float64), nb)
    d += rng.uniform(-0.2, 0.2, size=d.shape) * SPACING / R
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    centre = np.array([0.5, 0.5, 0.5])
    body = centre + d * (R + 0.05 * SPACING * rng.standard_normal((nb, 1)))

    def frames(g):
        dg = _fibonacci(np.float64(g), 12)
        a, b, _ = _basis(dg)
        return centre + dg * (R + 5 * SPACING), a, b

    return _finish(rng, body[rng.permutation(nb)], P, frames)


def cluster_cloud(P, seed, offset=1000.0):
    """up to twelve patches of random orientation around +1000 on every axis (float32 spacing there: 6e-5; the quantum: 1e-3)"""
    rng = np.random.default_rng(seed)
    k = min(12, max(1, P // 256))
    m = -(-P // k)
    origins = [offset + np.array([c % 4, (c // 4) % 3, 0.0]) * 120 * SPACING for c in range(k)]
    normals = [rng.standard_normal(3) for _ in range(k)]
    parts = [_patch(rng, m, o, n, 0.05 * SPACING) for o, n in zip(origins, normals)]
    body = np.stack(parts, axis=1).reshape(-1, 3)          # interleaved: a prefix holds rows of every patch
    return _finish(rng, body, P, _edge_frames(origins[0], normals[0]))


def lattice_cloud(P, seed):
    """rows (i / 8, j / 8, (i + j) / 16): a dyadic lattice in a tilted plane whose two steps have the SAME length - every
    coordinate, difference and squared distance is exact in float32, and every row's nearest rows are tied (four inside, three
    on an edge, two in a corner).  The rows the radius isolates form the same lattice four times coarser, eight rows below."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(P)))
    gy, gx = np.mgrid[0:side, 0:side]
    extra = P // 32
    q = side // 4 + 1
    m = np.arange(extra)
    i = np.concatenate([gx.ravel()[:P - extra], 4 * (m % q)]).astype(np.float64)
    j = np.concatenate([gy.ravel()[:P - extra], -8 - 4 * (m // q)]).astype(np.float64)
    pts = np.stack([i / 8, j / 8, (i + j) / 16], axis=1).astype(np.float32)
    return pts[rng.permutation(P)]


def duplicate_cloud(P, seed):
    """the plane cloud with a tenth of its body rows stored twice (distance 0: members) - twice, not more, so that a neighbourhood
    of max_nn >= 30 still spans the surface"""
    return plane_cloud(P, seed, twice=P // 10 if P >= 63 else 0)


CLOUDS = {"plane": plane_cloud, "sphere": sphere_cloud, "clusters": cluster_cloud, "lattice": lattice_cloud,
          "duplicates": duplicate_cloud}
SEEDS = {"plane": 1, "sphere": 2, "clusters": 3, "lattice": 4, "duplicates": 5}
# r2 = 3524.5 quanta^2 (2.9 spacings: about 26 grid rows inside - some neighbourhoods reach max_nn = 30, most do not; planted rows
# see 1 .. 3), half a step from the squared distances on either side
RADIUS = float(np.sqrt(3524.5) * QUANTUM)
LATTICE_RADIUS = 0.45            # r2 = 0.2025: the lattice's squared distances are multiples of 1 / 256 (51 / 256 = 0.1992, 52 / 256 = 0.2031)
# (radius, max_nn) per cloud: max_nn 3, 4 (K = 4), 30 and 33 (K = 32) at both radii on EVERY cloud.  Counts, eigenvalues, unit
# length, fallback and NaN rows are held on every row of every case.  The DIRECTION of a normal is compared where
# (l1 - l0) / l2 >= 1e-3 (GAP): that is every row with count >= 3 at max_nn 30 and 33 and on the lattice (shown in
# tests/test_normals_cpu.py), and all but the thin ones at max_nn 3 and 4 elsewhere - three or four rows of a jittered grid are a
# triangle of any thinness (two opposite grid neighbours are nearly collinear with the row), a row stored twice leaves two
# distinct positions, and no seed avoids either at 5000 rows; there the eigenvector of the smallest eigenvalue is not a stable
# function of the input, in any arithmetic.  The lattice also runs the sizes that change the kernel's list (9: K = 8, 10 and 17:
# K = 16, 18: K = 32).
GAP = 1e-3
WIDE = [(INF, 3), (INF, 4), (INF, 30), (INF, 33), (RADIUS, 3), (RADIUS, 4), (RADIUS, 30), (RADIUS, 33)]
LATTICE = [(INF, nn) for nn in (3, 4, 9, 10, 17, 18, 30, 33)] + [(LATTICE_RADIUS, nn) for nn in (3, 4, 30, 33)]


def combos(kind):
    return LATTICE if kind == "lattice" else WIDE


def cloud(kind, P):
    return CLOUDS[kind](P, SEEDS[kind] + 10 * P)


# ---- the three-plane scene --------------------------------------------------------------------------------------------------------------
SCENE_NORMALS = [[0.1, 0.15, 1.0], [1.0, 0.2, -0.1], [-0.15, 1.0, 0.2]]
SCENE_ORIGINS = [[0.0, 0.0, 0.0], [-0.3, 0.1, 0.3], [0.1, -0.3, 0.4]]


def three_planes(m, seed, noise, offset=0.0, h=SPACING):
    """three mutually tilted square patches of m rows each that do not touch -> (points float64 [3 m,3], their plane's unit
    normal [3 m,3])"""
    rng = np.random.default_rng(seed)
    pts, nrm = [], []
    for o, n in zip(SCENE_ORIGINS, SCENE_NORMALS):
        pts.append(_patch(rng, m, np.asarray(o) + offset, n, noise, h))
        nrm.append(np.repeat(_basis(n)[2][None, :], m, axis=0))
    return np.concatenate(pts), np.concatenate(nrm)


UPDATE_SEEDS = {6: 1}        # Ps -> seed offset, where the default's six rows leave J^T J worse than 1e6 (test_normals_cpu.py)


def update_case(Ps, offset):
    """target: 3 x 400 noisy rows with their planes' normals, slightly perturbed; source: Ps target rows moved back by a known
    motion, plus noise; correspondences of a nearby T0 within 3 spacings -> (source, target, normals, T0, corr)"""
    rng = np.random.default_rng(500 + Ps + int(offset) + UPDATE_SEEDS.get(Ps, 0))
    tgt, nrm = three_planes(400, 40 + int(offset), 0.1 * SPACING, offset)
    nrm = nrm + 0.02 * rng.standard_normal(nrm.shape)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    tgt, nrm = tgt.astype(np.float32), nrm.astype(np.float32)
    centre = tgt.astype(np.float64).mean(axis=0)
    truth = RR.rigid_about(centre, [0.3, 0.5, -0.8], 0.03, np.array([0.4, -0.3, 0.2]) * SPACING)
    p = tgt[rng.integers(0, tgt.shape[0], size=Ps)].astype(np.float64) + 0.2 * SPACING * rng.standard_normal((Ps, 3))
    inv = np.linalg.inv(truth)
    src = (p @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    T0 = RR.rigid_about(centre, [0.1, 0.2, 0.9], 0.01, np.array([0.1, 0.1, -0.1]) * SPACING)
    corr = RR.correspondences(RR.nearest(RR.apply_transform(T0, src), tgt, 3 * SPACING))
    if Ps == 6:                                                  # every row, or there is nothing to solve
        corr = RR.correspondences(RR.nearest(RR.apply_transform(T0, src), tgt))
    return src, tgt, nrm, T0, corr


E2E_SEED = 7
E2E_M = 1600
E2E_NORMAL_RADIUS = 2.5 * SPACING


def e2e_planes(seed=None):
    """target: three exact patches (no noise; float32 rounding only); source: OTHER samples of the same three patches, moved back
    by a motion that slides along them by several spacings -> (source, target, T_true, max_distance).  Point-to-point pairs
    hold the source where it is; the plane residual does not."""
    seed = E2E_SEED if seed is None else seed
    tgt, _ = three_planes(E2E_M, seed, 0.0)
    rng = np.random.default_rng(seed + 1000)
    src, _ = three_planes(E2E_M, seed + 1, 0.0)
    inner = []                                                   # keep the source off the patches' rims: the moved rows stay over the target
    for k in range(3):
        blk = src[k * E2E_M:(k + 1) * E2E_M]
        c = blk.mean(axis=0)
        inner.append(blk[np.abs(blk - c).max(axis=1) < 0.30 * np.sqrt(E2E_M) * SPACING])
    src = np.concatenate(inner)
    centre = tgt.mean(axis=0)
    T = RR.rigid_about(centre, [0.5, -0.3, 0.8], np.deg2rad(1.0), np.array([1.2, -0.9, 0.8]) * SPACING)
    inv = np.linalg.inv(T)
    src = (src @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    return src[rng.permutation(src.shape[0])], tgt.astype(np.float32)[rng.permutation(tgt.shape[0])], T, 4 * SPACING
