"""A float64 numpy restatement of the TSDF volume as include/gsr.h defines it (touch, integrate, surface points, marching
tetrahedra), written from that text and not from the kernels, with what a float32 evaluation may legitimately do differently:

* per voxel an error bound for tsdf and colour, propagated from the float32 unit roundoff EPS = 2^-24 over the operations the
  header lists (local offset add, projection, sdf, running average), and an `undecided` flag where a float32 evaluation may take
  the other branch (u + 0.5 or v + 0.5 within the projection's bound of an integer, sdf within its bound of -sdf_trunc, z within
  its bound of 0);
* for touch, a must-touch set (the box shrunk by the unprojection bound) and a may-touch set (the box grown by it).

Winding is decided here from geometry (the triangle's normal against the gradient of the tetrahedron's linear interpolant), not from
a combinatorial rule.  Scenes used by the tests are built at the bottom."""
import math

import numpy as np

EPS = 2.0 ** -24
BIAS = 1 << 20
NO_KEY = (1 << 63) - 1
KUHN = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))


def block_key(b):
    b = np.asarray(b, dtype=np.int64) + BIAS
    return (b[..., 0] << 42) | (b[..., 1] << 21) | b[..., 2]


def key_block(k):
    k = np.asarray(k, dtype=np.int64)
    m = (1 << 21) - 1
    return np.stack(((k >> 42) & m, (k >> 21) & m, k & m), axis=-1) - BIAS


def local_coords():
    lin = np.arange(512)
    return np.stack((lin & 7, (lin >> 3) & 7, lin >> 6), axis=1)          # [512,3]


def centre32(origin, vs, g):
    """float32 world position of voxel centres from global integer coordinates [...,3]: float64 product, float64 sum, one rounding"""
    return (np.asarray(origin, np.float64) + (np.asarray(g, np.float64) + 0.5) * np.float64(vs)).astype(np.float32)


class Frame:
    def __init__(self, depth, K, w2c, image=None, mask=None):
        self.depth = np.asarray(depth, np.float32)
        self.K = np.asarray(K, np.float32)                               # the kernels take K in float32
        self.w2c = np.asarray(w2c, np.float64)
        self.image = None if image is None else np.asarray(image, np.float32)
        self.mask = None if mask is None else np.asarray(mask, np.float32)


class RefVolume:
    def __init__(self, voxel_size, sdf_trunc, depth_trunc=10.0, origin=(0.0, 0.0, 0.0), max_weight=None):
        self.vs = float(voxel_size)
        self.trunc = float(np.float32(sdf_trunc))
        self.depth_trunc = float(np.float32(depth_trunc))
        self.origin = np.asarray(origin, np.float64)
        self.max_weight = float(np.float32(3.0e38 if max_weight is None else max_weight))
        self.keys = np.zeros(0, np.int64)                                # allocation order
        self.tsdf = np.zeros((0, 512))
        self.weight = np.zeros((0, 512))
        self.color = np.zeros((0, 512, 3))
        self.err = np.zeros((0, 512))                                    # bound of tsdf
        self.err_color = np.zeros((0, 512))
        self.undecided = np.zeros((0, 512), bool)

    # ---- touch -----------------------------------------------------------------------------------------------------------------------
    def _valid(self, fr):
        ok = (fr.depth > 0) & (fr.depth <= np.float32(self.depth_trunc))
        return ok if fr.mask is None else ok & (fr.mask != 0)

    def touch(self, fr):
        """-> (must, may, nominal): sorted unique keys.  Unprojection and the block index are float64 on both sides: the bound is
        64 units of 2^-53 on the magnitudes that enter (the point, the translation, the depth)."""
        H, W = fr.depth.shape
        v, u = np.nonzero(self._valid(fr))
        d = fr.depth[v, u].astype(np.float64)
        fx, fy, cx, cy = (float(k) for k in fr.K)
        R, t = fr.w2c[:3, :3], fr.w2c[:3, 3]
        q = np.stack(((u - cx) / fx * d, (v - cy) / fy * d, d), axis=1) - t
        p = q @ R                                                       # rows of R^T q
        eb = 64 * 2.0 ** -53 * (np.abs(p).max(axis=1, initial=0) + np.abs(t).max() + d + np.abs(self.origin).max())
        out = []
        for half in (self.trunc - eb, self.trunc + eb, np.full_like(eb, self.trunc)):
            lo = np.floor((p - half[:, None] - self.origin) / (8 * self.vs)).astype(np.int64)
            hi = np.floor((p + half[:, None] - self.origin) / (8 * self.vs)).astype(np.int64)
            keys = []
            for ox in range(3):
                for oy in range(3):
                    for oz in range(3):
                        b = lo + np.array([ox, oy, oz])
                        ok = np.all(b <= hi, axis=1) & np.all((b >= -BIAS) & (b < BIAS), axis=1)
                        keys.append(block_key(b[ok]))
            out.append(np.unique(np.concatenate(keys)) if keys else np.zeros(0, np.int64))
        return tuple(out)

    def _rows_of(self, keys):
        """rows of `keys`, allocating zeroed rows for the new ones (append-only, in ascending key order per frame)"""
        known = dict(zip(self.keys.tolist(), range(len(self.keys))))
        new = [k for k in keys.tolist() if k not in known]
        if new:
            n = len(new)
            self.keys = np.concatenate((self.keys, np.asarray(new, np.int64)))
            self.tsdf = np.concatenate((self.tsdf, np.zeros((n, 512))))
            self.weight = np.concatenate((self.weight, np.zeros((n, 512))))
            self.color = np.concatenate((self.color, np.zeros((n, 512, 3))))
            self.err = np.concatenate((self.err, np.zeros((n, 512))))
            self.err_color = np.concatenate((self.err_color, np.zeros((n, 512))))
            self.undecided = np.concatenate((self.undecided, np.zeros((n, 512), bool)))
            known = dict(zip(self.keys.tolist(), range(len(self.keys))))
        return np.asarray([known[k] for k in keys.tolist()], np.int64)

    # ---- integrate -------------------------------------------------------------------------------------------------------------------
    def integrate(self, fr, keys=None):
        """One frame into the blocks `keys` (default: the nominal touch set)."""
        if keys is None:
            keys = self.touch(fr)[2]
        keys = np.asarray(keys, np.int64)
        if keys.size == 0:
            return
        rows = self._rows_of(keys)
        H, W = fr.depth.shape
        fx, fy, cx, cy = (float(k) for k in fr.K)
        R, t = fr.w2c[:3, :3], fr.w2c[:3, 3]
        vs, trunc = self.vs, self.trunc
        b = key_block(keys)                                             # [n,3]
        g = 8 * b[:, None, :] + local_coords()[None]                    # [n,512,3]
        cam = (self.origin + (g + 0.5) * vs) @ R.T + t                  # exact positions
        corner = np.abs((self.origin + (8 * b + 0.5) * vs) @ R.T + t)   # [n,3]
        # local offset add: the corner's rounding, three rounded steps times <= 7 with their products' roundings, three sums
        e_pos = 1.01 * EPS * (4 * corner[:, None, :] + 110 * vs)        # [n,1,3] per component
        x, y, z = cam[..., 0], cam[..., 1], cam[..., 2]
        ex, ey, ez = e_pos[..., 0], e_pos[..., 1], e_pos[..., 2]
        und = np.abs(z) <= ez
        front = z > 0
        zs = np.where(front, z, 1.0)
        zl = np.maximum(zs - ez, 1e-300)
        qx, qy = x / zs, y / zs
        e_qx = (ex + np.abs(qx) * ez) / zl + EPS * np.abs(qx)
        e_qy = (ey + np.abs(qy) * ez) / zl + EPS * np.abs(qy)
        u, v = fx * qx + cx, fy * qy + cy
        e_u = fx * e_qx + EPS * (np.abs(fx * qx) + 2 * np.abs(u) + 1)
        e_v = fy * e_qy + EPS * (np.abs(fy * qy) + 2 * np.abs(v) + 1)
        pu, pv = np.floor(u + 0.5), np.floor(v + 0.5)
        near_u = np.abs(u + 0.5 - np.round(u + 0.5)) <= 1.01 * e_u
        near_v = np.abs(v + 0.5 - np.round(v + 0.5)) <= 1.01 * e_v
        roughly_in = (pu >= -1) & (pu <= W) & (pv >= -1) & (pv <= H)
        und |= front & roughly_in & (near_u | near_v)
        inside = front & (pu >= 0) & (pu < W) & (pv >= 0) & (pv < H)
        iu, iv = np.where(inside, pu, 0).astype(np.int64), np.where(inside, pv, 0).astype(np.int64)
        d = fr.depth[iv, iu].astype(np.float64)
        ok = inside & (d > 0) & (d <= self.depth_trunc)
        if fr.mask is not None:
            ok &= fr.mask[iv, iu] != 0
        s2 = 1 + qx * qx + qy * qy
        r = np.sqrt(s2)
        e_s2 = 2 * np.abs(qx) * e_qx + 2 * np.abs(qy) * e_qy + 4 * EPS * s2
        e_r = e_s2 / (2 * r) + EPS * r
        dz = d - z
        e_dz = ez + EPS * np.abs(dz)
        sdf = dz * r
        e_sdf = 1.01 * (np.abs(dz) * e_r + r * e_dz + EPS * np.abs(sdf))
        und |= ok & (np.abs(sdf + trunc) <= e_sdf)
        upd = ok & (sdf > -trunc)
        f = np.minimum(1.0, sdf / trunc)
        e_f = np.where(sdf / trunc - e_sdf / trunc >= 1.0, 0.0, e_sdf / trunc + EPS * np.abs(f))
        w = self.weight[rows]
        t_old, c_old = self.tsdf[rows], self.color[rows]
        t_new = (t_old * w + f) / (w + 1)
        e_new = (self.err[rows] * w + e_f) / (w + 1) + 3 * EPS * np.maximum(np.abs(t_new), (np.abs(t_old) * w + np.abs(f)) / (w + 1))
        self.tsdf[rows] = np.where(upd, t_new, t_old)
        self.err[rows] = np.where(upd, e_new, self.err[rows])
        if fr.image is not None:
            pix = fr.image[:, iv, iu].astype(np.float64).transpose(1, 2, 0)          # [n,512,3]
            c_new = (c_old * w[..., None] + pix) / (w[..., None] + 1)
            mag = np.maximum(np.abs(c_new), (np.abs(c_old) * w[..., None] + np.abs(pix)) / (w[..., None] + 1)).max(axis=-1)
            ec_new = self.err_color[rows] * w / (w + 1) + 3 * EPS * mag
            self.color[rows] = np.where(upd[..., None], c_new, c_old)
            self.err_color[rows] = np.where(upd, ec_new, self.err_color[rows])
        self.weight[rows] = np.where(upd, np.minimum(w + 1, self.max_weight), w)
        self.undecided[rows] |= und

    def sorted_view(self):
        order = np.argsort(self.keys, kind="stable")
        return self.keys[order], order


# ---- extraction on any volume given as arrays ----------------------------------------------------------------------------------------
class Dense:
    """The blocks `keys` [B] with rows tsdf / weight [B,512] (and optionally color [B,512,3], err [B,512]) as dense arrays over their
    bounding box plus a margin of 2 voxels: F is NaN where a voxel is unobserved (weight <= min_weight) or its block absent."""

    def __init__(self, keys, tsdf, weight, min_weight=0.0, color=None, err=None, flag=None):
        keys = np.asarray(keys, np.int64)
        self.keys = keys
        b = key_block(keys).reshape(-1, 3)
        self.b = b
        lo = b.min(axis=0) if len(b) else np.zeros(3, np.int64)
        hi = b.max(axis=0) if len(b) else np.zeros(3, np.int64)
        self.base = 8 * lo - 2                                           # global coordinate of index 0
        shape = tuple((8 * (hi - lo + 1) + 4).tolist())
        self.F = np.full(shape, np.nan)
        self.C = None if color is None else np.zeros(shape + (3,))
        self.E = None if err is None else np.zeros(shape)
        self.U = None if flag is None else np.zeros(shape, bool)
        self.owner = np.full(shape, -1, np.int64)                        # sorted position of the block of a voxel
        order = np.argsort(keys, kind="stable")
        for pos, i in enumerate(order.tolist()):
            o = 8 * b[i] - self.base
            sl = (slice(o[0], o[0] + 8), slice(o[1], o[1] + 8), slice(o[2], o[2] + 8))
            blk = lambda a: np.asarray(a[i], np.float64).reshape(8, 8, 8, *np.shape(a[i])[1:]).swapaxes(0, 2)   # [lz,ly,lx] -> [x,y,z]
            self.F[sl] = np.where(blk(weight) > min_weight, blk(tsdf), np.nan)
            self.owner[sl] = pos
            if color is not None:
                self.C[sl] = blk(color)
            if err is not None:
                self.E[sl] = blk(err)
            if flag is not None:
                self.U[sl] = np.asarray(flag[i]).reshape(8, 8, 8).swapaxes(0, 2)

    def order_key(self, idx):
        """(sorted block position, linear voxel index) of dense indices [N,3]"""
        g = idx + self.base
        l = g & 7
        return self.owner[idx[:, 0], idx[:, 1], idx[:, 2]], l[:, 0] + 8 * l[:, 1] + 64 * l[:, 2]


def _shift(a, axis, k):
    """a[i + k e_axis] as an array of a's shape (NaN / 0 beyond the end)"""
    out = np.full_like(a, np.nan if a.dtype.kind == "f" else 0)
    src = [slice(None)] * 3
    dst = [slice(None)] * 3
    if k > 0:
        src[axis], dst[axis] = slice(k, None), slice(None, -k)
    else:
        src[axis], dst[axis] = slice(None, k), slice(-k, None)
    out[tuple(dst)] = a[tuple(src)]
    return out


def gradient(F):
    """central differences in voxel units with the one-sided fall-backs -> [X,Y,Z,3] (0 where nothing is known)"""
    G = np.zeros(F.shape + (3,))
    for a in range(3):
        fp, fm = _shift(F, a, 1), _shift(F, a, -1)
        hp, hm = ~np.isnan(fp), ~np.isnan(fm)
        with np.errstate(invalid="ignore"):
            G[..., a] = np.where(hp & hm, 0.5 * (fp - fm), np.where(hp, fp - F, np.where(hm, F - fm, 0.0)))
    return np.nan_to_num(G)


def extract_points(D, vs, origin):
    """-> dict: edges [N,4] (global coordinate of i, axis), points, normals, colors [N,3] float64, t [N], in the specified order;
    with D.E also dt, the first-order bound of t from the tsdf bounds (times 1.1 for the second order)"""
    F = D.F
    G = gradient(F)
    rec = []
    for a in range(3):
        Fj = _shift(F, a, 1)
        with np.errstate(invalid="ignore"):
            hit = ~np.isnan(F) & ~np.isnan(Fj) & ((F < 0) != (Fj < 0))
        idx = np.argwhere(hit)
        rec.append(np.concatenate((idx, np.full((len(idx), 1), a)), axis=1))
    rec = np.concatenate(rec) if rec else np.zeros((0, 4), np.int64)
    idx, ax = rec[:, :3], rec[:, 3]
    blk, lin = D.order_key(idx)
    order = np.lexsort((ax, lin, blk))
    idx, ax = idx[order], ax[order]
    jdx = idx + np.eye(3, dtype=np.int64)[ax]
    at = lambda A, i: A[i[:, 0], i[:, 1], i[:, 2]]
    flo, fhi = at(F, idx), at(F, jdx)
    t = flo / (flo - fhi)
    plo = centre32(origin, vs, idx + D.base).astype(np.float64)
    phi = centre32(origin, vs, jdx + D.base).astype(np.float64)
    out = {"edges": np.concatenate((idx + D.base, ax[:, None]), axis=1), "t": t, "points": plo + t[:, None] * (phi - plo)}
    glo, ghi = at(G, idx), at(G, jdx)
    n = glo + t[:, None] * (ghi - glo)
    ln = np.linalg.norm(n, axis=1)
    out["normal_length"] = ln
    out["normals"] = np.where(ln[:, None] > 0, n / np.where(ln > 0, ln, 1.0)[:, None], 0.0)
    if D.C is not None:
        clo, chi = at(D.C, idx), at(D.C, jdx)
        out["colors"] = clo + t[:, None] * (chi - clo)
    if D.E is not None:
        elo, ehi = at(D.E, idx), at(D.E, jdx)
        out["dt"] = 1.1 * (np.abs(fhi) * elo + np.abs(flo) * ehi) / (flo - fhi) ** 2
    if D.U is not None:
        out["undecided"] = at(D.U, idx) | at(D.U, jdx)
    return out


def tet_edges(tm):
    """triangles of a tetrahedron whose path vertex k is inside where bit k of tm is set, each three (lo, hi) edges, in the
    header's default vertex order (the winding is decided by the caller from geometry)"""
    ins = [k for k in range(4) if tm >> k & 1]
    outs = [k for k in range(4) if not tm >> k & 1]
    e = lambda p, q: (min(p, q), max(p, q))
    if len(ins) in (1, 3):
        k = ins[0] if len(ins) == 1 else outs[0]
        o = [q for q in range(4) if q != k]
        return [[e(k, o[0]), e(k, o[1]), e(k, o[2])]]
    if len(ins) == 2:
        A, B, C, Dd = ins[0], ins[1], outs[0], outs[1]
        return [[e(A, C), e(A, Dd), e(B, Dd)], [e(A, C), e(B, Dd), e(B, C)]]
    return []


def extract_triangles(D, vs, origin):
    """-> dict: positions [T,3,3], colors [T,3,3] (when D.C), cubes [T,3] global coordinate, in the specified order"""
    F = D.F
    X, Y, Z = F.shape
    corners = np.stack([F[(c & 1):X - 1 + (c & 1), ((c >> 1) & 1):Y - 1 + ((c >> 1) & 1), (c >> 2):Z - 1 + (c >> 2)] for c in range(8)],
                       axis=-1)                                          # [X-1,Y-1,Z-1,8]
    used = ~np.isnan(corners).any(axis=-1)
    with np.errstate(invalid="ignore"):
        neg = corners < 0
    mixed = used & neg.any(axis=-1) & ~neg.all(axis=-1) & (D.owner[:-1, :-1, :-1] >= 0)
    idx = np.argwhere(mixed)                                             # cubes by their lowest corner
    fc = corners[idx[:, 0], idx[:, 1], idx[:, 2]]                        # [N,8]
    off = np.array([[c & 1, (c >> 1) & 1, c >> 2] for c in range(8)])
    pc = centre32(origin, vs, idx[:, None, :] + off[None] + D.base).astype(np.float64)        # [N,8,3]
    cc = None
    if D.C is not None:
        ci = idx[:, None, :] + off[None]
        cc = D.C[ci[..., 0], ci[..., 1], ci[..., 2]]                    # [N,8,3]
    blk, lin = D.order_key(idx)
    pos, col, keys = [], [], []
    for ti, (a, b, c) in enumerate(KUHN):
        path = [0, 1 << a, (1 << a) | (1 << b), 7]
        fv = fc[:, path]                                                 # [N,4]
        tm_all = ((fv < 0) * (1 << np.arange(4))).sum(axis=1)
        grad = np.zeros((len(idx), 3))
        grad[:, a], grad[:, b], grad[:, c] = fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 1], fv[:, 3] - fv[:, 2]
        for tm in range(1, 15):
            sel = np.nonzero(tm_all == tm)[0]
            if not len(sel):
                continue
            tris = tet_edges(tm)
            vert, vcol = [], []
            for tri in tris:
                pv, cv = [], []
                for lo, hi in tri:
                    flo, fhi = fv[sel, lo], fv[sel, hi]
                    tt = (flo / (flo - fhi))[:, None]
                    plo, phi = pc[sel, path[lo]], pc[sel, path[hi]]
                    pv.append(plo + tt * (phi - plo))
                    if cc is not None:
                        cv.append(cc[sel, path[lo]] + tt * (cc[sel, path[hi]] - cc[sel, path[lo]]))
                vert.append(np.stack(pv, axis=1))                        # [n,3,3]
                vcol.append(np.stack(cv, axis=1) if cc is not None else None)
            # winding: the right-hand normal of the first triangle against the gradient of the linear interpolant
            nrm = np.cross(vert[0][:, 1] - vert[0][:, 0], vert[0][:, 2] - vert[0][:, 0])
            flip = (nrm * grad[sel]).sum(axis=1) < 0
            for k, (vv, vc) in enumerate(zip(vert, vcol)):
                vv = np.where(flip[:, None, None], vv[:, [0, 2, 1]], vv)
                pos.append(vv)
                if vc is not None:
                    col.append(np.where(flip[:, None, None], vc[:, [0, 2, 1]], vc))
                keys.append(np.stack((blk[sel], lin[sel], np.full(len(sel), ti), np.full(len(sel), k)), axis=1))
    if not pos:
        return {"positions": np.zeros((0, 3, 3)), "colors": np.zeros((0, 3, 3)), "cubes": np.zeros((0, 3), np.int64)}
    pos, keys = np.concatenate(pos), np.concatenate(keys)
    order = np.lexsort((keys[:, 3], keys[:, 2], keys[:, 1], keys[:, 0]))
    out = {"positions": pos[order]}
    if col:
        out["colors"] = np.concatenate(col)[order]
    return out


def weld(positions):
    """float32 soup [T,3,3] -> (vertices [V,3] float32, triangles [T',3]): exact-bits unique, degenerate triangles dropped"""
    flat = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    bits = flat.view(np.int32)
    uniq, inv = np.unique(bits, axis=0, return_inverse=True)
    tri = inv.reshape(-1, 3)
    keep = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])
    return uniq.view(np.float32), tri[keep]


def mesh_stats(vertices, triangles):
    """-> dict: closed (every edge in exactly two triangles, once in each direction), euler, volume (signed), boundary_edges"""
    v, t = np.asarray(vertices, np.float64), np.asarray(triangles, np.int64)
    e = np.concatenate((t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]))
    und = np.sort(e, axis=1)
    uniq, counts = np.unique(und, axis=0, return_counts=True)
    directed = np.unique(e, axis=0)
    closed = bool(len(t) > 0 and np.all(counts == 2) and len(directed) == len(e))
    used = np.unique(t)
    vol = float(np.einsum("ij,ij->i", v[t[:, 0]], np.cross(v[t[:, 1]], v[t[:, 2]])).sum() / 6.0)
    return {"closed": closed, "euler": int(len(used) - len(uniq) + len(t)), "volume": vol,
            "boundary_edges": int((counts == 1).sum()), "non_manifold_edges": int((counts > 2).sum())}


# ---- scenes --------------------------------------------------------------------------------------------------------------------------
def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    eye = np.asarray(eye, np.float64)
    f = np.asarray(target, np.float64) - eye
    f /= np.linalg.norm(f)
    r = np.cross(f, np.asarray(up, np.float64))
    r /= np.linalg.norm(r)
    dn = np.cross(f, r)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = r, dn, f, eye
    return np.linalg.inv(c2w)


def intrinsics(W, H, fovx=0.9):
    fx = 0.5 * W / math.tan(0.5 * fovx)
    return np.array([fx, fx, 0.5 * (W - 1) + 0.25, 0.5 * (H - 1) - 0.25], np.float32)


def fibonacci_eyes(n, radius, seed=0):
    """the eye points of scene_utils.fibonacci_cameras"""
    phase = np.random.default_rng(seed).uniform(0.0, 2.0 * math.pi)
    golden = math.pi * (3.0 - math.sqrt(5.0))
    eyes = []
    for i in range(n):
        z = 1.0 - 2.0 * (i + 0.5) / n
        rho = math.sqrt(max(0.0, 1.0 - z * z))
        th = phase + golden * i
        eyes.append(radius * np.array([rho * math.cos(th), rho * math.sin(th), z]))
    return eyes


def pixel_rays(W, H, K, w2c):
    """camera centre and world-space ray directions with view-space z = 1 -> (o [3], dirs [H,W,3])"""
    fx, fy, cx, cy = (float(k) for k in K)
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    dc = np.stack(((u - cx) / fx, (v - cy) / fy, np.ones_like(u)), axis=-1)
    R, t = w2c[:3, :3], w2c[:3, 3]
    return -R.T @ t, dc @ R                                             # R^T d


def sphere_frames(W, H, n_views, centre, radius, cam_radius=1.3, seed=3, fovx=0.9):
    """analytic z-depth of a sphere from cameras on a Fibonacci sphere; colour = 0.5 + 0.5 outward normal"""
    K = intrinsics(W, H, fovx)
    centre = np.asarray(centre, np.float64)
    frames = []
    for eye in fibonacci_eyes(n_views, cam_radius, seed):
        w2c = look_at(eye + centre, centre)
        o, dirs = pixel_rays(W, H, K, w2c)
        oc = o - centre
        a = (dirs * dirs).sum(-1)
        bq = (dirs * oc).sum(-1)
        disc = bq * bq - a * (oc @ oc - radius * radius)
        lam = (-bq - np.sqrt(np.maximum(disc, 0.0))) / a
        hit = disc > 0
        depth = np.where(hit, lam, 0.0)
        nrm = (o + lam[..., None] * dirs - centre) / radius
        img = np.where(hit[..., None], 0.5 + 0.5 * nrm, 0.0).transpose(2, 0, 1)
        frames.append(Frame(depth, K, w2c, img))
    return frames


def plane_frames(W, H, poses, n, offset, fovx=0.9):
    """analytic z-depth of the plane n . x = offset from world-to-camera `poses`; colour varies smoothly with the hit point"""
    K = intrinsics(W, H, fovx)
    n = np.asarray(n, np.float64)
    frames = []
    for w2c in poses:
        o, dirs = pixel_rays(W, H, K, w2c)
        den = dirs @ n
        lam = (offset - o @ n) / np.where(np.abs(den) > 1e-9, den, 1.0)
        hit = (np.abs(den) > 1e-9) & (lam > 0)
        p = o + lam[..., None] * dirs
        img = np.where(hit[..., None], 0.5 + 0.4 * np.sin(3.0 * p + np.array([0.0, 1.0, 2.0])), 0.0).transpose(2, 0, 1)
        frames.append(Frame(np.where(hit, lam, 0.0), K, w2c, img))
    return frames


def shifted(frames, shift):
    """the same frames seen from a world frame moved by `shift`: x' = x + shift, so w2c' = w2c with t' = t - R shift"""
    out = []
    for f in frames:
        T = f.w2c.copy()
        T[:3, 3] = f.w2c[:3, 3] - f.w2c[:3, :3] @ np.asarray(shift, np.float64)
        out.append(Frame(f.depth, f.K, T, f.image, f.mask))
    return out


SPHERE = dict(centre=(0.013, -0.021, 0.017), radius=0.3, voxel_size=0.03, sdf_trunc=0.09)
FAR_SHIFT = (10000.0, -10000.0, 3000.0)


def scenes():
    """name -> (volume arguments, frames): every scene the GPU tests integrate"""
    s = {}
    s["sphere"] = (dict(voxel_size=SPHERE["voxel_size"], sdf_trunc=SPHERE["sdf_trunc"]),
                   sphere_frames(64, 48, 12, SPHERE["centre"], SPHERE["radius"]))
    # a tilted plane through the origin seen from both sides of every axis: negative block coordinates on every axis; 77 x 53
    poses = [look_at(e, (0.02, -0.03, 0.01)) for e in ((0.9, 0.5, 1.1), (-0.7, 0.8, 1.0), (0.3, -0.9, 1.2), (-0.5, -0.6, 1.3),
                                                        (0.1, 0.2, 1.4), (0.8, -0.2, 1.0), (-0.9, 0.1, 1.2), (0.4, 0.9, 1.1))]
    s["plane"] = (dict(voxel_size=0.04, sdf_trunc=0.1, depth_trunc=1.8), plane_frames(77, 53, poses, (0.1, -0.15, 1.0), 0.02))
    # a wall 0.16 in front of an identity camera: touched blocks reach behind the camera and beyond the image
    s["near"] = (dict(voxel_size=0.05, sdf_trunc=0.1, origin=(0.0, 0.0, -0.2)), plane_frames(64, 48, [np.eye(4)] * 2, (0.0, 0.0, 1.0), 0.16))
    half = plane_frames(64, 48, poses[:2], (0.1, -0.15, 1.0), 0.02)
    for f in half:
        f.mask = np.zeros((48, 64), np.float32)
        f.mask[:, :32] = 1.0
    s["half_mask"] = (dict(voxel_size=0.04, sdf_trunc=0.1), half)
    s["capped"] = (dict(voxel_size=0.04, sdf_trunc=0.1, max_weight=3.0), plane_frames(64, 48, poses[:6], (0.1, -0.15, 1.0), 0.02))
    # one reading in the middle of a block
    one = plane_frames(64, 48, [np.eye(4)], (0.0, 0.0, 1.0), 0.7)[0]
    keep = np.zeros((48, 64), np.float32)
    keep[20, 30] = 1.0
    one.mask = keep
    fx, fy, cx, cy = (float(k) for k in one.K)
    p = np.array([(30 - cx) / fx * 0.7, (20 - cy) / fy * 0.7, 0.7])
    s["one_block"] = (dict(voxel_size=0.05, sdf_trunc=0.05, origin=tuple((p - 0.2).tolist())), [one])
    return s


def run_scene(args, frames, shift=None):
    """the reference volume after every frame (nominal touch sets)"""
    args = dict(args)
    if shift is not None:
        args["origin"] = tuple((np.asarray(args.get("origin", (0.0, 0.0, 0.0))) + np.asarray(shift)).tolist())
        frames = shifted(frames, shift)
    vol = RefVolume(**args)
    for f in frames:
        vol.integrate(f)
    return vol
