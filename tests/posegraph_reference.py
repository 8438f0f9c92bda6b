"""Float64 numpy restatement of the pose-graph definitions of include/gsr.h (gsr_posegraph_*, gsr_registration_information),
with the case builders the pose-graph tests share.  H is assembled densely and solved by numpy.linalg.solve; `pcg` restates the
device's preconditioned conjugate gradients (block-Jacobi from the 6 x 6 LDL^T with its pivot rule, the same stopping rule)."""
import numpy as np

PIVOT_MIN = 1e-12
ST_STEP, ST_MAX_ITERATION, ST_SOLVER, ST_RESIDUAL, ST_ZERO, ST_LAMBDA = 0, 1, 2, 3, 4, 5
CONVERGED = (ST_STEP, ST_RESIDUAL, ST_ZERO)
EDGE_STRIDE, NODE_STRIDE = 35, 27      # e[6] r w W[21] g[6]; H_ii[21] b[6]
TRIU = np.triu_indices(6)


# ---- M(delta), vec6, lin6 ----------------------------------------------------------------------------------------------------
def compose(d):
    sa, ca, sb, cb, sg, cg = np.sin(d[0]), np.cos(d[0]), np.sin(d[1]), np.cos(d[1]), np.sin(d[2]), np.cos(d[2])
    M = np.eye(4)
    M[:3, :3] = [[cb * cg, sa * sb * cg - ca * sg, ca * sb * cg + sa * sg],
                 [cb * sg, sa * sb * sg + ca * cg, ca * sb * sg - sa * cg],
                 [-sb, sa * cb, ca * cb]]
    M[:3, 3] = d[3:6]
    return M


def vec6(D):
    R = D[:3, :3]
    sy = np.sqrt(R[0, 0] * R[0, 0] + R[1, 0] * R[1, 0])
    if sy > 1e-6:
        a, b, g = np.arctan2(R[2, 1], R[2, 2]), np.arctan2(-R[2, 0], sy), np.arctan2(R[1, 0], R[0, 0])
    else:
        a, b, g = np.arctan2(-R[1, 2], R[1, 1]), np.arctan2(-R[2, 0], sy), 0.0
    return np.array([a, b, g, D[0, 3], D[1, 3], D[2, 3]])


def lin6(M):
    return np.array([(M[2, 1] - M[1, 2]) / 2, (M[0, 2] - M[2, 0]) / 2, (M[1, 0] - M[0, 1]) / 2, M[0, 3], M[1, 3], M[2, 3]])


def inv_rigid(T):
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return out


def relative(Xt, Xs):
    """X_t^-1 X_s with the difference of the translations taken first (nothing is lost far from the origin)"""
    out = np.eye(4)
    out[:3, :3] = Xt[:3, :3].T @ Xs[:3, :3]
    out[:3, 3] = Xt[:3, :3].T @ (Xs[:3, 3] - Xt[:3, 3])
    return out


def _generators():
    G = np.zeros((6, 4, 4))
    G[0, 1, 2], G[0, 2, 1] = -1, 1
    G[1, 0, 2], G[1, 2, 0] = 1, -1
    G[2, 0, 1], G[2, 1, 0] = -1, 1
    for a in range(3):
        G[3 + a, a, 3] = 1
    return G


GEN = _generators()


def residual(Xs, Xt, T):
    return vec6(inv_rigid(T) @ relative(Xt, Xs))


def jacobian(Xs, Xt, T):
    A = inv_rigid(T) @ inv_rigid(Xt)
    return np.stack([lin6(A @ GEN[j] @ Xs) for j in range(6)], axis=1)


# ---- the graph ---------------------------------------------------------------------------------------------------------------
class Graph:
    def __init__(self, poses, fixed, s, t, T, L, uncertain, truth=None, mu=0.25, name=""):
        self.poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
        self.N = self.poses.shape[0]
        self.fixed = np.asarray(fixed, bool).reshape(self.N)
        self.s = np.asarray(s, np.int32).reshape(-1)
        self.t = np.asarray(t, np.int32).reshape(-1)
        self.E = self.s.shape[0]
        self.T = np.asarray(T, np.float64).reshape(self.E, 4, 4)
        self.L = np.asarray(L, np.float64).reshape(self.E, 6, 6)
        self.uncertain = np.asarray(uncertain, bool).reshape(self.E)
        self.truth = None if truth is None else np.asarray(truth, np.float64)
        self.mu, self.name = float(mu), name

    def extent(self):
        p = (self.truth if self.truth is not None else self.poses)[:, :3, 3]
        return float(np.linalg.norm(p.max(0) - p.min(0))) if self.N > 1 else 1.0

    def csr(self):
        """node_ptr [N+1], node_edge [2E]: 2 k + (1 where the node is the edge's target), ascending k per node"""
        lists = [[] for _ in range(self.N)]
        for k in range(self.E):
            lists[self.s[k]].append(2 * k)
            lists[self.t[k]].append(2 * k + 1)
        ptr = np.zeros(self.N + 1, np.int32)
        ptr[1:] = np.cumsum([len(l) for l in lists])
        return ptr, np.array([v for l in lists for v in l], np.int32)


def robust(r, uncertain, mu):
    """(cost, weight) of an edge"""
    if not uncertain:
        return r, 1.0
    return mu * r / (mu + r), (mu / (mu + r)) ** 2


def cost(G, X, mu):
    F = 0.0
    for k in range(G.E):
        e = residual(X[G.s[k]], X[G.t[k]], G.T[k])
        F += robust(e @ G.L[k] @ e, G.uncertain[k], mu)[0]
    return F


def linearize(G, X, mu):
    E, N = G.E, G.N
    out = dict(e=np.zeros((E, 6)), r=np.zeros(E), w=np.zeros(E), W=np.zeros((E, 6, 6)), g=np.zeros((E, 6)),
               H=np.zeros((N, 6, 6)), b=np.zeros((N, 6)), J=np.zeros((E, 6, 6)))
    F = 0.0
    for k in range(E):
        s, t = G.s[k], G.t[k]
        e = residual(X[s], X[t], G.T[k])
        J = jacobian(X[s], X[t], G.T[k])
        r = e @ G.L[k] @ e
        c, w = robust(r, G.uncertain[k], mu)
        F += c
        W = w * (J.T @ G.L[k] @ J)
        g = w * (J.T @ (G.L[k] @ e))
        out["e"][k], out["r"][k], out["w"][k], out["W"][k], out["g"][k], out["J"][k] = e, r, w, W, g, J
        if not G.fixed[s]:
            out["H"][s] += W
            out["b"][s] += g
        if not G.fixed[t]:
            out["H"][t] += W
            out["b"][t] -= g
    out["F"] = F
    out["maxdiag"] = float(max([0.0] + [out["H"][i][a, a] for i in range(N) for a in range(6)]))
    return out


def edge_records(lin):
    """[E,35] as gsr_posegraph_linearize writes them"""
    E = lin["e"].shape[0]
    return np.concatenate([lin["e"], lin["r"][:, None], lin["w"][:, None], lin["W"][:, TRIU[0], TRIU[1]].reshape(E, 21), lin["g"]], 1)


def node_records(lin):
    N = lin["b"].shape[0]
    return np.concatenate([lin["H"][:, TRIU[0], TRIU[1]].reshape(N, 21), lin["b"]], 1)


def dense_matrix(G, lin, lam):
    """(H + lam I over the free nodes, -b, the free nodes)"""
    free = np.flatnonzero(~G.fixed)
    pos = -np.ones(G.N, int)
    pos[free] = np.arange(free.size)
    n = 6 * free.size
    H = np.zeros((n, n))
    for i in free:
        H[6 * pos[i]:6 * pos[i] + 6, 6 * pos[i]:6 * pos[i] + 6] = lin["H"][i]
    for k in range(G.E):
        s, t = pos[G.s[k]], pos[G.t[k]]
        if s >= 0 and t >= 0:
            H[6 * s:6 * s + 6, 6 * t:6 * t + 6] -= lin["W"][k]
            H[6 * t:6 * t + 6, 6 * s:6 * s + 6] -= lin["W"][k].T
    return H + lam * np.eye(n), -lin["b"][free].reshape(-1), free


def ldlt6(A):
    """(L, D) or None: the pivot rule of the shared 6 x 6 body"""
    L, D = np.eye(6), np.zeros(6)
    for j in range(6):
        d = A[j, j] - sum(L[j, k] * L[j, k] * D[k] for k in range(j))
        if not np.isfinite(d) or not d > PIVOT_MIN * A[j, j]:
            return None
        D[j] = d
        for i in range(j + 1, 6):
            L[i, j] = (A[i, j] - sum(L[i, k] * L[j, k] * D[k] for k in range(j))) / d
    return L, D


def _blocks(G, lin, lam):
    facs = {}
    for i in np.flatnonzero(~G.fixed):
        f = ldlt6(lin["H"][i] + lam * np.eye(6))
        if ldlt6(lin["H"][i]) is None or f is None:      # H_ii alone first: lam I would hide a node that its edges do not fix
            return None
        facs[i] = np.linalg.inv(f[0] @ np.diag(f[1]) @ f[0].T)
    return facs


def solve(G, lin, lam, solver="dense", cg_rtol=1e-12, cg_max_iteration=None):
    """-> (delta [N,6], cg iterations, achieved |r| / |b|, status 0 / 1 (cg_max_iteration) / 2 (a rejected pivot))"""
    delta = np.zeros((G.N, 6))
    facs = _blocks(G, lin, lam)
    if facs is None:
        return delta, 0, 0.0, 2
    A, rhs, free = dense_matrix(G, lin, lam)
    bn = np.linalg.norm(rhs)
    if free.size == 0 or bn == 0.0:
        return delta, 0, 0.0, 0
    if solver == "dense":
        x = np.linalg.solve(A, rhs)
        delta[free] = x.reshape(-1, 6)
        return delta, 0, float(np.linalg.norm(A @ x - rhs) / bn), 0
    if cg_max_iteration is None:
        cg_max_iteration = min(6 * G.N, 1000)

    def prec(v):
        return np.concatenate([facs[i] @ v[6 * a:6 * a + 6] for a, i in enumerate(free)])
    x = np.zeros_like(rhs)
    r = rhs.copy()
    z = prec(r)
    p = z.copy()
    rz = r @ z
    it, status, rel = 0, 1, 1.0
    for it in range(1, cg_max_iteration + 1):
        Ap = A @ p
        pAp = p @ Ap
        if not pAp > 0:
            return np.zeros((G.N, 6)), it, rel, 2
        alpha = rz / pAp
        x += alpha * p
        r -= alpha * Ap
        rel = float(np.linalg.norm(r) / bn)
        if rel <= cg_rtol:
            status = 0
            break
        z = prec(r)
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
    delta[free] = x.reshape(-1, 6)
    return delta, it, rel, status


def apply_step(X, delta):
    out = X.copy()
    for i in range(X.shape[0]):
        out[i] = compose(delta[i]) @ X[i]
        out[i, 3] = [0, 0, 0, 1]
    return out


def optimize(G, mu=None, max_iteration=100, min_relative_increment=1e-6, min_relative_residual_increment=1e-6, solver="dense",
             cg_rtol=1e-12, cg_max_iteration=None):
    mu = G.mu if mu is None else mu
    X = G.poses.copy()
    lin = linearize(G, X, mu)
    F = F0 = lin["F"]
    lam, nu = 1e-5 * lin["maxdiag"], 2.0
    res = dict(status=ST_MAX_ITERATION, iterations=0, accepted=0, F_start=F0, cg_iterations=0, cg_worst=0.0)
    if F == 0.0:
        res["status"] = ST_ZERO
    else:
        for _ in range(max_iteration):
            delta, cgi, rel, st = solve(G, lin, lam, solver, cg_rtol, cg_max_iteration)
            res["cg_iterations"] += cgi
            res["cg_worst"] = max(res["cg_worst"], rel)
            if st == 2:
                res["status"] = ST_SOLVER
                break
            res["iterations"] += 1
            xinf = max(np.abs(vec6(Xi)).max() for Xi in X)
            if np.abs(delta).max() <= min_relative_increment * (xinf + min_relative_increment):
                res["status"] = ST_STEP
                break
            Xn = apply_step(X, delta)
            Fn = cost(G, Xn, mu)
            d, b = delta.reshape(-1), lin["b"].reshape(-1)
            rho = (F - Fn) / (d @ (lam * d - b))
            if Fn < F:
                X = Xn
                res["accepted"] += 1
                small = F - Fn <= min_relative_residual_increment * F
                F = Fn
                lam *= max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3)
                nu = 2.0
                if small:
                    res["status"] = ST_RESIDUAL
                    break
                if F == 0.0:
                    res["status"] = ST_ZERO
                    break
                lin = linearize(G, X, mu)
            else:
                lam *= nu
                nu *= 2.0
            if not np.isfinite(lam) or lam > 1e32:
                res["status"] = ST_LAMBDA
                break
    wr = [(lambda e: e @ G.L[k] @ e)(residual(X[G.s[k]], X[G.t[k]], G.T[k])) for k in range(G.E)]
    res.update(poses=X, F_end=F, lam=lam, r=np.array(wr), w=np.array([robust(r, G.uncertain[k], mu)[1] for k, r in enumerate(wr)]))
    return res


# ---- information matrix ------------------------------------------------------------------------------------------------------
def information(target, idx):
    """(Lambda [6,6], n): sum over the participating rows of G^T G, formed row by row"""
    target = np.asarray(target, np.float64)
    A, n = np.zeros((6, 6)), 0
    for i in idx:
        if not 0 <= i < target.shape[0] or not np.isfinite(target[i]).all():
            continue
        x, y, z = target[i]
        for row in ([0, z, -y, 1, 0, 0], [-z, 0, x, 0, 1, 0], [y, -x, 0, 0, 0, 1]):
            A += np.outer(row, row)
        n += 1
    return A, n


# ---- cases -------------------------------------------------------------------------------------------------------------------
INFO = 100.0 * np.eye(6)      # as if from 100 correspondences of unit spread; mu = 1.0 * 0.05^2 * 100 = 0.25


def _noise(rng, trans, rot_deg):
    return compose(np.concatenate([rng.normal(0, np.radians(rot_deg), 3), rng.normal(0, trans, 3)]))


def ring_truth(n, radius=2.0, offset=(0.0, 0.0, 0.0)):
    X = []
    for i in range(n):
        a = 2 * np.pi * i / n
        P = compose([0.1 * np.sin(a), 0.05 * np.cos(2 * a), a + np.pi / 2, 0, 0, 0])
        P[:3, 3] = np.array([radius * np.cos(a), radius * np.sin(a), 0.2 * np.sin(3 * a)]) + np.asarray(offset)
        X.append(P)
    return np.stack(X)


def _measure(truth, s, t, noise=None):
    T = relative(truth[t], truth[s])
    return T if noise is None else T @ noise


def ring(n, seed, trans=0.0, rot_deg=0.0, loops=(), false_loops=(), start_noise=None, offset=(0, 0, 0), certain_false=False,
         name=""):
    """a ring of n keyframes: odometry edges i -> i + 1, the closing edge n - 1 -> 0 and `loops` as uncertain edges, node 0 fixed;
    the start is the noisy odometry chained from node 0 (or the truth moved by `start_noise` = (m, degrees))"""
    rng = np.random.default_rng(seed)
    truth = ring_truth(n, offset=offset)
    s, t, T, unc = [], [], [], []
    for i in range(n - 1):
        s.append(i), t.append(i + 1), unc.append(False)
        T.append(_measure(truth, i, i + 1, _noise(rng, trans, rot_deg) if trans or rot_deg else None))
    for a, b in [(n - 1, 0)] + list(loops):
        s.append(a), t.append(b), unc.append(True)
        T.append(_measure(truth, a, b, _noise(rng, trans, rot_deg) if trans or rot_deg else None))
    for a, b in false_loops:
        off = np.eye(4)
        off[:3, 3] = [2.0, 0.0, 0.0]
        s.append(a), t.append(b), unc.append(not certain_false)
        T.append(_measure(truth, a, b) @ off)
    poses = [truth[0]]
    if start_noise is None:
        for i in range(n - 1):      # X_{i+1} = X_i T_i^-1
            poses.append(poses[-1] @ inv_rigid(T[i]))
    else:
        for i in range(1, n):
            poses.append(_noise(rng, *start_noise) @ truth[i])
    fixed = np.zeros(n, bool)
    fixed[0] = True
    return Graph(np.stack(poses), fixed, s, t, T, np.broadcast_to(INFO, (len(s), 6, 6)).copy(), unc, truth=truth, name=name)


def two_nodes():
    truth = ring_truth(5)[:2]
    poses = truth.copy()
    poses[1] = compose([0.02, -0.03, 0.05, 0.1, -0.05, 0.08]) @ truth[1]
    return Graph(poses, [True, False], [0], [1], [_measure(truth, 0, 1)], [INFO], [False], truth=truth, name="two_nodes")


def exact_ring():
    return ring(8, 1, loops=[(2, 6)], start_noise=(0.05, 2.0), name="exact_ring8")


def noisy_ring():
    return ring(16, 2, 0.01, 0.5, name="noisy_ring16")


def quiet_ring():
    """the ring of 16 at half the noise: where Open3D's linearisation ends within 1e-6 of the minimum of F (test_posegraph_cpu)"""
    return ring(16, 2, 0.005, 0.25, name="quiet_ring16")


FALSE_EDGE = (3, 11)


def false_loop_ring(certain=False):
    return ring(16, 2, 0.01, 0.5, false_loops=[FALSE_EDGE], certain_false=certain, name="false_loop_ring16")


def far_ring():
    return ring(16, 3, 0.01, 0.5, offset=(10000.0, -10000.0, 50.0), name="ring16_10km")


def two_fixed():
    """a chain 0 .. 5 with both ends fixed, and a free node 6 whose neighbours (0 and 5) are both fixed"""
    rng = np.random.default_rng(4)
    truth = ring_truth(12)[:7]
    pairs = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (6, 0), (5, 6), (1, 4)]
    T = [_measure(truth, a, b, _noise(rng, 0.01, 0.5)) for a, b in pairs]
    poses = np.stack([truth[0]] + [_noise(rng, 0.03, 1.0) @ truth[i] for i in range(1, 5)] + [truth[5]] +
                     [_noise(rng, 0.03, 1.0) @ truth[6]])
    fixed = np.array([1, 0, 0, 0, 0, 1, 0], bool)
    unc = [False] * 7 + [True]
    return Graph(poses, fixed, [p[0] for p in pairs], [p[1] for p in pairs], T, [INFO] * 8, unc, truth=truth, name="two_fixed")


def random_graph(N=257, seed=5):
    """a chain through all nodes plus random chords; node 7 has degree over 64; the nodes of the tail have degree 1"""
    rng = np.random.default_rng(seed)
    truth = np.stack([compose(np.concatenate([rng.uniform(-0.5, 0.5, 3), rng.uniform(-5, 5, 3)])) for _ in range(N)])
    pairs, seen = [], set()

    def add(a, b):
        if a != b and (a, b) not in seen and (b, a) not in seen:
            seen.add((a, b))
            pairs.append((a, b))
    tail = 8
    for i in range(N - tail - 1):
        add(i, i + 1)
    for i in range(N - tail, N):      # leaves: one edge each
        add(int(rng.integers(0, N - tail)), i)
    for j in rng.choice(N - tail, 70, replace=False):
        add(7, int(j))
    while len(pairs) < 1300:
        a, b = rng.integers(0, N - tail, 2)
        add(int(a), int(b))
    T = [_measure(truth, a, b, _noise(rng, 0.01, 0.5)) for a, b in pairs]
    poses = np.stack([truth[0]] + [_noise(rng, 0.03, 1.0) @ truth[i] for i in range(1, N)])
    fixed = np.zeros(N, bool)
    fixed[0] = True
    unc = rng.random(len(pairs)) < 0.2
    unc[:N - tail - 1] = False
    return Graph(poses, fixed, [p[0] for p in pairs], [p[1] for p in pairs], T, [INFO] * len(pairs), unc, truth=truth,
                 name="random257")


def no_edges():
    truth = ring_truth(4)
    return Graph(truth, [True, False, False, False], [], [], np.zeros((0, 4, 4)), np.zeros((0, 6, 6)), [], truth=truth, name="no_edges")


def zero_information():
    """0 (fixed) - 1 with information, 1 - 2 with Lambda = 0: nothing holds node 2"""
    truth = ring_truth(6)[:3]
    poses = truth.copy()
    poses[1] = compose([0.01, 0.02, -0.01, 0.05, 0.02, -0.03]) @ truth[1]
    return Graph(poses, [True, False, False], [0, 1], [1, 2], [_measure(truth, 0, 1), _measure(truth, 1, 2)],
                 [INFO, np.zeros((6, 6))], [False, False], truth=truth, name="zero_information")


def linearize_cases():
    return [two_nodes(), exact_ring(), noisy_ring(), false_loop_ring(), random_graph(), two_fixed(), far_ring(), zero_information()]


def solve_cases():
    """(graph, lambda factor of max diag(H)): well-conditioned systems"""
    return [two_nodes(), exact_ring(), noisy_ring(), false_loop_ring(), random_graph(), two_fixed()]


def noisy_cases():
    return [noisy_ring(), false_loop_ring(), random_graph(), two_fixed(), far_ring()]


def end_to_end_cases():
    return [two_nodes(), exact_ring()] + noisy_cases()
