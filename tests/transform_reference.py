"""float64 restatement of GaussianModel.transform_ (csrc/transform.hip) - a helper, not a test.

Independent of the kernel's route to the SH rotation: the band matrices come from a least-squares fit over 96 directions with
scene_utils.sh.sh_basis (M = lstsq(B(d), B(d @ R)), c' = c @ M^T), not from the kernel's 2 l + 1 sample directions and baked
inverses.  Every function takes the float32 tensors the kernel reads, upcasts them, and returns for each output tensor the
float64 value and, per element, the magnitude sum_j |a_j| |b_j| of the dot product that produces it (what the tolerances of
tests/test_transform_gpu.py are stated in)."""
import math

import numpy as np
import torch

from scene_utils.sh import sh_basis

U = 2.0 ** -24                 # unit roundoff of float32


def gamma(m):
    return m * U / (1.0 - m * U)


def fit_directions(n=96):
    """n unit vectors on a Fibonacci sphere, float64 [n,3]."""
    i = torch.arange(n, dtype=torch.float64) + 0.5
    z = 1.0 - 2.0 * i / n
    rho = torch.sqrt(1.0 - z * z)
    th = math.pi * (3.0 - math.sqrt(5.0)) * i
    return torch.stack([rho * torch.cos(th), rho * torch.sin(th), z], dim=1)


def sh_rotation(R, deg=3):
    """M [(deg+1)^2, (deg+1)^2] float64 with c' = c @ M^T: B(d) M = B(d @ R) for directions d as rows."""
    R = torch.as_tensor(np.asarray(R), dtype=torch.float64)
    d = fit_directions()
    return torch.linalg.lstsq(sh_basis(deg, d), sh_basis(deg, d @ R)).solution


def band(M, l):
    return M[l * l:(l + 1) ** 2, l * l:(l + 1) ** 2]


def random_rotation(rng, angle=1.0):
    """Rotation by `angle` rad about a random axis, float64 numpy [3,3] (Rodrigues)."""
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


def make_T(R, t, s=1.0):
    T = np.eye(4)
    T[:3, :3] = s * np.asarray(R)
    T[:3, 3] = t
    return T


def quat_of(R):
    """Unit quaternion (w, x, y, z) of R in float64 from its axis and angle (for angles away from 0 and pi, as the tests use),
    sign fixed like the kernel's: the component that the largest of (trace, R00, R11, R22) names is positive."""
    R = np.asarray(R, dtype=np.float64)
    axis = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    sin_t = 0.5 * np.linalg.norm(axis)
    theta = math.atan2(sin_t, 0.5 * (np.trace(R) - 1.0))
    assert 1e-3 < theta < math.pi - 1e-3, theta
    q = np.concatenate([[math.cos(0.5 * theta)], math.sin(0.5 * theta) * axis / np.linalg.norm(axis)])
    pivot = int(np.argmax([np.trace(R), R[0, 0], R[1, 1], R[2, 2]]))
    return q if q[pivot] > 0 else -q


def hamilton(a, b):
    """a [4] (x) b [P,4] -> (product [P,4], sum of |terms| [P,4]), (w, x, y, z)."""
    a0, a1, a2, a3 = (float(v) for v in a)
    b0, b1, b2, b3 = b.unbind(dim=1)
    terms = [[a0 * b0, -a1 * b1, -a2 * b2, -a3 * b3], [a0 * b1, a1 * b0, a2 * b3, -a3 * b2],
             [a0 * b2, -a1 * b3, a2 * b0, a3 * b1], [a0 * b3, a1 * b2, -a2 * b1, a3 * b0]]
    val = torch.stack([sum(t) for t in terms], dim=1)
    mag = torch.stack([sum(x.abs() for x in t) for t in terms], dim=1)
    return val, mag


def transform_reference(xyz, rotation, scaling, features_rest, T, index=None):
    """xyz [P,3], rotation [P,4], scaling [P,3], features_rest [P,M,3] (float32, any device), T [K,4,4] float64 (numpy), index
    None (every row by T[0]) or an integer tensor [P] (rows outside [0,K) stay).
    -> {"xyz" | "rotation" | "scaling" | "features_rest": (value float64, magnitude float64)}, moved bool [P]."""
    T = np.asarray(T, dtype=np.float64).reshape(-1, 4, 4)
    K, P = T.shape[0], xyz.shape[0]
    x, q, sc, f = (t.detach().cpu().double() for t in (xyz, rotation, scaling, features_rest))
    idx = torch.zeros(P, dtype=torch.long) if index is None else index.detach().cpu().long()
    moved = (idx >= 0) & (idx < K)
    out = {"xyz": [x.clone(), x.abs()], "rotation": [q.clone(), q.abs()], "scaling": [sc.clone(), sc.abs()],
           "features_rest": [f.clone(), f.abs()]}
    n_rest = f.shape[1]
    for k in range(K):
        rows = moved & (idx == k)
        if not bool(rows.any()):
            continue
        M3 = T[k, :3, :3]
        s = float(np.cbrt(np.linalg.det(M3)))
        R = M3 / s
        sR, t = torch.tensor(M3), torch.tensor(T[k, :3, 3])
        out["xyz"][0][rows] = x[rows] @ sR.T + t
        out["xyz"][1][rows] = x[rows].abs() @ sR.abs().T + t.abs()
        v, m = hamilton(quat_of(R), q[rows])
        out["rotation"][0][rows], out["rotation"][1][rows] = v, m
        out["scaling"][0][rows] = sc[rows] + math.log(s)
        out["scaling"][1][rows] = sc[rows].abs() + abs(math.log(s))
        if n_rest:
            deg = int(round(math.sqrt(n_rest + 1))) - 1
            M = sh_rotation(R, deg)[1:, 1:]                       # bands 1.. (band 0 is features_dc: invariant)
            c = f[rows]                                          # [n, M, 3]
            out["features_rest"][0][rows] = torch.einsum("ab,nbc->nac", M, c)
            out["features_rest"][1][rows] = torch.einsum("ab,nbc->nac", M.abs(), c.abs())
    return {k: tuple(v) for k, v in out.items()}, moved


def band_of_rest_row(n_rest):
    """[n_rest] long: the SH band of every row of features_rest."""
    return torch.tensor([int(math.isqrt(k + 1)) for k in range(n_rest)], dtype=torch.long)
