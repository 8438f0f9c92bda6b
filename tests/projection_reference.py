"""float64 replay of the projection kernels, Gaussian by Gaussian, on their own call arguments (csrc/preprocess.hip: k_preprocess_fwd
staged and unstaged, k_shade, k_preprocess_bwd).  numpy only, no GPU, nothing imported from the library.  The rules are the
published ones (oracle/gs_oracle.py) plus the guards, margins and the record layout include/gsr.h states
("Projection rules" there).  The forward is written from those.  The backward follows the hand derivation of the published
backward term by term, as k_preprocess_bwd does - the same grouping is what makes the float32 yardstick mean something -
so it is not independent of the kernel by construction: its independence comes from tests/test_projection_reference_cpu.py, which
holds it to central differences of the forward and to the oracle's autograd.

ARITHMETIC.  Every function runs in one of two arithmetics.  float64 (`np.float64`): the reference; every value is an `M` = (value,
S) where S is the float64 sum of the magnitudes of the terms added to form it, carried through the stages to first order:
    S(a + b) = S(a) + S(b)            S(a b) = S(a) |b| + |a| S(b) - |a b|          S(f(a)) = |f(a)| + |f'(a)| S(a)
(f = sqrt, exp, log: the argument's own rounding passes through f', which is what makes log near 1 and exp of a large power
ill-conditioned), so an input or a product of inputs has S = |value|, and a difference has the sum of its operands' magnitudes: the ill-conditioning of
a needle's a c - b^2 is in S, not in the bound.  float32 (`np.float32`): the YARDSTICK - plain numpy, every operation rounded on its
own, no fused multiply-add.  The error figure of a value is |got - float64| / S; the bound of a value class is max(2^-24, 4 x the
float32 replay's largest figure over all cases) (YARDSTICK below, measured by `measure()`, recomputed by
tests/test_projection_reference_cpu.py).  Nothing here is measured against a kernel.
Both arithmetics use the kernels' float32 constants (0.2f, 1.3f, 0.3f ...) unless published = True (the oracle's doubles).

DISCRETE VALUES.  A discrete value (visibility, radius, 3-sigma tile rectangle, first-stage box, clamp masks, colour clamp bits, the
AA floor switch) comes as a pair (lo, hi): decided where lo == hi.  It is UNDECIDED where its float64 argument lies within a margin
of the threshold (an integer, for ceil / truncation); the margin is 4 x the float32 replay's own largest error on that argument
(YARDSTICK["arg_*"], S-relative, floor 2^-24) x the argument's S.  A threshold hit exactly is undecided.  A case may have at most
UNDECIDED_CAP = 2 % of its visible Gaussians undecided per discrete value.

BACKWARD.  Starts from the ten per-Gaussian sums k_preprocess_bwd forms from the gradient records (first moments, second moments of
h = dL/dpower / op_eff - multiplied by op_eff here -, dL/dop_eff, dL/drgb, dL/d(depth channel)); each sum comes with the sum of the
magnitudes of its partial sums (slot order) as its S.  Returns the gradients and the cotangents between the stages."""
import math

import numpy as np

TILE = 16
U = 2.0 ** -24
FLOOR = U
FACTOR = 4.0
UNDECIDED_CAP = 0.02
LOG2E = 1.4426950408889634
SH_C0 = 0.28209479177387814
SH_C1 = 0.4886025119029199
SH_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
SH_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
         -0.5900435899266435)
RECORD = ("px", "py", "sA", "sB", "sC", "op", "spmin", "r", "g", "b", "dchan", "depth")
ARGS = ("arg_tz", "arg_radius", "arg_rect", "arg_box", "arg_pmin", "arg_clamp", "arg_aa")
GRADS = ("means2D", "means3D", "opacities", "scales", "rotations", "cov3D", "shs", "colors")
STAGES = ("conic->cov2D", "cov2D->Sigma", "cov2D->M", "M->J->t", "t,NDC->mean", "Sigma->s,q")
CLASSES = RECORD + ARGS + GRADS

# The float32 replay's largest |float32 - float64| / S per value class over all cases and the call forms of `yardstick_forms()`
# (measure() reprints them; tests/test_projection_reference_cpu.py recomputes them).
YARDSTICK = {
    "px": 1.4093e-07,   # regular / base
    "py": 1.5690e-07,   # partial_tiles / base
    "sA": 2.2978e-07,   # edge / cov
    "sB": 5.4053e-07,   # edge / cov
    "sC": 2.2084e-07,   # regular / cov
    "op": 1.5419e-07,   # regular / raw
    "spmin": 1.2780e-07,   # single_tile / base
    "r": 1.5940e-07,   # regular / raw-aa-mod2.3
    "g": 1.3187e-07,   # needles_08 / base
    "b": 1.2705e-07,   # saturating / base
    "dchan": 9.9687e-08,   # needles_08 / base
    "depth": 6.8454e-08,   # saturating / base
    "arg_tz": 6.8454e-08,   # saturating / base
    "arg_radius": 1.0946e-07,   # regular / cov
    "arg_rect": 1.4669e-07,   # regular / mod0.5
    "arg_box": 1.4551e-07,   # needles / cov
    "arg_pmin": 1.0297e-07,   # regular / raw
    "arg_clamp": 1.8172e-07,   # regular / base
    "arg_aa": 2.2598e-07,   # edge / cov
    "means2D": 2.5059e-07,   # edge / cov
    "means3D": 2.6623e-07,   # edge / cov
    "opacities": 7.7957e-08,   # edge / cov-aa
    "scales": 5.1846e-07,   # edge / mod0.5
    "rotations": 2.0212e-07,   # edge / base
    "cov3D": 5.5370e-07,   # edge / cov
    "shs": 1.8004e-07,   # needles_08 / base
    "colors": 5.5275e-08,   # regular / colors
}


# ---------------------------------------------------------------------------------------------------------------------------------
# the two arithmetics
# ---------------------------------------------------------------------------------------------------------------------------------
class M:
    """float64 value with the magnitude sum S of its terms"""
    __slots__ = ("v", "m")
    __array_ufunc__ = None

    def __init__(self, v, m=None):
        self.v = np.asarray(v, dtype=np.float64)
        # (inf / inf or 0 x inf in the magnitudes - a logit of -inf - falls back to the value's own magnitude: S >= |value| always)
        self.m = np.abs(self.v) if m is None else np.where(np.isnan(m), np.abs(self.v), np.asarray(m, dtype=np.float64))

    @staticmethod
    def of(o):
        return o if isinstance(o, M) else M(o)

    def __add__(self, o):
        o = M.of(o)
        return M(self.v + o.v, self.m + o.m)
    __radd__ = __add__

    def __sub__(self, o):
        o = M.of(o)
        return M(self.v - o.v, self.m + o.m)

    def __rsub__(self, o):
        return M.of(o).__sub__(self)

    def __neg__(self):
        return M(-self.v, self.m)

    def __mul__(self, o):
        o = M.of(o)
        v = self.v * o.v
        return M(v, self.m * np.abs(o.v) + np.abs(self.v) * o.m - np.abs(v))
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = M.of(o)
        with np.errstate(all="ignore"):
            v = self.v / o.v
            return M(v, self.m / np.abs(o.v) + np.abs(self.v) * o.m / (o.v * o.v) - np.abs(v))

    def __rtruediv__(self, o):
        return M.of(o).__truediv__(self)

    def __getitem__(self, i):
        return M(self.v[i], self.m[i])


class Arith:
    """dt = np.float64: values are M; dt = np.float32: plain float32 arrays"""

    def __init__(self, dt):
        self.dt = dt
        self.f64 = dt == np.float64

    def k(self, x):                      # a constant
        return M(np.float64(x)) if self.f64 else np.float32(x)

    def arr(self, x, mag=None):          # an input array (float32 data, promoted exactly)
        x = np.asarray(x)
        return M(x, mag) if self.f64 else x.astype(np.float32)

    def _un(self, a, f, df):
        if not self.f64:
            with np.errstate(all="ignore"):
                return f(a).astype(np.float32) if isinstance(a, np.ndarray) else np.float32(f(a))
        with np.errstate(all="ignore"):
            v = f(a.v)
            ex = np.abs(df(a.v)) * a.m
        return M(v, np.abs(v) + np.where(a.m > 0.0, ex, 0.0))

    def sqrt(self, a):
        return self._un(a, np.sqrt, lambda v: 0.5 / np.sqrt(v))

    def exp(self, a):
        return self._un(a, np.exp, np.exp)

    def log(self, a):
        return self._un(a, np.log, lambda v: 1.0 / v)

    def where(self, c, a, b):
        if not self.f64:
            return np.where(c, a, b).astype(np.float32)
        a, b = M.of(a), M.of(b)
        return M(np.where(c, a.v, b.v), np.where(c, a.m, b.m))

    def maximum(self, a, b):
        return self.where(self.val(a) >= self.val(b), a, b)

    def minimum(self, a, b):
        return self.where(self.val(a) <= self.val(b), a, b)

    def val(self, a):
        return a.v if isinstance(a, M) else np.asarray(a, dtype=np.float64)

    def mag(self, a):
        return a.m if isinstance(a, M) else np.abs(np.asarray(a, dtype=np.float64))

    def stack(self, xs):
        if self.f64:
            xs = [M.of(x) for x in xs]
            return M(np.stack(np.broadcast_arrays(*[x.v for x in xs]), axis=-1), np.stack(np.broadcast_arrays(*[x.m for x in xs]), axis=-1))
        return np.stack(np.broadcast_arrays(*xs), axis=-1).astype(np.float32)


def consts(published):
    """The constants of the rules: the kernels' float32 values, or (published) the decimal ones the oracle uses"""
    f = (lambda x: float(x)) if published else (lambda x: float(np.float32(x)))
    return dict(near=f(0.2), lim=f(1.3), dil=f(0.3), aa_floor=f(0.000025), eps=f(0.0000001), lam_floor=f(0.1), box_mul=f(1.0001),
                box_add=f(0.01), pmargin=f(0.01), log2e=f(LOG2E), c0=f(SH_C0), c1=f(SH_C1), c2=[f(x) for x in SH_C2],
                c3=[f(x) for x in SH_C3], qeps=f(1e-12), big=f(1.0e9))


# ---------------------------------------------------------------------------------------------------------------------------------
# shared geometry: everything up to the dilated covariance, in either arithmetic
# ---------------------------------------------------------------------------------------------------------------------------------
def _sh_basis(ar, K, deg, x, y, z):
    c1, c2, c3 = ar.k(K["c1"]), [ar.k(v) for v in K["c2"]], [ar.k(v) for v in K["c3"]]
    b = [ar.k(K["c0"]) + x * ar.k(0.0)]
    if deg > 0:
        b += [-c1 * y, c1 * z, -c1 * x]
    if deg > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        two, three, four = ar.k(2.0), ar.k(3.0), ar.k(4.0)
        b += [c2[0] * xy, c2[1] * yz, c2[2] * (two * zz - xx - yy), c2[3] * xz, c2[4] * (xx - yy)]
        if deg > 2:
            b += [c3[0] * y * (three * xx - yy), c3[1] * xy * z, c3[2] * y * (four * zz - xx - yy),
                  c3[3] * z * (two * zz - three * xx - three * yy), c3[4] * x * (four * zz - xx - yy), c3[5] * z * (xx - yy),
                  c3[6] * x * (xx - three * yy)]
    return b


def _sh_basis_grad(ar, K, deg, x, y, z):
    """d basis_k / d(x, y, z) for k >= 1: list of (dx, dy, dz)"""
    c1, c2, c3 = ar.k(K["c1"]), [ar.k(v) for v in K["c2"]], [ar.k(v) for v in K["c3"]]
    o = x * ar.k(0.0)
    g = []
    if deg > 0:
        g += [(o, o - c1, o), (o, o, o + c1), (o - c1, o, o)]
    if deg > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        two, three, four, six, eight = ar.k(2.0), ar.k(3.0), ar.k(4.0), ar.k(6.0), ar.k(8.0)
        g += [(c2[0] * y, c2[0] * x, o), (o, c2[1] * z, c2[1] * y), (c2[2] * (-two * x), c2[2] * (-two * y), c2[2] * (four * z)),
              (c2[3] * z, o, c2[3] * x), (c2[4] * (two * x), c2[4] * (-two * y), o)]
        if deg > 2:
            g += [(c3[0] * (six * xy), c3[0] * (three * xx - three * yy), o),
                  (c3[1] * yz, c3[1] * xz, c3[1] * xy),
                  (c3[2] * (-two * xy), c3[2] * (four * zz - xx - three * yy), c3[2] * (eight * yz)),
                  (c3[3] * (-six * xz), c3[3] * (-six * yz), c3[3] * (six * zz - three * xx - three * yy)),
                  (c3[4] * (four * zz - three * xx - yy), c3[4] * (-two * xy), c3[4] * (eight * xz)),
                  (c3[5] * (two * xz), c3[5] * (-two * yz), c3[5] * (xx - yy)),
                  (c3[6] * (three * xx - three * yy), c3[6] * (-six * xy), o)]
    return g


def _geometry(inp, ar, K, freeze=None):
    """Mean, covariance and EWA stages of every Gaussian.  freeze = (tx, ty) float64: the clamped view-space x / y held constant
    where the clamp is active (the published backward's view of them: finite differences of the forward must do the same)"""
    W, H = int(inp["W"]), int(inp["H"])
    V = [ar.k(v) for v in np.asarray(inp["viewmatrix"], dtype=np.float32).reshape(-1)]
    PV = [ar.k(v) for v in np.asarray(inp["projmatrix"], dtype=np.float32).reshape(-1)]
    p = [ar.arr(inp["means3D"][:, j]) for j in range(3)]
    t = [V[i] * p[0] + V[4 + i] * p[1] + V[8 + i] * p[2] + V[12 + i] for i in range(3)]
    hom = [PV[i] * p[0] + PV[4 + i] * p[1] + PV[8 + i] * p[2] + PV[12 + i] for i in range(4)]
    pw = ar.k(1.0) / (hom[3] + ar.k(K["eps"]))
    ndc = [hom[0] * pw, hom[1] * pw]
    g = dict(W=W, H=H, V=V, PV=PV, p=p, t=t, hom=hom, pw=pw, ndc=ndc)
    # covariance
    if inp.get("cov3D") is not None:
        cov6 = [ar.arr(inp["cov3D"][:, j]) for j in range(6)]
    else:
        s3 = [ar.arr(inp["scales"][:, j]) for j in range(3)]
        q4 = [ar.arr(inp["rotations"][:, j]) for j in range(4)]
        qden = ar.k(1.0)
        if inp["raw"]:
            s3 = [ar.exp(s) for s in s3]
            qden = ar.maximum(ar.sqrt(q4[0] * q4[0] + q4[1] * q4[1] + q4[2] * q4[2] + q4[3] * q4[3]), ar.k(K["qeps"]) + q4[0] * ar.k(0.0))
            q4 = [q / qden for q in q4]
        r, x, y, z = q4
        one, two = ar.k(1.0), ar.k(2.0)
        R = [[one - two * (y * y + z * z), two * (x * y - r * z), two * (x * z + r * y)],
             [two * (x * y + r * z), one - two * (x * x + z * z), two * (y * z - r * x)],
             [two * (x * z - r * y), two * (y * z + r * x), one - two * (x * x + y * y)]]
        mod = ar.k(np.float32(inp["scale_modifier"]))
        sp = [mod * s for s in s3]
        L = [[R[i][j] * sp[j] for j in range(3)] for i in range(3)]
        S = [[L[i][0] * L[k][0] + L[i][1] * L[k][1] + L[i][2] * L[k][2] for k in range(3)] for i in range(3)]
        cov6 = [S[0][0], S[0][1], S[0][2], S[1][1], S[1][2], S[2][2]]
        g.update(s3=s3, q4=q4, qden=qden, R=R, sp=sp, mod=mod)
    g["cov6"] = cov6
    # EWA
    tfx, tfy = ar.k(np.float32(inp["tanfovx"])), ar.k(np.float32(inp["tanfovy"]))
    limx, limy = ar.k(K["lim"]) * tfx, ar.k(K["lim"]) * tfy
    front = ar.val(t[2]) > K["near"]
    tz = ar.where(front, t[2], ar.k(1.0) + t[2] * ar.k(0.0))               # (culled rows stay finite; nothing of them is used)
    txtz, tytz = t[0] / tz, t[1] / tz
    in_x = ~((ar.val(txtz) < -ar.val(limx)) | (ar.val(txtz) > ar.val(limx)))
    in_y = ~((ar.val(tytz) < -ar.val(limy)) | (ar.val(tytz) > ar.val(limy)))
    tx = ar.minimum(limx + txtz * ar.k(0.0), ar.maximum(-limx + txtz * ar.k(0.0), txtz)) * tz
    ty = ar.minimum(limy + tytz * ar.k(0.0), ar.maximum(-limy + tytz * ar.k(0.0), tytz)) * tz
    if freeze is not None:
        tx = ar.where(in_x, tx, ar.arr(freeze[0]))
        ty = ar.where(in_y, ty, ar.arr(freeze[1]))
    fx, fy = ar.k(np.float32(W)) / (ar.k(2.0) * tfx), ar.k(np.float32(H)) / (ar.k(2.0) * tfy)
    j00, j02 = fx / tz, -(fx * tx) / (tz * tz)
    j11, j12 = fy / tz, -(fy * ty) / (tz * tz)
    m0 = [j00 * V[4 * j + 0] + j02 * V[4 * j + 2] for j in range(3)]
    m1 = [j11 * V[4 * j + 1] + j12 * V[4 * j + 2] for j in range(3)]
    c = cov6
    Sm0 = [c[0] * m0[0] + c[1] * m0[1] + c[2] * m0[2], c[1] * m0[0] + c[3] * m0[1] + c[4] * m0[2], c[2] * m0[0] + c[4] * m0[1] + c[5] * m0[2]]
    Sm1 = [c[0] * m1[0] + c[1] * m1[1] + c[2] * m1[2], c[1] * m1[0] + c[3] * m1[1] + c[4] * m1[2], c[2] * m1[0] + c[4] * m1[1] + c[5] * m1[2]]
    a0 = m0[0] * Sm0[0] + m0[1] * Sm0[1] + m0[2] * Sm0[2]
    b = m0[0] * Sm1[0] + m0[1] * Sm1[1] + m0[2] * Sm1[2]
    c0 = m1[0] * Sm1[0] + m1[1] * Sm1[1] + m1[2] * Sm1[2]
    det0 = a0 * c0 - b * b
    a, cc = a0 + ar.k(K["dil"]), c0 + ar.k(K["dil"])
    det = a * cc - b * b
    f = det0 / det
    aa_free = ar.val(f) > K["aa_floor"]
    h = ar.sqrt(ar.maximum(ar.k(K["aa_floor"]) + f * ar.k(0.0), f)) if inp["antialiasing"] else ar.k(1.0) + f * ar.k(0.0)
    opac = ar.arr(np.asarray(inp["opacities"]).reshape(-1))
    if inp["raw"]:                 # (whenever the raw form is set, with a precomputed covariance too: include/gsr.h)
        opac = ar.k(1.0) / (ar.k(1.0) + ar.exp(-opac))
    g.update(front=front, tz=tz, txtz=txtz, tytz=tytz, limx=limx, limy=limy, in_x=in_x, in_y=in_y, tx=tx, ty=ty, fx=fx, fy=fy,
             m0=m0, m1=m1, Sm0=Sm0, Sm1=Sm1, a0=a0, b=b, c0=c0, det0=det0, a=a, c=cc, det=det, f=f, aa_free=aa_free, h=h, opac=opac)
    return g


def _colour(inp, ar, K, g):
    """-> (rgb before the clamp [3], basis list, unit direction, 1/|v|) or the given colours"""
    if inp.get("colors") is not None:
        return [ar.arr(inp["colors"][:, c]) for c in range(3)], None, None, None
    cam = [ar.k(v) for v in np.asarray(inp["campos"], dtype=np.float32).reshape(-1)]
    v = [g["p"][j] - cam[j] for j in range(3)]
    inv = ar.k(1.0) / ar.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    d = [v[j] * inv for j in range(3)]
    deg = int(inp["deg"])
    bs = _sh_basis(ar, K, deg, *d)
    rgb = []
    for c in range(3):
        acc = bs[0] * ar.arr(inp["shs"][:, 0, c])
        for k in range(1, len(bs)):
            acc = acc + bs[k] * ar.arr(inp["shs"][:, k, c])
        rgb.append(acc + ar.k(0.5))
    return rgb, bs, d, inv


# ---------------------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------------------
def forward(inp, dt=np.float64, published=False, freeze=None, yard=None):
    """inp: W, H, tanfovx, tanfovy, viewmatrix [16], projmatrix [16], campos [3], scale_modifier, deg (active), antialiasing,
    depth_z, raw, means3D [P, 3], opacities [P], scales [P, 3] + rotations [P, 4] or cov3D [P, 6], shs [P, M, 3] (band 0 first: the
    dc + shs call form is the same array cut in two) or colors [P, 3] - float32 data.
    -> dict: rec [P, 12] (dt), S [P, 12] (float64 mode), clamp_pre [P, 3] = colours before the clamp, radius_arg ...; in float64
    mode also the discrete values as (lo, hi) pairs: front, in_x, in_y, aa_free, radius, rect [P, 4], visible, open, box [P, 4],
    clamp [P, 3]."""
    ar, K = Arith(dt), consts(published)
    g = _geometry(inp, ar, K, freeze)
    W, H = g["W"], g["H"]
    a, b, c, det = g["a"], g["b"], g["c"], g["det"]
    det_inv = ar.k(1.0) / det
    cA, cB, cC = c * det_inv, -b * det_inv, a * det_inv
    mid = ar.k(0.5) * (a + c)
    root = ar.sqrt(ar.maximum(ar.k(K["lam_floor"]) + mid * ar.k(0.0), mid * mid - det))
    lam = ar.maximum(mid + root, mid - root)
    rarg = ar.k(3.0) * ar.sqrt(lam)
    px = ((g["ndc"][0] + ar.k(1.0)) * ar.k(float(W)) - ar.k(1.0)) * ar.k(0.5)
    py = ((g["ndc"][1] + ar.k(1.0)) * ar.k(float(H)) - ar.k(1.0)) * ar.k(0.5)
    op = g["opac"] * g["h"]
    pos = ar.val(op) > 0.0
    with np.errstate(all="ignore"):
        pmin = ar.where(pos, -ar.log(ar.where(pos, ar.k(255.0) * op, ar.k(1.0) + op * ar.k(0.0))) - ar.k(K["pmargin"]), ar.k(1.0) + op * ar.k(0.0))
    l2 = ar.k(K["log2e"])
    sA, sB, sC, spmin = (ar.k(-0.5) * l2) * cA, -l2 * cB, (ar.k(-0.5) * l2) * cC, l2 * pmin
    rgb_pre, _, _, _ = _colour(inp, ar, K, g)
    zero = ar.k(0.0)
    rgb = [ar.maximum(x, zero + x * zero) for x in rgb_pre] if inp.get("colors") is None else rgb_pre
    tz = g["t"][2]
    dchan = tz if inp["depth_z"] else ar.k(1.0) / g["tz"]
    vals = [px, py, sA, sB, sC, op, spmin, rgb[0], rgb[1], rgb[2], dchan, tz]
    out = dict(rec=np.stack([ar.val(x) for x in vals], axis=1).astype(dt), g=g)
    # the arguments of the discrete values (what the float32 replay's error is measured on)
    q = ar.k(-2.0) * pmin
    qpos = ar.where(ar.val(q) > 0.0, q, zero + q * zero)
    hx = ar.sqrt(qpos * a) * ar.k(K["box_mul"]) + ar.k(K["box_add"])
    hy = ar.sqrt(qpos * c) * ar.k(K["box_mul"]) + ar.k(K["box_add"])
    with np.errstate(all="ignore"):
        radius = np.ceil(ar.val(rarg))
    rr = ar.arr(radius.astype(np.float32)) if not ar.f64 else M(radius)
    T, T1 = ar.k(float(TILE)), ar.k(float(TILE - 1))
    rect_args = [(px - rr) / T, (py - rr) / T, (px + rr + T1) / T, (py + rr + T1) / T]
    box_args = [(px - hx - T1) / T, (py - hy - T1) / T, (px + hx) / T, (py + hy) / T]
    args = dict(arg_tz=[tz], arg_radius=[rarg], arg_rect=rect_args, arg_box=box_args, arg_pmin=[pmin],
                arg_clamp=[g["txtz"], g["tytz"]], arg_aa=[g["f"]])
    out["args"] = {k: np.stack([ar.val(x) for x in v], axis=1) for k, v in args.items()}
    out["rgb_pre"] = np.stack([ar.val(x) for x in rgb_pre], axis=1)
    out["conic"] = np.stack([ar.val(x) for x in (cA, cB, cC)], axis=1)
    out["S_conic"] = np.stack([ar.mag(x) for x in (cA, cB, cC)], axis=1)
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    out["rect_nat"] = np.stack([_tile_clip(out["args"]["arg_rect"][:, j], (gx, gy, gx, gy)[j], K["big"]) for j in range(4)], axis=1)
    rn = out["rect_nat"]
    out["visible_nat"] = g["front"] & (ar.val(det) != 0.0) & ((rn[:, 2] - rn[:, 0]) * (rn[:, 3] - rn[:, 1]) > 0)
    out.update(in_x_nat=g["in_x"], in_y_nat=g["in_y"], aa_free_nat=g["aa_free"], front_nat=g["front"], radius_nat=radius)
    if not ar.f64:
        return out
    out["S"] = np.stack([ar.mag(x) for x in vals], axis=1)
    out["S_args"] = {k: np.stack([ar.mag(x) for x in v], axis=1) for k, v in args.items()}
    out["S_rgb_pre"] = np.stack([ar.mag(x) for x in rgb_pre], axis=1)
    out.update(_discrete(inp, out, K, YARDSTICK if yard is None else yard))
    return out


def _margin(yard, key, S):
    return np.nan_to_num(FACTOR * max(U, yard.get(key, 0.0)) * S, nan=0.0, posinf=1.0e9)


def _tile_clip(v, grid, big):
    with np.errstate(invalid="ignore"):
        return np.clip(np.trunc(np.clip(np.nan_to_num(v, nan=0.0, posinf=big, neginf=-big), -big, big)), 0, grid).astype(np.int64)


def _discrete(inp, o, K, yard):
    """Every discrete value as (lo, hi) from the float64 arguments and their margins"""
    W, H = int(inp["W"]), int(inp["H"])
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    A, S = o["args"], o["S_args"]
    d = {}
    mz = _margin(yard, "arg_tz", S["arg_tz"][:, 0])
    tz = A["arg_tz"][:, 0]
    d["front"] = (tz - mz > K["near"], tz + mz > K["near"])
    tfx, tfy = float(np.float32(inp["tanfovx"])), float(np.float32(inp["tanfovy"]))
    for j, (name, lim) in enumerate((("in_x", K["lim"] * tfx), ("in_y", K["lim"] * tfy))):
        v, m = np.abs(A["arg_clamp"][:, j]), _margin(yard, "arg_clamp", S["arg_clamp"][:, j])
        d[name] = (v < lim - m, v <= lim + m)                                # hit exactly: (False, True)
    f, mf = A["arg_aa"][:, 0], _margin(yard, "arg_aa", S["arg_aa"][:, 0])
    d["aa_free"] = (f - mf > K["aa_floor"], f + mf > K["aa_floor"]) if inp["antialiasing"] else (np.ones_like(f, bool), np.ones_like(f, bool))
    r, mr = A["arg_radius"][:, 0], _margin(yard, "arg_radius", S["arg_radius"][:, 0])
    near_int = np.abs(r - np.round(r)) <= mr
    rlo, rhi = np.where(near_int, np.round(r), np.ceil(r)), np.where(near_int, np.round(r) + 1, np.ceil(r))
    d["radius"] = (rlo.astype(np.int64), rhi.astype(np.int64))
    # 3-sigma rectangle: truncation then clamp, of arguments that fall with the radius (minimum) or rise with it (maximum)
    grid = (gx, gy, gx, gy)
    rect_lo, rect_hi = [], []
    for j in range(4):
        sign = -1.0 if j < 2 else 1.0
        m = _margin(yard, "arg_rect", S["arg_rect"][:, j])
        base = A["arg_rect"][:, j] - sign * o["radius_nat"] / TILE
        v_lo = base + sign * (rlo if sign > 0 else rhi) / TILE - m
        v_hi = base + sign * (rhi if sign > 0 else rlo) / TILE + m
        # (truncation is towards zero, the clamp at 0 absorbs the sign: the map is monotone)
        rect_lo.append(_tile_clip(v_lo, grid[j], K["big"]))
        rect_hi.append(_tile_clip(v_hi, grid[j], K["big"]))
    d["rect"] = (np.stack(rect_lo, axis=1), np.stack(rect_hi, axis=1))
    lo, hi = d["rect"]
    area_min = np.maximum(0, lo[:, 2] - hi[:, 0]) * np.maximum(0, lo[:, 3] - hi[:, 1])
    area_max = np.maximum(0, hi[:, 2] - lo[:, 0]) * np.maximum(0, hi[:, 3] - lo[:, 1])
    det_ok = np.abs(o["g"]["det"].v) > FACTOR * U * o["g"]["det"].m
    d["visible"] = (d["front"][0] & det_ok & (area_min > 0), d["front"][1] & (area_max > 0))
    pm, mp = A["arg_pmin"][:, 0], _margin(yard, "arg_pmin", S["arg_pmin"][:, 0])
    d["open"] = (pm + mp < 0.0, pm - mp < 0.0)                               # the first-stage box exists: q = -2 pmin > 0
    box_lo, box_hi = [], []
    for j in range(4):
        m = _margin(yard, "arg_box", S["arg_box"][:, j])
        v = A["arg_box"][:, j]
        with np.errstate(invalid="ignore"):
            v = np.clip(np.nan_to_num(v, nan=0.0, posinf=K["big"], neginf=-K["big"]), -K["big"], K["big"])
        if j < 2:
            blo, bhi = np.ceil(v - m).astype(np.int64), np.ceil(v + m).astype(np.int64)
            box_lo.append(np.maximum(lo[:, j], blo))
            box_hi.append(np.maximum(hi[:, j], bhi))
        else:
            blo, bhi = np.floor(v - m).astype(np.int64) + 1, np.floor(v + m).astype(np.int64) + 1
            box_lo.append(np.minimum(lo[:, j], blo))
            box_hi.append(np.minimum(hi[:, j], bhi))
    d["box"] = (np.stack(box_lo, axis=1), np.stack(box_hi, axis=1))
    blo, bhi = d["box"]
    d["box_empty"] = (~d["open"][1] | (bhi[:, 2] <= blo[:, 0]) | (bhi[:, 3] <= blo[:, 1]),
                      ~d["open"][0] | (blo[:, 2] <= bhi[:, 0]) | (blo[:, 3] <= bhi[:, 1]))
    if inp.get("colors") is None:
        mc = FACTOR * max(U, yard.get("r", 0.0), yard.get("g", 0.0), yard.get("b", 0.0)) * o["S_rgb_pre"]
        d["clamp"] = (o["rgb_pre"] + mc < 0.0, o["rgb_pre"] - mc <= 0.0)
    else:
        z = np.zeros_like(o["rgb_pre"], dtype=bool)
        d["clamp"] = (z, z)
    return d


DISCRETE = ("front", "in_x", "in_y", "aa_free", "radius", "rect", "visible", "open", "box", "clamp")


def undecided(ref):
    """{discrete value: bool [P]} of a float64 forward"""
    out = {}
    for k in DISCRETE:
        lo, hi = ref[k]
        u = lo != hi
        out[k] = u.any(axis=1) if u.ndim == 2 else u
    return out


def continuous_ok(ref):
    """Gaussians whose continuous values do not depend on an undecided switch (visible for sure, clamp masks and AA switch decided)"""
    u = undecided(ref)
    return ref["visible"][0] & ~u["in_x"] & ~u["in_y"] & ~u["aa_free"] & ~u["front"]


# ---------------------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------------------
def backward(inp, sums, sums_mag=None, clamp_bits=None, active=None, dt=np.float64, published=False, guard_det2=True):
    """sums [P, 10]: the per-Gaussian sums of the gradient records (sum h dx, sum h dy, sum h dx^2, sum h dx dy, sum h dy^2, dL/dop_eff,
    dL/dr, dL/dg, dL/db, dL/d(depth channel)); sums_mag: the sums of the records' magnitudes (their S; default |sums|); clamp_bits [P, 3]
    bool; active [P] bool: Gaussians with instances (the others get zero rows).  guard_det2 = False drops the + 1e-7 of
    1 / (det^2 + 1e-7), which the forward does not have (for finite differences and the oracle's autograd).
    -> dict: grads {name: [P, n] dt}, S {name: [P, n]} (float64), stages {stage: array}, S_stages"""
    ar, K = Arith(dt), consts(published)
    g = _geometry(inp, ar, K)
    W, H = g["W"], g["H"]
    P = np.asarray(inp["means3D"]).shape[0]
    sums = np.asarray(sums)
    mag = np.abs(sums).astype(np.float64) if sums_mag is None else np.asarray(sums_mag, dtype=np.float64)
    acc = [ar.arr(sums[:, j], mag[:, j]) if ar.f64 else sums[:, j].astype(np.float32) for j in range(10)]
    act = np.ones(P, dtype=bool) if active is None else np.asarray(active, dtype=bool)
    zero, one, two, half = ar.k(0.0), ar.k(1.0), ar.k(2.0), ar.k(0.5)
    a, b, c, det, a0, c0, det0 = g["a"], g["b"], g["c"], g["det"], g["a0"], g["c0"], g["det0"]
    opac, h = g["opac"], g["h"]
    aa = bool(inp["antialiasing"])
    op_eff = opac * h if aa else opac
    m = [acc[j] * op_eff for j in range(5)]
    g_op_eff, g_rgb, g_d = acc[5], [acc[6], acc[7], acc[8]], acc[9]
    gA, gB, gC = -half * m[2], -m[3], -half * m[4]
    det_inv = one / det
    cA, cB, cC = c * det_inv, -b * det_inv, a * det_inv
    g_m2d = [(half * ar.k(float(W))) * (-cA * m[0] - cB * m[1]), (half * ar.k(float(H))) * (-cC * m[1] - cB * m[0])]
    det2inv = one / (det * det + ar.k(K["eps"])) if guard_det2 else one / (det * det)
    g_a = det2inv * (-c * c * gA + b * c * gB - b * b * gC)
    g_c = det2inv * (-b * b * gA + a * b * gB - a * a * gC)
    g_b = det2inv * (two * b * c * gA - (det + two * b * b) * gB + two * a * b * gC)
    if aa:
        g_opac = g_op_eff * h
        g_f = (g_op_eff * opac) / (two * h)
        di = one / (det * det)
        free = g["aa_free"]
        g_a = g_a + ar.where(free, g_f * (c0 * det - det0 * c) * di, zero)
        g_c = g_c + ar.where(free, g_f * (a0 * det - det0 * a) * di, zero)
        g_b = g_b + ar.where(free, g_f * (two * b * (det0 - det)) * di, zero)
    else:
        g_opac = g_op_eff
    m0, m1, Sm0, Sm1, V, PV = g["m0"], g["m1"], g["Sm0"], g["Sm1"], g["V"], g["PV"]
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    g_cov6 = []
    for i, j in pairs:
        if i == j:
            g_cov6.append(g_a * m0[i] * m0[i] + g_b * m0[i] * m1[i] + g_c * m1[i] * m1[i])
        else:
            g_cov6.append(two * g_a * m0[i] * m0[j] + g_b * (m0[i] * m1[j] + m0[j] * m1[i]) + two * g_c * m1[i] * m1[j])
    gm0 = [two * g_a * Sm0[j] + g_b * Sm1[j] for j in range(3)]
    gm1 = [two * g_c * Sm1[j] + g_b * Sm0[j] for j in range(3)]
    gJ00 = gm0[0] * V[0] + gm0[1] * V[4] + gm0[2] * V[8]
    gJ02 = gm0[0] * V[2] + gm0[1] * V[6] + gm0[2] * V[10]
    gJ11 = gm1[0] * V[1] + gm1[1] * V[5] + gm1[2] * V[9]
    gJ12 = gm1[0] * V[2] + gm1[1] * V[6] + gm1[2] * V[10]
    fx, fy, tx, ty = g["fx"], g["fy"], g["tx"], g["ty"]
    tz1 = one / g["tz"]
    tz2 = tz1 * tz1
    tz3 = tz2 * tz1
    g_t = [ar.where(g["in_x"], -fx * tz2 * gJ02, zero), ar.where(g["in_y"], -fy * tz2 * gJ12, zero),
           -fx * tz2 * gJ00 - fy * tz2 * gJ11 + two * fx * tx * tz3 * gJ02 + two * fy * ty * tz3 * gJ12]
    g_t[2] = g_t[2] + (g_d if inp["depth_z"] else -g_d * tz2)
    g_mean = [V[4 * j + 0] * g_t[0] + V[4 * j + 1] * g_t[1] + V[4 * j + 2] * g_t[2] for j in range(3)]
    pw, hom = g["pw"], g["hom"]
    mul1, mul2 = hom[0] * pw * pw, hom[1] * pw * pw
    g_mean = [g_mean[j] + (PV[4 * j + 0] * pw - PV[4 * j + 3] * mul1) * g_m2d[0] + (PV[4 * j + 1] * pw - PV[4 * j + 3] * mul2) * g_m2d[1]
              for j in range(3)]
    grads, stages = {}, {}
    # colour
    if inp.get("colors") is not None:
        grads["colors"] = g_rgb
    else:
        cb = np.zeros((P, 3), dtype=bool) if clamp_bits is None else np.asarray(clamp_bits, dtype=bool)
        g_rgb = [ar.where(cb[:, ch], zero, g_rgb[ch]) for ch in range(3)]
        _, bs, d, inv = _colour(inp, ar, K, g)
        Kc = len(bs)
        if Kc > 1:
            db = _sh_basis_grad(ar, K, int(inp["deg"]), *d)
            gd = [zero, zero, zero]
            for k in range(1, Kc):
                qk = (ar.arr(inp["shs"][:, k, 0]) * g_rgb[0] + ar.arr(inp["shs"][:, k, 1]) * g_rgb[1] + ar.arr(inp["shs"][:, k, 2]) * g_rgb[2])
                gd = [gd[j] + db[k - 1][j] * qk for j in range(3)]
            dot = d[0] * gd[0] + d[1] * gd[1] + d[2] * gd[2]
            g_mean = [g_mean[j] + (gd[j] - d[j] * dot) * inv for j in range(3)]
        Mst = np.asarray(inp["shs"]).shape[1]
        grads["shs"] = [(bs[k] * g_rgb[ch] if k < Kc else zero + g_rgb[ch] * zero) for k in range(Mst) for ch in range(3)]
    # Sigma -> scale, rotation
    if inp.get("cov3D") is not None:
        grads["cov3D"] = g_cov6
    else:
        R, sp, mod, s3, q4, qden = g["R"], g["sp"], g["mod"], g["s3"], g["q4"], g["qden"]
        G = [[g_cov6[0], half * g_cov6[1], half * g_cov6[2]], [half * g_cov6[1], g_cov6[3], half * g_cov6[4]],
             [half * g_cov6[2], half * g_cov6[4], g_cov6[5]]]
        gR = [[None] * 3 for _ in range(3)]
        g_scale = []
        for j in range(3):
            gs = zero
            for i in range(3):
                dLij = two * sp[j] * (G[i][0] * R[0][j] + G[i][1] * R[1][j] + G[i][2] * R[2][j])
                gs = gs + dLij * R[i][j]
                gR[i][j] = dLij * sp[j]
            g_scale.append(mod * gs)
        r, x, y, z = q4
        g_rot = [two * (-z * gR[0][1] + y * gR[0][2] + z * gR[1][0] - x * gR[1][2] - y * gR[2][0] + x * gR[2][1]),
                 two * (y * gR[0][1] + z * gR[0][2] + y * gR[1][0] - two * x * gR[1][1] - r * gR[1][2] + z * gR[2][0] + r * gR[2][1] - two * x * gR[2][2]),
                 two * (-two * y * gR[0][0] + x * gR[0][1] + r * gR[0][2] + x * gR[1][0] + z * gR[1][2] - r * gR[2][0] + z * gR[2][1] - two * y * gR[2][2]),
                 two * (-two * z * gR[0][0] - r * gR[0][1] + x * gR[0][2] + r * gR[1][0] - two * z * gR[1][1] + y * gR[1][2] + x * gR[2][0] + y * gR[2][1])]
        if inp["raw"]:
            g_scale = [g_scale[j] * s3[j] for j in range(3)]
            live = ar.val(qden) > K["qeps"]
            dot = ar.where(live, q4[0] * g_rot[0] + q4[1] * g_rot[1] + q4[2] * g_rot[2] + q4[3] * g_rot[3], zero)
            g_rot = [(g_rot[j] - q4[j] * dot) / qden for j in range(4)]
        grads["scales"], grads["rotations"] = g_scale, g_rot
        stages["Sigma->s,q"] = g_scale + g_rot
    if inp["raw"]:                 # (whenever the raw form is set, with a precomputed covariance too: include/gsr.h)
        g_opac = g_opac * (opac * (one - opac))
    grads.update(means2D=g_m2d, means3D=g_mean, opacities=[g_opac])
    stages.update({"conic->cov2D": [g_a, g_b, g_c], "cov2D->Sigma": g_cov6, "cov2D->M": gm0 + gm1, "M->J->t": g_t, "t,NDC->mean": g_mean})

    def pack(xs, f):
        return np.where(act[:, None], np.stack(np.broadcast_arrays(*[f(x) + np.zeros(P) for x in xs]), axis=1), 0.0)
    out = dict(grads={k: pack(v, ar.val).astype(dt) for k, v in grads.items()},
               stages={k: pack(v, ar.val).astype(dt) for k, v in stages.items()})
    if ar.f64:
        out["S"] = {k: pack(v, ar.mag) for k, v in grads.items()}
        out["S_stages"] = {k: pack(v, ar.mag) for k, v in stages.items()}
    return out


def sums_for_cotangent(inp, cot, published=True):
    """The ten sums that carry a cotangent `cot` [P, 10] on the record values (px, py, sA, sB, sC, op, r, g, b, depth channel) into
    the backward (float64): the inverse of the backward's first lines (dL/dconic = -(1/2, 1, 1/2) op_eff x second moments ...)."""
    ar, K = Arith(np.float64), consts(published)
    g = _geometry(inp, ar, K)
    a, b, c = g["a"].v, g["b"].v, g["c"].v
    op_eff = (g["opac"] * g["h"]).v if inp["antialiasing"] else g["opac"].v
    l2 = K["log2e"]
    dA, dB, dC = cot[:, 2] * (-0.5 * l2), cot[:, 3] * (-l2), cot[:, 4] * (-0.5 * l2)
    with np.errstate(all="ignore"):
        s0 = -(a * cot[:, 0] + b * cot[:, 1]) / op_eff
        s1 = -(b * cot[:, 0] + c * cot[:, 1]) / op_eff
        sums = np.stack([s0, s1, -2.0 * dA / op_eff, -dB / op_eff, -2.0 * dC / op_eff, cot[:, 5], cot[:, 6], cot[:, 7], cot[:, 8], cot[:, 9]], axis=1)
    return np.nan_to_num(sums, nan=0.0, posinf=0.0, neginf=0.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# per-row column intervals of the alpha >= 1/255 ellipse inside the box (include/gsr.h "Projection rules"), with a slack
# ---------------------------------------------------------------------------------------------------------------------------------
def row_interval_tiles(rec, rect, shift):
    """Tiles the second stage keeps for one Gaussian: record (float32 [12]) and box (x0, y0, x1, y1), every interval end moved by
    `shift` pixels outwards (> 0) or inwards (< 0).  float64.  The rule and its slacks (1.0001 / 0.01 on the half-height, 1.0002 /
    0.002 on q, 0.01 on the column ends) are the ones include/gsr.h states under "Projection rules"; tests/tile_cull_reference.py has
    no row intervals to reuse.  Restated from the rule, this can differ from the kernel in roundings only: it is used for the
    zero / non-zero assertion alone, and the counts themselves stay with the tile-culling tests."""
    mx, my, As, Bs, Cs, pm = (float(rec[i]) for i in (0, 1, 2, 3, 4, 6))
    A, B, C, q = As * (-2.0 / LOG2E), Bs * (-1.0 / LOG2E), Cs * (-2.0 / LOG2E), pm * (-2.0 / LOG2E)
    det = A * C - B * B
    if not (det > 0.0 and A > 0.0 and C > 0.0 and q > 0.0):
        return 0
    hy = math.sqrt(max(0.0, q * A / det)) * 1.0001 + 0.01 + shift
    qa = q * 1.0002 + 0.002
    kept = 0
    for ty in range(int(rect[1]), int(rect[3])):
        yl = ty * TILE - my
        yh = yl + TILE - 1
        bl, bh = max(yl, -hy), min(yh, hy)
        if bl > bh:
            continue
        yr = -B * math.sqrt(max(0.0, q / C / det))
        y1, y2 = min(bh, max(bl, yr)), min(bh, max(bl, -yr))
        xhi = (-B * y1 + math.sqrt(max(0.0, A * qa - det * y1 * y1))) / A + 0.01 + shift
        xlo = (-B * y2 - math.sqrt(max(0.0, A * qa - det * y2 * y2))) / A - 0.01 - shift
        lo = max(math.ceil(max(-1e9, (mx + xlo - (TILE - 1)) / TILE)), int(rect[0]))
        hi = min(math.floor(min(1e9, (mx + xhi) / TILE)) + 1, int(rect[2]))
        kept += max(0, hi - lo)
    return kept


# ---------------------------------------------------------------------------------------------------------------------------------
# cases and call forms
# ---------------------------------------------------------------------------------------------------------------------------------
TAIL_SIZES = (1, 255, 256, 257, 513)
# Draws of the synthetic per-Gaussian sums per case and form.  The largest of N figures grows with N: the random cases take it over
# 3000 .. 6000 Gaussians, the edge scene - which sets most backward classes - over 254, so one draw there samples a twentieth of what
# the other cases do (its rotations figure, 4.8e-8, was below ONE float32 rounding).  Eight draws bring it to 2000 samples, the
# order of the smallest random case.  The count was fixed once, on the CPU, from this argument.
SUM_SEEDS = tuple(range(5, 13))
EDGE_W, EDGE_H = 100, 52
FORMS = {
    "base": dict(),
    "raw": dict(raw=True),
    "dc": dict(color="dc"),
    "colors": dict(color="colors"),
    "cov": dict(geom="cov"),
    "cov-aa": dict(geom="cov", aa=True),
    "aa": dict(aa=True),
    "raw-aa-mod2.3": dict(raw=True, aa=True, mod=2.3),
    "mod0.5": dict(mod=0.5),
    "raw-mod2.3": dict(raw=True, mod=2.3),
    "z": dict(depth_z=True),
    "raw-aa-z": dict(raw=True, aa=True, depth_z=True),
}


# the edge scene only (stored degree 3): an active degree below the stored one, which the unstaged kernels serve
DEG_FORMS = {"deg0": dict(deg=0), "deg1": dict(deg=1), "deg2": dict(deg=2), "dc-deg0": dict(color="dc", deg=0),
             "dc-deg2": dict(color="dc", deg=2)}


def form_of(name):
    f = dict(color="shs", geom="sr", raw=False, aa=False, mod=1.0, depth_z=False, deg=None)
    f.update({**FORMS, **DEG_FORMS}[name] if isinstance(name, str) else name)
    return f


def case_names():
    import compositing_reference as CR
    return list(CR.CASES) + ["edge"] + [f"tail_{n}" for n in TAIL_SIZES]


def _edge_raw():
    """The hand-built edge scene: identity view (t = mean exactly), 100 x 52 pixels.  -> (RawGaussians-like dict in ACTIVATED space,
    camera).  Rows 0 .. 39 are the specials, the rest ordinary splats in front of the camera."""
    import torch
    from scene_utils import look_at_camera
    cam = look_at_camera((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, -1.0, 0.0), 0.6911, EDGE_W, EDGE_H)
    rng = np.random.default_rng(77)
    n = 260
    z = rng.uniform(1.5, 6.0, n)
    xyz = np.stack([rng.uniform(-0.3, 0.3, n) * z, rng.uniform(-0.15, 0.15, n) * z, z], axis=1)
    s = np.exp(rng.normal(math.log(0.05), 0.5, (n, 3)))
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    o = rng.uniform(0.05, 0.95, n)
    sh = np.concatenate([rng.uniform(-0.5, 0.5, (n, 1, 3)) / SH_C0, 0.05 * rng.normal(size=(n, 15, 3))], axis=1)
    i = 0

    def put(p=None, sc=None, qq=None, oo=None, dc=None):
        nonlocal i
        if p is not None:
            xyz[i] = p
        if sc is not None:
            s[i] = sc
        if qq is not None:
            q[i] = qq
        if oo is not None:
            o[i] = oo
        if dc is not None:
            sh[i, 0] = dc
        i += 1
    f32 = np.float32
    for zz in (0.19, float(f32(0.2)), 0.21, -1.0, 0.1999, 0.2001):         # near plane: below, AT (0.2f exactly), above, behind
        put(p=(0.0, 0.0, zz), sc=(0.01, 0.01, 0.01))
    for p in ((1.2, 0.0, 2.0), (-1.2, 0.1, 2.0), (0.0, 0.7, 2.0), (0.1, -0.7, 2.0), (1.2, 0.7, 2.0), (-1.2, -0.7, 2.0)):
        put(p=p, sc=(0.35, 0.3, 0.32))                                       # beyond the clamp in x, in y, in both: wide enough to show
    for oo in (0.5 / 255.0, float(f32(1.0) / f32(255.0)), 2.0 / 255.0, 0.0, 0.999):
        put(p=(0.1, 0.05, 3.0), sc=(0.1, 0.1, 0.1), oo=oo)                   # opacity below, at, above 1/255; zero; near one
    put(p=(0.0, 0.0, 1.0), sc=(1.0, 1.0, 1.0))                               # radius beyond the image
    put(p=(2.0e8, 0.0, 1.0), sc=(0.05, 0.05, 0.05))                          # far off screen: the +-1e9 guard of the tile index
    put(p=(-2.0e8, 3.0e8, 1.0), sc=(0.05, 0.05, 0.05))
    put(p=(0.2, 0.1, 3.0), sc=(1e-4, 1e-4, 1e-4), qq=(1, 0, 0, 0))           # isotropic, far below a pixel: dilation dominates, AA at its floor
    put(p=(-0.2, 0.1, 3.0), sc=(1e-3, 1e-3, 1e-3), qq=(1, 0, 0, 0))
    put(p=(0.3, -0.2, 4.0), sc=(0.05, 0.1, 0.02), qq=(2.0, 0.5, -1.0, 0.3))  # unnormalised quaternion
    put(p=(-0.3, -0.2, 4.0), sc=(0.05, 0.1, 0.02), qq=(0.1, 0.05, -0.02, 0.03))
    put(p=(0.0, 0.2, 4.0), sc=(0.05, 0.1, 0.02), qq=(1e-13, 0, 0, 0))        # quaternion of norm 1e-13 (raw: below the 1e-12 of normalize)
    put(p=(0.1, 0.2, 4.0), sc=(0.05, 0.1, 0.02), qq=(0, 6e-14, 8e-14, 0))
    e4, em4 = math.exp(4.0), math.exp(-4.0)
    for sc in ((e4, e4, e4), (em4, em4, em4), (em4, 1.0, e4), (e4, em4, 1.0), (1.0, e4, em4)):
        put(p=(0.2, -0.1, 5.0), sc=sc)                                       # scales spanning e^-4 .. e^4
    for dc in ((-0.6 / SH_C0, 0.1, 0.2), (0.3, -0.8 / SH_C0, -0.7 / SH_C0), (-0.5 / SH_C0, 0.0, 0.0), (-3.0, -3.0, -3.0)):
        put(p=(-0.1, 0.1, 2.5), sc=(0.08, 0.08, 0.08), dc=dc)                # a colour channel below 0 (one exactly -0.5 / C0: at 0)
    assert i <= 40
    t = lambda x: torch.from_numpy(np.asarray(x, dtype=np.float32))
    return dict(means3D=t(xyz), scales=t(s), rotations=t(q), opacities=t(o).reshape(-1, 1), shs=t(sh)), cam, 3


def _scene_tensors(name):
    """-> (activated dict, raw dict, camera, stored degree, W, H) of a case, float32 torch tensors"""
    import torch
    if name == "edge":
        act, cam, deg = _edge_raw()
        with np.errstate(all="ignore"):
            raw = dict(scales=torch.log(act["scales"]), rotations=act["rotations"] * 1.0,
                       opacities=torch.log(act["opacities"] / (1.0 - act["opacities"])))
        return act, raw, cam, deg, EDGE_W, EDGE_H
    import compositing_reference as CR
    base = "regular" if name.startswith("tail_") else name
    rawg, cam, deg, W, H, _ = CR.case_scene(base)
    act = {k: v.float() for k, v in rawg.activated().items()}
    raw = dict(scales=rawg.scaling.float(), rotations=rawg.rotation.float(), opacities=rawg.opacity.float())
    if name.startswith("tail_"):
        n = int(name[5:])
        act = {k: v[:n].contiguous() for k, v in act.items()}
        raw = {k: v[:n].contiguous() for k, v in raw.items()}
    return act, raw, cam, deg, W, H


def case_inputs(name, form="base", torch_out=False):
    """The float32 call arguments of case `name` in call form `form` (a FORMS key or a dict).  -> inp dict for forward / backward
    (numpy); with torch_out also the tensors as the C ABI takes them (means3D, dc, shs, colors, opacities, scales, rotations, cov3D)."""
    import torch
    from oracle import gs_oracle as O
    f = form_of(form)
    act, raw, cam, deg, W, H = _scene_tensors(name)
    P = act["means3D"].shape[0]
    t = dict(means3D=act["means3D"].contiguous(), dc=None, shs=None, colors=None, scales=None, rotations=None, cov3D=None)
    use_raw = bool(f["raw"]) and f["geom"] != "cov"
    t["opacities"] = (raw["opacities"] if use_raw else act["opacities"]).reshape(P, 1).contiguous()
    if f["geom"] == "cov":
        # (with the modifier applied, as the reference's own precomputed covariance has it; the kernels ignore scale_modifier here)
        cov = O.cov3d_from_scale_rot(act["scales"].double(), act["rotations"].double(), 1.0)
        t["cov3D"] = torch.nan_to_num(cov.float(), posinf=3.0e38).contiguous()
    else:
        t["scales"] = (raw["scales"] if use_raw else act["scales"]).contiguous()
        t["rotations"] = (raw["rotations"] if use_raw else act["rotations"]).contiguous()
    active_deg = deg if f["deg"] is None else int(f["deg"])
    assert active_deg <= deg
    shs = act["shs"].contiguous()
    if f["color"] == "colors":
        gen = torch.Generator().manual_seed(7)
        t["colors"] = torch.rand(P, 3, generator=gen).contiguous()
    elif f["color"] == "dc":
        t["dc"], t["shs"] = shs[:, :1].contiguous(), shs[:, 1:].contiguous()
    else:
        t["shs"] = shs
    inp = dict(W=W, H=H, tanfovx=np.float32(math.tan(cam.FoVx * 0.5)), tanfovy=np.float32(math.tan(cam.FoVy * 0.5)),
               viewmatrix=cam.world_view_transform.float().numpy().reshape(-1), projmatrix=cam.full_proj_transform.float().numpy().reshape(-1),
               campos=cam.camera_center.float().numpy().reshape(-1), scale_modifier=np.float32(f["mod"]), deg=active_deg,
               antialiasing=bool(f["aa"]), depth_z=bool(f["depth_z"]), raw=use_raw, means3D=t["means3D"].numpy(),
               opacities=t["opacities"].numpy().reshape(-1), scales=None if t["scales"] is None else t["scales"].numpy(),
               rotations=None if t["rotations"] is None else t["rotations"].numpy(),
               cov3D=None if t["cov3D"] is None else t["cov3D"].numpy(),
               shs=None if f["color"] == "colors" else shs.numpy(), colors=None if t["colors"] is None else t["colors"].numpy())
    return (inp, t, cam, f) if torch_out else inp


def synthetic_sums(inp, ref, seed=5):
    """Per-Gaussian gradient records for the CPU yardstick (no compositing here): 1 .. 12 records per Gaussian whose moments have the
    magnitudes of a splat `radius / 3` pixels wide, summed in slot order in float32 and in float64.  The error figures are relative
    to S, so what the records are does not enter the bound - only that there are several and that they cancel.
    -> (sums32 [P, 10] float32, sums64, mag [P, 10])"""
    P = inp["means3D"].shape[0]
    rng = np.random.default_rng(seed)
    sig = np.maximum(ref["radius_nat"], 1.0) / 3.0
    n = rng.integers(1, 13, P)
    s32, s64, mag = np.zeros((P, 10), np.float32), np.zeros((P, 10)), np.zeros((P, 10))
    for k in range(12):
        live = (k < n)[:, None]
        hh = rng.standard_normal((P, 1))
        d = rng.standard_normal((P, 2)) * sig[:, None]
        r = np.concatenate([hh * d[:, :1], hh * d[:, 1:], hh * d[:, :1] ** 2, hh * d[:, :1] * d[:, 1:], hh * d[:, 1:] ** 2, hh,
                            rng.standard_normal((P, 4))], axis=1)
        r = np.where(live, np.nan_to_num(r, posinf=0.0, neginf=0.0), 0.0).astype(np.float32)
        s32 = (s32 + r).astype(np.float32)
        s64 += r.astype(np.float64)
        mag += np.where(live, np.abs(s64), 0.0)                              # (each addition rounds its own partial sum)
    return s32, s64, mag


def slot_order_sums(records, gid, P):
    """records [R, >= 10] float32 by slot, gid [R] = the Gaussian of every slot (contiguous per Gaussian; 0xFFFFFFFF: none).
    -> (sums [P, 10] float64 in slot order, S [P, 10] = the sum of the magnitudes of the partial sums: what a sequential float32
    sum's roundings are relative to)"""
    gid = np.asarray(gid, dtype=np.int64)
    real = gid != 0xFFFFFFFF
    g, r = gid[real], np.asarray(records)[real][:, :10].astype(np.float64)
    sums, mag = np.zeros((P, 10)), np.zeros((P, 10))
    if len(g):
        cs = np.cumsum(r, axis=0)
        first = np.r_[True, g[1:] != g[:-1]]
        start = np.maximum.accumulate(np.where(first, np.arange(len(g)), 0))
        before = np.where(start[:, None] > 0, cs[np.maximum(start - 1, 0)], 0.0)
        part = cs - before
        np.add.at(mag, g, np.abs(part))
        np.add.at(sums, g, r)
    return sums, mag


def slot_order_sums_f32(records, gid, P):
    """The same sums in float32, one addition per record in slot order (what the yardstick replay starts from on real records)"""
    gid = np.asarray(gid, dtype=np.int64)
    real = gid != 0xFFFFFFFF
    sums = np.zeros((P, 10), dtype=np.float32)
    np.add.at(sums, gid[real], np.asarray(records)[real][:, :10].astype(np.float32))     # (unbuffered: sequential per Gaussian)
    return sums


def figures(got, ref, S, rows):
    """largest |got - ref| / S over `rows` (bool [P]); 0 / 0 counts as 0"""
    got, ref, S = (np.asarray(x, dtype=np.float64) for x in (got, ref, S))
    if got.ndim == 1:
        got, ref, S = got[:, None], ref[:, None], S[:, None]
    with np.errstate(all="ignore"):
        e = np.abs(got - ref) / S
    e = np.where(got == ref, 0.0, e)                                       # (exact agreement, whatever S: 0 / 0, a row of zeros)
    e = np.where(np.isnan(e), np.inf, e)
    e = np.where(np.asarray(rows)[:, None], e, 0.0)
    return float(e.max(initial=0.0))


def yardstick_forms(name):
    """The call forms the yardstick scans on a case: every form on the edge scene and the needles, the base form elsewhere"""
    if name == "edge":
        return list(FORMS) + list(DEG_FORMS)
    if name in ("needles", "regular"):
        return list(FORMS)
    return ["base", "raw-aa-mod2.3"]


def yardstick(name, form, verbose=False):
    """One case and form on the CPU: float64 against the float32 replay.  -> {class: figure}, undecided counts, visible count"""
    inp = case_inputs(name, form)
    ref = forward(inp, np.float64, yard={})
    f32 = forward(inp, np.float32)
    g64 = ref["g"]
    same = (ref["visible"][0] & (f32["in_x_nat"] == ref["in_x_nat"]) & (f32["in_y_nat"] == ref["in_y_nat"])
            & (f32["front_nat"] == ref["front_nat"]) & (f32["aa_free_nat"] == ref["aa_free_nat"] if inp["antialiasing"] else True))
    fig = {}
    for j, k in enumerate(RECORD):
        rows = same & ((f32["rgb_pre"][:, j - 7] < 0) == (ref["rgb_pre"][:, j - 7] < 0)) if k in ("r", "g", "b") else same
        fig[k] = figures(f32["rec"][:, j], ref["rec"][:, j], ref["S"][:, j], rows)
    front_same = (f32["front_nat"] == ref["front_nat"]) & ref["front_nat"]
    for k in ARGS:
        rows = front_same if k in ("arg_tz", "arg_clamp") else same
        if k == "arg_tz":
            rows = np.ones_like(same)
        if k in ("arg_rect",):
            rows = same & (f32["radius_nat"] == ref["radius_nat"])
        if k in ("arg_box", "arg_pmin"):
            rows = same & (ref["rec"][:, 5] > 0) & (ref["args"]["arg_pmin"][:, 0] < 0) & (f32["args"]["arg_pmin"][:, 0] < 0)
        fig[k] = figures(f32["args"][k], ref["args"][k], ref["S_args"][k], rows)
    cb = ref["rgb_pre"] < 0
    same_b = same & ((f32["rgb_pre"] < 0) == cb).all(axis=1)
    for seed in SUM_SEEDS:                                                     # (the rounding of a sum of a few records is a draw: several)
        s32, s64, mag = synthetic_sums(inp, ref, seed)
        b64 = backward(inp, s64, mag, cb, same_b, np.float64)
        b32 = backward(inp, s32, None, cb, same_b, np.float32)
        for k in b64["grads"]:
            fig[k] = max(fig.get(k, 0.0), figures(b32["grads"][k], b64["grads"][k], b64["S"][k], same_b))
    if verbose:
        print(f"{name} / {form}: " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    return fig, int(ref["visible"][0].sum())


def yardstick_all(verbose=False):
    worst, where = {}, {}
    for name in case_names():
        for form in yardstick_forms(name):
            fig, _ = yardstick(name, form, verbose)
            for k, v in fig.items():
                if v > worst.get(k, -1.0):
                    worst[k], where[k] = v, f"{name} / {form}"
    return worst, where


def bounds(yard=None):
    yard = YARDSTICK if yard is None else yard
    return {k: max(FLOOR, FACTOR * v) for k, v in yard.items()}


def measure():
    """Reprints the constants of YARDSTICK"""
    worst, where = yardstick_all()
    for k in CLASSES:
        if k in worst:
            print(f'    "{k}": {worst[k]:.4e},   # {where[k]}')


def _rel_l2(b, a, rows):
    d = np.linalg.norm(np.asarray(a)[rows])
    return float(np.linalg.norm((np.asarray(b, dtype=np.float64) - a)[rows]) / d) if d > 0 else 0.0


def stage_table(inp, s32, s64, mag, clamp_bits=None):
    """The float32 replay against the float64 replay, stage by stage, on the sums given (synthetic_sums on the CPU; the kernel's own
    records summed in float32 / float64 in tests/test_projection_replay_gpu.py): the forward intermediates of the covariance chain,
    the backward's cotangents between the stages, the gradients.  Rows: Gaussians surely visible with the same clamp masks in both.
    -> (list of (label, largest S-relative figure, per-tensor rel-L2), number of Gaussians)"""
    ref, f32 = forward(inp, np.float64), forward(inp, np.float32)
    rows = continuous_ok(ref) & (f32["in_x_nat"] == ref["in_x_nat"]) & (f32["in_y_nat"] == ref["in_y_nat"])
    if inp["antialiasing"]:
        rows &= f32["aa_free_nat"] == ref["aa_free_nat"]
    cb = (ref["rgb_pre"] < 0) if clamp_bits is None else np.asarray(clamp_bits, dtype=bool)
    b64 = backward(inp, s64, mag, cb, rows, np.float64)
    b32 = backward(inp, s32, None, cb, rows, np.float32)
    g64, g32 = ref["g"], f32["g"]
    out = []

    def add(label, b, a, S):
        out.append((label, figures(b, a, S, rows), _rel_l2(np.asarray(b, dtype=np.float64).reshape(len(rows), -1),
                                                          np.asarray(a).reshape(len(rows), -1), rows)))
    add("fwd Sigma", np.stack(g32["cov6"], 1), np.stack([x.v for x in g64["cov6"]], 1), np.stack([x.m for x in g64["cov6"]], 1))
    for label, key in (("fwd cov2D a0", "a0"), ("fwd cov2D b", "b"), ("fwd cov2D c0", "c0"), ("fwd det", "det")):
        add(label, g32[key], g64[key].v, g64[key].m)
    add("fwd conic", f32["conic"], ref["conic"], ref["S_conic"])
    for st in STAGES:
        if st in b64["stages"]:
            add("bwd " + st, b32["stages"][st], b64["stages"][st], b64["S_stages"][st])
    for k in GRADS:
        if k in b64["grads"]:
            add("out " + k, b32["grads"][k], b64["grads"][k], b64["S"][k])
    return out, int(rows.sum())


def format_stage_table(table, n, title):
    return [f"   {title} ({n} Gaussians): largest S-relative figure | per-tensor rel-L2"] + \
           [f"     {label:22s} {fig:.2e} | {l2:.2e}" for label, fig, l2 in table]


def profile_text(gpu_log=None):
    """The text of profiles/projection_replay.txt: sections 1, 3 and the synthetic half of 4 from this module alone (CPU); section 2
    and the real-sums half of 4 from the output of `pytest -s tests/test_projection_replay_gpu.py` (gpu_log: its text)."""
    import re
    w = []
    w.append("Projection replay (tests/projection_reference.py profile_text; `python tests/projection_reference.py [pytest -s log]`)")
    w.append("=" * 120)
    w.append("Figures are |value - float64 replay| / S, S = the float64 sum of the magnitudes of the value's terms carried through the stages.")
    w.append("Yardstick = the float32 numpy replay's largest figure over all cases and forms (CPU); bound = max(2^-24, 4 x yardstick).")
    w += ["", "1. yardstick and bound per value class"]
    B = bounds()
    w += [f"   {k:12s} yardstick {YARDSTICK[k]:.4e}   bound {B[k]:.4e}" for k in CLASSES]
    w += ["", "2. the kernels' largest figure per class and case (MI355X; A = forward, B = backward; recorded, not used for any bound)"]
    real = []
    if gpu_log is None:
        w.append("   (no GPU log given)")
    else:
        agg = {}
        for m in re.finditer(r"\[(A|B)[^\]]*\] (\S+) / (\S+): ([^|\n]*)\| ([^\n]*)", gpu_log):
            kind, name, _, head, rest = m.groups()
            if "rel-L2" in head:
                real.append(m.group(0))
                continue
            d = agg.setdefault((kind, name), {})
            for k, v in re.findall(r"(\w+) ([0-9.]+e[+-][0-9]+)", rest):
                d[k] = max(d.get(k, 0.0), float(v))
        w += [f"   {kind} {name:14s} " + " ".join(f"{k} {v:.2e}" for k, v in d.items()) for (kind, name), d in sorted(agg.items())]
    w += ["", "3. undecided discrete values among the surely or possibly visible Gaussians (reference alone; cap 2 % per value)"]
    for name in case_names():
        for form in yardstick_forms(name):
            ref = forward(case_inputs(name, form), np.float64)
            nz = {k: int((u & ref["visible"][1]).sum()) for k, u in undecided(ref).items()}
            nz = {k: v for k, v in nz.items() if v}
            w.append(f"   {name:14s} {form:14s} visible {int(ref['visible'][0].sum()):5d}  "
                     + (" ".join(f"{k} {v}" for k, v in nz.items()) if nz else "none"))
    w += ["", "4. needle scenes, the backward stage by stage: float32 replay against float64 replay",
          "   (a) on SYNTHETIC per-Gaussian sums (synthetic_sums, seed 5; CPU): uncorrelated moments, so the cancellation inside a real",
          "       splat's sums is absent and the rel-L2 magnitudes are NOT those of a rendered frame - only where they rise is"]
    for name in ("needles", "needles_08"):
        inp = case_inputs(name, "base")
        s32, s64, mag = synthetic_sums(inp, forward(inp, np.float64))
        table, n = stage_table(inp, s32, s64, mag)
        w += format_stage_table(table, n, name + " / base, synthetic sums")
    w.append("   (b) on the kernels' OWN gradient records of a rendered frame (MI355X), with the kernels' rel-L2 against the float64 replay")
    if gpu_log is None:
        w.append("       (no GPU log given)")
    else:
        for m in re.finditer(r"\[stage table\] ([^\n]*)\n((?:   [^\n]*\n)+)", gpu_log):
            w += [ln for ln in m.group(2).rstrip("\n").split("\n")]
        w += ["   " + ln for ln in real]
    w.append("   float32 autograd of the oracle against float64 on anisotropic scenes (VERDICT.md): means3D 4.1e-5, scales 4.8e-5, rotations 7.9e-5")
    return "\n".join(w) + "\n"


if __name__ == "__main__":
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), os.path.join(os.path.dirname(here), "gaussian-splatting-slam_amd")]
    sys.stdout.write(profile_text(open(sys.argv[1]).read() if len(sys.argv) > 1 else None))
