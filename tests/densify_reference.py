"""float64 replay of densification (csrc/densify.hip: k_densify_plan, k_densify_apply with its counter-based normal stream,
k_densify_stats).  numpy only, no GPU, nothing imported from the library.  Written from the rules densify.hip states in its header
(reference scene/gaussian_model.py:367-433) and from the stream's integer recipe; held to oracle/densify_oracle.py by
tests/test_densify_reference_cpu.py.

STREAM.  A draw is a function of three integers (seed, source row, stream = copy * 3 + axis):
    a = hash(seed ^ hash(idx * A + stream * B)),  b = hash(a ^ 0x68bc21eb ^ (stream << 8)),  all in uint32
    u1 = ((a >> 8) + 1) / 2^24 in (0, 1],  u2 = (b >> 8) / 2^24 in [0, 1),  z = sqrt(-2 ln u1) cos(2 pi u2).
The two 24-bit integers are exact in any float type, so float64 Box-Muller on them IS the value the kernel approximates.

ARITHMETIC.  float64 (`np.float64`) is the reference.  float32 (`np.float32`) is the YARDSTICK replay: plain numpy in the kernel's
order of operations, every operation rounded on its own, no fused multiply-add; the cosine is cos(pi t), t = 2 u2, evaluated in
float64 and rounded once (the device's cospif works on t, it is not cosf(pi_f * t)).  The error figure of a child position is
|got - float64| / S with S_a = |xyz_a| + sum_b |R_ab| s_b r_b, r_b = sqrt(-2 ln u1) of that draw (not |z_b|: a cosine near zero must
not shrink the scale its own rounding is measured in); of a child scaling |got - float64| / max(1, |value|).  The bound of each is
max(2^-24, 4 x YARDSTICK): the factor 4 covers the hardware's expf / logf / rsqrtf / cospif and summation order, the project's
convention (tests/projection_reference.py).  Nothing here is measured against a kernel.  Both arithmetics use the kernel's float32
constants (1.6f, 0.1f).

DECISIONS (`plan`).  keep / clone / child of every row come as pairs (lo, hi), decided where lo == hi, the pattern of
tests/projection_reference.py's discrete values.  They are evaluated in float64 on the float32 inputs; every predicate carries the
interval its float32 evaluation can land in (u = 2^-24, the unit roundoff; 1 ulp <= 2 u relative, the documented accuracy of the
device's expf and logf):
    g = accum / denom                 one correctly rounded divide: u |g|; none if the float64 quotient is a float32 (then the
                                      divide is exact in any arithmetic); NaN -> 0 is exact
    s_k = expf(scaling_k)             2 u s_k; none at scaling_k = 0 or +-inf (exp is exact there)
    smax = max_k s_k                  exact on the interval ends; NaN if any s_k is NaN (torch.max propagates NaN): such a row is
                                      neither split (smax > T) nor cloned (smax <= T, a comparison of its own), it is kept as it is
    T = percent_dense * extent,       one product of two float32: u T; the torch reference rounds the product of the unrounded
    0.1f * extent                     doubles instead, each within u of its float32: 3 u T covers both; none if both factors and the
                                      product are float32 numbers
    sigmoid = 1 / (1 + expf(-o))      2 u on e = expf(-o) (none at o = 0, +-inf), u on 1 + e, u on the divide, each dropped where the
                                      exact result is a float32 (o = 0: e = 1, 1 + e = 2, 1 / 2 - all exact)
    min_opacity, max_grad             the float32 of the given number; u if the number is not a float32 (the torch reference
                                      compares in float32 as well)
    cmax = expf(logf(smax / 1.6f))    u on the divide, 2 u |L| on L = logf(.) which the exponential turns into 2 u |L| relative,
                                      2 u on expf: (3 + 2 |L|) u relative on top of smax's own interval
All of these are multiplied by (1 + 2^-20) for the second-order terms and float64's own rounding.  A comparison is true for sure
if it holds at both interval ends, false for sure if it fails at both, UNDECIDED otherwise; a NaN operand makes it false for sure, as
in torch.  A flag is decided if it takes one value under every combination of the values its predicates can take.  A case may have
at most UNDECIDED_CAP = 1 % of its rows undecided.

STATISTICS (`stats`, which returns the bound per row).  k_densify_stats forms n = sqrt(fma(gx, gx, gy * gy)) and accum' = accum + n with every
rounding spelled out: the product (u), the fused sum (u) - or two products and an add, (1 + u)^2 either way on gx^2 + gy^2, the
square root halves that to about u and adds its own u, so n = hypot (1 + d), |d| <= 2 u + u^2, and the last add contributes
u |accum + n|:      |accum' - (accum + hypot)| <= u |accum + hypot| + (2 u + 3 u^2) hypot      (no underflow: the test's
gradients keep gx^2, gy^2 normal)."""
import functools

import numpy as np

U = 2.0 ** -24
FLOOR = U
FACTOR = 4.0
UNDECIDED_CAP = 0.01
UB = U * (1.0 + 2.0 ** -20)
HASH_A = 2654435761
HASH_B = 0x9E3779B9
C16 = np.float32(1.6)
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")

# The float32 replay's largest figure over the children (both copies) of every case of `case_names()`
# (measure() reprints them; tests/test_densify_reference_cpu.py recomputes them).
YARDSTICK = {
    "xyz": 7.6580e-07,   # all_split
    "scaling": 2.0894e-07,   # P8192
}


def bounds(yard=None):
    yard = YARDSTICK if yard is None else yard
    return {k: max(FLOOR, FACTOR * v) for k, v in yard.items()}


# ---------------------------------------------------------------------------------------------------------------------------------
# the stream
# ---------------------------------------------------------------------------------------------------------------------------------
def hash_u32(x):
    x = np.array(x, dtype=np.uint32, ndmin=1)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def counter_of(idx, stream):
    """the inner counter idx * A + stream * B (mod 2^32)"""
    idx = np.array(idx, dtype=np.uint32, ndmin=1)
    stream = np.array(stream, dtype=np.uint32, ndmin=1)
    return idx * np.uint32(HASH_A) + stream * np.uint32(HASH_B)


def counter_uniforms(seed, idx, stream):
    """-> the integers (a >> 8) + 1 in [1, 2^24] and b >> 8 in [0, 2^24) of normal_from_counter, as int64"""
    seed = np.uint32(int(seed) & 0xFFFFFFFF)
    stream = np.array(stream, dtype=np.uint32, ndmin=1)
    a = hash_u32(seed ^ hash_u32(counter_of(idx, stream)))
    b = hash_u32(a ^ np.uint32(0x68bc21eb) ^ (stream << np.uint32(8)))
    return (a >> np.uint32(8)).astype(np.int64) + 1, (b >> np.uint32(8)).astype(np.int64)


def normals(seed, idx, stream, dtype=np.float64):
    """Box-Muller on the counter's uniforms -> (z, r), r = sqrt(-2 ln u1)"""
    i1, i2 = counter_uniforms(seed, idx, stream)
    if dtype == np.float64:
        r = np.sqrt(-2.0 * np.log(i1 / 16777216.0))
        return r * np.cos(np.pi * (2.0 * (i2 / 16777216.0))), r
    f = np.float32
    u1 = i1.astype(f) * f(1.0 / 16777216.0)
    u2 = i2.astype(f) * f(1.0 / 16777216.0)
    r = np.sqrt(f(-2.0) * np.log(u1))
    c = np.cos(np.pi * (f(2.0) * u2).astype(np.float64)).astype(f)
    return r * c, r


# ---------------------------------------------------------------------------------------------------------------------------------
# decisions
# ---------------------------------------------------------------------------------------------------------------------------------
def _is_f32(v):
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        return (v.astype(np.float32).astype(np.float64) == v) | np.isnan(v)


def _widen(lo, hi, k, exact=None):
    """the interval [lo, hi] after an operation with relative error k u; untouched where `exact` (default: the interval is one
    float32 number) or where an end is not finite"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    if exact is None:
        exact = (lo == hi) & _is_f32(lo)
    with np.errstate(all="ignore"):
        fin = np.isfinite(lo) & np.isfinite(hi) & ~exact
        k = np.broadcast_to(np.asarray(k, dtype=np.float64), lo.shape)
        wl = np.where(fin, lo - np.where(fin, k, 0.0) * UB * np.abs(np.where(fin, lo, 0.0)), lo)
        wh = np.where(fin, hi + np.where(fin, k, 0.0) * UB * np.abs(np.where(fin, hi, 0.0)), hi)
    return wl, wh


def _number(x):
    """a host number handed to the kernel as a float: (lo, hi) around its float32"""
    v = np.float64(np.float32(x))
    return _widen(v, v, 1.0, exact=np.asarray(_is_f32(np.float64(x))))


def _threshold(c, extent):
    """c * extent as the kernel (float32 product) or the torch reference (product of the doubles, rounded once) form it"""
    c32, e32 = np.float64(np.float32(c)), np.float64(np.float32(extent))
    t = c32 * e32
    exact = _is_f32(t) & _is_f32(np.float64(c)) & _is_f32(np.float64(extent))
    return _widen(t, t, 3.0, exact=np.asarray(exact))


def _gt(a, b):
    """a > b on intervals -> (can be false, can be true); NaN: false for sure"""
    with np.errstate(all="ignore"):
        return ~(a[0] > b[1]), a[1] > b[0]


def _ge(a, b):
    with np.errstate(all="ignore"):
        return ~(a[0] >= b[1]), a[1] >= b[0]


def _lt(a, b):
    with np.errstate(all="ignore"):
        return ~(a[1] < b[0]), a[0] < b[1]


def plan(accum, denom, scaling, opacity, max_grad, min_opacity, extent, max_screen_size, percent_dense):
    """-> dict keep / clone / child = (lo, hi) bool [P] (decided where equal), undecided = bool [P], pred = the five predicates as
    (can be false, can be true)."""
    f8 = lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)       # noqa: E731
    accum, denom, opacity = f8(accum).reshape(-1), f8(denom).reshape(-1), f8(opacity).reshape(-1)
    scaling = f8(scaling).reshape(-1, 3)
    P = accum.shape[0]
    use_ws = bool(max_screen_size)
    with np.errstate(all="ignore"):
        g = accum / denom
        g = np.where(np.isnan(g), 0.0, g)
        g = _widen(g, g, 1.0)
        sel = _ge(g, _number(max_grad))
        s = np.exp(scaling)
        s = _widen(s, s, 2.0, exact=(scaling == 0.0) | ~np.isfinite(scaling))
        smax = (np.max(s[0], axis=1), np.max(s[1], axis=1))                # (np.max propagates NaN)
        nan_smax = np.isnan(smax[0])
        big = _gt(smax, _threshold(percent_dense, extent))
        e = np.exp(-opacity)
        e = _widen(e, e, 2.0, exact=(opacity == 0.0) | ~np.isfinite(opacity))
        d = _widen(1.0 + e[0], 1.0 + e[1], 1.0)
        sg = _widen(1.0 / d[1], 1.0 / d[0], 1.0)
        low = _lt(sg, _number(min_opacity))
        t01 = _threshold(0.1, extent)
        size_self = _gt(smax, t01)
        c = _widen(smax[0] / np.float64(C16), smax[1] / np.float64(C16), 1.0, exact=np.zeros(P, dtype=bool))
        L = np.maximum(np.abs(np.log(c[0])), np.abs(np.log(c[1])))
        c = _widen(c[0], c[1], 2.0 * np.where(np.isfinite(L), L, 0.0) + 2.0, exact=np.zeros(P, dtype=bool))
        size_child = _gt(c, t01)
    preds = dict(sel=sel, big=big, low=low, size_self=size_self, size_child=size_child)
    order = ("sel", "big", "low", "size_self", "size_child")
    lo = {k: np.ones(P, dtype=bool) for k in ("keep", "clone", "child")}
    hi = {k: np.zeros(P, dtype=bool) for k in ("keep", "clone", "child")}
    for combo in range(32):
        v = {k: bool(combo >> j & 1) for j, k in enumerate(order)}
        feas = np.ones(P, dtype=bool)
        for k in order:
            feas &= preds[k][1] if v[k] else preds[k][0]
        # clone asks smax <= T with its own comparison: the negation of smax > T unless smax is NaN, when both are false
        split, clone = v["sel"] and v["big"], (v["sel"] and not v["big"]) & ~nan_smax
        prune_self = v["low"] or (use_ws and v["size_self"])
        prune_child = v["low"] or (use_ws and v["size_child"])
        val = dict(keep=not split and not prune_self, clone=clone & (not prune_self), child=split and not prune_child)
        for k, b in val.items():
            b = np.broadcast_to(np.asarray(b, dtype=bool), (P,))
            hi[k] |= feas & b
            lo[k] &= ~(feas & ~b)
    out = {k: (lo[k], hi[k]) for k in lo}
    out["undecided"] = (lo["keep"] != hi["keep"]) | (lo["clone"] != hi["clone"]) | (lo["child"] != hi["child"])
    out["pred"] = preds
    return out


def plan_of_case(c):
    return plan(c["accum"], c["denom"], c["params"]["scaling"], c["params"]["opacity"], c["max_grad"], c["min_opacity"],
                c["extent"], c["max_screen_size"], c["percent_dense"])


def flags_from_source(P, nk, nc, ns, src):
    """keep / clone / child [P] of a run that returned the counts and the source row of every output row"""
    src = np.asarray(src, dtype=np.int64)
    out = {}
    for k, (a, b) in dict(keep=(0, nk), clone=(nk, nk + nc), child=(nk + nc, nk + nc + ns)).items():
        f = np.zeros(P, dtype=bool)
        f[src[a:b]] = True
        assert int(f.sum()) == b - a                                          # no row twice
        out[k] = f
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# split children
# ---------------------------------------------------------------------------------------------------------------------------------
def _rotation(q, dt, transpose=False):
    """R of the normalised raw quaternion, the kernel's grouping; [n, 3, 3]"""
    q = q.astype(dt)
    n2 = q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3]
    qn = dt(1.0) / np.sqrt(n2)
    r, x, y, z = q[:, 0] * qn, q[:, 1] * qn, q[:, 2] * qn, q[:, 3] * qn
    one, two = dt(1.0), dt(2.0)
    R = np.stack([one - two * (y * y + z * z), two * (x * y - r * z), two * (x * z + r * y),
                  two * (x * y + r * z), one - two * (x * x + z * z), two * (y * z - r * x),
                  two * (x * z - r * y), two * (y * z + r * x), one - two * (x * x + y * y)], axis=1).reshape(-1, 3, 3)
    return R.transpose(0, 2, 1) if transpose else R


def children(params, rows, seed, dtype=np.float64, transpose_R=False):
    """Child xyz and scaling of the source rows `rows` for copies 0 and 1 -> dict xyz, scaling, S: [2, n, 3], z: [2, n, 3].
    S is float64 whatever `dtype` is.  transpose_R = True is the deliberately wrong variant the CPU test proves the bound against."""
    rows = np.asarray(rows, dtype=np.int64)
    dt = np.float64 if dtype == np.float64 else np.float32
    with np.errstate(all="ignore"):
        R = _rotation(params["rotation"][rows], dt, transpose_R)
        s = np.exp(params["scaling"][rows].astype(dt))
        x0 = params["xyz"][rows].astype(dt)
        R8 = np.abs(_rotation(params["rotation"][rows], np.float64))
        s8 = np.exp(params["scaling"][rows].astype(np.float64))
        xyz, S, zs = [], [], []
        for c in range(2):
            zr = [normals(seed, rows, c * 3 + a, dt) for a in range(3)]
            z = np.stack([v[0] for v in zr], axis=1).astype(dt)
            r8 = np.stack([normals(seed, rows, c * 3 + a, np.float64)[1] for a in range(3)], axis=1)
            smp = s * z
            xyz.append(np.stack([R[:, a, 0] * smp[:, 0] + R[:, a, 1] * smp[:, 1] + R[:, a, 2] * smp[:, 2] + x0[:, a]
                                 for a in range(3)], axis=1))
            S.append(np.abs(x0.astype(np.float64)) + np.einsum("nab,nb->na", R8, s8 * r8))
            zs.append(z)
        sc = np.log(s / dt(C16))
    return dict(xyz=np.stack(xyz), scaling=np.stack([sc, sc]), S=np.stack(S), z=np.stack(zs))


def figures(got, ref):
    """largest S-relative figure of child positions and scalings; `got` = dict or (xyz, scaling) arrays [2, n, 3]"""
    gx, gs = (got["xyz"], got["scaling"]) if isinstance(got, dict) else got
    if ref["xyz"].size == 0:
        return dict(xyz=0.0, scaling=0.0)
    with np.errstate(all="ignore"):
        fx = np.abs(np.asarray(gx, dtype=np.float64) - ref["xyz"]) / ref["S"]
        fs = np.abs(np.asarray(gs, dtype=np.float64) - ref["scaling"]) / np.maximum(1.0, np.abs(ref["scaling"]))
    fx, fs = np.where(np.isnan(fx), np.inf, fx), np.where(np.isnan(fs), np.inf, fs)
    return dict(xyz=float(fx.max()), scaling=float(fs.max()))


def within(got, ref, bnd=None):
    """every component of every child inside its bound -> (xyz ok, scaling ok)"""
    bnd = bounds() if bnd is None else bnd
    gx, gs = (got["xyz"], got["scaling"]) if isinstance(got, dict) else got
    with np.errstate(all="ignore"):
        okx = np.abs(np.asarray(gx, dtype=np.float64) - ref["xyz"]) <= bnd["xyz"] * ref["S"]
        oks = np.abs(np.asarray(gs, dtype=np.float64) - ref["scaling"]) <= bnd["scaling"] * np.maximum(1.0, np.abs(ref["scaling"]))
    return bool(okx.all()), bool(oks.all())


# ---------------------------------------------------------------------------------------------------------------------------------
# statistics kernel
# ---------------------------------------------------------------------------------------------------------------------------------
def stats(accum, denom, max_radii, grad, radii):
    """float64 accum + hypot(gx, gy), denom + 1, max(max_radii, radii) on the rows with radii > 0 -> (accum, denom, max_radii, bound)"""
    a, d, m = (np.asarray(v, dtype=np.float64).reshape(-1).copy() for v in (accum, denom, max_radii))
    g = np.asarray(grad, dtype=np.float64)
    vis = np.asarray(radii) > 0
    h = np.hypot(g[:, 0], g[:, 1])
    bound = np.zeros_like(a)
    with np.errstate(all="ignore"):
        a[vis] = a[vis] + h[vis]
        d[vis] += 1.0
        m[vis] = np.maximum(m[vis], np.asarray(radii, dtype=np.float64)[vis])
        bound[vis] = U * np.abs(a[vis]) + (2.0 * U + 3.0 * U * U) * h[vis]
    return a, d, m, bound


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
_P_CASES = {"P1": (1, 0, True), "P255": (255, 3, False), "P256": (256, 0, True), "P257": (257, 3, True),
            "P8192": (8192, 0, False), "P8193": (8193, 3, True)}
EDGE_MAX_GRAD = 2.0 ** -11
# constructed rows of the edges_* cases: (accum, denom, scaling, opacity); percent_dense * extent = 0.125 * 8 = 1 exactly, min_opacity
# 0.5, max_grad 2^-11.  Every one is exact in any arithmetic or far from its thresholds.
_L05, _L12, _L2 = float(np.log(0.5)), float(np.log(1.2)), float(np.log(2.0))
EDGE_ROWS = (
    ("grad == max_grad, 3 * 2^-11 / 3", 3 * EDGE_MAX_GRAD, 3.0, (_L05, -3.0, -2.0), 2.0),
    ("grad == max_grad, 2^-11 / 1", EDGE_MAX_GRAD, 1.0, (-3.0, _L05, -2.0), 2.0),
    ("grad one ulp below max_grad", float(np.nextafter(np.float32(EDGE_MAX_GRAD), np.float32(0))), 1.0, (_L05, -3.0, -2.0), 2.0),
    ("accum > 0, denom = 0: +inf", 1e-3, 0.0, (_L05, -3.0, -2.0), 2.0),
    ("0 / 0 -> 0", 0.0, 0.0, (_L05, -3.0, -2.0), 2.0),
    ("scaling = 0: smax == percent_dense * extent", 1.0, 1.0, (0.0, 0.0, 0.0), 2.0),
    ("one axis 0, the others smaller", 1.0, 1.0, (-1.0, 0.0, -2.0), 2.0),
    ("opacity = 0: sigmoid == min_opacity", 0.0, 1.0, (_L05, -3.0, -2.0), 0.0),
    ("opacity = -0", 1.0, 1.0, (_L05, -3.0, -2.0), -0.0),
    ("opacity = -1: low", 1.0, 1.0, (_L05, -3.0, -2.0), -1.0),
    ("0.1 extent < smax <= 0.16 extent: split, children survive", 1.0, 1.0, (-3.0, _L12, -2.0), 2.0),
    ("smax > 0.16 extent: split, children pruned by size", 1.0, 1.0, (-3.0, -2.0, _L2), 2.0),
    ("split source with low opacity: nothing survives", 1.0, 1.0, (_L2, -2.0, -1.0), -1.0),
)
# what the rules give for those rows, by hand: (keep, clone, child) without / with the world-size prune
EDGE_EXPECT = (
    ((1, 1, 0), (1, 1, 0)), ((1, 1, 0), (1, 1, 0)), ((1, 0, 0), (1, 0, 0)), ((1, 1, 0), (1, 1, 0)), ((1, 0, 0), (1, 0, 0)),
    ((1, 1, 0), (0, 0, 0)), ((1, 1, 0), (0, 0, 0)), ((1, 0, 0), (1, 0, 0)), ((1, 1, 0), (1, 1, 0)), ((0, 0, 0), (0, 0, 0)),
    ((0, 0, 1), (0, 0, 1)), ((0, 0, 1), (0, 0, 0)), ((0, 0, 0), (0, 0, 0)),
)
# rows of the `nonfinite` case that differ from `nonfinite_clean`: (scaling axes set to NaN, opacity or None)
_NAN = float("nan")
BAD_KINDS = (((0,), None), ((1,), None), ((2,), None), ((0, 1), None), ((1, 2), None), ((0, 2), None), ((0, 1, 2), None),
             ((), _NAN), ((), float("inf")), ((), float("-inf")))


def _random(P, deg, moments, seed, args):
    rng = np.random.default_rng(seed)
    f = np.float32
    K = (deg + 1) ** 2 - 1
    d = rng.standard_normal((P, 4))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    params = dict(xyz=rng.uniform(-100.0, 100.0, (P, 3)).astype(f), f_dc=((rng.random((P, 1, 3)) - 0.5) / 0.28209479177387814).astype(f),
                  f_rest=(0.05 * rng.standard_normal((P, K, 3))).astype(f), opacity=(1.5 * rng.standard_normal((P, 1))).astype(f),
                  scaling=(np.log(10.0) * rng.uniform(-2.5, 0.5, (P, 3))).astype(f),
                  rotation=(d * 10.0 ** rng.uniform(-1.0, 1.0, (P, 1))).astype(f))
    params["opacity"][rng.random(P) < 0.15] = -7.0
    accum = (rng.random((P, 1)) * 0.002).astype(f)
    denom = rng.integers(0, 4, (P, 1)).astype(f)
    accum[denom == 0] = 0.0
    c = dict(params=params, accum=accum, denom=denom, max_radii=(rng.random(P) * 50.0).astype(f), deg=deg, P=P,
             max_grad=0.0004, min_opacity=0.005, extent=15.0, max_screen_size=20, percent_dense=0.01, seed=11,
             expect=dict(keep=0, clone=0, split=0), moments=None)
    c.update(args)
    if moments:
        c["moments"] = {n: ((1e-3 * rng.standard_normal(params[n].shape)).astype(f), (1e-6 * rng.random(params[n].shape)).astype(f))
                        for n in NAMES}
    return c


def case_names():
    return ("aniso",) + tuple(_P_CASES) + ("all_split", "all_clone", "none_selected", "edges_none", "edges_zero", "edges_20",
                                           "nonfinite_clean", "nonfinite")


@functools.lru_cache(maxsize=None)
def case(name):
    """One case, built once and read-only: params (six float32 arrays), accum, denom, max_radii, moments (or None), the call's
    arguments, and `expect`: the least number of kept rows, clones and split sources the case is there for."""
    f = np.float32
    if name == "aniso":
        c = _random(4001, 3, True, 101, dict(expect=dict(keep=500, clone=100, split=500)))
    elif name in _P_CASES:
        P, deg, mom = _P_CASES[name]
        # (about a quarter of the rows are split sources whose children survive, two fifths are kept, one in fifteen is cloned)
        c = _random(P, deg, mom, 200 + P, dict(expect=dict(keep=P // 4, clone=P // 30, split=P // 5), seed=P))
        if P == 1:                                              # the one row is a split source whose children survive
            c["params"]["scaling"][:] = f(0.0)
            c["params"]["opacity"][:] = f(2.0)
            c["accum"][:], c["denom"][:] = f(0.01), f(2.0)
            c["expect"] = dict(keep=0, clone=0, split=1)
    elif name == "all_split":
        c = _random(3000, 0, True, 301, dict(max_screen_size=None, seed=0xC0FFEE, expect=dict(keep=0, clone=0, split=3000)))
        c["params"]["scaling"][:, 1] = np.maximum(c["params"]["scaling"][:, 1], f(np.log(0.3)))
        c["params"]["opacity"][:] = np.abs(c["params"]["opacity"]) + f(0.5)
        c["accum"][:], c["denom"][:] = f(0.002) + c["accum"], f(2.0)
    elif name == "all_clone":
        c = _random(3000, 0, False, 302, dict(seed=3, expect=dict(keep=3000, clone=3000, split=0)))
        c["params"]["scaling"][:] = np.minimum(c["params"]["scaling"], f(np.log(0.1)))
        c["params"]["opacity"][:] = np.abs(c["params"]["opacity"]) + f(0.5)
        c["accum"][:], c["denom"][:] = f(0.002) + c["accum"], f(2.0)
    elif name == "none_selected":
        c = _random(3000, 3, True, 303, dict(max_screen_size=None, seed=4, expect=dict(keep=2000, clone=0, split=0)))
        c["accum"][:] = f(0.0)
    elif name.startswith("edges_"):
        mss = {"edges_none": None, "edges_zero": 0, "edges_20": 20}[name]
        c = _random(2000, 0, True, 304, dict(max_grad=EDGE_MAX_GRAD, min_opacity=0.5, extent=8.0, percent_dense=0.125,
                                            max_screen_size=mss, seed=77, expect=dict(keep=200, clone=100, split=20 if mss else 200)))
        c["accum"] *= f(2.0)                                    # (grads around 2^-11 on both sides)
        for i, (_, a, d, s, o) in enumerate(EDGE_ROWS):
            c["accum"][i], c["denom"][i], c["params"]["scaling"][i], c["params"]["opacity"][i] = f(a), f(d), np.asarray(s, dtype=f), f(o)
    elif name in ("nonfinite_clean", "nonfinite"):
        c = _random(3000, 0, True, 305, dict(seed=9, expect=dict(keep=300, clone=100, split=300)))
        bad = np.arange(7, 3000, 23)                            # 131 rows, every block of the plan kernel has some
        c["bad_rows"] = bad
        # selected, the finite axes large: a maximum that drops the NaN axis would split these rows
        c["accum"][bad], c["denom"][bad] = f(0.002), f(1.0)
        c["params"]["scaling"][bad] = f(0.0)
        c["params"]["opacity"][bad] = f(2.0)
        if name == "nonfinite":
            for j, i in enumerate(bad):
                axes, op = BAD_KINDS[j % len(BAD_KINDS)]
                for a in axes:
                    c["params"]["scaling"][i, a] = f(_NAN)
                if op is not None:
                    c["params"]["opacity"][i] = f(op)
    else:
        raise KeyError(name)
    c["name"] = name

    def freeze(v):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, dict):
            for w in v.values():
                freeze(w)
        elif isinstance(v, tuple):
            for w in v:
                freeze(w)
    freeze(c)
    return c


def child_rows(c, p=None):
    """the source rows whose children may survive (plan's hi), in row order"""
    p = plan_of_case(c) if p is None else p
    return np.nonzero(p["child"][1])[0]


def yardstick(name):
    c = case(name)
    rows = child_rows(c)
    ref = children(c["params"], rows, c["seed"], np.float64)
    return figures(children(c["params"], rows, c["seed"], np.float32), ref), rows.shape[0]


def yardstick_all():
    worst = {k: (0.0, None) for k in YARDSTICK}
    for name in case_names():
        fig, _ = yardstick(name)
        for k, v in fig.items():
            if v > worst[k][0]:
                worst[k] = (v, name)
    return worst


def measure():
    """Reprints the constants of YARDSTICK"""
    for k, (v, name) in yardstick_all().items():
        print(f'    "{k}": {v:.4e},   # {name}')


def profile_text(gpu_lines=()):
    """profiles/densify_replay.txt: the yardstick, the bounds, the undecided counts of every case and the figures a GPU run printed"""
    B = bounds()
    w = ["Densification: float64 replay (tests/densify_reference.py) against csrc/densify.hip", "",
         "1. float32 replay against float64 over all cases (CPU): figure = |float32 - float64| / S; bound = max(2^-24, 4 x)"]
    w += [f"   {k:8s} yardstick {YARDSTICK[k]:.4e}   bound {B[k]:.4e}" for k in YARDSTICK]
    w += ["", "2. per case (CPU): rows, child sources, float32 replay figures, undecided rows (cap 1 %)"]
    for name in case_names():
        c = case(name)
        fig, n = yardstick(name)
        u = int(plan_of_case(c)["undecided"].sum())
        w.append(f"   {name:16s} P {c['P']:5d}  child sources {n:5d}  xyz {fig['xyz']:.3e}  scaling {fig['scaling']:.3e}  undecided {u}")
    w += ["", "3. the kernels on the MI355X (lines printed by tests/test_densify_replay_gpu.py)"]
    w += ["   " + ln for ln in gpu_lines]
    return "\n".join(w) + "\n"


if __name__ == "__main__":
    import sys
    if len(sys.argv) > 1:       # the log of pytest -s tests/test_densify_replay_gpu.py -> the text of profiles/densify_replay.txt
        sys.stdout.write(profile_text([ln.lstrip(".F") for ln in open(sys.argv[1]).read().splitlines() if "densify_replay " in ln
                                       and "print(" not in ln]))
    else:
        measure()
