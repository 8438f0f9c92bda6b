"""The inputs of tests/test_gn_updates_pinned_gpu.py: one update each of the point-to-point, point-to-plane and coloured ICP and of
the dense odometry, at the smallest sizes that reach every branch of the code the three 6-unknown updates share (the rows of
partial sums, the stats header, the n < 6 rule, the solve, the shift, `apply`).  numpy only: tests/test_gn_updates_cpu.py checks
on the float64 references that every case has what it is there for, the GPU test runs them on the device.

ICP inputs are handmade, not searched: idx[i] = i % Pt, every 7th row without a partner (-1), and - from eight rows on - one index
beyond the target.  Source = the target rows moved back by a small rigid motion plus seeded noise; random unit normals, random
colours and gradients."""
import functools

import numpy as np

import colored_reference as CR
import normals_reference as NR
import odometry_reference as OR
import registration_reference as RR

# 1: n < 3 and n < 6.  5, 6: n is exactly 5 and exactly 6 (no row of theirs is a 7th one).  9: n = 7, the point update has plenty,
# the 6-unknown system is barely determined.  255 .. 257: one or two workgroups.  65 536, 65 537: the 256-workgroup cap is reached
# and the grid-stride loop takes a second round.
ICP_SIZES = (1, 5, 6, 9, 255, 256, 257, 65536, 65537)
ICP_LAMBDAS = (0.0, 0.5, 0.968, 1.0)
ICP_PT_MAX = 1021
ICP_EXACT_N = {1: 1, 5: 5, 6: 6, 9: 7}
VARIANT_PS = 257                         # the size of the three variants below
ICP_VARIANTS = ("coplanar", "full_T", "offset")
MOTION_AXIS, MOTION_ANGLE, MOTION_SHIFT = (0.3, 0.5, -0.8), 0.02, (0.01, -0.008, 0.006)


@functools.lru_cache(maxsize=None)
def icp_inputs(Ps, variant="plain"):
    """-> dict(src, scol [Ps,3], tgt, nrm, tcol, grd [Pt,3] float32, corr int32 [Ps], T0 float64 [4,4]).  Shared: do not write.
    coplanar: every target row on z = 0.25 with the normal (0, 0, 1) - J^T J has three columns of exact zeros, status 2.
    full_T: a start that has every entry of its first three rows set.  offset: the cloud at +1000, so the shift matters."""
    rng = np.random.default_rng(7100 + Ps + 100000 * (("plain",) + ICP_VARIANTS).index(variant))
    Pt = min(Ps, ICP_PT_MAX)
    tgt = rng.uniform(-1.0, 1.0, size=(Pt, 3))
    nrm = rng.standard_normal((Pt, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    if variant == "coplanar":
        tgt[:, 2] = 0.25
        nrm[:] = (0.0, 0.0, 1.0)
    if variant == "offset":
        tgt += 1000.0
    tgt, nrm = tgt.astype(np.float32), nrm.astype(np.float32)
    tcol = rng.random((Pt, 3), dtype=np.float32)
    grd = (0.5 * rng.standard_normal((Pt, 3))).astype(np.float32)
    scol = rng.random((Ps, 3), dtype=np.float32)
    corr = (np.arange(Ps) % Pt).astype(np.int32)
    inv = np.linalg.inv(RR.rigid_about(tgt.astype(np.float64).mean(axis=0), MOTION_AXIS, MOTION_ANGLE, MOTION_SHIFT))
    T0 = np.eye(4)
    if variant == "full_T":
        T0 = RR.rigid_about((0.2, -0.1, 0.3), (0.2, 0.5, -0.4), 0.3, (0.04, 0.03, -0.05))
        inv = np.linalg.inv(T0) @ inv
    p = tgt[corr].astype(np.float64) + 0.005 * rng.standard_normal((Ps, 3))
    src = (p @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    corr[6::7] = -1
    if Ps > 7:
        corr[7] = Pt + 3                 # a row the target does not have
    return dict(src=src, scol=scol, tgt=tgt, nrm=nrm, tcol=tcol, grd=grd, corr=corr, T0=T0)


def _icp_names():
    names = {}
    for Ps in ICP_SIZES:
        names[f"icp_point_{Ps}"] = ("point", Ps, "plain", None)
        names[f"icp_plane_{Ps}"] = ("plane", Ps, "plain", None)
        for lam in ICP_LAMBDAS:
            names[f"icp_colored_{Ps}_lambda{lam}"] = ("colored", Ps, "plain", lam)
    for v in ICP_VARIANTS:
        names[f"icp_point_{v}"] = ("point", VARIANT_PS, v, None)
        names[f"icp_plane_{v}"] = ("plane", VARIANT_PS, v, None)
        # (the coplanar target at lambda = 1: the plane update's system, so status 2 as well; any colour term would fix the rest)
        names[f"icp_colored_{v}"] = ("colored", VARIANT_PS, v, 1.0 if v == "coplanar" else CR.LAMBDA)
    return names


ICP_CASES = _icp_names()                 # name -> (estimator, Ps, variant, lambda or None)


def icp_reference(name):
    """the float64 reference's result of one ICP case (status, n, cond where the estimator has one)"""
    est, Ps, variant, lam = ICP_CASES[name]
    a = icp_inputs(Ps, variant)
    if est == "point":                   # (RR.update knows -1 only: an index beyond the target is no partner either)
        corr = np.where(a["corr"] < a["tgt"].shape[0], a["corr"], -1)
        return RR.update(a["src"], a["tgt"], corr, a["T0"])
    if est == "plane" and variant != "coplanar":
        return NR.plane_update(a["src"], a["tgt"], a["nrm"], a["corr"], a["T0"])
    if est == "plane":                   # (NR.plane_update has no pivot rule: the coloured reference at lambda = 1 is the same system)
        lam = 1.0
    return CR.colored_update(a["src"], a["scol"], a["tgt"], a["nrm"], a["tcol"], a["grd"], a["corr"], a["T0"], lam)


def icp_expected_status(name):
    est, Ps, variant, _ = ICP_CASES[name]
    n = ICP_EXACT_N.get(Ps, 6)
    if n < (3 if est == "point" else 6):
        return 1
    return 2 if variant == "coplanar" and est != "point" else 0


# ---- odometry: every update case of tests/odometry_reference.py, and two levels of its scene that those sizes leave out --------------
EXTRA_LEVELS = {"size_1x1": (1, 1, 1), "size_16x16": (16, 16, 0)}      # name -> (w, h, status); 16 x 16: one workgroup exactly


@functools.lru_cache(maxsize=None)
def odometry_case(name):
    if name in EXTRA_LEVELS:
        w, h, status = EXTRA_LEVELS[name]
        c = OR._planes(w, h, OR.SMALL_MOTION)
        c.update(T=np.eye(4), depth_diff_max=0.03, status=status, lambdas=OR.UPDATE_LAMBDAS)
        return c
    return OR.update_case(name)


ODOMETRY_CASES = {f"odometry_{name}_lambda{lam}_{'apply' if apply else 'keep'}": (name, lam, apply)
                  for name in OR.UPDATE_CASES + tuple(EXTRA_LEVELS)
                  for lam in odometry_case(name)["lambdas"] for apply in (True, False)}

NAMES = tuple(ICP_CASES) + tuple(ODOMETRY_CASES)


# ---- what the fixture remembers of the inputs ---------------------------------------------------------------------------------------
def checksum(a):
    """float64 sum of the finite entries of an array (the odometry planes hold NaN on purpose)"""
    a = np.asarray(a, dtype=np.float64)
    return float(np.where(np.isfinite(a), a, 0.0).sum())


def input_checksums():
    """{key: float64} over every input array of every case"""
    out = {}
    for Ps, variant in sorted({(c[1], c[2]) for c in ICP_CASES.values()}):
        for k, v in icp_inputs(Ps, variant).items():
            out[f"sum_icp_{Ps}_{variant}_{k}"] = checksum(v)
    for name in sorted({c[0] for c in ODOMETRY_CASES.values()}):
        c = odometry_case(name)
        for k in ("K", "src_I", "src_D", "tgt_I", "tgt_D", "tgt_grad", "T"):
            out[f"sum_odometry_{name}_{k}"] = checksum(c[k])
    return out
