"""What the bounds of the generalized-ICP GPU tests rest on, shown on the CPU for every case those tests use (tests/gicp_reference.py),
and the argument checks of the new calls - each bad argument rejected before the native library is loaded.

Preconditions.  The adjugate inverse of include/gsr.h agrees with numpy.linalg.inv to 1e-12 relative; cond(M) <= 1 / epsilon (M =
Sigma_t + R Sigma_s R^T has eigenvalues in [2 epsilon, 2] - up to the float32 rounding of the twelve covariance entries, each <=
2^-24, which moves the smallest eigenvalue 2 epsilon by at most 6 x 2^-24: the check allows exactly that); cond(J^T W J) <= 1e6.
The estimator's two limits: isotropic covariances give the point-to-point Gauss-Newton step, a source without extent and a flat
target approach the point-to-plane step as epsilon falls."""
import functools
import math

import numpy as np
import pytest
import torch

import gicp_reference as G
import normals_reference as NR
import registration_reference as RR
import scene_utils as S
import simple_knn
from diff_gaussian_rasterization import _C

I6 = np.float32([1, 0, 0, 1, 0, 1])


def cond_M_bound(epsilon):
    return (1.0 / epsilon) * (1.0 + 6.0 * 2.0 ** -24 / (2.0 * epsilon))


@functools.lru_cache(maxsize=None)
def e2e():
    src, scov, tgt, tcov, T, md = G.e2e_case()
    return src, scov, tgt, tcov, T, md, G.icp_generalized(src, scov, tgt, tcov, md)


def nan_case():
    """the NaN rows of tests/test_gicp_update_gpu.py: the matrices that remain are those of update_case(257, 0)"""
    return G.update_case(257, 0.0)


def systems():
    """(name, epsilon, the system of generalized_system) of every update the GPU tests run"""
    for Ps in G.UPDATE_SIZES:
        for offset in G.UPDATE_OFFSETS:
            yield f"update {Ps} {offset}", G.EPSILON, G.generalized_system(*G.update_case(Ps, offset))
    yield "single plane", G.EPSILON, G.generalized_system(*G.single_plane_case())
    src, scov, tgt, tcov, _, _, ref = e2e()
    for k, h in enumerate(ref["history"]):
        yield f"e2e iteration {k}", G.E2E_EPSILON, G.generalized_system(src, scov, tgt, tcov, h["corr"], h["T"])


def test_preconditions_of_every_update_case():
    for name, eps, s in systems():
        assert s["n"] >= 6, name
        inv = np.linalg.inv(s["M"])
        adj = float((np.abs(s["W"] - inv).max(axis=(1, 2)) / np.abs(inv).max(axis=(1, 2))).max())
        cond_M, cond = float(np.linalg.cond(s["M"]).max()), float(np.linalg.cond(s["JTWJ"]))
        print(f"{name}: n={s['n']} adjugate against inv {adj:.3g}, cond(M) {cond_M:.6g}, cond(J^T W J) {cond:.4g}")
        assert adj <= 1e-12, name
        assert cond_M <= cond_M_bound(eps), name
        assert cond <= 1e6, name


def test_the_single_plane_is_solvable_with_isotropic_source_covariances():
    case = G.single_plane_case()
    u = G.generalized_update(*case)
    assert u["status"] == 0 and u["n"] == 300 and u["cond"] <= 1e3
    # M = diag(2, 2, 1 + epsilon): the step closes the 1 / 8 gap along z and nothing else
    want = np.eye(4)
    want[2, 3] = -0.125
    assert np.abs(u["dT"] - want).max() <= 1e-12
    # ... while the plane system of the same pairs is singular
    src, _, tgt, _, corr, T0 = case
    plane = NR.plane_system(src, tgt, np.tile(np.float32([0, 0, 1]), (500, 1)), corr, T0)
    assert np.linalg.matrix_rank(plane["JTJ"]) == 3


def test_the_e2e_reference_run_arrives_where_point_to_point_does_not():
    src, scov, tgt, tcov, T_true, md, ref = e2e()
    assert ref["converged"] and ref["iterations"] <= 10
    err = NR.displacement(ref["T"], T_true, src)
    print(f"e2e: {ref['iterations']} iterations, {err:.3g} from the truth at epsilon = {G.E2E_EPSILON}")
    assert err < 1e-6
    # the neighbour of every query is clear of the runner-up and of the cut-off: the device finds the same correspondences
    assert min(h["margins"][0] for h in ref["history"]) >= 1e-5 and ref["final_margins"][0] >= 1e-5
    # at the default epsilon the fixed point is further out (gicp_reference.E2E_EPSILON says why)
    s3 = G.covariances(src, G.COVARIANCE_RADIUS, 20)["cov"].astype(np.float32)
    t3 = G.covariances(tgt, G.COVARIANCE_RADIUS, 20)["cov"].astype(np.float32)
    far = G.icp_generalized(src, s3, tgt, t3, md)
    assert 1e-6 < NR.displacement(far["T"], T_true, src) < 1e-5


@pytest.mark.parametrize("kind", ["plane", "sphere", "clusters", "duplicates"])
def test_regularize_of_the_sample_covariance_is_the_covariance_of_the_reference_normal(kind):
    pts = NR.cloud(kind, 4097)
    pts[::97] = np.nan
    a = NR.analyse(pts, [(NR.RADIUS, 20)])[0]
    want = G.covariances(pts, NR.RADIUS, 20, analysis=a)
    C, count = G.sample_covariances(pts, NR.RADIUS, 20)
    assert np.array_equal(count, a["count"])
    got = G.regularize(G.six(C))["cov"]
    rows = a["finite"] & (a["count"] >= 3) & (a["gap"] >= NR.GAP)
    assert rows.sum() >= 3000
    # two float64 eigen-solves of matrices equal to rounding: the eigenvector moves by 1e-16 / gap
    assert np.abs(got[rows] - want["cov"][rows]).max() <= 1e-11
    few = a["finite"] & (a["count"] < 3)
    assert few.any() and np.array_equal(want["cov"][few], np.tile(I6.astype(np.float64), (few.sum(), 1)))
    assert np.isnan(want["cov"][~a["finite"]]).all() and (~a["finite"]).sum() == len(pts[::97])
    assert np.abs(want["cov"][rows][:, [0, 3, 5]].sum(axis=1) - (2 + G.EPSILON)).max() <= 1e-12


def test_regularize_rules():
    c = np.float64([[2, 0, 0, 2, 0, 2], [1, 0, 0, 1, 0, 0.25], [np.nan, 0, 0, 1, 0, 1], [4, 0, 0, 1, 0, 9]])
    r = G.regularize(c, 0.5)["cov"]
    assert np.array_equal(r[0], [1, 0, 0, 1, 0, 1]) and np.array_equal(r[1], [1, 0, 0, 1, 0, 0.5]) and np.isnan(r[2]).all()
    assert np.array_equal(r[3], [1, 0, 0, 0.5, 0, 1])


def point_to_point_step(source, target, corr, T):
    """the Gauss-Newton step of sum |dR q' + t - p'|^2 about the documented shift, by least squares on the stacked rows"""
    q = RR.apply_transform(T, source).astype(np.float64)
    use = corr >= 0
    p = np.asarray(target, dtype=np.float64)[np.where(use, corr, 0)]
    c = p[np.flatnonzero(use)[0]]
    q, p = q[use], p[use]
    rows, rhs = [], []
    for a in range(3):
        e = np.zeros(3)
        e[a] = 1.0
        J = np.concatenate([np.cross(q - c, e), np.tile(e, (q.shape[0], 1))], axis=1)      # d/dx of component a: ((q') x e_a, e_a)
        rows.append(J)
        rhs.append(-(q - p)[:, a])
    x = np.linalg.lstsq(np.concatenate(rows), np.concatenate(rhs), rcond=None)[0]
    dT = np.eye(4)
    dT[:3, :3] = NR.rot_zyx(x[0], x[1], x[2])
    dT[:3, 3] = x[3:] + c - dT[:3, :3] @ c
    return dT


@pytest.mark.parametrize("Ps,offset", [(256, 0.0), (257, 1000.0)])
def test_isotropic_covariances_give_the_point_to_point_step(Ps, offset):
    src, _, tgt, _, corr, T0 = G.update_case(Ps, offset)
    u = G.generalized_update(src, np.tile(I6, (Ps, 1)), tgt, np.tile(I6, (tgt.shape[0], 1)), corr, T0)
    want = point_to_point_step(src, tgt, corr, T0)
    assert u["status"] == 0
    assert NR.displacement(u["dT"], want, tgt) <= 1e-11 * float(np.abs(tgt).max())
    # (W = I / 2: d^T W d is half the squared distance)
    assert abs(u["sum_w"] - 0.5 * u["sum_d2"]) <= 1e-12 * u["sum_d2"]


@pytest.mark.parametrize("Ps,offset", [(256, 0.0), (257, 1000.0)])
def test_a_flat_target_and_a_source_without_extent_approach_the_plane_step(Ps, offset):
    """How it is compared: with Sigma_s = 0 the weight is W = Sigma_t^-1 = I + (1 / epsilon - 1) n n^T, so epsilon J^T W J = J^T n
    n^T J + epsilon J^T (I - n n^T) J - the plane system plus epsilon times the in-plane pull.  The generalized step and
    normals_reference.plane_update's therefore differ by O(epsilon): the largest displacement of a target row between the two is
    measured at epsilon = 1e-2 and 1e-4, and must fall at least thirtyfold (a hundredfold is the limit; float32 storage of Sigma_t
    perturbs the weight by 6e-8 / epsilon) and be below a hundredth of a spacing at 1e-4."""
    src, _, tgt, _, corr, T0 = G.update_case(Ps, offset)
    nrm = NR.update_case(Ps, offset)[2]
    plane = NR.plane_update(src, tgt, nrm, corr, T0)
    zero = np.zeros((Ps, 6), np.float32)
    gap = []
    for eps in (1e-2, 1e-4):
        u = G.generalized_update(src, zero, tgt, G.from_normals(nrm, eps).astype(np.float32), corr, T0)
        assert u["status"] == 0 and u["n"] == plane["n"]
        gap.append(NR.displacement(u["dT"], plane["dT"], tgt))
    print(f"Ps={Ps} offset={offset}: generalized against plane step {gap[0]:.3g} at 1e-2, {gap[1]:.3g} at 1e-4")
    assert gap[1] <= gap[0] / 30 and gap[1] <= 0.01 * NR.SPACING


def test_map_gaussians_are_flat_along_their_patch_normal():
    _, _, tgt, _, _, _, _ = e2e()
    q, s, patch = G.map_gaussians(tgt)
    reg = G.regularize(G.gaussian_covariances(q, s).astype(np.float32), G.E2E_EPSILON)
    normals = np.stack([NR._basis(n)[2] for n in NR.SCENE_NORMALS])[patch]
    assert np.nanmin(reg["gap"]) >= 0.99
    assert np.abs(reg["cov"] - G.from_normals(normals, G.E2E_EPSILON)).max() <= 1e-6


# ---- argument checks: every rejection comes before the native library -------------------------------------------------------------------
class OnDevice(torch.Tensor):
    """a tensor that says it lives on the device: what lies behind an is_cuda check is reached without one"""
    is_cuda = True


def dev(t):
    return t.as_subclass(OnDevice)


class LibraryTouched(BaseException):
    pass


def _no_library():
    raise LibraryTouched("the case reached the native library")


P4 = torch.arange(12, dtype=torch.float32).reshape(4, 3) * 0.1
P5 = torch.zeros(5, 3)
D4, D5, D0 = dev(P4), dev(P5), dev(torch.zeros(0, 3))
C4, C5 = torch.zeros(4, 6), torch.zeros(5, 6)
DC4, DC5 = dev(C4), dev(C5)
I4 = torch.zeros(4, dtype=torch.int32)
EYE = torch.eye(4, dtype=torch.float64)
NAN, INF = math.nan, math.inf


class Model:
    def __init__(self, xyz=D5, anchor=None):
        self.get_xyz, self._anchor = xyz, anchor

    def get_covariance(self):
        raise LibraryTouched("the case reached the model's covariances")


GICP = S.registration_generalized_icp
CASES = []


def c(id, exc, fn, *args, **kw):
    CASES.append(pytest.param(exc, fn, args, kw, id=id))


for v, exc in ((True, TypeError), ("1", TypeError), (0, ValueError), (-0.5, ValueError), (NAN, ValueError)):
    c(f"covariances-radius-{v!r}", exc, S.estimate_covariances, P4, v)
    c(f"gicp-radius-{v!r}", exc, GICP, P4, P5, 1.0, covariance_radius=v)
    c(f"scan-radius-{v!r}", exc, S.register_scan_to_map, Model(), P4, 1.0, covariance_radius=v)
for v, exc in ((False, TypeError), (3.0, TypeError), (2, ValueError), (34, ValueError)):
    c(f"covariances-max-nn-{v!r}", exc, S.estimate_covariances, P4, 0.1, v)
    c(f"gicp-max-nn-{v!r}", exc, GICP, P4, P5, 1.0, covariance_radius=0.1, covariance_max_nn=v)
    c(f"scan-max-nn-{v!r}", exc, S.register_scan_to_map, Model(), P4, 1.0, covariance_radius=0.1, covariance_max_nn=v)
for v, exc in ((True, TypeError), ("x", TypeError), (0, ValueError), (0.0, ValueError), (-1e-3, ValueError), (1.5, ValueError),
               (NAN, ValueError), (INF, ValueError)):
    c(f"covariances-epsilon-{v!r}", exc, S.estimate_covariances, P4, 0.1, epsilon=v)
    c(f"regularize-epsilon-{v!r}", exc, S.regularize_covariances, C4, v)
    c(f"gicp-epsilon-{v!r}", exc, GICP, P4, P5, 1.0, covariance_radius=0.1, epsilon=v)
    c(f"scan-epsilon-{v!r}", exc, S.register_scan_to_map, Model(), P4, 1.0, covariance_radius=0.1, epsilon=v)
c("covariances-cpu", _C.GsrError, S.estimate_covariances, P4, 0.1)
c("covariances-shape", ValueError, S.estimate_covariances, dev(torch.zeros(4, 2)), 0.1)
c("covariances-radius-before-device", ValueError, S.estimate_covariances, P4, -1.0)
c("knn-covariances-cpu", _C.GsrError, simple_knn.estimate_covariances, P4, 0.1)
c("knn-covariances-epsilon", ValueError, simple_knn.estimate_covariances, P4, 0.1, epsilon=2.0)
c("knn-regularize-cpu", _C.GsrError, simple_knn.regularize_covariances, C4)
c("regularize-cpu", _C.GsrError, S.regularize_covariances, C4)
c("regularize-shape", ValueError, S.regularize_covariances, dev(torch.zeros(4, 3)))
c("regularize-dim", ValueError, S.regularize_covariances, dev(torch.zeros(4, 3, 3)))
c("regularize-int", ValueError, S.regularize_covariances, dev(torch.zeros(4, 6, dtype=torch.int32)))
c("regularize-list", ValueError, S.regularize_covariances, [[1.0, 0, 0, 1, 0, 1]])
c("update-transformation", ValueError, S.gicp_update, D4, DC4, D5, DC5, I4, torch.eye(3))
c("update-source-cov-rows", ValueError, S.gicp_update, D4, DC5, D5, DC5, I4, EYE)
c("update-target-cov-rows", ValueError, S.gicp_update, D4, DC4, D5, DC4, I4, EYE)
c("update-source-cov-none", ValueError, S.gicp_update, D4, None, D5, DC5, I4, EYE)
c("update-target-cov-width", ValueError, S.gicp_update, D4, DC4, D5, dev(torch.zeros(5, 3)), I4, EYE)
c("update-shapes-before-devices", ValueError, S.gicp_update, D4, C4, D5, DC4, I4, EYE)
c("update-source-cov-cpu", _C.GsrError, S.gicp_update, D4, C4, D5, DC5, I4, EYE)
c("update-target-cov-cpu", _C.GsrError, S.gicp_update, D4, DC4, D5, C5, I4, EYE)
c("update-source-cpu", _C.GsrError, S.gicp_update, P4, DC4, D5, DC5, I4, EYE)
c("update-target-cpu", _C.GsrError, S.gicp_update, D4, DC4, P5, DC5, I4, EYE)
c("update-source-empty", ValueError, S.gicp_update, D0, dev(torch.zeros(0, 6)), D5, DC5, I4[:0], EYE)
c("update-target-empty", ValueError, S.gicp_update, D4, DC4, D0, dev(torch.zeros(0, 6)), I4, EYE)
c("update-correspondences-dtype", ValueError, S.gicp_update, D4, DC4, D5, DC5, I4.long(), EYE)
c("update-correspondences-rows", ValueError, S.gicp_update, D4, DC4, D5, DC5, torch.zeros(5, dtype=torch.int32), EYE)
c("gicp-neither", ValueError, GICP, D4, D5, 1.0)
c("gicp-source-neither", ValueError, GICP, D4, D5, 1.0, target_covariances=DC5)
c("gicp-target-neither", ValueError, GICP, D4, D5, 1.0, source_covariances=DC4)
c("gicp-both", ValueError, GICP, D4, D5, 1.0, source_covariances=DC4, target_covariances=DC5, covariance_radius=0.1)
c("gicp-source-cov-rows", ValueError, GICP, D4, D5, 1.0, source_covariances=DC5, target_covariances=DC5)
c("gicp-target-cov-rows", ValueError, GICP, D4, D5, 1.0, source_covariances=DC4, target_covariances=DC4)
c("gicp-source-cov-cpu", _C.GsrError, GICP, D4, D5, 1.0, source_covariances=C4, target_covariances=DC5)
c("gicp-target-cov-cpu", _C.GsrError, GICP, D4, D5, 1.0, source_covariances=DC4, target_covariances=C5)
c("gicp-distance", ValueError, GICP, D4, D5, -1.0, covariance_radius=0.1)
c("gicp-distance-type", TypeError, GICP, D4, D5, "1", covariance_radius=0.1)
c("gicp-init", ValueError, GICP, D4, D5, 1.0, init=torch.eye(3), covariance_radius=0.1)
c("gicp-index", TypeError, GICP, D4, D5, 1.0, index=5, covariance_radius=0.1)
c("gicp-max-iteration", ValueError, GICP, D4, D5, 1.0, covariance_radius=0.1, max_iteration=0)
c("gicp-check-every", ValueError, GICP, D4, D5, 1.0, covariance_radius=0.1, check_every=-1)
c("gicp-relative-fitness", ValueError, GICP, D4, D5, 1.0, covariance_radius=0.1, relative_fitness=NAN)
c("gicp-relative-rmse", TypeError, GICP, D4, D5, 1.0, covariance_radius=0.1, relative_rmse="x")
c("gicp-source-cpu", _C.GsrError, GICP, P4, D5, 1.0, covariance_radius=0.1)
c("gicp-source-empty", ValueError, GICP, D0, D5, 1.0, covariance_radius=0.1)
c("scan-distance", ValueError, S.register_scan_to_map, Model(), D4, NAN, covariance_radius=0.1)
c("scan-init", ValueError, S.register_scan_to_map, Model(), D4, 1.0, init=torch.eye(2), covariance_radius=0.1)
c("scan-no-radius", ValueError, S.register_scan_to_map, Model(), D4, 1.0)
c("scan-own-source-covariances", TypeError, S.register_scan_to_map, Model(), D4, 1.0, covariance_radius=0.1, source_covariances=DC4)
c("scan-own-target-covariances", TypeError, S.register_scan_to_map, Model(), D4, 1.0, covariance_radius=0.1, target_covariances=DC5)
c("scan-own-index", TypeError, S.register_scan_to_map, Model(), D4, 1.0, covariance_radius=0.1, index=None)
c("scan-max-iteration", ValueError, S.register_scan_to_map, Model(), D4, 1.0, covariance_radius=0.1, max_iteration=0)
c("scan-model-cpu", _C.GsrError, S.register_scan_to_map, Model(P5), D4, 1.0, covariance_radius=0.1)
c("scan-points-cpu", _C.GsrError, S.register_scan_to_map, Model(), P4, 1.0, covariance_radius=0.1)
c("scan-points-shape", ValueError, S.register_scan_to_map, Model(), dev(torch.zeros(4, 2)), 1.0, covariance_radius=0.1)
c("scan-ids-without-anchors", ValueError, S.register_scan_to_map, Model(), D4, 1.0, ids=[0], covariance_radius=0.1)


@pytest.mark.parametrize("exc,fn,args,kw", CASES)
def test_bad_arguments_are_rejected_before_the_library(exc, fn, args, kw):
    saved = _C.lib
    _C.lib = _no_library
    try:
        with pytest.raises(exc) as info:
            fn(*args, **kw)
        assert type(info.value) is exc, info.value      # (LibraryTouched is a BaseException: it passes through pytest.raises)
    finally:
        _C.lib = saved


def test_the_calls_are_exported():
    for name in ("estimate_covariances", "regularize_covariances", "gicp_update", "registration_generalized_icp",
                 "register_scan_to_map"):
        assert callable(getattr(S, name))
    for name in ("estimate_covariances", "regularize_covariances"):
        assert callable(getattr(simple_knn, name)) and name in simple_knn.__all__
    # generalized ICP is its own call: the estimator names of registration_icp are what they were
    assert S.registration.ESTIMATIONS == ("point_to_point", "point_to_plane", "colored")
