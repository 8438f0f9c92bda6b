"""Normals and point-to-plane ICP without a device: the new symbols, argument validation (before any device work, so it can be
seen here), self-checks of the float64 reference (tests/normals_reference.py) and the PRECONDITIONS of the GPU tests' inputs,
shown on the reference alone, for the seeds used and for EVERY row - no row is left out of a GPU comparison on these grounds:
  - membership: the largest included d2 lies more than 1e-5 relative below the smallest excluded one, and r2 more than 1e-5 from
    both - the float32 set is the float64 set.  The clouds' coordinates are multiples of 2^-10 (the lattice's: of 1 / 16), so
    ties are exact in any arithmetic and this holds by construction rather than by the luck of a seed;
  - (l1 - l0) / l2 >= 1e-3 on every row whose normal is compared: at max_nn 30 and 33 and on the lattice that is every row with
    count >= 3; at max_nn 3 and 4 on the other clouds it is the rows that are not thin triangles or two positions stored three
    times (NR.WIDE says why no seed avoids them) - at least 60 % of the rows, all but a few per cent off the duplicates cloud;
    every other check of the GPU test runs on every row there too;
  - cond(J^T J) <= 1e6 about the shift for every update case (the six-row case needed another seed: UPDATE_SEEDS);
  - the end-to-end scene: correspondences unambiguous at every reference iteration of both estimators, the point-to-plane run
    at the true motion within 10 iterations, the point-to-point run not after 30."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import normals_reference as NR
import registration_reference as RR

NEW_SYMBOLS = ("gsr_normals_workspace_bytes", "gsr_estimate_normals", "gsr_icp_update_plane")
MARGIN = 1e-5
GAP = NR.GAP
REACHED = 1e-6          # "at the true motion": every source row within 1e-6 (the scene is 1.5 across, the spacing 2e-2)


def test_new_symbols_resolve_and_the_abi_version_stays():
    from diff_gaussian_rasterization import _C
    raw = ctypes.CDLL(_C.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert hasattr(raw, n) and n in _C.EXPORTS, n
    lib = _C.lib()
    assert lib.gsr_abi_version() == 7
    sizes = [lib.gsr_normals_workspace_bytes(P) for P in (0, 1, 65, 4097, 307200, 1000000)]
    assert all(s > 0 and s % 256 == 0 for s in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert lib.gsr_icp_workspace_bytes(1) == lib.gsr_icp_workspace_bytes(1000000) >= 256 * 30 * 8


def test_entry_points_reject_bad_arguments_before_any_launch():
    from diff_gaussian_rasterization import _C
    lib = _C.lib()
    p = ctypes.c_void_p(4096)      # never dereferenced: every call below fails its argument check
    inf, nan = float("inf"), float("nan")
    e = lib.gsr_estimate_normals
    big = 1 << 40
    view = (ctypes.c_float * 3)(0.0, nan, 0.0)
    for args in ((0, p, 0.1, 30, None, p, None, None, p, big), (1 << 30, p, 0.1, 30, None, p, None, None, p, big),
                 (5, None, 0.1, 30, None, p, None, None, p, big), (5, p, 0.1, 30, None, None, None, None, p, big),
                 (5, p, 0.1, 30, None, p, None, None, None, big), (5, p, 0.0, 30, None, p, None, None, p, big),
                 (5, p, -1.0, 30, None, p, None, None, p, big), (5, p, nan, 30, None, p, None, None, p, big),
                 (5, p, 0.1, 2, None, p, None, None, p, big), (5, p, 0.1, 34, None, p, None, None, p, big),
                 (5, p, inf, 30, view, p, None, None, p, big)):
        assert e(*args, None) == -1, args
    assert e(5, p, inf, 33, None, p, None, None, p, lib.gsr_normals_workspace_bytes(5) - 1, None) == -5
    assert "needed" in _C.last_error()
    u = lib.gsr_icp_update_plane
    ws = lib.gsr_icp_workspace_bytes(5)
    assert u(5, p, 5, p, p, p, p, p, p, ws - 1, None) == -5
    assert u(0, p, 5, p, p, p, p, p, p, ws, None) == -1 and u(5, p, 1 << 30, p, p, p, p, p, p, ws, None) == -1
    for k in range(7):      # source, target, normals, idx, T, stats, workspace
        args = [p] * 7
        args[k] = None
        assert u(5, args[0], 5, args[1], args[2], args[3], args[4], args[5], args[6], ws, None) == -1, k


def test_python_validation_comes_first_and_there_is_no_cpu_path():
    import scene_utils as S
    import simple_knn
    from diff_gaussian_rasterization import _C
    a, b = torch.rand(10, 3), torch.rand(12, 3)
    idx = torch.zeros(10, dtype=torch.int32)
    for call in (lambda: S.estimate_normals(a, radius=0.0), lambda: S.estimate_normals(a, radius=-1.0),
                 lambda: S.estimate_normals(a, radius=float("nan")), lambda: S.estimate_normals(a, max_nn=2),
                 lambda: S.estimate_normals(a, max_nn=34), lambda: S.estimate_normals(a, viewpoint=[0.0, 1.0]),
                 lambda: S.estimate_normals(a, viewpoint=[0.0, float("inf"), 1.0]),
                 lambda: simple_knn.estimate_normals(a, max_nn=1),
                 lambda: S.registration_icp(a, b, 0.5, estimation="plane"),
                 lambda: S.registration_icp(a, b, 0.5, estimation="point_to_plane"),                  # no normals, no radius
                 lambda: S.registration_icp(a, b, 0.5, estimation="point_to_plane", normal_radius=0.0),
                 lambda: S.registration_icp(a, b, 0.5, estimation="point_to_plane", normal_radius=0.1, normal_max_nn=40),
                 lambda: S.registration_icp(a, b, 0.5, estimation="point_to_plane", target_normals=torch.rand(11, 3)),
                 lambda: S.registration_icp(a, b, 0.5, estimation="point_to_plane", target_normals=torch.rand(12, 2)),
                 lambda: S.registration_icp(a, b, 0.5, target_normals=torch.rand(12, 3)),                 # point-to-point takes none
                 lambda: S.registration_icp(a, b, 0.5, estimation="point_to_point", normal_radius=0.2),
                 lambda: S.registration_icp(a, b, 0.5, estimation="point_to_plane", normal_radius=0.2,
                                            target_normals=torch.rand(12, 3)),
                 lambda: S.icp_update(a, b, idx, None, target_normals=torch.rand(10, 3)),
                 lambda: S.icp_update(a, b, idx, None, target_normals=torch.zeros(12, 3, dtype=torch.int32)),
                 lambda: S.register_and_merge(a, None, b, None, estimation="p2p")):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: S.estimate_normals(a, radius="0.1"), lambda: S.estimate_normals(a, max_nn=30.0),
                 lambda: S.estimate_normals(a, radius=True), lambda: S.estimate_normals(a, viewpoint=3.0),
                 lambda: S.registration_icp(a, b, 0.5, estimation=1),
                 lambda: S.registration_icp(a, b, 0.5, estimation="point_to_plane", normal_radius="x"),
                 lambda: S.register_and_merge(a, None, b, None, estimation="point_to_plane", normal_radius=0.3),
                 lambda: S.register_and_merge(a, None, b, None, estimation="point_to_plane", target_normals=b)):
        with pytest.raises(TypeError):
            call()
    for call in (lambda: S.estimate_normals(a), lambda: simple_knn.estimate_normals(a, 0.2, 10, return_stats=True),
                 lambda: S.registration_icp(a, b, 0.5, estimation="point_to_plane", normal_radius=0.2),
                 lambda: S.registration_icp(a, b, 0.5, estimation="point_to_plane", target_normals=torch.rand(12, 3)),
                 lambda: S.icp_update(a, b, idx, None, target_normals=torch.rand(12, 3)),
                 lambda: S.register_and_merge(a, None, b, None, estimation="point_to_plane"),
                 lambda: S.align_map(S.GaussianModel.from_raw(S.make_gaussians(20, 1, seed=1)), b, 0.5,
                                     estimation="point_to_plane", normal_radius=0.2)):
        with pytest.raises(_C.GsrError, match="no CPU path"):
            call()
    assert callable(simple_knn.estimate_normals) and "estimate_normals" in simple_knn.__all__


# ---- the reference itself -----------------------------------------------------------------------------------------------------------
def test_reference_gives_an_exact_plane_its_normal():
    rng = np.random.default_rng(0)
    uv = rng.integers(-64, 64, size=(400, 2)).astype(np.float64) / 32
    pts = np.stack([uv[:, 0], uv[:, 1], 0.5 * uv[:, 0] - 0.25 * uv[:, 1] + 1.0], axis=1).astype(np.float32)      # dyadic: exact
    pts = np.unique(pts, axis=0)
    want = np.array([-0.5, 0.25, 1.0]) / np.linalg.norm([-0.5, 0.25, 1.0])
    for radius, nn in ((NR.INF, 10), (NR.INF, 33), (1.5, 33)):
        n, count, eig = NR.estimate(pts, radius, nn)
        assert (count >= 3).all() and np.abs(n - want).max() < 1e-12 and np.abs(eig[:, 0]).max() < 1e-15
        assert (eig[:, 0] <= eig[:, 1]).all() and (eig[:, 1] <= eig[:, 2]).all()
    towards = NR.estimate(pts, NR.INF, 10, viewpoint=[0.0, 0.0, -50.0])[0]
    assert np.abs(towards + want).max() < 1e-12
    # fewer than three rows, a non-finite row, duplicates
    few = np.array([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0], [0, 0, 0]], dtype=np.float32)
    n, count, eig = NR.estimate(few, NR.INF, 3)
    assert count.tolist() == [3, 3, 0, 3] and np.isnan(n[2]).all() and np.isnan(eig[2]).all()
    n, count, eig = NR.estimate(few[:2], NR.INF, 3)
    assert count.tolist() == [2, 2] and n.tolist() == [[0, 0, 1], [0, 0, 1]] and eig.tolist() == [[0, 0, 0], [0, 0, 0]]


def test_reference_normals_of_a_sphere_are_radial_within_its_curvature():
    pts = NR.sphere_cloud(4096, 99)
    a = NR.analyse(pts, [(NR.RADIUS, 30)])[0]
    body = a["count"] >= 10                                    # (not the planted rows above the shell)
    radial = pts.astype(np.float64) - 0.5
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    cosine = np.abs((a["normal"] * radial).sum(axis=1))[body]
    # a cap of angular radius rho = RADIUS / R, however its rows are spread, tilts the fitted plane by less than rho against the
    # radial direction of any of its points; the noise (0.05 spacings over a cap 5.8 spacings wide) adds a tenth of that at most
    rho = NR.RADIUS / NR.sphere_radius(4096 - 24)
    angle = np.arccos(np.clip(cosine, -1, 1))
    assert body.sum() == 4096 - 24 and angle.max() < rho, (int(body.sum()), float(angle.max()), rho)


def test_reference_plane_update_recovers_a_small_motion_in_two_steps():
    tgt, nrm = NR.three_planes(300, 5, 0.0)
    T = RR.rigid_about(tgt.mean(axis=0), [0.2, -0.4, 0.9], 0.02, [0.004, -0.003, 0.002])
    inv = np.linalg.inv(T)
    src = tgt @ inv[:3, :3].T + inv[:3, 3]
    corr = np.arange(tgt.shape[0])
    u = NR.plane_update(src.astype(np.float32), tgt.astype(np.float32), nrm.astype(np.float32), corr, None)
    u2 = NR.plane_update(src.astype(np.float32), tgt.astype(np.float32), nrm.astype(np.float32), corr, u["T"])
    assert u["status"] == 0 and NR.displacement(u["T"], T, src) < 1e-3 and NR.displacement(u2["T"], T, src) < 1e-6
    R = u["dT"][:3, :3]
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(R) - 1) < 1e-15
    assert NR.plane_update(src[:5].astype(np.float32), tgt.astype(np.float32), nrm.astype(np.float32), corr[:5], None)["status"] == 1


# ---- preconditions --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(NR.CLOUDS))
def test_preconditions_of_the_normal_clouds(kind):
    for P in NR.SIZES:
        pts = NR.cloud(kind, P)
        if kind != "lattice":
            assert np.array_equal(pts.astype(np.float64), np.round(pts.astype(np.float64) / NR.QUANTUM) * NR.QUANTUM)
        else:
            assert np.array_equal(pts.astype(np.float64) * 16, np.round(pts.astype(np.float64) * 16))      # dyadic: exact ties
        for (radius, nn), a in zip(NR.combos(kind), NR.analyse(pts, NR.combos(kind))):
            label = f"{kind} P={P} radius={radius} max_nn={nn}"
            assert NR.set_margin(a) > MARGIN, (label, NR.set_margin(a))
            full = a["count"] >= 3
            with np.errstate(invalid="ignore"):
                compared = full & (a["gap"] >= GAP)
            if nn >= 30 or kind == "lattice":
                assert compared.sum() == full.sum(), (label, np.nanmin(a["gap"]))
            else:
                assert compared.sum() >= (0.6 if kind == "duplicates" else 0.95) * full.sum(), (label, compared.sum(), full.sum())
            if P >= 63 and np.isfinite(radius):                  # the radius leaves rows below max_nn and rows below three
                assert (a["count"] < 3).any() and (nn < 30 or ((a["count"] >= 3) & (a["count"] < nn)).any()), label
            if P == 5000 and kind in ("lattice", "duplicates") and not np.isfinite(radius):
                assert (a["count"] > nn).any(), label            # ties at the bound: more than max_nn members
    if kind == "duplicates":
        pts = NR.cloud(kind, 5000)
        assert np.unique(pts, axis=0).shape[0] == 4500


@pytest.mark.parametrize("offset", [0.0, 1000.0])
@pytest.mark.parametrize("Ps", [6, 256, 257, 65537])
def test_preconditions_of_the_update_cases(Ps, offset):
    src, tgt, nrm, T0, corr = NR.update_case(Ps, offset)
    u = NR.plane_update(src, tgt, nrm, corr, T0)
    assert u["status"] == 0 and u["cond"] <= 1e6 and (Ps == 6 and u["n"] == 6 or 0.5 * Ps < u["n"] <= Ps), (u["n"], u["cond"])


@functools.lru_cache(maxsize=None)
def e2e():
    src, tgt, T, md = NR.e2e_planes()
    a = NR.analyse(tgt, [(NR.E2E_NORMAL_RADIUS, 30)])[0]
    nrm = NR.estimate(tgt, NR.E2E_NORMAL_RADIUS, 30)[0].astype(np.float32)
    plane = NR.icp_plane(src, tgt, nrm, md, max_iteration=30)
    point = RR.icp(src, tgt, md, relative_fitness=0.0, relative_rmse=0.0, max_iteration=30)
    return src, tgt, T, md, a, plane, point


def test_preconditions_of_the_end_to_end_scene():
    src, tgt, T, md, a, plane, point = e2e()
    assert NR.set_margin(a) > MARGIN and (a["count"] >= 3).all() and (a["gap"] >= GAP).all()
    for run in (plane, point):
        ms = [h["margins"] for h in run["history"]] + [run["final_margins"]]
        assert all(m[0] > MARGIN and m[1] > MARGIN for m in ms), min(min(m) for m in ms)
    assert all(h["cond"] <= 1e6 for h in plane["history"])
    # the user-visible gain: point-to-plane is at the motion within 10 iterations, point-to-point is not after 30
    assert plane["converged"] and plane["iterations"] <= 10 and NR.displacement(plane["T"], T, src) < REACHED
    assert point["iterations"] == 30 and NR.displacement(point["T"], T, src) > 1000 * REACHED
    assert plane["fitness"] == 1.0 and point["fitness"] == 1.0
