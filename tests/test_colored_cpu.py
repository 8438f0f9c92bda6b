"""CPU tests of the coloured-ICP work: the float64 restatement of tests/colored_reference.py against closed forms, finite
differences and normals_reference; the preconditions of the new Python functions (raised before anything touches a device); and
the conditions on the clouds and the scene that tests/test_color_gradient_gpu.py and tests/test_icp_colored_gpu.py rely on."""
import functools

import numpy as np
import pytest
import torch

import colored_reference as CR
import normals_reference as NR
import pointcloud_reference as PR
import registration_reference as RR

H = NR.SPACING
Q = NR.QUANTUM


def linear_colors(points, a, b):
    """r = g = b = a.p + b, exact in float32 for coordinates on the quantum and a, b on 1 / 16 - then I = (3 r) / 3 = r exactly"""
    v = np.asarray(points, dtype=np.float64) @ np.asarray(a) + b
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    return np.repeat(v.astype(np.float32)[:, None], 3, axis=1)


# ---- the gradient reference against the closed form ----------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [2, 0])
def test_linear_field_on_a_jittered_plane_gives_the_tangential_part(axis):
    """jitter IN the plane (an exact plane whose unit normal float32 holds exactly): u = delta, b = a.delta = a_t.u, so g = a_t"""
    rng = np.random.default_rng(5)
    gy, gx = np.mgrid[0:24, 0:24]
    uv = np.round((np.stack([gx.ravel(), gy.ravel()], axis=1) + rng.uniform(-0.3, 0.3, size=(576, 2))) * H / Q) * Q
    pts = np.insert(uv, axis, 0.375, axis=1).astype(np.float32)
    n = np.zeros(3)
    n[axis] = 1.0
    a, b = np.array([0.75, -0.5, 1.25]), 0.25
    nrm = np.tile(n.astype(np.float32), (576, 1))
    for radius, nn in ((CR.INF, 4), (2.9 * H, 30), (CR.INF, 33)):
        g = CR.gradient(pts, linear_colors(pts, a, b), nrm, radius, nn)
        assert (g["status"] == 0).all() and (g["count"] >= nn if radius == CR.INF else g["count"] >= 4).all()
        err = np.abs(g["gradient"] - (a - n * (n @ a))).max()
        print(f"plane axis {axis} radius {radius} max_nn {nn}: err {err:.3g}, cond max {g['cond'].max():.3g}")
        assert err <= 1e-10


def test_linear_field_on_a_sphere_patch_gives_the_tangential_part_at_the_pole():
    """Members of a curved patch leave the tangent plane: b = a_t.u + (a.n)(delta.n), and the second term only cancels where the
    neighbourhood is symmetric about the row.  The patch is therefore sampled in mirrored pairs (x, y, z), (-x, -y, z) about
    the pole (equal float32 distances: both members or neither - ties all belong), on the quantum, and the closed form is held
    at the pole, for a field with a component along the pole's normal."""
    rng = np.random.default_rng(6)
    R = 40 * H
    xy = np.round(rng.uniform(-6 * H, 6 * H, size=(300, 2)) / Q) * Q
    xy = xy[(np.abs(xy) > 0).any(axis=1)]
    xy = np.concatenate([xy, -xy, [[0.0, 0.0]]])
    z = np.round((np.sqrt(R * R - (xy ** 2).sum(axis=1)) - R) / Q * 64) * Q / 64
    pts = np.concatenate([xy, z[:, None] + 0.5], axis=1).astype(np.float32)
    pole = pts.shape[0] - 1
    n = np.array([0.0, 0.0, 1.0])
    a, b = np.array([-0.5, 1.0, 0.75]), 0.5
    v = pts.astype(np.float64) @ a + b
    cols = np.repeat(v.astype(np.float32)[:, None], 3, axis=1)
    assert np.array_equal(cols[:, 0].astype(np.float64), v)
    nrm = np.tile(n.astype(np.float32), (pts.shape[0], 1))      # (only the pole's normal is the sphere's; only the pole is held)
    for radius, nn in ((CR.INF, 9), (3 * H, 33), (CR.INF, 33)):
        g = CR.gradient(pts, cols, nrm, radius, nn)
        assert g["status"][pole] == 0 and g["count"][pole] % 2 == 1 and g["count"][pole] >= 9
        err = np.abs(g["gradient"][pole] - (a - n * (n @ a))).max()
        print(f"sphere patch radius {radius} max_nn {nn}: count {g['count'][pole]}, err {err:.3g}")
        assert err <= 1e-10


def test_reference_status_and_masking():
    pts, cols, nrm = CR.gradient_cloud("duplicates")
    cols, nrm, pts = cols.copy(), nrm.copy(), pts.copy()
    cols[3, 1] = np.nan
    nrm[5] = np.inf
    pts[7, 2] = -np.inf
    g = CR.gradient(pts, cols, nrm, NR.RADIUS, 30)
    assert g["status"][[3, 5, 7]].tolist() == [3, 3, 3] and g["count"][[3, 5, 7]].tolist() == [0, 0, 0]
    assert np.isnan(g["gradient"][[3, 5, 7]]).all() and np.isfinite(g["gradient"][g["status"] != 3]).all()
    assert (g["status"] == 1).sum() >= 3 and ((g["status"] == 1) == ((g["count"] < 4) & (g["count"] > 0))).all()
    assert (g["gradient"][g["status"] == 1] == 0).all()
    # a collinear neighbourhood: exact zero pivot
    line = np.stack([np.arange(9) / 8.0, np.zeros(9), np.zeros(9)], axis=1).astype(np.float32)
    g = CR.gradient(line, CR.texture(line, 2.0), np.tile(np.float32([0, 0, 1]), (9, 1)), CR.INF, 5)
    assert (g["status"] == 2).all() and (g["gradient"] == 0).all() and (g["count"] >= 5).all()


# ---- the joint update -------------------------------------------------------------------------------------------------------------------
def test_jacobians_are_the_finite_differences_of_the_residuals():
    src, scol, tgt, nrm, tcol, grd, T0, corr = CR.update_case(257, 0.0)
    for lam in (CR.LAMBDA, 0.5):
        s = CR.colored_system(src, scol, tgt, nrm, tcol, grd, corr, T0, lam)
        assert s["n_rows"] >= 100
        eps = 1e-6
        for k in range(6):
            x = np.zeros(6)
            x[k] = eps
            gp, ip = CR.residuals_at(s, x, lam)
            gm, im = CR.residuals_at(s, -x, lam)
            # central differences of a function whose third derivative is O(extent): eps^2 x that, and 1e-16 / eps of rounding
            assert np.abs((gp - gm) / (2 * eps) - s["JG"][:, k]).max() <= 1e-8 * max(1.0, np.abs(s["JG"]).max())
            assert np.abs((ip - im) / (2 * eps) - s["JI"][:, k]).max() <= 1e-8 * max(1.0, np.abs(s["JI"]).max())
        g0, i0 = CR.residuals_at(s, np.zeros(6), lam)
        assert np.allclose(g0, np.sqrt(lam) * s["rG"], rtol=0, atol=1e-15) and np.allclose(i0, np.sqrt(1 - lam) * s["rI"], rtol=0,
                                                                                           atol=1e-15)


@pytest.mark.parametrize("offset", [0.0, 1000.0])
@pytest.mark.parametrize("Ps", [6, 257])
def test_lambda_one_is_the_plane_update(Ps, offset):
    src, scol, tgt, nrm, tcol, grd, T0, corr = CR.update_case(Ps, offset)
    a = CR.colored_update(src, scol, tgt, nrm, tcol, grd, corr, T0, 1.0)
    b = NR.plane_update(src, tgt, nrm, corr, T0)
    assert a["status"] == b["status"] == 0 and a["n"] == b["n"] and a["sum_ri2"] == 0.0
    assert abs(a["sum_d2"] - b["sum_d2"]) <= 1e-12 * b["sum_d2"] and abs(a["sum_rg2"] - b["sum_r2"]) <= 1e-12 * b["sum_r2"]
    assert NR.displacement(a["T"], b["T"], src) <= 1e-9 * float(np.ptp(tgt.astype(np.float64), axis=0).max())


def test_update_conditions_of_the_gpu_cases():
    """cond(J^T J) of every case of tests/test_icp_colored_gpu.py stays where the plane update's bound was derived (<= 1e6)"""
    for Ps in (6, 256, 257, 65537):
        for offset in (0.0, 1000.0):
            c = CR.update_case(Ps, offset)
            for lam in (CR.LAMBDA, 0.5, 0.0):
                if lam == 0.0 and Ps == 6:
                    continue                                     # (six photometric residuals alone do not fix six unknowns)
                u = CR.colored_update(*c[:6], c[7], c[6], lam)
                print(f"colored update Ps={Ps} offset={offset} lambda={lam}: n={u['n']} cond {u['cond']:.3g}")
                assert u["status"] == 0 and u["cond"] <= 1e6


# ---- the preconditions of the Python surface -----------------------------------------------------------------------------------------
def test_python_validation_comes_first_and_there_is_no_cpu_path():
    import scene_utils as S
    import simple_knn
    from diff_gaussian_rasterization import _C
    a, b = torch.rand(10, 3), torch.rand(12, 3)
    ca, cb, g = torch.rand(10, 3), torch.rand(12, 3), torch.rand(12, 3)
    idx = torch.zeros(10, dtype=torch.int32)
    col = dict(source_colors=ca, target_colors=cb)
    for call in (lambda: S.estimate_color_gradients(a, ca, ca, 0.0), lambda: S.estimate_color_gradients(a, ca, ca, float("nan")),
                 lambda: S.estimate_color_gradients(a, ca, ca, 0.1, max_nn=3), lambda: S.estimate_color_gradients(a, ca, ca, 0.1, 34),
                 lambda: S.estimate_color_gradients(a, ca, torch.rand(9, 3), 0.1), lambda: S.estimate_color_gradients(a, None, ca, 0.1),
                 lambda: simple_knn.estimate_color_gradients(a, ca, torch.rand(10, 2), 0.1),
                 lambda: S.icp_update(a, b, idx, None, target_normals=g, source_colors=ca, target_colors=cb),      # a partial set
                 lambda: S.icp_update(a, b, idx, None, source_colors=ca, target_colors=cb, target_gradients=g),    # no normals
                 lambda: S.icp_update(a, b, idx, None, target_normals=g, target_gradients=g),
                 lambda: S.icp_update(a, b, idx, None, target_normals=g, source_colors=ca, target_colors=cb, target_gradients=g,
                                      lambda_geometric=1.5),
                 lambda: S.icp_update(a, b, idx, None, target_normals=g, source_colors=cb, target_colors=cb, target_gradients=g),
                 lambda: S.registration_icp(a, b, 0.5, estimation="colored", normal_radius=0.2, gradient_radius=0.2),      # no colours
                 lambda: S.registration_icp(a, b, 0.5, estimation="colored", gradient_radius=0.2, **col),                  # no normals
                 lambda: S.registration_icp(a, b, 0.5, estimation="colored", normal_radius=0.2, **col),                    # no gradients
                 lambda: S.registration_icp(a, b, 0.5, estimation="colored", normal_radius=0.2, gradient_radius=0.2,
                                            target_gradients=g, **col),
                 lambda: S.registration_icp(a, b, 0.5, estimation="colored", normal_radius=0.2, gradient_radius=0.2,
                                            gradient_max_nn=3, **col),
                 lambda: S.registration_icp(a, b, 0.5, estimation="colored", normal_radius=0.2, gradient_radius=0.2,
                                            lambda_geometric=-0.1, **col),
                 lambda: S.registration_icp(a, b, 0.5, estimation="colored", normal_radius=0.2, gradient_radius=0.2,
                                            source_colors=ca, target_colors=torch.rand(11, 3)),
                 lambda: S.registration_icp(a, b, 0.5, estimation="point_to_plane", normal_radius=0.2, **col),    # colours unused
                 lambda: S.registration_icp(a, b, 0.5, gradient_radius=0.2),
                 lambda: S.registration_colored_icp(a, ca, b, None, 0.5, normal_radius=0.2, gradient_radius=0.2),
                 lambda: S.registration_multiscale(a, ca, b, cb, [0.2, 0.1], [10]),
                 lambda: S.registration_multiscale(a, ca, b, cb, [], []),
                 lambda: S.registration_multiscale(a, ca, b, cb, [0.2, -0.1], [10, 10]),
                 lambda: S.registration_multiscale(a, ca, b, cb, [0.2], [0]),
                 lambda: S.registration_multiscale(a, None, b, None, [0.2], [10]),                              # coloured by default
                 lambda: S.registration_multiscale(a, ca, b, None, [0.2], [10], estimation="point_to_plane"),
                 lambda: S.registration_multiscale(a, ca, b, cb, [0.2], [10], estimation="p2p"),
                 lambda: S.register_and_merge(a, None, b, None, estimation="colored")):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: S.estimate_color_gradients(a, ca, ca, "0.1"), lambda: S.estimate_color_gradients(a, ca, ca, 0.1, 30.0),
                 lambda: S.registration_icp(a, b, 0.5, estimation="colored", normal_radius=0.2, gradient_radius=0.2,
                                            lambda_geometric="1", **col),
                 lambda: S.registration_colored_icp(a, ca, b, cb, 0.5, estimation="point_to_plane"),
                 lambda: S.registration_multiscale(a, ca, b, cb, 0.2, 10),
                 lambda: S.registration_multiscale(a, ca, b, cb, [0.2], [10.0]),
                 lambda: S.registration_multiscale(a, ca, b, cb, [0.2], [10], normal_radius=0.3),
                 lambda: S.registration_multiscale(a, ca, b, cb, [0.2], [10], max_iteration=3),
                 lambda: S.register_and_merge(a, ca, b, cb, estimation="colored", gradient_radius=0.3),
                 lambda: S.register_and_merge(a, ca, b, cb, estimation="colored", target_normals=g)):
        with pytest.raises(TypeError):
            call()
    for call in (lambda: S.estimate_color_gradients(a, ca, ca, 0.1), lambda: simple_knn.estimate_color_gradients(a, ca, ca, 0.1, 10, True),
                 lambda: S.icp_update(a, b, idx, None, target_normals=g, source_colors=ca, target_colors=cb, target_gradients=g),
                 lambda: S.registration_icp(a, b, 0.5, estimation="colored", normal_radius=0.2, gradient_radius=0.2, **col),
                 lambda: S.registration_colored_icp(a, ca, b, cb, 0.5, target_normals=g, target_gradients=g),
                 lambda: S.registration_multiscale(a, ca, b, cb, [0.2, 0.1], [10, 5]),
                 lambda: S.registration_multiscale(a, None, b, None, [0.2], [10], estimation="point_to_point"),
                 lambda: S.register_and_merge(a, ca, b, cb, estimation="colored")):
        with pytest.raises(_C.GsrError, match="no CPU path"):
            call()
    assert callable(simple_knn.estimate_color_gradients) and "estimate_color_gradients" in simple_knn.__all__
    assert S.registration_colored_icp.__defaults__ == (None, 0.968, 50)      # init, lambda_geometric, max_iteration: Open3D's


def test_c_entry_points_reject_bad_arguments_before_any_launch():
    """status codes alone: nothing is launched for any of these, so no device is needed"""
    from diff_gaussian_rasterization import _C
    lib = _C.lib()
    p = 256      # (a non-NULL address that is never followed)
    g = lib.gsr_color_gradient
    ws = lib.gsr_color_gradient_workspace_bytes(100)
    assert ws > lib.gsr_normals_workspace_bytes(100) and lib.gsr_color_gradient_workspace_bytes(0) > 0
    assert g(100, p, p, p, 0.1, 30, p, None, None, p, ws - 1, None) == -5
    for bad in ((0, 0.1, 30), (1 << 30, 0.1, 30), (100, 0.0, 30), (100, float("nan"), 30), (100, 0.1, 3), (100, 0.1, 34)):
        assert g(bad[0], p, p, p, bad[1], bad[2], p, None, None, p, ws, None) == -1, bad
    for k in range(5):      # points, colors, normals, gradient, workspace
        args = [p] * 5
        args[k] = None
        assert g(100, args[0], args[1], args[2], 0.1, 30, args[3], None, None, args[4], ws, None) == -1, k
    u = lib.gsr_icp_update_colored
    ws = lib.gsr_icp_colored_workspace_bytes(5)
    assert ws > lib.gsr_icp_workspace_bytes(5)
    assert u(5, p, p, 5, p, p, p, p, p, 0.968, p, p, p, ws - 1, None) == -5
    assert u(0, p, p, 5, p, p, p, p, p, 0.968, p, p, p, ws, None) == -1 and u(5, p, p, 1 << 30, p, p, p, p, p, 0.968, p, p, p, ws,
                                                                              None) == -1
    for lam in (-1e-9, 1.0000001, float("nan"), float("inf")):
        assert u(5, p, p, 5, p, p, p, p, p, lam, p, p, p, ws, None) == -1, lam
    for k in range(10):      # source, source_colors, target, normals, target_colors, gradient, idx, T, stats, workspace
        a = [p] * 10
        a[k] = None
        assert u(5, a[0], a[1], 5, a[2], a[3], a[4], a[5], a[6], 0.968, a[7], a[8], a[9], ws, None) == -1, k


# ---- what the GPU tests rely on ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(CR.GRADIENT_SIZES))
def test_gradient_clouds_meet_their_conditions(kind):
    """per (radius, max_nn): float32 membership is the float64 one (what decides it lies more than 1e-6 apart); every row's status
    is far from the pivot threshold (a solved row's smallest pivot ratio is above 1e-9, a rejected row's at or below 1e-15 or
    exactly zero); at most 2 % of the rows have a condition number above 1e8; the radius binds in some cases and not in others"""
    pts, cols, nrm = CR.gradient_cloud(kind)
    assert 257 <= pts.shape[0] <= 4097
    binds = []
    for radius, nn in CR.gradient_combos(kind):
        g = CR.gradient(pts, cols, nrm, radius, nn)
        assert NR.set_margin(g["analysis"]) > 1e-6, (kind, radius, nn)
        st, piv = g["status"], g["pivot"]
        assert (piv[st == 0] > 1e-9).all(), (kind, radius, nn, piv[st == 0].min())
        assert (~(piv[st == 2] > 1e-15)).all(), (kind, radius, nn)
        left_out = (st == 0) & (g["cond"] > CR.KAPPA_MAX)
        print(f"{kind} radius={radius:.4g} max_nn={nn}: status {np.bincount(st, minlength=4).tolist()}, cond median "
              f"{np.median(g['cond'][st == 0]):.3g} max {g['cond'][st == 0].max():.3g}, left out {int(left_out.sum())}")
        assert left_out.sum() <= CR.LEFT_OUT_MAX * pts.shape[0] and (st == 0).sum() >= 0.8 * pts.shape[0]
        binds.append(bool((g["count"][st == 0] < nn).any()))
    assert any(binds) and not all(binds)


@functools.lru_cache(maxsize=None)
def plane_scene_runs():
    src, scol, tgt, tcol, T, md = CR.plane_scene()
    nrm = NR.estimate(tgt, CR.PLANE_RADIUS, 30)[0].astype(np.float32)
    g = CR.gradient(tgt, tcol, nrm, CR.PLANE_RADIUS, 30)
    grd = g["gradient"].astype(np.float32)
    colored = CR.icp_colored(src, scol, tgt, nrm, tcol, grd, md)
    # normals_reference.plane_update has no answer for a singular J^T J (numpy raises); with lambda = 1 the coloured reference IS
    # that update (test_lambda_one_is_the_plane_update) and carries the product's pivot rule
    plane = CR.icp_colored(src, scol, tgt, nrm, tcol, grd, md, lam=1.0, max_iteration=30)
    return src, tgt, T, g, colored, plane


def test_the_scene_separates_coloured_from_point_to_plane():
    src, tgt, T, g, colored, plane = plane_scene_runs()
    assert 55 ** 2 <= tgt.shape[0] <= 65 ** 2 and (g["status"] == 0).all() and NR.set_margin(g["analysis"]) > 1e-6
    start = NR.displacement(np.eye(4), T, src)
    err_c, err_p = NR.displacement(colored["T"], T, src), NR.displacement(plane["T"], T, src)
    print(f"plane scene: start {start / H:.3f} spacings, coloured {colored['iterations']} iterations -> {err_c / H:.4f}, "
          f"point-to-plane {plane['iterations']} iterations (status {[h['status'] for h in plane['history']]}) -> {err_p / H:.3f}")
    assert start > 1.5 * H
    assert colored["converged"] and all(h["status"] == 0 for h in colored["history"]) and err_c <= 0.25 * H
    assert err_p > H


def test_the_scene_through_two_voxel_sizes():
    """registration_multiscale restated: voxel means (tests/pointcloud_reference.py), the reference's normals and gradients at
    2 x voxel, the reference loop per level"""
    src, scol, tgt, tcol, T, _ = CR.plane_scene()
    Tm = np.eye(4)
    for v, n in zip(CR.MULTISCALE_VOXELS, CR.MULTISCALE_ITERATIONS):
        s, t = PR.voxel_down_sample_reference(src, scol, v), PR.voxel_down_sample_reference(tgt, tcol, v)
        sp, sc = s["points"].astype(np.float32), s["colors"].astype(np.float32)
        tp, tc = t["points"].astype(np.float32), t["colors"].astype(np.float32)
        nrm = NR.estimate(tp, 2 * v, 30)[0].astype(np.float32)
        grd = CR.gradient(tp, tc, nrm, 2 * v, 30)["gradient"].astype(np.float32)
        Tm = CR.icp_colored(sp, sc, tp, nrm, tc, grd, v, init=Tm, max_iteration=n)["T"]
        print(f"voxel {v / H:.1f} spacings: {sp.shape[0]} / {tp.shape[0]} rows -> {NR.displacement(Tm, T, src) / H:.4f} spacings")
    assert NR.displacement(Tm, T, src) <= 0.25 * H
    # register_and_merge(estimation="colored") restated: one level at 1.5 spacings, correspondences within five voxel sizes
    v = 1.5 * H
    s, t = PR.voxel_down_sample_reference(src, scol, v), PR.voxel_down_sample_reference(tgt, tcol, v)
    tp, tc = t["points"].astype(np.float32), t["colors"].astype(np.float32)
    nrm = NR.estimate(tp, 2 * v, 30)[0].astype(np.float32)
    grd = CR.gradient(tp, tc, nrm, 2 * v, 30)["gradient"].astype(np.float32)
    res = CR.icp_colored(s["points"].astype(np.float32), s["colors"].astype(np.float32), tp, nrm, tc, grd, 5 * v, max_iteration=30)
    assert res["converged"] and NR.displacement(res["T"], T, src) <= 0.25 * H
