"""Dense RGB-D odometry without a GPU: the float64 reference of tests/odometry_reference.py on its own, the preconditions of every
case the GPU tests run, and the host-side code of scene_utils.odometry (validation, camera_after_odometry).

E_ref.  The reference, from the identity, on corner_scene at 160 x 120 over three levels (20, 10, 5 iterations; motion 1.5 deg and
4.4 cm, 5.47 cm as the largest displacement of an unprojected source pixel) ends 9.05e-4 m from the true motion by the same
measure (printed by test_reference_converges_on_the_corner_scene).  What is left is the bias of
nearest-pixel association and of Sobel gradients on a 160 x 120 grid, not iteration count: level 0 starts 1.07e-2 m away."""
import math

import numpy as np
import pytest
import torch

import odometry_reference as OR
import scene_utils as S
from scene_utils import odometry as O


def test_reference_converges_on_the_corner_scene():
    e = OR.e2e()
    ref = e["ref"]
    print(f"corner_scene {OR.E2E_W} x {OR.E2E_H}, levels {OR.E2E_ITERATIONS}: start {e['start']:.4e} m, E_ref = {e['error']:.4e} m, "
          f"fitness {ref['fitness']:.4f}, rmse {ref['rmse']:.3e}")
    rot = math.degrees(math.acos((np.trace(e["T_true"][:3, :3]) - 1) / 2))
    assert 1.0 <= rot <= 2.0 and 0.02 <= np.linalg.norm(e["T_true"][:3, 3]) <= 0.06
    assert ref["status"] == 0 and ref["iterations"] == sum(OR.E2E_ITERATIONS) and len(ref["first"]) == 3
    assert e["error"] < e["start"] / 50 and e["error"] < 1e-3
    assert ref["fitness"] > 0.9 and ref["rmse"] < 0.01
    # every level starts nearer than the one before, and its first step is a well-posed one
    starts = [OR.displacement(f["T0"], e["T_true"], e["points"]) for f in ref["first"]]
    assert starts[0] > starts[1] > starts[2] > e["error"]
    for f in ref["first"]:
        assert f["step"]["status"] == 0 and f["step"]["cond"] <= 1e6 and f["step"]["n"] >= 500


@pytest.mark.parametrize("name", OR.UPDATE_CASES)
def test_update_cases_have_what_they_are_there_for(name):
    c = OR.update_case(name)
    for lam in c["lambdas"]:
        r = OR.run_update(c, lam)
        assert r["status"] == c["status"], (name, lam, r["status"])
        if r["status"] == 0:
            assert r["cond"] <= 1e6, (name, lam, r["cond"])
            assert np.abs(r["T"][:3, :3] @ r["T"][:3, :3].T - np.eye(3)).max() <= 1e-14
        else:
            assert np.array_equal(r["T"], c["T"])
        again = OR.run_update(c, lam, apply=False)
        assert again["status"] == r["status"] and again["n"] == r["n"] and np.array_equal(again["T"], c["T"])
    why = np.bincount(OR.run_update(c, c["lambdas"][0])["why"].ravel(), minlength=9)
    n = int(why[0])
    if name == "size_4x3":
        assert n == 2                                  # (the two pixels that are not on the border)
    if name == "size_257x255":
        assert c["w"] * c["h"] == 256 * 256 - 1        # all 256 workgroups, the last thread idle
    if name == "size_257x257":
        assert c["w"] * c["h"] > 256 * 256             # more pixels than 256 workgroups x 256 threads: a second round
    if name == "outside":
        assert why[6] > 500 and why[8] > 0 and n > 1000
    if name == "behind":
        assert why[4] == 100
    if name == "edge":
        ok = OR.run_update(c, c["lambdas"][0])["ok"]
        assert why[8] == 8 and [bool(ok[20, 8 + k]) for k in range(8)] == [True, False] * 4
        assert [bool(ok[21, 24 + k]) for k in range(8)] == [True, False] * 4
    if name == "nan_planes":
        assert why[1] > 100 and why[7] > 400 and n > 2000
    if name == "all_invalid":
        assert n == 0 and OR.run_update(c, OR.LAMBDA)["rmse"] == 0.0
    if name == "wall":
        r = OR.run_update(c, OR.LAMBDA)
        assert n == 62 * 62 and r["sum_rD2"] == n * 0.015625 ** 2 and r["sum_rI2"] == 0.0
        assert r["JtJ"][2, 2] == 0.0 and r["JtJ"][3, 3] == 0.0 and r["JtJ"][4, 4] == 0.0      # rotation about z, x and y shifts


def test_unweighted_sums_are_zero_where_the_weight_is():
    c = OR.update_case("size_20x13")
    assert OR.run_update(c, 0.0)["sum_rD2"] == 0.0 and OR.run_update(c, 0.0)["sum_rI2"] > 0.0
    assert OR.run_update(c, 1.0)["sum_rI2"] == 0.0 and OR.run_update(c, 1.0)["sum_rD2"] > 0.0


def test_prepare_reference_rules():
    f = np.float32
    color = np.stack([np.full((5, 6), v, dtype=f) for v in (0.1, 0.2, 0.4)])
    depth = np.full((5, 6), 2.0, dtype=f)
    depth[0, :5] = [0.0, np.nan, np.inf, -1.0, 4.0]
    depth[1, 0] = np.nextafter(f(4.0), f(5.0))
    mask = np.ones((5, 6), dtype=f)
    mask[4, 0], mask[4, 1] = 0.0, 0.5
    I, D, g = OR.prepare(color, depth, mask, 0.0, 4.0)
    assert np.isnan(D[0, :4]).all() and D[0, 4] == 4.0 and np.isnan(D[1, 0]) and D[2, 2] == 2.0
    assert np.isnan(I[4, :2]).all() and np.isnan(D[4, :2]).all() and I[0, 0] == (f(0.1) + f(0.2) + f(0.4)) / f(3)
    assert g.shape == (4, 5, 6) and np.isnan(g[:, 0]).all() and np.isnan(g[:, :, 0]).all() and np.isnan(g[:, -1]).all()
    assert g[0, 2, 3] == 0.0 and g[2, 2, 3] == 0.0 and np.isnan(g[0, 3, 1]) and np.isnan(g[2, 1, 1])
    ramp = np.broadcast_to(np.arange(6, dtype=f)[None, :] * f(0.5), (5, 6))
    gx, gy = OR.sobel(ramp)
    assert gx[2, 2] == 0.5 and gy[2, 2] == 0.0
    assert OR.prepare(color, depth, None, 0.0, 4.0, gradients=False)[2] is None


# ---- camera_after_odometry --------------------------------------------------------------------------------------------------------
def test_camera_after_odometry_is_the_stated_product():
    w2c_t = OR.look_at((1.5, 1.3, 1.4))
    T = OR.E2E_MOTION
    cam_t = S.camera_from_intrinsics(140.0, 141.0, 80.3, 59.1, 160, 120, w2c=w2c_t, znear=0.05, zfar=50.0, name="kf")
    cam_s = S.camera_after_odometry(cam_t, torch.from_numpy(T))
    want = np.linalg.inv(T) @ w2c_t
    got = cam_s.world_view_transform.double().numpy().T
    assert np.abs(got - want).max() <= 4e-7                        # (the camera stores float32)
    assert S.camera_intrinsics(cam_s) == S.camera_intrinsics(cam_t) == (140.0, 141.0, 80.3, 59.1)
    assert (cam_s.image_width, cam_s.image_height, cam_s.znear, cam_s.zfar, cam_s.image_name) == (160, 120, 0.05, 50.0, "kf")
    # a world point seen at x_s by the source camera lies at T x_s in the target camera
    X = np.array([0.2, 0.1, 0.0, 1.0])
    assert np.abs(T @ (got @ X) - w2c_t @ X).max() <= 2e-6
    # the identity gives the target's own pose back; numpy and nested lists are taken too
    same = S.camera_after_odometry(cam_t, np.eye(4))
    assert (same.world_view_transform - cam_t.world_view_transform).abs().max() <= 1e-7      # (an inverse on the way: not bits)
    assert torch.equal(S.camera_after_odometry(cam_t, T.tolist()).world_view_transform, cam_s.world_view_transform)
    for bad in (np.eye(3), None, np.full((4, 4), np.nan)):
        with pytest.raises(ValueError):
            S.camera_after_odometry(cam_t, bad)


# ---- validation: ValueError / TypeError before any device work, GsrError for CPU tensors ---------------------------------------------
def _frame(w=32, h=24, depth=True, K=(30.0, 30.0, 15.5, 11.5)):
    cam = S.camera_from_intrinsics(*K, w, h)
    return S.Frame(torch.rand(3, h, w), torch.full((h, w), 2.0) if depth else None, torch.ones(h, w), cam)


def _level(w=8, h=6, grad=True, K=(7.0, 7.0, 3.5, 2.5)):
    z = torch.zeros(h, w)
    return S.OdometryLevel(z, z + 2.0, torch.zeros(4, h, w) if grad else None, K, w, h)


def test_prepare_level_validation():
    from diff_gaussian_rasterization import _C
    img, d, m, K = torch.rand(3, 6, 8), torch.ones(6, 8), torch.ones(6, 8), (7.0, 7.0, 3.5, 2.5)
    for bad in (torch.rand(6, 8), torch.rand(4, 6, 8), torch.zeros(3, 6, 8, dtype=torch.int32), torch.rand(3, 0, 8), "x"):
        with pytest.raises(ValueError, match="image"):
            S.prepare_odometry_level(bad, d, m, K)
    for bad in (torch.ones(6, 9), torch.ones(2, 6, 8), None, torch.ones(6, 8, dtype=torch.int64)):
        with pytest.raises(ValueError, match="depth"):
            S.prepare_odometry_level(img, bad, m, K)
    with pytest.raises(ValueError, match="mask"):
        S.prepare_odometry_level(img, d, torch.ones(5, 8), K)
    for bad in ((0.0, 7.0, 3.5, 2.5), (7.0, -1.0, 3.5, 2.5), (7.0, 7.0, math.nan, 2.5), (7.0, 7.0, math.inf, 2.5), (7.0, 7.0, 3.5)):
        with pytest.raises(ValueError, match="K"):
            S.prepare_odometry_level(img, d, m, bad)
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (math.nan, 1.0), (0.0, math.nan)):
        with pytest.raises(ValueError, match="depth_min"):
            S.prepare_odometry_level(img, d, m, K, depth_min=lo, depth_max=hi)
    with pytest.raises(TypeError, match="depth_max"):
        S.prepare_odometry_level(img, d, m, K, depth_max="4")
    with pytest.raises(_C.GsrError, match="no CPU path"):
        S.prepare_odometry_level(img, d, m, K)
    with pytest.raises(_C.GsrError, match="no CPU path"):
        S.prepare_odometry_level(img, d.unsqueeze(0), None, K, gradients=False)


def test_odometry_update_validation():
    s, t = _level(grad=False), _level()
    with pytest.raises(TypeError, match="source_level"):
        S.odometry_update((s.intensity, s.depth), t, None)
    with pytest.raises(ValueError, match="one size"):
        S.odometry_update(_level(w=9, grad=False), t, None)
    with pytest.raises(ValueError, match="one camera"):
        S.odometry_update(_level(grad=False, K=(7.5, 7.0, 3.5, 2.5)), t, None)
    with pytest.raises(ValueError, match="no gradients"):
        S.odometry_update(s, _level(grad=False), None)
    with pytest.raises(ValueError, match="transformation"):
        S.odometry_update(s, t, np.eye(3))
    for lam in (-0.1, 1.1, math.nan):
        with pytest.raises(ValueError, match="lambda_geometric"):
            S.odometry_update(s, t, None, lambda_geometric=lam)
    with pytest.raises(TypeError, match="lambda_geometric"):
        S.odometry_update(s, t, None, lambda_geometric=True)
    for ddm in (0.0, -1.0, math.nan):
        with pytest.raises(ValueError, match="depth_diff_max"):
            S.odometry_update(s, t, None, depth_diff_max=ddm)
    with pytest.raises(TypeError, match="depth_diff_max"):
        S.odometry_update(s, t, None, depth_diff_max=None)


def test_odometry_update_checks_every_plane_before_any_device_work():
    """an OdometryLevel is a plain tuple anybody can build: every plane's type, dtype and shape is held against width x height
    (ValueError), and a level of CPU tensors that is otherwise in order ends in GsrError - never in a launch"""
    from diff_gaussian_rasterization import _C
    s, t = _level(grad=False), _level()
    z = torch.zeros(6, 8)
    for field, bad in (("intensity", torch.zeros(6, 7)), ("intensity", torch.zeros(5, 8)), ("depth", torch.zeros(48)),
                       ("depth", torch.zeros(1, 6, 8)), ("depth", torch.zeros(6, 8, dtype=torch.int32)), ("intensity", None),
                       ("depth", z.numpy())):
        with pytest.raises(ValueError, match=f"source_level.{field}"):
            S.odometry_update(s._replace(**{field: bad}), t, None)
        with pytest.raises(ValueError, match=f"target_level.{field}"):
            S.odometry_update(s, t._replace(**{field: bad}), None)
    for bad in (torch.zeros(3, 6, 8), torch.zeros(4, 6, 7), torch.zeros(6, 8), torch.zeros(4, 48), torch.zeros(4, 6, 8, dtype=torch.int64)):
        with pytest.raises(ValueError, match="target_level.grad"):
            S.odometry_update(s, t._replace(grad=bad), None)
    for field, bad in (("width", 0), ("height", -1), ("width", 8.0), ("height", True)):
        with pytest.raises(ValueError, match=field):
            S.odometry_update(s._replace(**{field: bad}), t, None)
    with pytest.raises(ValueError, match="one size"):          # planes that fit a size the other level does not have
        S.odometry_update(S.OdometryLevel(torch.zeros(6, 9), torch.zeros(6, 9), None, s.K, 9, 6), t, None)
    with pytest.raises(ValueError, match="K"):
        S.odometry_update(s._replace(K=(7.0, 0.0, 3.5, 2.5)), t._replace(K=(7.0, 0.0, 3.5, 2.5)), None)
    # everything in order but the device: the product path fails loudly
    with pytest.raises(_C.GsrError, match="no CPU path"):
        S.odometry_update(s, t, None)
    with pytest.raises(_C.GsrError, match="no CPU path"):
        S.odometry_update(s._replace(depth=z.double()), t, torch.eye(4), apply=False)


def test_rgbd_odometry_validation():
    from diff_gaussian_rasterization import _C
    a, b = _frame(), _frame()
    for its in ((), (1, 2, 3, 4, 5), (3, -1)):
        with pytest.raises(ValueError, match="max_iterations"):
            S.rgbd_odometry(a, b, max_iterations=its)
    for its in (5, (2.5, 1), (True, 1)):
        with pytest.raises(TypeError, match="max_iterations"):
            S.rgbd_odometry(a, b, max_iterations=its)
    with pytest.raises(TypeError, match="source"):
        S.rgbd_odometry((a.image, a.depth), b)
    with pytest.raises(ValueError, match="no depth"):
        S.rgbd_odometry(a, _frame(depth=False))
    with pytest.raises(ValueError, match="one size"):
        S.rgbd_odometry(a, _frame(w=34))
    with pytest.raises(ValueError, match="one camera"):
        S.rgbd_odometry(a, _frame(K=(30.0, 30.5, 15.5, 11.5)))
    with pytest.raises(ValueError, match="has no pixels"):
        S.rgbd_odometry(_frame(h=3, K=(30.0, 30.0, 15.5, 1.0)), _frame(h=3, K=(30.0, 30.0, 15.5, 1.0)), max_iterations=(1, 1, 1))
    with pytest.raises(ValueError, match="init"):
        S.rgbd_odometry(a, b, init=np.eye(3))
    with pytest.raises(ValueError, match="lambda_geometric"):
        S.rgbd_odometry(a, b, lambda_geometric=2.0)
    with pytest.raises(ValueError, match="depth_min"):
        S.rgbd_odometry(a, b, depth_min=4.0, depth_max=4.0)
    with pytest.raises(ValueError, match="depth_diff_max"):
        S.rgbd_odometry(a, b, depth_diff_max=0.0)
    with pytest.raises(ValueError, match="check_every"):
        S.rgbd_odometry(a, b, check_every=-1)
    with pytest.raises(TypeError, match="check_every"):
        S.rgbd_odometry(a, b, check_every=1.5)
    for name in ("relative_rmse", "relative_fitness"):
        with pytest.raises(ValueError, match=name):
            S.rgbd_odometry(a, b, **{name: -1e-6})
        with pytest.raises(TypeError, match=name):
            S.rgbd_odometry(a, b, **{name: "small"})
    with pytest.raises(_C.GsrError, match="no CPU path"):
        S.rgbd_odometry(a, b)


def test_a_pyramid_with_too_few_levels_is_refused():
    class TwoLevels(S.FramePyramid):          # (a FramePyramid is built on the device: this one only counts)
        def __init__(self, frame):
            self.levels, self.frames = 1, [frame, frame]
    with pytest.raises(ValueError, match="pyramid of 2 levels"):
        S.rgbd_odometry(TwoLevels(_frame()), _frame(), max_iterations=(3, 2, 1))


def test_exports_and_defaults():
    import inspect
    for n in ("OdometryLevel", "OdometryResult", "prepare_odometry_level", "odometry_update", "rgbd_odometry", "camera_after_odometry"):
        assert getattr(S, n) is getattr(O, n)
    assert S.OdometryLevel._fields == ("intensity", "depth", "grad", "K", "width", "height")
    assert S.OdometryResult._fields == ("transformation", "fitness", "inlier_rmse", "iterations", "status")
    p = inspect.signature(S.rgbd_odometry).parameters
    assert [p[k].default for k in ("max_iterations", "lambda_geometric", "depth_min", "depth_max", "depth_diff_max", "check_every",
                                   "relative_rmse", "relative_fitness")] == [(20, 10, 5), 0.968, 0.0, 4.0, 0.03, 0, 1e-6, 1e-6]
    from diff_gaussian_rasterization import _C
    assert _C.lib().gsr_odometry_workspace_bytes(640, 480) == _C.lib().gsr_odometry_workspace_bytes(1, 1) >= 256 * 30 * 8
