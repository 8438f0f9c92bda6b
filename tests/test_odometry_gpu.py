"""scene_utils.rgbd_odometry on the device: against the float64 reference on the analytic corner scene, check_every, and the call
sequence rendered frames -> rgbd_odometry -> camera_after_odometry -> track_pose.

The end-to-end bound.  E_ref, the reference's own distance from the true motion (tests/test_odometry_cpu.py: 9.05e-4 m), is
computed in the same run; the device's must be <= 1.1 x E_ref.  Both sides run the same 35 steps on bit-identical planes; only a
projection that falls on a pixel boundary to the last bit can be associated differently, and each such tie is one term among
thousands - the margin is for that and nothing else."""
import functools
import math

import numpy as np
import pytest
import torch

import odometry_reference as OR
import scene_utils as S
from test_odometry_update_gpu import bits64, check_step, dev

pytestmark = pytest.mark.gpu


def frame(color, depth, K, w2c=None):
    h, w = depth.shape
    cam = S.camera_from_intrinsics(*K, w, h, w2c=w2c, device="cuda")
    return S.Frame(dev(color), dev(depth), None, cam)


@functools.lru_cache(maxsize=None)
def e2e_frames():
    e = OR.e2e()
    return frame(*e["source"][:2], e["K"]), frame(*e["target"][:2], e["K"])


def test_rgbd_odometry_against_the_reference_on_the_corner_scene():
    e = OR.e2e()
    ref = e["ref"]
    source, target = e2e_frames()
    res = S.rgbd_odometry(source, target, max_iterations=OR.E2E_ITERATIONS)
    T = res.transformation.cpu().numpy()
    err = OR.displacement(T, e["T_true"], e["points"])
    print(f"corner scene: start {e['start']:.4e} m, E_ref {e['error']:.4e} m, device {err:.4e} m (bound {1.1 * e['error']:.4e}); "
          f"device - reference {OR.displacement(T, ref['T'], e['points']):.3e} m; fitness {res.fitness:.6f} / {ref['fitness']:.6f}, "
          f"rmse {res.inlier_rmse:.6e} / {ref['rmse']:.6e}")
    assert err <= 1.1 * e["error"], (err, e["error"])
    # the closing apply=False evaluation at level 0, end to end: float64 sums of 18 632 terms in another order
    assert abs(res.fitness - ref["fitness"]) <= 1e-12 * ref["fitness"] and abs(res.inlier_rmse - ref["rmse"]) <= 1e-12 * ref["rmse"]
    assert res.iterations == ref["iterations"] == sum(OR.E2E_ITERATIONS) and res.status == ref["status"] == 0
    assert T[3].tolist() == [0.0, 0.0, 0.0, 1.0] and res.transformation.is_cuda and res.transformation.dtype == torch.float64
    # a pyramid handed in gives the bits of the pyramid built inside
    again = S.rgbd_odometry(S.FramePyramid(source, 2), S.FramePyramid(target, 3), max_iterations=OR.E2E_ITERATIONS)
    assert np.array_equal(bits64(again.transformation), bits64(res.transformation))
    assert (again.fitness, again.inlier_rmse, again.iterations, again.status) == (res.fitness, res.inlier_rmse, res.iterations, res.status)


def test_the_first_update_of_every_level_from_the_reference_transformation():
    e = OR.e2e()
    source, target = e2e_frames()
    ps, pt = S.FramePyramid(source, 2), S.FramePyramid(target, 2)
    for f in e["ref"]["first"]:
        level = f["level"]
        K, w, h, sI, sD, tI, tD, tg = f["planes"]
        fs, ft = ps[level], pt[level]
        assert S.camera_intrinsics(fs.camera) == tuple(K) and (fs.camera.image_width, fs.camera.image_height) == (w, h)
        src = S.prepare_odometry_level(fs.image, fs.depth, fs.mask, K, gradients=False)
        tgt = S.prepare_odometry_level(ft.image, ft.depth, ft.mask, K)
        T, stats = S.odometry_update(src, tgt, torch.from_numpy(f["T0"]))
        case = dict(K=K, w=w, h=h, src_D=sD, T=f["T0"])
        check_step(case, f["step"], T, stats, f"corner scene level {level}")


def test_check_every_reads_back_and_changes_nothing():
    source, target = e2e_frames()
    its = (6, 4, 3)
    a = S.rgbd_odometry(source, target, max_iterations=its, check_every=0)
    b = S.rgbd_odometry(source, target, max_iterations=its, check_every=1, relative_rmse=0.0, relative_fitness=0.0)
    assert a.iterations == b.iterations == sum(its)                 # (|difference| < 0 never holds: no early stop)
    assert np.array_equal(bits64(a.transformation), bits64(b.transformation))
    assert (a.fitness, a.inlier_rmse, a.status) == (b.fitness, b.inlier_rmse, b.status)
    # an early stop leaves the level, not the run: with bars nothing can miss, two iterations per level
    c = S.rgbd_odometry(source, target, max_iterations=its, check_every=1, relative_rmse=1.0, relative_fitness=1.0)
    assert c.iterations == 6 and c.status == 0
    # one level, and a start that is not the identity
    d = S.rgbd_odometry(source, target, init=a.transformation, max_iterations=(2,))
    assert d.iterations == 2 and d.status == 0


def test_integration_rendered_frames_to_a_start_pose_for_track_pose():
    """Two views of a synthetic model rendered with depth="z" at 128 x 96; odometry between them; the predicted camera is nearer
    the true one than the previous frame's camera reused unchanged, in rotation and in position; track_pose starts from it."""
    from gaussian_renderer import render, PipelineParams
    raw = S.make_gaussians(20000, 3, seed=4, scale_factor=0.35)
    model = S.GaussianModel.from_raw(raw.to("cuda"), requires_grad=False)
    prev = S.fibonacci_cameras(4, 128, 96, seed=2, device="cuda")[1]       # the last tracked frame: the target
    w2c_prev = prev.world_view_transform.transpose(0, 1).double().cpu()
    dist = float(prev.camera_center.norm())
    axis, tdir = torch.tensor([0.3, -0.8, 0.5], dtype=torch.float64), torch.tensor([0.6, 0.2, -0.77], dtype=torch.float64)
    delta = torch.cat([0.01 * dist * tdir / tdir.norm(), math.radians(1.0) * axis / axis.norm()])
    w2c_new = S.se3_exp(delta) @ w2c_prev                                  # the new frame: the source
    fx, fy, cx, cy = S.camera_intrinsics(prev)
    new = S.camera_from_intrinsics(fx, fy, cx, cy, 128, 96, w2c=w2c_new, device="cuda")
    bg = torch.zeros(3, device="cuda")
    frames, rendered_depth = [], []
    with torch.no_grad():
        for cam in (new, prev):
            pkg = render(cam, model, PipelineParams(), bg, depth="z", alpha=True)
            alpha = pkg["alpha"].detach().reshape(96, 128)
            mask = (alpha > 0.9).float()
            rendered_depth.append(pkg["depth"].detach().reshape(96, 128).clone())
            # (the rendered depth is sum_i w_i z_i: divided by the accumulated opacity it is what a sensor would report)
            frames.append(S.Frame(pkg["render"].detach().clone(), rendered_depth[-1] / alpha.clamp_min(1e-6), mask, cam))
    res = S.rgbd_odometry(frames[0], frames[1], depth_max=2.0 * dist, depth_diff_max=0.05 * dist)
    assert res.status == 0 and res.fitness > 0.1
    pred = S.camera_after_odometry(prev, res.transformation)
    r0, t0 = S.pose_error(w2c_prev, w2c_new)
    r1, t1 = S.pose_error(pred.world_view_transform.transpose(0, 1).double().cpu(), w2c_new)
    print(f"integration: previous camera reused {math.degrees(r0):.4f} deg / {t0:.5f}; camera_after_odometry {math.degrees(r1):.4f} deg / "
          f"{t1:.5f}; fitness {res.fitness:.3f}, rmse {res.inlier_rmse:.4f}")
    assert r1 < r0 and t1 < t0, (r0, t0, r1, t1)
    assert pred.world_view_transform.is_cuda and (pred.image_width, pred.image_height) == (128, 96)
    gt, gt_depth = frames[0].image, rendered_depth[0]
    pc, losses = S.track_pose(pred, model, gt, iters=20, bg=bg, gt_depth=gt_depth, mask=frames[0].mask)
    r2, t2 = S.pose_error(pc.w2c().detach().cpu(), w2c_new)
    print(f"integration: after 20 track_pose iterations {math.degrees(r2):.4f} deg / {t2:.5f}")
    assert losses.shape == (20,) and bool(torch.isfinite(losses).all())
    assert r2 < r0 and t2 < t0, (r0, t0, r2, t2)           # tracking from the predicted start stays nearer than no prediction


def test_pyramids_whose_coarse_levels_disagree_are_refused():
    """size and intrinsics are held level by level, not only at level 0"""
    source, target = e2e_frames()
    ps, pt = S.FramePyramid(source, 2), S.FramePyramid(target, 2)
    K1 = S.camera_intrinsics(pt[1].camera)
    other = S.camera_from_intrinsics(K1[0] * 1.01, K1[1], K1[2], K1[3], 80, 60, device="cuda")
    pt.frames[1] = S.Frame(pt[1].image, pt[1].depth, pt[1].mask, other)
    with pytest.raises(ValueError, match="one camera"):
        S.rgbd_odometry(ps, pt, max_iterations=(1, 1, 1))
    pt.frames[1] = S.FramePyramid(target, 3)[2]            # a 40 x 30 frame where 80 x 60 belongs
    with pytest.raises(ValueError, match="one size"):
        S.rgbd_odometry(ps, pt, max_iterations=(1, 1, 1))
    pt.frames[1] = S.Frame(ps[1].image, None, None, ps[1].camera)
    with pytest.raises(ValueError, match="no depth"):
        S.rgbd_odometry(ps, pt, max_iterations=(1, 1, 1))
