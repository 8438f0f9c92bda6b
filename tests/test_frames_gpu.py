"""Sensor frames on the device: back-projection with a principal point (gsr_unproject_rgbd_k), rendering through an off-centre
K-matrix camera against the float64 oracle, undistortion and the image / depth pyramid (csrc/frames.hip) against
tests/frames_reference.py, and coarse-to-fine tracking (track_pose(levels=...))."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import frames_reference as FR
from helpers import leaf_inputs, run_hip, run_oracle, settings_for, upstream_grads, rel_l2
from oracle import gs_oracle as O
from scene_utils import (make_gaussians, fibonacci_cameras, camera_from_intrinsics, scaled_camera, PoseCamera, DevicePoseCamera,
                         se3_exp, pose_error, track_pose, unproject_rgbd, Frame, FramePyramid, undistort, build_pyramid)
from scene_utils.model import GaussianModel
from test_camera_grad_gpu import check_camera
from test_depth_alpha_gpu import oracle_rgbd, hip_rgbd, new_grads, _close
from test_parity_gpu import check_forward, check_grads
from test_pose_device_gpu import CAM_REL, TWISTS, _hip_through_rasterizer, _perturbed_base, _device_camera

pytestmark = pytest.mark.gpu


def _pose(seed=3):
    g = torch.Generator().manual_seed(seed)
    tau = torch.cat([0.5 * torch.randn(3, generator=g, dtype=torch.float64), 0.4 * torch.randn(3, generator=g, dtype=torch.float64)])
    return se3_exp(tau).numpy()


# ------------------------------------------------------------------------------------------------------------------------------
# 1  back-projection with a principal point
# ------------------------------------------------------------------------------------------------------------------------------
def test_unproject_round_trip_with_a_principal_point():
    """64 x 48, cx = 29.3, cy = 25.1, a seeded pose, readings on about half the pixels: unproject_rgbd returns
    c2w ((u - cx) d / fx, (v - cy) d / fy, d) in row-major pixel order within 1e-5 (1 + |p|) of the float64 values.  (Without the
    principal point the points are off by (cx - (W - 1) / 2) d / fx.)"""
    W, H, fx, fy, cx, cy = 64, 48, 58.0, 61.0, 29.3, 25.1
    cam = camera_from_intrinsics(fx, fy, cx, cy, W, H, w2c=_pose(), device="cuda")
    rng = np.random.default_rng(21)
    depth = rng.uniform(0.8, 4.0, (H, W)).astype(np.float32)
    depth[rng.random((H, W)) < 0.5] = 0.0
    color = rng.random((3, H, W), dtype=np.float32)
    xyz, rgb = unproject_rgbd(cam, torch.tensor(color).cuda(), torch.tensor(depth).cuda())
    vs, us = np.nonzero(depth > 0.2)                                  # row-major
    assert 0.4 * W * H < len(us) < 0.6 * W * H and xyz.shape == (len(us), 3)
    d = depth[vs, us].astype(np.float64)
    view = np.stack([(us - cx) * d / fx, (vs - cy) * d / fy, d], 1)
    w2c = cam.world_view_transform.double().cpu().numpy().T
    want = (view - w2c[:3, 3]) @ w2c[:3, :3]
    err = np.abs(xyz.double().cpu().numpy() - want)
    bar = 1e-5 * (1.0 + np.linalg.norm(want, axis=1, keepdims=True))
    off = abs(cx - (W - 1) / 2) * d.max() / fx
    print(f"unproject with cx, cy: n = {len(us)}, max err / bar = {(err / bar).max():.3f}; dropping cx would cost up to {off:.3f}")
    assert (err <= bar).all(), float((err / bar).max())
    assert off > 100 * bar.max()
    assert torch.equal(rgb.cpu(), torch.tensor(color[:, vs, us].T.copy()))


@pytest.mark.parametrize("stride", [1, 3])
def test_unproject_k_with_a_centred_camera_is_the_old_entry_point_bit_for_bit(stride):
    from diff_gaussian_rasterization import _C
    lib = _C.lib()
    W, H = 64, 48
    cam = fibonacci_cameras(2, W, H, seed=3, device="cuda")[0]
    gen = torch.Generator().manual_seed(5)
    depth = (torch.rand(H, W, generator=gen) * 4.0).cuda()
    color = torch.rand(3, H, W, generator=gen).cuda()
    view = cam.world_view_transform.contiguous()
    cap = ((W + stride - 1) // stride) * ((H + stride - 1) // stride)
    ws = torch.empty(lib.gsr_unproject_workspace_bytes(W, H), dtype=torch.uint8, device="cuda")
    base = _C.gsr_unproject_params(H, W, math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2), view.data_ptr(), stride, 0.2, math.inf,
                                   0.5, 0.05)
    outs = []
    for entry, p in ((lib.gsr_unproject_rgbd, base), (lib.gsr_unproject_rgbd_k, _C.gsr_unproject_params_k(base, 0.0, 0.0))):
        xyz, rgb = torch.full((cap, 3), -7.0, device="cuda"), torch.full((cap, 3), -7.0, device="cuda")
        count = torch.zeros(1, dtype=torch.int64, device="cuda")
        _C.check(entry(C.byref(p), _C.ptr(depth), _C.ptr(color), None, None, _C.ptr(xyz), _C.ptr(rgb), cap, _C.ptr(count),
                       _C.ptr(ws), ws.numel(), _C._stream()))
        torch.cuda.synchronize()
        outs.append((int(count.item()), xyz.cpu(), rgb.cpu()))
    assert outs[0][0] == outs[1][0] > cap // 2
    assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][2], outs[1][2])
    # and the Python call (which always goes through the _k entry) gives those points for a camera without a principal point
    xyz, _ = unproject_rgbd(cam, color, depth, stride=stride)
    assert torch.equal(xyz.cpu(), outs[0][1][:outs[0][0]])


# ------------------------------------------------------------------------------------------------------------------------------
# 2  rendering through an off-centre camera
# ------------------------------------------------------------------------------------------------------------------------------
def _off_centre_camera():
    """80 x 64 with ox = 0.1, oy = -0.08, at the pose of one of the suite's orbit cameras."""
    W, H = 80, 64
    pose = fibonacci_cameras(3, W, H, seed=5)[1].world_view_transform.double().numpy().T
    cam = camera_from_intrinsics(110.0, 108.0, 0.5 * (W * 0.1 + W - 1), 0.5 * (H * -0.08 + H - 1), W, H, w2c=pose)
    assert abs(cam.ox - 0.1) < 1e-12 and abs(cam.oy + 0.08) < 1e-12
    return cam


def test_off_centre_render_matches_the_oracle():
    """500 Gaussians through a K-matrix camera whose principal point is 10 % / 8 % of the half-size off the centre: colour, inverse
    depth, radii and every gradient at test_parity_gpu's bars, z-depth, opacity and the camera's gradients at
    test_depth_alpha_gpu's (its constructions, its bars)."""
    raw = make_gaussians(500, 3, seed=11, scale_factor=0.6)
    cam = _off_centre_camera()
    bg = torch.tensor([0.2, 0.5, 0.7])
    gc, gd = upstream_grads(cam.image_height, cam.image_width)
    ref = run_oracle(raw, cam, 3, bg, torch.float64, gc=gc, gd=gd)
    out = run_hip(raw, cam, 3, bg, gc=gc, gd=gd, debug=True)
    assert int((ref["radii"] > 0).sum()) > 100
    check_forward(out, ref)
    check_grads(out, ref)
    # the means sit where the K matrix puts them, 4 px and 2.6 px from where a centred camera would
    vm = cam.world_view_transform.double()
    t = raw.xyz.double() @ vm[:3, :3] + vm[3, :3]
    front = t[:, 2] > 0.2
    xy = ref["state"]["pre"].xy.detach()[front]
    for i, (f, c) in enumerate(((cam.fx, cam.cx), (cam.fy, cam.cy))):       # (the camera's matrices are float32)
        want = f * t[front, i] / t[front, 2] + c
        assert bool(((xy[:, i] - want).abs() <= 1e-5 * (1.0 + want.abs())).all())
    assert abs(cam.cx - 39.5) == 4.0 and abs(cam.cy - 31.5) > 2.5
    # z-depth, accumulated opacity, camera gradients
    grads = new_grads(cam.image_height, cam.image_width)
    ref = oracle_rgbd(raw, cam, grads=grads)
    out = hip_rgbd(raw, cam, grads=grads)
    dmax = float(ref["D"].abs().max())
    assert dmax > 1.0 and float(ref["A"].max()) > 0.5
    ok, err = _close(out["D"], ref["D"], dmax)
    assert ok, err
    ok, err = _close(out["A"], ref["A"])
    assert ok, err
    ok, err = _close(out["color"], ref["color"])
    assert ok, err
    check_grads(out, ref)
    check_camera(out["cam"], ref["cam"])


def test_off_centre_camera_gradients_through_device_pose_camera():
    """dL/dtau through DevicePoseCamera (which must carry ox, oy into its projection) within CAM_REL of the float64 oracle driven by
    a host PoseCamera at the same twist: test_device_pose_camera_autograd_surface's comparison on the off-centre camera."""
    raw = make_gaussians(500, 3, seed=11, scale_factor=0.6)
    cam = _off_centre_camera()
    ref_pc = PoseCamera(cam, dtype=torch.float64, device="cpu")
    with torch.no_grad():
        ref_pc.tau.copy_(torch.tensor(TWISTS["chain"], dtype=torch.float64))
    inp = leaf_inputs(raw, torch.float64, "cpu", "sh")
    s = settings_for(ref_pc, 3, torch.tensor([0.2, 0.5, 0.7]))
    color, _, invd = O.rasterize(inp["means3D"], inp["means2D"], inp["opacities"], s, shs=inp["shs"], scales=inp["scales"],
                                 rotations=inp["rotations"])
    gc, gd = upstream_grads(cam.image_height, cam.image_width)
    ((color * gc.double()).sum() + (invd * gd.double()).sum()).backward()
    ref = ref_pc.tau.grad.detach()
    pc = DevicePoseCamera(cam, device="cuda")
    assert (pc.ox, pc.oy) == (cam.ox, cam.oy)
    with torch.no_grad():
        pc.tau.copy_(torch.tensor(TWISTS["chain"], dtype=torch.float64).cuda())
    assert float((pc.full_proj_transform.detach().cpu().double() - ref_pc.full_proj_transform.detach()).abs().max()) < 1e-5
    _hip_through_rasterizer(raw, pc)
    out = pc.tau.grad.detach().cpu()
    e, m = rel_l2(out, ref), float((out - ref).abs().max() / ref.abs().max())
    print(f"off-centre dL/dtau through DevicePoseCamera: rel-L2 {e:.3e}, max-abs / max|g| {m:.3e}")
    assert float(ref.abs().max()) > 0 and e <= CAM_REL and m <= CAM_REL, (out, ref)
    # set_intrinsics keeps the pose and the twist and drops the cache
    base, tau = pc.base_w2c.clone(), pc.tau.detach().clone()
    lv = scaled_camera(cam, 1)
    pc.set_intrinsics(lv)
    assert torch.equal(pc.base_w2c, base) and torch.equal(pc.tau.detach(), tau) and pc._cache is None
    assert (pc.image_width, pc.image_height, pc.ox) == (40, 32, lv.ox)
    host = PoseCamera(lv, dtype=torch.float64, device="cpu")
    with torch.no_grad():
        host.tau.copy_(tau.cpu())
        assert float((pc.full_proj_transform.cpu().double() - host.full_proj_transform).abs().max()) < 1e-5


# ------------------------------------------------------------------------------------------------------------------------------
# 3  undistortion
# ------------------------------------------------------------------------------------------------------------------------------
def test_undistort_matches_the_reference():
    """The shared scene (80 x 60 source, D = (-0.28, 0.07, 1e-3, -5e-4, 0), 72 x 56 target with its own K) through Frame.from_sensor.
    Colour where the mask is 1: within max(1e-6, 4 x the float32 restatement's own error against float64 on this input) of the
    float64 reference (the factor 4 dates from when the compiler contracted the kernel's arithmetic to fma; frames.hip is now
    compiled without contraction and equals the restatement bit for bit, so 1 would do: tests/test_frames_bits_gpu.py holds it
    to that, with no pixel left out).  Mask: the float64 reference's, except where a tap lies within 1e-3 px of the source
    border.  Depth: the float64 reference's exactly, target pixels within 1e-3 px of a nearest-pixel tie left out (under 1 % of
    the image: tests/test_frames_cpu.py) - float32 and float64 coordinates may round to different sides there.
    Measured on an MI355X: see profiles/frames.txt."""
    sc = FR.undistort_scene()
    args = (sc["color"], sc["depth"], sc["K"], sc["D"], sc["new_K"], sc["W"], sc["H"])
    r64, r32 = FR.undistort_reference(*args, np.float64), FR.undistort_reference(*args, np.float32)
    pose = _pose(4)
    fr = Frame.from_sensor(torch.tensor(sc["color"]).cuda(), torch.tensor(sc["depth"]).cuda(), sc["K"], sc["D"], pose=pose,
                           size=(sc["W"], sc["H"]), new_K=sc["new_K"])
    torch.cuda.synchronize()
    col, dep, msk = fr.image.cpu().numpy(), fr.depth.cpu().numpy(), fr.mask.cpu().numpy()
    assert col.shape == (3, sc["H"], sc["W"]) and dep.shape == msk.shape == (sc["H"], sc["W"]) and col.dtype == np.float32
    cam = fr.camera
    assert (cam.fx, cam.fy, cam.cx, cam.cy, cam.image_width, cam.image_height) == (*sc["new_K"], sc["W"], sc["H"])
    assert np.abs(cam.world_view_transform.cpu().numpy().T - pose).max() < 1e-6 and cam.world_view_transform.is_cuda
    # mask
    edge = FR.near_border(r64["us"], r64["vs"], sc["Ws"], sc["Hs"])
    assert set(np.unique(msk).tolist()) == {0.0, 1.0}
    assert np.array_equal(msk[~edge], r64["mask"][~edge]) and edge.mean() < 0.01
    inside = (msk == 1) & (r64["mask"] == 1)
    assert (col[:, msk == 0] == 0).all() and (dep[msk == 0] == 0).all()
    # colour
    yard = np.abs(r32["color"].astype(np.float64) - r64["color"])[:, inside & (r32["mask"] == 1)].max()
    bar = max(1e-6, 4.0 * yard)
    err = np.abs(col.astype(np.float64) - r64["color"])[:, inside].max()
    bits = np.abs(col - r32["color"])[:, inside & (r32["mask"] == 1)].max()
    print(f"undistort colour: max |hip - float64| = {err:.3e}, float32 restatement's own error {yard:.3e}, bar {bar:.3e}; "
          f"max |hip - float32 restatement| = {bits:.3e}")
    assert err <= bar, (err, bar)
    # depth
    tie = FR.near_half_integer(r64["us"], r64["vs"])
    assert tie.mean() <= 0.01
    keep = inside & ~tie
    assert np.array_equal(dep[keep], r64["depth"][keep].astype(np.float32))
    assert set(np.unique(dep[keep]).tolist()) == {0.0, 2.0, 3.5}                 # both sides of the edge and the hole: no blend
    print(f"undistort depth: exact on {int(keep.sum())} pixels, {tie.mean():.4f} of the image left out as ties; "
          f"mask: {edge.mean():.4f} of the image within 1e-3 px of the border")


def test_undistort_identity_copies_the_frame():
    """All-zero coefficients and the same K: pixels copied exactly, mask 1 everywhere - with and without depth, and through an
    explicit new_K equal to K."""
    sc = FR.undistort_scene()
    color, depth = torch.tensor(sc["color"]).cuda(), torch.tensor(sc["depth"]).cuda()
    for kw in (dict(dist=None), dict(dist=(0.0,) * 5, new_K=sc["K"]), dict(dist=(0.0,) * 4)):
        col, dep, msk = undistort(color, depth, sc["K"], **kw)
        assert torch.equal(col, color) and torch.equal(dep, depth) and bool((msk == 1).all())
    col, dep, msk = undistort(color, None, sc["K"])
    assert dep is None and torch.equal(col, color) and bool((msk == 1).all())
    # no distortion but another K is a resampling, not a copy: the reference's
    K2 = (sc["K"][0] * 0.9, sc["K"][1] * 0.9, sc["K"][2] + 0.25, sc["K"][3] - 0.5)
    col, dep, msk = undistort(color, depth, sc["K"], None, new_K=K2)
    r64 = FR.undistort_reference(sc["color"], sc["depth"], sc["K"], (0,) * 5, K2, sc["Ws"], sc["Hs"], np.float64)
    inside = (msk.cpu().numpy() == 1) & (r64["mask"] == 1)
    assert 0.5 < inside.mean() < 1.0
    assert np.abs(col.cpu().numpy().astype(np.float64) - r64["color"])[:, inside].max() < 1e-5


# ------------------------------------------------------------------------------------------------------------------------------
# 4  pyramid
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,levels", [((70, 54), 3), ((32, 32), 3), ((33, 17), 2)])
def test_pyramid_is_the_float32_reference_bit_for_bit(size, levels):
    """70 x 54 (several workgroups, odd halves 35 -> 17 -> 8), 32 x 32 (one workgroup, last level 4 x 4), 33 x 17 (a partial block,
    odd both ways: the 4-byte load path).  The scene has a depth edge wider than the band, quads with zero, one and two valid
    readings and mask dropouts (tests/test_frames_cpu.py checks that it does)."""
    W, H = size
    color, depth, mask = FR.pyramid_scene(W, H, seed=W)
    ref = FR.pyramid_reference(color, depth, mask, levels)
    c, d, m = build_pyramid(torch.tensor(color).cuda(), torch.tensor(depth).cuda(), torch.tensor(mask).cuda(), levels)
    torch.cuda.synchronize()
    assert len(c) == len(d) == len(m) == levels
    for l in range(levels):
        rc, rd, rm = ref[l]
        assert c[l].shape == rc.shape and d[l].shape == rd.shape and m[l].shape == rm.shape, l
        assert np.array_equal(c[l].cpu().numpy(), rc), (l, np.abs(c[l].cpu().numpy() - rc).max())
        assert np.array_equal(d[l].cpu().numpy(), rd), (l, np.abs(d[l].cpu().numpy() - rd).max())
        assert np.array_equal(m[l].cpu().numpy(), rm), l
    a, b, cc, dd = FR._quads(depth)
    empty = (a <= 0) & (b <= 0) & (cc <= 0) & (dd <= 0)
    assert empty.any() and bool((d[0].cpu().numpy()[empty] == 0).all())
    # colour alone (no depth, no mask): the same colours
    c2, d2, m2 = build_pyramid(torch.tensor(color).cuda(), None, None, levels)
    assert d2 is None and m2 is None and all(torch.equal(x, y) for x, y in zip(c, c2))
    # FramePyramid: the same tensors, with scaled_camera's cameras
    cam = camera_from_intrinsics(90.0, 88.0, (W - 1) / 2 + 1.3, (H - 1) / 2 - 0.7, W, H, device="cuda")
    pyr = FramePyramid(Frame(torch.tensor(color).cuda(), torch.tensor(depth).cuda(), torch.tensor(mask).cuda(), cam), levels)
    assert len(pyr) == levels + 1 and pyr[0].camera is cam
    for l in range(1, levels + 1):
        f, want = pyr[l], scaled_camera(cam, l)
        assert torch.equal(f.image, c[l - 1]) and torch.equal(f.depth, d[l - 1]) and torch.equal(f.mask, m[l - 1])
        assert (f.camera.image_width, f.camera.image_height) == (W >> l, H >> l) == tuple(f.image.shape[:0:-1])
        assert (f.camera.fx, f.camera.cx, f.camera.cy) == (want.fx, want.cx, want.cy)
        assert torch.equal(f.camera.full_proj_transform, want.full_proj_transform)


def test_pyramid_level_without_pixels_raises():
    from diff_gaussian_rasterization import _C
    img = torch.rand(3, 6, 12, device="cuda")
    with pytest.raises(_C.GsrError, match="no pixels"):
        build_pyramid(img, torch.rand(6, 12, device="cuda"), None, 3)
    cam = camera_from_intrinsics(20.0, 20.0, 5.5, 2.5, 12, 6, device="cuda")
    with pytest.raises(ValueError, match="no pixels"):
        FramePyramid(Frame(img, None, None, cam), 3)
    c, _, _ = build_pyramid(img, None, None, 2)          # 6 x 3, 3 x 1
    assert [tuple(x.shape) for x in c] == [(3, 3, 6), (3, 1, 3)]


def test_cpu_tensors_raise():
    from diff_gaussian_rasterization import _C
    img, depth = torch.rand(3, 48, 64), torch.rand(48, 64) + 1
    with pytest.raises(_C.GsrError, match="no CPU path"):
        Frame.from_sensor(img, depth, (58.0, 61.0, 29.3, 25.1), (-0.1, 0.01, 0, 0, 0))
    with pytest.raises(_C.GsrError, match="no CPU path"):
        Frame.from_sensor(img.cuda(), depth, (58.0, 61.0, 29.3, 25.1), None)
    cam = camera_from_intrinsics(58.0, 61.0, 29.3, 25.1, 64, 48)
    with pytest.raises(_C.GsrError, match="no CPU path"):
        FramePyramid(Frame(img, depth, torch.ones(48, 64), cam), 2)


# ------------------------------------------------------------------------------------------------------------------------------
# 5  coarse-to-fine tracking
# ------------------------------------------------------------------------------------------------------------------------------
ITERS = 150       # test_track_pose_converges' iteration count


@pytest.fixture(scope="module")
def tracking_scene():
    """test_track_pose_converges' scene and target, rendered once."""
    from gaussian_renderer import render, PipelineParams
    raw = make_gaussians(20000, 3, seed=4, scale_factor=0.35)
    cam = fibonacci_cameras(4, 256, 192, seed=2, device="cuda")[1]
    model = GaussianModel.from_raw(raw.to("cuda"), requires_grad=False)
    with torch.no_grad():
        gt = render(cam, model, PipelineParams(), torch.zeros(3, device="cuda"))["render"].detach().clone()
    return cam, model, gt


def _twice_perturbed_base(cam):
    """_perturbed_base's twist, doubled: 2 deg, 4 % of the camera distance."""
    true_w2c = cam.world_view_transform.transpose(0, 1).double().cpu()
    dist = float(cam.camera_center.norm())
    axis = torch.tensor([0.3, -0.8, 0.5], dtype=torch.float64)
    tdir = torch.tensor([0.6, 0.2, -0.77], dtype=torch.float64)
    delta = 2.0 * torch.cat([0.02 * dist * tdir / tdir.norm(), math.radians(1.0) * axis / axis.norm()])
    return se3_exp(delta) @ true_w2c, true_w2c


def test_track_pose_levels_zero_is_the_old_call_bit_for_bit(tracking_scene):
    cam, model, gt = tracking_scene
    base, _ = _perturbed_base(cam)
    a, la = track_pose(_device_camera(cam, base), model, gt, iters=ITERS)
    b, lb = track_pose(_device_camera(cam, base), model, gt, iters=ITERS, levels=0)
    assert la.shape == (ITERS,) and torch.equal(la, lb)
    assert torch.equal(a.w2c().detach(), b.w2c().detach())


def test_track_pose_two_levels_converges(tracking_scene):
    """test_track_pose_converges' start and its absolute bars (rotation <= 1e-2 deg, translation <= 2e-3) with levels=2:
    ITERS // 2 iterations at 64 x 48, ITERS // 2 at 128 x 96, ITERS at 256 x 192.  Measured on an MI355X: profiles/frames.txt."""
    cam, model, gt = tracking_scene
    base, true_w2c = _perturbed_base(cam)
    pc = _device_camera(cam, base)
    r0, t0 = pose_error(pc.w2c().detach().cpu(), true_w2c)
    out, losses = track_pose(pc, model, gt, iters=ITERS, levels=2)
    assert out is pc and torch.all(pc.tau == 0) and losses.is_cuda and losses.shape == (ITERS + 2 * (ITERS // 2),)
    assert (pc.image_width, pc.image_height) == (256, 192)                  # back at level 0's intrinsics
    r1, t1 = pose_error(pc.w2c().detach().cpu(), true_w2c)
    print(f"track_pose(levels=2): rotation {math.degrees(r0):.4f} -> {math.degrees(r1):.3e} deg, translation {t0:.5f} -> {t1:.3e}")
    assert math.degrees(r1) <= 1e-2 and t1 <= 2e-3, (math.degrees(r1), t1)
    # level_iters picks the counts, coarsest level last in the list
    _, l2 = track_pose(_device_camera(cam, base), model, gt, iters=ITERS, levels=1, level_iters=[3, 2])
    assert l2.shape == (5,)
    with pytest.raises(ValueError, match="level_iters"):
        track_pose(_device_camera(cam, base), model, gt, levels=2, level_iters=[3, 2])


def test_track_pose_from_twice_the_perturbation(tracking_scene):
    """2 deg and 4 % of the camera distance, single-level against levels=2: both final errors are printed (profiles/frames.txt
    records them); what is asserted is that the multi-level run ends below its starting error - how much a pyramid buys on this
    scene has not been fixed."""
    cam, model, gt = tracking_scene
    base, true_w2c = _twice_perturbed_base(cam)
    r0, t0 = pose_error(base, true_w2c)
    res = {}
    for levels in (0, 2):
        pc, _ = track_pose(_device_camera(cam, base), model, gt, iters=ITERS, levels=levels)
        res[levels] = pose_error(pc.w2c().detach().cpu(), true_w2c)
    print(f"twice the perturbation: start {math.degrees(r0):.4f} deg / {t0:.5f}; levels=0 -> {math.degrees(res[0][0]):.3e} deg / "
          f"{res[0][1]:.3e}; levels=2 -> {math.degrees(res[2][0]):.3e} deg / {res[2][1]:.3e}")
    assert res[2][0] < r0 and res[2][1] < t0, (res, r0, t0)


def test_track_pose_rgbd_one_level_in_a_constant_colour_scene():
    """test_track_pose_rgbd_depth_only_in_a_constant_colour_scene's scene and demand (translation error down tenfold), with
    levels=1 and a mask: the depth pyramid and the mask pyramid drive the coarse level."""
    from gaussian_renderer import render, PipelineParams
    raw = make_gaussians(20000, 3, seed=4, scale_factor=0.35)
    with torch.no_grad():
        raw.features_dc.zero_()
        raw.features_rest.zero_()
    cam = fibonacci_cameras(4, 256, 192, seed=2, device="cuda")[1]
    model = GaussianModel.from_raw(raw.to("cuda"), requires_grad=False)
    bg = torch.full((3,), 0.5, device="cuda")
    with torch.no_grad():
        pkg = render(cam, model, PipelineParams(), bg, depth="z", alpha=True)
        gt, gt_depth = pkg["render"].detach().clone(), pkg["depth"].detach().clone()
    base, true_w2c = _perturbed_base(cam)
    pc = _device_camera(cam, base)
    r0, t0 = pose_error(pc.w2c().detach().cpu(), true_w2c)
    pc, losses = track_pose(pc, model, gt, iters=ITERS, bg=bg, gt_depth=gt_depth, depth_weight=1.0, alpha_min=0.5, levels=1)
    r1, t1 = pose_error(pc.w2c().detach().cpu(), true_w2c)
    mask = torch.ones(192, 256, device="cuda")
    mask[:, :16] = 0                               # a band the sensor did not see
    pm, _ = track_pose(_device_camera(cam, base), model, gt * mask, iters=ITERS, bg=bg, gt_depth=gt_depth * mask, depth_weight=0.5,
                       alpha_min=0.5, levels=1, mask=mask)
    r2, t2 = pose_error(pm.w2c().detach().cpu(), true_w2c)
    print(f"constant colour, levels=1: translation {t0:.5f} -> {t1:.3e} (depth only), {t2:.3e} (masked, depth_weight 0.5)")
    assert losses.shape == (ITERS + ITERS // 2,)
    assert t1 <= t0 / 10, (t0, t1)
    assert t2 < t0, (t0, t2)                       # (the masked RGB-D run: nobody has measured it; it must at least improve)
