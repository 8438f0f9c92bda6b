"""CPU tests of the K-matrix cameras (scene_utils.cameras: camera_from_intrinsics, camera_projection, scaled_camera), of the pose
cameras' and transform_camera's handling of the principal point, of the new C-ABI entry points' argument checks, and of the numpy
reference the GPU tests of the frame front end compare with (tests/frames_reference.py)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import frames_reference as FR
from oracle import gs_oracle as O
from scene_utils import (camera_from_RT, camera_from_intrinsics, camera_projection, scaled_camera, projection_matrix, focal2fov,
                         PoseCamera, transform_camera, fibonacci_cameras, se3_exp)

W, H = 64, 48
K = (58.0, 61.0, 29.3, 25.1)          # cx, cy off the centre (31.5, 23.5)


def _pose(seed=3):
    """A seeded rigid world-to-camera matrix (float64)."""
    g = torch.Generator().manual_seed(seed)
    tau = torch.cat([0.5 * torch.randn(3, generator=g, dtype=torch.float64), 0.4 * torch.randn(3, generator=g, dtype=torch.float64)])
    return se3_exp(tau).numpy()


def _pixels(cam, pts):
    """Pixel means of world points through the camera's float64 matrices: world_view_transform as stored, the projection rebuilt
    in float64 by camera_projection - the chain every consumer uses - and the rasterizer's ndc -> pixel map."""
    wv = cam.world_view_transform.double().numpy()
    full = wv @ camera_projection(cam, dtype=torch.float64).numpy().T
    hom = pts @ full[:3] + full[3]
    ndc = hom[:, :2] / hom[:, 3:4]
    return ((ndc + 1.0) * np.array([cam.image_width, cam.image_height]) - 1.0) * 0.5


def test_projection_convention_against_the_oracle():
    """The oracle's preprocess in float64 puts a view-space point (x, y, z) of an off-centre camera_from_intrinsics camera at
    (fx x / z + cx, fy y / z + cy), to 1e-9 px, for 200 seeded points in front of the camera.  The matrices are the camera's own
    pose and camera_projection(cam) evaluated in float64 (the float32 tensors the camera stores are checked against them below to
    float32 rounding).  The oracle divides by w + 1e-7 - its restatement of the rasterizer's guard - which moves a pixel by
    (u - c) 1e-7 / (z + 1e-7), c = (S - 1) / 2, up to 1e-6 px here: that known factor is divided out, exactly, before the
    comparison, so the bound tests the convention and nothing else."""
    fx, fy, cx, cy = K
    cam = camera_from_intrinsics(fx, fy, cx, cy, W, H, w2c=_pose())
    assert abs(cam.ox - (2 * cx - (W - 1)) / W) < 1e-15 and abs(cam.oy - (2 * cy - (H - 1)) / H) < 1e-15
    assert (cam.fx, cam.fy, cam.cx, cam.cy) == K and abs(cam.ox) > 0.05 and abs(cam.oy) > 0.05
    rng = np.random.default_rng(7)
    P = 200
    view = np.stack([rng.uniform(-1.5, 1.5, P), rng.uniform(-1.0, 1.0, P), rng.uniform(1.0, 6.0, P)], 1)
    wv = cam.world_view_transform.double()                          # W2C^T
    w2c = wv.numpy().T
    pts = (view - w2c[:3, 3]) @ w2c[:3, :3]                          # rigid inverse: R^T (v - t)
    view = pts @ w2c[:3, :3].T + w2c[:3, 3]                          # (the view-space points these world points really have)
    full = wv @ camera_projection(cam, dtype=torch.float64).transpose(0, 1)
    s = O.OracleSettings(image_height=H, image_width=W, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5),
                         bg=torch.zeros(3), scale_modifier=1.0, viewmatrix=wv, projmatrix=full, sh_degree=0,
                         campos=cam.camera_center.double(), prefiltered=False, debug=False, antialiasing=False)
    pre = O.preprocess(torch.tensor(pts), None, torch.full((P, 1), 0.5, dtype=torch.float64), s,
                       colors_precomp=torch.zeros(P, 3, dtype=torch.float64), scales=torch.full((P, 3), 0.01, dtype=torch.float64),
                       rotations=torch.tensor([[1.0, 0, 0, 0]], dtype=torch.float64).repeat(P, 1))
    xy = pre.xy.numpy()
    z = view[:, 2]
    c = np.array([(W - 1) / 2, (H - 1) / 2])
    xy = c + (xy - c) * ((z + 1e-7) / z)[:, None]                    # the oracle's w + 1e-7, divided out
    want = np.stack([fx * view[:, 0] / z + cx, fy * view[:, 1] / z + cy], 1)
    err = np.abs(xy - want).max()
    print(f"projection convention: max |pixel - (f x / z + c)| = {err:.3e} px over {P} points")
    assert err <= 1e-9, err
    # the camera's own float32 full_proj_transform is that matrix to float32 rounding
    assert float((cam.full_proj_transform.double() - full).abs().max()) <= 4 * 2.0 ** -24 * float(full.abs().max())
    # and this module's own float64 chain agrees with the oracle
    assert np.abs(_pixels(cam, pts) - want).max() <= 1e-9


def test_centred_intrinsics_equal_the_fov_camera():
    fx, fy = 71.0, 69.5
    pose = _pose(5)
    a = camera_from_intrinsics(fx, fy, (W - 1) / 2, (H - 1) / 2, W, H, w2c=pose)
    b = camera_from_RT(pose[:3, :3].T, pose[:3, 3], focal2fov(fx, W), focal2fov(fy, H), W, H)
    assert a.ox == 0.0 and a.oy == 0.0 and b.ox == 0.0 and b.oy == 0.0
    assert abs(b.fx - fx) < 1e-9 and abs(b.cx - (W - 1) / 2) < 1e-12 and abs(b.cy - (H - 1) / 2) < 1e-12
    for name in ("world_view_transform", "full_proj_transform", "camera_center"):
        x, y = getattr(a, name), getattr(b, name)
        assert float((x - y).abs().max()) <= 2.0 ** -23 * max(1.0, float(y.abs().max())), name
    assert (a.image_width, a.image_height, a.znear, a.zfar) == (b.image_width, b.image_height, b.znear, b.zfar)
    assert abs(a.FoVx - b.FoVx) < 1e-15 and abs(a.FoVy - b.FoVy) < 1e-15


def test_projection_matrix_defaults_are_the_old_matrix_bit_for_bit():
    for zn, zf, fovx, fovy in ((0.01, 100.0, 0.6911, 0.52), (0.1, 30.0, 1.3, 1.1)):
        ty, tx = math.tan(fovy / 2.0), math.tan(fovx / 2.0)
        top, right = ty * zn, tx * zn
        old = torch.zeros(4, 4)                      # the matrix as it was built before the offsets existed
        old[0, 0] = 2.0 * zn / (right + right)
        old[1, 1] = 2.0 * zn / (top + top)
        old[3, 2] = 1.0
        old[2, 2] = zf / (zf - zn)
        old[2, 3] = -(zf * zn) / (zf - zn)
        new = projection_matrix(zn, zf, fovx, fovy)
        assert new.dtype == torch.float32 and torch.equal(new, old)
        assert torch.equal(projection_matrix(zn, zf, fovx, fovy, 0.0, 0.0), old)
        off = projection_matrix(zn, zf, fovx, fovy, 0.1, -0.08)
        assert float(off[0, 2]) == np.float32(0.1) and float(off[1, 2]) == np.float32(-0.08)
        off[0, 2] = off[1, 2] = 0.0
        assert torch.equal(off, old)
    cam = fibonacci_cameras(2, 40, 24, seed=1)[0]
    assert torch.equal(camera_projection(cam), projection_matrix(cam.znear, cam.zfar, cam.FoVx, cam.FoVy))

    class Bare:           # a camera object without ox / oy: the old matrix
        znear, zfar, FoVx, FoVy = cam.znear, cam.zfar, cam.FoVx, cam.FoVy
    assert torch.equal(camera_projection(Bare()), camera_projection(cam))


@pytest.mark.parametrize("level", [1, 2, 3])
def test_scaled_camera_pixels(level):
    """70 x 54 -> 35 x 27 -> 17 x 13 -> 8 x 6 (odd halves on the way): a world point's pixel at level l is (u + 0.5) / 2^l - 0.5 of
    its level-0 pixel, to 1e-9."""
    Wp, Hp = 70, 54
    cam = camera_from_intrinsics(80.0, 78.0, 33.2, 27.9, Wp, Hp, w2c=_pose(9))
    lv = scaled_camera(cam, level)
    assert (lv.image_width, lv.image_height) == (Wp >> level, Hp >> level)
    fx, fy, cx, cy, w, h = FR.scaled_intrinsics(80.0, 78.0, 33.2, 27.9, Wp, Hp, level)
    assert (lv.fx, lv.fy, lv.cx, lv.cy) == (fx, fy, cx, cy)
    assert abs(lv.ox - (2 * cx - (w - 1)) / w) < 1e-15 and abs(lv.oy - (2 * cy - (h - 1)) / h) < 1e-15
    # the pose is shared, not copied
    assert lv.world_view_transform.data_ptr() == cam.world_view_transform.data_ptr()
    assert lv.camera_center.data_ptr() == cam.camera_center.data_ptr()
    rng = np.random.default_rng(11)
    view = np.stack([rng.uniform(-1, 1, 200), rng.uniform(-0.8, 0.8, 200), rng.uniform(1.5, 5, 200)], 1)
    w2c = cam.world_view_transform.double().numpy().T
    pts = (view - w2c[:3, 3]) @ w2c[:3, :3]
    p0, pl = _pixels(cam, pts), _pixels(lv, pts)
    err = np.abs(pl - ((p0 + 0.5) / 2 ** level - 0.5)).max()
    assert err <= 1e-9, err


def test_scaled_camera_keeps_ox_on_even_sizes():
    cam = camera_from_intrinsics(90.0, 88.0, 36.7, 22.4, 64, 48)
    for level in (1, 2, 3):           # 64 x 48 halves evenly three times
        lv = scaled_camera(cam, level)
        assert abs(lv.ox - cam.ox) < 1e-15 and abs(lv.oy - cam.oy) < 1e-15
    odd = scaled_camera(camera_from_intrinsics(90.0, 88.0, 34.0, 22.4, 69, 48), 1)     # 69 -> 34: the dropped column shifts ox
    assert abs(odd.ox - (2 * ((34.0 + 0.5) / 2 - 0.5) - 33) / 34) < 1e-15 and abs(odd.ox) > 1e-3
    # a camera without the new attributes (any object with the old surface) is centred
    base = fibonacci_cameras(2, 64, 48, seed=1)[0]

    class Old:
        pass
    old = Old()
    for a in ("image_width", "image_height", "FoVx", "FoVy", "znear", "zfar", "world_view_transform", "camera_center"):
        setattr(old, a, getattr(base, a))
    lv = scaled_camera(old, 2)
    assert lv.ox == 0.0 and abs(lv.fx - base.fx / 4) < 1e-12 and torch.equal(lv.full_proj_transform, scaled_camera(base, 2).full_proj_transform)


def test_value_errors():
    with pytest.raises(ValueError, match="principal point"):
        camera_from_intrinsics(60.0, 60.0, 31.5 + 0.26 * 32, 23.5, W, H)          # ox = 0.26
    with pytest.raises(ValueError, match="principal point"):
        camera_from_intrinsics(60.0, 60.0, 31.5, 23.5 - 0.26 * 24, W, H)          # oy = -0.26
    camera_from_intrinsics(60.0, 60.0, 31.5 + 0.24 * 32, 23.5 - 0.24 * 24, W, H)  # inside the band
    cam = camera_from_intrinsics(60.0, 60.0, 5.5, 2.5, 12, 6)
    assert scaled_camera(cam, 1).image_height == 3
    with pytest.raises(ValueError, match="no pixels"):
        scaled_camera(cam, 3)                                                     # 12 x 6 -> 6 x 3 -> 3 x 1 -> 1 x 0
    # a level may leave the band although level 0 is inside it: 9 -> 4 drops a column
    edge = camera_from_intrinsics(20.0, 20.0, 4.0 + 0.245 * 4.5, 4.0, 9, 9)
    with pytest.raises(ValueError, match="principal point"):
        scaled_camera(edge, 1)


def test_pose_cameras_and_transform_camera_keep_the_principal_point():
    fx, fy, cx, cy = K
    cam = camera_from_intrinsics(fx, fy, cx, cy, W, H, w2c=_pose(13))
    P_T = projection_matrix(cam.znear, cam.zfar, cam.FoVx, cam.FoVy, cam.ox, cam.oy).transpose(0, 1)
    assert float(P_T[2, 0]) == np.float32(cam.ox) and float(P_T[2, 1]) == np.float32(cam.oy)
    pc = PoseCamera(cam, dtype=torch.float64, device="cpu", requires_grad=False)
    assert (pc.ox, pc.oy) == (cam.ox, cam.oy)
    assert torch.equal(pc.full_proj_transform, pc.w2c().transpose(0, 1) @ P_T.double())
    assert float((pc.full_proj_transform.float() - cam.full_proj_transform).abs().max()) <= 1e-6
    # set_intrinsics: another level's size and projection, the pose untouched
    base, lv = pc.base_w2c.clone(), scaled_camera(cam, 1)
    assert pc.set_intrinsics(lv) is pc and torch.equal(pc.base_w2c, base)
    assert (pc.image_width, pc.image_height, pc.ox, pc.oy, pc.FoVx) == (lv.image_width, lv.image_height, lv.ox, lv.oy, lv.FoVx)
    assert float((pc.full_proj_transform.float() - lv.full_proj_transform).abs().max()) <= 1e-6
    # a pose camera wrapping a pose camera keeps them too
    assert PoseCamera(pc, requires_grad=False).ox == lv.ox
    # transform_camera
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = _pose(17)[:3, :3], [0.3, -0.2, 0.5]
    moved = transform_camera(cam, T)
    assert (moved.ox, moved.oy, moved.fx, moved.cx, moved.cy) == (cam.ox, cam.oy, cam.fx, cam.cx, cam.cy)
    want = moved.world_view_transform.unsqueeze(0).bmm(P_T.unsqueeze(0)).squeeze(0)
    assert torch.equal(moved.full_proj_transform, want)
    # the same point of the moved map lands on the same pixel
    rng = np.random.default_rng(19)
    view = np.stack([rng.uniform(-1, 1, 50), rng.uniform(-0.8, 0.8, 50), rng.uniform(1.5, 5, 50)], 1)
    w2c = cam.world_view_transform.double().numpy().T
    pts = (view - w2c[:3, 3]) @ w2c[:3, :3]
    assert np.abs(_pixels(moved, pts @ T[:3, :3].T + T[:3, 3]) - _pixels(cam, pts)).max() <= 1e-4
    # an old-style camera comes out as before: centred
    old = fibonacci_cameras(2, 40, 24, seed=1)[0]
    assert transform_camera(old, T).ox == 0.0 and PoseCamera(old).oy == 0.0


def test_abi_has_the_frame_entry_points_and_checks_arguments_without_a_gpu():
    from diff_gaussian_rasterization import _C
    lib = _C.lib()
    for n in ("gsr_unproject_rgbd_k", "gsr_frame_undistort", "gsr_frame_pyramid"):
        assert n in _C.EXPORTS and hasattr(lib, n)
    assert C.sizeof(_C.gsr_unproject_params_k) == C.sizeof(_C.gsr_unproject_params) + 8
    assert _C.gsr_unproject_params_k.base.offset == 0 and _C.gsr_unproject_params_k.ox.offset == C.sizeof(_C.gsr_unproject_params)
    fake = C.c_void_p(256)             # never dereferenced: every check below fails before any device work
    outs = (C.c_void_p * 3)(256, 256, 256)
    # a level whose side would reach 0 is an error, not a clamp: 12 x 6, L = 3
    assert lib.gsr_frame_pyramid(12, 6, 3, fake, None, None, 0.05, outs, None, None, None) == -1
    assert "no pixels" in _C.last_error()
    for bad in ((12, 6, 0), (12, 6, 4), (0, 6, 1)):
        assert lib.gsr_frame_pyramid(*bad, fake, None, None, 0.05, outs, None, None, None) == -1
    assert lib.gsr_frame_pyramid(64, 48, 2, fake, fake, None, 0.05, outs, None, None, None) == -1       # depth without outputs
    assert lib.gsr_frame_pyramid(64, 48, 2, fake, None, None, -1.0, outs, None, None, None) == -1
    k = (C.c_float * 4)(60.0, 60.0, 31.5, 23.5)
    d = (C.c_float * 5)()
    assert lib.gsr_frame_undistort(64, 48, None, None, k, d, 64, 48, None, fake, None, fake, None) == -1
    assert lib.gsr_frame_undistort(64, 48, fake, fake, k, d, 64, 48, None, fake, None, fake, None) == -1  # depth in, none out
    assert lib.gsr_frame_undistort(64, 48, fake, None, k, d, 0, 48, None, fake, None, fake, None) == -1
    bad_k = (C.c_float * 4)(0.0, 60.0, 31.5, 23.5)
    assert lib.gsr_frame_undistort(64, 48, fake, None, bad_k, d, 64, 48, None, fake, None, fake, None) == -1
    nan_d = (C.c_float * 5)(float("nan"))
    assert lib.gsr_frame_undistort(64, 48, fake, None, k, nan_d, 64, 48, None, fake, None, fake, None) == -1
    view = torch.eye(4)
    p = _C.gsr_unproject_params_k(_C.gsr_unproject_params(48, 64, 0.5, 0.4, view.data_ptr(), 1, 0.2, math.inf, 0.5, 0.05), 2.0, 0.0)
    assert lib.gsr_unproject_rgbd_k(C.byref(p), fake, fake, None, None, fake, fake, 10, fake, fake, 1 << 30, None) == -1


def test_cpu_tensors_raise():
    from diff_gaussian_rasterization import _C
    from scene_utils import Frame, FramePyramid
    img, depth = torch.rand(3, 48, 64), torch.rand(48, 64) + 1
    with pytest.raises(_C.GsrError, match="no CPU path"):
        Frame.from_sensor(img, depth, K, (-0.1, 0.01, 0, 0, 0))
    cam = camera_from_intrinsics(*K, W, H)
    with pytest.raises(_C.GsrError, match="no CPU path"):
        FramePyramid(Frame(img, depth, torch.ones(48, 64), cam), 2)


def test_the_undistort_reference_on_the_shared_scene():
    """What the GPU test relies on, checked on the reference alone: the target's border falls outside the source (both mask values
    occur), the nearest-pixel depth sees both sides of the edge and the hole, target pixels within 1e-3 px of a nearest-pixel tie
    are under 1 % of the image, and the float32 restatement stays close to float64 where both call a pixel inside."""
    sc = FR.undistort_scene()
    r64 = FR.undistort_reference(sc["color"], sc["depth"], sc["K"], sc["D"], sc["new_K"], sc["W"], sc["H"], np.float64)
    r32 = FR.undistort_reference(sc["color"], sc["depth"], sc["K"], sc["D"], sc["new_K"], sc["W"], sc["H"], np.float32)
    m = r64["mask"] > 0
    assert 0.5 < m.mean() < 0.95, m.mean()
    vals = set(np.unique(r64["depth"][m]).tolist())
    assert vals == {0.0, 2.0, 3.5}, vals
    tie = FR.near_half_integer(r64["us"], r64["vs"])
    assert tie.mean() <= 0.01, tie.mean()
    both = m & (r32["mask"] > 0)
    err = np.abs(r32["color"].astype(np.float64) - r64["color"])[:, both].max()
    print(f"undistort: float32 restatement vs float64, max colour error {err:.3e}; ties left out {tie.mean():.4f}")
    assert err < 1e-5
    # the identity: pixels copied exactly, mask all ones
    ident = FR.undistort_reference(sc["color"], sc["depth"], sc["K"], (0,) * 5, sc["K"], sc["Ws"], sc["Hs"], np.float32)
    assert np.array_equal(ident["color"], sc["color"]) and np.array_equal(ident["depth"], sc["depth"]) and ident["mask"].all()


@pytest.mark.parametrize("size,levels", [((70, 54), 3), ((32, 32), 3), ((33, 17), 2)])
def test_the_pyramid_reference_on_the_shared_scenes(size, levels):
    """The scenes have what the GPU test wants to see - quads with zero, one and two valid readings, quads across the depth edge -
    and the reference treats them as stated: the near side survives at the edge, empty quads give 0, sizes halve with the odd
    remainder dropped."""
    Wp, Hp = size
    color, depth, mask = FR.pyramid_scene(Wp, Hp, seed=Wp)
    a, b, c, d = FR._quads(depth)
    nvalid = (a > 0).astype(int) + (b > 0) + (c > 0) + (d > 0)
    assert {0, 1, 2}.issubset(set(np.unique(nvalid).tolist()))
    q = np.stack([a, b, c, d])
    near = np.where(q > 0, q, np.inf).min(0)
    far = q.max(0)
    across = (nvalid >= 2) & (far > 1.2 * near)
    assert across.any()
    lv = FR.pyramid_reference(color, depth, mask, levels)
    w, h = Wp, Hp
    for col, dep, msk in lv:
        w, h = w // 2, h // 2
        assert col.shape == (3, h, w) and dep.shape == (h, w) and msk.shape == (h, w) and col.dtype == np.float32
    d1 = lv[0][1]
    assert (d1[nvalid == 0] == 0).all() and (d1[nvalid > 0] > 0).all()
    assert (d1[across] <= 1.06 * near[across]).all()                   # never a blend of the two sides
    assert ((lv[0][2] == 1) == (np.stack(FR._quads(mask)).min(0) == 1)).all()
    # float64 form: same rule, rounding apart
    l64 = FR.pyramid_reference(color, depth, mask, levels, dtype=np.float64)
    for (c32, d32, _), (c64, d64, _) in zip(lv, l64):
        assert np.abs(c32 - c64).max() < 1e-6
        same = np.abs(d32 - d64) < 1e-5
        assert same.mean() > 0.98            # (a reading exactly at the band's edge may fall either way)
