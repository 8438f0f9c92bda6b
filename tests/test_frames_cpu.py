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


# ------------------------------------------------------------------------------------------------------------------------------
# what tests/test_frames_bits_gpu.py relies on, on the reference alone
# ------------------------------------------------------------------------------------------------------------------------------
def _ref32(case):
    return FR.undistort_reference(case["color"], case["depth"], case["K"], case["D"], case["new_K"], case["W"], case["H"], np.float32)


@pytest.mark.parametrize("dist", [FR.BARREL, FR.PINCUSHION], ids=["barrel", "pincushion"])
def test_the_edge_size_undistort_cases_are_partly_inside(dist):
    """W in {1, 63, 64, 65, 129} x H in {1, 3, 4, 5, 9}, k3, p1, p2 all non-zero: in the float32 restatement the inside share of
    every target lies in 0.2 .. 0.98, so both mask values occur - except the 1 x 1 target, whose share can only be 0 or 1: its
    one pixel is inside.  (With the shared scene's fixed new_K every one of these targets would lie wholly outside the source.)"""
    assert dist[4] != 0 and dist[2] != 0 and dist[3] != 0
    for W in FR.EDGE_W:
        for H in FR.EDGE_H:
            r = _ref32(FR.undistort_case(80, 60, W, H, dist))
            share = float(r["mask"].mean())
            if (W, H) == (1, 1):
                assert share == 1.0
                continue
            assert 0.2 <= share <= 0.98, (W, H, share)
            assert set(np.unique(r["mask"]).tolist()) == {0.0, 1.0}
            assert (r["color"][:, r["mask"] == 0] == 0).all() and (r["depth"][r["mask"] == 0] == 0).all()
    sc = FR.undistort_scene()
    for W, H in ((1, 1), (63, 3), (64, 4), (65, 5)):
        fixed = FR.undistort_reference(sc["color"], sc["depth"], sc["K"], sc["D"], sc["new_K"], W, H, np.float32)
        assert fixed["mask"].sum() == 0


def test_the_tiny_source_undistort_cases():
    """1 x 1: the pixel (4, 4) alone is inside, at us = vs = 0 exactly, and carries the source pixel; 2 x 1 and 1 x 2: five pixels
    of row / column 4, with fractional coordinates between the two source pixels."""
    for Ws, Hs in FR.TINY_SOURCES:
        case, n = FR.undistort_tiny_source_case(Ws, Hs)
        r = _ref32(case)
        assert int(r["mask"].sum()) == n and r["mask"][4, 4] == 1
        if (Ws, Hs) == (1, 1):
            assert r["us"][4, 4] == 0 and r["vs"][4, 4] == 0
            assert np.array_equal(r["color"][:, 4, 4], case["color"][:, 0, 0]) and r["depth"][4, 4] == case["depth"][0, 0]
        else:
            line = r["us"][4, 2:7] if Ws == 2 else r["vs"][2:7, 4]
            assert (r["mask"][4, 2:7] if Ws == 2 else r["mask"][2:7, 4]).all()
            assert line[0] > 0 and line[-1] < 1 and len(set(line.tolist())) == 5
            assert set(np.unique(r["depth"]).tolist()) == {0.0, float(case["depth"].flat[0]), float(case["depth"].flat[1])}


@pytest.mark.parametrize("name", list(FR.EXACT_SHIFTS))
def test_the_exact_coordinate_undistort_cases(name):
    """undistort_map in float32 gives us = u + dx, vs = v + dy with no rounding at all, through the general path (not the identity:
    K' differs), so every coordinate sits on the intended grid: all ties, all integers, the last column on src_w - 1.  The mask is
    the one those coordinates give by hand, and on the integer grid the restatement copies the source."""
    dx, dy, W, H = FR.EXACT_SHIFTS[name]
    case = FR.undistort_exact_case(name)
    assert all(v == 0 for v in case["D"]) and case["new_K"][:2] == case["K"][:2] and case["new_K"] != case["K"]
    us, vs = FR.undistort_map(case["K"], case["D"], case["new_K"], W, H, np.float32)
    u, v = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    assert us.dtype == np.float32 and np.array_equal(us, u + np.float32(dx)) and np.array_equal(vs, v + np.float32(dy))
    inside = (u + dx >= 0) & (u + dx <= 15) & (v + dy >= 0) & (v + dy <= 11)
    r = _ref32(case)
    assert np.array_equal(r["mask"] == 1, inside) and inside.any()
    if name.startswith("last"):
        if "col" in name or "both" in name:
            assert (us[:, -1] == case["Ws"] - 1).all() and inside[:, -1].any()
        if "row" in name or "both" in name:
            assert (vs[-1] == case["Hs"] - 1).all() and inside[-1].any()
    if name in ("half_y", "half_x"):
        assert (us[:, 0] == 0).all() if name == "half_y" else (vs[0] == 0).all()
    if name == "minus_one":
        assert not inside[:, 0].any() and not inside[0].any() and (us[:, 1] == 0).all() and (vs[1] == 0).all() and inside[1:, 1:].all()
    if dx % 1 == 0 and dy % 1 == 0:            # the taps coincide: a copy, bit for bit
        ys, xs = np.nonzero(inside)
        sy, sx = ys + int(dy), xs + int(dx)
        assert np.array_equal(r["color"][:, ys, xs], case["color"][:, sy, sx]) and np.array_equal(r["depth"][ys, xs], case["depth"][sy, sx])
    else:                                      # ties: the nearest pixel is the one half a pixel UP (floor(us + 0.5))
        ys, xs = np.nonzero(inside)
        sy, sx = np.floor(ys + dy + 0.5).astype(int), np.floor(xs + dx + 0.5).astype(int)
        assert np.array_equal(r["depth"][ys, xs], case["depth"][sy, sx])
    assert len(np.unique(case["depth"])) == case["depth"].size          # a wrong nearest pixel is another value


def test_the_overflow_undistort_case():
    """Non-finite coordinates (inf and NaN) on part of the target, finite ones elsewhere; every non-finite pixel is outside and
    exactly 0, and a large part of the rest is inside."""
    case = FR.undistort_overflow_case()
    assert all(np.isfinite(np.float32(v)) for v in case["D"] + case["K"] + case["new_K"])
    r = _ref32(case)
    bad = ~(np.isfinite(r["us"]) & np.isfinite(r["vs"]))
    assert 0.1 < bad.mean() < 0.9 and np.isnan(r["us"]).any() and np.isinf(r["us"]).any() and np.isinf(r["vs"]).any()
    assert (r["mask"][bad] == 0).all() and (r["color"][:, bad] == 0).all() and (r["depth"][bad] == 0).all()
    assert 0.2 < r["mask"].mean() < 0.98 and r["mask"][~bad].mean() > 0.5


def test_the_other_undistort_cases_have_both_mask_values():
    cases = FR.undistort_named_cases()
    for name in ("source_80x60", "source_80x60_pincushion", "upsample", "downsample", "special_values"):
        r = _ref32(cases[name])
        assert 0.2 <= r["mask"].mean() <= 0.98, (name, r["mask"].mean())
    r = _ref32(cases["special_values"])
    d = r["depth"]
    assert np.isnan(r["color"]).any() and np.isinf(r["color"]).any()
    assert np.isposinf(d).any() and np.isneginf(d).any() and (d == -1.5).any() and np.isnan(d).any() and (np.signbit(d) & (d == 0)).any()
    full = FR.undistort_full_frame_case()
    assert (full["W"], full["H"]) == (640, 480) and 0.5 < _ref32(full)["mask"].mean() < 0.99
    # FR.differing: bits, with any NaN equal to a NaN
    a = np.array([0.0, -0.0, np.nan, 1.0, np.inf], dtype=np.float32)
    b = np.array([0.0, 0.0, -np.nan, np.nextafter(np.float32(1), np.float32(2)), np.inf], dtype=np.float32)
    assert FR.differing(a, b).tolist() == [False, True, False, True, False]


@pytest.mark.parametrize("band", [0.05, 0.0, 1e6, 3e38])
def test_the_hand_built_pyramid_quads(band):
    """depth_class_quads has the classes the GPU test is there for, and the reference treats each as include/gsr.h says - in both
    dtypes, and at the stride of every level (the class sits in the level below the last)."""
    q = FR.depth_class_quads(band)
    nvalid = {k: sum(1 for r in v if 0 < r < np.inf) for k, v in q.items()}
    assert [nvalid[f"valid{i}"] for i in range(5)] == [0, 1, 2, 3, 4]
    assert all(np.isposinf(r) for r in q["inf_alone"]) and nvalid["inf_beside_finite"] == 1 and np.isposinf(q["inf_beside_finite"][0])
    assert np.isnan(q["nan"][0]) and q["negative"][0] < 0 and np.signbit(q["minus_zero"][0]) and q["minus_zero"][0] == 0
    assert 0 < q["denormal_alone"][0] < np.finfo(np.float32).tiny and len(set(q["equal4"])) == 1
    one = np.float32(1) + np.float32(band)
    with np.errstate(over="ignore"):
        edge = np.float32(np.float32(2) * one)
    assert q["at_edge"][1] == edge and (q["above_edge"][1] == np.nextafter(edge, np.float32(np.inf)) or np.isinf(edge))
    for dtype in (np.float32, np.float64):
        for level in (1, 2, 3):
            color, depth, mask, where = FR.depth_class_scene(band, level)
            assert depth.shape == (4 << level, 6 << level) and set(where) == set(q)
            out = FR.pyramid_reference(color, depth, mask, level, band, dtype)[-1]
            got = {k: out[1][rc] for k, rc in where.items()}
            assert np.isfinite(out[1]).all()                                  # +inf (and NaN) never enter a mean
            for k in ("valid0", "inf_alone", "inf_and_holes", "nan_alone", "negative_alone", "minus_zero_alone"):
                assert got[k] == 0 and not np.signbit(got[k]), (k, got[k])
            assert got["valid1"] == 2 and got["inf_beside_finite"] == 2 and got["equal4"] == 2.5
            assert got["denormal_alone"] == q["denormal_alone"][0] and got["denormal_beside_finite"] == q["denormal_alone"][0]
            if level == 1 and dtype == np.float32:                           # (deeper, an invalid square has become 0: still invalid)
                if band == 0.05:
                    assert got["at_edge"] == (np.float32(2) + edge) / np.float32(2) and got["above_edge"] == 2
                    assert got["far"] == 2 and got["inf_beside_three"] == (np.float32(2) + np.float32(2.05)) / np.float32(2)
                if band == 0.0:
                    assert got["valid4"] == 2 and got["at_edge"] == 2 and got["denormals"] == q["denormals"][0]
                if band >= 1e6:                                              # every finite valid reading is taken, +inf still not
                    assert got["far"] == 2.75 and got["inf_beside_three"] == np.float32(7.55) / np.float32(3)
            # mask values other than 1 give 0
            m0 = np.stack(FR._quads(mask)) if level == 1 else None
            if m0 is not None:
                assert {0.5, 2.0}.issubset(set(np.unique(mask[~np.isnan(mask)]).tolist())) and np.isnan(mask).any()
                assert np.array_equal(out[2] == 1, (m0 == 1).all(0)) and (out[2] == 1).any() and (out[2] == 0).any()


@pytest.mark.parametrize("size", [(66, 65), (33, 33), (64, 32), (31, 3)])
def test_the_float32_and_float64_pyramid_chains_agree(size):
    """Colour and depth of the two chains within 1e-6 at every level, apart from quads with a reading within 1e-5 (relative) of
    the band's edge in the float64 chain, and whatever such a quad feeds further up."""
    Wp, Hp = size
    color, depth, mask = FR.pyramid_scene(Wp, Hp, seed=Wp)
    levels = FR.max_levels(Wp, Hp)
    l32 = FR.pyramid_reference(color, depth, mask, levels)
    l64 = FR.pyramid_reference(color, depth, mask, levels, dtype=np.float64)
    below, tainted = depth.astype(np.float64), np.zeros(depth.shape, dtype=bool)
    for (c32, d32, m32), (c64, d64, m64) in zip(l32, l64):
        assert np.abs(c32 - c64).max() <= 1e-6 and np.array_equal(m32, m64)
        q = np.stack(FR._quads(below))
        m = np.where(q > 0, q, np.inf).min(0)
        lim = m * 1.05
        with np.errstate(invalid="ignore"):
            near = ((q > 0) & (np.abs(q - lim) <= 1e-5 * lim)).any(0)
        tainted = near | np.stack(FR._quads(tainted)).any(0)
        assert tainted.mean() < 0.02
        assert np.abs(d32 - d64)[~tainted].max() <= 1e-6, np.abs(d32 - d64)[~tainted].max()
        below = d64
