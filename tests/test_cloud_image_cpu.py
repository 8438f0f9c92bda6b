"""CPU tests of the cloud-in-camera layer (scene_utils.lidar, csrc/cloud_image.hip): the new symbols resolve and the ABI version
stays; every bad argument is refused by the library and by the Python layer without a device - which shows that the refusal comes
before any device work (there is no device here); and the numpy restatement of the rules (tests/cloud_image_reference.py), which
the GPU tests compare bits against, behaves on scenes whose answer is known."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import cloud_image_reference as CR
import scene_utils as S
from diff_gaussian_rasterization import _C as GSR

F32 = np.float32
INVALID, TOO_SMALL = -1, -5
IDENT = (1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)


# ---- the library ------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_resolve_and_abi_stays_7():
    lib = GSR.lib()
    for name in ("gsr_cloud_project_workspace_bytes", "gsr_cloud_project", "gsr_depth_densify"):
        assert name in GSR.EXPORTS and getattr(lib, name) is not None
    assert lib.gsr_abi_version() == 7 and GSR.ABI_VERSION == 7
    assert GSR.CLOUD_MAX_FOOTPRINT == CR.MAX_FOOTPRINT == 4 and GSR.DENSIFY_MAX_RADIUS == CR.MAX_RADIUS == 8
    assert C.sizeof(GSR.gsr_cloud_camera) == 8 + 16 + 96 + 16      # no padding: the C struct's layout


def test_workspace_size_is_monotone_and_aligned():
    lib = GSR.lib()
    sizes = [lib.gsr_cloud_project_workspace_bytes(w, h) for w, h in ((1, 1), (64, 1), (65, 3), (131, 67), (640, 480), (1280, 720))]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0 and sizes[-1] > sizes[0]
    assert all(s % 256 == 0 for s in sizes)
    assert sizes[-1] >= 1280 * 720 * 12      # a uint32 and a uint64 per pixel
    assert lib.gsr_cloud_project_workspace_bytes(0, 0) > 0


def _cam(W=8, H=6, K=(8, 8, 3.5, 2.5), T=IDENT, z_near=0.05, z_far=100.0, footprint=2, scale=1.05):
    return GSR.gsr_cloud_camera(W, H, (C.c_float * 4)(*K), (C.c_double * 12)(*T), z_near, z_far, footprint, scale)


def _project(cam, N=4, points=256, image=None, mask=None, depth=256, index=256, pixel=256, z=256, visible=256, colors=None,
             count=256, ws=256, ws_bytes=1 << 20):
    """the call on fake pointers (never dereferenced: every call made with them fails a check)"""
    p = [None if v is None else C.c_void_p(v) for v in (points, image, mask, depth, index, pixel, z, visible, colors, count, ws)]
    return GSR.lib().gsr_cloud_project(None if cam is None else C.byref(cam), N, *p, ws_bytes, None)


def test_cloud_project_rejects_bad_arguments_before_any_launch():
    nan, inf = math.nan, math.inf
    assert _project(None) == INVALID and "NULL" in GSR.last_error()
    for null in ("points", "depth", "index", "pixel", "z", "visible", "count", "ws"):
        assert _project(_cam(), **{null: None}) == INVALID, null
        assert "NULL" in GSR.last_error(), null
    assert _project(_cam(), N=-1) == INVALID and "N = -1" in GSR.last_error()
    assert _project(_cam(), N=1 << 30) == INVALID
    assert _project(_cam(), colors=256) == INVALID and "image" in GSR.last_error()      # colors without image
    bad = [_cam(W=0), _cam(H=0), _cam(W=-3), _cam(W=1 << 15, H=1 << 15),
           _cam(K=(0, 8, 1, 1)), _cam(K=(8, -1, 1, 1)), _cam(K=(nan, 8, 1, 1)), _cam(K=(8, 8, inf, 1)), _cam(K=(8, 8, 1, nan)),
           _cam(T=(nan,) + IDENT[1:]), _cam(T=IDENT[:11] + (inf,)),
           _cam(z_near=0.0), _cam(z_near=-1.0), _cam(z_near=nan), _cam(z_near=2.0, z_far=2.0), _cam(z_far=inf), _cam(z_far=nan),
           _cam(footprint=-1), _cam(footprint=5),
           _cam(scale=0.99), _cam(scale=nan), _cam(scale=inf)]
    for i, cam in enumerate(bad):
        assert _project(cam) == INVALID, i
        assert GSR.last_error().startswith("cloud_project:"), i
    need = GSR.lib().gsr_cloud_project_workspace_bytes(8, 6)
    assert _project(_cam(), ws_bytes=need - 1) == TOO_SMALL
    assert "needed" in GSR.last_error()
    assert _project(_cam(), N=0, points=None, pixel=None, z=None, visible=None, ws_bytes=0) == TOO_SMALL      # N = 0 is checked alike


def test_depth_densify_rejects_bad_arguments_before_any_launch():
    lib = GSR.lib()
    fake = C.c_void_p(256)

    def call(W=8, H=6, depth=fake, radius=4, band=1.05, k=2, dense=fake, valid=fake):
        return lib.gsr_depth_densify(W, H, depth, radius, band, k, dense, valid, None)
    for kw in (dict(depth=None), dict(dense=None), dict(valid=None), dict(W=0), dict(H=0), dict(H=-1), dict(W=1 << 15, H=1 << 15),
               dict(radius=0), dict(radius=9), dict(radius=-1), dict(band=0.99), dict(band=math.nan), dict(band=math.inf),
               dict(k=0), dict(k=-2)):
        assert call(**kw) == INVALID, kw
        assert GSR.last_error().startswith("depth_densify:"), kw


# ---- validation in Python ---------------------------------------------------------------------------------------------------------------
def _camera(W=8, H=6):
    return S.camera_from_intrinsics(8.0, 8.0, 3.5, 2.5, W, H)


@pytest.mark.parametrize("kw, exc", [
    (dict(points=np.zeros((4, 3))), ValueError),
    (dict(points=torch.zeros(4, 2)), ValueError),
    (dict(points=torch.zeros(4, 3, dtype=torch.int32)), ValueError),
    (dict(image=torch.zeros(3, 5, 8)), ValueError),
    (dict(image=torch.zeros(6, 8)), ValueError),
    (dict(mask=torch.zeros(6, 7)), ValueError),
    (dict(w2c=torch.zeros(3, 4)), ValueError),
    (dict(w2c=torch.full((4, 4), math.nan)), ValueError),
    (dict(footprint=2.0), TypeError),
    (dict(footprint=True), TypeError),
    (dict(footprint=-1), ValueError),
    (dict(footprint=5), ValueError),
    (dict(occlusion="0.1"), TypeError),
    (dict(occlusion=-0.1), ValueError),
    (dict(occlusion=math.nan), ValueError),
    (dict(z_near=0.0), ValueError),
    (dict(z_near=None), TypeError),
    (dict(z_near=3.0, z_far=3.0), ValueError),
    (dict(z_far=math.inf), ValueError),
    (dict(), GSR.GsrError),                                  # all well, but a CPU tensor: no CPU path
    (dict(image=torch.zeros(3, 6, 8)), GSR.GsrError),
])
def test_project_cloud_validation(kw, exc):
    kw = dict(kw)
    points = kw.pop("points", torch.zeros(4, 3))
    with pytest.raises(exc, match="no CPU path" if exc is GSR.GsrError else None):
        S.project_cloud(points, _camera(), **kw)


@pytest.mark.parametrize("depth, kw, exc", [
    (np.zeros((6, 8), dtype=np.float32), {}, ValueError),
    (torch.zeros(6), {}, ValueError),
    (torch.zeros(2, 6, 8), {}, ValueError),
    (torch.zeros(6, 8, dtype=torch.int32), {}, ValueError),
    (torch.zeros(0, 8), {}, ValueError),
    (torch.zeros(6, 8), dict(radius=0), ValueError),
    (torch.zeros(6, 8), dict(radius=9), ValueError),
    (torch.zeros(6, 8), dict(radius=2.5), TypeError),
    (torch.zeros(6, 8), dict(depth_band=-0.01), ValueError),
    (torch.zeros(6, 8), dict(depth_band=math.inf), ValueError),
    (torch.zeros(6, 8), dict(depth_band=None), TypeError),
    (torch.zeros(6, 8), dict(min_neighbors=0), ValueError),
    (torch.zeros(6, 8), dict(min_neighbors=1.0), TypeError),
    (torch.zeros(6, 8), {}, GSR.GsrError),
])
def test_densify_depth_validation(depth, kw, exc):
    with pytest.raises(exc, match="no CPU path" if exc is GSR.GsrError else None):
        S.densify_depth(depth, **kw)


def test_frame_level_validation():
    cam = _camera()
    frame = S.Frame(torch.zeros(3, 6, 8), None, None, cam)
    pts = torch.zeros(4, 3)
    with pytest.raises(TypeError, match="unexpected option"):
        S.lidar_frame(frame, pts, radiu=3)
    with pytest.raises(TypeError, match="unexpected option"):
        S.colorize_cloud(pts, frame, radius=3)              # a densify option where only projection options go
    with pytest.raises(ValueError, match="densify=False"):
        S.lidar_frame(frame, pts, densify=False, radius=3)
    with pytest.raises(ValueError, match="radius"):
        S.lidar_frame(frame, pts, radius=9)                 # refused before the projection runs
    with pytest.raises(ValueError, match="cloud_to_world"):
        S.lidar_frame(frame, pts, cloud_to_world=torch.zeros(3, 3))
    with pytest.raises(ValueError, match="colors"):
        S.colorize_cloud(pts, frame, colors=torch.zeros(5, 3))
    with pytest.raises(ValueError, match="no image"):
        S.colorize_cloud(pts, S.Frame(None, None, None, cam))
    with pytest.raises(GSR.GsrError, match="no CPU path"):
        S.lidar_frame(frame, pts)
    with pytest.raises(GSR.GsrError, match="no CPU path"):
        S.colorize_cloud(pts, frame, colors=torch.zeros(4, 3))

    class Msg:
        Image = CameraInfo = CameraPose = None
    with pytest.raises(TypeError, match="Local_Map"):
        S.frame_from_visual_merged_map(Msg())
    Msg.Local_Map = None
    with pytest.raises(TypeError, match="decode"):
        S.frame_from_visual_merged_map(Msg(), decode=3)
    with pytest.raises(TypeError):
        S.frame_from_visual_merged_map(Msg())               # frame_from_messages refuses the empty Image


# ---- the reference on scenes with a known answer ----------------------------------------------------------------------------------------
K64 = (60.0, 60.0, 31.5, 23.5)
W64, H64 = 64, 48


@pytest.mark.parametrize("r", [0, 1, 2, 4])
def test_reference_wall_behind_box(r):
    """Box samples every 2 pixels, wall samples on every pixel: the wall rows behind the box land between box samples.  With a
    footprint of r >= 1 (2 <= 2 r + 1) the box's footprints tile its rectangle and every such row is hidden; with r = 0 only the
    wall rows that share a pixel with a box sample are - the case the footprint exists for."""
    pts, is_box, behind = CR.wall_and_box(W64, H64, K64, box_step=2.0)
    P = CR.project(pts, W64, H64, K64, np.eye(4), footprint=r, scale=CR.occlusion_scale(0.05))
    assert P.takes_part.all() and P.n_candidates == len(pts)
    assert P.visible[is_box].all()
    assert behind.sum() > 100
    if r >= 1:
        assert not P.visible[behind].any()
    else:
        shares = np.isin(P.pixel, P.pixel[is_box]) & ~is_box
        assert np.array_equal(P.visible[behind], ~shares[behind]) and P.visible[behind].sum() > behind.sum() // 2
    # the per-pixel outputs follow from the winners: index >= 0 exactly where a visible row has that pixel
    seen = np.zeros(W64 * H64, bool)
    seen[P.pixel[P.visible]] = True
    assert np.array_equal(P.index.reshape(-1) >= 0, seen)
    rows = P.index[P.index >= 0]
    assert np.array_equal(P.depth[P.index >= 0], P.z[rows]) and P.visible[rows].all()
    assert (P.depth[P.index < 0] == 0).all()


def test_reference_equal_z_lower_row_wins_and_duplicates_count():
    pts = np.array([[0.1, 0.1, 2.0], [0.1, 0.1, 2.0], [0.1, 0.1, 2.0], [0.2, 0.2, 4.0]], dtype=np.float32)      # one ray
    P = CR.project(pts[[3, 1, 0, 2]], W64, H64, K64, np.eye(4), footprint=0)
    at = int(P.pixel[1])
    assert (P.pixel == at).all() and P.index.reshape(-1)[at] == 1          # rows 1, 2, 3 tie: the lowest wins
    assert P.visible.tolist() == [False, True, True, True] and (P.n_visible, P.n_candidates) == (3, 4)
    assert P.depth.reshape(-1)[at] == F32(2.0)


def test_reference_range_rounding_and_mask_corners():
    zn, zf = F32(0.5), F32(8.0)
    below, above = np.nextafter(zn, F32(0)), np.nextafter(zf, F32(np.inf))
    pts = np.array([[0, 0, zn], [0, 0, zf], [0, 0, below], [0, 0, above], [0, 0, -1.0], [np.nan, 0, 1], [0, np.inf, 1]], dtype=F32)
    P = CR.project(pts, W64, H64, K64, np.eye(4), footprint=1, z_near=zn, z_far=zf)
    assert P.takes_part.tolist() == [True, True, False, False, False, False, False]
    assert P.z.tolist() == [0.5, 8.0, 0, 0, 0, 0, 0] and (P.pixel[2:] == -1).all()
    # px + 0.5 exactly an integer rounds up: px = 10.5 -> u = 11
    K = (64.0, 64.0, 10.5, 7.5)
    P = CR.project(np.array([[0, 0, 1.0]], dtype=F32), W64, H64, K, np.eye(4), footprint=0)
    assert P.pixel[0] == 8 * W64 + 11
    # a centre one pixel outside reaches in with r = 1 and is no candidate; two outside does not reach
    K = (64.0, 64.0, -1.0, 5.0)
    P = CR.project(np.array([[0, 0, 1.0]], dtype=F32), W64, H64, K, np.eye(4), footprint=1)
    assert P.pixel[0] == -1 and P.n_candidates == 0 and (P.zocc[4:7, 0].view(F32) == 1.0).all() and (P.zocc[:, 1] == CR.UNTOUCHED).all()
    P = CR.project(np.array([[0, 0, 1.0]], dtype=F32), W64, H64, (64.0, 64.0, -2.0, 5.0), np.eye(4), footprint=1)
    assert (P.zocc == CR.UNTOUCHED).all()
    # a masked-out row still hides what lies behind it
    mask = np.ones((H64, W64), dtype=F32)
    mask[23, 31] = 0
    pts = np.array([[0, 0, 1.0], [0, 0, 2.0], [1 / 60.0, 0, 2.0]], dtype=F32)
    P = CR.project(pts, W64, H64, (60.0, 60.0, 31.0, 23.0), np.eye(4), footprint=1, mask=mask)
    assert P.pixel.tolist() == [-1, -1, 23 * W64 + 32] and not P.visible.any() and (P.index == -1).all()


def test_reference_bilinear_on_a_linear_image():
    """colour = the linear function at (px, py) within BILINEAR_OPS_BOUND M eps (cloud_image_reference's docstring)"""
    rng = np.random.default_rng(5)
    W, H = 40, 30
    coef = np.array([[0.013, -0.021, 0.4], [-0.017, 0.009, 0.7], [0.02, 0.02, -0.3]])
    xx, yy = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    exact = np.stack([c[0] * xx + c[1] * yy + c[2] for c in coef])
    image = exact.astype(F32)
    px = rng.uniform(0, W - 1, 4000).astype(F32)
    py = rng.uniform(0, H - 1, 4000).astype(F32)
    px[:4], py[:4] = [0, W - 1, 7, 7.5], [0, H - 1, 3.25, 3]      # taps on pixel centres, the last column and row
    got = CR.bilinear(image, px, py).astype(np.float64)
    want = np.stack([c[0] * px.astype(np.float64) + c[1] * py.astype(np.float64) + c[2] for c in coef], axis=1)
    M = float(np.abs(exact).max())
    err = np.abs(got - want).max()
    print(f"bilinear on a linear image: max error {err:.3e}, bound {CR.BILINEAR_OPS_BOUND * M * CR.EPS:.3e}")
    assert err <= CR.BILINEAR_OPS_BOUND * M * CR.EPS
    assert np.array_equal(CR.bilinear(image, px[:2], py[:2]), image[:, [0, H - 1], [0, W - 1]].T)      # exact on pixel centres
    # through project: only visible rows are painted, the others keep what they had
    K = (30.0, 30.0, 19.5, 14.5)
    pts = np.array([[0.01, 0.02, 1.0], [0.01, 0.02, 3.0], [50.0, 0, 1.0]], dtype=F32)
    before = np.full((3, 3), 9.0, dtype=F32)
    P = CR.project(pts, W, H, K, np.eye(4), footprint=1, image=image, colors=before)
    assert P.visible.tolist() == [True, False, False]
    assert np.array_equal(P.colors[1:], before[1:]) and np.array_equal(P.colors[0], CR.bilinear(image, P.px[:1], P.py[:1])[0])


@pytest.mark.parametrize("R", [1, 4, 8])
def test_reference_densify_fills_inside_the_band(R):
    rng = np.random.default_rng(R)
    H, W = 37, 53
    depth = np.where(rng.random((H, W)) < 0.12, rng.uniform(1.0, 1.03, (H, W)), 0).astype(F32)
    depth[:, W // 2:] = np.where(depth[:, W // 2:] > 0, depth[:, W // 2:] * F32(4.0), 0)      # a depth step: 1 m | 4 m
    scale = CR.occlusion_scale(0.05)
    dense, valid, (zn, lo, hi, cnt) = CR.densify(depth, R, scale, 2, details=True)
    kept = depth > 0
    assert np.array_equal(dense[kept], depth[kept]) and (valid[kept] == 1).all()
    filled = ~kept & (valid == 1)
    assert filled.sum() > 100 and (cnt[filled] >= 2).all() and (dense[~kept & (valid == 0)] == 0).all()
    # a weighted mean of the in-band readings: between the smallest and the largest of them (one rounding of slack per sum step)
    slack = 1 + (2 * R + 1) ** 2 * 2.0 ** -23
    assert (dense[filled] >= lo[filled] / slack).all() and (dense[filled] <= hi[filled] * slack).all()
    # foreground first: across the step nothing exceeds zn * band_scale - no mix of 1 m and 4 m
    assert (hi[filled] <= zn[filled] * scale).all() and (dense[filled] <= zn[filled] * scale * F32(slack)).all()
    near_edge = filled & (zn < 2.0)
    assert near_edge[:, W // 2:].any() and (dense[near_edge] < 1.1).all()
    # min_neighbors above what any window holds: only the readings stay
    d2, v2 = CR.densify(depth, R, scale, (2 * R + 1) ** 2)
    assert np.array_equal(d2, depth) and np.array_equal(v2, kept.astype(F32))
    # an empty image and a full one
    z0, v0 = CR.densify(np.zeros((5, 7), F32), R, scale, 1)
    assert not z0.any() and not v0.any()
    full = rng.uniform(0.5, 9.0, (5, 7)).astype(F32)
    z1, v1 = CR.densify(full, R, scale, 1)
    assert np.array_equal(z1.view(np.uint32), full.view(np.uint32)) and v1.all()


def test_reference_densify_by_hand():
    d = np.zeros((3, 3), F32)
    d[0, 0], d[1, 2], d[2, 2] = 2.0, 2.05, 5.0      # corner (w = 1/2), right (w = 1), far corner (out of band)
    dense, valid = CR.densify(d, 1, F32(1.05), 2)
    w0, w1 = F32(1) / F32(2), F32(1) / F32(1)
    want = ((F32(0) + w0 * F32(2.0)) + w1 * F32(2.05)) / ((F32(0) + w0) + w1)
    assert dense[1, 1] == want and valid[1, 1] == 1
    assert CR.densify(d, 1, F32(1.05), 3)[1][1, 1] == 0      # only two in band
