"""Camera math for the rasterizer boundary.

Restates (does not import) the conventions of the reference:
  * `utils/graphics_utils.py:38-49`  getWorld2View2     (R is stored transposed, T = w2c translation)
  * `utils/graphics_utils.py:51-71`  getProjectionMatrix (z_sign = +1, w = z_view)
  * `utils/graphics_utils.py:73-77`  fov2focal / focal2fov
  * `scene/cameras.py:63-72,74-85`   world_view_transform = W2C^T, full_proj_transform = W2C^T . P^T,
                                     camera_center = inverse(world_view_transform)[3,:3]
Pinned against the reference's own functions by tests/golden/reference_helpers.npz.
"""
from __future__ import annotations

import math

import numpy as np
import torch


def fov2focal(fov: float, pixels: int) -> float:
    return pixels / (2.0 * math.tan(fov / 2.0))


def focal2fov(focal: float, pixels: int) -> float:
    return 2.0 * math.atan(pixels / (2.0 * focal))


def qvec2rotmat(qvec) -> np.ndarray:
    """COLMAP's quaternion (w, x, y, z) -> rotation matrix, float64 (the reference reads a pose message's rotation through it,
    scene/dataset_readers.py:365); the quaternion is taken as given, not normalised."""
    w, x, y, z = (float(c) for c in qvec)
    return np.array([[1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
                     [2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x],
                     [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y]], dtype=np.float64)


def world_to_view(R: np.ndarray, t: np.ndarray, translate=(0.0, 0.0, 0.0), scale: float = 1.0) -> np.ndarray:
    Rt = np.zeros((4, 4), dtype=np.float64)
    Rt[:3, :3] = np.asarray(R, dtype=np.float64).T
    Rt[:3, 3] = np.asarray(t, dtype=np.float64)
    Rt[3, 3] = 1.0
    c2w = np.linalg.inv(Rt)
    c2w[:3, 3] = (c2w[:3, 3] + np.asarray(translate, dtype=np.float64)) * scale
    return np.linalg.inv(c2w).astype(np.float32)


MAX_PRINCIPAL_OFFSET = 0.25     # largest |ox|, |oy| a camera may have (the EWA guard band is symmetric: DESIGN.md section 4 item 28)


def projection_matrix(znear: float, zfar: float, fovX: float, fovY: float, ox: float = 0.0, oy: float = 0.0,
                      dtype=torch.float32) -> torch.Tensor:
    """`ox`, `oy`: the principal point's offset from the image centre in NDC units, P[0,2] and P[1,2] (zero: the symmetric
    pinhole of the reference, bit for bit)."""
    ty, tx = math.tan(fovY / 2.0), math.tan(fovX / 2.0)
    top, right = ty * znear, tx * znear
    bottom, left = -top, -right
    P = torch.zeros(4, 4, dtype=dtype)
    P[0, 0] = 2.0 * znear / (right - left)
    P[1, 1] = 2.0 * znear / (top - bottom)
    P[0, 2] = (right + left) / (right - left) + ox
    P[1, 2] = (top + bottom) / (top - bottom) + oy
    P[3, 2] = 1.0
    P[2, 2] = zfar / (zfar - znear)
    P[2, 3] = -(zfar * znear) / (zfar - znear)
    return P


class MiniCam:
    """Same attribute surface as reference `scene/cameras.py:74-85` (what `render()` reads:
    `gaussian_renderer/__init__.py:33-46`)."""

    def __init__(self, width, height, fovy, fovx, znear, zfar, world_view_transform, full_proj_transform,
                 image_name: str = "", ox: float = 0.0, oy: float = 0.0, camera_center=None):
        self.image_width = int(width)
        self.image_height = int(height)
        self.FoVy = float(fovy)
        self.FoVx = float(fovx)
        self.znear = znear
        self.zfar = zfar
        # intrinsics in pixels (pixel centres at integer coordinates: u = fx x / z + cx); ox, oy are what the projection
        # matrix carries: ox = (2 cx - (W - 1)) / W.  A camera built from two FoV angles is centred: ox = oy = 0.
        self.ox, self.oy = float(ox), float(oy)
        self.fx, self.fy = fov2focal(self.FoVx, self.image_width), fov2focal(self.FoVy, self.image_height)
        self.cx = 0.5 * (self.image_width * self.ox + self.image_width - 1)
        self.cy = 0.5 * (self.image_height * self.oy + self.image_height - 1)
        # contiguous once, here: the rasterizer wrapper hands raw pointers to the library and would otherwise copy the
        # (transposed-view) matrices on every call
        self.world_view_transform = world_view_transform.contiguous()
        self.full_proj_transform = full_proj_transform.contiguous()
        if camera_center is None:
            camera_center = torch.inverse(world_view_transform.float().cpu())[3][:3].to(world_view_transform.device)
        self.camera_center = camera_center
        self.image_name = image_name

    def to(self, device):
        self.world_view_transform = self.world_view_transform.to(device).contiguous()
        self.full_proj_transform = self.full_proj_transform.to(device).contiguous()
        self.camera_center = self.camera_center.to(device)
        return self


def camera_from_RT(R: np.ndarray, T: np.ndarray, fovx: float, fovy: float, width: int, height: int,
                   znear: float = 0.01, zfar: float = 100.0, device="cpu", name: str = "") -> MiniCam:
    wv = torch.tensor(world_to_view(R, T)).transpose(0, 1)
    proj = projection_matrix(znear, zfar, fovx, fovy).transpose(0, 1)
    full = wv.unsqueeze(0).bmm(proj.unsqueeze(0)).squeeze(0)
    return MiniCam(width, height, fovy, fovx, znear, zfar, wv.to(device), full.to(device), name)


def camera_projection(cam, dtype=torch.float32) -> torch.Tensor:
    """The projection matrix P (not transposed) of any camera object with the attribute surface `render()` reads: its FoV,
    znear / zfar and - where it has them - the principal-point offsets `ox`, `oy` (a camera without them: the symmetric matrix)."""
    return projection_matrix(cam.znear, cam.zfar, cam.FoVx, cam.FoVy, float(getattr(cam, "ox", 0.0)),
                             float(getattr(cam, "oy", 0.0)), dtype=dtype)


def _check_offsets(ox, oy, what):
    if not (abs(ox) <= MAX_PRINCIPAL_OFFSET and abs(oy) <= MAX_PRINCIPAL_OFFSET):
        raise ValueError(f"{what}: principal point offset (ox, oy) = ({ox:.4f}, {oy:.4f}) in NDC units exceeds "
                         f"{MAX_PRINCIPAL_OFFSET}: the rasterizer's covariance guard band is symmetric about the optical axis")


def camera_from_intrinsics(fx: float, fy: float, cx: float, cy: float, width: int, height: int, R=None, T=None, w2c=None,
                           znear: float = 0.01, zfar: float = 100.0, device="cpu", name: str = "") -> MiniCam:
    """A camera from a sensor's K = (fx, fy, cx, cy), in pixels with the centre of pixel (0, 0) at (0, 0) (OpenCV's convention):
    a view-space point projects to u = fx x / z + cx, v = fy y / z + cy.  Pose: `w2c` (4x4 world-to-camera) or the reference's
    pair (R stored transposed, T); neither: the identity.  ValueError when the principal point lies more than
    MAX_PRINCIPAL_OFFSET of the image size off the centre."""
    width, height = int(width), int(height)
    if width < 1 or height < 1 or not (fx > 0 and fy > 0):
        raise ValueError(f"camera_from_intrinsics: size {width} x {height}, focal lengths ({fx}, {fy})")
    ox, oy = (2.0 * cx - (width - 1)) / width, (2.0 * cy - (height - 1)) / height
    _check_offsets(ox, oy, "camera_from_intrinsics")
    if w2c is not None:
        if R is not None or T is not None:
            raise ValueError("camera_from_intrinsics: give w2c or (R, T), not both")
        w2c = w2c.detach().cpu().numpy() if isinstance(w2c, torch.Tensor) else w2c
        w2c = np.asarray(w2c, dtype=np.float64).reshape(4, 4)
        R, T = w2c[:3, :3].T, w2c[:3, 3]
    elif R is None and T is None:
        R, T = np.eye(3), np.zeros(3)
    elif R is None or T is None:
        raise ValueError("camera_from_intrinsics: R and T come together")
    fovx, fovy = focal2fov(fx, width), focal2fov(fy, height)
    wv = torch.tensor(world_to_view(R, T)).transpose(0, 1)
    proj = projection_matrix(znear, zfar, fovx, fovy, ox, oy).transpose(0, 1)
    full = wv.unsqueeze(0).bmm(proj.unsqueeze(0)).squeeze(0)
    cam = MiniCam(width, height, fovy, fovx, znear, zfar, wv.to(device), full.to(device), name, ox=ox, oy=oy)
    cam.fx, cam.fy, cam.cx, cam.cy = float(fx), float(fy), float(cx), float(cy)      # as given, not through atan / tan
    return cam


def camera_intrinsics(cam):
    """(fx, fy, cx, cy) in pixels of any camera object (one without them: derived from its FoV, centred)."""
    W, H = int(cam.image_width), int(cam.image_height)
    fx = getattr(cam, "fx", None)
    if fx is not None:
        return float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy)
    ox, oy = float(getattr(cam, "ox", 0.0)), float(getattr(cam, "oy", 0.0))
    return fov2focal(cam.FoVx, W), fov2focal(cam.FoVy, H), 0.5 * (W * ox + W - 1), 0.5 * (H * oy + H - 1)


def scaled_camera(cam, level: int) -> MiniCam:
    """The camera of pyramid level `level` of `cam`'s image: each level halves the one below and drops a trailing odd row or
    column (W' = W >> level), so the pixel (u, v) of level 0 lies at ((u + 0.5) / 2^level - 0.5, ...) and fx' = fx / 2^level,
    cx' = (cx + 0.5) / 2^level - 0.5.  The pose tensors (world_view_transform, camera_center) are `cam`'s own, detached, not
    copies.  ValueError when a side would reach 0 or the new principal point leaves the +-MAX_PRINCIPAL_OFFSET band."""
    level = int(level)
    W, H = int(cam.image_width), int(cam.image_height)
    if level < 0 or (W >> level) < 1 or (H >> level) < 1:
        raise ValueError(f"scaled_camera: level {level} of a {W} x {H} image has no pixels")
    fx, fy, cx, cy = camera_intrinsics(cam)
    s = float(1 << level)
    W2, H2 = W >> level, H >> level
    fx2, fy2, cx2, cy2 = fx / s, fy / s, (cx + 0.5) / s - 0.5, (cy + 0.5) / s - 0.5
    ox, oy = (2.0 * cx2 - (W2 - 1)) / W2, (2.0 * cy2 - (H2 - 1)) / H2
    _check_offsets(ox, oy, f"scaled_camera level {level}")
    fovx, fovy = focal2fov(fx2, W2), focal2fov(fy2, H2)
    with torch.no_grad():
        wv = cam.world_view_transform.detach()
        center = cam.camera_center.detach()
        proj = projection_matrix(cam.znear, cam.zfar, fovx, fovy, ox, oy).transpose(0, 1).to(dtype=wv.dtype, device=wv.device)
        full = wv @ proj
    out = MiniCam(W2, H2, fovy, fovx, cam.znear, cam.zfar, wv, full, getattr(cam, "image_name", ""), ox=ox, oy=oy,
                  camera_center=center)
    out.fx, out.fy, out.cx, out.cy = fx2, fy2, cx2, cy2
    return out


def look_at_camera(eye, target, up, fovx: float, width: int, height: int, device="cpu", name: str = "") -> MiniCam:
    """COLMAP-style camera (x right, y down, z forward) at `eye` looking at `target`."""
    eye = np.asarray(eye, dtype=np.float64)
    f = np.asarray(target, dtype=np.float64) - eye
    f /= np.linalg.norm(f)
    upv = np.asarray(up, dtype=np.float64)
    if abs(np.dot(f, upv)) > 0.999:                          # looking along `up`: pick another
        upv = np.array([0.0, 1.0, 0.0]) if abs(upv[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    r = np.cross(f, upv)
    r /= np.linalg.norm(r)
    d = np.cross(f, r)                                       # camera "down"
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = r, d, f, eye
    w2c = np.linalg.inv(c2w)
    R = w2c[:3, :3].T                                        # stored transposed (dataset_readers.py:208-209)
    T = w2c[:3, 3]
    fovy = focal2fov(fov2focal(fovx, width), height)         # dataset_readers.py:224
    return camera_from_RT(R, T, fovx, fovy, width, height, device=device, name=name)


def fibonacci_cameras(n_views: int, width: int, height: int, radius: float = 4.0, fovx: float = 0.6911,
                      seed: int = 0, device="cpu"):
    """V cameras on a Fibonacci sphere looking at the origin, up = +z."""
    rng = np.random.default_rng(seed)
    phase = rng.uniform(0.0, 2.0 * math.pi)
    golden = math.pi * (3.0 - math.sqrt(5.0))
    cams = []
    for i in range(n_views):
        z = 1.0 - 2.0 * (i + 0.5) / n_views
        rho = math.sqrt(max(0.0, 1.0 - z * z))
        th = phase + golden * i
        eye = radius * np.array([rho * math.cos(th), rho * math.sin(th), z])
        cams.append(look_at_camera(eye, (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), fovx, width, height,
                                   device=device, name=f"view_{i:04d}"))
    return cams
