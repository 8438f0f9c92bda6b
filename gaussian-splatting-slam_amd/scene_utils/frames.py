"""The front end of a sensor frame: a distorted RGB-D image with its K matrix and distortion coefficients becomes a `Frame` - an
ideal pinhole image, its depth, a validity mask and a camera built from the intrinsics - and a `FramePyramid` of it, whose levels
carry exact intrinsics (scene_utils.cameras.scaled_camera), for coarse-to-fine tracking (scene_utils.pose.track_pose(levels=...)).
Undistortion and the pyramid each run as ONE HIP launch (csrc/frames.hip: gsr_frame_undistort, gsr_frame_pyramid); there is no CPU
path.  Conventions (include/gsr.h): K = (fx, fy, cx, cy) in pixels with the centre of pixel (0, 0) at (0, 0), as in OpenCV;
`dist` = (k1, k2, p1, p2, k3), the Brown-Conrady "plumb_bob" model of a ROS CameraInfo.D; depth is view-space z, 0 = no reading."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _args as A
from .cameras import camera_from_intrinsics, camera_intrinsics, scaled_camera

MAX_LEVELS = 3


def _device_plane(t, name, H, W, n=1):
    t = t.detach().float().contiguous()
    if t.numel() != n * H * W:
        raise ValueError(f"{name}: {tuple(t.shape)} does not hold {n} x {H} x {W} values")
    return t


def undistort(image, depth, K, dist=None, size=None, new_K=None):
    """gsr_frame_undistort: `image` [3,Hs,Ws], `depth` [Hs,Ws] / [1,Hs,Ws] or None, on the HIP device, taken with intrinsics `K`
    and distortion `dist` (None: none) -> (image [3,H,W], depth [H,W] or None, mask [H,W]) of an ideal pinhole camera with
    intrinsics `new_K` (default K) and `size` = (W, H) (default the source's).  Colour is bilinear, depth the nearest reading
    (never blended), mask 1 where the bilinear taps lie inside the source - elsewhere all three are 0."""
    _C = A.gsr()
    if not (isinstance(image, torch.Tensor) and image.is_cuda) or (depth is not None and not (isinstance(depth, torch.Tensor)
                                                                                             and depth.is_cuda)):
        raise _C.GsrError("undistort needs image and depth on the HIP device (no CPU path)")
    if image.dim() != 3 or image.shape[0] != 3:
        raise ValueError(f"image: expected [3,H,W], got {tuple(image.shape)}")
    Hs, Ws = int(image.shape[1]), int(image.shape[2])
    W, H = (Ws, Hs) if size is None else (int(size[0]), int(size[1]))
    dev = image.device
    src = _device_plane(image, "image", Hs, Ws, 3)
    d = None if depth is None else _device_plane(depth.to(dev), "depth", Hs, Ws)
    k_src = (C.c_float * 4)(*A.k4(K, "K"))
    k_dst = None if new_K is None else (C.c_float * 4)(*A.k4(new_K, "new_K"))
    coef = [0.0] * 5 if dist is None else [float(v) for v in np.asarray(
        dist.detach().cpu().numpy() if isinstance(dist, torch.Tensor) else dist, dtype=np.float64).reshape(-1)]
    if len(coef) == 4:
        coef.append(0.0)
    if len(coef) != 5:
        raise ValueError(f"dist: expected (k1, k2, p1, p2[, k3]), got {len(coef)} values")
    color = torch.empty((3, H, W), dtype=torch.float32, device=dev)
    out_d = None if d is None else torch.empty((H, W), dtype=torch.float32, device=dev)
    mask = torch.empty((H, W), dtype=torch.float32, device=dev)
    with _C.on_device(dev):
        _C.check(_C.lib().gsr_frame_undistort(Ws, Hs, _C.ptr(src), _C.ptr(d), k_src, (C.c_float * 5)(*coef), W, H, k_dst,
                                              _C.ptr(color), _C.ptr(out_d), _C.ptr(mask), _C._stream()))
    return color, out_d, mask


def build_pyramid(image, depth, mask, levels, depth_band=0.05):
    """gsr_frame_pyramid: levels 1 .. `levels` of `image` [3,H,W], `depth` [H,W] or None and `mask` [H,W] or None on the HIP device
    -> three lists (None where the input is): each level halves the one below (a trailing odd row or column is dropped); colour
    is the mean of the 2 x 2 quad, depth the mean of the quad's valid readings within `depth_band` (relative) of the nearest one,
    mask the AND of the quad."""
    _C = A.gsr()
    for t in (image, depth, mask):
        if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise _C.GsrError("build_pyramid needs its tensors on the HIP device (no CPU path)")
    levels = int(levels)
    if image.dim() != 3 or image.shape[0] != 3:
        raise ValueError(f"image: expected [3,H,W], got {tuple(image.shape)}")
    H, W = int(image.shape[1]), int(image.shape[2])
    dev = image.device
    img = _device_plane(image, "image", H, W, 3)
    d = None if depth is None else _device_plane(depth.to(dev), "depth", H, W)
    m = None if mask is None else _device_plane(mask.to(dev), "mask", H, W)
    sizes = [(W >> l, H >> l) for l in range(1, max(levels, 0) + 1)]

    def outs(t, n):
        if t is None or not sizes or min(min(s) for s in sizes) < 1:
            return None, None
        ts = [torch.empty(((n, h, w) if n > 1 else (h, w)), dtype=torch.float32, device=dev) for w, h in sizes]
        return ts, (C.c_void_p * len(ts))(*[x.data_ptr() for x in ts])
    (c_out, c_ptr), (d_out, d_ptr), (m_out, m_ptr) = outs(img, 3), outs(d, 1), outs(m, 1)
    if c_ptr is None:          # (no such level: the library's own check words the error)
        c_ptr = d_ptr = m_ptr = (C.c_void_p * 3)()
    with _C.on_device(dev):
        _C.check(_C.lib().gsr_frame_pyramid(W, H, levels, _C.ptr(img), _C.ptr(d), _C.ptr(m), float(depth_band), c_ptr, d_ptr, m_ptr,
                                            _C._stream()))
    return c_out, d_out, m_out


class Frame:
    """One pinhole frame: `image` [3,H,W], `depth` [H,W] (view-space z, 0 = no reading) or None, `mask` [H,W] (1 = the pixel was
    seen by the sensor; what render(alpha_mask=...) and the trackers take) or None, and its `camera`."""

    def __init__(self, image, depth, mask, camera):
        self.image, self.depth, self.mask, self.camera = image, depth, mask, camera

    @classmethod
    def from_sensor(cls, image, depth, K, dist=None, pose=None, size=None, new_K=None, znear=0.01, zfar=100.0, name=""):
        """A frame as the sensor hands it over: `image` [3,Hs,Ws] and `depth` ([Hs,Ws] or None) on the HIP device, `K` (3x3 or
        (fx, fy, cx, cy)), `dist` (k1, k2, p1, p2, k3) or None, `pose` the 4x4 world-to-camera matrix (None: the identity).  One
        undistort launch; the camera is camera_from_intrinsics(new_K or K, size or the source's size)."""
        _C = A.gsr()
        if not (isinstance(image, torch.Tensor) and image.is_cuda):
            raise _C.GsrError("Frame.from_sensor needs the image (and depth) on the HIP device (no CPU path)")
        W, H = (int(image.shape[-1]), int(image.shape[-2])) if size is None else (int(size[0]), int(size[1]))
        fx, fy, cx, cy = A.k4(K if new_K is None else new_K, "K")
        cam = camera_from_intrinsics(fx, fy, cx, cy, W, H, w2c=pose, znear=znear, zfar=zfar, device=image.device, name=name)
        color, d, mask = undistort(image, depth, K, dist, size=(W, H), new_K=new_K)
        return cls(color, d, mask, cam)


class FramePyramid:
    """Levels 0 .. `levels` of a Frame: `pyr[i]` is the Frame of level i (level 0 is the frame itself), its camera
    scaled_camera(frame.camera, i).  One gsr_frame_pyramid launch for all levels."""

    def __init__(self, frame, levels, depth_band=0.05):
        _C = A.gsr()
        if not (isinstance(frame.image, torch.Tensor) and frame.image.is_cuda):
            raise _C.GsrError("FramePyramid needs the frame on the HIP device (no CPU path)")
        levels = int(levels)
        if not 0 <= levels <= MAX_LEVELS:
            raise ValueError(f"levels={levels}: expected 0 .. {MAX_LEVELS}")
        self.levels = levels
        self.frames = [frame]
        if levels == 0:
            return
        H, W = int(frame.image.shape[-2]), int(frame.image.shape[-1])
        if (W >> levels) < 1 or (H >> levels) < 1:
            raise ValueError(f"FramePyramid: level {levels} of a {W} x {H} image has no pixels")
        cams = [scaled_camera(frame.camera, l) for l in range(1, levels + 1)]
        c, d, m = build_pyramid(frame.image, frame.depth, frame.mask, levels, depth_band)
        for i in range(levels):
            self.frames.append(Frame(c[i], None if d is None else d[i], None if m is None else m[i], cams[i]))

    def __len__(self):
        return len(self.frames)

    def __getitem__(self, i):
        return self.frames[i]


__all__ = ["Frame", "FramePyramid", "undistort", "build_pyramid", "camera_intrinsics", "MAX_LEVELS"]
