"""Dense frame-to-frame RGB-D odometry: the motion between two depth images with colour taken from the same sensor - the hybrid
photometric + depth term of Steinbruecker et al. 2011 / Park et al. 2017, what Open3D offers as compute_rgbd_odometry with the
hybrid Jacobian.  It is the image-grid sibling of the coloured ICP of scene_utils.registration: the same 6-unknown Gauss-Newton
step, the association by projection instead of by search.  Everything runs in HIP (csrc/odometry.hip: gsr_odometry_prepare,
gsr_odometry_update; the exact arithmetic is stated in include/gsr.h); there is no CPU path.  Arguments are validated before any
device work.

The transformation T (float64 [4,4]) takes source-camera coordinates to target-camera coordinates.  With the source the new frame
and the target the last tracked one, `camera_after_odometry(target.camera, T)` is the new frame's camera: the start pose of
scene_utils.pose.track_pose, or a loop-closure edge between two keyframes without clouds, neighbour index or ICP."""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple

import numpy as np
import torch

from . import _args as A
from .cameras import camera_from_intrinsics, camera_intrinsics
from .frames import Frame, FramePyramid, MAX_LEVELS
from .registration import LAMBDA_GEOMETRIC, check_lambda

DEPTH_MIN, DEPTH_MAX, DEPTH_DIFF_MAX = 0.0, 4.0, 0.03      # Open3D's OdometryOption defaults
MAX_ITERATIONS = (20, 10, 5)                               # per level, coarse to fine (Open3D's iteration_number_per_pyramid_level)


class OdometryLevel(NamedTuple):
    intensity: torch.Tensor           # float32 [H,W]: ((r + g) + b) / 3 where the mask is 1, NaN elsewhere
    depth: torch.Tensor               # float32 [H,W]: the depth where valid (depth_min < d <= depth_max), NaN elsewhere
    grad: torch.Tensor | None         # float32 [4,H,W]: dI/dx, dI/dy, dD/dx, dD/dy (Sobel / 8), or None (a source level)
    K: tuple                          # (fx, fy, cx, cy)
    width: int
    height: int


class OdometryResult(NamedTuple):
    transformation: torch.Tensor      # float64 [4,4] on the device: x_target ~ T x_source, in camera coordinates
    fitness: float                    # participating pixels / pixels at level 0, under `transformation`
    inlier_rmse: float                # sqrt(mean squared depth residual of the participants), under `transformation`
    iterations: int                   # updates enqueued over all levels
    status: int                       # of the closing evaluation: 0 = a step could be taken, 1 = n < 6, 2 = a rejected pivot


def _check_depth_range(depth_min, depth_max):
    lo, hi = A.number("depth_min", depth_min), A.number("depth_max", depth_max)
    if math.isnan(lo) or math.isnan(hi) or not hi > lo:
        raise ValueError(f"depth_min={lo}, depth_max={hi}: expected depth_min < depth_max")
    return lo, hi


def _check_depth_diff(depth_diff_max):
    v = A.number("depth_diff_max", depth_diff_max)
    if not v > 0:      # (false for NaN)
        raise ValueError(f"depth_diff_max={v}: expected a value > 0")
    return v


def _check_K(K):
    k = A.k4(K, "K")
    if not all(math.isfinite(v) for v in k) or not (k[0] > 0 and k[1] > 0):
        raise ValueError(f"K={k}: expected finite (fx, fy, cx, cy) with fx, fy > 0")
    return k


def prepare_odometry_level(image, depth, mask, K, depth_min=DEPTH_MIN, depth_max=DEPTH_MAX, gradients=True):
    """gsr_odometry_prepare: `image` [3,H,W], `depth` [H,W] (view-space z) and `mask` ([H,W], 1 = seen; or None) on the HIP device
    -> OdometryLevel: the intensity, the depth with everything outside (depth_min, depth_max] or outside the mask NaN, and - with
    `gradients` - their Sobel derivatives.  One launch.  The source of an update needs no gradients."""
    if not isinstance(image, torch.Tensor) or not image.is_floating_point() or image.dim() != 3 or image.shape[0] != 3 or \
            image.shape[1] < 1 or image.shape[2] < 1:
        raise ValueError(f"image: expected a floating-point [3,H,W] tensor, got {tuple(getattr(image, 'shape', ()))}")
    H, W = int(image.shape[1]), int(image.shape[2])
    if H * W > 0x3FFFFFFF:
        raise ValueError(f"image: {W} x {H} is more than 2^30 - 1 pixels")
    A.tensor(depth, "depth", (H, W), also=(1, H, W), convert=False)
    if mask is not None:
        A.tensor(mask, "mask", (H, W), also=(1, H, W), convert=False)
    k = _check_K(K)
    lo, hi = _check_depth_range(depth_min, depth_max)
    _C = A.gsr()
    if not image.is_cuda or not depth.is_cuda or (mask is not None and not mask.is_cuda):
        raise _C.GsrError("prepare_odometry_level needs image, depth and mask on the HIP device (no CPU path)")
    dev = image.device
    img = image.detach().float().contiguous()
    d = depth.detach().to(dev).float().contiguous()
    m = None if mask is None else mask.detach().to(dev).float().contiguous()
    intensity = torch.empty((H, W), dtype=torch.float32, device=dev)
    out_d = torch.empty((H, W), dtype=torch.float32, device=dev)
    grad = torch.empty((4, H, W), dtype=torch.float32, device=dev) if gradients else None
    with _C.on_device(dev):
        _C.check(_C.lib().gsr_odometry_prepare(W, H, _C.ptr(img), _C.ptr(d), _C.ptr(m), lo, hi, _C.ptr(intensity), _C.ptr(out_d),
                                               _C.ptr(grad), _C._stream()))
    return OdometryLevel(intensity, out_d, grad, k, W, H)


def _check_levels(source_level, target_level):
    """-> the two levels with every plane a contiguous float32 tensor on one HIP device.  Types, sizes, intrinsics and every
    plane's shape first (ValueError / TypeError), then the device (GsrError for a CPU tensor): nothing that has not passed
    reaches a kernel, which reads width x height values of every plane."""
    for lv, name in ((source_level, "source_level"), (target_level, "target_level")):
        if not isinstance(lv, OdometryLevel):
            raise TypeError(f"{name}={lv!r}: expected an OdometryLevel (prepare_odometry_level)")
        for n, v in (("width", lv.width), ("height", lv.height)):
            if not A.is_integer(v) or v < 1:
                raise ValueError(f"{name}.{n}={v!r}: expected an int >= 1")
        if lv.width * lv.height > 0x3FFFFFFF:
            raise ValueError(f"{name}: {lv.width} x {lv.height} is more than 2^30 - 1 pixels")
    s, t = source_level, target_level
    if (s.width, s.height) != (t.width, t.height):
        raise ValueError(f"odometry: source {s.width} x {s.height}, target {t.width} x {t.height}: expected one size")
    Ks, Kt = _check_K(s.K), _check_K(t.K)
    if Ks != Kt:
        raise ValueError(f"odometry: source K {Ks}, target K {Kt}: expected one camera")
    if t.grad is None:
        raise ValueError("odometry: the target level has no gradients (prepare_odometry_level(gradients=True))")
    W, H = int(s.width), int(s.height)
    planes = [(s.intensity, "source_level.intensity", (H, W)), (s.depth, "source_level.depth", (H, W)),
              (t.intensity, "target_level.intensity", (H, W)), (t.depth, "target_level.depth", (H, W)),
              (t.grad, "target_level.grad", (4, H, W))]
    for p, name, shape in planes:
        A.tensor(p, name, shape, f", got {tuple(p.shape) if isinstance(p, torch.Tensor) else type(p).__name__}", convert=False)
    for p, name, _ in planes:
        if not p.is_cuda:
            raise A.gsr().GsrError(f"{name} must live on the HIP device (no CPU path)")
    dev = s.intensity.device
    for p, name, _ in planes:
        if p.device != dev:
            raise ValueError(f"odometry: {name} on {p.device}, source_level.intensity on {dev}: expected one device")
    sI, sD, tI, tD, tg = (p.detach().float().contiguous() for p, _, _ in planes)
    return OdometryLevel(sI, sD, None, Ks, W, H), OdometryLevel(tI, tD, tg, Kt, W, H)


class _Updater:
    """gsr_odometry_update on two fixed levels that _check_levels has passed: the workspace is allocated once"""

    def __init__(self, src, tgt, lam, ddm):
        _C = A.gsr()
        self.src, self.tgt, self.lam, self.ddm = src, tgt, lam, ddm
        self.K = (C.c_double * 4)(*src.K)
        self.dev = src.intensity.device
        with _C.on_device(self.dev):
            self.ws = torch.empty(_C.lib().gsr_odometry_workspace_bytes(src.width, src.height), dtype=torch.uint8, device=self.dev)

    def __call__(self, Td, stats, apply=True):
        _C = A.gsr()
        s, t = self.src, self.tgt
        with _C.on_device(self.dev):
            _C.check(_C.lib().gsr_odometry_update(s.width, s.height, self.K, _C.ptr(s.intensity), _C.ptr(s.depth), _C.ptr(t.intensity),
                                                  _C.ptr(t.depth), _C.ptr(t.grad), self.lam, self.ddm, 1 if apply else 0,
                                                  _C.ptr(Td), _C.ptr(stats), _C.ptr(self.ws), self.ws.numel(), _C._stream()))


def odometry_update(source_level, target_level, transformation, lambda_geometric=LAMBDA_GEOMETRIC, depth_diff_max=DEPTH_DIFF_MAX,
                    apply=True):
    """One Gauss-Newton step of the hybrid term (include/gsr.h gsr_odometry_update) -> (new transformation float64 [4,4] on the
    device, stats float64 [8] on the device: n, fitness, inlier_rmse, status, sum r_D^2, sum r_I^2, 0, 0 - all of the
    transformation that was passed in).  status 1 (n < 6) or 2 (a rejected pivot), or apply=False, return the transformation as
    it was, bit for bit.  No read-back."""
    T = A.transform(transformation)
    lam = check_lambda(lambda_geometric)
    ddm = _check_depth_diff(depth_diff_max)
    source_level, target_level = _check_levels(source_level, target_level)
    dev = source_level.intensity.device
    Td = A.device_T(T, dev)
    stats = torch.zeros(8, dtype=torch.float64, device=dev)
    _Updater(source_level, target_level, lam, ddm)(Td, stats, bool(apply))
    return Td, stats


def _check_iterations(max_iterations):
    try:
        its = list(max_iterations)
    except TypeError:
        raise TypeError(f"max_iterations={max_iterations!r}: expected a sequence of ints, one per level, coarse to fine") from None
    for n in its:
        if not A.is_integer(n):
            raise TypeError(f"max_iterations={max_iterations!r}: expected ints")
    if not 1 <= len(its) <= MAX_LEVELS + 1 or min(its) < 0:
        raise ValueError(f"max_iterations={its}: expected 1 .. {MAX_LEVELS + 1} counts >= 0, one per level, coarse to fine")
    return [int(n) for n in its]


def _as_pyramid(frame, levels, name):
    """a Frame or a FramePyramid -> something indexable by level with at least `levels` + 1 frames"""
    if isinstance(frame, FramePyramid):
        if len(frame) < levels + 1:
            raise ValueError(f"{name}: a pyramid of {len(frame)} levels, max_iterations asks for {levels + 1}")
        return frame
    if not isinstance(frame, Frame):
        raise TypeError(f"{name}={frame!r}: expected a Frame or a FramePyramid")
    if frame.depth is None:
        raise ValueError(f"{name}: the frame has no depth")
    if not (isinstance(frame.image, torch.Tensor) and frame.image.dim() == 3):
        raise ValueError(f"{name}: expected an image of shape [3,H,W]")
    H, W = int(frame.image.shape[-2]), int(frame.image.shape[-1])
    if (W >> levels) < 1 or (H >> levels) < 1:
        raise ValueError(f"{name}: level {levels} of a {W} x {H} image has no pixels")
    return None      # (built by the caller, after every argument has been looked at)


def rgbd_odometry(source, target, init=None, max_iterations=MAX_ITERATIONS, lambda_geometric=LAMBDA_GEOMETRIC, depth_min=DEPTH_MIN,
                  depth_max=DEPTH_MAX, depth_diff_max=DEPTH_DIFF_MAX, check_every=0, relative_rmse=1e-6, relative_fitness=1e-6):
    """The motion between two RGB-D frames of one camera, coarse to fine -> OdometryResult; `transformation` takes source-camera
    coordinates to target-camera coordinates (`init`, None = identity, likewise).

    source, target: each a Frame or a FramePyramid (scene_utils.frames) on the HIP device, same size and intrinsics.
    len(max_iterations) levels are used, listed coarse to fine - the last entry is level 0; a Frame is given a FramePyramid of
    that depth, a pyramid with fewer levels is a ValueError.  Every level's intrinsics are its frame's camera's
    (scaled_camera).  At each level both frames are prepared once (gsr_odometry_prepare) and the level's count of
    gsr_odometry_update steps is enqueued on the transformation, which stays on the device from level to level.
    check_every as in registration_icp: 0 reads nothing back until the end; k > 0 reads fitness and RMSE every k iterations and
    leaves the LEVEL once both moved by less than relative_fitness / relative_rmse since the iteration before.
    fitness, inlier_rmse and status of the result come from one closing apply=False evaluation at level 0."""
    its = _check_iterations(max_iterations)
    levels = len(its) - 1
    T = A.transform(init, "init")
    lam = check_lambda(lambda_geometric)
    lo, hi = _check_depth_range(depth_min, depth_max)
    ddm = _check_depth_diff(depth_diff_max)
    for n, v in (("relative_fitness", relative_fitness), ("relative_rmse", relative_rmse)):
        A.number(n, v, lambda v: math.isfinite(v) and v >= 0, "a finite value >= 0")
    A.integer("check_every", check_every, 0)
    pyr = [_as_pyramid(source, levels, "source"), _as_pyramid(target, levels, "target")]
    base = [p[0] if p is not None else f for p, f in zip(pyr, (source, target))]
    for f, name in zip(base, ("source", "target")):
        if f.depth is None:
            raise ValueError(f"{name}: the frame has no depth")
    size = [(int(f.image.shape[-1]), int(f.image.shape[-2])) for f in base]
    Ks = [camera_intrinsics(f.camera) for f in base]
    if size[0] != size[1] or Ks[0] != Ks[1]:
        raise ValueError(f"rgbd_odometry: source {size[0]} K {Ks[0]}, target {size[1]} K {Ks[1]}: expected one size and one camera")
    _C = A.gsr()
    for f in base:
        if not (isinstance(f.image, torch.Tensor) and f.image.is_cuda):
            raise _C.GsrError("rgbd_odometry needs both frames on the HIP device (no CPU path)")
    pyr = [p if p is not None else FramePyramid(f, levels) for p, f in zip(pyr, (source, target))]
    dev = base[0].image.device
    Td = A.device_T(T, dev)
    iterations = 0
    closing = None
    for level, n in zip(range(levels, -1, -1), its):
        if n == 0 and level != 0:
            continue
        fs, ft = pyr[0][level], pyr[1][level]
        for f, name in ((fs, "source"), (ft, "target")):
            if f.depth is None:
                raise ValueError(f"{name}: level {level} of the pyramid has no depth")
        src = prepare_odometry_level(fs.image, fs.depth, fs.mask, camera_intrinsics(fs.camera), lo, hi, gradients=False)
        tgt = prepare_odometry_level(ft.image, ft.depth, ft.mask, camera_intrinsics(ft.camera), lo, hi, gradients=True)
        update = _Updater(*_check_levels(src, tgt), lam, ddm)      # (a pyramid whose levels disagree in size or K: ValueError)
        stats = torch.zeros((max(n, 1), 8), dtype=torch.float64, device=dev)
        for k in range(n):
            update(Td, stats[k])
            iterations += 1
            if check_every and k >= 1 and (k + 1) % check_every == 0:
                prev, cur = stats[k - 1:k + 1, 1:3].tolist()
                if abs(cur[0] - prev[0]) < relative_fitness and abs(cur[1] - prev[1]) < relative_rmse:
                    break
        if level == 0:
            closing = update
    stats = torch.zeros(8, dtype=torch.float64, device=dev)
    closing(Td, stats, apply=False)
    s = stats.tolist()
    return OdometryResult(Td, s[1], s[2], iterations, int(s[3]))


def camera_after_odometry(target_camera, transformation):
    """The camera of the SOURCE frame, given the target's and the odometry result T (source-camera to target-camera coordinates):
    world-to-camera = T^-1 . W2C_target, the target's intrinsics, size, clip planes and device.  With the source the new frame and
    the target the last tracked one this is the start pose of track_pose."""
    T = A.transform(transformation)
    if T is None:
        raise ValueError("transformation: expected a floating-point [4,4] matrix, got None")
    T = T.detach().cpu().double().numpy()
    if not np.isfinite(T).all():
        raise ValueError("transformation: not finite")
    wv = target_camera.world_view_transform.detach()
    w2c_t = wv.cpu().double().numpy().T
    w2c = np.linalg.inv(T) @ w2c_t
    fx, fy, cx, cy = camera_intrinsics(target_camera)
    return camera_from_intrinsics(fx, fy, cx, cy, int(target_camera.image_width), int(target_camera.image_height), w2c=w2c,
                                  znear=target_camera.znear, zfar=target_camera.zfar, device=wv.device,
                                  name=getattr(target_camera, "image_name", ""))


__all__ = ["OdometryLevel", "OdometryResult", "prepare_odometry_level", "odometry_update", "rgbd_odometry", "camera_after_odometry"]
