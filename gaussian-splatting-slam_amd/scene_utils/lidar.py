"""A LiDAR cloud in the colour camera: the step that joins the two sensors of a gs_slam_msgs/visual_merged_msg (Image, CameraInfo,
CameraPose, Local_Map).  The cloud is projected into the image (csrc/cloud_image.hip; the rules: include/gsr.h, gsr_cloud_project
and gsr_depth_densify): a sparse depth image, the row that won each pixel, which rows the camera
sees, the image's colours for those rows - and the sparse depth filled into a dense one, which is what everything built on
Frame.depth takes.  The reference has the message field and no code for this step: parity is self-stated.  Occlusion by a square
footprint is the crude, standard form; hidden-point removal by convex hull and per-beam ray tests are out of scope.  There is no
CPU path."""
from __future__ import annotations

import ctypes as C
import math
from collections import namedtuple

import numpy as np
import torch

from . import _args as A
from .cameras import camera_intrinsics
from .tsdf import _w2c64

MAX_ROWS = (1 << 30) - 1

CloudProjection = namedtuple("CloudProjection", "depth index pixel z visible colors n_visible n_candidates")
CloudProjection.__doc__ = """What project_cloud returns, on the HIP device: `depth` float32 [H,W] (0 = no visible point), `index`
int32 [H,W] (the row seen at the pixel, -1 = none), `pixel` int32 [N] (v W + u of a candidate row, else -1), `z` float32 [N]
(camera-space depth, 0 for a row outside the depth range or not finite), `visible` bool [N], `colors` float32 [N,3] or None (the
image's colour at visible rows), and the two counts as ints."""

_PROJECT_OPTIONS = ("footprint", "occlusion", "z_near", "z_far")
_DENSIFY_OPTIONS = ("radius", "depth_band", "min_neighbors")


def _project_options(footprint, occlusion, z_near, z_far):
    _C = A.gsr()
    r = A.integer("footprint", footprint, 0, _C.CLOUD_MAX_FOOTPRINT)
    occ = A.number("occlusion", occlusion, lambda v: v >= 0 and math.isfinite(v), "a finite value >= 0")
    zn = A.number("z_near", z_near, lambda v: v > 0 and math.isfinite(v), "a finite value > 0")
    zf = A.number("z_far", z_far, lambda v: math.isfinite(v), "a finite value")
    if not float(np.float32(zn)) < float(np.float32(zf)):
        raise ValueError(f"z_far={z_far}: expected a value above z_near={z_near}")
    return r, float(np.float32(1.0 + occ)), zn, zf


def _densify_options(radius, depth_band, min_neighbors):
    _C = A.gsr()
    R = A.integer("radius", radius, 1, _C.DENSIFY_MAX_RADIUS)
    band = A.number("depth_band", depth_band, lambda v: v >= 0 and math.isfinite(v), "a finite value >= 0")
    k = A.integer("min_neighbors", min_neighbors, 1, (1 << 31) - 1)
    return R, float(np.float32(1.0 + band)), k


def _rows64(T, name):
    """a float64 [4,4] numpy matrix -> its rows 0 .. 2 as 12 floats; ValueError unless all are finite"""
    vals = [float(v) for v in np.asarray(T, dtype=np.float64)[:3].reshape(-1)]
    if not all(math.isfinite(v) for v in vals):
        raise ValueError(f"{name}: expected finite values")
    return vals


def _project(points, camera, T, image, mask, options, colors_init=None):
    """project_cloud on a float64 [4,4] numpy cloud-frame -> camera matrix; colors_init: the array the visible rows are painted
    into (None with an image: zeros)"""
    _C = A.gsr()
    r, occ_scale, zn, zf = _project_options(*options)
    W, H = int(camera.image_width), int(camera.image_height)
    if W < 1 or H < 1 or W * H > MAX_ROWS:
        raise ValueError(f"camera: {W} x {H}: expected sides >= 1 and at most 2^30 - 1 pixels")
    K = [float(np.float32(v)) for v in camera_intrinsics(camera)]
    if not all(math.isfinite(v) for v in K) or not (K[0] > 0.0 and K[1] > 0.0):
        raise ValueError(f"camera: (fx, fy, cx, cy) = {tuple(K)}: expected finite values, fx and fy positive")
    rows = _rows64(T, "w2c")
    # every shape first, then the devices
    A.tensor(points, "points", ("N", 3), convert=False)
    if int(points.shape[0]) > MAX_ROWS:
        raise ValueError(f"points: {int(points.shape[0])} rows: at most 2^30 - 1")
    if image is not None:
        A.tensor(image, "image", (3, H, W), convert=False)
    if mask is not None:
        A.tensor(mask, "mask", (H, W), also=(1, H, W), convert=False)
    if colors_init is not None:
        if image is None:
            raise ValueError("colors: nothing to paint them from without an image")
        A.tensor(colors_init, "colors", tuple(int(s) for s in points.shape), convert=False)
    pts = A.tensor(points, "points", ("N", 3))
    dev = pts.device
    img = None if image is None else A.tensor(image, "image", (3, H, W)).to(dev)
    msk = None if mask is None else A.tensor(mask, "mask", (H, W), also=(1, H, W)).to(dev)
    N = int(pts.shape[0])
    colors = None
    if img is not None:
        colors = torch.zeros((N, 3), dtype=torch.float32, device=dev) if colors_init is None else \
            A.tensor(colors_init, "colors", (N, 3)).to(dev).clone()
    depth = torch.empty((H, W), dtype=torch.float32, device=dev)
    index = torch.empty((H, W), dtype=torch.int32, device=dev)
    pixel = torch.empty(N, dtype=torch.int32, device=dev)
    z = torch.empty(N, dtype=torch.float32, device=dev)
    visible = torch.empty(N, dtype=torch.uint8, device=dev)
    count = torch.empty(2, dtype=torch.int64, device=dev)
    cam = _C.gsr_cloud_camera(W, H, (C.c_float * 4)(*K), (C.c_double * 12)(*rows), zn, zf, r, occ_scale)
    lib = _C.lib()
    with _C.on_device(dev):
        ws = torch.empty(lib.gsr_cloud_project_workspace_bytes(W, H), dtype=torch.uint8, device=dev)
        _C.check(lib.gsr_cloud_project(C.byref(cam), N, _C.ptr(pts), _C.ptr(img), _C.ptr(msk), _C.ptr(depth), _C.ptr(index),
                                       _C.ptr(pixel), _C.ptr(z), _C.ptr(visible), _C.ptr(colors), _C.ptr(count), _C.ptr(ws),
                                       ws.numel(), _C._stream()))
    n_visible, n_candidates = (int(v) for v in count.tolist())      # the one read-back
    return CloudProjection(depth, index, pixel, z, visible.view(torch.bool), colors, n_visible, n_candidates)


def project_cloud(points, camera, w2c=None, image=None, mask=None, footprint=2, occlusion=0.05, z_near=0.05, z_far=100.0):
    """gsr_cloud_project: `points` float32 [N,3] on the HIP device, in the frame `camera`'s pose starts from (`w2c`: that pose
    as a float64 [4,4] cloud-frame -> camera matrix where the camera's float32 one is too coarse) -> CloudProjection.  A row takes
    part when its camera-space z lies in [z_near, z_far]; it then hides what lies behind it on the (2 footprint + 1)^2 pixels
    around its own: a row is visible iff its z is at most (1 + occlusion) times the nearest z that reached its pixel.  Per pixel
    the nearest visible row wins (`depth`, `index`).  `mask` [H,W]: rows that land where it is 0 still hide others and are never
    seen themselves.  `image` [3,H,W]: visible rows get its bilinear colour.  Costs one read-back, the two counts."""
    T = _w2c64(camera, w2c)
    return _project(points, camera, T, image, mask, (footprint, occlusion, z_near, z_far))


def densify_depth(depth, radius=4, depth_band=0.05, min_neighbors=2):
    """gsr_depth_densify: a sparse depth image float32 [H,W] on the HIP device (0 = no reading) -> (dense [H,W], valid [H,W],
    float32 1 / 0).  A reading stays; a hole takes the inverse-square-distance weighted mean of the readings of its
    (2 radius + 1)^2 window that lie within `depth_band` (relative) of the nearest one - the foreground, as build_pyramid prefers
    it - if there are at least `min_neighbors` of them, and stays 0 otherwise."""
    _C = A.gsr()
    R, band_scale, k = _densify_options(radius, depth_band, min_neighbors)
    A.tensor(depth, "depth", ("H", "W"), also=(1, "H", "W"), convert=False)
    H, W = int(depth.shape[-2]), int(depth.shape[-1])
    if W < 1 or H < 1 or W * H > MAX_ROWS:
        raise ValueError(f"depth: {W} x {H}: expected sides >= 1 and at most 2^30 - 1 pixels")
    d = A.tensor(depth, "depth", ("H", "W"), also=(1, "H", "W")).reshape(H, W)
    dense, valid = torch.empty_like(d), torch.empty_like(d)
    with _C.on_device(d.device):
        _C.check(_C.lib().gsr_depth_densify(W, H, _C.ptr(d), R, band_scale, k, _C.ptr(dense), _C.ptr(valid), _C._stream()))
    return dense, valid


def _split(options, names, who):
    unknown = sorted(set(options) - set(names))
    if unknown:
        raise TypeError(f"{who}: unexpected option(s) {', '.join(unknown)}")


def _frame_pose(frame, cloud_to_world):
    """the float64 cloud-frame -> camera matrix of a frame: its camera's pose, after cloud_to_world ([4,4], None: the cloud is in
    the world frame already)"""
    T = _w2c64(frame.camera, None)
    M = A.transform(cloud_to_world, "cloud_to_world")
    if M is not None:
        T = T @ np.asarray(M.detach().cpu().numpy(), dtype=np.float64)
    return T


def _project_args(project):
    defaults = dict(footprint=2, occlusion=0.05, z_near=0.05, z_far=100.0)
    defaults.update(project)
    return tuple(defaults[k] for k in _PROJECT_OPTIONS)


def colorize_cloud(points, frame, colors=None, cloud_to_world=None, **project):
    """-> (colors float32 [N,3], visible bool [N]): the rows of `points` that `frame`'s camera sees (project_cloud with the
    frame's mask and the options `project`) painted from frame.image; the others keep their row of `colors`, or are 0 where none
    is given.  Called frame after frame with its own result, it paints one colour array over a whole trajectory."""
    _split(project, _PROJECT_OPTIONS, "colorize_cloud")
    if frame.image is None:
        raise ValueError("colorize_cloud: the frame has no image")
    proj = _project(points, frame.camera, _frame_pose(frame, cloud_to_world), frame.image, frame.mask, _project_args(project),
                    colors_init=colors)
    return proj.colors, proj.visible


def lidar_frame(frame, points, cloud_to_world=None, densify=True, **options):
    """-> (Frame, CloudProjection): `frame` with the depth image that `points` (float32 [N,3] on the HIP device; moved into the
    world frame by `cloud_to_world`, [4,4], None: already there) give in its camera - project_cloud(...).depth, or with
    densify=True densify_depth of it.  The image, mask and camera are the old frame's; the projection carries the rows'
    colours.  `options`: those of project_cloud (footprint, occlusion, z_near, z_far) and of densify_depth (radius, depth_band,
    min_neighbors)."""
    from .frames import Frame
    _split(options, _PROJECT_OPTIONS + _DENSIFY_OPTIONS, "lidar_frame")
    dens = {k: v for k, v in options.items() if k in _DENSIFY_OPTIONS}
    if dens and not densify:
        raise ValueError(f"lidar_frame: {', '.join(sorted(dens))} given with densify=False")
    _densify_options(*({"radius": 4, "depth_band": 0.05, "min_neighbors": 2, **dens}[k] for k in _DENSIFY_OPTIONS))
    proj = _project(points, frame.camera, _frame_pose(frame, cloud_to_world), frame.image, frame.mask,
                    _project_args({k: v for k, v in options.items() if k in _PROJECT_OPTIONS}))
    depth = densify_depth(proj.depth, **dens)[0] if densify else proj.depth
    return Frame(frame.image, depth, frame.mask, frame.camera), proj


def frame_from_visual_merged_map(msg, cloud_to_world=None, decode=None, **kw):
    """gs_slam_msgs/visual_merged_msg with its cloud (anything with .Image, .CameraInfo, .CameraPose and .Local_Map) ->
    (frame, points, colors): frame_from_messages(msg.Image, msg.CameraInfo, msg.CameraPose, ...), decode_pointcloud2(msg.Local_Map,
    **decode), then lidar_frame - a Frame with depth, the decoded cloud, and its colours: painted from the image where the
    camera sees a row, the message's own (0 without a colour field) elsewhere.  `kw`: the options of lidar_frame go there, the
    rest to frame_from_messages.  Message bytes in, everything else on the device; only the counts are read back."""
    from .messages import decode_pointcloud2, frame_from_messages
    try:
        image, info, pose, cloud = msg.Image, msg.CameraInfo, msg.CameraPose, msg.Local_Map
    except AttributeError as e:
        raise TypeError(f"msg: expected .Image, .CameraInfo, .CameraPose and .Local_Map: {e}") from None
    if decode is not None and not isinstance(decode, dict):
        raise TypeError(f"decode={decode!r}: expected a dict of decode_pointcloud2 options")
    decode = dict(decode or {})
    if decode.get("return_index"):
        raise ValueError("decode: return_index is not used here")
    lidar_names = _PROJECT_OPTIONS + _DENSIFY_OPTIONS + ("densify",)
    lidar = {k: v for k, v in kw.items() if k in lidar_names}
    frame = frame_from_messages(image, info, pose, **{k: v for k, v in kw.items() if k not in lidar_names})
    points, msg_colors = decode_pointcloud2(cloud, **decode)[:2]
    frame, proj = lidar_frame(frame, points, cloud_to_world, **lidar)
    colors = proj.colors if msg_colors is None else torch.where(proj.visible[:, None], proj.colors, msg_colors)
    return frame, points, colors


__all__ = ["CloudProjection", "project_cloud", "densify_depth", "colorize_cloud", "lidar_frame", "frame_from_visual_merged_map"]
