"""The mapping half of a SLAM loop: new Gaussians from point clouds (reference scene/gaussian_model.py:130-153 create_from_pcd)
and from RGB-D keyframes (the pixels the map does not explain yet, back-projected and appended to a live, optimised model).
Back-projection / selection (gsr_unproject_rgbd_k) and the neighbour distances that size the new Gaussians (gsr_knn_dist2) run in
HIP (csrc/knn.hip); there is no CPU path."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch
import torch.nn as nn

from . import _args as A
from .model import GaussianModel, _PARAM_ATTRS, _inverse_sigmoid, _replace_params
from .sh import RGB2SH


def _as_tensor(a):
    return a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))


def create_from_pcd(self, points, colors=None, spatial_lr_scale=1.0, anchor=None, voxel_size=None, nb_neighbors=None,
                    std_ratio=2.0):
    """reference scene/gaussian_model.py:130-153.  `points` [P,3] / `colors` [P,3] in [0,1]: tensors or numpy arrays - or, as in
    the reference, one object with `.points` / `.colors` (its BasicPointCloud) as the first argument.  The points decide the
    device: arrays are moved to the HIP device as in the reference, tensors are used where they live and must live there - CPU
    tensors raise, there is no CPU path for the neighbour search.  `anchor`: the keyframe id the rows are labelled with
    (model._anchor, scene_utils.transform; a model that tracks anchors labels them -1 without it).  `voxel_size` /
    `nb_neighbors` (+ `std_ratio`): condition the cloud first - voxel-grid down-sampling and / or the statistical outlier filter
    (scene_utils.pointcloud.condition_point_cloud, the reference's process_point_cloud); None, the default, takes the cloud as it
    is.  Returns the model."""
    if hasattr(points, "points") and hasattr(points, "colors"):
        if colors is not None:                       # (pcd, spatial_lr_scale): the reference's call form
            spatial_lr_scale = colors
        points, colors = points.points, points.colors
    elif colors is None:
        raise TypeError("create_from_pcd(points, colors): colours missing")
    if not isinstance(points, torch.Tensor) and torch.cuda.is_available():
        points = _as_tensor(points).cuda()           # arrays go to the device, as in the reference (:132)
    xyz, rgb = _as_tensor(points), _as_tensor(colors)
    if not xyz.is_cuda:
        raise A.gsr().GsrError("create_from_pcd: points must be on the HIP device (the neighbour search has no CPU path)")
    if voxel_size is not None or nb_neighbors is not None:
        from .pointcloud import condition_point_cloud
        xyz, rgb = condition_point_cloud(xyz, rgb.detach().to(xyz.device).float(), voxel_size, nb_neighbors, std_ratio)
    from simple_knn._C import distCUDA2
    self.spatial_lr_scale = float(spatial_lr_scale)
    dev = xyz.device
    fused_point_cloud = xyz.detach().float().contiguous().clone()
    fused_color = RGB2SH(rgb.detach().to(dev).float())
    P = int(fused_point_cloud.shape[0])
    features = torch.zeros((P, 3, (self.max_sh_degree + 1) ** 2), dtype=torch.float32, device=dev)
    features[:, :3, 0] = fused_color
    dist2 = torch.clamp_min(distCUDA2(fused_point_cloud), 0.0000001)
    scales = torch.log(torch.sqrt(dist2))[..., None].repeat(1, 3)
    rots = torch.zeros((P, 4), dtype=torch.float32, device=dev)
    rots[:, 0] = 1
    opacities = _inverse_sigmoid(0.1 * torch.ones((P, 1), dtype=torch.float32, device=dev))
    self._xyz = nn.Parameter(fused_point_cloud.requires_grad_(True))
    self._features_dc = nn.Parameter(features[:, :, 0:1].transpose(1, 2).contiguous().requires_grad_(True))
    self._features_rest = nn.Parameter(features[:, :, 1:].transpose(1, 2).contiguous().requires_grad_(True))
    self._scaling = nn.Parameter(scales.requires_grad_(True))
    self._rotation = nn.Parameter(rots.requires_grad_(True))
    self._opacity = nn.Parameter(opacities.requires_grad_(True))
    self.max_radii2D = torch.zeros((P,), device=dev)
    self.active_sh_degree = 0
    tracked = anchor is not None or getattr(self, "_anchor", None) is not None
    self._anchor = torch.full((P,), -1 if anchor is None else int(anchor), dtype=torch.int32, device=dev) if tracked else None
    return self


def unproject_rgbd(cam, image, depth, alpha=None, rendered_z=None, stride=1, min_depth=0.2, max_depth=math.inf,
                   alpha_below=0.5, front_margin=0.05):
    """Back-projects the selected pixels of an RGB-D frame into the world: -> (xyz [n,3], rgb [n,3]) in row-major pixel order.
    `image` [3,H,W], `depth` [H,W] or [1,H,W] view-space z.  Of the pixels with x % stride == 0 and y % stride == 0, those with
    a valid reading (finite, min_depth < d <= max_depth) are taken - all of them without `alpha`; with `alpha` (the accumulated
    opacity of the map's render of this view) only where alpha < alpha_below or, given `rendered_z` (the "depth" of a
    render(..., depth="z")) too, where the reading lies in front of the rendered surface: d < rendered_z / alpha - front_margin d.
    One read-back (the count, to slice the outputs)."""
    _C = A.gsr()
    if not (isinstance(depth, torch.Tensor) and depth.is_cuda and isinstance(image, torch.Tensor) and image.is_cuda):
        raise _C.GsrError("unproject_rgbd needs image and depth on the HIP device (no CPU path)")
    H, W = int(cam.image_height), int(cam.image_width)
    if int(stride) < 1:
        raise ValueError(f"stride={stride}: expected an integer >= 1")
    dev = depth.device

    def plane(t, name, n=1):
        if t is None:
            return None
        t = t.detach().float().to(dev).contiguous()
        if t.numel() != n * H * W:
            raise ValueError(f"{name}: {tuple(t.shape)} does not hold {n} x {H} x {W} values")
        return t
    d, col, a, rz = plane(depth, "depth"), plane(image, "image", 3), plane(alpha, "alpha"), plane(rendered_z, "rendered_z")
    view = cam.world_view_transform.detach().float().to(dev).contiguous()
    stride = int(stride)
    cap = ((W + stride - 1) // stride) * ((H + stride - 1) // stride)
    lib = _C.lib()
    # (the principal point travels as the projection matrix's offsets; a camera without them is centred)
    p = _C.gsr_unproject_params_k(_C.gsr_unproject_params(H, W, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5),
                                                          view.data_ptr(), stride, float(min_depth), float(max_depth),
                                                          float(alpha_below), float(front_margin)),
                                  float(getattr(cam, "ox", 0.0)), float(getattr(cam, "oy", 0.0)))
    xyz = torch.empty((cap, 3), dtype=torch.float32, device=dev)
    rgb = torch.empty((cap, 3), dtype=torch.float32, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    with _C.on_device(dev):
        ws = torch.empty(lib.gsr_unproject_workspace_bytes(W, H), dtype=torch.uint8, device=dev)
        _C.check(lib.gsr_unproject_rgbd_k(C.byref(p), _C.ptr(d), _C.ptr(col), _C.ptr(a), _C.ptr(rz), _C.ptr(xyz), _C.ptr(rgb), cap,
                                        _C.ptr(count), _C.ptr(ws), ws.numel(), _C._stream()))
    n = int(count.item())
    return xyz[:n], rgb[:n]


def add_from_rgbd(self, cam, image, depth, render_pkg=None, init_opacity=0.5, scale="knn", anchor=None, voxel_size=None,
                  voxel_origin=None, nb_neighbors=None, std_ratio=2.0, **selection):
    """Appends Gaussians for the pixels of an RGB-D keyframe that the map does not explain; returns how many.  `render_pkg`: the
    result of render(cam, self, ..., depth="z", alpha=True) (None: first keyframe, every valid reading is taken); `selection`:
    the keyword arguments of unproject_rgbd.  New rows: colour -> SH band 0, higher bands 0, identity rotation, opacity
    `init_opacity`, isotropic scale sqrt(mean squared distance to the three nearest points of map + new points)
    (scale="knn") or the footprint of a pixel at the reading's depth, d 2 tanfovx / W stride (scale="pixel", no search).
    With an optimizer attached the old rows keep their Adam moments and the new rows start from zero; xyz_gradient_accum, denom
    and max_radii2D are extended with zeros (the old rows' statistics stay valid).  n == 0 changes nothing.  A model without
    parameters yet (GaussianModel(sh_degree)) is created from the keyframe.  `anchor`: the keyframe id the new rows are labelled
    with in model._anchor, so that a later pose correction of that keyframe can move them (scene_utils.transform); without it
    they get -1 if the model tracks anchors.  `voxel_size` (+ `voxel_origin`: one world-anchored lattice for every keyframe) /
    `nb_neighbors` (+ `std_ratio`): the NEW points are conditioned (scene_utils.pointcloud.condition_point_cloud) before the
    neighbour search that sizes them - one Gaussian per occupied voxel instead of one per pixel, depth-edge flying pixels
    dropped; the map's rows are not touched.  None, the default: every selected pixel becomes a Gaussian."""
    _C = A.gsr()
    if self._xyz is not None and not self._xyz.is_cuda:
        raise _C.GsrError("add_from_rgbd runs in HIP kernels (no CPU path): the model must live on the HIP device")
    if scale not in ("knn", "pixel"):
        raise ValueError(f"scale={scale!r}: expected 'knn' or 'pixel'")
    if not 0.0 < float(init_opacity) < 1.0:
        raise ValueError(f"init_opacity={init_opacity}: expected a value in (0, 1)")
    if voxel_size is not None or nb_neighbors is not None:
        from .pointcloud import check_conditioning
        check_conditioning(voxel_size, voxel_origin, nb_neighbors, std_ratio)
    alpha = rendered_z = None
    if render_pkg is not None:
        if "alpha" not in render_pkg:
            raise ValueError("render_pkg: expected the result of render(..., depth='z', alpha=True)")
        alpha, rendered_z = render_pkg["alpha"], render_pkg["depth"]
    with torch.no_grad():
        xyz, rgb = unproject_rgbd(cam, image, depth, alpha=alpha, rendered_z=rendered_z, **selection)
        if voxel_size is not None or nb_neighbors is not None:
            from .pointcloud import condition_point_cloud
            xyz, rgb = condition_point_cloud(xyz, rgb, voxel_size, nb_neighbors, std_ratio, origin=voxel_origin)
        n = int(xyz.shape[0])
        if n == 0:
            return 0
        for hook in getattr(self, "_resize_hooks", ()):
            hook("before")
        if self._xyz is None:            # an empty model: the first keyframe creates the map
            m = (self.max_sh_degree + 1) ** 2 - 1
            for attr, shape in zip(_PARAM_ATTRS, ((0, 3), (0, 1, 3), (0, m, 3), (0, 1), (0, 3), (0, 4))):
                setattr(self, attr, nn.Parameter(torch.zeros(shape, dtype=torch.float32, device=xyz.device)))
            self.max_radii2D = torch.zeros((0,), device=xyz.device)
        dev, P = self._xyz.device, int(self._xyz.shape[0])
        all_xyz = torch.cat([self._xyz.detach(), xyz.to(dev)], dim=0)
        if scale == "knn":
            from simple_knn._C import knn_dist2
            dist2 = torch.clamp_min(knn_dist2(all_xyz, first_query=P), 0.0000001)
            scales = torch.log(torch.sqrt(dist2))[..., None].repeat(1, 3)
        else:
            w2c_z = cam.world_view_transform.detach().float().to(dev)[:, 2]          # view z = p . column 2 of W2C^T
            z = xyz @ w2c_z[:3] + w2c_z[3]
            px = z * (2.0 * math.tan(cam.FoVx * 0.5) / int(cam.image_width) * int(selection.get("stride", 1)))
            scales = torch.log(px.clamp_min(1e-7))[..., None].repeat(1, 3)
        rest = int(self._features_rest.shape[1])
        rots = torch.zeros((n, 4), dtype=torch.float32, device=dev)
        rots[:, 0] = 1
        new_rows = [xyz.to(dev), RGB2SH(rgb.to(dev)).view(n, 1, 3), torch.zeros((n, rest, 3), dtype=torch.float32, device=dev),
                    _inverse_sigmoid(float(init_opacity) * torch.ones((n, 1), dtype=torch.float32, device=dev)), scales, rots]
        opt = getattr(self, "optimizer", None)
        tensors, moments = [], []
        for attr, rows in zip(_PARAM_ATTRS, new_rows):
            old = getattr(self, attr)
            tensors.append(torch.cat([old.detach(), rows], dim=0).contiguous())
            st = opt.state.get(old, None) if opt is not None else None
            if st and "exp_avg" in st:
                zeros = torch.zeros_like(rows)
                moments.append((torch.cat([st["exp_avg"], zeros], dim=0).contiguous(),
                                torch.cat([st["exp_avg_sq"], zeros], dim=0).contiguous()))
            else:
                moments.append(None)
        _replace_params(self, tensors, moments)
        from .transform import extend_anchors
        extend_anchors(self, P, n, anchor, dev)
        if getattr(self, "xyz_gradient_accum", None) is not None:
            self.xyz_gradient_accum = torch.cat([self.xyz_gradient_accum, torch.zeros((n, 1), device=dev)], dim=0)
            self.denom = torch.cat([self.denom, torch.zeros((n, 1), device=dev)], dim=0)
        if getattr(self, "max_radii2D", None) is not None:
            self.max_radii2D = torch.cat([self.max_radii2D, torch.zeros((n,), device=dev)], dim=0)
        for hook in getattr(self, "_resize_hooks", ()):
            hook("after")
    return n


GaussianModel.create_from_pcd = create_from_pcd
GaussianModel.add_from_rgbd = add_from_rgbd
