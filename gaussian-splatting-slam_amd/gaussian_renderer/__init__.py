"""`render()` with the contract of reference `gaussian_renderer/__init__.py:18-121`, calling the MI355X-native
rasterizer.  Same arguments, same branches (python-vs-native covariance / SH, `separate_sh`, `override_color`,
`use_trained_exp`), same returned keys; `"depth"` (the inverse-depth image the reference computes at :90,:101
and `train.py:126` reads) is returned as an additional key.
"""
import math

import torch

from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer, RasterOptions, check_options
from scene_utils.sh import eval_sh


class PipelineParams:
    """Fields of reference arguments/__init__.py:65-71."""

    def __init__(self, convert_SHs_python=False, compute_cov3D_python=False, debug=False, antialiasing=False):
        self.convert_SHs_python = convert_SHs_python
        self.compute_cov3D_python = compute_cov3D_python
        self.debug = debug
        self.antialiasing = antialiasing


class RenderPackage(dict):
    """The dict `render()` returns.  `"visibility_filter"` (= `radii > 0`, reference :118-121) is computed when it is first
    looked at - by key, or by anything that enumerates the dict - instead of in every call: a training step whose
    densification statistics ride in the rasterizer's backward never reads it, and the launch is ~1 % of a 1080p step."""

    def _fill(self):
        if not dict.__contains__(self, "visibility_filter"):
            dict.__setitem__(self, "visibility_filter", dict.__getitem__(self, "radii") > 0)

    def __getitem__(self, key):
        if key == "visibility_filter":
            self._fill()
        return dict.__getitem__(self, key)


def _filled(name):
    def method(self, *a, **k):
        self._fill()
        return getattr(dict, name)(self, *a, **k)
    method.__name__ = name
    return method


for _name in ("get", "__contains__", "keys", "items", "values", "__iter__", "__len__", "__repr__", "copy", "__eq__", "pop"):
    setattr(RenderPackage, _name, _filled(_name))

_zeros = {}


def _screenspace_zeros(like):
    """A fresh leaf of zeros for every call (its .grad is what the callers read, reference :26-30) on top of ONE zero buffer
    per shape: the rasterizer never reads or writes its values, so the fill kernel of `torch.zeros_like` per call buys
    nothing."""
    key = (tuple(like.shape), like.dtype, like.device)
    z = _zeros.get(key)
    if z is None:
        _zeros.clear()
        z = _zeros[key] = torch.zeros_like(like, requires_grad=False)
    return z.detach().requires_grad_(True)


def render(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, scaling_modifier=1.0, separate_sh=False,
           override_color=None, use_trained_exp=False, depth="inverse", alpha=False, n_touched=False, touched_T_min=0.5,
           alpha_mask=None, **rasterizer_kw):
    """`rasterizer_kw`: per-call extensions of this rasterizer, the keywords of `GaussianRasterizer.forward` (`fold`, `sh_ready_event`,
    `forward_mode`, `camera_only` - tracking against a frozen map: the backward returns the camera's gradients alone);
    none given = the reference's call forms, unchanged.  `depth="z"`: the `"depth"` key holds the view-space
    z-depth sum_i w_i z_i instead of the inverse depth; `alpha=True`: the package gains `"alpha"`, the accumulated opacity
    1 - T_final [1,H,W] - both from the same single rasterization, both differentiable.  `n_touched=True`: the package gains
    `"n_touched"`, int32 [P]: for every Gaussian the number of pixels that blend it while their transmittance before it is
    > `touched_T_min` (GaussianRasterizer.forward; scene_utils.keyframes turns it into keyframe and pruning decisions).
    `alpha_mask` ([1,H,W] or [H,W] float32, the camera's mask of train.py:109-111): `"render"` is multiplied by it, in the same
    launch as the `use_trained_exp` exposure (scene_utils.exposure; with `use_trained_exp=False` the exposure is the identity).
    The mask is not differentiated."""
    # (validated here, once, before any device work: neither the model nor the camera is touched for a bad option)
    opts = check_options(RasterOptions(depth=depth, alpha=alpha, n_touched=n_touched, touched_T_min=touched_T_min,
                                       **rasterizer_kw))
    # zero tensor that receives the screen-space (NDC) gradient of the 2-D means (reference :26-30)
    # (a leaf here: its .grad is what the callers read; the reference's `+ 0` / retain_grad() pair gives the same .grad at
    # the price of one more launch per step)
    screenspace_points = _screenspace_zeros(pc.get_xyz)

    tanfovx = math.tan(viewpoint_camera.FoVx * 0.5)
    tanfovy = math.tan(viewpoint_camera.FoVy * 0.5)
    raster_settings = GaussianRasterizationSettings(
        image_height=int(viewpoint_camera.image_height),
        image_width=int(viewpoint_camera.image_width),
        tanfovx=tanfovx,
        tanfovy=tanfovy,
        bg=bg_color,
        scale_modifier=scaling_modifier,
        viewmatrix=viewpoint_camera.world_view_transform,
        projmatrix=viewpoint_camera.full_proj_transform,
        sh_degree=pc.active_sh_degree,
        campos=viewpoint_camera.camera_center,
        prefiltered=False,
        debug=pipe.debug,
        antialiasing=pipe.antialiasing,
    )
    rasterizer = GaussianRasterizer(raster_settings=raster_settings)

    means3D = pc.get_xyz
    means2D = screenspace_points

    scales = rotations = cov3D_precomp = None
    # A model that hands out its RAW parameters (scene_utils.model.GaussianModel.get_raw_geometry) lets the rasterizer apply
    # exp / normalize / sigmoid inside its projection kernel (and chain them in its backward): no activation kernels at all
    # in the step.  Any other model object goes through the reference's getters.
    raw = getattr(pc, "get_raw_geometry", None)
    use_raw = raw is not None and not pipe.compute_cov3D_python
    if use_raw:
        scales, rotations, opacity = raw()
    else:
        opacity = pc.get_opacity
        if pipe.compute_cov3D_python:
            cov3D_precomp = pc.get_covariance(scaling_modifier)
        else:
            scales = pc.get_scaling
            rotations = pc.get_rotation

    shs = colors_precomp = dc = None
    if override_color is None:
        if pipe.convert_SHs_python:
            shs_view = pc.get_features.transpose(1, 2).view(-1, 3, (pc.max_sh_degree + 1) ** 2)
            dir_pp = pc.get_xyz - viewpoint_camera.camera_center.repeat(pc.get_features.shape[0], 1)
            dir_pp_normalized = dir_pp / dir_pp.norm(dim=1, keepdim=True)
            sh2rgb = eval_sh(pc.active_sh_degree, shs_view, dir_pp_normalized)
            colors_precomp = torch.clamp_min(sh2rgb + 0.5, 0.0)
        elif separate_sh:
            dc, shs = pc.get_features_dc, pc.get_features_rest
        else:
            shs = pc.get_features
    else:
        colors_precomp = override_color

    # (dc is None unless separate_sh: the reference's two call forms are one here)
    out = rasterizer.forward_with(opts._replace(raw_activations=True) if use_raw else opts, means3D, means2D, opacity, shs,
                                  colors_precomp, scales, rotations, cov3D_precomp, dc)
    rendered_image, radii, depth_image = out[:3]

    if use_trained_exp or alpha_mask is not None:
        # (reference :141-144 and the alpha-mask multiply of train.py:109-111: one HIP launch, csrc/exposure.hip)
        from scene_utils.exposure import render_exposure
        rendered_image = render_exposure(rendered_image, pc, viewpoint_camera, use_trained_exp, alpha_mask)

    pkg = RenderPackage({"render": rendered_image,
                         "viewspace_points": screenspace_points,
                         "radii": radii,
                         "depth": depth_image})
    if alpha:
        dict.__setitem__(pkg, "alpha", out[3])
    if n_touched:
        dict.__setitem__(pkg, "n_touched", out[-1])
    return pkg
