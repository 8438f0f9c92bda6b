"""Camera pose as a differentiable SE(3) correction, and photometric pose refinement against a frozen model.

The rasterizer returns gradients for the camera's `viewmatrix` / `projmatrix` / `campos` when one of them requires grad
(diff_gaussian_rasterization, gsr_backward_camera).  `PoseCamera` derives all three from a base world-to-camera matrix and a leaf
twist `tau` with torch ops, so those gradients reach `tau`; `refine_pose` optimises `tau` against an image (tracking: the map
stays frozen).  Conventions: the matrices are the reference's row-major transposed 4x4 tensors (world_view_transform = W2C^T,
full_proj_transform = (P W2C)^T), and the correction is applied on the left, W2C' = exp(tau) W2C, tau = (rho, theta): rho
a translation and theta a rotation vector, both in the camera frame.

`DevicePoseCamera` / `track_pose` are the same camera and the same optimisation with the pose arithmetic and the optimizer step in
two HIP kernels (csrc/pose.hip) and the state in device memory: a tracking iteration then never crosses to the host."""
from __future__ import annotations

import ctypes as C
import math

import torch

from .cameras import camera_projection, scaled_camera


def _hat(w):
    """[..., 3] -> [..., 3, 3] skew-symmetric matrices (w x v = hat(w) v)."""
    z = torch.zeros_like(w[..., 0])
    return torch.stack([z, -w[..., 2], w[..., 1],
                        w[..., 2], z, -w[..., 0],
                        -w[..., 1], w[..., 0], z], dim=-1).reshape(*w.shape[:-1], 3, 3)


def se3_exp(tau):
    """tau [6] = (rho, theta) -> 4x4 exp of the twist [[hat(theta), rho], [0, 0]] = [[R, V rho], [0, 1]], with
    R = I + A K + B K^2, V = I + B K + C K^2 (K = hat(theta), A = sin t / t, B = (1 - cos t) / t^2, C = (t - sin t) / t^3,
    t = |theta|).  Differentiable, float32 or float64; below a small angle A, B, C come from their Taylor series (no 0 / 0, and
    finite gradients at theta = 0)."""
    rho, theta = tau[:3], tau[3:]
    dt = tau.dtype
    t2 = (theta * theta).sum()
    small = t2 < (1e-6 if dt == torch.float64 else 1e-4)
    t2s = torch.where(small, torch.ones_like(t2), t2)         # (the unused branch of torch.where must stay finite)
    t = torch.sqrt(t2s)
    s, h = torch.sin(t), torch.sin(0.5 * t)
    A = torch.where(small, 1.0 - t2 / 6.0 + t2 * t2 / 120.0, s / t)
    B = torch.where(small, 0.5 - t2 / 24.0 + t2 * t2 / 720.0, 2.0 * h * h / t2s)     # (1 - cos t) = 2 sin^2(t / 2): no cancellation
    C = torch.where(small, 1.0 / 6.0 - t2 / 120.0 + t2 * t2 / 5040.0, (t - s) / (t2s * t))
    K = _hat(theta)
    K2 = K @ K
    eye = torch.eye(3, dtype=dt, device=tau.device)
    R = eye + A * K + B * K2
    V = eye + B * K + C * K2
    top = torch.cat([R, (V @ rho).unsqueeze(1)], dim=1)
    bottom = torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=dt, device=tau.device)
    return torch.cat([top, bottom], dim=0)


def _copy_intrinsics(dst, cam):
    """Image size, FoV, principal-point offsets (a camera without them: centred) and depth range of `cam` onto `dst`."""
    dst.image_width, dst.image_height = int(cam.image_width), int(cam.image_height)
    dst.FoVx, dst.FoVy = float(cam.FoVx), float(cam.FoVy)
    dst.ox, dst.oy = float(getattr(cam, "ox", 0.0)), float(getattr(cam, "oy", 0.0))
    dst.znear, dst.zfar = cam.znear, cam.zfar


class PoseCamera:
    """A camera with the attribute surface `render()` reads (scene_utils.MiniCam, reference scene/cameras.py:74-85) whose
    `world_view_transform`, `full_proj_transform` and `camera_center` are torch functions of a base W2C and the leaf twist
    `tau` (W2C' = exp(tau) W2C): the rasterizer's camera gradients flow into `tau.grad`.  Built from any camera with that
    surface; `dtype` / `device` choose where it lives (float64 on the CPU drives the oracle with the same object)."""

    def __init__(self, cam, dtype=None, device=None, requires_grad=True):
        wv = cam.world_view_transform
        dtype = dtype or wv.dtype
        device = torch.device(device) if device is not None else wv.device
        self.image_name = getattr(cam, "image_name", "")
        self.base_w2c = wv.detach().to(dtype=dtype, device=device).transpose(0, 1).contiguous()
        self.set_intrinsics(cam)
        self.tau = torch.zeros(6, dtype=dtype, device=device, requires_grad=requires_grad)

    def set_intrinsics(self, cam):
        """Points this pose camera at the image size and projection of `cam` (any camera object: another pyramid level, say);
        the pose - base_w2c, tau - and whatever optimizes it stay as they are."""
        _copy_intrinsics(self, cam)
        self.proj_T = camera_projection(self).transpose(0, 1).to(dtype=self.base_w2c.dtype, device=self.base_w2c.device)
        return self

    def w2c(self):
        """The corrected world-to-camera matrix exp(tau) W2C (4x4, column-vector convention)."""
        return se3_exp(self.tau) @ self.base_w2c

    @property
    def world_view_transform(self):
        return self.w2c().transpose(0, 1).contiguous()

    @property
    def full_proj_transform(self):
        return (self.w2c().transpose(0, 1) @ self.proj_T).contiguous()

    @property
    def camera_center(self):
        T = self.w2c()
        return -(T[:3, :3].transpose(0, 1) @ T[:3, 3])          # -R^T t (rigid: no general inverse)

    def commit(self):
        """Folds tau into the base pose and zeroes it (the pose is unchanged; an optimizer over `tau` keeps the same leaf)."""
        with torch.no_grad():
            self.base_w2c = (se3_exp(self.tau) @ self.base_w2c).contiguous()
            self.tau.zero_()
        return self


def pose_error(w2c_a, w2c_b):
    """(rotation angle in radians, camera-centre distance) between two 4x4 world-to-camera matrices."""
    Ra, Rb = w2c_a[:3, :3].double(), w2c_b[:3, :3].double()
    ca = -(Ra.transpose(0, 1) @ w2c_a[:3, 3].double())
    cb = -(Rb.transpose(0, 1) @ w2c_b[:3, 3].double())
    cos = ((Ra @ Rb.transpose(0, 1)).trace() - 1.0) * 0.5
    return float(torch.arccos(cos.clamp(-1.0, 1.0))), float((ca - cb).norm())


def _level_plan(iters, levels, level_iters):
    """[(level, iterations)] from the coarsest level down to 0: `level_iters` (a sequence indexed by level) or `iters` at level 0
    and iters // 2 at every coarser one."""
    levels = int(levels)
    if levels < 0:
        raise ValueError(f"levels={levels}: expected an integer >= 0")
    if level_iters is None:
        level_iters = [int(iters)] + [int(iters) // 2] * levels
    level_iters = [int(n) for n in level_iters]
    if len(level_iters) != levels + 1 or min(level_iters) < 0:
        raise ValueError(f"level_iters={level_iters}: expected {levels + 1} counts >= 0, one per level from 0 up")
    return [(l, level_iters[l]) for l in range(levels, -1, -1)]


def _target_pyramid(pc, gt_image, gt_depth, mask, levels):
    """The targets of a coarse-to-fine run: scene_utils.frames.FramePyramid (HIP) of the image, the depth and the mask.  Its
    cameras are snapshots of `pc`'s intrinsics per level (level 0 too: `pc` itself is re-pointed while the levels run)."""
    from .frames import Frame, FramePyramid
    H, W = gt_image.shape[-2:]
    return FramePyramid(Frame(gt_image.detach().float().reshape(3, H, W), None if gt_depth is None else gt_depth.reshape(H, W),
                              None if mask is None else mask.detach().float().reshape(H, W), scaled_camera(pc, 0)), levels)


def refine_pose(cam, model, gt_image, iters=100, lr=3e-3, lr_final=1.5e-4, lambda_dssim=0.0, bg=None, pipe=None,
                separate_sh=False, callback=None, gt_depth=None, depth_weight=0.5, alpha_min=0.5, levels=0, level_iters=None,
                mask=None):
    """Photometric (or RGB-D) pose refinement of one camera against a frozen `model` (tracking): Adam over the twist of a `PoseCamera`,
    loss = L1(render, gt_image) (lambda_dssim > 0: the fused L1 + D-SSIM training loss), learning rate decaying
    exponentially from `lr` to `lr_final`.  `cam`: a PoseCamera (refined in place) or any camera (wrapped in a float64 PoseCamera
    on the host: the pose arithmetic is a few dozen 4x4 operations, cheaper there than as many device launches; the rasterizer
    moves the three matrices to the device and returns their gradients where they came from).  The model's tensors are read,
    never written; whether they require grad does not matter.  Returns (the PoseCamera with tau committed, the loss of every
    iteration).

    RGB-D tracking: `gt_depth` [1,H,W] or [H,W], the sensor's view-space z-depth (0 = no reading).  Every iteration then renders
    ONCE with depth="z", alpha=True and minimises (1 - depth_weight) L_rgb + depth_weight mean|(D_z - gt_depth) valid|, the mean
    over all pixels (the form of the reference's Ll1depth, train.py:130; no count is read back), valid = (gt_depth > 0) &
    (A > alpha_min): pixels with a reading that the map covers (the mask is not differentiated).  gt_depth=None: the photometric
    loss alone, exactly as before.

    `mask` [H,W] or [1,H,W] (a Frame's validity mask): multiplies `valid` and goes to render() as `alpha_mask` for the colour
    loss.  `levels` = L > 0: coarse to fine over the FramePyramid of the targets - the same loop at level L, then L - 1 ... 0, the
    camera re-pointed with set_intrinsics(scaled_camera(cam, l)), a fresh Adam and the learning-rate schedule restarted at every
    level; `level_iters[l]` iterations at level l (default: `iters` at level 0, iters // 2 above); the losses of all levels are
    returned in the order they ran.  levels=0 is the single-level loop, unchanged."""
    from gaussian_renderer import PipelineParams
    if gt_depth is not None:
        if not 0.0 <= float(depth_weight) <= 1.0:
            raise ValueError(f"depth_weight={depth_weight}: expected a value in [0, 1]")
        gt_depth = gt_depth.detach().float().reshape(1, *gt_image.shape[-2:]).contiguous()
    pc = cam if isinstance(cam, PoseCamera) else PoseCamera(cam, dtype=torch.float64, device="cpu")
    pipe = pipe or PipelineParams()
    if bg is None:
        bg = torch.zeros(3, dtype=torch.float32, device=gt_image.device)
    kw = dict(lr=lr, lr_final=lr_final, lambda_dssim=lambda_dssim, bg=bg, pipe=pipe, separate_sh=separate_sh, callback=callback,
              depth_weight=depth_weight, alpha_min=alpha_min)
    if levels == 0 and level_iters is None:
        history = _refine_level(pc, model, gt_image, gt_depth, mask, iters, **kw)
        return pc.commit(), history
    plan = _level_plan(iters, levels, level_iters)
    pyr = _target_pyramid(pc, gt_image, gt_depth, mask, int(levels))
    history = []
    try:
        for l, n in plan:
            f = pyr[l]
            pc.set_intrinsics(f.camera)
            history += _refine_level(pc, model, f.image, None if gt_depth is None else f.depth.reshape(1, *f.depth.shape),
                                     None if mask is None else f.mask, n, **kw)
    finally:
        pc.set_intrinsics(pyr[0].camera)
    return pc.commit(), history


def _refine_level(pc, model, gt_image, gt_depth, mask, iters, lr, lr_final, lambda_dssim, bg, pipe, separate_sh, callback,
                  depth_weight, alpha_min):
    """refine_pose's loop at one image size: a fresh torch Adam over pc.tau, `iters` iterations; -> the losses."""
    from gaussian_renderer import render
    from .losses import l1_loss, training_loss_fused
    if gt_depth is not None:
        from fused_ssim import l1_mean_loss
        has_reading = gt_depth > 0
        if mask is not None:
            has_reading = has_reading & (mask.reshape(gt_depth.shape) > 0)
    mkw = {} if mask is None else dict(alpha_mask=mask)
    opt = torch.optim.Adam([pc.tau], lr=lr)
    gamma = math.exp(math.log(lr_final / lr) / max(1, iters - 1)) if iters > 1 else 1.0
    history = []
    for it in range(iters):
        opt.zero_grad(set_to_none=True)
        if gt_depth is None:
            image = render(pc, model, pipe, bg, separate_sh=separate_sh, **mkw)["render"]
            loss = training_loss_fused(image, gt_image, lambda_dssim) if lambda_dssim > 0 else l1_loss(image, gt_image)
        else:
            pkg = render(pc, model, pipe, bg, separate_sh=separate_sh, depth="z", alpha=True, **mkw)
            valid = (has_reading & (pkg["alpha"].detach() > alpha_min)).float()
            loss = l1_mean_loss(pkg["depth"], gt_depth, float(depth_weight), valid)
            if depth_weight < 1.0:
                image = pkg["render"]
                rgb = training_loss_fused(image, gt_image, lambda_dssim) if lambda_dssim > 0 else l1_loss(image, gt_image)
                loss = loss + (1.0 - float(depth_weight)) * rgb
        loss.backward()
        opt.step()
        for g in opt.param_groups:
            g["lr"] *= gamma
        history.append(float(loss.detach()))
        if callback is not None:
            callback(it, pc)
    return history


class _DevicePose(torch.autograd.Function):
    """(tau; the camera) -> (world_view_transform, full_proj_transform, camera_center), float32: ONE gsr_pose_forward launch for
    the three tensors, ONE gsr_pose_backward launch for their three gradients (a missing one is NULL = zero).  With the camera's
    Adam state armed (track_pose) that launch also takes the optimizer step on tau, and tau gets no .grad."""

    @staticmethod
    def forward(ctx, tau, cam):
        from diff_gaussian_rasterization import _C
        dev = tau.device
        view = torch.empty(4, 4, dtype=torch.float32, device=dev)
        proj = torch.empty(4, 4, dtype=torch.float32, device=dev)
        center = torch.empty(3, dtype=torch.float32, device=dev)
        with _C.on_device(dev):
            _C.check(_C.lib().gsr_pose_forward(_C.ptr(cam.base_w2c), _C.ptr(tau), _C.ptr(cam.proj_T), _C.ptr(view), _C.ptr(proj),
                                               _C.ptr(center), _C._stream()))
        ctx.cam = cam
        ctx.base = cam.base_w2c              # (commit() replaces the attribute: this graph keeps the matrix it was built from)
        ctx.set_materialize_grads(False)
        return view, proj, center

    @staticmethod
    def backward(ctx, g_view, g_proj, g_center):
        from diff_gaussian_rasterization import _C
        cam = ctx.cam
        tau = cam.tau
        dev = tau.device

        def f32(g):
            return None if g is None else g.to(dtype=torch.float32, device=dev).contiguous()
        g_view, g_proj, g_center = f32(g_view), f32(g_proj), f32(g_center)
        adam = cam._adam
        grad = None if adam is not None else torch.empty(6, dtype=torch.float64, device=dev)
        with _C.on_device(dev):
            _C.check(_C.lib().gsr_pose_backward(_C.ptr(ctx.base), _C.ptr(tau), _C.ptr(cam.proj_T), _C.ptr(g_view),
                                                _C.ptr(g_proj), _C.ptr(g_center), _C.ptr(grad), _C.ptr(adam), _C._stream()))
        if adam is not None:
            cam._cache = None                # (tau was stepped by the kernel: autograd's version counter did not see it)
        return grad, None


class DevicePoseCamera:
    """`PoseCamera` with the pose state - `base_w2c`, `proj_T` and the leaf twist `tau` - in float64 DEVICE memory and the
    arithmetic in two HIP kernels (gsr_pose_forward / gsr_pose_backward): same attribute surface, same conventions.  The three
    transform properties come from one autograd Function evaluated once per value of `tau` (cached on tau's version counter), so
    a render() costs one small launch for the pose and its backward one more; `tau.grad` arrives as float64 on the device.  Works
    with any loss and any torch optimizer over `tau`; `track_pose` additionally folds the Adam step into the backward launch.
    There is no CPU path: a camera on the CPU needs `device=` (GsrError otherwise)."""

    def __init__(self, cam, device=None, requires_grad=True):
        from diff_gaussian_rasterization import _C
        wv = cam.world_view_transform
        device = torch.device(device) if device is not None else wv.device
        if device.type != "cuda":
            raise _C.GsrError("DevicePoseCamera keeps the pose on the HIP device (no CPU path): pass device='cuda' or a camera "
                              "whose tensors are there - PoseCamera is the host form")
        self.image_name = getattr(cam, "image_name", "")
        base = getattr(cam, "base_w2c", None)
        if base is not None and hasattr(cam, "w2c"):          # a PoseCamera / DevicePoseCamera: its corrected pose, in full precision
            with torch.no_grad():
                base = cam.w2c().detach()
        else:
            base = wv.detach().transpose(0, 1)
        self.base_w2c = base.to(dtype=torch.float64, device=device).contiguous()
        self._cache = None         # (tau version, grad mode, the three tensors)
        self.set_intrinsics(cam)
        self.tau = torch.zeros(6, dtype=torch.float64, device=device, requires_grad=requires_grad)
        self._adam = None          # device Adam state (gsr_pose_adam) while track_pose drives this camera

    def set_intrinsics(self, cam):
        """Points this pose camera at the image size and projection of `cam` (any camera object: another pyramid level, say).
        base_w2c, tau and the Adam state stay; the cached transforms are dropped."""
        _copy_intrinsics(self, cam)
        self.proj_T = camera_projection(self).transpose(0, 1).to(dtype=torch.float64, device=self.base_w2c.device).contiguous()
        self._cache = None
        return self

    def _transforms(self):
        key = (self.tau._version, torch.is_grad_enabled() and self.tau.requires_grad)
        if self._cache is None or self._cache[0] != key:
            self._cache = (key, _DevicePose.apply(self.tau, self))
        return self._cache[1]

    def w2c(self):
        """The corrected world-to-camera matrix exp(tau) W2C (4x4 float64 on the device; torch ops, not on the per-iteration
        path)."""
        return se3_exp(self.tau) @ self.base_w2c

    @property
    def world_view_transform(self):
        return self._transforms()[0]

    @property
    def full_proj_transform(self):
        return self._transforms()[1]

    @property
    def camera_center(self):
        return self._transforms()[2]

    def commit(self):
        """Folds tau into the base pose and zeroes it (once per frame: torch ops)."""
        with torch.no_grad():
            self.base_w2c = (se3_exp(self.tau) @ self.base_w2c).contiguous()
            self.tau.zero_()
        self._cache = None
        return self


def _pose_adam_state(device, lr, lr_decay, betas=(0.9, 0.999), eps=1e-8):
    """gsr_pose_adam in device memory, as a float64 tensor of its eighteen 8-byte words (moments and step zero)."""
    from diff_gaussian_rasterization import _C
    st = _C.gsr_pose_adam()
    st.lr, st.beta1, st.beta2, st.eps, st.lr_decay, st.step = float(lr), float(betas[0]), float(betas[1]), float(eps), \
        float(lr_decay), 0
    assert C.sizeof(st) == 8 * _C.POSE_ADAM_WORDS
    host = torch.frombuffer(bytearray(bytes(st)), dtype=torch.float64)
    return host.to(device)


def track_pose(cam, model, gt_image, iters=100, lr=3e-3, lr_final=1.5e-4, lambda_dssim=0.0, bg=None, pipe=None,
               separate_sh=False, gt_depth=None, depth_weight=0.5, alpha_min=0.5, levels=0, level_iters=None, mask=None):
    """`refine_pose` with the host taken out of the loop: same loss, masks, Adam and learning-rate schedule, the pose in a
    `DevicePoseCamera`.  Every iteration is gsr_pose_forward, render(..., camera_only=True) (with depth="z", alpha=True for
    RGB-D), the loss, its backward - the rasterizer's camera-only backward returns the three camera gradients and nothing per
    Gaussian - and gsr_pose_backward with the Adam step on tau, the learning-rate decay and the step count folded into that
    launch.  Nothing is copied to the host inside the loop: each loss is written into its slot of a device tensor.  The one host
    wait left is the forward's own instance-count check: the frames are rendered with forward_mode="exact", because a truncated
    unverified frame would hand Adam exact-zero gradients.  `cam`: a DevicePoseCamera (refined in place) or any camera (wrapped;
    its tensors, or `gt_image`, say which device).  Returns (the DevicePoseCamera with tau committed, losses: a DEVICE tensor
    [iters], float32 - read it once, after the loop).  No `callback`: `refine_pose` stays for callers that need one.
    `levels`, `level_iters`, `mask`: coarse-to-fine tracking and a Frame's validity mask, as in refine_pose (a fresh device Adam
    state per level; `losses` then holds every level's, coarsest first)."""
    from diff_gaussian_rasterization import _C
    from gaussian_renderer import PipelineParams
    if not torch.is_tensor(gt_image) or not gt_image.is_cuda:
        raise _C.GsrError("track_pose runs on the HIP device (no CPU path): gt_image must be a device tensor - refine_pose is "
                          "the host form")
    if gt_depth is not None:
        if not 0.0 <= float(depth_weight) <= 1.0:
            raise ValueError(f"depth_weight={depth_weight}: expected a value in [0, 1]")
        gt_depth = gt_depth.detach().float().reshape(1, *gt_image.shape[-2:]).contiguous()
    pc = cam if isinstance(cam, DevicePoseCamera) else DevicePoseCamera(cam, device=gt_image.device)
    pipe = pipe or PipelineParams()
    if bg is None:
        bg = torch.zeros(3, dtype=torch.float32, device=gt_image.device)
    kw = dict(lr=lr, lr_final=lr_final, lambda_dssim=lambda_dssim, bg=bg, pipe=pipe, separate_sh=separate_sh,
              depth_weight=depth_weight, alpha_min=alpha_min)
    if levels == 0 and level_iters is None:
        losses = _track_level(pc, model, gt_image, gt_depth, mask, iters, **kw)
        return pc.commit(), losses
    plan = _level_plan(iters, levels, level_iters)
    pyr = _target_pyramid(pc, gt_image, gt_depth, mask, int(levels))
    losses = []
    try:
        for l, n in plan:
            f = pyr[l]
            pc.set_intrinsics(f.camera)
            losses.append(_track_level(pc, model, f.image, None if gt_depth is None else f.depth.reshape(1, *f.depth.shape),
                                       None if mask is None else f.mask, n, **kw))
    finally:
        pc.set_intrinsics(pyr[0].camera)
    return pc.commit(), torch.cat(losses)


def _track_level(pc, model, gt_image, gt_depth, mask, iters, lr, lr_final, lambda_dssim, bg, pipe, separate_sh, depth_weight,
                 alpha_min):
    """track_pose's loop at one image size: a fresh device Adam state, `iters` iterations; -> the losses (device tensor)."""
    from gaussian_renderer import render
    from .losses import l1_loss, training_loss_fused
    if gt_depth is not None:
        from fused_ssim import l1_mean_loss
        has_reading = gt_depth > 0
        if mask is not None:
            has_reading = has_reading & (mask.reshape(gt_depth.shape) > 0)
    gamma = math.exp(math.log(lr_final / lr) / max(1, iters - 1)) if iters > 1 else 1.0
    losses = torch.zeros(iters, dtype=torch.float32, device=gt_image.device)
    pc._adam = _pose_adam_state(pc.tau.device, lr, gamma)
    pc._cache = None
    kw = dict(separate_sh=separate_sh, camera_only=True, forward_mode="exact")
    if mask is not None:
        kw["alpha_mask"] = mask
    try:
        for it in range(iters):
            if gt_depth is None:
                image = render(pc, model, pipe, bg, **kw)["render"]
                loss = training_loss_fused(image, gt_image, lambda_dssim) if lambda_dssim > 0 else l1_loss(image, gt_image)
            else:
                pkg = render(pc, model, pipe, bg, depth="z", alpha=True, **kw)
                valid = (has_reading & (pkg["alpha"].detach() > alpha_min)).float()
                loss = l1_mean_loss(pkg["depth"], gt_depth, float(depth_weight), valid)
                if depth_weight < 1.0:
                    image = pkg["render"]
                    rgb = training_loss_fused(image, gt_image, lambda_dssim) if lambda_dssim > 0 else l1_loss(image, gt_image)
                    loss = loss + (1.0 - float(depth_weight)) * rgb
            loss.backward()                      # ... -> gsr_backward_camera_only -> gsr_pose_backward (+ Adam on tau)
            losses[it].copy_(loss.detach().reshape(()))
    finally:
        pc._adam = None
        pc._cache = None
    return losses
