"""Pose tracking on the device: the SE(3) kernels (gsr_pose_forward / gsr_pose_backward, csrc/pose.hip) in isolation, the Adam step
folded into the backward launch, the autograd surface of scene_utils.DevicePoseCamera and the loop scene_utils.track_pose.

The reference throughout is the host path that exists already and is not under test: PoseCamera(dtype=float64, device="cpu") with
se3_exp under torch autograd, and torch.optim.Adam."""
import ctypes as C
import math

import pytest
import torch

from helpers import leaf_inputs, settings_for, upstream_grads, rel_l2
from oracle import gs_oracle as O
from scene_utils import make_gaussians, fibonacci_cameras, PoseCamera, se3_exp, refine_pose, pose_error
from scene_utils.model import GaussianModel

pytestmark = pytest.mark.gpu

CAM_REL = 1e-4      # the suite's bar for camera gradients (tests/test_camera_grad_gpu.py)
TWISTS = {
    "zero": (0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
    "chain": (0.01, -0.02, 0.015, 0.004, -0.006, 0.003),          # test_pose_twist_chain_matches_oracle's
    "taylor": (0.3, 0.1, -0.2, 6e-4, 5e-4, -6e-4),                # |theta|^2 = 9.7e-7: the Taylor branch, large translation
    "over": (0.3, 0.1, -0.2, 6e-4 * 1.02, 5e-4 * 1.02, -6e-4 * 1.02),   # just over the threshold
    "large": (0.3, 0.1, -0.2, 0.7, -0.4, 0.9),
}


def _camera():
    return fibonacci_cameras(3, 150, 100, seed=5)[1]


def _host_pose(cam, tau):
    pc = PoseCamera(cam, dtype=torch.float64, device="cpu")
    with torch.no_grad():
        pc.tau.copy_(torch.tensor(tau, dtype=torch.float64))
    return pc


def _device_state(pc):
    """(base_w2c, tau, proj_T) of a host PoseCamera as float64 device tensors: what the kernels take."""
    return (pc.base_w2c.detach().cuda().contiguous(), pc.tau.detach().cuda().contiguous(),
            pc.proj_T.detach().cuda().contiguous())


def _pose_forward(base, tau, proj_T):
    from diff_gaussian_rasterization import _C
    out = torch.full((35,), float("nan"), dtype=torch.float32, device="cuda")
    _C.check(_C.lib().gsr_pose_forward(_C.ptr(base), _C.ptr(tau), _C.ptr(proj_T), out.data_ptr(), out.data_ptr() + 64,
                                       out.data_ptr() + 128, _C._stream()))
    torch.cuda.synchronize()
    return out.cpu()


def _pose_backward(base, tau, proj_T, gv, gp, gc, adam=None, want_grad=True):
    from diff_gaussian_rasterization import _C
    grad = torch.full((6,), float("nan"), dtype=torch.float64, device="cuda") if want_grad else None
    _C.check(_C.lib().gsr_pose_backward(_C.ptr(base), _C.ptr(tau), _C.ptr(proj_T), _C.ptr(gv), _C.ptr(gp), _C.ptr(gc),
                                        _C.ptr(grad), _C.ptr(adam), _C._stream()))
    torch.cuda.synchronize()
    return None if grad is None else grad.cpu()


def _upstream(seed=3):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(4, 4, generator=gen), torch.randn(4, 4, generator=gen), torch.randn(3, generator=gen))


def test_abi_has_the_pose_kernels():
    from diff_gaussian_rasterization import _C
    lib = _C.lib()
    assert lib.gsr_abi_version() == 7
    for n in ("gsr_pose_forward", "gsr_pose_backward", "gsr_backward_camera_only", "gsr_backward_camera_only_ex"):
        assert n in _C.EXPORTS and hasattr(lib, n)
    assert C.sizeof(_C.gsr_pose_adam) == 8 * _C.POSE_ADAM_WORDS


@pytest.mark.parametrize("name", list(TWISTS))
def test_pose_forward_matches_host_float64(name):
    """Each of the 35 float32 outputs within 2^-23 |ref| + 1e-12 of the host float64 result cast to float32: both sides are float64
    with errors near 1e-15, so they can differ only by a rounding flip of the final cast (the absolute term: entries that are
    differences of O(1) values).  At tau = 0 exp is exactly I: bit-equal."""
    pc = _host_pose(_camera(), TWISTS[name])
    with torch.no_grad():
        ref = torch.cat([pc.world_view_transform.flatten(), pc.full_proj_transform.flatten(), pc.camera_center.flatten()])
    ref = ref.float()
    out = _pose_forward(*_device_state(pc))
    assert torch.isfinite(out).all()
    err = (out.double() - ref.double()).abs()
    bound = 2.0 ** -23 * ref.double().abs() + 1e-12
    print(f"{name}: max err / bound {float((err / bound).max()):.3f}, entries that differ {int((out != ref).sum())}")
    assert bool((err <= bound).all()), (out, ref)
    if name == "zero":
        assert torch.equal(out, ref)


@pytest.mark.parametrize("which", ["all", "view", "proj", "center"])
@pytest.mark.parametrize("name", list(TWISTS))
def test_pose_backward_matches_float64_autograd(name, which):
    """dL/dtau of random float32 upstream gradients (all three, and each alone with the others NULL) within rel-L2 1e-9 and max-abs /
    max|g| 1e-9 of float64 autograd through PoseCamera: ~100 float64 operations sit near 1e-13, the bar leaves three orders of
    margin and is five orders below the float32 chain's 1e-4, so it cannot hide a wrong Jacobian term.  Bit-equal over two runs."""
    pc = _host_pose(_camera(), TWISTS[name])
    ups = _upstream()
    use = {"all": (True, True, True), "view": (True, False, False), "proj": (False, True, False),
           "center": (False, False, True)}[which]
    loss = sum((t.double() * g.double()).sum() for t, g, u in
               zip((pc.world_view_transform, pc.full_proj_transform, pc.camera_center), ups, use) if u)
    loss.backward()
    ref = pc.tau.grad.detach()
    base, tau, proj_T = _device_state(pc)
    dev_ups = [g.cuda().contiguous() if u else None for g, u in zip(ups, use)]
    out = _pose_backward(base, tau, proj_T, *dev_ups)
    again = _pose_backward(base, tau, proj_T, *dev_ups)
    assert torch.equal(tau.cpu(), pc.tau.detach())           # (no Adam state: tau is not written)
    e = rel_l2(out, ref)
    m = float((out - ref).abs().max() / ref.abs().max())
    print(f"{name}/{which}: rel-L2 {e:.3e}, max-abs / max|g| {m:.3e}")
    assert float(ref.abs().max()) > 0
    assert e <= 1e-9 and m <= 1e-9, (out, ref)
    assert torch.equal(out.view(torch.int64), again.view(torch.int64))


def test_adam_fold_matches_torch_adam():
    """25 steps over a fixed sequence of synthetic upstream gradients, lr = 3e-3 and lr_decay as refine_pose computes it for
    iters = 25: after every step tau within 1e-9 relative (max-norm) of torch.optim.Adam + the host's lr *= gamma (the backward's
    float64 argument, errors accumulating over 25 steps); the stored step is 25 and the stored lr is bit-equal to the host's
    repeated product - both do the same IEEE multiplications."""
    from diff_gaussian_rasterization import _C
    from scene_utils.pose import _pose_adam_state
    iters, lr, lr_final = 25, 3e-3, 1.5e-4
    gamma = math.exp(math.log(lr_final / lr) / max(1, iters - 1))
    pc = _host_pose(_camera(), TWISTS["chain"])
    opt = torch.optim.Adam([pc.tau], lr=lr)
    base, tau, proj_T = _device_state(pc)
    state = _pose_adam_state("cuda", lr, gamma)
    assert state.dtype == torch.float64 and state.numel() == _C.POSE_ADAM_WORDS and state.is_cuda
    worst = 0.0
    for it in range(iters):
        ups = _upstream(seed=100 + it)
        opt.zero_grad(set_to_none=True)
        sum((t.double() * g.double()).sum() for t, g in
            zip((pc.world_view_transform, pc.full_proj_transform, pc.camera_center), ups)).backward()
        ref_grad = pc.tau.grad.detach().clone()
        opt.step()
        for g in opt.param_groups:
            g["lr"] *= gamma
        # alternate between asking for dL/dtau too and the fold alone (dL_dtau = NULL)
        grad = _pose_backward(base, tau, proj_T, *[g.cuda().contiguous() for g in ups], adam=state, want_grad=it % 2 == 0)
        if grad is not None:
            assert rel_l2(grad, ref_grad) <= 1e-9
        ref_tau, out_tau = pc.tau.detach(), tau.cpu()
        err = float((out_tau - ref_tau).abs().max() / ref_tau.abs().max())
        worst = max(worst, err)
        assert err <= 1e-9, (it, out_tau, ref_tau)
    host = state.cpu()
    print(f"Adam fold: worst relative max-norm error of tau over {iters} steps {worst:.3e}")
    assert int(host.view(torch.int64)[_C.POSE_ADAM_STEP]) == iters
    assert host[_C.POSE_ADAM_LR].item() == opt.param_groups[0]["lr"]          # bit-equal
    assert float(host[:12].abs().max()) > 0


def _hip_through_rasterizer(raw, pc, counts=None):
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    inp = {k: v.detach() for k, v in leaf_inputs(raw, torch.float32, "cuda", "sh").items()}
    s = settings_for(pc, 3, torch.tensor([0.2, 0.5, 0.7]), 1.0, False, cls=GaussianRasterizationSettings,
                     device="cuda")._replace(viewmatrix=pc.world_view_transform, projmatrix=pc.full_proj_transform,
                                             campos=pc.camera_center)
    color, radii, invd = GaussianRasterizer(s)(means3D=inp["means3D"], means2D=inp["means2D"], opacities=inp["opacities"],
                                               shs=inp["shs"], scales=inp["scales"], rotations=inp["rotations"],
                                               camera_only=True)
    gc, gd = upstream_grads(pc.image_height, pc.image_width)
    ((color * gc.cuda()).sum() + (invd * gd.cuda()).sum()).backward()
    torch.cuda.synchronize()


class _Counted:
    """Wraps one bound function of the loaded library and counts its calls."""

    def __init__(self, lib, name):
        self.lib, self.name, self.f, self.n = lib, name, getattr(lib, name), 0

    def __call__(self, *a):
        self.n += 1
        return self.f(*a)

    def __enter__(self):
        setattr(self.lib, self.name, self)
        return self

    def __exit__(self, *exc):
        setattr(self.lib, self.name, self.f)


def test_device_pose_camera_autograd_surface():
    """DevicePoseCamera through the rasterizer on small_scene() with helpers.upstream_grads: tau.grad (float64, on the device)
    within CAM_REL of the float64 oracle driven by a host PoseCamera at the same twist (test_pose_twist_chain_matches_oracle's
    comparison and bar); ONE pose-forward and ONE pose-backward launch per iteration; works with a torch optimizer."""
    from diff_gaussian_rasterization import _C
    from scene_utils import DevicePoseCamera
    raw = make_gaussians(3000, 3, seed=11, scale_factor=0.6)
    cam = _camera()
    tau0 = torch.tensor(TWISTS["chain"], dtype=torch.float64)
    ref_pc = _host_pose(cam, TWISTS["chain"])
    inp = leaf_inputs(raw, torch.float64, "cpu", "sh")
    s = settings_for(ref_pc, 3, torch.tensor([0.2, 0.5, 0.7]))
    color, _, invd = O.rasterize(inp["means3D"], inp["means2D"], inp["opacities"], s, shs=inp["shs"], scales=inp["scales"],
                                 rotations=inp["rotations"])
    gc, gd = upstream_grads(cam.image_height, cam.image_width)
    ((color * gc.double()).sum() + (invd * gd.double()).sum()).backward()
    ref = ref_pc.tau.grad.detach()

    pc = DevicePoseCamera(cam, device="cuda")
    for a in ("image_width", "image_height", "FoVx", "FoVy", "znear", "zfar", "image_name", "tau", "base_w2c", "w2c", "commit",
              "world_view_transform", "full_proj_transform", "camera_center"):
        assert hasattr(pc, a), a
    assert pc.tau.dtype == torch.float64 and pc.tau.is_cuda and pc.base_w2c.dtype == torch.float64 and pc.base_w2c.is_cuda
    with torch.no_grad():
        pc.tau.copy_(tau0.cuda())
    lib = _C.lib()
    opt = torch.optim.SGD([pc.tau], lr=1e-6)
    with _Counted(lib, "gsr_pose_forward") as fw, _Counted(lib, "gsr_pose_backward") as bw:
        _hip_through_rasterizer(raw, pc)
        assert (fw.n, bw.n) == (1, 1), (fw.n, bw.n)
        out = pc.tau.grad
        assert out is not None and out.dtype == torch.float64 and out.is_cuda
        out = out.detach().cpu().clone()
        opt.step()                      # (any torch optimizer: tau changes, the next iteration evaluates the pose again - once)
        opt.zero_grad(set_to_none=True)
        _hip_through_rasterizer(raw, pc)
        assert (fw.n, bw.n) == (2, 2), (fw.n, bw.n)
    e, m = rel_l2(out, ref), float((out - ref).abs().max() / ref.abs().max())
    print(f"dL/dtau through DevicePoseCamera: rel-L2 {e:.3e}, max-abs / max|g| {m:.3e}")
    assert float(ref.abs().max()) > 0 and e <= CAM_REL and m <= CAM_REL, (out, ref)
    # commit(): the pose is unchanged, tau is zero
    before = pc.w2c().detach().cpu()
    pc.commit()
    assert torch.all(pc.tau == 0) and float((pc.w2c().detach().cpu() - before).abs().max()) < 1e-14
    with torch.no_grad():
        host = PoseCamera(cam, dtype=torch.float64, device="cpu")
        host.base_w2c = before
        assert float((pc.world_view_transform.cpu() - host.world_view_transform.float()).abs().max()) < 1e-6


def _perturbed_base(cam):
    """test_refine_pose_converges' perturbation: 1 deg rotation, 2 % of the camera distance in translation."""
    true_w2c = cam.world_view_transform.transpose(0, 1).double().cpu()
    dist = float(cam.camera_center.norm())
    axis = torch.tensor([0.3, -0.8, 0.5], dtype=torch.float64)
    tdir = torch.tensor([0.6, 0.2, -0.77], dtype=torch.float64)
    delta = torch.cat([0.02 * dist * tdir / tdir.norm(), math.radians(1.0) * axis / axis.norm()])
    return se3_exp(delta) @ true_w2c, true_w2c


def _device_camera(cam, base):
    from scene_utils import DevicePoseCamera
    pc = DevicePoseCamera(cam, device="cuda")
    pc.base_w2c = base.to(dtype=torch.float64, device="cuda").contiguous()
    return pc


def test_track_pose_converges():
    """test_refine_pose_converges' scene, perturbation, iteration count and thresholds, through track_pose; `losses` is a device
    tensor of length 150 whose first entry is bit-equal to refine_pose's first loss from the same start (at tau = 0 both paths
    hand the rasterizer identical matrices)."""
    from gaussian_renderer import render, PipelineParams
    from scene_utils import track_pose, DevicePoseCamera
    raw = make_gaussians(20000, 3, seed=4, scale_factor=0.35)
    cam = fibonacci_cameras(4, 256, 192, seed=2, device="cuda")[1]
    model = GaussianModel.from_raw(raw.to("cuda"), requires_grad=False)
    bg = torch.zeros(3, device="cuda")
    with torch.no_grad():
        gt = render(cam, model, PipelineParams(), bg)["render"].detach().clone()
    base, true_w2c = _perturbed_base(cam)
    host = PoseCamera(cam, dtype=torch.float64, device="cpu")
    host.base_w2c = base.clone()
    _, hist = refine_pose(host, model, gt, iters=1)
    pc = _device_camera(cam, base)
    r0, t0 = pose_error(pc.w2c().detach().cpu(), true_w2c)
    out, losses = track_pose(pc, model, gt, iters=150)
    assert out is pc and isinstance(out, DevicePoseCamera) and torch.all(pc.tau == 0) and pc.tau.grad is None
    assert losses.is_cuda and losses.shape == (150,) and losses.dtype == torch.float32
    losses = losses.cpu()
    r1, t1 = pose_error(pc.w2c().detach().cpu(), true_w2c)
    print(f"track_pose: rotation {math.degrees(r0):.4f} -> {math.degrees(r1):.3e} deg, translation {t0:.5f} -> {t1:.3e}, "
          f"loss {float(losses[0]):.5f} -> {float(losses[-1]):.3e}")
    # Thresholds: those of test_refine_pose_converges (which measured 0.9998 -> 0.0 deg, 0.0800 -> 3.80e-5 on the host path);
    # measured on this path (MI355X): rotation 0.9998 -> 0.0 deg, translation 0.0800 -> 3.803e-5, loss 0.03783 -> 2.067e-4
    assert float(losses[0]) == hist[0], (float(losses[0]), hist[0])
    assert r1 <= r0 / 10 and t1 <= t0 / 10, (r0, r1, t0, t1)
    assert math.degrees(r1) <= 1e-2 and t1 <= 2e-3, (math.degrees(r1), t1)


def test_track_pose_rgbd_depth_only_in_a_constant_colour_scene():
    """tests/test_depth_alpha_gpu.py's constant-colour scene at its size, depth_weight = 1.0: depth-only track_pose reduces the
    translation error at least tenfold; a photometric-only run leaves it above half its start."""
    from gaussian_renderer import render, PipelineParams
    from scene_utils import track_pose
    raw = make_gaussians(20000, 3, seed=4, scale_factor=0.35)
    with torch.no_grad():
        raw.features_dc.zero_()
        raw.features_rest.zero_()                   # colour 0.5 everywhere
    cam = fibonacci_cameras(4, 256, 192, seed=2, device="cuda")[1]
    model = GaussianModel.from_raw(raw.to("cuda"), requires_grad=False)
    bg = torch.full((3,), 0.5, device="cuda")
    with torch.no_grad():
        pkg = render(cam, model, PipelineParams(), bg, depth="z", alpha=True)
        gt, gt_depth = pkg["render"].detach().clone(), pkg["depth"].detach().clone()
    assert float((gt - 0.5).abs().max()) < 1e-5           # nothing to see in colour
    base, true_w2c = _perturbed_base(cam)
    pc = _device_camera(cam, base)
    r0, t0 = pose_error(pc.w2c().detach().cpu(), true_w2c)
    pc_d, losses = track_pose(pc, model, gt, iters=150, bg=bg, gt_depth=gt_depth, depth_weight=1.0, alpha_min=0.5)
    r1, t1 = pose_error(pc_d.w2c().detach().cpu(), true_w2c)
    pc_p, _ = track_pose(_device_camera(cam, base), model, gt, iters=150, bg=bg)
    r2, t2 = pose_error(pc_p.w2c().detach().cpu(), true_w2c)
    print(f"constant colour: translation {t0:.5f} -> depth-only {t1:.3e}, photometric {t2:.3e}; rotation {math.degrees(r0):.4f} "
          f"-> {math.degrees(r1):.3e} / {math.degrees(r2):.3e} deg")
    # (the host path measured 0.0800 -> 1.25e-5 depth-only, 0.0802 photometric; measured on this path (MI355X): 0.0800 ->
    # 1.247e-5 depth-only, 8.020e-2 photometric)
    assert losses.is_cuda and losses.shape == (150,)
    assert t1 <= t0 / 10, (t0, t1)
    assert t2 > t0 / 2, (t0, t2)                  # photometric: (almost) no signal


def test_cpu_inputs_raise():
    from diff_gaussian_rasterization import _C
    from scene_utils import DevicePoseCamera, track_pose
    cam = _camera()                  # (its tensors are on the CPU)
    with pytest.raises(_C.GsrError, match="no CPU path"):
        DevicePoseCamera(cam)
    with pytest.raises(_C.GsrError, match="no CPU path"):
        DevicePoseCamera(cam, device="cpu")
    raw = make_gaussians(64, 3, seed=4, scale_factor=0.35)
    model = GaussianModel.from_raw(raw.to("cuda"), requires_grad=False)
    with pytest.raises(_C.GsrError, match="no CPU path"):
        track_pose(cam, model, torch.zeros(3, 100, 150), iters=2)

