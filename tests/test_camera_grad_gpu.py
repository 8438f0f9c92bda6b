"""Camera gradients of the rasterizer backward (gsr_backward_camera): dL/dviewmatrix, dL/dprojmatrix, dL/dcampos against the
float64 oracle's autograd on the same settings tensors; the SE(3) chain through scene_utils.PoseCamera; bit identity of every
per-Gaussian gradient with and without the camera form; the tracking form (map frozen); photometric pose refinement."""
import math

import pytest
import torch

from helpers import leaf_inputs, settings_for, upstream_grads, rel_l2
from oracle import gs_oracle as O
from scene_utils import make_gaussians, fibonacci_cameras, look_at_camera, PoseCamera, se3_exp, refine_pose, pose_error
from scene_utils.model import GaussianModel

pytestmark = pytest.mark.gpu

CAM_REL = 1e-4      # the suite's stated bar (test_parity_gpu.check_grads): rel-L2 and max-abs / max|g| per tensor
VIEW_ZERO = [3, 7, 11, 15]     # column 3 of dL/dviewmatrix (storage index 4 r + 3)
PROJ_ZERO = [2, 6, 10, 14]     # column 2 of dL/dprojmatrix


def small_scene(P=3000, W=150, H=100, deg=3, seed=11, scale=0.6, view=1):
    """tests/test_parity_gpu.small_scene's recipe."""
    raw = make_gaussians(P, deg, seed=seed, scale_factor=scale)
    cam = fibonacci_cameras(3, W, H, seed=5)[view]
    return raw, cam


def clamp_camera(W=150, H=100):
    """Close to the cloud (box 1.3): many visible Gaussians lie beyond the 1.3 tanfov clamp of the EWA Jacobian."""
    return look_at_camera((1.9, 0.8, 0.6), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 0.6911, W, H)


def _gauss_kw(inp, mode, cov):
    kw = dict(shs=inp.get("shs"), colors_precomp=inp.get("colors_precomp"), dc=inp.get("dc"))
    if cov:
        kw["cov3D_precomp"] = inp["cov3D_precomp"]
    else:
        kw.update(scales=inp["scales"], rotations=inp["rotations"])
    return kw


def _inputs(raw, dtype, device, mode, cov, raw_act):
    inp = leaf_inputs(raw, dtype, device, mode)
    if raw_act:         # the model's raw parameters; the oracle applies the activations itself
        for k, v in (("opacities", raw.opacity), ("scales", raw.scaling), ("rotations", raw.rotation)):
            inp[k] = v.detach().to(device=device, dtype=dtype).clone().requires_grad_(True)
    if cov:
        c = O.cov3d_from_scale_rot(inp["scales"].detach().cpu().double(), inp["rotations"].detach().cpu().double(), 1.0)
        inp["cov3D_precomp"] = c.to(device=device, dtype=dtype).requires_grad_(True)
    return inp


def cam_leaves(cam, dtype, device):
    return [t.detach().to(device=device, dtype=dtype).clone().requires_grad_(True)
            for t in (cam.world_view_transform, cam.full_proj_transform, cam.camera_center)]


def oracle_camera_grads(raw, cam, mode="sh", aa=False, cov=False, raw_act=False, depth=True, deg=3, dtype=torch.float64):
    inp = _inputs(raw, dtype, "cpu", mode, cov, raw_act)
    vm, pm, cp = cam_leaves(cam, dtype, "cpu")
    s = settings_for(cam, deg, torch.tensor([0.2, 0.5, 0.7]), 1.0, aa)._replace(viewmatrix=vm, projmatrix=pm, campos=cp)
    kw = dict(shs=inp.get("shs"), colors_precomp=inp.get("colors_precomp"))
    if mode == "dc":
        kw["shs"] = torch.cat([inp["dc"], inp["shs"]], dim=1)
    op, sc, rot = inp["opacities"], inp.get("scales"), inp.get("rotations")
    if raw_act:
        op, sc, rot = torch.sigmoid(op), torch.exp(sc), torch.nn.functional.normalize(rot)
    if cov:
        kw["cov3D_precomp"] = inp["cov3D_precomp"]
    else:
        kw.update(scales=sc, rotations=rot)
    color, radii, invd = O.rasterize(inp["means3D"], inp["means2D"], op, s, **kw)
    gc, gd = upstream_grads(cam.image_height, cam.image_width)
    loss = (color * gc.to(dtype)).sum()
    if depth:
        loss = loss + (invd * gd.to(dtype)).sum()
    loss.backward()
    # (colors_precomp: campos is not in the oracle's graph at all - its gradient is zero)
    return [torch.zeros_like(t) if t.grad is None else t.grad for t in (vm, pm, cp)], radii


def hip_call(raw, cam, mode="sh", aa=False, cov=False, raw_act=False, depth=True, deg=3, camera=True, gauss_grad=True,
             fold=None, leaves=None):
    """One forward + backward through GaussianRasterizer on cuda.  -> (camera grads or None, per-Gaussian grads dict)"""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    inp = _inputs(raw, torch.float32, "cuda", mode, cov, raw_act)
    if not gauss_grad:
        inp = {k: v.detach() for k, v in inp.items()}
    if leaves is None:
        leaves = cam_leaves(cam, torch.float32, "cuda") if camera else \
            [t.to("cuda") for t in (cam.world_view_transform, cam.full_proj_transform, cam.camera_center)]
    vm, pm, cp = leaves
    s = settings_for(cam, deg, torch.tensor([0.2, 0.5, 0.7]), 1.0, aa, cls=GaussianRasterizationSettings,
                     device="cuda")._replace(viewmatrix=vm, projmatrix=pm, campos=cp)
    kw = _gauss_kw(inp, mode, cov)
    if raw_act:
        kw["raw_activations"] = True
    color, radii, invd = GaussianRasterizer(s)(means3D=inp["means3D"], means2D=inp["means2D"], opacities=inp["opacities"],
                                               fold=fold, **kw)
    gc, gd = upstream_grads(cam.image_height, cam.image_width)
    loss = (color * gc.cuda()).sum()
    if depth:
        loss = loss + (invd * gd.cuda()).sum()
    loss.backward()
    torch.cuda.synchronize()
    cg = [None if t.grad is None else t.grad.detach().cpu() for t in leaves] if camera and all(t.is_leaf for t in leaves) \
        else None
    grads = {k: (None if v.grad is None else v.grad.detach().cpu()) for k, v in inp.items()}
    return cg, grads


def check_camera(out, ref, rel=CAM_REL):
    for name, g, r in zip(("viewmatrix", "projmatrix", "campos"), out, ref):
        assert g is not None, f"no gradient for {name}"
        assert g.shape == r.shape and g.dtype == torch.float32
        e = rel_l2(g, r)
        m = float((g.double() - r).abs().max() / (r.abs().max() + 1e-30))
        assert e <= rel and m <= rel, (name, e, m)
    assert torch.all(out[0].flatten()[VIEW_ZERO] == 0) and torch.all(out[1].flatten()[PROJ_ZERO] == 0)
    assert torch.all(ref[0].flatten()[VIEW_ZERO] == 0) and torch.all(ref[1].flatten()[PROJ_ZERO] == 0)


@pytest.mark.parametrize("mode,aa,cov,raw_act,depth", [
    ("sh", False, False, False, True), ("sh", True, False, False, True), ("dc", False, False, False, True),
    ("dc", True, False, False, False), ("colors", False, False, False, True), ("colors", True, False, False, True),
    ("sh", False, True, False, True), ("sh", False, False, True, True), ("sh", False, False, False, False)])
def test_camera_grads_match_float64_oracle(mode, aa, cov, raw_act, depth):
    """Fails on a rasterizer without camera gradients: the settings' tensors then get no .grad."""
    raw, cam = small_scene()
    ref, _ = oracle_camera_grads(raw, cam, mode, aa, cov, raw_act, depth)
    out, _ = hip_call(raw, cam, mode, aa, cov, raw_act, depth)
    check_camera(out, ref)
    if mode == "colors":        # no view-dependent colour: the camera centre takes no gradient
        assert torch.all(out[2] == 0)


def test_camera_grads_with_clamped_gaussians():
    """A view whose visible Gaussians include many beyond the 1.3 tanfov clamp (the Jacobian then uses the clamped tx / ty)."""
    raw, _ = small_scene()
    cam = clamp_camera()
    ref, radii = oracle_camera_grads(raw, cam)
    vm = cam.world_view_transform.double()
    t = raw.xyz.double() @ vm[:3, :3] + vm[3, :3]
    lim = 1.3 * math.tan(cam.FoVx * 0.5)
    clamped = ((t[:, 0] / t[:, 2]).abs() > lim) & (radii > 0) & (t[:, 2] > 0.2)
    assert int(clamped.sum()) >= 20, int(clamped.sum())
    out, _ = hip_call(raw, cam)
    check_camera(out, ref)


def test_pose_twist_chain_matches_oracle():
    """dL/dtau through PoseCamera on the device against the same PoseCamera driving the float64 oracle on the CPU."""
    raw, cam = small_scene()
    tau0 = torch.tensor([0.01, -0.02, 0.015, 0.004, -0.006, 0.003], dtype=torch.float64)
    res = []
    for dev, dt in (("cpu", torch.float64), ("cuda", torch.float32)):
        pc = PoseCamera(cam, dtype=dt, device=dev)
        with torch.no_grad():
            pc.tau.copy_(tau0.to(dt))
        if dev == "cpu":
            inp = _inputs(raw, dt, dev, "sh", False, False)
            s = settings_for(pc, 3, torch.tensor([0.2, 0.5, 0.7]))
            color, _, invd = O.rasterize(inp["means3D"], inp["means2D"], inp["opacities"], s, shs=inp["shs"],
                                         scales=inp["scales"], rotations=inp["rotations"])
            gc, gd = upstream_grads(cam.image_height, cam.image_width)
            ((color * gc.to(dt)).sum() + (invd * gd.to(dt)).sum()).backward()
        else:
            hip_call(raw, pc, leaves=[pc.world_view_transform, pc.full_proj_transform, pc.camera_center])
        res.append(pc.tau.grad.detach().cpu())
    ref, out = res
    assert rel_l2(out, ref) <= CAM_REL, (out, ref)
    assert float((out.double() - ref).abs().max() / ref.abs().max()) <= CAM_REL


def test_per_gaussian_grads_bit_identical_and_deterministic():
    raw, cam = small_scene()
    for mode, aa in (("sh", False), ("dc", True), ("colors", False)):
        cam_a, ga = hip_call(raw, cam, mode, aa)
        cam_b, gb = hip_call(raw, cam, mode, aa)
        _, g0 = hip_call(raw, cam, mode, aa, camera=False)
        for k in g0:
            assert torch.equal(ga[k], g0[k]), (mode, k)      # means2D included
        for x, y in zip(cam_a, cam_b):
            assert torch.equal(x, y)


def test_tracking_form_frozen_map():
    """Only tau is a leaf: the backward runs, the Gaussians get no .grad, and dL/dtau equals (bitwise) the one of the call where
    every Gaussian tensor requires grad too."""
    raw, cam = small_scene()
    taus = []
    for gauss_grad in (False, True):
        pc = PoseCamera(cam, dtype=torch.float32, device="cuda")
        _, grads = hip_call(raw, pc, gauss_grad=gauss_grad,
                            leaves=[pc.world_view_transform, pc.full_proj_transform, pc.camera_center])
        if not gauss_grad:
            assert all(g is None for g in grads.values())
        taus.append(pc.tau.grad.detach().cpu())
    assert torch.equal(taus[0], taus[1]) and float(taus[0].abs().max()) > 0


def test_empty_and_facing_away_give_zero_camera_grads():
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    raw, cam = small_scene()
    # a camera outside the cloud looking away from it: nothing visible
    away = look_at_camera((4.0, 0.0, 0.0), (8.0, 0.0, 0.0), (0.0, 0.0, 1.0), 0.6911, 150, 100)
    for P in (0, 3000):
        c = cam if P == 0 else away
        pc = PoseCamera(c, dtype=torch.float32, device="cuda")
        inp = leaf_inputs(raw, torch.float32, "cuda", "sh")
        inp = {k: v.detach()[:P] for k, v in inp.items()}
        s = settings_for(c, 3, torch.tensor([0.2, 0.5, 0.7]), cls=GaussianRasterizationSettings, device="cuda")._replace(
            viewmatrix=pc.world_view_transform, projmatrix=pc.full_proj_transform, campos=pc.camera_center)
        color, radii, invd = GaussianRasterizer(s)(inp["means3D"], inp["means2D"], inp["opacities"], shs=inp["shs"],
                                                   scales=inp["scales"], rotations=inp["rotations"])
        assert int((radii > 0).sum()) == 0
        (color.sum() + invd.sum()).backward()
        torch.cuda.synchronize()
        assert pc.tau.grad is not None and torch.all(pc.tau.grad == 0), (P, pc.tau.grad)


def test_fused_optimizer_fold_falls_back_with_camera_leaf():
    from diff_gaussian_rasterization import BackwardFold, FusedAdam
    raw, cam = small_scene()
    params = [raw.xyz, raw.features_dc, raw.features_rest, raw.opacity, raw.scaling, raw.rotation]
    names = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
    ts = [p.detach().cuda().clone().requires_grad_(True) for p in params]
    opt = FusedAdam([{"params": [t], "lr": 1e-3, "name": n} for t, n in zip(ts, names)], lr=0.0, eps=1e-15)
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    outs = []
    for use_fold in (True, False):
        for t in ts:
            t.grad = None
        vm, pm, cp = cam_leaves(cam, torch.float32, "cuda")
        s = settings_for(cam, 3, torch.tensor([0.2, 0.5, 0.7]), cls=GaussianRasterizationSettings, device="cuda")._replace(
            viewmatrix=vm, projmatrix=pm, campos=cp)
        fold = BackwardFold(optimizer=opt) if use_fold else None
        m2d = torch.zeros(ts[0].shape[0], 3, device="cuda", requires_grad=True)
        color, _, invd = GaussianRasterizer(s)(ts[0], m2d, ts[3], dc=ts[1], shs=ts[2], scales=ts[4], rotations=ts[5],
                                               raw_activations=True, fold=fold)
        gc, gd = upstream_grads(cam.image_height, cam.image_width)
        ((color * gc.cuda()).sum() + (invd * gd.cuda()).sum()).backward()
        torch.cuda.synchronize()
        if use_fold:
            assert fold.optimizer_taken is False
        outs.append([t.grad.detach().cpu() for t in ts] + [vm.grad.cpu(), pm.grad.cpu(), cp.grad.cpu()])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_refine_pose_converges():
    """Photometric tracking of one perturbed camera (1 deg rotation, 2 % of the camera distance in translation) against a frozen
    20 k-Gaussian model rendered at the true pose.  Measured once (MI355X): see the thresholds below."""
    raw = make_gaussians(20000, 3, seed=4, scale_factor=0.35)
    cam = fibonacci_cameras(4, 256, 192, seed=2, device="cuda")[1]
    model = GaussianModel.from_raw(raw.to("cuda"), requires_grad=False)
    from gaussian_renderer import render, PipelineParams
    bg = torch.zeros(3, device="cuda")
    with torch.no_grad():
        gt = render(cam, model, PipelineParams(), bg)["render"].detach().clone()
    true_w2c = cam.world_view_transform.transpose(0, 1).double()
    dist = float(cam.camera_center.norm())
    axis = torch.tensor([0.3, -0.8, 0.5], dtype=torch.float64)
    tdir = torch.tensor([0.6, 0.2, -0.77], dtype=torch.float64)
    delta = torch.cat([0.02 * dist * tdir / tdir.norm(), math.radians(1.0) * axis / axis.norm()])
    pc = PoseCamera(cam, dtype=torch.float64, device="cpu")          # (refine_pose's own choice for a plain camera)
    true_w2c = true_w2c.cpu()
    pc.base_w2c = se3_exp(delta) @ true_w2c
    r0, t0 = pose_error(pc.w2c().detach(), true_w2c)
    pc, hist = refine_pose(pc, model, gt, iters=150)
    r1, t1 = pose_error(pc.w2c().detach(), true_w2c)
    print(f"pose refinement: rotation {math.degrees(r0):.4f} -> {math.degrees(r1):.3e} deg, translation {t0:.5f} -> {t1:.3e}, "
          f"loss {hist[0]:.5f} -> {hist[-1]:.3e}")
    # measured once (MI355X): rotation 0.9998 -> 0.0 deg (below what arccos resolves), translation 0.0800 -> 3.80e-5 (2100x),
    # L1 0.0378 -> 2.07e-4.  Thresholds: the 10x the feature promises, and absolute bounds with wide margin (0.01 deg, 2e-3).
    assert r1 <= r0 / 10 and t1 <= t0 / 10, (r0, r1, t0, t1)
    assert math.degrees(r1) <= 1e-2 and t1 <= 2e-3, (math.degrees(r1), t1)
