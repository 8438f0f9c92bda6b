"""Back-projection of RGB-D keyframes (gsr_unproject_rgbd), GaussianModel.create_from_pcd / add_from_rgbd, and the
track -> insert -> optimise loop they were built for."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import mapping_reference as MR
from scene_utils import (GaussianModel, Trainer, fibonacci_cameras, make_config, make_gaussians, unproject_rgbd, refine_pose,
                         PoseCamera, se3_exp, RGB2SH)

pytestmark = pytest.mark.gpu
U = 2.0 ** -24                # unit roundoff of float32


def keyframe_inputs(cam, seed, invalid_frac=0.02, min_depth=0.2, max_depth=3.0, alpha_below=0.5, front_margin=0.05):
    """depth / colour / alpha / rendered_z [H,W] float32 such that no pixel sits within 1e-3 relative of a selection threshold:
    readings in [1.3, 2.7] or invalid (0, NaN, 1e4), alpha outside 0.5 (1 +- 2e-3), the rendered surface z / A at
    d (1 + front_margin) r with r outside 1 +- 2e-3."""
    H, W = cam.image_height, cam.image_width
    rng = np.random.default_rng(seed)
    depth = MR.depth_sheet(H, W, seed=seed, invalid_frac=invalid_frac)
    color = rng.uniform(size=(3, H, W)).astype(np.float32)
    A = rng.uniform(0.0, 1.0, size=(H, W))
    near = np.abs(A - alpha_below) < 2e-3 * alpha_below
    A[near] = alpha_below * 1.01
    A[rng.uniform(size=(H, W)) < 0.02] = 0.0                      # nothing rendered there at all
    A = A.astype(np.float32)
    r = np.where(rng.uniform(size=(H, W)) < 0.5, rng.uniform(0.8, 0.998, size=(H, W)), rng.uniform(1.002, 1.2, size=(H, W)))
    d_ok = np.where(np.isfinite(depth), depth, 1.0).astype(np.float64)
    z = (d_ok * (1.0 + front_margin) * r * A.astype(np.float64)).astype(np.float32)
    return depth, color, A, z


@pytest.mark.parametrize("stride", [1, 4])
@pytest.mark.parametrize("with_alpha,with_z", [(False, False), (True, False), (False, True), (True, True)])
def test_unproject_matches_the_restatement(stride, with_alpha, with_z):
    W, H = 203, 149                                         # not multiples of the stride or of 16
    cam = fibonacci_cameras(4, W, H, seed=11, device="cuda")[2]
    depth, color, A, z = keyframe_inputs(cam, seed=5 + stride)
    sel = dict(stride=stride, min_depth=0.2, max_depth=3.0, alpha_below=0.5, front_margin=0.05,
               alpha=A if with_alpha else None, rendered_z=z if with_z else None)
    ref_sel = dict(sel)
    if not with_alpha:
        ref_sel["rendered_z"] = None                        # without alpha the rule has no A to divide by: every valid pixel
    # the inputs keep every pixel away from the thresholds: the masks of a float32 and a float64 evaluation agree
    m32, m64 = MR.selection_mask(depth, dtype=np.float32, **ref_sel), MR.selection_mask(depth, dtype=np.float64, **ref_sel)
    assert (m32 == m64).all()
    xyz_ref, rgb_ref, mask = MR.unproject_reference(cam, color, depth, **ref_sel)
    n_strided = ((W + stride - 1) // stride) * ((H + stride - 1) // stride)
    assert 0 < mask.sum() < n_strided
    dev = {k: (torch.tensor(v).cuda() if isinstance(v, np.ndarray) else v) for k, v in sel.items()}
    xyz, rgb = unproject_rgbd(cam, torch.tensor(color).cuda(), torch.tensor(depth).cuda(), **dev)
    assert xyz.shape == (int(mask.sum()), 3) and rgb.shape == xyz.shape
    assert np.array_equal(rgb.cpu().numpy(), rgb_ref)       # same count, same row order, colours bit-equal
    # fp32 chain: ndc (2 roundings, |ndc| <= 1), x tan x d (2, + 1 for the rounded tangent), - t (1): each view-space component is
    # within 6 u S of exact, S = d max(1, tanfovx, tanfovy) + |t|_inf; the 3-term dot product with |R_ij| <= 1 adds the three
    # component errors and 3 roundings of sums bounded by 3 S: 27 u S.  Stated as 32 u S.
    V = cam.world_view_transform.cpu().double().numpy()
    ys, xs = np.nonzero(mask)
    S = depth[ys, xs].astype(np.float64) * max(1.0, math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2)) + np.abs(V[3, :3]).max()
    err = np.abs(xyz.cpu().double().numpy() - xyz_ref).max(axis=1)
    print(f"unproject stride {stride} alpha {with_alpha} z {with_z}: n = {len(ys)}, max err / (u S) = {(err / (U * S)).max():.2f}")
    assert (err <= 32 * U * S).all()


def test_capacity_and_count():
    """Rows beyond `capacity` are dropped, never written; the count is the number selected."""
    from diff_gaussian_rasterization import _C
    W, H = 64, 40
    cam = fibonacci_cameras(2, W, H, seed=3, device="cuda")[0]
    depth = torch.tensor(MR.depth_sheet(H, W, seed=1)).cuda()
    color = torch.rand(3, H, W, device="cuda")
    full_xyz, full_rgb = unproject_rgbd(cam, color, depth)
    assert full_xyz.shape[0] == W * H
    lib = _C.lib()
    cap = 1000
    xyz = torch.full((cap + 8, 3), -7.0, device="cuda")
    rgb = torch.full((cap + 8, 3), -7.0, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    ws = torch.empty(lib.gsr_unproject_workspace_bytes(W, H), dtype=torch.uint8, device="cuda")
    view = cam.world_view_transform.contiguous()
    p = _C.gsr_unproject_params(H, W, math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2), view.data_ptr(), 1, 0.2, math.inf, 0.5, 0.05)
    _C.check(lib.gsr_unproject_rgbd(C.byref(p), _C.ptr(depth), _C.ptr(color), None, None, _C.ptr(xyz), _C.ptr(rgb), cap,
                                    _C.ptr(count), _C.ptr(ws), ws.numel(), _C._stream()))
    assert int(count.item()) == W * H
    assert torch.equal(xyz[:cap], full_xyz[:cap]) and torch.equal(rgb[:cap], full_rgb[:cap])
    assert bool((xyz[cap:] == -7.0).all()) and bool((rgb[cap:] == -7.0).all())


def test_round_trip_through_the_rasterizer():
    """Gaussians at the unprojected points project (gsr_debug_geometry_views: the splat records' 2-D means) onto the pixels they
    came from.  Bound: the unprojection leaves each world coordinate within 32 u S (above), S = d k + |t|_inf; the projection is a
    4-term dot product per homogeneous coordinate (|F| <= 1 / min tan) on values up to S, a division by w = d and the map to
    pixels (x side / 2): together under 128 u (S / d) / min(tanfov) in NDC, i.e. 64 u side (1 + |t| / d_min) k / min(tanfov)
    pixels - a hundredth of a pixel at this size."""
    from helpers import lowlevel_forward
    from scene_utils.synthetic import RawGaussians
    W, H = 203, 149
    cam = fibonacci_cameras(4, W, H, seed=11, device="cuda")[1]
    depth = MR.depth_sheet(H, W, seed=9, invalid_frac=0.02)
    color = np.random.default_rng(1).uniform(size=(3, H, W)).astype(np.float32)
    xyz, rgb = unproject_rgbd(cam, torch.tensor(color).cuda(), torch.tensor(depth).cuda(), stride=2, max_depth=3.0)
    mask = MR.selection_mask(depth, stride=2, max_depth=3.0)
    ys, xs = np.nonzero(mask)
    n = xyz.shape[0]
    assert n == len(ys) > 1000
    raw = RawGaussians(xyz.cpu(), torch.zeros(n, 1, 3), torch.zeros(n, 0, 3), torch.full((n, 3), math.log(0.01)),
                       torch.tensor([[1.0, 0, 0, 0]]).repeat(n, 1), torch.zeros(n, 1), 0)
    ll = lowlevel_forward(raw, cam, 0, torch.zeros(3))
    assert bool((ll["radii"] > 0).all())
    mean2d = ll["rec"][:, :2].double().numpy()
    k = max(1.0, math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2))
    t_inf = float(cam.world_view_transform[3, :3].abs().max())
    d_min = float(depth[ys, xs].min())
    tol = 64 * U * max(W, H) * (1.0 + t_inf / d_min) * k / min(math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2))
    err = max(np.abs(mean2d[:, 0] - xs).max(), np.abs(mean2d[:, 1] - ys).max())
    print(f"round trip: n = {n}, max pixel error {err:.3e}, bound {tol:.3e}")
    assert err <= tol


def _scene(P=20000, W=256, H=256, views=8):
    from gaussian_renderer import render, PipelineParams
    raw, cams, _ = make_config(1, device="cuda", P=P, W=W, H=H, views=views)
    teacher = GaussianModel.from_raw(raw, requires_grad=False)
    bg = torch.zeros(3, device="cuda")
    frames = []
    with torch.no_grad():
        for cam in cams:
            pkg = render(cam, teacher, PipelineParams(), bg, depth="z", alpha=True)
            A = pkg["alpha"][0]
            # the sensor: the surface depth sum w z / A where the teacher is (nearly) opaque, no reading (0) elsewhere
            depth = torch.where(A > 0.9, pkg["depth"][0] / A.clamp_min(1e-6), torch.zeros_like(A))
            frames.append((pkg["render"].clone(), depth.clone()))
    return cams, frames, bg


def test_create_from_pcd_follows_the_reference_lines():
    from gaussian_renderer import render, PipelineParams
    g = torch.Generator().manual_seed(3)
    pts = (torch.rand(5000, 3, generator=g) * 2.6 - 1.3)
    cols = torch.rand(5000, 3, generator=g)
    m = GaussianModel(3).create_from_pcd(pts.cuda(), cols.cuda(), spatial_lr_scale=2.5)
    P = 5000
    dist2 = MR.knn_dist2_bruteforce(pts, device="cuda")
    want_scale = torch.log(torch.sqrt(torch.clamp_min(dist2, 0.0000001)))[..., None].repeat(1, 3)
    assert m.spatial_lr_scale == 2.5 and m.active_sh_degree == 0 and m.max_sh_degree == 3
    assert torch.equal(m._xyz.detach().cpu(), pts) and m._xyz.requires_grad
    assert torch.allclose(m._features_dc.detach().cpu(), RGB2SH(cols).view(P, 1, 3), rtol=0, atol=1e-6)
    assert m._features_rest.shape == (P, 15, 3) and float(m._features_rest.detach().abs().max()) == 0.0
    # dist2 within 1e-6 relative (test_knn_gpu.py) -> log sqrt within 5e-7 absolute, + float32 rounding of a value of size <= 8
    assert float((m._scaling.detach().cpu().double() - want_scale).abs().max()) <= 5e-7 + 4 * U * 8
    assert torch.equal(m._rotation.detach().cpu(), torch.tensor([[1.0, 0, 0, 0]]).repeat(P, 1))
    assert torch.allclose(m._opacity.detach().cpu(), torch.full((P, 1), math.log(0.1 / 0.9)), rtol=0, atol=1e-6)
    assert m.max_radii2D.shape == (P,) and float(m.max_radii2D.abs().max()) == 0.0

    class Pcd:                                              # the reference's BasicPointCloud call form, numpy arrays
        points, colors = pts.numpy(), cols.numpy()
    m2 = GaussianModel(3).create_from_pcd(Pcd(), 1.0)
    assert torch.equal(m2._xyz, m._xyz) and torch.equal(m2._scaling, m._scaling) and torch.equal(m2._features_dc, m._features_dc)
    # renders and trains
    cams = fibonacci_cameras(2, 128, 96, seed=1, device="cuda")
    bg = torch.zeros(3, device="cuda")
    gts = {i: torch.rand(3, 96, 128, device="cuda") for i in range(2)}
    img = render(cams[0], m, PipelineParams(), bg)["render"]
    assert torch.isfinite(img).all() and float(img.max()) > 0
    tr = Trainer(m, cams, gts, render, PipelineParams(), bg, separate_sh=True)
    before = m._xyz.detach().clone()
    out = tr.step(0)
    tr.finish()
    assert torch.isfinite(out["loss"]) and not torch.equal(before, m._xyz.detach())


@pytest.mark.parametrize("optimizer", ["hip", "hip_fused"])
def test_add_from_rgbd_on_a_live_model(optimizer):
    from gaussian_renderer import render, PipelineParams
    from scene_utils.model import _PARAM_ATTRS
    cams, frames, bg = _scene(P=6000, W=160, H=128, views=6)
    pipe = PipelineParams()
    model = GaussianModel.from_raw(make_gaussians(3000, 3, seed=5, scale_factor=0.5).to("cuda"))
    gts = {i: f[0] for i, f in enumerate(frames)}
    tr = Trainer(model, cams, gts, render, pipe, bg, separate_sh=True, optimizer=optimizer)
    for it in range(4):
        tr.step(it % 3)
    tr.finish()
    P = model.get_xyz.shape[0]
    old = [getattr(model, a).detach().clone() for a in _PARAM_ATTRS]
    old_m = [(model.optimizer.state[getattr(model, a)]["exp_avg"].clone(),
              model.optimizer.state[getattr(model, a)]["exp_avg_sq"].clone()) for a in _PARAM_ATTRS]
    assert all(float(m[0].abs().max()) > 0 for m in old_m)                    # the moments are live
    stats = [model.xyz_gradient_accum.clone(), model.denom.clone(), model.max_radii2D.clone()]
    assert float(stats[1].max()) > 0
    with torch.no_grad():
        pkg = render(cams[4], model, pipe, bg, depth="z", alpha=True)
    # a frame without a valid reading adds nothing and changes nothing
    ids = [id(getattr(model, a)) for a in _PARAM_ATTRS]
    assert model.add_from_rgbd(cams[4], frames[4][0], torch.zeros_like(frames[4][1]), render_pkg=pkg) == 0
    assert ids == [id(getattr(model, a)) for a in _PARAM_ATTRS]
    assert model.get_xyz.shape[0] == P
    n = model.add_from_rgbd(cams[4], frames[4][0], frames[4][1], render_pkg=pkg, stride=2)
    assert n > 0 and model.get_xyz.shape[0] == P + n
    groups = {g["name"]: g for g in model.optimizer.param_groups}
    for a, name, o, (m1, m2) in zip(_PARAM_ATTRS, ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"), old, old_m):
        p = getattr(model, a)
        assert p.shape[0] == P + n and p.requires_grad and p.is_contiguous()
        assert torch.equal(p.detach()[:P], o)
        assert groups[name]["params"][0] is p                                   # the optimizer steps the new tensors
        st = model.optimizer.state[p]
        assert torch.equal(st["exp_avg"][:P], m1) and torch.equal(st["exp_avg_sq"][:P], m2)
        assert float(st["exp_avg"][P:].abs().max()) == 0.0 and float(st["exp_avg_sq"][P:].abs().max()) == 0.0
    assert len(model.optimizer.state) == 6
    for t, o in zip((model.xyz_gradient_accum, model.denom, model.max_radii2D), stats):
        assert t.shape[0] == P + n and torch.equal(t[:P], o) and float(t[P:].abs().max()) == 0.0
    # the new rows: colours of the frame, identity rotation, the requested opacity, isotropic finite scales
    assert torch.allclose(torch.sigmoid(model._opacity.detach()[P:]), torch.full((n, 1), 0.5, device="cuda"), atol=1e-6)
    sc = model._scaling.detach()[P:]
    assert torch.isfinite(sc).all() and torch.equal(sc[:, 0], sc[:, 1]) and torch.equal(sc[:, 0], sc[:, 2])
    from simple_knn._C import knn_dist2
    want = torch.log(torch.sqrt(knn_dist2(model._xyz.detach(), first_query=P).clamp_min(1e-7)))
    assert torch.equal(sc[:, 0], want)
    out = tr.step(4)                                                            # default forward mode, right after the insertion
    tr.finish()
    assert torch.isfinite(out["loss"])
    assert float(model.optimizer.state[model._xyz]["exp_avg"][P:].abs().max()) > 0
    nk, nc, ns = model.densify_and_prune(0.0002, 0.005, 2.6, None)
    assert model.get_xyz.shape[0] == nk + nc + 2 * ns > 0
    assert torch.isfinite(tr.step(1)["loss"])
    tr.finish()


def test_pixel_scale_needs_no_search():
    cams, frames, bg = _scene(P=6000, W=160, H=128, views=6)
    m = GaussianModel(0)
    n = m.add_from_rgbd(cams[0], frames[0][0], frames[0][1], scale="pixel", stride=2)
    assert n > 0 and m.get_xyz.shape[0] == n
    z = frames[0][1][::2, ::2].reshape(-1)
    z = z[z > 0.2]
    want = torch.log(z * (2.0 * math.tan(cams[0].FoVx / 2) / 160 * 2))
    assert torch.allclose(m._scaling.detach()[:, 0], want, atol=1e-4)


def test_track_insert_loop():
    """Map from keyframe 0 alone; keyframe 1 (the neighbouring Fibonacci view) is tracked with refine_pose(gt_depth=...) from a
    perturbed pose, then add_from_rgbd inserts what the map does not explain; rendering keyframe 1 again, the same selection
    finds fewer pixels than before."""
    from gaussian_renderer import render, PipelineParams
    cams, frames, bg = _scene(P=20000, W=256, H=256, views=8)
    pipe = PipelineParams()
    model = GaussianModel(3)
    n0 = model.add_from_rgbd(cams[3], frames[3][0], frames[3][1])
    assert n0 > 0 and model.get_xyz.shape[0] == n0
    with torch.no_grad():
        cover0 = render(cams[3], model, pipe, bg, depth="z", alpha=True)["alpha"][0]
    seen = frames[3][1] > 0.2
    print(f"keyframe 0: {n0} rows; its own pixels covered (A > 0.5): {float((cover0[seen] > 0.5).float().mean()):.3f}")
    # keyframe 1: tracked from a perturbed pose against the frozen map
    img1, depth1 = frames[4]
    pc = PoseCamera(cams[4], dtype=torch.float64, device="cpu")
    true_w2c = pc.base_w2c.clone()
    delta = torch.tensor([0.01, -0.008, 0.012, 0.003, -0.002, 0.002], dtype=torch.float64)
    pc.base_w2c = se3_exp(delta) @ true_w2c
    pc, hist = refine_pose(pc, model, img1, iters=40, gt_depth=depth1, depth_weight=0.5)
    print(f"tracking loss {hist[0]:.5f} -> {hist[-1]:.5f}")

    def selected():
        with torch.no_grad():
            pkg = render(pc, model, pipe, bg, depth="z", alpha=True)
            xyz, _ = unproject_rgbd(pc, img1, depth1, alpha=pkg["alpha"], rendered_z=pkg["depth"])
        return pkg, int(xyz.shape[0])
    pkg, before = selected()
    n1 = model.add_from_rgbd(pc, img1, depth1, render_pkg=pkg)
    assert n1 == before > 0 and model.get_xyz.shape[0] == n0 + n1
    _, after = selected()
    print(f"track -> insert: keyframe 0 gave {n0} rows, keyframe 1 selected {before} pixels, {after} after the insertion")
    assert after < before
