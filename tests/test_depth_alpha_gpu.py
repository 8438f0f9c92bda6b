"""Z-depth and accumulated-opacity images of the rasterizer (GaussianRasterizer(depth="z", alpha=True), include/gsr.h
gsr_render_extras) and RGB-D tracking (scene_utils.refine_pose(gt_depth=...)).

The oracle is the unmodified float64 oracle.gs_oracle.rasterize, with two constructions:
  z-depth  D_z = sum_i w_i z_i : colors_precomp = z (all three channels), bg = 0, channel 0; z = means3D . V[:3, 2] + V[3, 2]
           formed with torch from the (possibly grad) viewmatrix;
  opacity  A = 1 - T_final     : colors_precomp = 0, bg = e_0: channel 0 is T_final.
All three renders share the leaves, so one backward of <color, gc> + <D_z, gd> + <A, ga> gives every gradient."""
import ctypes as C
import math
import os

import pytest
import torch

from helpers import leaf_inputs, settings_for, upstream_grads, rel_l2, _view
from oracle import gs_oracle as O
from scene_utils import make_gaussians, fibonacci_cameras, PoseCamera, se3_exp, refine_pose, pose_error
from scene_utils.model import GaussianModel
from test_camera_grad_gpu import CAM_REL, cam_leaves, check_camera
from test_parity_gpu import FWD_ATOL, FWD_FRAC, check_grads

pytestmark = pytest.mark.gpu

BG = torch.tensor([0.2, 0.5, 0.7])


class _env:
    """Sets library switches for a block, restoring the previous values."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_UNSET = dict(GSR_BWD_FORM=None, GSR_BWD_LPT=None, GSR_BWD_MASK=None, GSR_BWD_REDUCE=None, GSR_FWD_MASK=None)


@pytest.fixture(autouse=True)
def _restore_mode():
    import diff_gaussian_rasterization as dgr
    mode = dgr.forward_mode()
    yield
    dgr.set_forward_mode(mode)


def small_scene(P=3000, W=150, H=100, deg=3, seed=11, scale=0.6, view=1):
    """tests/test_parity_gpu.small_scene's recipe."""
    raw = make_gaussians(P, deg, seed=seed, scale_factor=scale)
    cam = fibonacci_cameras(3, W, H, seed=5)[view]
    return raw, cam


def new_grads(H, W, seed=17):
    """Upstream gradients of the colour, the depth plane and the opacity plane."""
    gc, gd = upstream_grads(H, W, seed=seed)
    ga = torch.randn(1, H, W, generator=torch.Generator().manual_seed(seed + 1))
    return gc, gd, ga


def _inputs(raw, dtype, device, mode, cov, raw_act):
    inp = leaf_inputs(raw, dtype, device, mode)
    if raw_act:
        for k, v in (("opacities", raw.opacity), ("scales", raw.scaling), ("rotations", raw.rotation)):
            inp[k] = v.detach().to(device=device, dtype=dtype).clone().requires_grad_(True)
    if cov:
        c = O.cov3d_from_scale_rot(inp["scales"].detach().cpu().double(), inp["rotations"].detach().cpu().double(), 1.0)
        inp["cov3D_precomp"] = c.to(device=device, dtype=dtype).requires_grad_(True)
    return inp


def oracle_rgbd(raw, cam, mode="sh", aa=False, cov=False, raw_act=False, deg=3, grads=None, leaves=None, bg=BG):
    """float64 oracle: (color, radii, D_z, A) and, with `grads` = (gc, gd, ga), the gradients of every input leaf and of the
    camera leaves (viewmatrix, projmatrix, campos)."""
    dt = torch.float64
    inp = _inputs(raw, dt, "cpu", mode, cov, raw_act)
    vm, pm, cp = leaves if leaves is not None else cam_leaves(cam, dt, "cpu")
    s = settings_for(cam, deg, bg, 1.0, aa)._replace(viewmatrix=vm, projmatrix=pm, campos=cp)
    op, sc, rot = inp["opacities"], inp.get("scales"), inp.get("rotations")
    if raw_act:
        op, sc, rot = torch.sigmoid(op), torch.exp(sc), torch.nn.functional.normalize(rot)
    geo = dict(cov3D_precomp=inp["cov3D_precomp"]) if cov else dict(scales=sc, rotations=rot)
    shs = torch.cat([inp["dc"], inp["shs"]], dim=1) if mode == "dc" else inp.get("shs")
    m3, m2 = inp["means3D"], inp["means2D"]
    color, radii, _ = O.rasterize(m3, m2, op, s, shs=shs, colors_precomp=inp.get("colors_precomp"), **geo)
    P = m3.shape[0]
    z = m3 @ vm[:3, 2] + vm[3, 2]
    dz, _, _ = O.rasterize(m3, m2, op, s._replace(bg=torch.zeros(3, dtype=dt)), colors_precomp=z[:, None].expand(P, 3), **geo)
    tf, _, _ = O.rasterize(m3, m2, op, s._replace(bg=torch.tensor([1.0, 0.0, 0.0], dtype=dt)),
                           colors_precomp=torch.zeros(P, 3, dtype=dt), **geo)
    D, A = dz[0:1], 1.0 - tf[0:1]
    out = dict(color=color.detach(), radii=radii, D=D.detach(), A=A.detach())
    if grads is not None:
        gc, gd, ga = (t.to(dt) for t in grads)
        ((color * gc).sum() + (D * gd).sum() + (A * ga).sum()).backward()
        out["grads"] = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in inp.items()}
        if leaves is None:
            out["cam"] = [torch.zeros_like(t) if t.grad is None else t.grad.detach() for t in (vm, pm, cp)]
    return out


def hip_rgbd(raw, cam, mode="sh", aa=False, cov=False, raw_act=False, deg=3, grads=None, depth="z", alpha=True, camera=True,
             leaves=None, bg=BG, **call_kw):
    """One forward (+ backward of <color, gc> + <depth plane, gd> + <A, ga>, the terms whose upstream is not None) through
    GaussianRasterizer on cuda."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    inp = _inputs(raw, torch.float32, "cuda", mode, cov, raw_act)
    if leaves is None:
        leaves = cam_leaves(cam, torch.float32, "cuda") if camera else \
            [t.to("cuda") for t in (cam.world_view_transform, cam.full_proj_transform, cam.camera_center)]
    vm, pm, cp = leaves
    s = settings_for(cam, deg, bg, 1.0, aa, cls=GaussianRasterizationSettings, device="cuda")._replace(
        viewmatrix=vm, projmatrix=pm, campos=cp)
    kw = dict(shs=inp.get("shs"), colors_precomp=inp.get("colors_precomp"), dc=inp.get("dc"))
    if cov:
        kw["cov3D_precomp"] = inp["cov3D_precomp"]
    else:
        kw.update(scales=inp["scales"], rotations=inp["rotations"])
    if raw_act:
        kw["raw_activations"] = True
    ext = {} if (depth == "inverse" and not alpha) else dict(depth=depth, alpha=alpha)
    res = GaussianRasterizer(s)(means3D=inp["means3D"], means2D=inp["means2D"], opacities=inp["opacities"], **kw, **ext,
                                **call_kw)
    color, radii, D = res[:3]
    A = res[3] if alpha else None
    out = dict(color=color.detach().cpu(), radii=radii.cpu(), D=D.detach().cpu(), A=None if A is None else A.detach().cpu())
    if grads is not None:
        gc, gd, ga = grads
        loss = (color * gc.cuda()).sum()
        if gd is not None:
            loss = loss + (D * gd.cuda()).sum()
        if ga is not None:
            loss = loss + (A * ga.cuda()).sum()
        loss.backward()
        out["grads"] = {k: (v.grad.detach().cpu() if v.grad is not None else torch.zeros_like(v).cpu()) for k, v in inp.items()}
        out["cam"] = [None if t.grad is None else t.grad.detach().cpu() for t in leaves] \
            if camera and all(t.is_leaf for t in leaves) else None
    torch.cuda.synchronize()
    return out


def _close(x, ref, scale=None):
    """The forward parity bar of test_parity_gpu (|err| <= 2e-5 on >= 99.99 % of pixels), relative to `scale`."""
    d = (x.double() - ref.double()).abs() / (scale or 1.0)
    return float((d <= FWD_ATOL).double().mean()) >= FWD_FRAC, float(d.max())


# ------------------------------------------------------------------------------------------------------------------------------
# 1  forward
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aa", [False, True])
def test_forward_matches_oracle_and_leaves_the_rest_alone(aa):
    raw, cam = small_scene()
    ref = oracle_rgbd(raw, cam, aa=aa)
    out = hip_rgbd(raw, cam, aa=aa)
    dmax = float(ref["D"].abs().max())
    assert dmax > 1.0 and float(ref["A"].max()) > 0.5
    ok, err = _close(out["D"], ref["D"], dmax)
    assert ok, err
    ok, err = _close(out["A"], ref["A"])
    assert ok, err
    assert int((out["radii"] != ref["radii"]).sum()) <= 2
    # colour, radii (and the inverse depth, where it is asked for) do not depend on the options: bit for bit
    plain = hip_rgbd(raw, cam, aa=aa, depth="inverse", alpha=False)
    for depth, alpha in (("z", True), ("z", False), ("inverse", True)):
        o = out if (depth, alpha) == ("z", True) else hip_rgbd(raw, cam, aa=aa, depth=depth, alpha=alpha)
        assert torch.equal(o["color"], plain["color"]) and torch.equal(o["radii"], plain["radii"]), (depth, alpha)
        if depth == "inverse":
            assert torch.equal(o["D"], plain["D"])
        else:
            assert torch.equal(o["D"], out["D"])
        if alpha:
            assert torch.equal(o["A"], out["A"])


def test_alpha_is_one_minus_final_T_and_state_unchanged():
    """Through the C ABI (gsr_forward_prepare_ex / gsr_forward_render_ex): A = 1 - final_T of gsr_debug_image_views bit for bit;
    final_T, n_contrib, colour and radii bit-identical to the calls without extras."""
    from diff_gaussian_rasterization import _C, GaussianRasterizationSettings
    from diff_gaussian_rasterization import _settings_struct, _gauss_struct, _stream
    lib = _C.lib()
    raw, cam = small_scene()
    inp = leaf_inputs(raw, torch.float32, "cuda", "sh")
    P, H, W = inp["means3D"].shape[0], cam.image_height, cam.image_width
    rs = settings_for(cam, 3, BG, 1.0, False, cls=GaussianRasterizationSettings, device="cuda")
    s, keep = _settings_struct(rs, "cuda")
    t = {k: v.detach().contiguous() for k, v in inp.items()}
    g = _gauss_struct(P, t["means3D"], None, t["shs"], None, t["opacities"], t["scales"], t["rotations"], None)
    res = {}
    for kind, want_alpha in ((None, False), (1, True), (0, True)):
        geom = torch.zeros(lib.gsr_geometry_state_bytes(P), dtype=torch.uint8, device="cuda")
        img = torch.zeros(lib.gsr_image_state_bytes(W, H), dtype=torch.uint8, device="cuda")
        radii = torch.zeros(P, dtype=torch.int32, device="cuda")
        color, invd = torch.empty(3, H, W, device="cuda"), torch.empty(1, H, W, device="cuda")
        alpha = torch.full((H, W), float("nan"), device="cuda")
        ex = None if kind is None else C.byref(_C.gsr_render_extras(kind, _C.ptr(alpha) if want_alpha else None, None))
        R = _C.check(lib.gsr_forward_prepare_ex(C.byref(s), C.byref(g), _C.ptr(geom), geom.numel(), _C.ptr(radii), _stream(),
                                                ex))
        binning = torch.zeros(lib.gsr_binning_state_bytes(P, W, H, R), dtype=torch.uint8, device="cuda")
        _C.check(lib.gsr_forward_render_ex(C.byref(s), C.byref(g), _C.ptr(geom), _C.ptr(binning), binning.numel(), R,
                                           _C.ptr(img), img.numel(), _C.ptr(color), _C.ptr(invd), 1, _stream(), ex))
        torch.cuda.synchronize()
        pi = [C.c_void_p() for _ in range(2)]
        lib.gsr_debug_image_views(_C.ptr(img), W, H, C.byref(pi[0]), C.byref(pi[1]))
        res[kind] = dict(final_T=_view(img, pi[0].value, W * H, torch.float32).view(H, W),
                         n_contrib=_view(img, pi[1].value, W * H, torch.int32).view(H, W), color=color.cpu(),
                         radii=radii.cpu(), invd=invd.cpu(), alpha=alpha.cpu())
    base = res[None]
    for kind in (1, 0):
        r = res[kind]
        for k in ("final_T", "n_contrib", "color", "radii"):
            assert torch.equal(r[k], base[k]), (kind, k)
        assert torch.equal(r["alpha"], 1.0 - r["final_T"]), kind
    assert torch.equal(res[0]["invd"], base["invd"])
    assert not torch.equal(res[1]["invd"], base["invd"])
    # an unknown depth kind is refused before anything is enqueued
    bad = _C.gsr_render_extras(7, None, None)
    geom = torch.zeros(lib.gsr_geometry_state_bytes(P), dtype=torch.uint8, device="cuda")
    radii = torch.zeros(P, dtype=torch.int32, device="cuda")
    rc = lib.gsr_forward_prepare_ex(C.byref(s), C.byref(g), _C.ptr(geom), geom.numel(), _C.ptr(radii), _stream(), C.byref(bad))
    assert rc == -1 and "depth_kind" in _C.last_error()


# ------------------------------------------------------------------------------------------------------------------------------
# 2  gradients against the float64 oracle
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,aa,cov,raw_act", [
    ("sh", False, False, False),
    ("sh", True, False, False),
    ("colors", False, True, False),
    ("colors", True, False, False),
    ("dc", True, False, True),
    ("sh", False, True, False)])
def test_gradients_match_oracle(mode, aa, cov, raw_act):
    raw, cam = small_scene()
    grads = new_grads(cam.image_height, cam.image_width)
    ref = oracle_rgbd(raw, cam, mode, aa, cov, raw_act, grads=grads)
    out = hip_rgbd(raw, cam, mode, aa, cov, raw_act, grads=grads)
    check_grads(out, ref)
    check_camera(out["cam"], ref["cam"])
    # the new terms are really there: without them the gradients are different
    plain = hip_rgbd(raw, cam, mode, aa, cov, raw_act, grads=(grads[0], None, None), depth="inverse", alpha=False)
    assert not torch.equal(plain["grads"]["means3D"], out["grads"]["means3D"])
    assert not torch.equal(plain["cam"][0], out["cam"][0])


@pytest.mark.parametrize("which", ["depth", "alpha"])
def test_each_new_plane_alone_matches_oracle(which):
    """Each chain on its own (the other upstream zero): z-depth through g_t.z, opacity through the background term."""
    raw, cam = small_scene(seed=23, view=2)
    gc, gd, ga = new_grads(cam.image_height, cam.image_width, seed=29)
    z = torch.zeros_like(gd)
    grads = (gc * 0, gd, z) if which == "depth" else (gc * 0, z, ga)
    ref = oracle_rgbd(raw, cam, aa=True, grads=grads)
    out = hip_rgbd(raw, cam, aa=True, grads=grads)
    check_grads(out, ref)
    check_camera(out["cam"], ref["cam"])


# ------------------------------------------------------------------------------------------------------------------------------
# 3  every path
# ------------------------------------------------------------------------------------------------------------------------------
def _form_scene():
    raw = make_gaussians(6000, 3, seed=401, scale_factor=0.8)
    cam = fibonacci_cameras(3, 208, 144, seed=403)[2]
    return raw, cam


@pytest.mark.parametrize("name,env,binning,fmode", [
    ("tile", dict(GSR_BWD_FORM="tile"), None, None),
    ("quad", dict(GSR_BWD_FORM="quad"), None, None),
    ("lpt0", dict(GSR_BWD_LPT="0"), None, None),
    ("lpt1", dict(GSR_BWD_LPT="1"), None, None),
    ("tile-lpt0", dict(GSR_BWD_FORM="tile", GSR_BWD_LPT="0"), None, None),
    ("tile-lpt1", dict(GSR_BWD_FORM="tile", GSR_BWD_LPT="1"), None, None),
    ("tile-mask0", dict(GSR_BWD_FORM="tile", GSR_BWD_MASK="0"), None, None),
    ("fwd-mask1", dict(GSR_FWD_MASK="1"), None, None),
    ("mfma", dict(GSR_BWD_FORM="tile", GSR_BWD_REDUCE="mfma"), None, None),
    ("global", {}, "global", None),
    ("exact", {}, None, "exact"),
    ("sync", {}, None, "sync"),
    ("async", {}, None, "async")])
def test_every_path(name, env, binning, fmode, monkeypatch):
    """208x144, 6000 Gaussians, anti-aliasing, random upstream on colour, D_z and A.  Within each compositing-backward form
    (four-wave, one-wave tile, matrix pipe) walk order, masks, binning form and forward mode change no bit of any output or
    gradient; the forms themselves, and the masked forward, are each within the bar of the float64 oracle."""
    from diff_gaussian_rasterization import _workspace as ws
    raw, cam = _form_scene()
    grads = new_grads(cam.image_height, cam.image_width, seed=41)
    tile_form = env.get("GSR_BWD_FORM") == "tile"
    with _env(**{**_UNSET, **({"GSR_BWD_FORM": "tile"} if tile_form else {})}):
        base = hip_rgbd(raw, cam, aa=True, grads=grads)
    if binning is not None:
        monkeypatch.setattr(ws, "_BINNING", binning)
    kw = {} if fmode is None else dict(forward_mode=fmode)
    with _env(**{**_UNSET, **env}):
        out = hip_rgbd(raw, cam, aa=True, grads=grads, **kw)
    for k in ("color", "D", "A", "radii"):
        assert torch.equal(out[k], base[k]), (name, k)
    if name != "mfma":
        for k in base["grads"]:
            assert torch.equal(out["grads"][k], base["grads"][k]), (name, k)
        for i, (x, y) in enumerate(zip(out["cam"], base["cam"])):
            assert torch.equal(x, y), (name, i)
    if name in ("tile", "quad", "mfma", "fwd-mask1"):
        ref = oracle_rgbd(raw, cam, aa=True, grads=grads)
        check_grads(out, ref)
        check_camera(out["cam"], ref["cam"])
        assert _close(out["D"], ref["D"], float(ref["D"].abs().max()))[0] and _close(out["A"], ref["A"])[0]


def test_tile_cull_and_deferred_colour_paths():
    """The lists truncated by depth (tile_cull, unverified frames) and the split geometry / shade forward give the same images and
    gradients as the plain call, bit for bit."""
    import diff_gaussian_rasterization as dgr
    raw, cam = _form_scene()
    grads = new_grads(cam.image_height, cam.image_width, seed=43)
    dgr.set_forward_mode("async")
    base = hip_rgbd(raw, cam, grads=grads)
    cull = dgr.new_tile_cull(cam.image_height, cam.image_width)
    for _ in range(3):                     # the cut-offs are learnt by the first calls, then applied
        out = hip_rgbd(raw, cam, grads=grads, tile_cull=cull)
        dgr.call_stats()
    assert dgr.call_stats().get("culled_frames", 0) > 0
    for k in ("color", "D", "A"):
        assert torch.equal(out[k], base[k]), k
    for k in base["grads"]:
        assert torch.equal(out["grads"][k], base["grads"][k]), k
    ev = torch.cuda.Event()
    ev.record()
    for mode in ("sync", "exact"):
        dgr.set_forward_mode(mode)
        o = hip_rgbd(raw, cam, grads=grads, sh_ready_event=ev)
        for k in ("color", "D", "A"):
            assert torch.equal(o[k], base[k]), (mode, k)
        for k in base["grads"]:
            assert torch.equal(o["grads"][k], base["grads"][k]), (mode, k)


@pytest.mark.parametrize("kind", ["hip", "hip_sparse"])
def test_adam_fold_bit_identical(kind):
    """BackwardFold(optimizer, stats) with an RGB-D loss: parameters, both moments and the densification statistics after several
    steps equal backward + optimizer.step() + add_densification_stats bit for bit."""
    import diff_gaussian_rasterization as dgr
    from gaussian_renderer import render, PipelineParams
    cams = fibonacci_cameras(3, 176, 112, seed=91, device="cuda")
    bg = torch.tensor([0.1, 0.2, 0.05], device="cuda")
    pipe = PipelineParams()
    gen = torch.Generator().manual_seed(97)
    gt = torch.rand(3, 112, 176, generator=gen).cuda()
    gdep = (2.0 + torch.rand(1, 112, 176, generator=gen)).cuda()
    ga = torch.randn(1, 112, 176, generator=gen).cuda()
    res = {}
    for folded in (False, True):
        model = GaussianModel.from_raw(make_gaussians(3000, 3, seed=93, scale_factor=0.7).to("cuda"))
        opt = model.training_setup(optimizer=kind)
        n0 = dgr.call_stats().get("folded_backwards", 0)
        for it in range(4):
            fold = dgr.BackwardFold(optimizer=opt, stats=(model.xyz_gradient_accum, model.denom, model.max_radii2D)) \
                if folded else None
            pkg = render(cams[it % 3], model, pipe, bg, separate_sh=True, fold=fold, depth="z", alpha=True)
            loss = (pkg["render"] - gt).abs().mean() + 0.1 * (pkg["depth"] - gdep).abs().mean() + (pkg["alpha"] * ga).mean()
            loss.backward()
            if not folded:
                model.add_densification_stats(pkg["viewspace_points"], pkg["visibility_filter"], pkg["radii"])
                if kind == "hip_sparse":          # (reference train.py:173-176)
                    opt.step(pkg["radii"] > 0, pkg["radii"].shape[0])
                else:
                    opt.step()
                opt.zero_grad(set_to_none=True)
            else:
                assert fold.optimizer_taken and fold.stats_taken
        torch.cuda.synchronize()
        assert dgr.call_stats().get("folded_backwards", 0) - n0 == (4 if folded else 0)
        res[folded] = [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone())
                       for p in model.parameters()] + [(model.xyz_gradient_accum.clone(), model.denom.clone(),
                                                         model.max_radii2D.clone())]
    for a, b in zip(res[False], res[True]):
        for x, y in zip(a, b):
            assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------------------------------------
# 4  zero upstream on the new planes
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,alpha", [("z", True), ("z", False), ("inverse", True)])
def test_zero_gradient_identity(depth, alpha):
    """Zero upstream gradients on the new planes: every gradient (per Gaussian and camera) equals the default call's bit for bit;
    with inverse depth the inverse-depth gradient rides along in both."""
    raw, cam = small_scene(seed=31, view=0)
    gc, gd, ga = new_grads(cam.image_height, cam.image_width, seed=37)
    z1 = torch.zeros_like(gd)
    gd_default = gd if depth == "inverse" else z1
    plain = hip_rgbd(raw, cam, aa=True, grads=(gc, gd_default, None), depth="inverse", alpha=False)
    out = hip_rgbd(raw, cam, aa=True, grads=(gc, gd_default, z1 if alpha else None), depth=depth, alpha=alpha)
    assert float(plain["grads"]["shs"].abs().max()) > 0 and float(plain["grads"]["means3D"].abs().max()) > 0
    for k in plain["grads"]:
        assert torch.equal(out["grads"][k], plain["grads"][k]), k
    for x, y in zip(out["cam"], plain["cam"]):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------------------------------------
# 5  an overflowed async frame
# ------------------------------------------------------------------------------------------------------------------------------
def test_async_overflow_gives_zero_gradients(monkeypatch):
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _workspace as ws
    monkeypatch.setattr(ws, "_BINNING", "global")
    raw = make_gaussians(5000, 3, seed=301, scale_factor=0.7)
    cam = fibonacci_cameras(2, 160, 96, seed=302)[0]
    grads = new_grads(96, 160, seed=47)
    dgr.set_forward_mode("sync")
    ref = hip_rgbd(raw, cam, grads=grads)
    R = dgr.call_stats()["num_rendered"]
    assert R > 4096 and float(ref["grads"]["means3D"].abs().max()) > 0
    dgr.set_forward_mode("async")
    pool = ws.pool(torch.device("cuda", 0))
    key = (5000, 160, 96)
    old_min, ws.MIN_CAPACITY = ws.MIN_CAPACITY, 256
    try:
        pool.capacity[key] = max(256, R // 3)
        for w in pool.free:
            w.binning = w.scratch = None
        n0 = dgr.call_stats()["overflow_frames"]
        dgr.take_overflowed()
        with pytest.warns(RuntimeWarning, match="truncated"):
            out = hip_rgbd(raw, cam, grads=grads)
            st = dgr.call_stats()
        assert st["overflow_frames"] == n0 + 1
        for k, g in out["grads"].items():
            assert not g.any(), k
        for t in out["cam"]:
            assert not t.any()
        again = hip_rgbd(raw, cam, grads=grads)       # the capacity was raised: the next frame is exact
        for k in ref["grads"]:
            assert torch.equal(again["grads"][k], ref["grads"][k]), k
    finally:
        ws.MIN_CAPACITY = old_min


def test_graph_capture_refuses_the_options(monkeypatch):
    """Under HIP-graph capture a call with depth / alpha raises a clear error, before anything is enqueued, instead of capturing
    something unverified (the capture state is what the forward asks torch for; here torch is told it is capturing)."""
    from diff_gaussian_rasterization import _C
    raw, cam = small_scene(P=500)
    hip_rgbd(raw, cam, camera=False)                       # (eager warm-up of the shape)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    for depth, alpha in (("z", False), ("inverse", True)):
        with pytest.raises(_C.GsrError, match="graph capture"):
            with torch.no_grad():
                hip_rgbd(raw, cam, camera=False, depth=depth, alpha=alpha)


# ------------------------------------------------------------------------------------------------------------------------------
# 6, 7  tracking
# ------------------------------------------------------------------------------------------------------------------------------
def test_pose_twist_chain_rgbd_matches_oracle():
    """dL/dtau of <color, gc> + <D_z, gd> + <A, ga> through PoseCamera on the device against the same PoseCamera driving the
    float64 oracle on the CPU."""
    raw, cam = small_scene()
    tau0 = torch.tensor([0.01, -0.02, 0.015, 0.004, -0.006, 0.003], dtype=torch.float64)
    grads = new_grads(cam.image_height, cam.image_width, seed=53)
    res = []
    for dev, dt in (("cpu", torch.float64), ("cuda", torch.float32)):
        pc = PoseCamera(cam, dtype=dt, device=dev)
        with torch.no_grad():
            pc.tau.copy_(tau0.to(dt))
        leaves = [pc.world_view_transform, pc.full_proj_transform, pc.camera_center]
        if dev == "cpu":
            oracle_rgbd(raw, pc, grads=grads, leaves=leaves)
        else:
            hip_rgbd(raw, pc, grads=grads, leaves=leaves)
        res.append(pc.tau.grad.detach().cpu())
    ref, out = res
    assert rel_l2(out, ref) <= CAM_REL, (out, ref)
    assert float((out.double() - ref).abs().max() / ref.abs().max()) <= CAM_REL


def _perturbed(cam):
    """test_refine_pose_converges' perturbation: 1 deg rotation, 2 % of the camera distance in translation."""
    true_w2c = cam.world_view_transform.transpose(0, 1).double().cpu()
    dist = float(cam.camera_center.norm())
    axis = torch.tensor([0.3, -0.8, 0.5], dtype=torch.float64)
    tdir = torch.tensor([0.6, 0.2, -0.77], dtype=torch.float64)
    delta = torch.cat([0.02 * dist * tdir / tdir.norm(), math.radians(1.0) * axis / axis.norm()])
    pc = PoseCamera(cam, dtype=torch.float64, device="cpu")
    pc.base_w2c = se3_exp(delta) @ true_w2c
    return pc, true_w2c


def test_refine_pose_rgbd_converges():
    """RGB-D tracking of test_refine_pose_converges' perturbed camera against its frozen 20 k-Gaussian model; the depth reading
    is the z-depth rendered at the true pose.  Measured once (MI355X): see the thresholds below."""
    from gaussian_renderer import render, PipelineParams
    raw = make_gaussians(20000, 3, seed=4, scale_factor=0.35)
    cam = fibonacci_cameras(4, 256, 192, seed=2, device="cuda")[1]
    model = GaussianModel.from_raw(raw.to("cuda"), requires_grad=False)
    bg = torch.zeros(3, device="cuda")
    with torch.no_grad():
        pkg = render(cam, model, PipelineParams(), bg, depth="z", alpha=True)
        gt, gt_depth = pkg["render"].detach().clone(), pkg["depth"].detach().clone()
    assert set(pkg.keys()) == {"render", "viewspace_points", "visibility_filter", "radii", "depth", "alpha"}
    pc, true_w2c = _perturbed(cam)
    r0, t0 = pose_error(pc.w2c().detach(), true_w2c)
    pc, hist = refine_pose(pc, model, gt, iters=150, gt_depth=gt_depth, depth_weight=0.5, alpha_min=0.5)
    r1, t1 = pose_error(pc.w2c().detach(), true_w2c)
    print(f"RGB-D pose refinement: rotation {math.degrees(r0):.4f} -> {math.degrees(r1):.3e} deg, translation {t0:.5f} -> "
          f"{t1:.3e}, loss {hist[0]:.5f} -> {hist[-1]:.3e}")
    # measured once (MI355X): rotation 0.9998 -> 0.0 deg (below what arccos resolves), translation 0.0800 -> 4.50e-5 (1780x),
    # loss 0.0581 -> 1.08e-4.  Thresholds: those of test_refine_pose_converges
    assert r1 <= r0 / 10 and t1 <= t0 / 10, (r0, r1, t0, t1)
    assert math.degrees(r1) <= 1e-2 and t1 <= 2e-3, (math.degrees(r1), t1)
    assert hist[-1] < hist[0] / 10


def test_depth_only_tracking_in_a_constant_colour_scene():
    """Every Gaussian the same colour, on a background of that colour: the image carries almost no pose signal, the z-depth
    does.  Depth-only refinement (depth_weight = 1) reduces the translation error at least tenfold."""
    from gaussian_renderer import render, PipelineParams
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
    pc, true_w2c = _perturbed(cam)
    r0, t0 = pose_error(pc.w2c().detach(), true_w2c)
    pc_d, _ = refine_pose(pc, model, gt, iters=150, bg=bg, gt_depth=gt_depth, depth_weight=1.0, alpha_min=0.5)
    r1, t1 = pose_error(pc_d.w2c().detach(), true_w2c)
    pc_p, _ = _perturbed(cam)
    pc_p, _ = refine_pose(pc_p, model, gt, iters=150, bg=bg)
    r2, t2 = pose_error(pc_p.w2c().detach(), true_w2c)
    print(f"constant colour: translation {t0:.5f} -> depth-only {t1:.3e}, photometric {t2:.3e}; rotation {math.degrees(r0):.4f} "
          f"-> {math.degrees(r1):.3e} / {math.degrees(r2):.3e} deg")
    # measured once (MI355X): translation 0.0800 -> 1.25e-5 depth-only (rotation 1 deg -> 0), photometric 0.0802 (0.82 deg)
    assert t1 <= t0 / 10, (t0, t1)
    assert t2 > t0 / 2, (t0, t2)                  # photometric: (almost) no signal
