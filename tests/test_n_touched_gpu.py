"""Per-Gaussian visibility counts of the rasterizer (GaussianRasterizer(n_touched=True, touched_T_min=...), include/gsr.h
gsr_render_extras.n_touched) and the keyframe policy layer on top (scene_utils.keyframes).

n_touched[i] = number of pixels in which Gaussian i is blended (power <= 0, alpha >= 1/255, pixel not finished, not the entry
that stops the pixel) while the pixel's transmittance BEFORE blending it is > T_min.

The oracle is the unmodified float64 oracle.gs_oracle.rasterize(return_state=True); `band_counts` below restates the per-entry
decisions of its `composite` and returns, per Gaussian, the exact count and a certain lower / possible upper count: a (entry,
pixel) pair is UNCERTAIN when a float32 kernel may legitimately decide it the other way -
  * its own alpha lies within 1e-3 relative of 1/255, or its power within 1e-5 of 0;
  * its T before blending lies within (1 +- 1e-4) (1 - 1/255)^(+-k) of T_min, k = uncertain entries in front of it in the pixel;
  * it lies behind an entry whose stop test (T_incl < 1e-4) is within 1 % (same widening by k) - or IS that entry: the stop test
    is what decides whether the stopping entry itself is blended.
The test asserts lo <= n_hip <= hi for EVERY row, and - on the oracle alone, so that the band cannot hide a failure - that
rows with lo != hi are at most 10 % of P, sum(hi - lo) <= 0.2 % of sum(exact) and lo <= exact <= hi."""
import ctypes as C
import math

import pytest
import torch

from helpers import leaf_inputs, settings_for, upstream_grads
from oracle import gs_oracle as O
from scene_utils import make_gaussians, fibonacci_cameras, look_at_camera, GaussianModel, RawGaussians
from test_depth_alpha_gpu import _env, _inputs, small_scene, BG

pytestmark = pytest.mark.gpu
T_MINS = (0.0, 0.05, 0.5, 0.9)


@pytest.fixture(autouse=True)
def _restore_mode():
    import diff_gaussian_rasterization as dgr
    mode = dgr.forward_mode()
    yield
    dgr.set_forward_mode(mode)


# ------------------------------------------------------------------------------------------------------------------------------
# the oracle's per-entry decisions, with the band
# ------------------------------------------------------------------------------------------------------------------------------
def band_counts(pre, point_list, ranges, W, H, T_min):
    """-> (exact, lo, hi) int64 [P] from the state of oracle.gs_oracle.rasterize (any dtype)."""
    dt = pre.xy.dtype
    P = pre.xy.shape[0]
    gx, gy = (W + O.BLOCK_X - 1) // O.BLOCK_X, (H + O.BLOCK_Y - 1) // O.BLOCK_Y
    exact, lo, hi = (torch.zeros(P, dtype=torch.int64) for _ in range(3))
    amin, f = 1.0 / 255.0, 1.0 - 1.0 / 255.0
    for tile in range(gx * gy):
        a, b = int(ranges[tile, 0]), int(ranges[tile, 1])
        if b <= a:
            continue
        ty, tx = divmod(tile, gx)
        x0, y0 = tx * O.BLOCK_X, ty * O.BLOCK_Y
        xs = torch.arange(x0, min(x0 + O.BLOCK_X, W), dtype=dt)
        ys = torch.arange(y0, min(y0 + O.BLOCK_Y, H), dtype=dt)
        pxx = xs[None, :].expand(len(ys), len(xs)).reshape(-1)
        pyy = ys[:, None].expand(len(ys), len(xs)).reshape(-1)
        ids = point_list[a:b]
        xy, con, op = pre.xy[ids], pre.conic[ids], pre.opacity[ids]
        dx, dy = xy[:, 0:1] - pxx[None, :], xy[:, 1:2] - pyy[None, :]
        power = -0.5 * (con[:, 0:1] * dx * dx + con[:, 2:3] * dy * dy) - con[:, 1:2] * dx * dy
        alpha = torch.clamp_max(op[:, None] * torch.exp(power), 0.99)
        valid = (power <= 0) & (alpha >= amin)
        near = ((alpha - amin).abs() <= 1e-3 * amin) | (power.abs() <= 1e-5)
        unc = near & (power <= 1e-5) & (alpha >= (1.0 - 1e-3) * amin)       # its own validity may go either way
        vc, vp = valid & ~unc, valid | unc
        a_eff = torch.where(valid, alpha, torch.zeros_like(alpha))
        T_incl = torch.cumprod(1.0 - a_eff, dim=0)
        T_before = torch.cat([torch.ones(1, T_incl.shape[1], dtype=dt), T_incl[:-1]], dim=0)
        k = torch.cumsum(unc.to(torch.int64), dim=0) - unc.to(torch.int64)  # uncertain entries in front
        fk = torch.pow(torch.tensor(f, dtype=dt), k.to(dt))
        T_test = T_before * (1.0 - alpha)
        stop = valid & (T_incl < 1e-4)
        stop_c = vc & (T_test / fk < 0.99e-4)                               # stops whichever way the roundings go
        stop_p = vp & (T_test * fk < 1.01e-4)                               # may stop
        at_or_after = lambda s: torch.cummax(s.to(torch.int8), dim=0).values.bool()
        done, done_c, done_p = at_or_after(stop), at_or_after(stop_c), at_or_after(stop_p)
        seen = T_before > T_min
        seen_c = T_before * (1.0 - 1e-4) * fk > T_min
        seen_p = T_before * (1.0 + 1e-4) / fk > T_min
        for acc, m in ((exact, valid & ~done & seen), (lo, vc & ~done_p & seen_c), (hi, vp & ~done_c & seen_p)):
            acc.index_add_(0, ids, m.sum(dim=1))
    return exact, lo, hi


def oracle_counts(raw, cam, T_min, mode="sh", aa=False, cov=False, raw_act=False, dtype=torch.float64):
    inp = _inputs(raw, dtype, "cpu", mode, cov, raw_act)
    s = settings_for(cam, 3, BG, 1.0, aa)
    op, sc, rot = inp["opacities"], inp.get("scales"), inp.get("rotations")
    if raw_act:
        op, sc, rot = torch.sigmoid(op), torch.exp(sc), torch.nn.functional.normalize(rot)
    geo = dict(cov3D_precomp=inp["cov3D_precomp"]) if cov else dict(scales=sc, rotations=rot)
    shs = torch.cat([inp["dc"], inp["shs"]], dim=1) if mode == "dc" else inp.get("shs")
    with torch.no_grad():
        _, radii, _, st = O.rasterize(inp["means3D"], inp["means2D"], op, s, shs=shs, colors_precomp=inp.get("colors_precomp"),
                                      return_state=True, **geo)
        return band_counts(st["pre"], st["point_list"], st["ranges"], cam.image_width, cam.image_height, T_min) + (radii,)


def hip_touch(raw, cam, T_min=0.5, mode="sh", aa=False, cov=False, raw_act=False, grads=None, touched=True, depth="inverse",
              alpha=False, no_grad=False, bg=BG, **call_kw):
    """One forward through GaussianRasterizer on cuda (+ a backward of <color, gc> + <depth, gd>); n_touched as int64 on the CPU."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    inp = _inputs(raw, torch.float32, "cuda", mode, cov, raw_act)
    s = settings_for(cam, 3, bg, 1.0, aa, cls=GaussianRasterizationSettings, device="cuda")
    kw = dict(shs=inp.get("shs"), colors_precomp=inp.get("colors_precomp"), dc=inp.get("dc"))
    if cov:
        kw["cov3D_precomp"] = inp["cov3D_precomp"]
    else:
        kw.update(scales=inp["scales"], rotations=inp["rotations"])
    if raw_act:
        kw["raw_activations"] = True
    if touched:
        kw.update(n_touched=True, touched_T_min=T_min)
    if depth != "inverse" or alpha:
        kw.update(depth=depth, alpha=alpha)
    with torch.set_grad_enabled(not no_grad):
        res = GaussianRasterizer(s)(means3D=inp["means3D"], means2D=inp["means2D"], opacities=inp["opacities"], **kw, **call_kw)
    out = dict(color=res[0].detach().cpu(), radii=res[1].cpu(), depth=res[2].detach().cpu(), res=res, inputs=inp)
    if touched:
        out["n"] = res[-1].cpu().to(torch.int64)
    if grads is not None:
        gc, gd = grads
        ((res[0] * gc.cuda()).sum() + (res[2] * gd.cuda()).sum()).backward()
        out["grads"] = {k: (v.grad.detach().cpu() if v.grad is not None else None) for k, v in inp.items()}
    torch.cuda.synchronize()
    return out


def _eq(a, b):
    return (a is None and b is None) or (a is not None and b is not None and torch.equal(a, b))


# ------------------------------------------------------------------------------------------------------------------------------
# 1  against the float64 oracle, with the band
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale,T_min,mode,aa,cov,raw_act", [
    (0.6, 0.5, "sh", False, False, False),
    (0.25, 0.5, "sh", False, False, False),
    (0.6, 0.05, "sh", False, False, False),
    (0.25, 0.0, "sh", False, False, False),
    (0.6, 0.5, "sh", True, False, False),          # anti-aliasing
    (0.6, 0.5, "dc", True, False, True),           # dc + rest, raw activations
    (0.6, 0.5, "colors", False, False, False),     # colours given
    (0.6, 0.5, "sh", False, True, False)])         # covariances given
def test_counts_within_the_oracle_band(scale, T_min, mode, aa, cov, raw_act):
    raw, cam = small_scene(scale=scale)
    P = raw.xyz.shape[0]
    exact, lo, hi, radii = oracle_counts(raw, cam, T_min, mode, aa, cov, raw_act)
    e32, _, _, _ = oracle_counts(raw, cam, T_min, mode, aa, cov, raw_act, dtype=torch.float32)
    rows, width, total = int((lo != hi).sum()), int((hi - lo).sum()), int(exact.sum())
    print(f"oracle band: rows with lo != hi {rows} of {P}, sum(hi - lo) {width} of sum(exact) {total}; float32 restatement: "
          f"{int(((e32 < lo) | (e32 > hi)).sum())} rows outside the band, sum|e32 - exact| {int((e32 - exact).abs().sum())}")
    # on the oracle alone: the band is narrow
    assert total > 50000
    assert rows <= 0.10 * P, rows
    assert width <= 0.002 * total, (width, total)
    assert bool(((lo <= exact) & (exact <= hi)).all())
    assert bool(((lo <= e32) & (e32 <= hi)).all())             # the same restatement in float32 stays inside the band
    out = hip_touch(raw, cam, T_min, mode, aa, cov, raw_act, no_grad=True)
    n = out["n"]
    assert out["res"][-1].dtype == torch.int32 and tuple(n.shape) == (P,)
    bad = (n < lo) | (n > hi)
    print(f"hip: sum n_touched {int(n.sum())}, sum|n_hip - exact| {int((n - exact).abs().sum())}, rows != exact "
          f"{int((n != exact).sum())}, rows outside [lo, hi] {int(bad.sum())}")
    assert not bool(bad.any()), [(int(i), int(n[i]), int(lo[i]), int(hi[i])) for i in torch.nonzero(bad).flatten()[:10]]


# ------------------------------------------------------------------------------------------------------------------------------
# 2  exact identity with the instrumented forward
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [0.6, 1.5])
def test_sum_equals_blended_pairs_at_T_min_zero(scale):
    from diff_gaussian_rasterization import GaussianRasterizationSettings, pair_evaluations
    raw, cam = small_scene(scale=scale)
    out = hip_touch(raw, cam, 0.0, no_grad=True)
    inp = out["inputs"]
    rs = settings_for(cam, 3, BG, 1.0, False, cls=GaussianRasterizationSettings, device="cuda")
    pe = pair_evaluations(rs, inp["means3D"], inp["opacities"], shs=inp["shs"], scales=inp["scales"], rotations=inp["rotations"])
    assert pe["fwd_blended"] > 50000
    assert int(out["n"].sum()) == pe["fwd_blended"]


# ------------------------------------------------------------------------------------------------------------------------------
# 3  monotone and bounded
# ------------------------------------------------------------------------------------------------------------------------------
def test_monotone_in_T_min_bounded_and_zero_where_culled():
    raw, cam = small_scene()
    W, H = cam.image_width, cam.image_height
    outs = [hip_touch(raw, cam, t, no_grad=True) for t in T_MINS]
    for a, b in zip(outs[:-1], outs[1:]):
        assert bool((a["n"] >= b["n"]).all())
    assert int(outs[0]["n"].sum()) > int(outs[2]["n"].sum()) > int(outs[3]["n"].sum()) > 0
    for o in outs:
        assert int(o["n"].min()) >= 0 and int(o["n"].max()) <= W * H
        assert int(o["n"][o["radii"] == 0].abs().sum()) == 0
    assert int((outs[0]["radii"] == 0).sum()) > 0


def _wall(x, n=40, half=1.0, opacity=0.99, rgb=(0.8, 0.3, 0.2)):
    """n x n isotropic Gaussians on the plane x = const over [-half, half]^2, spacing = sigma: at every point of the plane the
    nearest one alone has alpha >= 0.99 exp(-1/4) = 0.77, so whatever lies behind is more than half occluded."""
    s = 2.0 * half / n
    g = (torch.arange(n, dtype=torch.float32) + 0.5) * s - half
    yy, zz = torch.meshgrid(g, g, indexing="ij")
    P = n * n
    xyz = torch.stack([torch.full((P,), float(x)), yy.reshape(-1), zz.reshape(-1)], dim=1)
    rot = torch.zeros(P, 4)
    rot[:, 0] = 1
    dc = ((torch.tensor(rgb) - 0.5) / 0.28209479177387814).expand(P, 1, 3).contiguous()
    return RawGaussians(xyz, dc, torch.zeros(P, 15, 3), torch.full((P, 3), math.log(s)), rot,
                        torch.full((P, 1), math.log(opacity / (1 - opacity))), 3)


def _cat(a, b):
    return RawGaussians(*(torch.cat([x, y], dim=0) for x, y in zip(a.tensors(), b.tensors())), 3)


def test_rear_of_two_opaque_coincident_layers_is_not_seen():
    """Two fully opaque layers at the same image positions (the rear one scaled along the viewing rays), both larger than the
    frustum so that no border of the front layer is in view (beyond a border the two layers' tails coincide too, and there the
    rear one IS seen): at T_min = 0.5 every row of the rear layer gets 0 while the front layer is seen in every pixel."""
    front = _wall(-0.2, n=64, half=1.6)
    rear = _wall(-0.2, n=64, half=1.6)
    eye = torch.tensor([-4.0, 0.0, 0.0])
    rear.xyz.copy_(eye + (rear.xyz - eye) * 1.1)
    rear.scaling.add_(math.log(1.1))
    cam = look_at_camera((-4.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 0.6911, 160, 160)
    both = _cat(front, rear)
    P = front.xyz.shape[0]
    n = hip_touch(both, cam, 0.5, no_grad=True)["n"]
    assert int(n[P:].sum()) == 0
    assert int(n[:P].sum()) >= 160 * 160 and int((n[:P] > 0).sum()) > P // 4
    n0 = hip_touch(both, cam, 0.0, no_grad=True)["n"]
    assert bool((n0 >= n).all())


# ------------------------------------------------------------------------------------------------------------------------------
# 4  bit-identity
# ------------------------------------------------------------------------------------------------------------------------------
def _form_scene():
    raw = make_gaussians(6000, 3, seed=401, scale_factor=0.8)
    cam = fibonacci_cameras(3, 208, 144, seed=403)[2]
    return raw, cam


@pytest.mark.parametrize("T_min", [0.0, 0.5])
def test_counts_bit_identical_on_every_path(T_min, monkeypatch):
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _workspace as ws
    raw, cam = _form_scene()
    grads = upstream_grads(cam.image_height, cam.image_width, seed=41)
    with _env(GSR_FWD_MASK=None):
        dgr.set_forward_mode("sync")
        plain = hip_touch(raw, cam, touched=False, grads=grads, aa=True)
        base = hip_touch(raw, cam, T_min, grads=grads, aa=True)
        assert int(base["n"].sum()) > 100000
        # with the option on, every other output and every gradient is the call's without it
        for k in ("color", "radii", "depth"):
            assert torch.equal(base[k], plain[k]), k
        for k in plain["grads"]:
            assert _eq(base["grads"][k], plain["grads"][k]), k
        again = hip_touch(raw, cam, T_min, grads=grads, aa=True)
        assert torch.equal(again["n"], base["n"])                                     # run to run
        fo = hip_touch(raw, cam, T_min, aa=True, no_grad=True)                        # no backward to follow
        assert torch.equal(fo["n"], base["n"]) and torch.equal(fo["color"], base["color"])
        ev = torch.cuda.Event()
        ev.record()
        for mode in ("sync", "exact", "async"):
            for binning in ("tile", "global"):
                monkeypatch.setattr(ws, "_BINNING", binning)
                for kw in ({}, dict(sh_ready_event=ev)):                              # split geometry / shade
                    o = hip_touch(raw, cam, T_min, grads=grads, aa=True, forward_mode=mode, **kw)
                    assert torch.equal(o["n"], base["n"]), (mode, binning, kw)
                    assert torch.equal(o["color"], base["color"])
                    for k in plain["grads"]:
                        assert _eq(o["grads"][k], plain["grads"][k]), (mode, binning, k)
        monkeypatch.undo()
    with _env(GSR_FWD_MASK="1"):
        o = hip_touch(raw, cam, T_min, aa=True, no_grad=True)
        assert torch.equal(o["n"], base["n"])
    with _env(GSR_FWD_MASK=None):
        # depth="z" + alpha ride along: five outputs, the z-depth and the opacity plane those of the call without the counts
        # (final_T and n_contrib: test_state_planes_unchanged_through_the_c_abi)
        o = hip_touch(raw, cam, T_min, aa=True, no_grad=True, depth="z", alpha=True)
        oz = hip_touch(raw, cam, aa=True, no_grad=True, depth="z", alpha=True, touched=False)
        assert torch.equal(o["n"], base["n"]) and len(o["res"]) == 5 and len(oz["res"]) == 4
        assert torch.equal(o["res"][3], oz["res"][3]) and torch.equal(o["depth"], oz["depth"])
        assert torch.equal(o["color"], base["color"]) and torch.equal(o["radii"], base["radii"])
        # tile cull: the cut-offs are learnt by the first calls, then applied (unverified frames)
        dgr.set_forward_mode("async")
        cull = dgr.new_tile_cull(cam.image_height, cam.image_width)
        c0 = dgr.call_stats().get("culled_frames", 0)
        for _ in range(3):
            o = hip_touch(raw, cam, T_min, grads=grads, aa=True, tile_cull=cull)
            dgr.call_stats()
        assert dgr.call_stats().get("culled_frames", 0) > c0
        assert torch.equal(o["n"], base["n"]) and torch.equal(o["color"], base["color"])
        # cut-offs that have become too tight (here: moved to 0.6 of their depth): lists PARTLY truncated, the frame flags
        # itself; the view rendered again without applying them gives the counts of the untruncated frame, once
        finite = cull != -1
        assert int(finite.sum()) > 0
        tight = cull.clone()
        tight[finite] = (cull[finite].view(torch.float32) * 0.6).view(torch.int32)
        m0 = dgr.call_stats().get("cull_miss_frames", 0)
        dgr.take_overflowed()
        flagged = hip_touch(raw, cam, T_min, aa=True, no_grad=True, tile_cull=tight)
        ticket = dgr.last_ticket()
        assert dgr.call_stats().get("cull_miss_frames", 0) == m0 + 1 and ticket in dgr.take_overflowed(wait=True)
        assert 0 < int(flagged["n"].sum()) and not torch.equal(flagged["n"], base["n"])
        o = hip_touch(raw, cam, T_min, aa=True, no_grad=True, tile_cull=tight, tile_cull_apply=False)
        assert torch.equal(o["n"], base["n"]) and torch.equal(o["color"], base["color"])


def test_with_a_backward_fold_and_the_camera_form():
    """A BackwardFold (optimizer step + statistics in the backward) and a camera that requires grad leave the counts alone."""
    import diff_gaussian_rasterization as dgr
    from gaussian_renderer import render, PipelineParams
    from scene_utils import PoseCamera
    cam = fibonacci_cameras(3, 176, 112, seed=91, device="cuda")[0]
    bg = torch.tensor([0.1, 0.2, 0.05], device="cuda")
    model = GaussianModel.from_raw(make_gaussians(3000, 3, seed=93, scale_factor=0.7).to("cuda"))
    with torch.no_grad():
        want = render(cam, model, PipelineParams(), bg, separate_sh=True, n_touched=True)["n_touched"].clone()
    pc = PoseCamera(cam, dtype=torch.float32, device="cuda")
    pkg = render(pc, model, PipelineParams(), bg, separate_sh=True, n_touched=True)
    pkg["render"].sum().backward()
    assert pc.tau.grad is not None and torch.equal(pkg["n_touched"], want)
    opt = model.training_setup(optimizer="hip")
    fold = dgr.BackwardFold(optimizer=opt, stats=(model.xyz_gradient_accum, model.denom, model.max_radii2D))
    pkg = render(cam, model, PipelineParams(), bg, separate_sh=True, fold=fold, n_touched=True)
    got = pkg["n_touched"].clone()
    pkg["render"].mean().backward()
    torch.cuda.synchronize()
    assert fold.optimizer_taken and fold.stats_taken and torch.equal(got, want)


# ------------------------------------------------------------------------------------------------------------------------------
# 5, 6  through the C ABI: nothing counted twice, guard word, refused thresholds, sizes
# ------------------------------------------------------------------------------------------------------------------------------
class _LowLevel:
    def __init__(self, raw, cam, bg=BG, deg=3):
        from diff_gaussian_rasterization import _C, GaussianRasterizationSettings, _settings_struct, _gauss_struct
        self.C, self.lib = _C, _C.lib()
        inp = leaf_inputs(raw, torch.float32, "cuda", "sh")
        self.t = {k: v.detach().contiguous() for k, v in inp.items()}
        t = self.t
        self.P, self.H, self.W = t["means3D"].shape[0], cam.image_height, cam.image_width
        rs = settings_for(cam, deg, bg, 1.0, False, cls=GaussianRasterizationSettings, device="cuda")
        self.s, self.keep = _settings_struct(rs, "cuda")
        self.g = _gauss_struct(self.P, t["means3D"], None, t["shs"], None, t["opacities"], t["scales"], t["rotations"], None)
        self.new_state()

    def new_state(self):
        lib, P, W, H = self.lib, self.P, self.W, self.H
        self.geom = torch.zeros(lib.gsr_geometry_state_bytes(P), dtype=torch.uint8, device="cuda")
        self.img = torch.zeros(lib.gsr_image_state_bytes(W, H), dtype=torch.uint8, device="cuda")
        self.radii = torch.zeros(P, dtype=torch.int32, device="cuda")
        self.color, self.invd = torch.full((3, H, W), -7.0, device="cuda"), torch.full((1, H, W), -7.0, device="cuda")

    def buf(self):
        """[P + 1] words of 0xFFFFFFFF: the library owns the zeroing of [P]; the last word is the guard."""
        return torch.full((self.P + 1,), -1, dtype=torch.int32, device="cuda")

    def extras(self, buf, T_min):
        return self.C.gsr_render_extras(0, None, None, self.C.ptr(buf), T_min)

    def binning(self, cap):
        return torch.zeros(self.lib.gsr_binning_state_bytes(self.P, self.W, self.H, cap), dtype=torch.uint8, device="cuda")

    def blocking(self, buf, T_min, for_backward=1):
        """gsr_forward_prepare_ex + gsr_forward_render_ex; buf = None: extras == NULL, the entry points without _ex."""
        from diff_gaussian_rasterization import _stream
        _C, lib = self.C, self.lib
        ex = self.extras(buf, T_min) if buf is not None else None
        exp = C.byref(ex) if ex is not None else None
        R = lib.gsr_forward_prepare_ex(C.byref(self.s), C.byref(self.g), _C.ptr(self.geom), self.geom.numel(), _C.ptr(self.radii),
                                       _stream(), exp)
        if R < 0:
            return R
        b = self.binning(R)
        rc = lib.gsr_forward_render_ex(C.byref(self.s), C.byref(self.g), _C.ptr(self.geom), _C.ptr(b), b.numel(), R,
                                       _C.ptr(self.img), self.img.numel(), _C.ptr(self.color), _C.ptr(self.invd), for_backward,
                                       _stream(), exp)
        torch.cuda.synchronize()
        return rc if rc < 0 else R

    def planes(self):
        """CPU copies of everything the compositing forward writes: colour, depth, radii, final_T, n_contrib."""
        from helpers import _view
        pi = [C.c_void_p() for _ in range(2)]
        self.lib.gsr_debug_image_views(self.C.ptr(self.img), self.W, self.H, C.byref(pi[0]), C.byref(pi[1]))
        n = self.W * self.H
        return dict(color=self.color.cpu(), invd=self.invd.cpu(), radii=self.radii.cpu(),
                    final_T=_view(self.img, pi[0].value, n, torch.float32), n_contrib=_view(self.img, pi[1].value, n, torch.int32))

    def async_culled(self, buf, T_min, cap, b, tlo, count=None, cutoff=None, apply=0):
        from diff_gaussian_rasterization import _stream
        _C = self.C
        ex = self.extras(buf, T_min)
        self.status = torch.zeros(4, dtype=torch.int64).pin_memory()
        rc = self.lib.gsr_forward_async_culled_ex(
            C.byref(self.s), C.byref(self.g), _C.ptr(self.geom), self.geom.numel(), _C.ptr(self.radii), _C.ptr(b), b.numel(), cap,
            _C.ptr(self.img), self.img.numel(), _C.ptr(self.color), _C.ptr(self.invd), 1, 0, None,
            C.c_void_p(self.status.data_ptr()), tlo, _stream(), C.byref(count) if count is not None else None, _C.ptr(cutoff),
            apply, C.byref(ex))
        return rc

    def rerender(self, buf, T_min, cap, b, tlo):
        from diff_gaussian_rasterization import _stream
        _C = self.C
        ex = self.extras(buf, T_min)
        return self.lib.gsr_forward_rerender_ex(C.byref(self.s), C.byref(self.g), _C.ptr(self.geom), _C.ptr(b), b.numel(), cap,
                                                _C.ptr(self.img), self.img.numel(), _C.ptr(self.color), _C.ptr(self.invd), 1, tlo,
                                                C.c_void_p(self.status.data_ptr()), _stream(), C.byref(ex))


def _counts(buf):
    torch.cuda.synchronize()
    assert int(buf[-1]) == -1, "guard word behind [P] overwritten"
    return buf[:-1].cpu().to(torch.int64)


@pytest.mark.parametrize("for_backward", [0, 1])
@pytest.mark.parametrize("mask", [None, "1"])
def test_state_planes_unchanged_through_the_c_abi(mask, for_backward):
    """With n_touched in the extras, colour, radii, depth, final_T and n_contrib (gsr_debug_image_views) are bit for bit those of
    the call with extras == NULL: the plain and the GSR_FWD_MASK=1 walk, with and without a backward to follow."""
    raw, cam = small_scene()
    ll = _LowLevel(raw, cam)
    with _env(GSR_FWD_MASK=mask):
        assert ll.blocking(None, 0.0, for_backward) > 0
        plain = ll.planes()
        assert float(plain["final_T"].min()) < 0.5 and int(plain["n_contrib"].max()) > 0
        counts = {}
        for T_min in (0.0, 0.5):
            ll.new_state()
            buf = ll.buf()
            assert ll.blocking(buf, T_min, for_backward) > 0
            counts[T_min] = _counts(buf)
            got = ll.planes()
            for k, v in plain.items():
                assert torch.equal(got[k], v), (T_min, k)
    assert int(counts[0.0].sum()) > int(counts[0.5].sum()) > 0
    with _env(GSR_FWD_MASK=None):                            # ... and the counts are those of the Python call, default walk
        assert torch.equal(counts[0.5], hip_touch(raw, cam, 0.5, no_grad=True)["n"])


@pytest.mark.parametrize("tlo", [0, 1])
def test_async_frame_whose_capacity_did_not_hold_counts_once(tlo):
    """gsr_forward_async_ex(num_rendered_out) with a third of the needed capacity (the forcing of test_async_forward_gpu), then
    gsr_forward_rerender_ex into the SAME buffer - and once more: the counts are the blocking path's, not a multiple."""
    raw = make_gaussians(4000, 3, seed=7, scale_factor=0.8)
    cam = fibonacci_cameras(1, 176, 112, seed=11)[0]
    ll = _LowLevel(raw, cam)
    ref_buf = ll.buf()
    R = ll.blocking(ref_buf, 0.5)
    assert R > 4096
    ref = _counts(ref_buf)
    assert int(ref.sum()) > 10000
    ll.new_state()
    buf = ll.buf()
    small = max(256, R // 3)
    count = C.c_int64(-1)
    assert ll.async_culled(buf, 0.5, small, ll.binning(small), tlo, count=count) == 0
    assert count.value == R > small
    truncated = _counts(buf)
    assert int(truncated.sum()) == 0                # a frame truncated by its capacity reports zeros, like its gradients
    cap = R + 17
    big = ll.binning(cap)
    assert ll.rerender(buf, 0.5, cap, big, tlo) == 0
    assert torch.equal(_counts(buf), ref)
    assert ll.rerender(buf, 0.5, cap, big, tlo) == 0          # an explicit re-render into the same buffer
    assert torch.equal(_counts(buf), ref)
    assert ll.rerender(buf, 0.0, cap, big, tlo) == 0          # ... also with another threshold
    assert int(_counts(buf).sum()) > int(ref.sum())


def test_culled_frame_rendered_again_counts_once():
    """gsr_forward_async_culled_ex: frame 1 learns the cut-offs, frame 2 applies them (same counts: the walk never reached what
    was cut), frame 3 with cut-offs in front of everything flags itself; the view rendered again untruncated into the same buffer
    gives the blocking path's counts."""
    raw = make_gaussians(4000, 1, seed=151, scale_factor=2.5)
    cam = fibonacci_cameras(2, 192, 128, seed=152)[0]
    ll = _LowLevel(raw, cam, bg=torch.zeros(3), deg=1)
    tiles = (192 // 16) * (128 // 16)
    ref_buf = ll.buf()
    R = ll.blocking(ref_buf, 0.5)
    ref = _counts(ref_buf)
    assert R > 0 and int(ref.sum()) > 10000
    cap = 1 << 20
    cut = torch.full((tiles,), -1, dtype=torch.int32, device="cuda")
    buf = ll.buf()
    ll.new_state()
    assert ll.async_culled(buf, 0.5, cap, ll.binning(cap), 1, cutoff=cut, apply=0) == 0
    assert torch.equal(_counts(buf), ref) and int(ll.status[1]) == R
    ll.new_state()
    assert ll.async_culled(buf, 0.5, cap, ll.binning(cap), 1, cutoff=cut, apply=1) == 0
    assert torch.equal(_counts(buf), ref)
    assert int(ll.status[1]) < 0.8 * R and int(ll.status[3]) & 0xFFFFFFFF == 0
    zero = torch.zeros_like(cut)
    ll.new_state()
    assert ll.async_culled(buf, 0.5, cap, ll.binning(cap), 1, cutoff=zero, apply=1) == 0
    flagged = _counts(buf)
    assert int(ll.status[3]) & 0xFFFFFFFF == 1 and int(flagged.sum()) == 0
    ll.new_state()
    assert ll.async_culled(buf, 0.5, cap, ll.binning(cap), 1, cutoff=zero, apply=0) == 0     # the view again, untruncated
    assert torch.equal(_counts(buf), ref)
    # the more telling case: a frame PARTLY truncated - every fourth tile cut off in front of everything (that flags the frame),
    # every fourth moved to 0.85 of its learnt depth, the rest as learnt - flags itself with counts of its own in the buffer;
    # the view again, untruncated, into the same buffer: the blocking path's counts, once
    tight = cut.clone()
    idx = torch.arange(tiles, device="cuda")
    nearer = (cut != -1) & (idx % 4 == 2)
    tight[nearer] = (cut[nearer].view(torch.float32) * 0.85).view(torch.int32)
    tight[idx % 4 == 0] = 0
    ll.new_state()
    assert ll.async_culled(buf, 0.5, cap, ll.binning(cap), 1, cutoff=tight.clone(), apply=1) == 0
    part = _counts(buf)
    assert int(ll.status[3]) & 0xFFFFFFFF == 1 and 0 < int(ll.status[1]) < R
    assert 0 < int(part.sum()) and not torch.equal(part, ref)
    ll.new_state()
    assert ll.async_culled(buf, 0.5, cap, ll.binning(cap), 1, cutoff=tight, apply=0) == 0
    assert torch.equal(_counts(buf), ref)


def test_python_modes_count_once_when_phase_two_is_repeated(monkeypatch):
    """Default mode with a capacity estimate that does not hold (phase 2 repeated by the wrapper): the blocking path's counts."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _workspace as ws
    raw = make_gaussians(5000, 3, seed=403, scale_factor=0.9)
    cam = fibonacci_cameras(2, 160, 96, seed=402)[0]
    dgr.set_forward_mode("sync")
    ref = hip_touch(raw, cam, 0.5, no_grad=True)
    R = dgr.call_stats()["num_rendered"]
    dgr.set_forward_mode("exact")
    pool = ws.pool(torch.device("cuda", 0))
    old_min, ws.MIN_CAPACITY = ws.MIN_CAPACITY, 256
    try:
        pool.capacity[(5000, 160, 96)] = max(256, R // 3)
        for w in pool.free:
            w.binning = w.scratch = None
        n_re = dgr.call_stats()["rerendered_frames"]
        out = hip_touch(raw, cam, 0.5, no_grad=True)
        assert dgr.call_stats()["rerendered_frames"] == n_re + 1
        assert torch.equal(out["n"], ref["n"]) and torch.equal(out["color"], ref["color"])
    finally:
        ws.MIN_CAPACITY = old_min


def test_bad_thresholds_are_refused_with_outputs_untouched():
    raw, cam = small_scene(P=500)
    ll = _LowLevel(raw, cam)
    for bad in (1.0, -0.1, float("nan")):
        buf = ll.buf()
        ll.new_state()
        assert ll.blocking(buf, bad) == -1 and "touched_T_min" in ll.C.last_error()
        cap = 1 << 16
        assert ll.async_culled(buf, bad, cap, ll.binning(cap), 1) == -1
        torch.cuda.synchronize()
        assert int((buf != -1).sum()) == 0 and int(ll.radii.abs().sum()) == 0
        assert float((ll.color + 7.0).abs().max()) == 0.0 and float((ll.invd + 7.0).abs().max()) == 0.0
    # the threshold is only looked at when counts are asked for
    from diff_gaussian_rasterization import _stream
    ex = ll.C.gsr_render_extras(0, None, None, None, 5.0)
    assert ll.lib.gsr_forward_prepare_ex(C.byref(ll.s), C.byref(ll.g), ll.C.ptr(ll.geom), ll.geom.numel(), ll.C.ptr(ll.radii),
                                         _stream(), C.byref(ex)) >= 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("P", [1, 63, 65, 257, 3001])
def test_sizes_straddling_workgroups_and_the_guard_word(P):
    raw = make_gaussians(P, 3, seed=100 + P, scale_factor=0.6 if P > 100 else 0.2)
    cam = fibonacci_cameras(3, 150, 100, seed=5)[1]
    ll = _LowLevel(raw, cam)
    buf = ll.buf()
    assert ll.blocking(buf, 0.0) >= 0
    n = _counts(buf)                                           # (checks the guard word)
    want = hip_touch(raw, cam, 0.0, no_grad=True)
    assert torch.equal(n, want["n"])
    assert int(n[want["radii"] == 0].sum()) == 0 and int(n.sum()) > 0


# ------------------------------------------------------------------------------------------------------------------------------
# 7  Python surface
# ------------------------------------------------------------------------------------------------------------------------------
def test_python_surface(monkeypatch):
    from diff_gaussian_rasterization import _C
    from gaussian_renderer import render, PipelineParams
    raw, cam = small_scene(P=800)
    camd = fibonacci_cameras(3, 150, 100, seed=5, device="cuda")[1]
    model = GaussianModel.from_raw(raw.to("cuda"))
    bg = BG.cuda()
    pkg = render(camd, model, PipelineParams(), bg)
    assert "n_touched" not in pkg and set(pkg.keys()) == {"render", "viewspace_points", "visibility_filter", "radii", "depth"}
    pkg = render(camd, model, PipelineParams(), bg, n_touched=True)
    n = pkg["n_touched"]
    assert n.dtype == torch.int32 and tuple(n.shape) == (800,) and not n.requires_grad and pkg["render"].requires_grad
    pkg["render"].sum().backward()                             # the extra output does not disturb the backward
    assert model._xyz.grad is not None
    pkg0 = render(camd, model, PipelineParams(), bg, n_touched=True, touched_T_min=0.0)
    assert bool((pkg0["n_touched"] >= n).all()) and int(pkg0["n_touched"].sum()) > int(n.sum())
    # composes with depth="z", alpha=True: five outputs in the stated order
    out = hip_touch(raw, cam, 0.5, depth="z", alpha=True)
    res = out["res"]
    assert len(res) == 5 and tuple(res[3].shape) == (1, 100, 150) and res[3].dtype == torch.float32
    assert res[4].dtype == torch.int32 and not res[4].requires_grad and res[3].requires_grad
    assert torch.equal(res[4], n)
    pkg = render(camd, model, PipelineParams(), bg, depth="z", alpha=True, n_touched=True)
    assert {"alpha", "n_touched"} <= set(pkg.keys()) and torch.equal(pkg["n_touched"], n)
    # arguments are validated before any device work
    for bad, exc in ((1, TypeError), ("yes", TypeError), (None, TypeError)):
        with pytest.raises(exc):
            render(camd, model, PipelineParams(), bg, n_touched=bad)
    for bad, exc in ((1.0, ValueError), (-0.1, ValueError), (float("nan"), ValueError), ("0.5", TypeError), (True, TypeError)):
        with pytest.raises(exc):
            hip_touch(raw, cam, bad)
        with pytest.raises(exc):
            render(camd, model, PipelineParams(), bg, n_touched=True, touched_T_min=bad)
    # under HIP-graph capture the option raises (the capture state is what the forward asks torch for)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(_C.GsrError, match="graph capture"):
        hip_touch(raw, cam, 0.5, no_grad=True)


# ------------------------------------------------------------------------------------------------------------------------------
# 8  loop rehearsal at small size
# ------------------------------------------------------------------------------------------------------------------------------
def test_opposite_views_of_a_wall_are_covisible_to_radii_but_not_to_n_touched():
    """The scene: an opaque wall of two layers (x = -0.2 and x = +0.2, each 40 x 40 Gaussians whose spacing equals their sigma, so
    the layer in front hides the one behind: see _wall), looked at from x = -4 and from x = +4.  Every Gaussian projects into both
    frustums (radii > 0 in both: IoU = 1), but each view blends, at T > 0.5, only the layer facing it."""
    from gaussian_renderer import render, PipelineParams
    from scene_utils import covisibility, KeyframeWindow
    model = GaussianModel.from_raw(_cat(_wall(-0.2), _wall(0.2)).to("cuda"), requires_grad=False)
    bg = torch.zeros(3, device="cuda")
    pk = []
    for x in (-4.0, 4.0):
        cam = look_at_camera((x, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 0.6911, 160, 160, device="cuda")
        with torch.no_grad():
            pk.append(render(cam, model, PipelineParams(), bg, n_touched=True))
    iou_r, ov_r = covisibility(pk[0]["radii"] > 0, pk[1]["radii"] > 0)
    iou_t, ov_t = covisibility(pk[0]["n_touched"], pk[1]["n_touched"])
    print(f"wall: radii IoU {iou_r:.3f} overlap {ov_r:.3f}; n_touched IoU {iou_t:.3f} overlap {ov_t:.3f}")
    assert int((pk[0]["n_touched"] > 0).sum()) >= 1600
    assert iou_r > iou_t
    cutoff = 0.4                                   # KeyframeWindow.add's default
    assert ov_t < cutoff < ov_r
    # what the window makes of it: with n_touched the far side is a new keyframe and, two keyframes later, leaves the window
    w = KeyframeWindow(4)
    assert w.is_keyframe(pk[0]["n_touched"]) and w.add("front", pk[0]["n_touched"]) == []
    assert w.is_keyframe(pk[1]["n_touched"]) and not w.is_keyframe(pk[0]["n_touched"])
    assert w.add("back", pk[1]["n_touched"]) == []
    assert w.add("back2", pk[1]["n_touched"]) == ["front"]
    wr = KeyframeWindow(4)
    wr.add("front", pk[0]["radii"] > 0)
    assert not wr.is_keyframe(pk[1]["radii"] > 0)


def test_insert_then_prune_unobserved_with_a_trainer_attached():
    from gaussian_renderer import render, PipelineParams
    from scene_utils import Trainer, KeyframeWindow, prune_unobserved, make_config
    from scene_utils.model import _PARAM_ATTRS
    from test_mapping_gpu import _scene
    cams, frames, bg = _scene(P=6000, W=160, H=128, views=6)
    pipe = PipelineParams()
    model = GaussianModel.from_raw(make_gaussians(3000, 3, seed=5, scale_factor=0.5).to("cuda"))
    gts = {i: f[0] for i, f in enumerate(frames)}
    tr = Trainer(model, cams, gts, render, pipe, bg, separate_sh=True, optimizer="hip_fused")
    for it in range(4):
        tr.step(it % 3)
    tr.finish()
    P0 = model.get_xyz.shape[0]
    with torch.no_grad():
        pkg = render(cams[4], model, pipe, bg, depth="z", alpha=True)
    n_new = model.add_from_rgbd(cams[4], frames[4][0], frames[4][1], render_pkg=pkg, stride=2)
    assert n_new > 0
    P1 = P0 + n_new
    tr.step(4)
    tr.finish()

    def counts(i):
        with torch.no_grad():
            return render(cams[i], model, pipe, bg, separate_sh=True, n_touched=True)["n_touched"].clone()
    window = KeyframeWindow(4)
    for i in (3, 4, 5):
        window.add(i, counts(i), overlap_cutoff=0.0)
    assert len(window) == 3
    obs = window.observations()
    candidates = torch.zeros(P1, dtype=torch.bool, device="cuda")
    candidates[P0:] = True
    # the bound is chosen from the scene so that the prune is neither empty nor total: the smallest number of keyframes that some
    # of the new rows reach and some do not
    hist = torch.bincount(obs[P0:].cpu().to(torch.int64), minlength=4).tolist()
    print(f"inserted rows by number of window keyframes that see them: {hist}")
    ks = [k for k in (1, 2, 3) if 0 < int((obs[P0:] < k).sum()) < n_new]
    assert ks, hist
    min_kf = ks[0]
    mask = candidates & (obs.cuda() < min_kf)
    want = int(mask.sum())
    old = [getattr(model, a).detach().clone() for a in _PARAM_ATTRS]
    old_m = [(model.optimizer.state[getattr(model, a)]["exp_avg"].clone(),
              model.optimizer.state[getattr(model, a)]["exp_avg_sq"].clone()) for a in _PARAM_ATTRS]
    stats = [model.xyz_gradient_accum.clone(), model.denom.clone(), model.max_radii2D.clone()]
    removed = prune_unobserved(model, window, candidates, min_keyframes=min_kf)
    keep = ~mask
    assert removed == want and model.get_xyz.shape[0] == P1 - want
    groups = {g["name"]: g for g in model.optimizer.param_groups}
    for a, name, o, (m1, m2) in zip(_PARAM_ATTRS, ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"), old, old_m):
        p = getattr(model, a)
        assert p.requires_grad and p.is_contiguous() and torch.equal(p.detach(), o[keep])
        assert groups[name]["params"][0] is p
        st = model.optimizer.state[p]
        assert torch.equal(st["exp_avg"], m1[keep]) and torch.equal(st["exp_avg_sq"], m2[keep])
    assert len(model.optimizer.state) == 6
    for t, o in zip((model.xyz_gradient_accum, model.denom, model.max_radii2D), stats):
        assert torch.equal(t, o[keep])
    assert torch.equal(window.observations().cpu(), obs.cpu()[keep.cpu()])
    for i in (3, 4, 5):                                         # the renderer and the window agree on the new length
        window.is_keyframe(counts(i))
    out = tr.step(4)                                            # the trainer goes on: its step sees the pruned model
    tr.finish()
    assert torch.isfinite(out["loss"])
    assert torch.isfinite(tr.step(1)["loss"])
    tr.finish()
    assert model.prune_points(torch.zeros(P1 - want, dtype=torch.bool, device="cuda")) == 0

