"""Camera gradients (gsr_backward_camera) on the kernel paths the small scene of tests/test_camera_grad_gpu.py never reaches:

  A  float64-oracle parity: active SH degree below the stored one (the unstaged 256-thread camera instantiation), scale_modifier,
     partial last workgroups of both instantiations, big splats with the gradient records' validity flags off / on, and calls
     that ask for only one of the three camera tensors;
  B  invariance to the compositing-backward form, walk order, sub-block masks, binning form and forward mode; an "async" frame
     truncated by its capacity;
  C  full frame size (C3, 1 M Gaussians at 1080p; 200 k with anti-aliasing) against the oracle on sampled tiles;
  D  the C ABI directly: k_cam_reduce's levels restated bit for bit in numpy (tests/helpers.py), no write past the scratch, the
     scratch-size check;
  E  dL/dtau of the tracking objective (render() + fused L1 / D-SSIM) through PoseCamera, on the device and on the host.

The bar is the suite's: per camera tensor rel-L2 <= 1e-4 and max-abs <= 1e-4 max|g| against the float64 oracle (CAM_REL)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from helpers import (leaf_inputs, settings_for, upstream_grads, rel_l2, cam_reduce_levels, cam_slots_to_grads, CAM_SLOTS,
                     CAM_RED_ROWS)
from oracle import gs_oracle as O
from scene_utils import make_gaussians, make_config, fibonacci_cameras, PoseCamera, GaussianModel
from scene_utils.synthetic import RawGaussians
from test_camera_grad_gpu import CAM_REL, cam_leaves, check_camera

pytestmark = pytest.mark.gpu

BG = torch.tensor([0.2, 0.5, 0.7])
NAN_BITS = 0x7FC0DEAD          # the fill of the caller-owned buffers: a quiet NaN no kernel computes


@pytest.fixture(autouse=True)
def _restore_mode():
    import diff_gaussian_rasterization as dgr
    mode = dgr.forward_mode()
    yield
    dgr.set_forward_mode(mode)


class _env:
    """Sets environment switches of the library for a block, restoring the previous values (test_walk_order_changes_no_bit)."""

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


def _gauss_kw(inp, mode):
    return dict(shs=inp.get("shs"), colors_precomp=inp.get("colors_precomp"), dc=inp.get("dc"), scales=inp["scales"],
                rotations=inp["rotations"])


def oracle_cam(raw, cam, deg, mode="sh", aa=False, depth=True, sm=1.0, gc=None, gd=None, tiles=None, bg=BG,
               dtype=torch.float64):
    """Camera gradients of <color, gc> (+ <invdepth, gd>) from the oracle's autograd, the three tensors as `dtype` leaves."""
    inp = leaf_inputs(raw, dtype, "cpu", mode)
    vm, pm, cp = cam_leaves(cam, dtype, "cpu")
    s = settings_for(cam, deg, bg, sm, aa)._replace(viewmatrix=vm, projmatrix=pm, campos=cp)
    shs = torch.cat([inp["dc"], inp["shs"]], dim=1) if mode == "dc" else inp.get("shs")
    color, radii, invd = O.rasterize(inp["means3D"], inp["means2D"], inp["opacities"], s, shs=shs,
                                     colors_precomp=inp.get("colors_precomp"), scales=inp["scales"], rotations=inp["rotations"],
                                     tiles=tiles)
    if gc is None:
        gc, gd = upstream_grads(cam.image_height, cam.image_width)
    loss = (color * gc.to(dtype)).sum()
    if depth:
        loss = loss + (invd * gd.to(dtype)).sum()
    loss.backward()
    return [torch.zeros_like(t) if t.grad is None else t.grad.detach() for t in (vm, pm, cp)], radii


def hip_cam(raw, cam, deg, mode="sh", aa=False, depth=True, sm=1.0, gc=None, gd=None, bg=BG, want=(True, True, True),
            **call_kw):
    """One forward + backward through GaussianRasterizer; the camera tensors require grad where `want` says so.
    -> (camera grads [3] (None where no .grad), per-Gaussian grads dict, radii)"""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    inp = leaf_inputs(raw, torch.float32, "cuda", mode)
    leaves = [t if w else t.detach() for t, w in zip(cam_leaves(cam, torch.float32, "cuda"), want)]
    s = settings_for(cam, deg, bg, sm, aa, cls=GaussianRasterizationSettings, device="cuda")._replace(
        viewmatrix=leaves[0], projmatrix=leaves[1], campos=leaves[2])
    color, radii, invd = GaussianRasterizer(s)(means3D=inp["means3D"], means2D=inp["means2D"], opacities=inp["opacities"],
                                               **_gauss_kw(inp, mode), **call_kw)
    if gc is None:
        gc, gd = upstream_grads(cam.image_height, cam.image_width)
    loss = (color * gc.cuda()).sum()
    if depth:
        loss = loss + (invd * gd.cuda()).sum()
    loss.backward()
    torch.cuda.synchronize()
    cg = [None if t.grad is None else t.grad.detach().cpu() for t in leaves]
    grads = {k: (None if v.grad is None else v.grad.detach().cpu()) for k, v in inp.items()}
    return cg, grads, radii.cpu()


def _subset(raw, idx):
    return RawGaussians(*(t[idx].clone() for t in raw.tensors()), raw.sh_degree)


def _visible_first(raw, cam, P):
    """P Gaussians of `raw` whose centres project well inside `cam`'s image, in front of it, with opacity > 0.3 (so that each
    one, the last in particular, has tile instances)."""
    vm, pm = cam.world_view_transform.double(), cam.full_proj_transform.double()
    x = raw.xyz.double()
    z = x @ vm[:3, 2] + vm[3, 2]
    hom = x @ pm[:3] + pm[3]
    ndc = hom[:, :2] / hom[:, 3:4]
    ok = (z > 0.5) & (ndc.abs() < 0.7).all(dim=1) & (torch.sigmoid(raw.opacity[:, 0].double()) > 0.3)
    idx = torch.nonzero(ok).flatten()
    assert idx.numel() >= P, (idx.numel(), P)
    return _subset(raw, idx[:P])


def _check_nonzero(out, ref):
    """(check_camera compares; this makes sure there was something to compare)"""
    for g, r in zip(out, ref):
        assert float(r.abs().max()) > 0 and float(g.abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------------------------
# A  oracle parity on the paths the small scene misses
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deg,mode,aa,depth", [(0, "sh", False, True), (1, "sh", False, True), (2, "sh", False, False),
                                               (0, "dc", False, False), (1, "dc", True, True), (2, "dc", False, True)])
def test_active_degree_below_stored(deg, mode, aa, depth):
    """16 stored coefficients, active degree 0 / 1 / 2: the camera instantiation without LDS staging (256 Gaussians per
    workgroup).  Degree 0: no view-dependent colour, dL/dcampos is exactly zero in both; degrees 1, 2: SH drives it."""
    raw = make_gaussians(3000, 3, seed=11, scale_factor=0.6)
    cam = fibonacci_cameras(3, 150, 100, seed=5)[1]
    ref, _ = oracle_cam(raw, cam, deg, mode, aa, depth)
    out, _, _ = hip_cam(raw, cam, deg, mode, aa, depth)
    check_camera(out, ref)
    if deg == 0:
        assert torch.all(out[2] == 0) and torch.all(ref[2] == 0), (out[2], ref[2])
    else:
        assert float(ref[2].abs().max()) > 0 and float(out[2].abs().max()) > 0
        assert rel_l2(out[2], ref[2]) <= CAM_REL


@pytest.mark.parametrize("sm", [0.7, 1.4])
def test_scale_modifier(sm):
    raw = make_gaussians(3000, 3, seed=12, scale_factor=0.6)
    cam = fibonacci_cameras(3, 150, 100, seed=5)[1]
    ref, _ = oracle_cam(raw, cam, 3, sm=sm)
    out, _, _ = hip_cam(raw, cam, 3, sm=sm)
    check_camera(out, ref)
    _check_nonzero(out, ref)


@pytest.mark.parametrize("P,deg", [(1, 3), (63, 3), (65, 3), (3001, 3), (1, 1), (255, 1), (257, 1)])
def test_partial_last_workgroup(P, deg):
    """Partial last workgroup of the staged (deg 3 = stored: 64 Gaussians per workgroup) and the unstaged (deg 1 of 3: 256 per
    workgroup) camera instantiation.  Idle lanes mirror Gaussian P - 1 and must add nothing: the scene keeps only Gaussians that
    project inside the image, and the test asserts that the LAST one is visible (radii[P - 1] > 0) - with an invisible tail
    Gaussian a double count would add zeros and go unnoticed."""
    big = make_gaussians(max(4 * P, 2000), 3, seed=21 + P, scale_factor=0.6)
    cam = fibonacci_cameras(3, 150, 100, seed=5)[1]
    raw = _visible_first(big, cam, P)
    ref, radii_ref = oracle_cam(raw, cam, deg)
    out, _, radii = hip_cam(raw, cam, deg)
    assert int(radii[P - 1]) > 0 and int(radii_ref[P - 1]) > 0
    check_camera(out, ref)
    _check_nonzero(out, ref)


def test_big_splats_validity_flags_off_and_on():
    """800 big splats at 208x144 (many Gaussians with more than 16 instances: the second flag chunk), the validity flags of the
    gradient records forced off, then on: both within the bar, and bit-identical to each other."""
    from diff_gaussian_rasterization import _C
    lib = _C.lib()
    raw = make_gaussians(800, 3, seed=431, scale_factor=2.5)
    cam = fibonacci_cameras(3, 208, 144, seed=433)[0]
    ref, _ = oracle_cam(raw, cam, 3, aa=True)
    before = lib.gsr_debug_set_flags_min_r(-1)
    try:
        lib.gsr_debug_set_flags_min_r(0xFFFFFFFF)
        a, ga, _ = hip_cam(raw, cam, 3, aa=True)
        lib.gsr_debug_set_flags_min_r(0)
        b, gb, _ = hip_cam(raw, cam, 3, aa=True)
    finally:
        lib.gsr_debug_set_flags_min_r(before)
    from helpers import lowlevel_forward
    tt = lowlevel_forward(raw, cam, 3, BG, antialiasing=True)["tiles_touched"]
    assert int((tt > 16).sum()) >= 50, int((tt > 16).sum())
    check_camera(a, ref)
    check_camera(b, ref)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k


@pytest.mark.parametrize("which", [0, 1, 2])
def test_partial_camera_requests(which):
    """Only one of viewmatrix / projmatrix / campos requires grad: its gradient equals (bitwise) the one of the call that asks
    for all three, and the other two get no .grad."""
    raw = make_gaussians(3000, 3, seed=11, scale_factor=0.6)
    cam = fibonacci_cameras(3, 150, 100, seed=5)[1]
    full, gfull, _ = hip_cam(raw, cam, 3)
    want = tuple(i == which for i in range(3))
    one, gone, _ = hip_cam(raw, cam, 3, want=want)
    for i in range(3):
        if i == which:
            assert one[i] is not None and torch.equal(one[i], full[i]), i
        else:
            assert one[i] is None, i
    for k in gfull:
        assert torch.equal(gfull[k], gone[k]), k


# ------------------------------------------------------------------------------------------------------------------------------
# B  form invariance
# ------------------------------------------------------------------------------------------------------------------------------
def _form_scene():
    raw = make_gaussians(6000, 3, seed=401, scale_factor=0.8)
    cam = fibonacci_cameras(3, 208, 144, seed=403)[2]
    return raw, cam


_UNSET = dict(GSR_BWD_FORM=None, GSR_BWD_LPT=None, GSR_BWD_MASK=None, GSR_BWD_REDUCE=None)


@pytest.mark.parametrize("name,env,binning,fmode", [
    ("tile", dict(GSR_BWD_FORM="tile"), None, None),
    ("quad", dict(GSR_BWD_FORM="quad"), None, None),
    ("lpt0", dict(GSR_BWD_LPT="0"), None, None),
    ("lpt1", dict(GSR_BWD_LPT="1"), None, None),
    ("tile-lpt0", dict(GSR_BWD_FORM="tile", GSR_BWD_LPT="0"), None, None),
    ("tile-lpt1", dict(GSR_BWD_FORM="tile", GSR_BWD_LPT="1"), None, None),
    ("tile-mask0", dict(GSR_BWD_FORM="tile", GSR_BWD_MASK="0"), None, None),
    ("tile-mask1", dict(GSR_BWD_FORM="tile", GSR_BWD_MASK="1"), None, None),
    ("mfma", dict(GSR_BWD_FORM="tile", GSR_BWD_REDUCE="mfma"), None, None),
    ("global", {}, "global", None),
    ("exact", {}, None, "exact"),
    ("sync", {}, None, "sync"),
    ("async", {}, None, "async")])
def test_camera_grads_form_invariant(name, env, binning, fmode, monkeypatch):
    """208x144, 6000 Gaussians, inverse depth + anti-aliasing (117 tiles: the four-wave form by default).  Walk order, sub-block
    masks, binning form and forward mode change no bit of the camera gradients: each call equals its compositing-backward
    form's default call (quad, or GSR_BWD_FORM=tile).  The two forms, and the opt-in matrix-pipe reduction, add the sums inside a
    tile in different fixed orders - the per-Gaussian gradients differ in the last bits too - so across them the camera
    gradients agree within 2e-6 rel-L2, and each is within the bar of the float64 oracle.  In every form the per-Gaussian
    gradients equal, bit for bit, the same form's call without a camera leaf."""
    from diff_gaussian_rasterization import _workspace as ws
    raw, cam = _form_scene()
    tile_form = env.get("GSR_BWD_FORM") == "tile"
    with _env(**_UNSET):
        base, _, _ = hip_cam(raw, cam, 3, aa=True)
    if tile_form:
        with _env(**{**_UNSET, "GSR_BWD_FORM": "tile"}):
            base_tile, _, _ = hip_cam(raw, cam, 3, aa=True)
    if binning is not None:
        monkeypatch.setattr(ws, "_BINNING", binning)
    kw = {} if fmode is None else dict(forward_mode=fmode)
    with _env(**{**_UNSET, **env}):
        out, g_cam, _ = hip_cam(raw, cam, 3, aa=True, **kw)
        none, g_plain, _ = hip_cam(raw, cam, 3, aa=True, want=(False, False, False), **kw)
    assert all(t is None for t in none)
    for k in g_plain:
        assert torch.equal(g_cam[k], g_plain[k]), (name, k)
    assert float(g_cam["means3D"].abs().sum()) > 0
    same = base_tile if tile_form and name != "mfma" else base
    if name != "mfma":
        for i, (x, y) in enumerate(zip(out, same)):
            assert torch.equal(x, y), (name, i, float((x - y).abs().max()))
    if name in ("tile", "mfma"):
        for x, y in zip(out, base):
            assert rel_l2(x, y) <= 2e-6, rel_l2(x, y)
        ref, _ = oracle_cam(raw, cam, 3, aa=True)
        check_camera(out, ref)
        check_camera(base, ref)


def test_async_overflow_frame_gives_zero_camera_grads(monkeypatch):
    """An "async" frame beyond its binning capacity (test_async_capacity_overflow_is_contained_reported_and_heals): its backward
    is a no-op - the camera gradients are exact zeros like every other gradient - and the frame is reported by ticket."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _workspace as ws
    monkeypatch.setattr(ws, "_BINNING", "global")
    raw = make_gaussians(5000, 3, seed=301, scale_factor=0.7)
    cam = fibonacci_cameras(2, 160, 96, seed=302)[0]
    dgr.set_forward_mode("sync")
    ref, _, _ = hip_cam(raw, cam, 3)
    R = dgr.call_stats()["num_rendered"]
    assert R > 4096 and all(float(t.abs().max()) > 0 for t in ref)
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
            out, grads, _ = hip_cam(raw, cam, 3)
            ticket = dgr.last_ticket()
            st = dgr.call_stats()           # (the frame's status is looked at - and the overflow reported - here)
        assert st["overflow_frames"] == n0 + 1 and st["num_rendered"] == R
        assert dgr.take_overflowed() == [ticket]
        for i, t in enumerate(out):
            assert t is not None and not t.any(), (i, t)
        for k, g in grads.items():
            assert not g.any(), k
        again, _, _ = hip_cam(raw, cam, 3)          # the capacity was raised: the next frame is exact
        for x, y in zip(again, ref):
            assert torch.equal(x, y)
    finally:
        ws.MIN_CAPACITY = old_min


# ------------------------------------------------------------------------------------------------------------------------------
# C  full frame size, sampled-tile oracle
# ------------------------------------------------------------------------------------------------------------------------------
def _tile_mask(W, H, n, seed):
    gx, gy = (W + 15) // 16, (H + 15) // 16
    gen = torch.Generator().manual_seed(seed)
    tiles = sorted(torch.randperm(gx * gy, generator=gen)[:n].tolist())
    mask = torch.zeros(1, H, W)
    for t in tiles:
        ty, tx = divmod(t, gx)
        mask[:, ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] = 1
    return tiles, mask


def _cam_err(g, r):
    r = r.double()
    return rel_l2(g, r), float((g.double() - r).abs().max() / (r.abs().max() + 1e-30))


@pytest.mark.parametrize("P,aa", [(1_000_000, False), (200_000, True)])
def test_full_size_sampled_tiles(P, aa):
    """C3 (1920x1080, SH 3): the tile form of the compositing backward, walk order and validity flags on, the side-stream colour
    pass, and at 1 M Gaussians two reduction levels of the camera sums (15 625 -> 123 -> 1 rows).  The upstream gradients are
    masked to 32 random tiles and the oracle renders just those tiles: a Gaussian outside them adds exact zeros on both sides,
    so the comparison covers the whole sum.  Tolerance per tensor: max(CAM_REL, 2 x the float32 oracle's own error).
    Measured once (MI355X), rel-L2 / max-abs over max|g| against the float64 oracle:
                                  HIP                  float32 oracle
      1 M      viewmatrix   2.09e-5 / 1.57e-5     1.81e-5 / 1.75e-5
               projmatrix   2.71e-5 / 1.79e-5     3.21e-5 / 2.83e-5
               campos       1.19e-5 / 1.69e-5     6.39e-6 / 8.29e-6
      200 k AA viewmatrix   5.78e-6 / 6.05e-6     5.37e-6 / 5.02e-6
               projmatrix   4.16e-5 / 4.98e-5     2.99e-5 / 3.05e-5
               campos       8.49e-7 / 1.02e-6     3.65e-7 / 4.51e-7
    (within CAM_REL everywhere: no kernel change was called for)."""
    raw, cams, c = make_config(3, P=P, views=4)
    cam, W, H = cams[1], c["W"], c["H"]
    assert (W, H) == (1920, 1080)
    tiles, mask = _tile_mask(W, H, 32, seed=31)
    gc, gd = upstream_grads(H, W, seed=32)
    gc, gd = gc * mask, gd * mask
    bg = torch.tensor([0.02, 0.03, 0.04])
    out, _, _ = hip_cam(raw, cam, 3, aa=aa, gc=gc, gd=gd, bg=bg)
    out2, _, _ = hip_cam(raw, cam, 3, aa=aa, gc=gc, gd=gd, bg=bg)
    for x, y in zip(out, out2):
        assert torch.equal(x, y)
    ref, _ = oracle_cam(raw, cam, 3, aa=aa, gc=gc, gd=gd, tiles=tiles, bg=bg)
    ref32, _ = oracle_cam(raw, cam, 3, aa=aa, gc=gc, gd=gd, tiles=tiles, bg=bg, dtype=torch.float32)
    for name, g, r, r32 in zip(("viewmatrix", "projmatrix", "campos"), out, ref, ref32):
        e, m = _cam_err(g, r)
        e32, m32 = _cam_err(r32, r)
        print(f"P={P} aa={aa} {name}: HIP rel-L2 {e:.3e} max {m:.3e}; float32 oracle rel-L2 {e32:.3e} max {m32:.3e}")
        assert float(r.abs().max()) > 0
        assert e <= max(CAM_REL, 2 * e32) and m <= max(CAM_REL, 2 * m32), (name, e, m, e32, m32)
    assert torch.all(out[0].flatten()[[3, 7, 11, 15]] == 0) and torch.all(out[1].flatten()[[2, 6, 10, 14]] == 0)


# ------------------------------------------------------------------------------------------------------------------------------
# D  the reduction and the scratch contract through the C ABI
# ------------------------------------------------------------------------------------------------------------------------------
GUARD = 4096


def _abi_backward_camera(P, deg, W=64, H=48, scratch_short=0):
    """gsr_forward_prepare + gsr_forward_render + gsr_backward_camera on caller-owned buffers; the camera scratch is
    gsr_camera_grad_scratch_bytes(P) - scratch_short bytes followed by GUARD bytes, all filled with NAN_BITS first.
    -> dict(rc, scratch (int32 words, host), need (bytes), outs (dV, dPV, dcam as int32 words, host))"""
    from diff_gaussian_rasterization import _C, GaussianRasterizationSettings, _settings_struct, _gauss_struct, _stream
    lib = _C.lib()
    dev = "cuda"
    cam = fibonacci_cameras(3, W, H, seed=78)[0]
    if P < 1000:        # (every Gaussian of a small P in view: the last one's terms must count)
        raw = _visible_first(make_gaussians(2000, 3, seed=77, scale_factor=0.5), cam, max(P, 1))
    else:
        raw = make_gaussians(P, 3, seed=77, scale_factor=0.5)
    inp = leaf_inputs(raw, torch.float32, dev, "sh")
    # (P = 0: one-row buffers behind the pointers, the struct says P = 0)
    t = {k: v.detach().contiguous() for k, v in inp.items()}
    rs = settings_for(cam, deg, BG, 1.0, False, cls=GaussianRasterizationSettings, device=dev)
    s, keep = _settings_struct(rs, dev)
    g = _gauss_struct(P, t["means3D"], None, t["shs"], None, t["opacities"], t["scales"], t["rotations"], None)
    geom = torch.zeros(lib.gsr_geometry_state_bytes(P), dtype=torch.uint8, device=dev)
    img = torch.zeros(lib.gsr_image_state_bytes(W, H), dtype=torch.uint8, device=dev)
    radii = torch.zeros(max(P, 1), dtype=torch.int32, device=dev)
    color = torch.empty(3, H, W, device=dev)
    invd = torch.empty(1, H, W, device=dev)
    R = _C.check(lib.gsr_forward_prepare(C.byref(s), C.byref(g), _C.ptr(geom), geom.numel(), _C.ptr(radii), _stream()))
    binning = torch.zeros(max(1, lib.gsr_binning_state_bytes(P, W, H, R)), dtype=torch.uint8, device=dev)
    _C.check(lib.gsr_forward_render(C.byref(s), C.byref(g), _C.ptr(geom), _C.ptr(binning), binning.numel(), R,
                                    _C.ptr(img), img.numel(), _C.ptr(color), _C.ptr(invd), 1, _stream()))
    gc, gd = upstream_grads(H, W, seed=79)
    gc, gd = gc.cuda().contiguous(), gd.cuda().contiguous()
    scratch = torch.zeros(max(1, lib.gsr_backward_scratch_bytes(P, R)), dtype=torch.uint8, device=dev)
    n = max(P, 1)
    bufs = dict(m3=torch.empty(n, 3, device=dev), m2=torch.empty(n, 3, device=dev), sh=torch.empty(n, 16, 3, device=dev),
                op=torch.empty(n, 1, device=dev), sc=torch.empty(n, 3, device=dev), ro=torch.empty(n, 4, device=dev))
    gr = _C.gsr_grads(*[b.data_ptr() for b in (bufs["m3"], bufs["m2"])], None, bufs["sh"].data_ptr(), None,
                      *[b.data_ptr() for b in (bufs["op"], bufs["sc"], bufs["ro"])], None, None, None, None)
    need = lib.gsr_camera_grad_scratch_bytes(P)
    assert need % 4 == 0 and need >= CAM_SLOTS * 4
    have = need - scratch_short
    cam_scratch = torch.full(((have + GUARD + 3) // 4,), NAN_BITS, dtype=torch.int32, device=dev)
    outs = torch.full((16 + 16 + 3,), NAN_BITS, dtype=torch.int32, device=dev)
    cs = _C.gsr_camera_grads(outs.data_ptr(), outs.data_ptr() + 64, outs.data_ptr() + 128)
    torch.cuda.synchronize()
    rc = lib.gsr_backward_camera(C.byref(s), C.byref(g), _C.ptr(radii), _C.ptr(geom), _C.ptr(binning), _C.ptr(img), R,
                                 _C.ptr(gc), _C.ptr(gd), _C.ptr(scratch), scratch.numel(), C.byref(gr), C.byref(cs),
                                 cam_scratch.data_ptr(), have, _stream())
    torch.cuda.synchronize()
    return dict(rc=rc, scratch=cam_scratch.cpu().numpy(), need=need, have=have, outs=outs.cpu().numpy(), R=R,
                visible=int((radii[:P] > 0).sum()))


@pytest.mark.parametrize("P,deg", [(0, 3), (1, 3), (64, 3), (8192, 3), (8193, 3), (1_048_577, 3),
                                   (1, 1), (8193, 1), (32_768, 1), (32_769, 1)])
def test_cam_reduce_bit_exact_and_scratch_bounds(P, deg):
    """The partial rows the backward leaves in the caller's scratch (64 Gaussians per row with staged SH, deg 3 = stored; 256
    unstaged, deg 1 of 3), replayed through tests/helpers.py's float32 restatement of k_cam_reduce: every intermediate level
    and the three outputs bit for bit (slot map and always-zero entries included); nothing written behind the last level, the
    guard after the scratch untouched; the float32 sum within 1e-6 sum|rows| of the float64 sum of the rows."""
    r = _abi_backward_camera(P, deg)
    assert r["rc"] == 0
    words = r["scratch"]
    nfl = r["need"] // 4
    assert (words[nfl:] == NAN_BITS).all(), "write past the camera scratch"
    outs = r["outs"].view(np.float32)
    dV, dPV, dcam = outs[:16], outs[16:32], outs[32:]
    if P == 0:
        assert (r["outs"] == 0).all()         # +0.0 everywhere
        return
    bt = 64 if deg == 3 else 256
    n0 = (P + bt - 1) // bt
    fl = words[:nfl].view(np.float32).reshape(-1, CAM_SLOTS)
    rows = fl[:n0]
    assert (rows.view(np.int32) != NAN_BITS).all() and np.isfinite(rows).all()
    levels, tot = cam_reduce_levels(rows)
    off = n0
    for lv in levels:
        got = fl[off:off + lv.shape[0]]
        assert np.array_equal(got.view(np.int32), lv.view(np.int32)), (off, lv.shape)
        off += lv.shape[0]
    assert (fl[off:].view(np.int32) == NAN_BITS).all()      # the rest of the scratch: never written
    if P == 1_048_577:
        assert [lv.shape[0] for lv in levels] == [129, 2]
    elif n0 > CAM_RED_ROWS:
        assert len(levels) == 1
    wV, wPV, wc = cam_slots_to_grads(tot)
    for got, want in ((dV, wV), (dPV, wPV), (dcam, wc)):
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (got, want)
    assert (rows[:, 27:] == 0).all()
    exact = rows.astype(np.float64).sum(axis=0)
    scale = np.abs(rows.astype(np.float64)).sum(axis=0)
    assert (np.abs(tot.astype(np.float64) - exact) <= 1e-6 * scale).all()
    assert r["visible"] > 0 and np.abs(tot[:24]).max() > 0
    if deg > 0:
        assert np.abs(dcam).max() > 0


def test_camera_scratch_one_byte_short():
    from diff_gaussian_rasterization import _C
    r = _abi_backward_camera(1000, 3, scratch_short=1)
    assert r["rc"] == -5          # GSR_ERR_STATE_TOO_SMALL
    assert (r["outs"] == NAN_BITS).all() and (r["scratch"] == NAN_BITS).all()
    assert "camera scratch" in _C.lib().gsr_last_error().decode()


# ------------------------------------------------------------------------------------------------------------------------------
# E  the tracking objective end to end
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("separate_sh", [False, True])
@pytest.mark.parametrize("host", [False, True])
def test_tracking_objective_dtau(separate_sh, host):
    """dL/dtau of render() + training_loss_fused(lambda 0.2) through PoseCamera (tau != 0) against the same PoseCamera in float64
    on the CPU driving the oracle + oracle.loss_oracle.training_loss.  host: the PoseCamera as refine_pose builds it (float64 on
    the host; the rasterizer takes the matrices to the device and returns the gradients in float64 on the CPU)."""
    from gaussian_renderer import render, PipelineParams
    from scene_utils.losses import training_loss_fused
    from oracle.loss_oracle import training_loss
    raw = make_gaussians(3000, 3, seed=11, scale_factor=0.6)
    cam = fibonacci_cameras(3, 150, 100, seed=5)[1]
    tau0 = torch.tensor([0.01, -0.02, 0.015, 0.004, -0.006, 0.003], dtype=torch.float64)
    gen = torch.Generator().manual_seed(9)
    gt = torch.rand(3, 150, 100, generator=gen).transpose(1, 2).contiguous()
    # oracle
    pc_ref = PoseCamera(cam, dtype=torch.float64, device="cpu")
    with torch.no_grad():
        pc_ref.tau.copy_(tau0)
    inp = leaf_inputs(raw, torch.float64, "cpu", "sh")
    inp = {k: v.detach() for k, v in inp.items()}
    s = settings_for(pc_ref, 3, torch.zeros(3, dtype=torch.float64))
    color, _, _ = O.rasterize(inp["means3D"], inp["means2D"], inp["opacities"], s, shs=inp["shs"], scales=inp["scales"],
                              rotations=inp["rotations"])
    training_loss(color, gt.double(), 0.2).backward()
    ref = pc_ref.tau.grad.detach().clone()
    # HIP
    model = GaussianModel.from_raw(raw.to("cuda"), requires_grad=False)
    pc = PoseCamera(cam, dtype=torch.float64, device="cpu") if host else PoseCamera(cam, dtype=torch.float32, device="cuda")
    with torch.no_grad():
        pc.tau.copy_(tau0.to(pc.tau.dtype))
    image = render(pc, model, PipelineParams(), torch.zeros(3, device="cuda"), separate_sh=separate_sh)["render"]
    training_loss_fused(image, gt.cuda(), 0.2).backward()
    torch.cuda.synchronize()
    out = pc.tau.grad
    assert out is not None and out.dtype == pc.tau.dtype and out.device == pc.tau.device
    out = out.detach().cpu()
    assert float(ref.abs().max()) > 0
    assert rel_l2(out, ref) <= CAM_REL, (out, ref)
    assert float((out.double() - ref).abs().max() / ref.abs().max()) <= CAM_REL, (out, ref)
