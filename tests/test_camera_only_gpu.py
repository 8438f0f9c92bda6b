"""The camera-only backward (GaussianRasterizer.forward(..., camera_only=True), gsr_backward_camera_only): the tracking form of
the camera backward - the map is frozen, so no per-Gaussian gradient is formed or stored.  The acceptance test is bit identity of
the three camera gradients with the full camera form (gsr_backward_camera), not a tolerance: same terms, same sums, same order."""
import ctypes as C

import pytest
import torch

from helpers import leaf_inputs, settings_for, upstream_grads
from oracle import gs_oracle as O
from scene_utils import make_gaussians, fibonacci_cameras, look_at_camera, PoseCamera
from scene_utils.synthetic import RawGaussians

pytestmark = pytest.mark.gpu

BG = torch.tensor([0.2, 0.5, 0.7])
NAN_BITS = 0x7FC0DEAD          # the fill of caller-owned buffers: a quiet NaN no kernel computes


@pytest.fixture(autouse=True)
def _restore_mode():
    import diff_gaussian_rasterization as dgr
    mode = dgr.forward_mode()
    yield
    dgr.set_forward_mode(mode)


def cam_leaves(cam, dtype, device):
    return [t.detach().to(device=device, dtype=dtype).clone().requires_grad_(True)
            for t in (cam.world_view_transform, cam.full_proj_transform, cam.camera_center)]


def _inputs(raw, mode, cov):
    inp = leaf_inputs(raw, torch.float32, "cuda", mode)
    if cov:
        c = O.cov3d_from_scale_rot(inp["scales"].detach().cpu().double(), inp["rotations"].detach().cpu().double(), 1.0)
        inp["cov3D_precomp"] = c.to(device="cuda", dtype=torch.float32).requires_grad_(True)
        del inp["scales"], inp["rotations"]          # (not inputs of a cov3D call: every leaf left is one the call takes)
    return inp


def hip_call(raw, cam, mode="sh", aa=False, cov=False, extras=False, deg=3, camera_only=False, want=(True, True, True),
             fold=None, **call_kw):
    """One forward + backward through GaussianRasterizer on the device, every Gaussian tensor a leaf that requires grad.  extras:
    depth="z", alpha=True with upstream gradients for both planes (else the inverse depth's).
    -> (camera grads [3] (None where no .grad), per-Gaussian .grad dict, radii)"""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    inp = _inputs(raw, mode, cov)
    leaves = [t if w else t.detach() for t, w in zip(cam_leaves(cam, torch.float32, "cuda"), want)]
    s = settings_for(cam, deg, BG, 1.0, aa, cls=GaussianRasterizationSettings, device="cuda")._replace(
        viewmatrix=leaves[0], projmatrix=leaves[1], campos=leaves[2])
    kw = dict(shs=inp.get("shs"), colors_precomp=inp.get("colors_precomp"), dc=inp.get("dc"))
    if cov:
        kw["cov3D_precomp"] = inp["cov3D_precomp"]
    else:
        kw.update(scales=inp["scales"], rotations=inp["rotations"])
    if extras:
        kw.update(depth="z", alpha=True)
    if camera_only:
        kw["camera_only"] = True
    if fold is not None:
        kw["fold"] = fold
    out = GaussianRasterizer(s)(means3D=inp["means3D"], means2D=inp["means2D"], opacities=inp["opacities"], **kw, **call_kw)
    H, W = cam.image_height, cam.image_width
    gc, gd = upstream_grads(H, W)
    loss = (out[0] * gc.cuda()).sum() + (out[2] * gd.cuda()).sum()
    if extras:
        ga = torch.randn(1, H, W, generator=torch.Generator().manual_seed(17))
        loss = loss + (out[3] * ga.cuda()).sum()
    loss.backward()
    torch.cuda.synchronize()
    cg = [None if t.grad is None else t.grad.detach().cpu() for t in leaves]
    grads = {k: (None if v.grad is None else v.grad.detach().cpu()) for k, v in inp.items()}
    return cg, grads, out[1].cpu()


def _subset(raw, idx):
    return RawGaussians(*(t[idx].clone() for t in raw.tensors()), raw.sh_degree)


def _visible_first(raw, cam, P):
    """P Gaussians of `raw` whose centres project well inside `cam`'s image, in front of it, with opacity > 0.3 (each one, the
    last in particular, has tile instances: tests/test_camera_grad_paths_gpu.py)."""
    vm, pm = cam.world_view_transform.double(), cam.full_proj_transform.double()
    x = raw.xyz.double()
    z = x @ vm[:3, 2] + vm[3, 2]
    hom = x @ pm[:3] + pm[3]
    ndc = hom[:, :2] / hom[:, 3:4]
    ok = (z > 0.5) & (ndc.abs() < 0.7).all(dim=1) & (torch.sigmoid(raw.opacity[:, 0].double()) > 0.3)
    idx = torch.nonzero(ok).flatten()
    assert idx.numel() >= P, (idx.numel(), P)
    return _subset(raw, idx[:P])


_SCENES = {}


def _scene(P):
    """(raw, cam) at 150x100 with exactly P Gaussians, all visible (so the last one of a partial workgroup counts)."""
    if P not in _SCENES:
        cam = fibonacci_cameras(3, 150, 100, seed=5)[1]
        big = make_gaussians(max(4 * P, 2000), 3, seed=21 + P, scale_factor=0.6)
        _SCENES[P] = (_visible_first(big, cam, P), cam)
    return _SCENES[P]


FORMS = [("sh", False, False), ("dc", True, False), ("colors", False, False), ("sh", False, True)]
# staged (active degree = stored: 64 Gaussians per workgroup) and unstaged (degree 1 of 3: 256 per workgroup) instantiations, at
# the partial-workgroup sizes tests/test_camera_grad_paths_gpu.py found necessary
SIZES = [(1, 3), (63, 3), (65, 3), (3001, 3), (1, 1), (255, 1), (257, 1)]


@pytest.mark.parametrize("extras", [False, True])
@pytest.mark.parametrize("mode,aa,cov", FORMS)
@pytest.mark.parametrize("P,deg", SIZES)
def test_camera_only_is_bit_identical_to_the_full_camera_form(P, deg, mode, aa, cov, extras):
    raw, cam = _scene(P)
    full, gfull, radii = hip_call(raw, cam, mode, aa, cov, extras, deg)
    only, gonly, radii2 = hip_call(raw, cam, mode, aa, cov, extras, deg, camera_only=True)
    assert int(radii[P - 1]) > 0 and torch.equal(radii, radii2)
    for i, (a, b) in enumerate(zip(only, full)):
        assert a is not None and b is not None
        assert torch.equal(a, b), (i, float((a - b).abs().max()))
    assert float(full[0].abs().max()) > 0 and float(full[1].abs().max()) > 0
    if mode != "colors" and deg > 0:
        assert float(full[2].abs().max()) > 0
    assert all(g is not None for g in gfull.values())                # (the full form fills every leaf ...)
    assert float(gfull["means3D"].abs().max()) > 0
    for k, g in gonly.items():                                       # (... the camera-only form none, means2D included)
        assert g is None, k


@pytest.mark.parametrize("which", [0, 1, 2])
def test_camera_only_partial_requests(which):
    """Only one of the three camera tensors requires grad: its gradient equals the full form's, the others get none."""
    raw, cam = _scene(3001)
    full, _, _ = hip_call(raw, cam)
    want = tuple(i == which for i in range(3))
    one, g, _ = hip_call(raw, cam, camera_only=True, want=want)
    for i in range(3):
        if i == which:
            assert torch.equal(one[i], full[i])
        else:
            assert one[i] is None
    assert all(v is None for v in g.values())


def test_camera_only_allocates_no_gradient_arena(monkeypatch):
    import diff_gaussian_rasterization as dgr
    calls = []
    real = dgr._grad_arena
    monkeypatch.setattr(dgr, "_grad_arena", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    raw, cam = _scene(3001)
    hip_call(raw, cam)
    assert len(calls) == 1
    hip_call(raw, cam, camera_only=True)
    assert len(calls) == 1


def test_empty_and_facing_away_give_exact_zeros():
    """test_empty_and_facing_away_give_zero_camera_grads' scenes: P = 0, and a camera outside the cloud looking away from it."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    raw = make_gaussians(3000, 3, seed=11, scale_factor=0.6)
    cam = fibonacci_cameras(3, 150, 100, seed=5)[1]
    away = look_at_camera((4.0, 0.0, 0.0), (8.0, 0.0, 0.0), (0.0, 0.0, 1.0), 0.6911, 150, 100)
    for P in (0, 3000):
        c = cam if P == 0 else away
        leaves = cam_leaves(c, torch.float32, "cuda")
        inp = leaf_inputs(raw, torch.float32, "cuda", "sh")
        inp = {k: v.detach()[:P] for k, v in inp.items()}
        s = settings_for(c, 3, BG, cls=GaussianRasterizationSettings, device="cuda")._replace(
            viewmatrix=leaves[0], projmatrix=leaves[1], campos=leaves[2])
        color, radii, invd = GaussianRasterizer(s)(inp["means3D"], inp["means2D"], inp["opacities"], shs=inp["shs"],
                                                   scales=inp["scales"], rotations=inp["rotations"], camera_only=True)
        assert int((radii > 0).sum()) == 0
        (color.sum() + invd.sum()).backward()
        torch.cuda.synchronize()
        for t in leaves:
            assert t.grad is not None and t.grad.dtype == torch.float32 and not t.grad.any(), (P, t.grad)


def test_truncated_async_frame_gives_exact_zeros_and_is_reported(monkeypatch):
    """An "async" frame beyond a forced-small binning capacity (test_async_overflow_frame_gives_zero_camera_grads' set-up): the
    camera-only backward is a no-op like every other - exact-zero camera gradients, a verified-zero result, not a fault - and the
    frame is reported by take_overflowed()."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _workspace as ws
    monkeypatch.setattr(ws, "_BINNING", "global")
    raw = make_gaussians(5000, 3, seed=301, scale_factor=0.7)
    cam = fibonacci_cameras(2, 160, 96, seed=302)[0]
    dgr.set_forward_mode("sync")
    ref, _, _ = hip_call(raw, cam, camera_only=True)
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
            out, grads, _ = hip_call(raw, cam, camera_only=True)
            ticket = dgr.last_ticket()
            st = dgr.call_stats()           # (the frame's status is looked at - and the overflow reported - here)
        assert st["overflow_frames"] == n0 + 1 and st["num_rendered"] == R
        assert dgr.take_overflowed() == [ticket]
        for i, t in enumerate(out):
            assert t is not None and not t.any(), (i, t)
        assert all(g is None for g in grads.values())
        again, _, _ = hip_call(raw, cam, camera_only=True)          # the capacity was raised: the next frame is exact
        for x, y in zip(again, ref):
            assert torch.equal(x, y)
    finally:
        ws.MIN_CAPACITY = old_min


def test_camera_only_needs_the_camera_form():
    from diff_gaussian_rasterization import _C
    raw, cam = _scene(63)
    with pytest.raises(_C.GsrError, match="camera form"):
        hip_call(raw, cam, camera_only=True, want=(False, False, False))
    with torch.no_grad():
        with pytest.raises(_C.GsrError, match="camera form"):
            hip_call(raw, cam, camera_only=True)


def test_camera_only_refuses_a_backward_fold():
    from diff_gaussian_rasterization import _C, BackwardFold
    raw, cam = _scene(63)
    stats = tuple(torch.zeros(63, 1, device="cuda") for _ in range(2)) + (torch.zeros(63, device="cuda"),)
    with pytest.raises(_C.GsrError, match="BackwardFold"):
        hip_call(raw, cam, camera_only=True, fold=BackwardFold(stats=stats))


def test_render_passes_camera_only_through():
    """render(..., camera_only=True) with a host PoseCamera: tau.grad equals (bitwise) the one of the plain tracking call."""
    from gaussian_renderer import render, PipelineParams
    from scene_utils.model import GaussianModel
    raw, cam = _scene(3001)
    model = GaussianModel.from_raw(raw.to("cuda"), requires_grad=True)
    gc, _ = upstream_grads(cam.image_height, cam.image_width)
    taus = []
    for only in (False, True):
        pc = PoseCamera(cam, dtype=torch.float32, device="cuda")
        for p in (model._xyz, model._features_dc, model._features_rest, model._opacity, model._scaling, model._rotation):
            p.grad = None
        pkg = render(pc, model, PipelineParams(), BG.cuda(), **({"camera_only": True} if only else {}))
        (pkg["render"] * gc.cuda()).sum().backward()
        torch.cuda.synchronize()
        taus.append(pc.tau.grad.detach().cpu())
        assert (model._xyz.grad is None) == only and (pkg["viewspace_points"].grad is None) == only
    assert torch.equal(taus[0], taus[1]) and float(taus[0].abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------------------------
# the C ABI directly
# ------------------------------------------------------------------------------------------------------------------------------
GUARD = 4096


def _abi_backward_camera_only(P, deg, W=64, H=48, scratch_short=0):
    """gsr_forward_prepare + gsr_forward_render + gsr_backward_camera_only on caller-owned buffers; the camera scratch is
    gsr_camera_grad_scratch_bytes(P) - scratch_short bytes followed by GUARD bytes, all filled with NAN_BITS first."""
    from diff_gaussian_rasterization import _C, GaussianRasterizationSettings, _settings_struct, _gauss_struct, _stream
    lib = _C.lib()
    dev = "cuda"
    cam = fibonacci_cameras(3, W, H, seed=78)[0]
    raw = make_gaussians(P, 3, seed=77, scale_factor=0.5)
    t = {k: v.detach().contiguous() for k, v in leaf_inputs(raw, torch.float32, dev, "sh").items()}
    rs = settings_for(cam, deg, BG, 1.0, False, cls=GaussianRasterizationSettings, device=dev)
    s, keep = _settings_struct(rs, dev)
    g = _gauss_struct(P, t["means3D"], None, t["shs"], None, t["opacities"], t["scales"], t["rotations"], None)
    geom = torch.zeros(lib.gsr_geometry_state_bytes(P), dtype=torch.uint8, device=dev)
    img = torch.zeros(lib.gsr_image_state_bytes(W, H), dtype=torch.uint8, device=dev)
    radii = torch.zeros(P, dtype=torch.int32, device=dev)
    color = torch.empty(3, H, W, device=dev)
    invd = torch.empty(1, H, W, device=dev)
    R = _C.check(lib.gsr_forward_prepare(C.byref(s), C.byref(g), _C.ptr(geom), geom.numel(), _C.ptr(radii), _stream()))
    binning = torch.zeros(max(1, lib.gsr_binning_state_bytes(P, W, H, R)), dtype=torch.uint8, device=dev)
    _C.check(lib.gsr_forward_render(C.byref(s), C.byref(g), _C.ptr(geom), _C.ptr(binning), binning.numel(), R,
                                    _C.ptr(img), img.numel(), _C.ptr(color), _C.ptr(invd), 1, _stream()))
    gc, gd = upstream_grads(H, W, seed=79)
    gc, gd = gc.cuda().contiguous(), gd.cuda().contiguous()
    scratch = torch.zeros(max(1, lib.gsr_backward_scratch_bytes(P, R)), dtype=torch.uint8, device=dev)
    need = lib.gsr_camera_grad_scratch_bytes(P)
    have = need - scratch_short
    cam_scratch = torch.full(((have + GUARD + 3) // 4,), NAN_BITS, dtype=torch.int32, device=dev)
    outs = torch.full((16 + 16 + 3,), NAN_BITS, dtype=torch.int32, device=dev)
    cs = _C.gsr_camera_grads(outs.data_ptr(), outs.data_ptr() + 64, outs.data_ptr() + 128)
    torch.cuda.synchronize()
    rc = lib.gsr_backward_camera_only(C.byref(s), C.byref(g), _C.ptr(radii), _C.ptr(geom), _C.ptr(binning), _C.ptr(img), R,
                                      _C.ptr(gc), _C.ptr(gd), _C.ptr(scratch), scratch.numel(), C.byref(cs),
                                      cam_scratch.data_ptr(), have, _stream())
    torch.cuda.synchronize()
    return dict(rc=rc, scratch=cam_scratch.cpu().numpy(), need=need, outs=outs.cpu().numpy())


def test_camera_scratch_one_byte_short_is_refused():
    """Mirrors test_camera_scratch_one_byte_short: GSR_ERR_STATE_TOO_SMALL before anything is launched, outputs untouched; with
    the full size the same call succeeds, writes every output and nothing behind the scratch."""
    from diff_gaussian_rasterization import _C
    r = _abi_backward_camera_only(1000, 3, scratch_short=1)
    assert r["rc"] == -5          # GSR_ERR_STATE_TOO_SMALL
    assert (r["outs"] == NAN_BITS).all() and (r["scratch"] == NAN_BITS).all()
    assert "camera scratch" in _C.lib().gsr_last_error().decode()
    ok = _abi_backward_camera_only(1000, 3)
    assert ok["rc"] == 0 and (ok["outs"] != NAN_BITS).all()
    assert (ok["scratch"][ok["need"] // 4:] == NAN_BITS).all(), "write past the camera scratch"
