"""The autograd contract of every backward form of the rasterizer through the public call (GaussianRasterizer.forward): how
many outputs come back and in which order, which inputs get a `.grad` and of which shape, what the camera tensors get.  No
numerical value is compared here - the parity tests do that; this is what a miscounted return tuple of the backward breaks."""
import pytest
import torch

from helpers import leaf_inputs, settings_for
from oracle import gs_oracle as O
from scene_utils import make_gaussians, fibonacci_cameras

pytestmark = pytest.mark.gpu

P_FULL, W, H, DEG = 300, 48, 32, 1          # a 3 x 2 tile grid with partial tiles
BG = torch.tensor([0.2, 0.5, 0.7])
INPUTS = ["shs", "dc+shs", "colors_precomp", "cov3D_precomp"]
_SCENE = []


def _scene():
    if not _SCENE:
        _SCENE.append((make_gaussians(P_FULL, DEG, seed=77, scale_factor=0.6), fibonacci_cameras(2, W, H, seed=5)[0]))
    return _SCENE[0]


def _leaves(inputs, P):
    """The Gaussian tensors of one call form as fresh leaves that require grad, cut to P rows."""
    raw, _ = _scene()
    inp = leaf_inputs(raw, torch.float32, "cuda", {"shs": "sh", "dc+shs": "dc", "colors_precomp": "colors"}.get(inputs, "sh"))
    if inputs == "cov3D_precomp":
        c = O.cov3d_from_scale_rot(inp["scales"].detach().cpu().double(), inp["rotations"].detach().cpu().double(), 1.0)
        inp["cov3D_precomp"] = c.to(device="cuda", dtype=torch.float32)
        del inp["scales"], inp["rotations"]
    return {k: v.detach()[:P].clone().requires_grad_(True) for k, v in inp.items()}


def _run(inputs, form, extras, P):
    """-> (outputs, Gaussian leaves, camera leaves (None: not the camera form), fold)"""
    from diff_gaussian_rasterization import BackwardFold, GaussianRasterizationSettings, GaussianRasterizer
    _, cam = _scene()
    inp = _leaves(inputs, P)
    s = settings_for(cam, DEG, BG, cls=GaussianRasterizationSettings, device="cuda")
    cam_leaves = None
    if form in ("camera", "camera_only"):
        # (the view matrix in float64: each camera gradient comes back in its own input's dtype)
        cam_leaves = [t.detach().to(device="cuda", dtype=dt).clone().requires_grad_(True) for t, dt in
                      ((cam.world_view_transform, torch.float64), (cam.full_proj_transform, torch.float32),
                       (cam.camera_center, torch.float32))]
        s = s._replace(viewmatrix=cam_leaves[0], projmatrix=cam_leaves[1], campos=cam_leaves[2])
    kw = {k: v for k, v in inp.items() if k not in ("means3D", "means2D", "opacities")}
    fold = None
    if form == "fold":
        fold = kw["fold"] = BackwardFold(stats=(torch.zeros(P, 1, device="cuda"), torch.zeros(P, 1, device="cuda"),
                                                torch.zeros(P, device="cuda")))
    if form == "camera_only":
        kw["camera_only"] = True
    if extras:
        kw.update(depth="z", alpha=True, n_touched=True)
    out = GaussianRasterizer(s)(inp["means3D"], inp["means2D"], inp["opacities"], **kw)
    return out, inp, cam_leaves, fold


def _check_outputs(out, extras, P):
    assert isinstance(out, tuple) and len(out) == 3 + (2 if extras else 0)
    assert out[0].shape == (3, H, W) and out[0].dtype == torch.float32 and out[0].requires_grad
    assert out[1].shape == (P,) and out[1].dtype == torch.int32 and not out[1].requires_grad
    assert out[2].shape == (1, H, W) and out[2].dtype == torch.float32 and out[2].requires_grad
    if extras:      # (the opacity plane, then - LAST - the visibility counts)
        assert out[3].shape == (1, H, W) and out[3].dtype == torch.float32 and out[3].requires_grad
        assert out[4].shape == (P,) and out[4].dtype == torch.int32 and not out[4].requires_grad


def _backward(out, extras):
    loss = out[0].sum() + out[2].sum()
    if extras:
        loss = loss + out[3].sum()
    loss.backward()
    torch.cuda.synchronize()


def _check_camera(cam_leaves, zero=False):
    for t in cam_leaves:
        assert t.grad is not None and t.grad.shape == t.shape and t.grad.dtype == t.dtype and t.grad.device == t.device
        assert bool(torch.isfinite(t.grad).all())
        if zero:
            assert not t.grad.any()


# every call form x every backward form x {no extras, all three}; P = 0 for the forms that have no rows to fold statistics over
CASES = [(inputs, form, extras, P) for P in (P_FULL, 0) for inputs in INPUTS
         for form in ("plain", "fold", "camera", "camera_only") if P or form != "fold" for extras in (False, True)]


@pytest.mark.parametrize("inputs,form,extras,P", CASES,
                         ids=[f"{i}-{f}-{'extras' if e else 'bare'}-P{p}" for i, f, e, p in CASES])
def test_autograd_contract(inputs, form, extras, P):
    """P = 0: empty gradients for the tensors the call passes on (an empty optional input counts as absent: None), zero camera
    gradients, no error."""
    out, inp, cam_leaves, fold = _run(inputs, form, extras, P)
    _check_outputs(out, extras, P)
    assert P == 0 or int((out[1] > 0).sum()) > 0
    _backward(out, extras)
    for k, t in inp.items():
        if form == "camera_only" or (P == 0 and k not in ("means3D", "means2D", "opacities")):
            assert t.grad is None, k
        else:
            assert t.grad is not None and t.grad.shape == t.shape and t.grad.dtype == torch.float32, k
    if cam_leaves is not None:
        _check_camera(cam_leaves, zero=P == 0)
    if fold is not None:
        assert fold.stats_taken and not fold.optimizer_taken and not fold.sh_rest_skipped
