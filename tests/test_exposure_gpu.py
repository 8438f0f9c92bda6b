"""Per-view exposure on the device (csrc/exposure.hip through scene_utils.exposure and render()) against the float64 restatement
of tests/exposure_reference.py.  Every bound here is a-priori (float32 rounding of the stated number of terms, or the tolerance
the Adam comparison is given), none is read off the code under test.

Shapes: 1x1; 3x5; 37x29 (odd plane size: planes 1 and 2 are not 16-byte aligned, and less than one workgroup of vector loads);
64x64 (exact multiples: the 16-byte path); 131x67 (several workgroups and a tail, 4-byte path).  Inputs: a non-symmetric exposure
(identity + N(0, 0.3)), three differently distributed channels and a random upstream gradient, so that a transposed index or a
dropped bias is an O(1) error."""
import pytest
import torch

from exposure_reference import apply_exposure_ref, exposure_grads_ref, forward_bound, image_grad_bound, exposure_grad_bound

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 5), (37, 29), (64, 64), (131, 67)]
MASKS = ["none", "random", "zero"]


def _inputs(H, W, mask_kind, seed=0):
    gen = torch.Generator().manual_seed(1000 * H + W + seed)
    E = torch.eye(3, 4) + 0.3 * torch.randn(3, 4, generator=gen)
    img = torch.stack([torch.rand(H, W, generator=gen),                              # uniform [0, 1)
                       2.0 + 0.5 * torch.randn(H, W, generator=gen),                 # offset normal
                       -torch.log(torch.rand(H, W, generator=gen).clamp_min(1e-6))])   # exponential
    g = torch.randn(3, H, W, generator=gen)
    if mask_kind == "none":
        mask = None
    elif mask_kind == "zero":
        mask = torch.zeros(1, H, W)
    else:
        mask = (torch.rand(1, H, W, generator=gen) > 0.3).float()
    return E, img, g, mask


_cases = {}


def _case(H, W, mask_kind):
    """Inputs and their float64 reference, computed once per case and shared (read-only) by the tests."""
    key = (H, W, mask_kind)
    if key not in _cases:
        E, img, g, mask = _inputs(H, W, mask_kind)
        out, d_img, d_E = exposure_grads_ref(img, E, g, mask)
        _cases[key] = dict(E=E, img=img, g=g, mask=mask, out=out, d_img=d_img, d_E=d_E, fb=forward_bound(img, E),
                           ib=image_grad_bound(g, E), eb=exposure_grad_bound(img, g, mask))
    return _cases[key]


def _run(c, image_grad=True, exposure_grad=True):
    from scene_utils import apply_exposure
    img = c["img"].cuda().requires_grad_(image_grad)
    E = c["E"].cuda().requires_grad_(exposure_grad)
    mask = None if c["mask"] is None else c["mask"].cuda()
    out = apply_exposure(img, E, mask)
    out.backward(c["g"].cuda())
    return out.detach().cpu(), (None if img.grad is None else img.grad.cpu()), (None if E.grad is None else E.grad.cpu())


def _within(name, got, ref, bound):
    err = (got.double() - ref).abs()
    worst = (err - bound).max().item()
    print(f"{name}: max err {err.max().item():.3e}, max bound {bound.max().item():.3e}, max (err - bound) {worst:.3e}")
    assert bool((err <= bound).all()), (name, err.max().item(), worst)


@pytest.mark.parametrize("mask_kind", MASKS)
@pytest.mark.parametrize("H,W", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_forward_and_backward_against_float64(H, W, mask_kind):
    c = _case(H, W, mask_kind)
    out, d_img, d_E = _run(c)
    assert out.dtype == torch.float32 and tuple(out.shape) == (3, H, W)
    assert tuple(d_img.shape) == (3, H, W) and tuple(d_E.shape) == (3, 4)
    _within("forward", out, c["out"], c["fb"])
    _within("dL/dimage", d_img, c["d_img"], c["ib"])
    _within("dL/dexposure", d_E, c["d_E"], c["eb"])
    if mask_kind == "zero":
        assert out.abs().max() == 0 and d_img.abs().max() == 0 and d_E.abs().max() == 0


@pytest.mark.parametrize("mask_kind", ["none", "random"])
@pytest.mark.parametrize("H,W", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_missing_gradients_and_reproducibility(H, W, mask_kind):
    c = _case(H, W, mask_kind)
    out, d_img, d_E = _run(c)
    # no exposure gradient asked for (a plain tensor, a foreign model's constant): no reduction, the image gradient alone
    out1, d_img1, d_E1 = _run(c, exposure_grad=False)
    assert d_E1 is None and torch.equal(out1, out)
    _within("dL/dimage alone", d_img1, c["d_img"], c["ib"])
    # no image gradient asked for (NULL dL/dimage): the twelve sums alone
    out2, d_img2, d_E2 = _run(c, image_grad=False)
    assert d_img2 is None and torch.equal(out2, out)
    _within("dL/dexposure alone", d_E2, c["d_E"], c["eb"])
    # the same bits every run
    out3, d_img3, d_E3 = _run(c)
    assert torch.equal(out3, out) and torch.equal(d_img3, d_img) and torch.equal(d_E3, d_E)


def test_mask_shapes_and_non_contiguous_upstream():
    from scene_utils import apply_exposure
    c = _case(37, 29, "random")
    img, E, m = c["img"].cuda(), c["E"].cuda(), c["mask"].cuda()
    a = apply_exposure(img, E, m)
    b = apply_exposure(img, E, m[0])
    assert torch.equal(a, b)
    # a transposed (non-contiguous) upstream gradient and a non-contiguous image are taken as their values
    img_t = c["img"].permute(0, 2, 1).contiguous().cuda().permute(0, 2, 1).requires_grad_(True)
    assert not img_t.is_contiguous()
    g_t = c["g"].permute(0, 2, 1).contiguous().cuda().permute(0, 2, 1)
    Eg = E.clone().requires_grad_(True)
    out = apply_exposure(img_t, Eg, m)
    out.backward(g_t)
    _within("forward", out.detach().cpu(), c["out"], c["fb"])
    _within("dL/dimage", img_t.grad.cpu(), c["d_img"], c["ib"])
    _within("dL/dexposure", Eg.grad.cpu(), c["d_E"], c["eb"])


# ------------------------------------------------------------------------------------------------------------------------------
# the optimizer step folded into the backward
# ------------------------------------------------------------------------------------------------------------------------------
class _Cam:
    def __init__(self, name):
        self.image_name = name


def _exposure_model(V):
    from scene_utils import GaussianModel, make_gaussians
    m = GaussianModel.from_raw(make_gaussians(8, 0, seed=1).to("cuda"))
    m.setup_exposures([f"v{i}" for i in range(V)])
    return m


def test_folded_adam_equals_torch_adam_step_by_step():
    """V = 5, eight steps over the views [2,0,2,2,4,0,1,2] (view 3 never seen), then two more after disarming.  After every step
    the folded run equals the unfolded run - the same kernels' gradient through `_exposure.grad` and torch.optim.Adam on the
    device - within S (lr 2^-20 + 2^-23 max|E|) after S steps."""
    from scene_utils.exposure import render_exposure
    V, H, W, lr = 5, 37, 29, 1e-3
    seq = [2, 0, 2, 2, 4, 0, 1, 2]
    tail = [3, 0]
    folded, plain = _exposure_model(V), _exposure_model(V)
    assert folded.exposure_optimizer.param_groups[0]["lr"] == lr
    folded.fold_exposure_adam()
    assert folded._exposure_adam is not None
    eye = torch.eye(3, 4, device="cuda")
    at_last_visit = {}

    def step(model, view, s):
        _, img, g, mask = _inputs(H, W, "random" if s % 2 else "none", seed=77 + s)
        img = img.cuda().requires_grad_(True)
        out = render_exposure(img, model, _Cam(f"v{view}"), True, None if mask is None else mask.cuda())
        out.backward(g.cuda())
        if model._exposure_adam is None:
            assert model._exposure.grad is not None
            model.exposure_optimizer.step()
            model.exposure_optimizer.zero_grad(set_to_none=True)
        else:
            assert model._exposure.grad is None
        return img.grad

    def compare(S):
        a, b = folded._exposure.detach(), plain._exposure.detach()
        tol = S * (lr * 2.0 ** -20 + 2.0 ** -23 * b.abs().max().item())
        diff = (a.double() - b.double()).abs().max().item()
        print(f"after {S} steps: max |folded - torch| {diff:.3e}, tolerance {tol:.3e}")
        assert diff <= tol, (S, diff, tol)

    for s, view in enumerate(seq):
        gi_f = step(folded, view, s)
        gi_p = step(plain, view, s)
        assert gi_f is not None and gi_p is not None
        compare(s + 1)
        at_last_visit[view] = folded._exposure.detach()[view].clone()
        assert torch.equal(folded._exposure.detach()[3], eye)       # never seen: zero gradient, zero moments, not a bit moves
    moved = (folded._exposure.detach() - eye).abs().amax(dim=(1, 2))
    assert bool((moved[[0, 1, 2, 4]] > 0.5 * lr).all()), moved      # every seen row moved by about lr per step
    for view in (0, 4):                                             # rows seen earlier keep moving on their decaying moments
        assert not torch.equal(folded._exposure.detach()[view], at_last_visit[view])
    # the device state counted the steps; disarming hands moments and count to the torch optimizer
    folded.fold_exposure_adam(on=False)
    assert folded._exposure_adam is None
    st = folded.exposure_optimizer.state[folded._exposure]
    assert float(st["step"]) == len(seq) and tuple(st["exp_avg"].shape) == (V, 3, 4)
    ref_st = plain.exposure_optimizer.state[plain._exposure]
    assert (st["exp_avg"] - ref_st["exp_avg"]).abs().max().item() <= 1e-5 * ref_st["exp_avg"].abs().max().item()
    assert (st["exp_avg_sq"] - ref_st["exp_avg_sq"]).abs().max().item() <= 1e-5 * ref_st["exp_avg_sq"].abs().max().item()
    for i, view in enumerate(tail):
        step(folded, view, len(seq) + i)
        step(plain, view, len(seq) + i)
        compare(len(seq) + i + 1)
    # and back: arming again takes the moments over from the optimizer
    folded.fold_exposure_adam()
    step(folded, 1, 20)
    step(plain, 1, 20)
    compare(len(seq) + len(tail) + 1)
    folded.fold_exposure_adam(on=False)
    assert float(folded.exposure_optimizer.state[folded._exposure]["step"]) == len(seq) + len(tail) + 1


# ------------------------------------------------------------------------------------------------------------------------------
# render()
# ------------------------------------------------------------------------------------------------------------------------------
def test_render_with_exposure_and_alpha_mask():
    from gaussian_renderer import render, PipelineParams
    from helpers import rel_l2
    from scene_utils import GaussianModel, make_gaussians, fibonacci_cameras
    W, H, P = 48, 40, 500
    model = GaussianModel.from_raw(make_gaussians(P, 1, seed=4, scale_factor=0.6).to("cuda"))
    cam = fibonacci_cameras(3, W, H, seed=2, device="cuda")[1]
    cam.image_name = "view_b"
    gen = torch.Generator().manual_seed(11)
    E = torch.eye(3, 4) + 0.3 * torch.randn(3, 4, generator=gen)
    mask = (torch.rand(1, H, W, generator=gen) > 0.3).float()
    g = torch.randn(3, H, W, generator=gen)
    model.setup_exposures(["view_a", "view_b", "view_c"], pretrained={"view_b": E})
    pipe, bg = PipelineParams(), torch.tensor([0.1, 0.2, 0.3], device="cuda")
    kw = dict(forward_mode="exact")

    def grads_of(image, upstream):
        for p in model.parameters() + [model._exposure]:
            p.grad = None
        image.backward(upstream)
        return model._xyz.grad.detach().clone()

    pkg = render(cam, model, pipe, bg, **kw)
    plain = pkg["render"].detach().clone()
    # neither option: exactly the plain render
    again = render(cam, model, pipe, bg, use_trained_exp=False, alpha_mask=None, **kw)["render"]
    assert torch.equal(again.detach(), plain)
    # the reference's dL/dimage fed into the plain render's backward
    ref_out, ref_dimg, ref_dE = exposure_grads_ref(plain.cpu(), E, g, mask)
    want = grads_of(pkg["render"], ref_dimg.float().cuda())
    assert want.abs().max() > 0
    # exposure + mask inside render()
    pkg = render(cam, model, pipe, bg, use_trained_exp=True, alpha_mask=mask.cuda(), **kw)
    assert set(pkg.keys()) == {"render", "viewspace_points", "visibility_filter", "radii", "depth"}
    _within("render forward", pkg["render"].detach().cpu(), ref_out, forward_bound(plain.cpu(), E))
    with_exposure = pkg["render"].detach().clone()
    got = grads_of(pkg["render"], g.cuda())
    r = rel_l2(got, want)
    print(f"means3D gradient through the exposure: rel_l2 {r:.3e}")
    assert r <= 1e-6, r
    dE = model._exposure.grad.detach().cpu()
    assert dE[0].abs().max() == 0 and dE[2].abs().max() == 0
    _within("render dL/dexposure", dE[1], ref_dE, exposure_grad_bound(plain.cpu(), g, mask))
    # the mask alone: the identity exposure in the same launch ([H,W] form of the mask)
    masked = render(cam, model, pipe, bg, alpha_mask=mask[0].cuda(), **kw)["render"]
    assert torch.equal(masked.detach(), plain * mask.cuda())
    # armed: the backward takes the step, no gradient reaches the parameter
    for p in model.parameters() + [model._exposure]:
        p.grad = None
    before = model._exposure.detach().clone()
    model.fold_exposure_adam()
    pkg = render(cam, model, pipe, bg, use_trained_exp=True, alpha_mask=mask.cuda(), **kw)
    assert torch.equal(pkg["render"].detach(), with_exposure)            # the same forward, armed or not
    pkg["render"].backward(g.cuda())
    after = model._exposure.detach()
    assert model._exposure.grad is None and model._xyz.grad is not None
    assert torch.equal(after[0], before[0]) and torch.equal(after[2], before[2])
    step = (after[1] - before[1]).abs()
    nonzero = ref_dE.abs() > 0
    assert bool(((step.cpu() - 1e-3).abs()[nonzero] < 1e-5).all()), step       # Adam's first step: lr * sign(gradient)
    model.fold_exposure_adam(on=False)
