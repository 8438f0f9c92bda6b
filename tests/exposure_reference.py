"""Pure-torch restatement of the per-view exposure for the exposure tests: the reference's expression (gaussian_renderer/
__init__.py:141-144) in the form it is written there, the alpha-mask multiply of train.py:109-111, and gradients by autograd.
Works in any float dtype (the tests evaluate it in float64).  Independent of the library: nothing here calls the HIP path."""
import torch


def apply_exposure_ref(img, E, mask=None):
    """img [3,H,W], E [3,4], mask [H,W] / [1,H,W] or None, all of one dtype -> [3,H,W]."""
    out = torch.matmul(img.permute(1, 2, 0), E[:3, :3]).permute(2, 0, 1) + E[:3, 3, None, None]
    if mask is not None:
        out = out * mask.reshape(1, *img.shape[-2:])
    return out


def exposure_grads_ref(img, E, g, mask=None, dtype=torch.float64):
    """(out, dL/dimg, dL/dE) for L = sum(out * g), evaluated in `dtype` on exactly the given values, by autograd."""
    img = img.detach().to(dtype).clone().requires_grad_(True)
    E = E.detach().to(dtype).clone().requires_grad_(True)
    mask = None if mask is None else mask.detach().to(dtype)
    out = apply_exposure_ref(img, E, mask)
    d_img, d_E = torch.autograd.grad(out, (img, E), grad_outputs=g.detach().to(dtype))
    return out.detach(), d_img, d_E


def forward_bound(img, E, terms=4):
    """terms * 2^-23 * (sum_k |E[k][j]| |I[k]| + |E[j][3]|) per element, float64: the a-priori bound of a float32 evaluation of
    `terms` terms per output (contracted or not)."""
    img, E = img.detach().double(), E.detach().double()
    mag = torch.einsum("kj,khw->jhw", E[:3, :3].abs(), img.abs()) + E[:3, 3].abs()[:, None, None]
    return terms * 2.0 ** -23 * mag


def image_grad_bound(g, E, terms=3):
    """terms * 2^-23 * sum_j |E[k][j]| |g[j]| per element of dL/dimg, float64."""
    g, E = g.detach().double(), E.detach().double()
    return terms * 2.0 ** -23 * torch.einsum("kj,jhw->khw", E[:3, :3].abs(), g.abs())


def exposure_grad_bound(img, g, mask=None):
    """(N + 3) * 2^-24 * sum_p |term| for each of the twelve sums ([3,4], float64): holds for every summation order."""
    img, g = img.detach().double(), g.detach().double()
    m = torch.ones(img.shape[-2:], dtype=torch.float64, device=img.device) if mask is None else \
        mask.detach().double().reshape(img.shape[-2:])
    N = img.shape[-2] * img.shape[-1]
    mag = torch.zeros(3, 4, dtype=torch.float64, device=img.device)
    mag[:, :3] = torch.einsum("khw,jhw->kj", img.abs(), (g * m).abs())
    mag[:, 3] = (g * m).abs().sum(dim=(1, 2))
    return (N + 3) * 2.0 ** -24 * mag
