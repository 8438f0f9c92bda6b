"""Per-view exposure: the learned affine colour correction of reference gaussian_renderer/__init__.py:141-144 and the alpha-mask
multiply of train.py:109-111, as HIP kernels (csrc/exposure.hip), and the exposure parameters of the model with their optimizer
(reference scene/gaussian_model.py:178, stepped at train.py:171-172).

    out[j, p] = mask[p] * (sum_k E[k][j] * image[k, p] + E[j][3])

The 3x3 part of `E` multiplies the pixel from the right (it acts transposed), the bias of channel j is `E[j][3]`: the reference's
convention.  Two optimizer flows over `GaussianModel._exposure` [V,3,4]:
  - the reference's: `setup_exposures()` builds `exposure_optimizer = torch.optim.Adam([_exposure])`; the backward writes the
    selected row's gradient into `_exposure.grad`, the caller steps the optimizer;
  - folded: `fold_exposure_adam()` arms an Adam state in device memory; the backward's finalize launch then takes the same dense
    Adam step itself and `_exposure.grad` stays None.
There is no CPU path.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .model import GaussianModel

_scratch = {}


def _partials(device):
    """Scratch of the backward's per-workgroup sums, one per device (stream-ordered reuse: written and read by consecutive
    launches of one backward)."""
    from diff_gaussian_rasterization import _C
    t = _scratch.get(device)
    if t is None:
        t = _scratch[device] = torch.empty(12 * _C.lib().gsr_exposure_blocks(), dtype=torch.float32, device=device)
    return t


def _check(image, exposure, mask):
    """Shapes and dtypes first (ValueError), then the device (GsrError): nothing is launched for a bad call."""
    from diff_gaussian_rasterization import _C
    if not torch.is_tensor(image) or image.dim() != 3 or image.shape[0] != 3 or image.shape[1] < 1 or image.shape[2] < 1:
        raise ValueError(f"image: expected a [3,H,W] tensor, got "
                         f"{tuple(image.shape) if torch.is_tensor(image) else type(image).__name__}")
    if image.dtype != torch.float32:
        raise ValueError(f"image: expected float32, got {image.dtype}")
    if not torch.is_tensor(exposure) or tuple(exposure.shape) != (3, 4):
        raise ValueError(f"exposure: expected a [3,4] tensor, got "
                         f"{tuple(exposure.shape) if torch.is_tensor(exposure) else type(exposure).__name__}")
    if exposure.dtype != torch.float32:
        raise ValueError(f"exposure: expected float32, got {exposure.dtype}")
    H, W = int(image.shape[1]), int(image.shape[2])
    if mask is not None:
        if not torch.is_tensor(mask) or tuple(mask.shape) not in ((H, W), (1, H, W)):
            raise ValueError(f"mask: expected a [{H},{W}] or [1,{H},{W}] tensor, got "
                             f"{tuple(mask.shape) if torch.is_tensor(mask) else type(mask).__name__}")
        if mask.dtype != torch.float32:
            raise ValueError(f"mask: expected float32, got {mask.dtype}")
    if not image.is_cuda:
        raise _C.GsrError("apply_exposure runs in HIP kernels (no CPU path): image must be a device tensor")
    if exposure.device != image.device or (mask is not None and mask.device != image.device):
        raise ValueError(f"exposure / mask: expected tensors on {image.device}")


class _Exposure(torch.autograd.Function):
    """(image, exposure[, mask]) -> image': ONE gsr_exposure_forward launch; the backward is gsr_exposure_backward (a streaming
    launch + a one-workgroup finalize).  `fold` = (model, row) while the model's device Adam state is armed: the finalize launch
    then steps the whole `_exposure` tensor and the exposure gets no gradient."""

    @staticmethod
    def forward(ctx, image, exposure, mask, fold):
        from diff_gaussian_rasterization import _C
        image = image.contiguous()
        exposure = exposure.contiguous()
        out = torch.empty_like(image)
        n = int(image.shape[1]) * int(image.shape[2])
        with _C.on_device(image.device):
            _C.check(_C.lib().gsr_exposure_forward(n, _C.ptr(image), _C.ptr(exposure), _C.ptr(mask), _C.ptr(out), _C._stream()))
        ctx.save_for_backward(image, exposure, mask)
        ctx.fold = fold
        return out

    @staticmethod
    def backward(ctx, g):
        from diff_gaussian_rasterization import _C
        image, exposure, mask = ctx.saved_tensors
        dev = image.device
        g = g.to(dtype=torch.float32).contiguous()
        n = int(image.shape[1]) * int(image.shape[2])
        d_image = torch.empty_like(image) if ctx.needs_input_grad[0] else None
        fold = ctx.fold
        d_exp = exposures = adam = None
        views = row = 0
        lr = b1 = b2 = eps = 0.0
        if fold is not None:
            model, row = fold
            st = model._exposure_adam
            if st is None:
                raise _C.GsrError("the exposure Adam state was disarmed between this graph's forward and its backward")
            adam, (lr, b1, b2, eps) = st["state"], st["hyper"]
            exposures = model._exposure.data
            views = int(exposures.shape[0])
        elif ctx.needs_input_grad[1]:
            d_exp = torch.empty(3, 4, dtype=torch.float32, device=dev)
        if d_image is None and d_exp is None and adam is None:
            return None, None, None, None
        partials = _partials(dev) if (d_exp is not None or adam is not None) else None
        with _C.on_device(dev):
            _C.check(_C.lib().gsr_exposure_backward(n, _C.ptr(image), _C.ptr(exposure), _C.ptr(mask), _C.ptr(g), _C.ptr(d_image),
                                                    _C.ptr(partials), _C.ptr(d_exp), _C.ptr(exposures), views, int(row),
                                                    _C.ptr(adam), lr, b1, b2, eps, _C._stream()))
        return d_image, d_exp, None, None


def _flat_mask(mask):
    return None if mask is None else mask.detach().contiguous()


def apply_exposure(image, exposure, mask=None):
    """image [3,H,W] float32 on the HIP device, exposure [3,4] (any device tensor: a row of `GaussianModel._exposure`, or what a
    foreign model's `get_exposure_from_name` returns), mask [H,W] / [1,H,W] or None -> mask * (exposure applied to image), one
    launch.  Gradients go to `image` and, if it requires grad, to `exposure`; the mask is not differentiated."""
    _check(image, exposure, mask)
    return _Exposure.apply(image, exposure, _flat_mask(mask), None)


_identity = {}


def render_exposure(image, pc, camera, use_trained_exp, alpha_mask):
    """What render() does behind the rasterizer when `use_trained_exp` or an `alpha_mask` is given: the model's exposure of this
    camera (the identity without `use_trained_exp`) and the mask in one launch.  With the model's device Adam state armed
    (`fold_exposure_adam`) the row index and the state travel down and the backward takes the optimizer step."""
    fold = None
    if use_trained_exp:
        if getattr(pc, "_exposure_adam", None) is not None:
            row = pc.exposure_mapping[camera.image_name]
            exposure = pc._exposure.detach()[row]
            fold = (pc, row)
        else:
            exposure = pc.get_exposure_from_name(camera.image_name)
    else:
        exposure = _identity.get(image.device)
        if exposure is None:
            exposure = _identity[image.device] = torch.eye(3, 4, dtype=torch.float32, device=image.device)
    _check(image, exposure, alpha_mask)
    return _Exposure.apply(image, exposure, _flat_mask(alpha_mask), fold)


# ---------------------------------------------------------------------------------------------------------------------
# the model's side
# ---------------------------------------------------------------------------------------------------------------------
def setup_exposures(self, image_names, lr=1e-3, pretrained=None):
    """One [3,4] exposure per training view, `eye(3,4)` each (or `pretrained[name]`), as ONE nn.Parameter `_exposure` [V,3,4] on
    the model's device; `exposure_mapping` name -> row; `exposure_optimizer = torch.optim.Adam([_exposure], lr=lr)` (reference
    scene/gaussian_model.py:178).  Duplicate names raise ValueError."""
    names = list(image_names)
    mapping = {}
    for i, name in enumerate(names):
        if name in mapping:
            raise ValueError(f"setup_exposures: duplicate image name {name!r}")
        mapping[name] = i
    if not names:
        raise ValueError("setup_exposures: no image names")
    dev = self._xyz.device if self._xyz is not None else torch.device("cpu")
    rows = torch.eye(3, 4, dtype=torch.float32).repeat(len(names), 1, 1)
    for name, value in (pretrained or {}).items():
        if name not in mapping:
            continue                      # (an exposure file may cover more views than this run trains on)
        value = torch.as_tensor(value, dtype=torch.float32)
        if tuple(value.shape) != (3, 4):
            raise ValueError(f"setup_exposures: pretrained[{name!r}] has shape {tuple(value.shape)}, expected (3, 4)")
        rows[mapping[name]] = value
    self._exposure = nn.Parameter(rows.to(dev).contiguous().requires_grad_(True))
    self.exposure_mapping = mapping
    self.exposure_optimizer = torch.optim.Adam([self._exposure], lr=float(lr))
    self._exposure_adam = None
    return self.exposure_optimizer


def _adam_hyper(opt, lr):
    g = opt.param_groups[0]
    if g.get("weight_decay", 0) or g.get("amsgrad", False) or g.get("maximize", False):
        raise ValueError("fold_exposure_adam: the device step is plain Adam (no weight decay, amsgrad or maximize)")
    return (float(g["lr"] if lr is None else lr), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]))


def fold_exposure_adam(self, on=True, lr=None):
    """on=True: arms the Adam state in device memory (moments and step count taken over from `exposure_optimizer`, so the flows
    can be switched mid-run); while armed `render(use_trained_exp=True)` hands the row and the state to the backward, whose
    finalize launch takes the step: `_exposure.grad` stays None and `exposure_optimizer.step()` is not to be called.  `lr`: the
    step's learning rate (default: the optimizer's).  on=False: copies the moments and the step count back into
    `exposure_optimizer.state` (one read-back: the count) and disarms."""
    from diff_gaussian_rasterization import _C
    if getattr(self, "_exposure", None) is None or getattr(self, "exposure_optimizer", None) is None:
        raise ValueError("fold_exposure_adam: call setup_exposures() first")
    p = self._exposure
    opt = self.exposure_optimizer
    V = int(p.shape[0])
    H = _C.EXPOSURE_ADAM_HEADER_FLOATS
    if on:
        if not p.is_cuda:
            raise _C.GsrError("fold_exposure_adam keeps the optimizer state on the HIP device (no CPU path)")
        hyper = _adam_hyper(opt, lr)
        if getattr(self, "_exposure_adam", None) is not None:
            self._exposure_adam["hyper"] = hyper
            return
        state = torch.zeros(H + 24 * V, dtype=torch.float32, device=p.device)
        st = opt.state.get(p, None)
        if st and "exp_avg" in st:
            state[H:H + 12 * V].copy_(st["exp_avg"].reshape(-1))
            state[H + 12 * V:].copy_(st["exp_avg_sq"].reshape(-1))
            state[:2].view(torch.int64).fill_(int(float(st["step"])))
        self._exposure_adam = {"state": state, "hyper": hyper}
        p.grad = None
        return
    armed = getattr(self, "_exposure_adam", None)
    if armed is None:
        return
    state = armed["state"]
    opt.param_groups[0]["lr"] = armed["hyper"][0]
    step = int(state[:2].view(torch.int64).item())
    if step > 0 or p in opt.state:
        opt.state[p] = {"step": torch.tensor(float(step)),
                        "exp_avg": state[H:H + 12 * V].clone().view_as(p),
                        "exp_avg_sq": state[H + 12 * V:].clone().view_as(p)}
    self._exposure_adam = None


GaussianModel.setup_exposures = setup_exposures
GaussianModel.fold_exposure_adam = fold_exposure_adam
