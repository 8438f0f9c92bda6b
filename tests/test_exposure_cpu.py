"""Host side of the per-view exposure (scene_utils.exposure): the model's API, argument validation before any launch, the
pure-torch reference of the GPU tests against a hand-written per-pixel loop, and render()'s signature.  No GPU needed."""
import inspect

import pytest
import torch

from exposure_reference import apply_exposure_ref, exposure_grads_ref


def _model(P=6):
    from scene_utils import GaussianModel, make_gaussians
    return GaussianModel.from_raw(make_gaussians(P, 1, seed=2))


def test_model_starts_without_exposures():
    m = _model()
    assert m._exposure is None and m.exposure_mapping == {} and m.exposure_optimizer is None and m._exposure_adam is None
    assert torch.equal(m.get_exposure_from_name("anything"), torch.eye(3, 4))


def test_setup_exposures_mapping_shapes_identity_and_optimizer():
    m = _model()
    names = ["a.png", "b.png", "c.png", "d.png"]
    opt = m.setup_exposures(names, lr=2e-3)
    assert isinstance(m._exposure, torch.nn.Parameter) and m._exposure.requires_grad
    assert tuple(m._exposure.shape) == (4, 3, 4) and m._exposure.dtype == torch.float32
    assert m._exposure.device == m._xyz.device and m._exposure.is_contiguous()
    assert m.exposure_mapping == {n: i for i, n in enumerate(names)}
    for n in names:
        e = m.get_exposure_from_name(n)
        assert tuple(e.shape) == (3, 4) and torch.equal(e.detach(), torch.eye(3, 4))
    assert opt is m.exposure_optimizer and isinstance(opt, torch.optim.Adam)
    g = opt.param_groups[0]
    assert len(opt.param_groups) == 1 and len(g["params"]) == 1 and g["params"][0] is m._exposure
    assert g["lr"] == 2e-3 and tuple(g["betas"]) == (0.9, 0.999) and g["eps"] == 1e-8 and g["weight_decay"] == 0
    assert m._exposure_adam is None
    # the default learning rate is torch.optim.Adam's own (reference scene/gaussian_model.py:178 passes none)
    assert _model().setup_exposures(["x"]).param_groups[0]["lr"] == 1e-3


def test_setup_exposures_pretrained_and_bad_input():
    m = _model()
    E = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    m.setup_exposures(["a", "b", "c"], pretrained={"b": E, "not_in_this_run": E + 1, "c": (E * 2).tolist()})
    assert torch.equal(m.get_exposure_from_name("a").detach(), torch.eye(3, 4))
    assert torch.equal(m.get_exposure_from_name("b").detach(), E)
    assert torch.equal(m.get_exposure_from_name("c").detach(), E * 2)
    with pytest.raises(ValueError, match="duplicate image name 'a'"):
        _model().setup_exposures(["a", "b", "a"])
    with pytest.raises(ValueError, match="shape"):
        _model().setup_exposures(["a"], pretrained={"a": torch.eye(3)})
    with pytest.raises(ValueError, match="no image names"):
        _model().setup_exposures([])


def test_row_gradient_reaches_the_parameter_through_the_getter():
    """The reference's flow: the gradient of one view's row arrives in `_exposure.grad`, zero on the other rows."""
    m = _model()
    m.setup_exposures(["a", "b", "c"])
    img = torch.rand(3, 2, 3)
    apply_exposure_ref(img, m.get_exposure_from_name("b")).sum().backward()
    g = m._exposure.grad
    assert tuple(g.shape) == (3, 3, 4) and g[0].abs().sum() == 0 and g[2].abs().sum() == 0 and g[1].abs().sum() > 0


def test_fold_needs_setup_and_a_device():
    from diff_gaussian_rasterization import _C
    m = _model()
    with pytest.raises(ValueError, match="setup_exposures"):
        m.fold_exposure_adam()
    m.setup_exposures(["a"])
    with pytest.raises(_C.GsrError, match="no CPU path"):
        m.fold_exposure_adam()
    m.fold_exposure_adam(on=False)          # disarming what is not armed: nothing happens
    assert m._exposure_adam is None


def test_validation_errors_come_before_the_device_check():
    from scene_utils import apply_exposure
    img, E = torch.rand(3, 4, 5), torch.eye(3, 4)
    bad = [
        (dict(image=torch.rand(4, 5), exposure=E), "image"),
        (dict(image=torch.rand(1, 4, 5), exposure=E), "image"),
        (dict(image=torch.rand(3, 4, 5, dtype=torch.float64), exposure=E), "image"),
        (dict(image=img, exposure=torch.eye(3)), "exposure"),
        (dict(image=img, exposure=torch.eye(4)), "exposure"),
        (dict(image=img, exposure=E.double()), "exposure"),
        (dict(image=img, exposure=E, mask=torch.ones(5, 4)), "mask"),
        (dict(image=img, exposure=E, mask=torch.ones(3, 4, 5)), "mask"),
        (dict(image=img, exposure=E, mask=torch.ones(4, 5) > 0), "mask"),
    ]
    for kw, name in bad:
        with pytest.raises(ValueError, match=f"^{name}: expected"):
            apply_exposure(**kw)


def test_cpu_tensors_raise_gsr_error():
    from diff_gaussian_rasterization import _C
    from scene_utils import apply_exposure
    with pytest.raises(_C.GsrError, match="no CPU path"):
        apply_exposure(torch.rand(3, 4, 5), torch.eye(3, 4))
    with pytest.raises(_C.GsrError, match="no CPU path"):
        apply_exposure(torch.rand(3, 4, 5), torch.eye(3, 4), torch.ones(1, 4, 5))


def test_reference_module_against_a_per_pixel_loop():
    """out[j,p] = m[p] (sum_k E[k][j] I[k,p] + E[j][3]) and its gradients, spelled out index by index on a 2x3 image with a
    non-symmetric E: pins the reference module's (= the reference's) index convention."""
    H, W = 2, 3
    gen = torch.Generator().manual_seed(5)
    E = torch.tensor([[1.1, 0.2, -0.3, 0.05], [0.4, 0.9, 0.15, -0.1], [-0.25, 0.35, 1.2, 0.2]], dtype=torch.float64)
    I = torch.rand(3, H, W, generator=gen, dtype=torch.float64)
    g = torch.randn(3, H, W, generator=gen, dtype=torch.float64)
    m = torch.tensor([[1.0, 0.0, 1.0], [0.5, 1.0, 0.0]], dtype=torch.float64)
    for mask in (None, m):
        out = torch.zeros(3, H, W, dtype=torch.float64)
        dI = torch.zeros(3, H, W, dtype=torch.float64)
        dE = torch.zeros(3, 4, dtype=torch.float64)
        for y in range(H):
            for x in range(W):
                w = 1.0 if mask is None else float(mask[y, x])
                for j in range(3):
                    out[j, y, x] = w * (sum(float(E[k, j]) * float(I[k, y, x]) for k in range(3)) + float(E[j, 3]))
                    dE[j, 3] += w * float(g[j, y, x])
                    for k in range(3):
                        dE[k, j] += w * float(I[k, y, x]) * float(g[j, y, x])
                for k in range(3):
                    dI[k, y, x] = w * sum(float(E[k, j]) * float(g[j, y, x]) for j in range(3))
        r_out, r_dI, r_dE = exposure_grads_ref(I, E, g, mask)
        assert (r_out - out).abs().max() < 1e-14 and (r_dI - dI).abs().max() < 1e-14 and (r_dE - dE).abs().max() < 1e-14
        assert torch.equal(apply_exposure_ref(I, E, None if mask is None else mask[None]), r_out)
    # the asymmetry is real: the transposed matrix, or the bias read from the last ROW's columns, is an O(1) change
    wrong = torch.matmul(I.permute(1, 2, 0), E[:3, :3].T).permute(2, 0, 1) + E[:3, 3, None, None]
    assert (wrong - apply_exposure_ref(I, E)).abs().max() > 0.05


def test_render_signature_starts_with_the_references_parameters():
    from gaussian_renderer import render
    sig = inspect.signature(render).parameters
    names = list(sig)
    # reference gaussian_renderer/__init__.py:18
    assert names[:8] == ["viewpoint_camera", "pc", "pipe", "bg_color", "scaling_modifier", "separate_sh", "override_color",
                         "use_trained_exp"]
    assert sig["scaling_modifier"].default == 1.0 and sig["separate_sh"].default is False
    assert sig["override_color"].default is None and sig["use_trained_exp"].default is False
    assert sig["alpha_mask"].default is None and sig["alpha_mask"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    assert sig[names[-1]].kind is inspect.Parameter.VAR_KEYWORD


def test_abi_additions_are_bound():
    import ctypes as C
    from diff_gaussian_rasterization import _C
    for n in ("gsr_exposure_blocks", "gsr_exposure_forward", "gsr_exposure_backward"):
        assert n in _C.EXPORTS
    assert C.sizeof(_C.gsr_exposure_adam) == 4 * _C.EXPOSURE_ADAM_HEADER_FLOATS == 16
    assert _C.lib().gsr_exposure_blocks() >= 1
    # bad arguments are refused by the entry points before any launch
    assert _C.lib().gsr_exposure_forward(0, None, None, None, None, None) == -1
    assert _C.lib().gsr_exposure_backward(16, None, None, None, None, None, None, None, None, 0, 0, None, 0, 0, 0, 0, None) == -1
