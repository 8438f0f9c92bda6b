"""CPU tests of the depth / opacity options (GaussianRasterizer(depth=..., alpha=...), render(depth=..., alpha=...)): the render
package's keys, and argument validation that happens before any device work (no GPU needed: a bad value never gets there)."""
import pytest
import torch

from gaussian_renderer import RenderPackage, render, PipelineParams


class _NoDevice:
    """A model / camera whose every attribute access fails: render() must refuse a bad option before touching either."""

    def __getattr__(self, name):
        raise AssertionError(f"device work started: {name} was read")


def test_package_keys_without_and_with_alpha():
    base = {"render": 1, "viewspace_points": 2, "radii": torch.tensor([0, 3]), "depth": 4}
    assert set(RenderPackage(base).keys()) == {"render", "viewspace_points", "visibility_filter", "radii", "depth"}
    p = RenderPackage(dict(base, alpha=5))
    assert set(p.keys()) == {"render", "viewspace_points", "visibility_filter", "radii", "depth", "alpha"} and p["alpha"] == 5


@pytest.mark.parametrize("depth", ["Z", "inv", "", None, 1])
def test_unknown_depth_kind_raises_before_device_work(depth):
    with pytest.raises(ValueError, match="depth="):
        render(_NoDevice(), _NoDevice(), PipelineParams(), torch.zeros(3), depth=depth)


def test_alpha_must_be_a_bool():
    with pytest.raises(TypeError, match="alpha="):
        render(_NoDevice(), _NoDevice(), PipelineParams(), torch.zeros(3), alpha="yes")


@pytest.mark.parametrize("kw,exc", [(dict(depth="near"), ValueError), (dict(alpha=1), TypeError)])
def test_rasterizer_validates_before_device_work(kw, exc):
    """GaussianRasterizer.forward refuses the option with CPU tensors in hand - before it would refuse them for being on the CPU."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    eye = torch.eye(4)
    s = GaussianRasterizationSettings(image_height=8, image_width=8, tanfovx=1.0, tanfovy=1.0, bg=torch.zeros(3),
                                      scale_modifier=1.0, viewmatrix=eye, projmatrix=eye, sh_degree=0, campos=torch.zeros(3),
                                      prefiltered=False, debug=False, antialiasing=False)
    P = 4
    with pytest.raises(exc):
        GaussianRasterizer(s)(means3D=torch.zeros(P, 3), means2D=torch.zeros(P, 3), opacities=torch.ones(P, 1),
                              colors_precomp=torch.zeros(P, 3), scales=torch.ones(P, 3), rotations=torch.ones(P, 4), **kw)


def test_depth_kinds_of_the_abi():
    from diff_gaussian_rasterization import _C
    assert _C.DEPTH_KINDS == {"inverse": 0, "z": 1}
    ex = _C.gsr_render_extras()
    assert ex.depth_kind == 0 and ex.out_alpha is None and ex.dL_dalpha is None


def test_refine_pose_rejects_a_bad_depth_weight():
    from scene_utils import refine_pose
    with pytest.raises(ValueError, match="depth_weight"):
        refine_pose(_NoDevice(), _NoDevice(), torch.zeros(3, 4, 4), gt_depth=torch.ones(1, 4, 4), depth_weight=1.5)
