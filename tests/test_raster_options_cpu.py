"""CPU tests of the rasterizer's per-call options record (diff_gaussian_rasterization.RasterOptions / check_options): every public
surface - render(), GaussianRasterizer.forward(), rasterize_gaussians() - refuses the same bad values with the same exception
before any device work; and the ctypes signatures of diff_gaussian_rasterization._C against the declarations of include/gsr.h."""
import ctypes as C
import os
import re

import pytest
import torch

from test_depth_alpha_cpu import _NoDevice

INVALID = [("depth", "Z", ValueError), ("depth", "", ValueError), ("depth", None, ValueError), ("depth", 1, ValueError),
           ("alpha", 1, TypeError),
           ("n_touched", "yes", TypeError),
           ("touched_T_min", True, TypeError), ("touched_T_min", "0.5", TypeError), ("touched_T_min", 1.0, ValueError),
           ("touched_T_min", -0.1, ValueError), ("touched_T_min", float("nan"), ValueError),
           ("camera_only", 1, TypeError)]
VALID = [dict(), dict(depth="z", alpha=True), dict(n_touched=True, touched_T_min=0), dict(touched_T_min=0.999),
         dict(depth="inverse", alpha=False, n_touched=False, touched_T_min=0.5, camera_only=False)]
P = 4


def _settings():
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    eye = torch.eye(4)
    return GaussianRasterizationSettings(image_height=8, image_width=8, tanfovx=1.0, tanfovy=1.0, bg=torch.zeros(3),
                                         scale_modifier=1.0, viewmatrix=eye, projmatrix=eye, sh_degree=0, campos=torch.zeros(3),
                                         prefiltered=False, debug=False, antialiasing=False)


def _call_render(**kw):
    from gaussian_renderer import render, PipelineParams
    return render(_NoDevice(), _NoDevice(), PipelineParams(), torch.zeros(3), **kw)


def _call_rasterizer(**kw):
    from diff_gaussian_rasterization import GaussianRasterizer
    return GaussianRasterizer(_settings())(means3D=torch.zeros(P, 3), means2D=torch.zeros(P, 3), opacities=torch.ones(P, 1),
                                           colors_precomp=torch.zeros(P, 3), scales=torch.ones(P, 3),
                                           rotations=torch.ones(P, 4), **kw)


def _call_rasterize_gaussians(**kw):
    from diff_gaussian_rasterization import rasterize_gaussians
    return rasterize_gaussians(torch.zeros(P, 3), torch.zeros(P, 3), None, None, torch.zeros(P, 3), torch.ones(P, 1),
                               torch.ones(P, 3), torch.ones(P, 4), None, _settings(), **kw)


SURFACES = [_call_render, _call_rasterizer, _call_rasterize_gaussians]


@pytest.mark.parametrize("name,value,exc", INVALID, ids=[f"{n}={v!r}" for n, v, _ in INVALID])
@pytest.mark.parametrize("surface", SURFACES, ids=["render", "GaussianRasterizer", "rasterize_gaussians"])
def test_every_surface_refuses_a_bad_option_alike(surface, name, value, exc):
    with pytest.raises(exc, match=f"{name}=") as e:
        surface(**{name: value})
    assert type(e.value) is exc and str(e.value).startswith(f"{name}={value!r}")


@pytest.mark.parametrize("kw", VALID, ids=[str(i) for i in range(len(VALID))])
@pytest.mark.parametrize("surface", SURFACES[1:], ids=["GaussianRasterizer", "rasterize_gaussians"])
def test_valid_options_reach_the_device_check(surface, kw):
    from diff_gaussian_rasterization import _C
    with pytest.raises(_C.GsrError, match="no CPU path"):
        surface(**kw)


def test_record_defaults_are_the_surfaces_defaults():
    import inspect
    from diff_gaussian_rasterization import GaussianRasterizer, RasterOptions, check_options, rasterize_gaussians
    o = check_options(RasterOptions())
    assert o == (False, None, None, None, None, True, "inverse", False, False, 0.5, False)
    for f in (GaussianRasterizer.forward, rasterize_gaussians):
        sig = inspect.signature(f).parameters
        assert {n: sig[n].default for n in RasterOptions._fields} == o._asdict(), f


# ------------------------------------------------------------------------------------------------------------------------------
# include/gsr.h against the hand-written argtypes

def _declared_parameter_counts():
    """{function name: number of parameters} of every function declared in include/gsr.h: comments stripped, the parenthesised
    list split on commas, `(void)` = 0 (the header has no function-pointer parameters)."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "gsr.h")
    with open(path) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = "\n".join(l for l in text.split("\n") if not l.lstrip().startswith("#"))
    out = {}
    for name, params in re.findall(r"\b(gsr_\w+)\s*\(([^()]*)\)\s*;", text):
        assert name not in out, name
        params = params.strip()
        out[name] = 0 if params in ("void", "") else len(params.split(","))
    return out


def test_every_declared_function_has_argtypes_of_its_parameter_count():
    from diff_gaussian_rasterization import _C
    declared = _declared_parameter_counts()
    assert len(declared) > 60 and set(declared) == set(_C.EXPORTS)
    wrong = {n: (c, len(_C.EXPORTS[n][1])) for n, c in declared.items() if c != len(_C.EXPORTS[n][1])}
    assert not wrong, wrong


def test_every_ex_entry_is_its_base_plus_the_extras_pointer():
    from diff_gaussian_rasterization import _C
    ex = [n for n in _C.EXPORTS if n.endswith("_ex")]
    assert len(ex) == 11
    for n in ex:
        res, args = _C.EXPORTS[n]
        base_res, base_args = _C.EXPORTS[n[:-3]]
        assert res is base_res and args == base_args + [C.POINTER(_C.gsr_render_extras)], n
