"""GaussianModel.transform_ / correct_keyframes on the device (csrc/transform.hip, gsr_transform_gaussians) against the float64
restatement of tests/transform_reference.py, and what the feature means: the moved map seen from the moved camera is the old
map seen from the old camera - image, depth, opacity and gradients, held to the float64 oracle of the ORIGINAL scene.

Tolerances of the parameter comparison are derived, not tuned.  Every output of a moved row is a dot product of n terms of
float32-rounded factors accumulated in float32: at most n + 2 roundings (one factor rounded from float64, n products or fused
steps, the final store is exact), so |out - ref| <= gamma_(n+2) sum_j |a_j| |b_j| with gamma_m = m u / (1 - m u), u = 2^-24:
n = 4 for the quaternion, n = 2 l + 1 for SH band l, n = 2 for log-scale + ln s.  Positions are formed in float64 and rounded
once: |out - ref| <= u |ref|."""
import functools
import math

import numpy as np
import pytest
import torch

import mapping_reference as MR
import transform_reference as TR
from scene_utils import (GaussianModel, RawGaussians, correct_keyframes, fibonacci_cameras, make_gaussians, transform_camera)
from scene_utils.model import _PARAM_ATTRS
from test_depth_alpha_gpu import BG, _close, hip_rgbd, oracle_rgbd
from test_parity_gpu import check_grads

pytestmark = pytest.mark.gpu
U = TR.U
MOVED = ("_xyz", "_rotation", "_scaling", "_features_rest")


def device_model(P, deg, seed=5, optimizer=True, box_offset=0.0):
    raw = make_gaussians(P, deg, seed=seed)
    raw.xyz += box_offset
    m = GaussianModel.from_raw(raw.to("cuda"))
    if optimizer:
        m.training_setup(optimizer="hip")
        gen = torch.Generator().manual_seed(seed + 1)
        for a in _PARAM_ATTRS:                                # live moments, as after a few steps
            p = getattr(m, a)
            m.optimizer.state[p] = {"step": torch.tensor(3.0), "exp_avg": torch.randn(p.shape, generator=gen).cuda(),
                                    "exp_avg_sq": torch.rand(p.shape, generator=gen).cuda() + 0.1}
    return m


def snapshot(m):
    params = {a: getattr(m, a).detach().clone() for a in _PARAM_ATTRS}
    opt = getattr(m, "optimizer", None)
    mom = {}
    for a in _PARAM_ATTRS:                                    # (an optimizer that has not stepped yet holds no moments)
        st = opt.state.get(getattr(m, a)) if opt is not None else None
        if st and "exp_avg" in st:
            mom[a] = (st["exp_avg"].clone(), st["exp_avg_sq"].clone())
    return params, mom


def transforms(K, seed, t_scale=1.0, s=1.0):
    rng = np.random.default_rng(seed)
    return np.stack([TR.make_T(TR.random_rotation(rng, rng.uniform(0.8, 1.2)), t_scale * rng.normal(size=3), s)
                     for _ in range(K)])


def check_parameters(m, before, T, index, label):
    """Moved rows within the derived bounds of the float64 reference; every other row and f_dc / opacity bit-equal."""
    ref, moved = TR.transform_reference(before["_xyz"], before["_rotation"], before["_scaling"], before["_features_rest"], T, index)
    for a in ("_features_dc", "_opacity"):
        assert torch.equal(getattr(m, a).detach(), before[a]), (label, a)
    n_rest = before["_features_rest"].shape[1]
    g_rest = torch.tensor([TR.gamma(2 * int(l) + 1 + 2) for l in TR.band_of_rest_row(n_rest)], dtype=torch.float64)[None, :, None]
    bounds = {"_xyz": lambda v, mag: U * v.abs(), "_rotation": lambda v, mag: TR.gamma(6) * mag,
              "_scaling": lambda v, mag: TR.gamma(4) * mag, "_features_rest": lambda v, mag: g_rest * mag}
    for a, key in zip(MOVED, ("xyz", "rotation", "scaling", "features_rest")):
        out = getattr(m, a).detach().cpu()
        assert torch.equal(out[~moved], before[a].cpu()[~moved]), (label, a, "an unmoved row changed")
        if out.numel() == 0 or not bool(moved.any()):
            continue
        val, mag = ref[key]
        err = (out.double() - val).abs()[moved]
        bound = bounds[a](val, mag)[moved]
        print(f"{label} {a}: max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), (label, a, float((err / bound.clamp_min(1e-300)).max()))
    return moved


def check_moments(m, mom_before, moved, mode, label):
    for a in _PARAM_ATTRS:
        st = m.optimizer.state[getattr(m, a)]
        for got, old in zip((st["exp_avg"], st["exp_avg_sq"]), mom_before[a]):
            got, old = got.cpu(), old.cpu()
            if mode == "keep" or a not in MOVED:
                assert torch.equal(got, old), (label, a)
            else:
                assert torch.equal(got[~moved], old[~moved]), (label, a)
                assert float(got[moved].abs().sum()) == 0.0 if got[moved].numel() else True, (label, a)


# ------------------------------------------------------------------------------------------------------------------------------
# 1, 2  parameters and moments against the float64 reference
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 255, 257, 1000])
@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_one_transform_moves_every_row(P, deg):
    m = device_model(P, deg)
    before, mom = snapshot(m)
    T = transforms(1, seed=P + deg)
    assert m.transform_(T[0]) == P
    moved = check_parameters(m, before, T, None, f"K=1 P={P} deg={deg}")
    assert bool(moved.all())
    check_moments(m, mom, moved, "reset", f"K=1 P={P} deg={deg}")


@pytest.mark.parametrize("P", [1, 255, 257, 1000])
@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_five_transforms_by_anchor(P, deg):
    m = device_model(P, deg)
    choices = torch.tensor([-1, 0, 1, 2, 3, 4, 7])
    anchors = choices[torch.randint(0, 7, (P,), generator=torch.Generator().manual_seed(P))]
    m.set_anchors(anchors)
    before, mom = snapshot(m)
    T = transforms(5, seed=10 + P + deg)
    n = m.transform_(torch.tensor(T).cuda(), ids=[0, 1, 2, 3, 4])            # device matrices: trusted, not read back
    moved = check_parameters(m, before, T, anchors, f"K=5 P={P} deg={deg}")
    assert n == int(moved.sum()) == int(((anchors >= 0) & (anchors < 5)).sum())
    check_moments(m, mom, moved, "reset", f"K=5 P={P} deg={deg}")
    assert torch.equal(m._anchor.cpu().long(), anchors)


def test_ids_are_keyframe_ids_not_positions():
    """ids = (7, 2): rows anchored to 7 move by T[0], rows anchored to 2 by T[1], the rest stay."""
    P = 600
    m = device_model(P, 3)
    anchors = torch.tensor([-1, 0, 1, 2, 3, 4, 7])[torch.randint(0, 7, (P,), generator=torch.Generator().manual_seed(1))]
    m.set_anchors(anchors)
    before, mom = snapshot(m)
    T = transforms(2, seed=77)
    index = torch.where(anchors == 7, 0, torch.where(anchors == 2, 1, -1))
    assert m.transform_(T, ids=[7, 2], moments="keep") == int((index >= 0).sum())
    moved = check_parameters(m, before, T, index, "ids=(7,2)")
    check_moments(m, mom, moved, "keep", "ids=(7,2)")


def test_far_from_the_origin_positions_keep_their_bits():
    """t of order 1e4 and a map that sits 3e3 from the origin: the float64 position arithmetic rounds once."""
    m = device_model(1000, 1, box_offset=3.0e3)
    before, mom = snapshot(m)
    T = transforms(1, seed=3, t_scale=1.0e4)
    assert float(np.abs(T[0, :3, 3]).max()) > 5.0e3
    assert m.transform_(T) == 1000
    check_parameters(m, before, T, None, "t ~ 1e4")


def test_empty_model_and_no_transforms():
    few = make_gaussians(4, 2, seed=1)
    m = GaussianModel.from_raw(RawGaussians(*(t[:0] for t in few.tensors()), 2).to("cuda"))
    assert m.transform_(transforms(1, seed=1)[0]) == 0
    m = device_model(10, 2)
    before, _ = snapshot(m.set_anchors(0))
    assert m.transform_(np.zeros((0, 4, 4)), ids=[]) == 0
    assert all(torch.equal(getattr(m, a).detach(), before[a]) for a in _PARAM_ATTRS)


def test_without_an_optimizer_and_bitwise_reproducible():
    T = transforms(3, seed=9)
    outs = []
    for _ in range(2):
        m = device_model(700, 3, optimizer=False)
        m.set_anchors(torch.arange(700) % 4)
        assert m.transform_(T, ids=[0, 1, 2], count=False) is None
        outs.append([getattr(m, a).detach().clone() for a in _PARAM_ATTRS])
    assert all(torch.equal(a, b) for a, b in zip(*outs))


def test_c_abi_rejects_bad_arguments_before_any_device_work():
    import ctypes as C
    from diff_gaussian_rasterization import _C
    lib = _C.lib()
    m = device_model(64, 3, optimizer=False)
    before, _ = snapshot(m)
    T = torch.tensor(transforms(1, seed=2)).cuda()
    ws = torch.empty(lib.gsr_transform_workspace_bytes(1), dtype=torch.uint8, device="cuda")
    assert lib.gsr_transform_workspace_bytes(64) >= 64 * (12 * 8 + 4 * 4 + 4 + 83 * 4)

    def call(P=64, rest=15, ws_bytes=ws.numel(), xyz=m._xyz):
        return lib.gsr_transform_gaussians(P, None, 1, _C.ptr(T), _C.ptr(ws), ws_bytes, _C.ptr(xyz), _C.ptr(m._rotation),
                                           _C.ptr(m._scaling), _C.ptr(m._features_rest), rest, None, _C._stream())
    for kw in (dict(rest=4), dict(rest=-1), dict(ws_bytes=16), dict(xyz=None)):
        assert call(**kw) == -1, kw                          # GSR_ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert all(torch.equal(getattr(m, a).detach(), before[a]) for a in _PARAM_ATTRS)
    assert call(P=0) == 0 and call() == 0


# ------------------------------------------------------------------------------------------------------------------------------
# 3, 4, 5  the moved map from the moved camera is the old map from the old camera
# ------------------------------------------------------------------------------------------------------------------------------
W, H, P_SCENE = 80, 48, 2000


@functools.lru_cache(maxsize=None)
def scene():
    """The scene, its camera, the upstream colour gradient and the float64 oracle's render + gradients of the ORIGINAL scene
    (computed once, shared, never modified)."""
    raw = make_gaussians(P_SCENE, 3, seed=31)
    cam = fibonacci_cameras(1, W, H, seed=8)[0]
    gc = torch.randn(3, H, W, generator=torch.Generator().manual_seed(4))
    zero = torch.zeros(1, H, W)
    ref = oracle_rgbd(raw, cam, grads=(gc, zero, zero))
    assert float(raw.features_rest.abs().max()) > 0.05
    return raw, cam, gc, ref


def moved_scene(T, **kw):
    """The scene's model on the device after transform_(T) -> (RawGaussians on the host, the model)."""
    raw = scene()[0]
    m = GaussianModel.from_raw(raw.to("cuda"), active_sh_degree=3)
    assert m.transform_(T, **kw) == P_SCENE
    out = RawGaussians(*(getattr(m, a).detach().cpu() for a in ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation",
                                                               "_opacity")), 3)
    return out, m


def assert_same_render(out, ref, depth_scale=1.0):
    dmax = float(ref["D"].abs().max())
    assert dmax > 0.5 and float(ref["A"].max()) > 0.5          # there is something to compare
    for name, x, r, scale in (("color", out["color"], ref["color"], None), ("alpha", out["A"], ref["A"], None),
                              ("depth", out["D"], depth_scale * ref["D"], depth_scale * dmax)):
        ok, err = _close(x, r, scale)
        over = int(((x.double() - r.double()).abs() / (scale or 1.0) > 2e-5).sum())
        print(f"render {name}: max err {err:.3e}, {over} of {x.numel()} values over 2e-5")
        assert ok, (name, err)


def test_render_is_invariant_and_needs_the_sh_rotation():
    raw, cam, gc, ref = scene()
    T = TR.make_T(TR.random_rotation(np.random.default_rng(12), 1.0), [0.4, -0.7, 0.5])
    raw2, _ = moved_scene(T)
    cam2 = transform_camera(cam, T)
    out = hip_rgbd(raw2, cam2, camera=False)
    assert_same_render(out, ref)
    # the same move with features_rest left as it was: the view-dependent colour points the wrong way, and the comparison sees it
    stale = RawGaussians(raw2.xyz, raw2.features_dc, raw.features_rest, raw2.scaling, raw2.rotation, raw2.opacity, 3)
    bad = hip_rgbd(stale, cam2, camera=False)
    ok, err = _close(bad["color"], ref["color"])
    print(f"unrotated f_rest: max colour err {err:.3e}")
    assert not ok
    assert _close(bad["A"], ref["A"])[0]                     # geometry alone is right: only the SH bands were missing


def test_gradients_are_equivariant():
    raw, cam, gc, ref = scene()
    R = TR.random_rotation(np.random.default_rng(13), 1.0)
    T = TR.make_T(R, [-0.3, 0.2, 0.6])
    raw2, _ = moved_scene(T)
    out = hip_rgbd(raw2, transform_camera(cam, T), grads=(gc, None, None), camera=False)
    M = TR.sh_rotation(R, 3)
    g = ref["grads"]
    mapped = {"means3D": g["means3D"] @ torch.tensor(R).T,                       # dL/dxyz' = R dL/dxyz
              "shs": torch.einsum("ab,nbc->nac", M, g["shs"])}                   # dL/dc'_l = D_l dL/dc_l (band 0: identity)
    check_grads(dict(grads={k: out["grads"][k] for k in mapped}), dict(grads=mapped))


def test_similarity_scales_the_depth_and_nothing_else():
    raw, cam, gc, ref = scene()
    s = 1.5
    T = TR.make_T(TR.random_rotation(np.random.default_rng(16), 1.0), [0.2, 0.1, -0.4], s)
    # Precondition, from the oracle alone: the float64-moved scene through the moved (float32) camera is the original render.
    # The moved camera is rounded to float32, a perturbation of 1e-7 that can carry one (pixel, Gaussian) pair across the
    # rasterizer's alpha >= 1/255 threshold; at 80x48 the bar admits no such pixel.  (Seed 14 is such a case: the float64
    # oracle itself then differs from the original render by 2.5e-4 in one pixel.  Seeds 15..18 are not.)
    r64, _ = TR.transform_reference(raw.xyz, raw.rotation, raw.scaling, raw.features_rest, T[None], None)
    exact = RawGaussians(r64["xyz"][0], raw.features_dc, r64["features_rest"][0], r64["scaling"][0], r64["rotation"][0],
                         raw.opacity, 3)
    assert_same_render(oracle_rgbd(exact, transform_camera(cam, T)), ref, depth_scale=s)
    m = GaussianModel.from_raw(raw.to("cuda"), active_sh_degree=3)
    with pytest.raises(ValueError, match="allow_scale"):
        m.transform_(T)
    before, _ = snapshot(m)
    raw2, m = moved_scene(T, allow_scale=True)
    check_parameters(m, before, T[None], None, "s=1.5")
    assert float((raw2.scaling - raw.scaling - math.log(s)).abs().max()) < 1e-6
    # every Gaussian is farther than the 0.2 near plane before and after: the cull removes nothing new
    vm = cam.world_view_transform.double()
    z = raw.xyz.double() @ vm[:3, 2] + vm[3, 2]
    assert float(z.min()) > 0.2 and s * float(z.min()) > 0.2
    out = hip_rgbd(raw2, transform_camera(cam, T), camera=False)
    assert_same_render(out, ref, depth_scale=s)


# ------------------------------------------------------------------------------------------------------------------------------
# 6  anchors end to end
# ------------------------------------------------------------------------------------------------------------------------------
def anchor_scene(sheet_seed=0, stride=4):
    """Two 32x32 RGB-D keyframes inserted with anchors 0 and 1 (every fourth pixel each way: 64 Gaussians per frame), then a
    densification (clones and splits) and a prune, the anchor bookkeeping checked at every step -> (model, the two cameras).
    Why the stride: with a Gaussian per pixel the part rendered below is a thousand one-pixel-wide splats of opacity 0.5, and
    some eight pixels of it sit so close to the rasterizer's alpha >= 1/255 cut that the float32 rounding of ANY re-expression
    of the scene moves them across it (measured over six such scenes: colour differences of 2.6e-4 .. 4.9e-3 <= 1.3 / 255 in
    4 .. 9 pixels of five of them, 1.2e-6 everywhere in the sixth, radii identical in all) - at 32x32 the parity bar admits no
    such pixel.  Sixteen times fewer, four times wider splats leave the bar meaningful."""
    cams = fibonacci_cameras(6, 32, 32, seed=4, device="cuda")[2:4]
    m = GaussianModel(3)
    for k, cam in enumerate(cams):
        depth = torch.tensor(MR.depth_sheet(32, 32, seed=sheet_seed + k)).cuda()
        image = torch.rand(3, 32, 32, generator=torch.Generator().manual_seed(k)).cuda()
        n = m.add_from_rgbd(cam, image, depth, anchor=k, stride=stride)
        assert n == (32 // stride) ** 2 and m._anchor.shape[0] == m.get_xyz.shape[0] == (k + 1) * n
    assert torch.equal(m._anchor.cpu(), torch.arange(2, dtype=torch.int32).repeat_interleave((32 // stride) ** 2))
    P = m.get_xyz.shape[0]
    m.training_setup(optimizer="hip")
    with torch.no_grad():
        m._features_rest.copy_(0.05 * torch.randn(m._features_rest.shape, generator=torch.Generator().manual_seed(9)))
    # a densification that clones and splits: every new row carries its source's anchor
    m.xyz_gradient_accum = torch.rand(P, 1, generator=torch.Generator().manual_seed(2)).cuda()
    m.denom = torch.ones(P, 1, device="cuda")
    old = m._anchor.clone()
    med = float(m.get_scaling.detach().max(dim=1).values.median())
    nk, nc, ns, src = m.densify_and_prune(0.7, 0.005, med / m.percent_dense, None, return_source=True)
    assert nc > 0 and ns > 0 and m._anchor.shape[0] == m.get_xyz.shape[0] == nk + nc + 2 * ns
    assert torch.equal(m._anchor, old[src.long()])
    old = m._anchor.clone()
    mask = torch.rand(m.get_xyz.shape[0], generator=torch.Generator().manual_seed(3)).cuda() < 0.2
    assert m.prune_points(mask) == int(mask.sum())
    assert m._anchor.shape[0] == m.get_xyz.shape[0] and torch.equal(m._anchor, old[~mask])
    return m, cams


def model_part(m, rows):
    return RawGaussians(*(getattr(m, a).detach().cpu()[rows] for a in ("_xyz", "_features_dc", "_features_rest", "_scaling",
                                                                      "_rotation", "_opacity")), 3)


def test_anchors_follow_rows_and_one_keyframe_correction_moves_only_its_rows():
    m, cams = anchor_scene()
    # loop closure: keyframe 1 is corrected, keyframe 0 is not
    mine = (m._anchor == 1).cpu()
    assert 0 < int(mine.sum()) < mine.numel()
    view_before = hip_rgbd(model_part(m, mine), cams[1], camera=False)
    before, _ = snapshot(m)
    T = TR.make_T(TR.random_rotation(np.random.default_rng(15), 0.4), [0.05, -0.1, 0.08])
    new_cams = correct_keyframes(m, {0: cams[0], 1: cams[1]}, {1: T})
    assert new_cams[0] is cams[0] and new_cams[1] is not cams[1]
    for a in _PARAM_ATTRS:
        assert torch.equal(getattr(m, a).detach().cpu()[~mine], before[a].cpu()[~mine]), a
    index = torch.where(mine, 0, -1)
    moved = check_parameters(m, before, T[None], index, "keyframe 1")
    assert torch.equal(moved, mine)
    view_after = hip_rgbd(model_part(m, mine), new_cams[1], camera=False)
    flips = view_after["radii"] != view_before["radii"]
    print(f"keyframe 1: {int(mine.sum())} rows, radii that differ after the move: {int(flips.sum())}")
    assert float(view_before["A"].max()) > 0.5
    assert_same_render(view_after, view_before)
