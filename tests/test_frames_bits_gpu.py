"""The sensor-frame kernels (csrc/frames.hip) held to the float32 rule of include/gsr.h bit for bit: gsr_frame_undistort against
FR.undistort_reference(..., np.float32) - mask, depth and colour on EVERY pixel, ties and border pixels included - and
gsr_frame_pyramid against FR.pyramid_reference at every size around the 32-px block, plane combination, load path and class of
depth reading.  tests/test_frames_cpu.py checks on the reference alone that each case has what it is here for."""
import numpy as np
import pytest
import torch

import frames_reference as FR
from scene_utils import Frame, undistort, build_pyramid

pytestmark = pytest.mark.gpu


def _dev(a):
    return None if a is None else torch.tensor(a).cuda()


def _undistort_bits(case, with_depth=True, label=""):
    """One launch of `case`; asserts zero differing elements in mask, depth and colour over the whole target, no pixel left out.
    -> (color, depth, mask) as numpy."""
    depth = case["depth"] if with_depth else None
    ref = FR.undistort_reference(case["color"], depth, case["K"], case["D"], case["new_K"], case["W"], case["H"], np.float32)
    col, dep, msk = undistort(_dev(case["color"]), _dev(depth), case["K"], case["D"], size=(case["W"], case["H"]), new_K=case["new_K"])
    torch.cuda.synchronize()
    col, msk = col.cpu().numpy(), msk.cpu().numpy()
    assert col.shape == (3, case["H"], case["W"]) and msk.shape == (case["H"], case["W"])
    n_mask = int(FR.differing(msk, ref["mask"]).sum())
    n_col = int(FR.differing(col, ref["color"]).any(0).sum())
    n_dep = 0
    if with_depth:
        dep = dep.cpu().numpy()
        n_dep = int(FR.differing(dep, ref["depth"]).sum())
    else:
        assert dep is None
    print(f"undistort bits {label}: {case['Ws']} x {case['Hs']} -> {case['W']} x {case['H']}, depth {with_depth}: differing pixels "
          f"mask {n_mask}, depth {n_dep}, colour {n_col} of {case['W'] * case['H']} (inside {ref['mask'].mean():.3f})")
    assert (n_mask, n_dep, n_col) == (0, 0, 0), (label, n_mask, n_dep, n_col)
    return col, dep, msk


# ------------------------------------------------------------------------------------------------------------------------------
# undistortion
# ------------------------------------------------------------------------------------------------------------------------------
def test_undistort_shared_scene_bit_for_bit_and_repeatable():
    """test_frames_gpu's scene (80 x 60 -> 72 x 56) with no pixel left out, twice: the same bits both times.  With the kernel's
    arithmetic contracted to fma (before frames.hip was compiled without contraction) this differed: profiles/frames.txt."""
    sc = FR.undistort_scene()
    first = _undistort_bits(sc, label="shared scene")
    again = _undistort_bits(sc, label="shared scene, again")
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(first, again))
    _undistort_bits(sc, with_depth=False, label="shared scene")


@pytest.mark.parametrize("H", FR.EDGE_H)
@pytest.mark.parametrize("W", FR.EDGE_W)
def test_undistort_target_sizes_at_the_workgroup_edges(W, H):
    """80 x 60 -> W x H around the 64 x 4 workgroup, barrel and pincushion (k3, p1, p2 non-zero), with depth and without (the
    latter k_frame_undistort<false, false>)."""
    for name, dist in (("barrel", FR.BARREL), ("pincushion", FR.PINCUSHION)):
        case = FR.undistort_case(80, 60, W, H, dist)
        for with_depth in (True, False):
            _undistort_bits(case, with_depth, label=name)


@pytest.mark.parametrize("name", list(FR.undistort_named_cases()))
def test_undistort_named_cases(name):
    """Tiny sources (1 x 1: only us = vs = 0 is inside), coordinates exactly on integers, half-integers (every pixel a nearest-pixel
    tie), 0 and src_w - 1, coordinates that overflow to inf / NaN (outside, exactly 0), up- and strong downsampling, and NaN / inf /
    negative source values (depth copied verbatim, colour as IEEE 754 propagates them)."""
    case = FR.undistort_named_cases()[name]
    col, dep, msk = _undistort_bits(case, True, label=name)
    _undistort_bits(case, False, label=name)
    assert (col[:, msk == 0] == 0).all() and (dep[msk == 0] == 0).all() and set(np.unique(msk).tolist()) <= {0.0, 1.0}
    if name == "overflow":
        us, vs = FR.undistort_map(case["K"], case["D"], case["new_K"], case["W"], case["H"], np.float32)
        bad = ~(np.isfinite(us) & np.isfinite(vs))
        assert bad.any() and (msk[bad] == 0).all() and (msk == 1).any()
    if name == "special_values":
        assert np.isnan(col).any() and np.isposinf(dep).any() and np.isneginf(dep).any() and (dep == -1.5).any()


def test_undistort_full_frame_through_from_sensor():
    """640 x 480 through Frame.from_sensor, every pixel, and a second run with identical bits."""
    case = FR.undistort_full_frame_case()
    ref = FR.undistort_reference(case["color"], case["depth"], case["K"], case["D"], case["new_K"], case["W"], case["H"], np.float32)
    color, depth = _dev(case["color"]), _dev(case["depth"])
    runs = []
    for _ in range(2):
        fr = Frame.from_sensor(color, depth, case["K"], case["D"])
        torch.cuda.synchronize()
        runs.append((fr.image.cpu().numpy(), fr.depth.cpu().numpy(), fr.mask.cpu().numpy()))
    col, dep, msk = runs[0]
    n = (int(FR.differing(msk, ref["mask"]).sum()), int(FR.differing(dep, ref["depth"]).sum()),
         int(FR.differing(col, ref["color"]).any(0).sum()))
    print(f"undistort bits, 640 x 480: differing pixels mask {n[0]}, depth {n[1]}, colour {n[2]} (inside {ref['mask'].mean():.3f})")
    assert n == (0, 0, 0), n
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(*runs))


# ------------------------------------------------------------------------------------------------------------------------------
# pyramid
# ------------------------------------------------------------------------------------------------------------------------------
def _same(t, want):
    return t.shape == want.shape and not FR.differing(t.cpu().numpy(), want).any()


def _check_pyramid(out, ref, levels, planes="cdm"):
    c, d, m = out
    assert len(c) == levels and (d is None) == ("d" not in planes) and (m is None) == ("m" not in planes)
    for l in range(levels):
        rc, rd, rm = ref[l]
        assert _same(c[l], rc), ("colour", l)
        assert d is None or _same(d[l], rd), ("depth", l)
        assert m is None or _same(m[l], rm), ("mask", l)


@pytest.mark.parametrize("H", FR.PYR_H)
@pytest.mark.parametrize("W", FR.PYR_W)
def test_pyramid_sizes_levels_and_plane_combinations(W, H):
    """W x H around the 32-px block and its halvings, every `levels` the size allows, colour alone / + depth / + mask / all three:
    each call bit-equal to the float32 chain for the planes it has (so to the all-three call)."""
    color, depth, mask = FR.pyramid_scene(W, H, seed=W * 100 + H)
    top = FR.max_levels(W, H)
    assert top >= 1
    ref = FR.pyramid_reference(color, depth, mask, top)
    c, d, m = _dev(color), _dev(depth), _dev(mask)
    for levels in range(1, top + 1):
        for planes, (dd, mm) in (("c", (None, None)), ("cd", (d, None)), ("cm", (None, m)), ("cdm", (d, m))):
            _check_pyramid(build_pyramid(c, dd, mm, levels), ref, levels, planes)
    if (W, H) == (2, 2):
        assert tuple(build_pyramid(c, d, m, 1)[0][0].shape) == (3, 1, 1)


@pytest.mark.parametrize("size", [(66, 33), (4, 2), (32, 32)])
def test_pyramid_misaligned_inputs_take_the_scalar_loads(size):
    """An even width with each input in turn starting one float past an 8-byte boundary (a contiguous view into a larger buffer,
    which the Python wrapper passes on unchanged): the 4-byte load path, the same bits as the aligned call."""
    W, H = size
    color, depth, mask = FR.pyramid_scene(W, H, seed=W)
    levels = FR.max_levels(W, H)
    ref = FR.pyramid_reference(color, depth, mask, levels)

    def shifted(a):
        buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
        t = buf[1:].view(a.shape)
        t.copy_(torch.tensor(a))
        assert t.is_contiguous() and t.data_ptr() % 8 == 4
        return t
    aligned = [_dev(color), _dev(depth), _dev(mask)]
    assert all(t.data_ptr() % 8 == 0 for t in aligned)
    _check_pyramid(build_pyramid(*aligned, levels), ref, levels)
    for i, a in enumerate((color, depth, mask)):
        args = list(aligned)
        args[i] = shifted(a)
        _check_pyramid(build_pyramid(*args, levels), ref, levels)
    _check_pyramid(build_pyramid(shifted(color), shifted(depth), shifted(mask), levels), ref, levels)


@pytest.mark.parametrize("band", [0.05, 0.0, 1e6, 3e38])
@pytest.mark.parametrize("level", [1, 2, 3])
def test_pyramid_depth_classes_and_mask_values(level, band):
    """FR.depth_class_quads - 0 to 4 valid readings, +inf alone and beside finite readings, NaN, negative, -0.0, denormals, four
    equal readings, a reading exactly on m (1 + band) (inside) and one ulp above it (outside) - at the stride of level `level`,
    with the default band, band 0, a band that takes every reading and one whose product overflows; mask values 0.5, 2 and NaN."""
    color, depth, mask, where = FR.depth_class_scene(band, level)
    ref = FR.pyramid_reference(color, depth, mask, level, band)
    out = build_pyramid(_dev(color), _dev(depth), _dev(mask), level, depth_band=band)
    _check_pyramid(out, ref, level)
    d = out[1][-1].cpu().numpy()
    assert np.isfinite(d).all()
    for name in ("inf_alone", "inf_and_holes", "valid0", "nan_alone"):
        assert d[where[name]] == 0, name
    assert d[where["inf_beside_finite"]] == 2
    m = out[2][0].cpu().numpy()
    assert set(np.unique(m).tolist()) == {0.0, 1.0}
