"""gsr_depth_densify on the device against tests/cloud_image_reference.py, bit for bit on every pixel of both outputs: image sizes
that give one tile, partial tiles and tile seams in both axes (a tile is 32 x 8), the smallest, the default and the largest
radius, and the input variants of the rule."""
import numpy as np
import pytest
import torch

import cloud_image_reference as CR
import scene_utils as S

pytestmark = pytest.mark.gpu
F32 = np.float32
SIZES = [(1, 1), (33, 9), (64, 16), (131, 67)]
BAND = 0.05


def sparse(W, H, seed, fill=0.1):
    """readings on a tenth of the pixels: a near layer on the left, a far one on the right, noise of a few percent on both"""
    rng = np.random.default_rng(seed)
    z = np.where(np.arange(W)[None, :] < W / 2, 1.5, 6.0) * (1.0 + 0.04 * rng.random((H, W)))
    return np.where(rng.random((H, W)) < fill, z, 0).astype(F32)


def two_layers(W, H, seed):
    """two surfaces interleaved pixel by pixel (a fence in front of a wall), with holes"""
    rng = np.random.default_rng(seed)
    z = np.where(rng.random((H, W)) < 0.5, 1.0, 3.0) * (1.0 + 0.03 * rng.random((H, W)))
    return np.where(rng.random((H, W)) < 0.35, z, 0).astype(F32)


def run(depth, R, k):
    dense, valid = S.densify_depth(torch.from_numpy(depth).cuda(), radius=R, depth_band=BAND, min_neighbors=k)
    assert dense.shape == depth.shape and valid.shape == depth.shape
    return dense.cpu().numpy(), valid.cpu().numpy()


def check(depth, R, k, what):
    want_d, want_v = CR.densify(depth, R, CR.occlusion_scale(BAND), k)
    got_d, got_v = run(depth, R, k)
    bad = got_d.view(np.uint32) != want_d.view(np.uint32)
    assert not bad.any(), f"{what}: dense differs on {int(bad.sum())} of {bad.size} pixels, first at {np.argwhere(bad)[0]}"
    bad = got_v.view(np.uint32) != want_v.view(np.uint32)
    assert not bad.any(), f"{what}: valid differs on {int(bad.sum())} of {bad.size} pixels, first at {np.argwhere(bad)[0]}"
    return got_d, got_v


@pytest.mark.parametrize("R", [1, 4, 8])
@pytest.mark.parametrize("W, H", SIZES)
def test_bit_exact(W, H, R):
    depth = sparse(W, H, seed=W + R)
    got_d, got_v = check(depth, R, 2, f"sparse {W}x{H} R={R}")
    if W >= 33:
        filled = (depth == 0) & (got_v == 1)
        assert filled.any()
        assert (got_d[depth > 0] == depth[depth > 0]).all()
    check(two_layers(W, H, seed=H + R), R, 2, f"two layers {W}x{H} R={R}")
    check(two_layers(W, H, seed=H + R), R, 1, f"two layers, one neighbour, {W}x{H} R={R}")


@pytest.mark.parametrize("R", [1, 4, 8])
@pytest.mark.parametrize("W, H", SIZES)
def test_empty_full_and_unreachable_count(W, H, R):
    empty = np.zeros((H, W), F32)
    d, v = check(empty, R, 1, "empty")
    assert not d.any() and not v.any()
    full = np.random.default_rng(W).uniform(0.3, 20.0, (H, W)).astype(F32)
    d, v = check(full, R, 1, "full")
    assert np.array_equal(d.view(np.uint32), full.view(np.uint32)) and (v == 1).all()
    depth = sparse(W, H, seed=5, fill=0.3)
    d, v = check(depth, R, (2 * R + 1) ** 2, "min_neighbors above what a window holds")
    assert np.array_equal(d.view(np.uint32), depth.view(np.uint32)) and np.array_equal(v, (depth > 0).astype(F32))


def test_a_single_reading_far_from_the_tile_of_its_hole():
    """one reading in the corner of a tile reaches holes of the three neighbouring tiles through their halos, and nothing else"""
    W, H, R = 96, 32, 8
    depth = np.zeros((H, W), F32)
    depth[15, 31] = 2.5      # last column and row of tile (0, 1); its window, rows 7 .. 23 and columns 23 .. 39, lies inside
    d, v = check(depth, R, 1, "single reading")
    # (w * z) / w: two roundings, 2^-23 relative at the most
    assert (v == 1).sum() == (2 * R + 1) ** 2 and np.allclose(d[v == 1], 2.5, rtol=2.0 ** -22, atol=0)
    assert v[23, 39] == 1 and v[24, 39] == 0 and v[23, 40] == 0 and v[6, 31] == 0 and v[7, 23] == 1
