"""gsr_odometry_prepare on the device against tests/odometry_reference.py: bit equality - NaN in the same places, identical float32
bits elsewhere.  Sizes: 1 x 1, 2 x 2, 3 x 3 (no, no and one pixel off the border), one less than, equal to and one more than the
32 x 8 tile in each direction, and 257 x 67 (nine tiles by nine, the last column of tiles one pixel wide)."""
import functools

import numpy as np
import pytest
import torch

import frames_reference as FR
import odometry_reference as OR
import scene_utils as S
from diff_gaussian_rasterization import _C

pytestmark = pytest.mark.gpu

TW, TH = _C.ODOMETRY_TILE_W, _C.ODOMETRY_TILE_H
SIZES = [(1, 1), (2, 2), (3, 3)] + [(w, h) for w in (TW - 1, TW, TW + 1) for h in (TH - 1, TH, TH + 1)] + [(257, 67)]
DEPTH_MIN, DEPTH_MAX = 0.5, 3.0


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def scene(w, h):
    """colour noise with NaN and inf sprinkled in; a depth between 1 and 2.5 with holes - 0, NaN, +-inf, negative, and values
    exactly at depth_min (invalid) and depth_max (valid) and one float32 step to either side; a mask with 0, 0.5 and 1"""
    f = np.float32
    rng = np.random.default_rng([w, h])
    color = rng.random((3, h, w), dtype=f)
    hit = rng.random((3, h, w)) < 0.02
    color[hit] = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype=f), size=int(hit.sum()))
    depth = (1.0 + 1.5 * rng.random((h, w))).astype(f)
    special = np.array([0.0, np.nan, np.inf, -np.inf, -1.5, DEPTH_MIN, np.nextafter(f(DEPTH_MIN), f(1)), DEPTH_MAX,
                        np.nextafter(f(DEPTH_MAX), f(4)), np.nextafter(f(DEPTH_MAX), f(0))], dtype=f)
    hit = rng.random((h, w)) < 0.15
    depth[hit] = rng.choice(special, size=int(hit.sum()))
    mask = rng.choice(np.array([1, 1, 1, 1, 1, 1, 1, 1, 0, 0.5], dtype=f), size=(h, w))
    return color, depth, mask


def check(got, want, what):
    bad = FR.differing(got.cpu().numpy(), want)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist())


@pytest.mark.parametrize("w,h", SIZES)
def test_prepare_bits(w, h):
    color, depth, mask = scene(w, h)
    K = OR.size_K(w, h)
    for m in (mask, None):
        I, D, g = OR.prepare(color, depth, m, DEPTH_MIN, DEPTH_MAX)
        lv = S.prepare_odometry_level(dev(color), dev(depth), dev(m), K, DEPTH_MIN, DEPTH_MAX)
        assert (lv.width, lv.height, lv.K) == (w, h, K) and lv.grad.shape == (4, h, w)
        check(lv.intensity, I, "intensity")
        check(lv.depth, D, "depth")
        check(lv.grad, g, "grad")
        # without gradients: the same two planes, nothing else
        src = S.prepare_odometry_level(dev(color), dev(depth), dev(m), K, DEPTH_MIN, DEPTH_MAX, gradients=False)
        assert src.grad is None
        check(src.intensity, I, "intensity, no gradients")
        check(src.depth, D, "depth, no gradients")


def test_the_scene_has_what_it_is_there_for():
    color, depth, mask = scene(257, 67)
    I, D, g = OR.prepare(color, depth, mask, DEPTH_MIN, DEPTH_MAX)
    f = np.float32
    assert np.isnan(D[depth == f(DEPTH_MIN)]).all() and (depth == f(DEPTH_MIN)).any()
    at_max = (depth == f(DEPTH_MAX)) & (mask == 1)
    assert at_max.any() and (D[at_max] == f(DEPTH_MAX)).all()
    assert np.isnan(D[depth > f(DEPTH_MAX)]).all() and np.isnan(D[mask == f(0.5)]).all() and np.isnan(I[mask == 0]).all()
    inner = np.zeros_like(depth, dtype=bool)
    inner[1:-1, 1:-1] = True
    assert np.isfinite(g[:, inner]).any() and np.isnan(g[:, inner]).any() and np.isnan(g[:, ~inner]).all()
    assert np.isinf(I).any()                           # an inf colour stays an inf (and its neighbours' gradients are not finite)


def test_depth_with_a_leading_axis_and_a_view():
    color, depth, mask = scene(33, 9)
    I, D, g = OR.prepare(color, depth, mask, DEPTH_MIN, DEPTH_MAX)
    wide = torch.zeros(3, 9, 40, device="cuda")
    wide[:, :, :33] = dev(color)
    lv = S.prepare_odometry_level(wide[:, :, :33], dev(depth).unsqueeze(0), dev(mask).double(), OR.size_K(33, 9), DEPTH_MIN, DEPTH_MAX)
    check(lv.intensity, I, "intensity")
    check(lv.depth, D, "depth")
    check(lv.grad, g, "grad")


def test_error_codes():
    lib = _C.lib()
    c, d = torch.zeros(3, 4, 4, device="cuda"), torch.zeros(4, 4, device="cuda")
    i, o, g = torch.zeros(4, 4, device="cuda"), torch.zeros(4, 4, device="cuda"), torch.zeros(4, 4, 4, device="cuda")
    p = _C.ptr

    def call(w=4, h=4, color=c, depth=d, lo=0.0, hi=4.0, io=i, do=o):
        return lib.gsr_odometry_prepare(w, h, p(color), p(depth), None, lo, hi, p(io), p(do), p(g), _C._stream())
    assert call() == 0
    for kw in (dict(color=None), dict(depth=None), dict(io=None), dict(do=None), dict(w=0), dict(h=0), dict(w=-1), dict(w=1 << 15, h=1 << 15),
               dict(lo=float("nan")), dict(hi=float("nan")), dict(lo=1.0, hi=1.0), dict(lo=2.0, hi=1.0)):
        assert call(**kw) == -1, kw                    # GSR_ERR_INVALID_ARGUMENT, before the launch
        assert "odometry_prepare" in _C.last_error()
    torch.cuda.synchronize()
