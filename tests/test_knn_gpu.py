"""gsr_knn_dist2 / simple_knn.distCUDA2 against the float64 brute force on the same float32 inputs.

Tolerance: relative 1e-6 per entry, exactly 0 where the oracle gives 0.  Derived, not measured: with exact neighbours the fp32
result differs from float64 only by the rounding of three differences, three squares, two adds, twice more for the mean - under
8 * 2^-24 = 4.8e-7 relative - and the mean of the three smallest distances is continuous in which neighbour wins a tie.  A missed
neighbour shows up orders of magnitude above that."""
import functools
import math

import numpy as np
import pytest
import torch

import mapping_reference as MR

pytestmark = pytest.mark.gpu
REL = 1e-6
BOX = 64                      # GSR_KNN_BOX of csrc/knn.hip


def check(points, label=""):
    from simple_knn._C import distCUDA2
    pts = points.float().contiguous()
    got = distCUDA2(pts.cuda()).cpu().double()
    want = MR.knn_dist2_bruteforce(pts, device="cuda")
    assert got.shape == want.shape
    zero = want == 0
    err = ((got - want).abs() / want.clamp_min(1e-300))[~zero]
    print(f"knn {label}: P = {pts.shape[0]}, zeros {int(zero.sum())}, max rel err {float(err.max()) if err.numel() else 0.0:.3e}")
    assert bool((got[zero] == 0).all())
    assert err.numel() == 0 or float(err.max()) <= REL, float(err.max())
    return got


def gen(seed):
    return torch.Generator().manual_seed(seed)


def test_bruteforce_is_the_same_on_both_devices():
    pts = torch.rand(3000, 3, generator=gen(0))
    a, b = MR.knn_dist2_bruteforce(pts), MR.knn_dist2_bruteforce(pts, device="cuda")
    assert float(((a - b).abs() / a).max()) < 1e-14


def test_uniform():
    check(torch.rand(20000, 3, generator=gen(1)) * 2.6 - 1.3, "uniform")


def test_clusters():
    g = gen(2)
    centres = torch.rand(50, 3, generator=g) * 10
    pts = centres[torch.randint(0, 50, (20000,), generator=g)] + 1e-3 * torch.randn(20000, 3, generator=g)
    check(pts, "50 tight clusters")


def test_plane_and_line():
    g = gen(3)
    plane = torch.rand(20000, 3, generator=g)
    plane[:, 2] = 0.25                                   # Morton codes collapse on one axis
    check(plane, "plane")
    line = torch.zeros(15000, 3)
    line[:, 1] = torch.rand(15000, generator=g) * 7 - 2  # ... and on two
    check(line, "line")


def test_exact_duplicates():
    g = gen(4)
    pts = torch.rand(20000, 3, generator=g)
    pts[18000:] = pts[torch.randint(0, 18000, (2000,), generator=g)]      # 10 % exact copies
    pts[:40] = pts[0]                                                      # and one point 40 times: zeros in the result
    got = check(pts[torch.randperm(20000, generator=g)], "10 % duplicates")
    assert int((got == 0).sum()) >= 40


def test_far_from_the_origin():
    check(1000.0 + 0.5 * torch.rand(20000, 3, generator=gen(5)), "[1000, 1000.5]^3")


@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, BOX - 1, BOX, BOX + 1, BOX * BOX - 1, BOX * BOX + 1])
def test_small_sets(P):
    got = check(torch.rand(P, 3, generator=gen(100 + P)), f"P = {P}")
    assert bool(torch.isfinite(got).all())
    if P == 1:
        assert got.tolist() == [0.0]


def sheet_points(H, W, seed=0):
    """>= 200 k points back-projected from a synthetic depth image: a 2-D sheet in 3-D."""
    from scene_utils import fibonacci_cameras
    cam = fibonacci_cameras(3, W, H, seed=seed)[0]
    depth = MR.depth_sheet(H, W, seed=seed)
    xyz, _, _ = MR.unproject_reference(cam, np.zeros((3, H, W), dtype=np.float32), depth)
    return torch.tensor(xyz, dtype=torch.float32)


def test_depth_sheet_200k():
    pts = sheet_points(400, 512, seed=6)
    assert pts.shape[0] >= 200000
    check(pts, "depth sheet")


def test_first_query_is_the_tail_and_runs_repeat_bit_for_bit():
    from simple_knn._C import knn_dist2
    g = gen(7)
    a = (torch.rand(30000, 3, generator=g) * 2.6 - 1.3).cuda()
    b = sheet_points(60, 80, seed=8).cuda() * 0.4
    both = torch.cat([a, b])
    full, full2 = knn_dist2(both), knn_dist2(both)
    tail, tail2 = knn_dist2(both, first_query=a.shape[0]), knn_dist2(both, first_query=a.shape[0])
    assert tail.shape[0] == b.shape[0]
    assert torch.equal(full, full2) and torch.equal(tail, tail2)
    assert torch.equal(full[a.shape[0]:], tail)
    one = knn_dist2(both, first_query=both.shape[0] - 1)
    assert torch.equal(one, full[-1:])
    want = MR.knn_dist2_bruteforce(both, first_query=a.shape[0], device="cuda")
    assert float(((tail.cpu().double() - want).abs() / want).max()) <= REL


def test_non_finite_rows_do_not_disturb_the_finite_ones():
    """The call returns (no hang, no fault); rows with a non-finite coordinate are unspecified, the others see the finite rows."""
    from simple_knn._C import distCUDA2
    g = gen(9)
    pts = torch.rand(5000, 3, generator=g)
    bad = torch.randperm(5000, generator=g)[:60]
    pts[bad[:20], 0] = float("nan")
    pts[bad[20:40], 1] = float("inf")
    pts[bad[40:], 2] = float("-inf")
    got = distCUDA2(pts.cuda()).cpu().double()
    torch.cuda.synchronize()
    ok = torch.ones(5000, dtype=torch.bool)
    ok[bad] = False
    want = MR.knn_dist2_bruteforce(pts[ok], device="cuda")
    assert float(((got[ok] - want).abs() / want).max()) <= REL


# ---- the sweep's LDS staging loop in its second round (csrc/knn_common.h knn_sweep, 256 super-boxes per round) -----------------
STAGED = 256 * BOX * BOX + 1      # the smallest cloud with 257 super-boxes (tests/test_registration_gpu.py uses it as a target)
TAIL = 600


@functools.lru_cache(maxsize=None)
def staged_cloud():
    """-> (points on the device, the row sorted last).  Super-box 257 - the only one staged in round two - holds ONE point, the
    row sorted last, and only rows next to it depend on that round: the rows of the bounding box's top corner (every coordinate
    > 15 / 16, some 256 of them), which it lies in, are moved to the END of the cloud, behind a random remainder, so that the
    last TAIL rows are queries around it."""
    pts = torch.rand(STAGED, 3, generator=gen(31))
    corner = (pts > 1 - 1 / 16).all(dim=1)
    assert 0 < int(corner.sum()) <= TAIL - 100
    pts = torch.cat([pts[~corner], pts[corner]])
    last = MR.last_sorted_row(pts.numpy())
    assert last >= STAGED - int(corner.sum())
    return pts.cuda(), last


def held(got, want, label):
    """`check`'s comparison on given rows: got float32, want float64, same shape"""
    got = got.cpu().double()
    zero = want == 0
    err = ((got - want).abs() / want.clamp_min(1e-300))[~zero]
    print(f"knn {label}: {tuple(got.shape)}, zeros {int(zero.sum())}, max rel err {float(err.max()) if err.numel() else 0.0:.3e}")
    assert got.shape == want.shape and bool((got[zero] == 0).all())
    assert err.numel() == 0 or float(err.max()) <= REL, float(err.max())


def tail_bruteforce(pts, last):
    """float64 [TAIL, 3]: the three smallest d2 of the last TAIL rows, as knn_dist2_bruteforce forms them; asserts that the row
    sorted last is one of the three nearest of some OTHER queried row - an answer that only the second round can give"""
    x = pts.double()
    rows = torch.arange(STAGED - TAIL, STAGED, device="cuda")
    d = torch.zeros((TAIL, STAGED), dtype=torch.float64, device="cuda")
    for a in range(3):
        d += (x[rows, a:a + 1] - x[None, :, a]) ** 2
    d[torch.arange(TAIL, device="cuda"), rows] = math.inf                    # the row itself
    top = torch.topk(d, 3, dim=1, largest=False, sorted=True)
    users = int((top.indices == last).any(dim=1).sum())
    print(f"knn 1M + 1: the row sorted last is among the three nearest of {users} queried rows")
    assert users >= 1
    return top.values.cpu()


def test_dist2_staging_loop_second_round():
    from simple_knn._C import knn_dist2
    pts, last = staged_cloud()
    got = knn_dist2(pts, first_query=STAGED - TAIL)
    held(got, tail_bruteforce(pts, last).sum(dim=1) / 3, "dist2, 1M + 1, the last 600 rows")
    held(got, MR.knn_dist2_bruteforce(pts, first_query=STAGED - TAIL, device="cuda"), "dist2, 1M + 1, the file's brute force")


def test_knn_k_staging_loop_second_round():
    from simple_knn._C import knn_k
    pts, last = staged_cloud()
    held(knn_k(pts, 3)[STAGED - TAIL:], tail_bruteforce(pts, last), "knn_k(3), 1M + 1, the last 600 rows")
