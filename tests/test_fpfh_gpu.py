"""gsr_compute_fpfh on the device (csrc/features.hip) against the float64 restatement of tests/global_registration_reference.py.

Bounds.  count and spfh_counts: exact - tests/test_global_registration_cpu.py shows, for these seeds and on every pair of every
neighbourhood, that membership and every bin are the same in any float64 arithmetic.  fpfh: 1e-4 absolute on every row - values
lie in [0, 200] and one float32 rounding of a float64 result is at most 200 x 2^-24 = 1.2e-5; every non-empty block sums to 200
within the same bar."""
import functools

import numpy as np
import pytest
import torch

import global_registration_reference as G
import scene_utils as S

pytestmark = pytest.mark.gpu
BAR = 1e-4


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def case(kind, P):
    pts, nrm = G.cloud(kind, P)
    return pts, nrm, G.analyse(pts, nrm, G.combos(kind))


def check(a, got, label):
    fpfh, counts, count = (t.cpu().numpy() for t in got)
    P = a["count"].shape[0]
    assert fpfh.dtype == np.float32 and fpfh.shape == (P, 33) and counts.dtype == np.int32 and counts.shape == (P, 33) and \
        count.dtype == np.int32 and count.shape == (P,), label
    assert np.array_equal(count, a["count"]), (label, int((count != a["count"]).sum()))
    assert np.array_equal(counts, a["counts"]), (label, int((counts != a["counts"]).any(axis=1).sum()))
    ok = a["finite"]
    assert np.isnan(fpfh[~ok]).all() and np.isfinite(fpfh[ok]).all(), label
    err = np.abs(fpfh[ok].astype(np.float64) - a["fpfh"][ok]).max(initial=0.0)
    live = ok & (a["m"] > 0)
    sums = np.abs(fpfh[live].astype(np.float64).reshape(-1, 3, 11).sum(axis=2) - 200.0).max(initial=0.0)
    print(f"{label}: rows {int(ok.sum())}, m = 0 on {int((ok & (a['m'] == 0)).sum())}, err {err:.3g}, block sums off by {sums:.3g}")
    assert err <= BAR, (label, err)
    assert sums <= BAR, (label, sums)
    assert (fpfh[ok & (a["m"] == 0)] == 0).all(), label


@pytest.mark.parametrize("P", G.SIZES)
@pytest.mark.parametrize("kind", list(G.CLOUDS))
def test_fpfh_against_the_reference(kind, P):
    pts, nrm, refs = case(kind, P)
    d, n = dev(pts), dev(nrm)
    for (radius, nn), a in zip(G.combos(kind), refs):
        check(a, S.compute_fpfh_feature(d, n, radius, nn, return_stats=True), f"{kind} P={P} radius={radius:.4g} max_nn={nn}")


def test_runs_are_bit_identical_and_simple_knn_is_the_same_call():
    import simple_knn
    for kind, radius, nn in (("twice", G.RADIUS, 0), ("far", G.RADIUS, 30), ("sphere", G.INF, 4), ("lattice", G.INF, 9),
                             ("lattice", G.INF, 17), ("edge", G.INF, 33)):
        pts, nrm = (dev(x) for x in G.cloud(kind, 5000))
        a = S.compute_fpfh_feature(pts, nrm, radius, nn, return_stats=True)
        b = simple_knn.compute_fpfh(pts, nrm, radius, nn, return_stats=True)
        for x, y in zip(a, b):
            assert torch.equal(bits(x), bits(y)), (kind, nn)
        assert torch.equal(bits(a[0]), bits(S.compute_fpfh_feature(pts, nrm, radius, nn)))


def test_non_finite_rows_get_nan_and_change_no_other_row():
    pts, nrm = G.cloud("noisy", 4097)
    junk_p = np.array([[np.nan, 0, 0], [0.3, np.inf, 0.1], [0.3, -0.2, 0.1], [0.31, -0.2, 0.1]], dtype=np.float32)
    junk_n = np.array([[0, 0, 1], [0, 0, 1], [np.nan, 0, 1], [0, -np.inf, 0]], dtype=np.float32)      # a bad point, or a bad normal
    both_p, both_n = np.concatenate([pts, np.repeat(junk_p, 10, axis=0)]), np.concatenate([nrm, np.repeat(junk_n, 10, axis=0)])
    for radius, nn in ((G.RADIUS, 0), (G.INF, 30), (G.RADIUS, 33), (G.INF, 3)):
        clean = S.compute_fpfh_feature(dev(pts), dev(nrm), radius, nn, return_stats=True)
        f, counts, count = S.compute_fpfh_feature(dev(both_p), dev(both_n), radius, nn, return_stats=True)
        for x, y in zip(clean, (f, counts, count)):
            assert torch.equal(bits(x), bits(y[:4097]))
        assert bool(torch.isnan(f[4097:]).all()) and count[4097:].tolist() == [0] * 40 and int(counts[4097:].abs().sum()) == 0
    # rows with a FINITE point far outside the cloud and a bad normal: masked before the structure is built, so neither the bounding
    # box, nor the sort, nor any other row's bits know where they lie
    away_p = np.array([[50, 50, 50], [-80, 3, 0.1], [0.3, -0.2, 1e6]], dtype=np.float32)
    away_n = np.array([[np.nan, 0, 1], [0, np.inf, 0], [0, 0, -np.inf]], dtype=np.float32)
    order = np.random.default_rng(3).permutation(4100)
    mixed_p, mixed_n = np.concatenate([pts, away_p])[order], np.concatenate([nrm, away_n])[order]
    for radius, nn in ((G.RADIUS, 0), (G.INF, 30)):
        clean = S.compute_fpfh_feature(dev(pts[order[order < 4097]]), dev(nrm[order[order < 4097]]), radius, nn, return_stats=True)
        f, counts, count = S.compute_fpfh_feature(dev(mixed_p), dev(mixed_n), radius, nn, return_stats=True)
        keep = torch.from_numpy(np.flatnonzero(order < 4097)).cuda()
        for x, y in zip(clean, (f, counts, count)):
            assert torch.equal(bits(x), bits(y[keep]))
        assert bool(torch.isnan(f[torch.from_numpy(np.flatnonzero(order >= 4097)).cuda()]).all())
    f, counts, count = S.compute_fpfh_feature(dev(junk_p), dev(junk_n), 1.0, 0, return_stats=True)
    assert bool(torch.isnan(f).all()) and count.tolist() == [0] * 4


def test_a_shuffled_cloud_gives_every_point_its_feature():
    for kind, radius, nn in (("sphere", G.RADIUS, 0), ("twice", G.RADIUS, 30), ("lattice", G.INF, 10)):
        pts, nrm = G.cloud(kind, 5000)
        perm = np.random.default_rng(0).permutation(5000)
        f, counts, count = S.compute_fpfh_feature(dev(pts), dev(nrm), radius, nn, return_stats=True)
        g, counts2, count2 = S.compute_fpfh_feature(dev(pts[perm]), dev(nrm[perm]), radius, nn, return_stats=True)
        p = torch.from_numpy(perm).cuda()
        assert torch.equal(counts[p], counts2) and torch.equal(count[p], count2)
        # two float32 roundings of sums taken in different orders (float64: 1e-13): within the bar of either
        assert float((f[p].double() - g.double()).abs().max()) <= BAR


def test_empty_and_tiny_clouds():
    z = torch.zeros((0, 3), device="cuda")
    assert tuple(S.compute_fpfh_feature(z, z, 0.1).shape) == (0, 33)
    f, counts, count = S.compute_fpfh_feature(torch.rand(1, 3).cuda(), torch.rand(1, 3).cuda(), 0.5, 0, return_stats=True)
    assert f.tolist() == [[0.0] * 33] and count.tolist() == [1] and int(counts.sum()) == 0


def test_staging_loop_second_round_counts():
    """P = 64 * 4096 + 1: the smallest cloud with 65 super-boxes, so k_fpfh_spfh and k_fpfh_sum - one wave per workgroup - stage the
    AABBs through LDS twice (knn_sweep<64>, csrc/knn_common.h).  The only super-box of round two holds ONE point, the row sorted
    last, and only rows next to it depend on that round: besides 200 sampled rows, every row of the bounding box's top corner
    (all coordinates > 15 / 16, some 64 rows), which that row lies in, is checked, and the row must be a member of other checked
    rows' neighbourhoods.  count against the brute force of G.analyse on those rows alone: float32 differences promoted, d2 =
    (dx dx + dy dy) + dz dz in float64, members d2 <= r2.  Exact, given the precondition asserted below: no d2 within 1e-6
    (relative) of r2, five times what the float32 and the float64 d2 can differ by."""
    import mapping_reference as MR
    P, radius = 64 * 4096 + 1, 0.03                   # unit cube: 29.6 other rows within the radius on average
    rng = np.random.default_rng(52)
    pts = rng.random((P, 3), dtype=np.float32)
    nrm = rng.standard_normal((P, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    last = MR.last_sorted_row(pts)
    corner = np.flatnonzero((pts > 1 - 1 / 16).all(axis=1))
    assert last in corner and corner.size < 200
    rows = torch.from_numpy(np.union1d(rng.choice(P, 200, replace=False), corner)).cuda()
    R = rows.numel()
    d = dev(pts)
    fpfh, _, count = S.compute_fpfh_feature(d, dev(nrm), radius, 0, return_stats=True)
    r2 = G.NR.radius2(radius)
    delta = (d[None, :, :] - d[rows, None, :]).double()                               # float32 differences, promoted
    d2 = (delta[..., 0] * delta[..., 0] + delta[..., 1] * delta[..., 1]) + delta[..., 2] * delta[..., 2]
    d2[torch.arange(R, device="cuda"), rows] = G.INF                                  # the row itself
    assert float(((d2 - r2).abs() / r2).min()) > 1e-6
    member = d2 <= r2
    want = 1 + member.sum(dim=1)
    users = int(member[:, last].sum())
    print(f"fpfh 256k + 1: {R} rows, counts {int(want.min())} .. {int(want.max())}, mean {float(want.double().mean()):.1f}, the "
          f"row sorted last is a member of {users} checked neighbourhoods")
    assert users >= 1
    assert 15 <= float(want.double().mean()) <= 40
    assert torch.equal(count[rows].long(), want)
    assert bool(torch.isfinite(fpfh[rows]).all())
