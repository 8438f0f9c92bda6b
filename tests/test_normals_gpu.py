"""gsr_estimate_normals on the device (csrc/normals.hip) against the float64 restatement of tests/normals_reference.py.

Bounds.  count: exact - tests/test_normals_cpu.py shows, for these seeds and for every row, that the float32 membership is the
float64 one.  Eigenvalues: 1e-6 of the row's largest (float32 output of float64 arithmetic).  Normals: after aligning the sign,
max-abs component error <= 1e-6 - 2^-24 output rounding plus 1e-15 / gap from the solve - on the rows with
(l1 - l0) / l2 >= 1e-3: the same file shows that this is EVERY row with count >= 3 at max_nn 30 and 33 and on the lattice, and all
but the thin three- and four-row neighbourhoods at max_nn 3 and 4 on the other clouds (NR.WIDE); every other check runs on
every row of every case.  Unit length to 2e-7 (three float32
roundings of a unit vector).  The sign rules are checked where the deciding quantity is more than 1e-3 from zero."""
import functools

import numpy as np
import pytest
import torch

import normals_reference as NR
import scene_utils as S

pytestmark = pytest.mark.gpu
VIEWPOINT = [0.4, 0.3, 2.5]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def case(kind, P):
    pts = NR.cloud(kind, P)
    return pts, NR.analyse(pts, NR.combos(kind))


def check(pts, a, got, label, viewpoint=None):
    n, count, eig = (t.cpu().numpy() for t in got)
    P = pts.shape[0]
    assert n.dtype == np.float32 and n.shape == (P, 3) and count.dtype == np.int32 and count.shape == (P,) and \
        eig.dtype == np.float32 and eig.shape == (P, 3), label
    assert np.array_equal(count, a["count"]), (label, int((count != a["count"]).sum()))
    finite, few = a["finite"], a["finite"] & (a["count"] < 3)
    full = a["finite"] & (a["count"] >= 3)
    assert np.isnan(n[~finite]).all() and np.isnan(eig[~finite]).all(), label
    assert np.array_equal(n[few], np.tile(np.float32([0, 0, 1]), (int(few.sum()), 1))) and (eig[few] == 0).all(), label
    err_e = np.abs(eig[full].astype(np.float64) - a["eig"][full]).max(initial=0.0)
    scale = a["eig"][full][:, 2]
    assert (np.abs(eig[full].astype(np.float64) - a["eig"][full]) <= 1e-6 * scale[:, None]).all(), (label, err_e)
    assert (np.diff(eig[full], axis=1) >= 0).all(), label
    g = n[full].astype(np.float64)
    length = np.abs(np.linalg.norm(g, axis=1) - 1.0).max(initial=0.0)
    assert length <= 2e-7, (label, length)
    with np.errstate(invalid="ignore"):
        shaped = full & (a["gap"] >= NR.GAP)
    ref = a["normal"][shaped]
    g = n[shaped].astype(np.float64)
    aligned = np.where(((g * ref).sum(axis=1) < 0)[:, None], -ref, ref)
    err = np.abs(g - aligned).max(initial=0.0)
    print(f"{label}: rows {int(full.sum())}, normals compared {int(shaped.sum())}, err {err:.3g}, |n| - 1 {length:.3g}, "
          f"eig err {err_e:.3g}")
    assert err <= 1e-6, (label, err)
    want, decider = NR.orient(a["normal"], pts, viewpoint)
    sure = shaped & (np.abs(decider) > 1e-3)
    assert sure.sum() >= 0.9 * shaped.sum(), label
    assert np.abs(n[sure].astype(np.float64) - want[sure]).max(initial=0.0) <= 1e-6, (label, "sign")


@pytest.mark.parametrize("P", NR.SIZES)
@pytest.mark.parametrize("kind", list(NR.CLOUDS))
def test_normals_against_the_reference(kind, P):
    pts, refs = case(kind, P)
    d = dev(pts)
    for (radius, nn), a in zip(NR.combos(kind), refs):
        check(pts, a, S.estimate_normals(d, radius, nn, return_stats=True), f"{kind} P={P} radius={radius:.4g} max_nn={nn}")
    radius, nn = NR.combos(kind)[-1]
    check(pts, refs[-1], S.estimate_normals(d, radius, nn, viewpoint=VIEWPOINT, return_stats=True), f"{kind} P={P} viewpoint",
          viewpoint=VIEWPOINT)
    only = S.estimate_normals(d, radius, nn)
    assert torch.equal(only.view(torch.int32), S.estimate_normals(d, radius, nn, return_stats=True)[0].view(torch.int32))


def test_one_and_two_rows_fall_back():
    for P in (1, 2):
        n, count, eig = S.estimate_normals(torch.rand(P, 3).cuda(), NR.INF, 3, viewpoint=[0, 0, -9], return_stats=True)
        assert n.tolist() == [[0.0, 0.0, 1.0]] * P and count.tolist() == [P] * P and eig.tolist() == [[0.0] * 3] * P


def bits(t):
    return t.contiguous().view(torch.int32)


def test_runs_are_bit_identical_and_simple_knn_is_the_same_call():
    import simple_knn
    for kind, radius, nn in (("duplicates", NR.RADIUS, 30), ("clusters", NR.RADIUS, 3), ("sphere", NR.INF, 4),
                             ("lattice", NR.INF, 9), ("lattice", NR.INF, 17)):
        pts = dev(NR.cloud(kind, 5000))
        a = S.estimate_normals(pts, radius, nn, return_stats=True)
        b = simple_knn.estimate_normals(pts, radius, nn, return_stats=True)
        for x, y in zip(a, b):
            assert torch.equal(bits(x), bits(y)), (kind, nn)


def test_non_finite_rows_get_nan_and_change_no_other_row():
    pts = NR.cloud("plane", 4097)
    junk = np.array([[np.nan, 0, 0], [0.3, np.inf, 0.1], [0.3, -0.2, -np.inf], [np.nan] * 3], dtype=np.float32)
    both = np.concatenate([pts, np.repeat(junk, 10, axis=0)])
    for radius, nn in ((NR.INF, 30), (NR.RADIUS, 33), (NR.RADIUS, 3), (NR.INF, 4)):
        clean = S.estimate_normals(dev(pts), radius, nn, return_stats=True)
        n, count, eig = S.estimate_normals(dev(both), radius, nn, return_stats=True)
        for x, y in zip(clean, (n, count, eig)):
            assert torch.equal(bits(x), bits(y[:4097]))
        assert bool(torch.isnan(n[4097:]).all()) and bool(torch.isnan(eig[4097:]).all()) and count[4097:].tolist() == [0] * 40
    n, count, _ = S.estimate_normals(dev(junk), NR.INF, 3, return_stats=True)
    assert bool(torch.isnan(n).all()) and count.tolist() == [0] * 4


@pytest.mark.parametrize("kind,radius,nn", [("sphere", NR.INF, 30), ("clusters", NR.RADIUS, 33), ("lattice", NR.INF, 3)])
def test_a_shuffled_cloud_gives_every_point_the_same_answer(kind, radius, nn):
    pts = NR.cloud(kind, 5000)
    perm = np.random.default_rng(1).permutation(5000)
    n, count, _ = S.estimate_normals(dev(pts), radius, nn, return_stats=True)
    m, mcount, _ = S.estimate_normals(dev(pts[perm]), radius, nn, return_stats=True)
    assert torch.equal(mcount.cpu(), count.cpu()[perm])
    # (the order of the sums may differ: both lie within 1e-6 of the reference, and the sign rule does not depend on the order)
    full = (count >= 3).cpu().numpy()
    diff = (m.cpu().numpy().astype(np.float64) - n.cpu().numpy()[perm].astype(np.float64))[full[perm]]
    assert np.abs(diff).max() <= 1e-6


def test_staging_loop_second_round_counts():
    """P = 256 * 4096 + 1: 257 super-boxes, so both sweeps of k_normals stage their AABBs through LDS twice (knn_sweep,
    csrc/knn_common.h).  The only super-box of round two holds ONE point, the row sorted last, and only rows next to it depend on
    that round: besides 200 sampled rows, every row of the bounding box's top corner (all coordinates > 15 / 16, some 256 rows),
    which that row lies in, is checked, and the row must be a member of another checked row's neighbourhood.  count against the
    brute force of NR.analyse on those rows alone: float32 differences promoted, d2 in float64, bound = min(r2, d_8), ties at
    the bound all members.  Exact, given the precondition asserted below: what decides membership lies more than 1e-6 (relative)
    apart, five times what the float32 and the float64 d2 can differ by (three roundings of 2^-24)."""
    import mapping_reference as MR
    P, nn = 256 * 4096 + 1, 9
    radius = 0.0125                                   # unit cube: 8.6 other rows within it on average - both cuts decide
    rng = np.random.default_rng(51)
    pts = rng.random((P, 3), dtype=np.float32)
    last = MR.last_sorted_row(pts)
    corner = np.flatnonzero((pts > 1 - 1 / 16).all(axis=1))
    assert last in corner and corner.size < 400
    rows = torch.from_numpy(np.union1d(rng.choice(P, 200, replace=False), corner)).cuda()
    R = rows.numel()
    d = dev(pts)
    _, count, _ = S.estimate_normals(d, radius, nn, return_stats=True)
    r2 = NR.radius2(radius)
    delta = (d[None, :, :] - d[rows, None, :]).double()                               # float32 differences, promoted
    d2 = (delta[..., 0] * delta[..., 0] + delta[..., 1] * delta[..., 1]) + delta[..., 2] * delta[..., 2]
    d2[torch.arange(R, device="cuda"), rows] = NR.INF                                 # the row itself
    small = torch.topk(d2, nn, dim=1, largest=False, sorted=True).values              # d_1 .. d_9
    bound = torch.clamp(small[:, nn - 2], max=r2)
    member = d2 <= bound[:, None]
    want = 1 + member.sum(dim=1)
    inc = torch.where(member, d2, torch.full_like(d2, -NR.INF)).max(dim=1).values
    exc = torch.where(~member, d2, torch.full_like(d2, NR.INF)).min(dim=1).values
    margin = torch.minimum((exc - inc) / exc, torch.minimum((r2 - inc).abs() / r2, (exc - r2).abs() / r2))
    assert float(margin.min()) > 1e-6
    users = int(member[:, last].sum())
    want = want.cpu().numpy()
    print(f"normals 1M + 1: {R} rows, counts {np.bincount(want, minlength=nn + 1).tolist()}, the row sorted last is a member of "
          f"{users} checked neighbourhoods")
    assert users >= 1
    assert want.min() < nn and (want == nn).sum() >= 20      # the radius cuts some neighbourhoods, max_nn others
    assert np.array_equal(count[rows].cpu().numpy(), want)
