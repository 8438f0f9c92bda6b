"""gsr_color_gradient on the device (csrc/colored.hip) against the float64 restatement of tests/colored_reference.py.

Bounds.  count and status: exact - tests/test_colored_cpu.py shows, for these clouds and on every row, that the float32 membership
is the float64 one and that no row's pivots come near the threshold of status 2.  Gradient, per component: kappa_i 2^-40 |g_i| +
2^-22 max|g_i| with kappa_i the reference's condition number of the row's 3 x 3 matrix - two float64 solves of it from sums taken
in another order, and one rounding to float32; rows with kappa_i > 1e8 are left out (at most 2 % of a cloud, shown there too).
Rows of status 1 and 2 are exactly zero, masked rows NaN."""
import functools

import numpy as np
import pytest
import torch

import colored_reference as CR
import normals_reference as NR
import scene_utils as S

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def case(kind):
    pts, cols, nrm = CR.gradient_cloud(kind)
    return pts, cols, nrm, [CR.gradient(pts, cols, nrm, r, nn) for r, nn in CR.gradient_combos(kind)]


def check(got, ref, label, rows=None):
    g, count, status = (t.cpu().numpy() for t in got)
    if rows is not None:
        g, count, status = g[rows], count[rows], status[rows]
    P = ref["count"].shape[0]
    assert g.dtype == np.float32 and g.shape == (P, 3) and count.dtype == np.int32 and status.dtype == np.uint8, label
    assert np.array_equal(count, ref["count"]), (label, int((count != ref["count"]).sum()))
    assert np.array_equal(status, ref["status"]), (label, int((status != ref["status"]).sum()))
    assert np.isnan(g[status == 3]).all() and (g[(status == 1) | (status == 2)] == 0).all(), label
    solved = status == 0
    held = solved & (ref["cond"] <= CR.KAPPA_MAX)
    assert (solved & ~held).sum() <= CR.LEFT_OUT_MAX * P, label
    r = ref["gradient"][held]
    bound = ref["cond"][held] * 2.0 ** -40 * np.linalg.norm(r, axis=1) + 2.0 ** -22 * np.abs(r).max(axis=1)
    err = np.abs(g[held].astype(np.float64) - r)
    worst = float((err / bound[:, None]).max(initial=0.0))
    print(f"{label}: status {np.bincount(status, minlength=4).tolist()}, held {int(held.sum())}, worst error / bound {worst:.3g}, "
          f"max error {err.max(initial=0.0):.3g}")
    assert np.isfinite(g[solved]).all() and (err <= bound[:, None]).all(), (label, worst)


@pytest.mark.parametrize("kind", list(CR.GRADIENT_SIZES))
def test_gradients_against_the_reference(kind):
    pts, cols, nrm, refs = case(kind)
    d, c, n = dev(pts), dev(cols), dev(nrm)
    for (radius, nn), ref in zip(CR.gradient_combos(kind), refs):
        check(S.estimate_color_gradients(d, c, n, radius, nn, return_stats=True), ref, f"{kind} P={pts.shape[0]} radius={radius:.4g} "
                                                                                      f"max_nn={nn}")
    radius, nn = CR.gradient_combos(kind)[2]
    only = S.estimate_color_gradients(d, c, n, radius, nn)
    assert torch.equal(bits(only), bits(S.estimate_color_gradients(d, c, n, radius, nn, return_stats=True)[0]))


def test_runs_are_bit_identical_and_simple_knn_is_the_same_call():
    import simple_knn
    for kind in ("duplicates", "clusters", "lattice"):
        pts, cols, nrm, _ = case(kind)
        for radius, nn in CR.gradient_combos(kind)[1:3]:
            a = S.estimate_color_gradients(dev(pts), dev(cols), dev(nrm), radius, nn, return_stats=True)
            b = simple_knn.estimate_color_gradients(dev(pts), dev(cols), dev(nrm), radius, nn, return_stats=True)
            assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), (kind, nn)


def test_masked_rows_get_nan_and_change_no_other_row():
    """rows whose point, colour or normal is not finite, placed ON rows of the cloud (they would be everybody's nearest neighbour):
    NaN, count 0, status 3 - and the other rows' bits are those of the cloud without them"""
    pts, cols, nrm, _ = case("plane")
    P = pts.shape[0]
    at = np.arange(0, 300, 10)
    jp, jc, jn = pts[at].copy(), cols[at].copy(), nrm[at].copy()
    jp[0:10, 1] = np.inf
    jp[3] = np.nan
    jc[10:20, 2] = np.nan
    jc[13] = -np.inf
    jn[20:30, 0] = np.nan
    jn[23] = np.inf
    both = [np.concatenate(x) for x in ((pts, jp), (cols, jc), (nrm, jn))]
    for radius, nn in ((NR.RADIUS, 30), (CR.INF, 4), (CR.INF, 33)):
        clean = S.estimate_color_gradients(dev(pts), dev(cols), dev(nrm), radius, nn, return_stats=True)
        g, count, status = S.estimate_color_gradients(*(dev(x) for x in both), radius, nn, return_stats=True)
        for x, y in zip(clean, (g, count, status)):
            assert torch.equal(bits(x) if x.dtype == torch.float32 else x, bits(y[:P]) if y.dtype == torch.float32 else y[:P])
        assert bool(torch.isnan(g[P:]).all()) and count[P:].tolist() == [0] * 30 and status[P:].tolist() == [3] * 30
        check((g, count, status), CR.gradient(*both, radius, nn), f"masked rows radius={radius:.4g} max_nn={nn}")
    # masked rows INSIDE the cloud: their neighbours lose them
    pts2, cols2, nrm2 = pts.copy(), cols.copy(), nrm.copy()
    pts2[5, 0], cols2[17, 1], nrm2[29] = np.nan, np.inf, np.nan
    ref = CR.gradient(pts2, cols2, nrm2, NR.RADIUS, 30)
    full = CR.gradient(pts, cols, nrm, NR.RADIUS, 30)
    assert (ref["count"] < full["count"]).sum() >= 20          # rows that had one of the three as a member
    check(S.estimate_color_gradients(dev(pts2), dev(cols2), dev(nrm2), NR.RADIUS, 30, return_stats=True), ref, "masked inside")
    g, count, status = S.estimate_color_gradients(dev(jp[:4]), dev(jc[:4]), dev(jn[:4]), CR.INF, 4, return_stats=True)
    assert bool(torch.isnan(g).all()) and count.tolist() == [0] * 4 and status.tolist() == [3] * 4


def test_fewer_than_four_rows_and_collinear_rows_give_zero():
    for P in (1, 2, 3):
        p = torch.rand(P, 3).cuda()
        g, count, status = S.estimate_color_gradients(p, torch.rand(P, 3).cuda(), torch.tensor([[0.0, 0.0, 1.0]] * P).cuda(), CR.INF, 4,
                                                      return_stats=True)
        assert g.tolist() == [[0.0] * 3] * P and count.tolist() == [P] * P and status.tolist() == [1] * P
    # four rows: solved from the three others
    quad = np.float32([[0, 0, 0], [0.125, 0, 0], [0, 0.125, 0], [0.125, 0.25, 0]])
    nrm = np.tile(np.float32([0, 0, 1]), (4, 1))
    cols = np.repeat((quad @ np.float32([0.5, -0.25, 0]) + np.float32(0.5))[:, None], 3, axis=1)
    ref = CR.gradient(quad, cols, nrm, CR.INF, 4)
    assert (ref["status"] == 0).all() and np.abs(ref["gradient"] - [0.5, -0.25, 0]).max() <= 1e-12
    check(S.estimate_color_gradients(dev(quad), dev(cols), dev(nrm), CR.INF, 4, return_stats=True), ref, "four rows")
    # rows on one line, the normal across it: the direction across the line in the tangent plane is not fixed - an exact zero pivot
    line = np.stack([np.arange(9) / 8.0, np.zeros(9), np.zeros(9)], axis=1).astype(np.float32)
    nrm = np.tile(np.float32([0, 0, 1]), (9, 1))
    cols = CR.texture(line, 2.0)
    ref = CR.gradient(line, cols, nrm, CR.INF, 5)
    assert (ref["status"] == 2).all()
    got = S.estimate_color_gradients(dev(line), dev(cols), dev(nrm), CR.INF, 5, return_stats=True)
    check(got, ref, "collinear")
    assert got[0].tolist() == [[0.0] * 3] * 9


def test_staging_loop_second_round():
    """P = 256 * 4096 + 1: 257 super-boxes, so both sweeps of k_color_gradient stage their AABBs through LDS twice (knn_sweep,
    csrc/knn_common.h).  The only super-box of round two holds ONE point, the row sorted last, and only rows next to it depend on
    that round: besides 200 sampled rows, every row of the bounding box's top corner, which that row lies in, is checked, and the
    row must be a member of another checked row's neighbourhood.  Membership by brute force on those rows alone, as
    tests/test_normals_gpu.py does it, under the same precondition; the gradient from those members in float64 on the host."""
    import mapping_reference as MR
    P, nn = 256 * 4096 + 1, 9
    radius = 0.0125
    rng = np.random.default_rng(53)
    pts = rng.random((P, 3), dtype=np.float32)
    cols = rng.random((P, 3), dtype=np.float32)
    nrm = rng.standard_normal((P, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    last = MR.last_sorted_row(pts)
    corner = np.flatnonzero((pts > 1 - 1 / 16).all(axis=1))
    assert last in corner and corner.size < 400
    rows_np = np.union1d(rng.choice(P, 200, replace=False), corner)
    rows = torch.from_numpy(rows_np).cuda()
    R = rows.numel()
    d = dev(pts)
    g, count, status = S.estimate_color_gradients(d, dev(cols), dev(nrm), radius, nn, return_stats=True)
    r2 = NR.radius2(radius)
    delta = (d[None, :, :] - d[rows, None, :]).double()                               # float32 differences, promoted
    d2 = (delta[..., 0] * delta[..., 0] + delta[..., 1] * delta[..., 1]) + delta[..., 2] * delta[..., 2]
    del delta
    d2[torch.arange(R, device="cuda"), rows] = NR.INF                                 # the row itself
    small = torch.topk(d2, nn, dim=1, largest=False, sorted=True).values
    bound = torch.clamp(small[:, nn - 2], max=r2)
    member = d2 <= bound[:, None]
    inc = torch.where(member, d2, torch.full_like(d2, -NR.INF)).max(dim=1).values
    exc = torch.where(~member, d2, torch.full_like(d2, NR.INF)).min(dim=1).values
    margin = torch.minimum((exc - inc) / exc, torch.minimum((r2 - inc).abs() / r2, (exc - r2).abs() / r2))
    assert float(margin.min()) > 1e-6
    assert int(member[:, last].sum()) >= 1
    pairs = member.nonzero().cpu().numpy()
    del d2, member
    want_count = 1 + np.bincount(pairs[:, 0], minlength=R)
    assert want_count.min() < nn and (want_count == nn).sum() >= 20      # the radius cuts some neighbourhoods, max_nn others
    assert np.array_equal(count[rows].cpu().numpy(), want_count)
    n64, I = nrm.astype(np.float64), CR.intensity(cols)
    got, st = g[rows].cpu().numpy().astype(np.float64), status[rows].cpu().numpy()
    held = 0
    for k in range(R):
        i, mem = rows_np[k], pairs[pairs[:, 0] == k, 1]
        if want_count[k] < 4:
            assert st[k] == 1 and (got[k] == 0).all()
            continue
        delta = (pts[mem] - pts[i]).astype(np.float64)
        u = delta - (delta @ n64[i])[:, None] * n64[i]
        M = u.T @ u + (mem.size ** 2) * np.outer(n64[i], n64[i])
        ratio = CR._ldl_pivot_ratio(M[None])[0]
        assert ratio > 1e-9 and st[k] == 0, (k, ratio, st[k])
        kappa = np.linalg.cond(M)
        if kappa > CR.KAPPA_MAX:
            continue
        want = np.linalg.solve(M, u.T @ (I[mem] - I[i]))
        assert (np.abs(got[k] - want) <= kappa * 2.0 ** -40 * np.linalg.norm(want) + 2.0 ** -22 * np.abs(want).max()).all(), k
        held += 1
    print(f"colour gradient 1M + 1: {R} rows, counts {np.bincount(want_count, minlength=nn + 1).tolist()}, {held} gradients held")
    assert held >= 0.9 * (want_count >= 4).sum()
