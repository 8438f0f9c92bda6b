"""The generalized ICP update on the device (csrc/gicp.hip gsr_icp_update_generalized) against the float64 restatement of
tests/gicp_reference.py; the twin of tests/test_icp_plane_gpu.py::test_update_against_the_reference.

Bounds.  n exact.  sum |d|^2, and fitness / RMSE formed from it: 1e-12 relative - float64 sums of at most 65 537 non-negative terms
in another order.  sum d^T W d: a term's error is about cond(M) 2^-52 <= 1e3 x 2.2e-16 (tests/test_gicp_reference_cpu.py shows
cond(M) <= 1 / epsilon for every case), which with two decades for the order gives 1e-11 relative; measured on the MI355X it is
at most 1.42e-15 over the eight cases (the terms are positive and their errors do not line up), so the bound held here is
SUM_W_REL = 1e-13 - two decades above the measurement, two below the estimate.  Transform: the
largest displacement of a source row between the kernel's T and the reference's <= 1e-9 x the cloud's extent; the same file shows
cond(J^T W J) <= 1e6, so two float64 solves of it agree to 1e-10.  dT's rotation block: orthonormal, determinant +1, to 1e-14."""
import numpy as np
import pytest
import torch

import gicp_reference as G
import normals_reference as NR
import scene_utils as S

pytestmark = pytest.mark.gpu
SUM_W_REL = 1e-13


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def extent(points):
    return float(np.ptp(np.asarray(points, dtype=np.float64), axis=0).max())


def bits64(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint64)


def rel(a, b):
    return abs(a - b) / abs(b) if b else abs(a)


def run(src, scov, tgt, tcov, corr, T0):
    T, stats = S.gicp_update(dev(src), dev(scov), dev(tgt), dev(tcov), dev(corr), None if T0 is None else torch.from_numpy(T0))
    return T.cpu().numpy(), stats.tolist()


@pytest.mark.parametrize("offset", G.UPDATE_OFFSETS)
@pytest.mark.parametrize("Ps", G.UPDATE_SIZES)
def test_update_against_the_reference(Ps, offset):
    case = G.update_case(Ps, offset)
    src, scov, tgt, tcov, corr, T0 = case
    ref = G.generalized_update(*case)
    assert ref["status"] == 0
    T, st = run(*case)
    err = NR.displacement(T, ref["T"], src)
    print(f"generalized update Ps={Ps} offset={offset}: n={ref['n']} displacement {err:.3g} (bound {1e-9 * extent(tgt):.3g}), "
          f"sum_d2 rel {rel(st[4], ref['sum_d2']):.3g}, sum_w rel {rel(st[5], ref['sum_w']):.3g}")
    assert st[0] == ref["n"] and st[3] == 0.0 and st[6] == 0.0 and st[7] == 0.0
    assert rel(st[1], ref["fitness"]) <= 1e-12 and rel(st[2], ref["rmse"]) <= 1e-12
    assert rel(st[4], ref["sum_d2"]) <= 1e-12 and rel(st[5], ref["sum_w"]) <= SUM_W_REL
    assert err <= 1e-9 * extent(tgt)
    assert T[3].tolist() == [0.0, 0.0, 0.0, 1.0]
    dR = (T @ np.linalg.inv(T0))[:3, :3]
    # (T0 itself is orthonormal to 1e-16; the product with its inverse adds a few units of that)
    assert np.abs(dR @ dR.T - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(dR) - 1.0) <= 1e-14
    # two runs: the same bits
    T2, st2 = run(*case)
    assert np.array_equal(T.view(np.uint64), T2.view(np.uint64)) and np.array_equal(np.float64(st).view(np.uint64),
                                                                                   np.float64(st2).view(np.uint64))


def test_update_status_one_leaves_T():
    src, scov, tgt, tcov, corr, T0 = G.update_case(256, 0.0)
    keep = np.flatnonzero(corr >= 0)[:5]
    few = np.full_like(corr, -1)
    few[keep] = corr[keep]
    for c, n in ((few, 5), (np.full_like(corr, -1), 0), (np.full_like(corr, tgt.shape[0]), 0)):      # (a row the target lacks)
        T, stats = S.gicp_update(dev(src), dev(scov), dev(tgt), dev(tcov), dev(c), torch.from_numpy(T0))
        st = stats.tolist()
        assert np.array_equal(bits64(T), T0.view(np.uint64)) and st[0] == n and st[3] == 1.0 and st[1] == n / 256
        if n:
            ref = G.generalized_update(src, scov, tgt, tcov, c, T0)
            assert rel(st[2], ref["rmse"]) <= 1e-12 and rel(st[5], ref["sum_w"]) <= SUM_W_REL


def test_non_finite_covariances_on_either_side_drop_their_rows_only():
    src, scov, tgt, tcov, corr, T0 = G.update_case(257, 0.0)
    bad_t, bad_s = tcov.copy(), scov.copy()
    hit = np.unique(corr[corr >= 0])[::7]
    bad_t[hit[0::3], 0] = np.nan
    bad_t[hit[1::3], 4] = np.inf
    bad_t[hit[2::3]] = -np.inf
    bad_s[5::11, 2] = np.nan
    bad_s[7::13] = np.inf
    full = G.generalized_update(src, scov, tgt, tcov, corr, T0)
    seen = []
    for sc, tc in ((scov, bad_t), (bad_s, tcov), (bad_s, bad_t)):
        ref = G.generalized_update(src, sc, tgt, tc, corr, T0)
        assert 6 <= ref["n"] < full["n"] and ref["status"] == 0
        seen.append(ref["n"])
        T, st = run(src, sc, tgt, tc, corr, T0)
        assert st[0] == ref["n"] and st[3] == 0.0 and rel(st[4], ref["sum_d2"]) <= 1e-12 and rel(st[5], ref["sum_w"]) <= SUM_W_REL
        assert NR.displacement(T, ref["T"], src) <= 1e-9 * extent(tgt)
    assert seen[2] < min(seen[:2])


def test_a_row_with_a_singular_combined_covariance_is_dropped():
    src, scov, tgt, tcov, corr, T0 = G.update_case(257, 0.0)
    zs, zt = scov.copy(), tcov.copy()
    rows = np.flatnonzero(corr >= 0)[::9]
    zs[rows] = 0.0
    zt[corr[rows]] = 0.0                                         # (other source rows that meet these target rows keep their own Sigma_s)
    ref = G.generalized_update(src, zs, tgt, zt, corr, T0)
    full = G.generalized_update(src, scov, tgt, tcov, corr, T0)
    assert ref["n"] == full["n"] - rows.size and ref["status"] == 0
    T, st = run(src, zs, tgt, zt, corr, T0)
    assert st[0] == ref["n"] and st[3] == 0.0 and rel(st[4], ref["sum_d2"]) <= 1e-12 and rel(st[5], ref["sum_w"]) <= SUM_W_REL
    assert NR.displacement(T, ref["T"], src) <= 1e-9 * extent(tgt)
    # every row singular: nothing to solve, T stays
    T, st = run(src, np.zeros_like(scov), tgt, np.zeros_like(tcov), corr, T0)
    assert st[0] == 0 and st[3] == 1.0 and np.array_equal(T.view(np.uint64), T0.view(np.uint64))
    # an indefinite M (negative determinant) is dropped as well
    neg = tcov.copy()
    neg[corr[rows]] = np.float32([-3, 0, 0, 1, 0, 1])
    ref = G.generalized_update(src, scov, tgt, neg, corr, T0)
    T, st = run(src, scov, tgt, neg, corr, T0)
    assert st[0] == ref["n"] < full["n"] and NR.displacement(T, ref["T"], src) <= 1e-9 * extent(tgt)


def test_a_single_exact_plane_with_isotropic_source_covariances_is_solved():
    """the scene on which the point-to-plane update returns status 2 (tests/test_icp_plane_gpu.py
    test_update_status_two_on_a_single_exact_plane)"""
    case = G.single_plane_case()
    src, scov, tgt, tcov, corr, T0 = case
    nrm = np.tile(np.float32([0, 0, 1]), (500, 1))
    _, plane = S.icp_update(dev(src), dev(tgt), dev(corr), torch.from_numpy(T0), target_normals=dev(nrm))
    assert plane.tolist()[3] == 2.0
    ref = G.generalized_update(*case)
    T, st = run(*case)
    assert st[0] == 300 and st[3] == 0.0
    assert rel(st[2], 0.125) <= 1e-12 and rel(st[5], ref["sum_w"]) <= SUM_W_REL
    assert NR.displacement(T, ref["T"], src) <= 1e-9 * extent(tgt)
    # the step closes the gap along the normal and leaves the rest
    want = T0.copy()
    want[2, 3] -= 0.125
    assert np.abs(T - want).max() <= 1e-12


def test_the_identity_is_the_default_transformation():
    src, scov, tgt, tcov, corr, _ = G.update_case(256, 0.0)
    a, sa = run(src, scov, tgt, tcov, corr, None)
    b, sb = run(src, scov, tgt, tcov, corr, np.eye(4))
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)) and sa == sb
    R = a[:3, :3]
    if sa[3] == 0.0:      # from the identity dT is T itself: no inverse between the kernel's rotations and the check
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(R) - 1.0) <= 1e-14
