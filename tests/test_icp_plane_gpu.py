"""The point-to-plane update and its drivers on the device (csrc/registration.hip gsr_icp_update_plane) against the float64
restatement of tests/normals_reference.py.

Bounds.  n exact.  Sums (sum |q - p|^2, sum r^2, and RMSE / fitness formed from them): 1e-12 relative - float64 sums of at most
65 537 non-negative terms in another order.  Transform: the largest displacement of a source row between the kernel's T and the
reference's <= 1e-9 x the cloud's extent; tests/test_normals_cpu.py shows cond(J^T J) <= 1e6 for every case, so two float64
solves of it agree to 1e-10.  dT's rotation block: orthonormal, determinant +1, to 1e-14 (a product of three exact rotations)."""
import functools

import numpy as np
import pytest
import torch

import normals_reference as NR
import pointcloud_reference as PR
import registration_reference as RR
import scene_utils as S
from scene_utils import NeighborIndex

pytestmark = pytest.mark.gpu


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def extent(points):
    return float(np.ptp(np.asarray(points, dtype=np.float64), axis=0).max())


def bits64(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint64)


def rel(a, b):
    return abs(a - b) / abs(b) if b else abs(a)


@pytest.mark.parametrize("offset", [0.0, 1000.0])
@pytest.mark.parametrize("Ps", [6, 256, 257, 65537])
def test_update_against_the_reference(Ps, offset):
    src, tgt, nrm, T0, corr = NR.update_case(Ps, offset)
    ref = NR.plane_update(src, tgt, nrm, corr, T0)
    assert ref["status"] == 0
    T, stats = S.icp_update(dev(src), dev(tgt), dev(corr), torch.from_numpy(T0), target_normals=dev(nrm))
    T, st = T.cpu().numpy(), stats.tolist()
    err = NR.displacement(T, ref["T"], src)
    print(f"plane update Ps={Ps} offset={offset}: n={ref['n']} displacement {err:.3g} (bound {1e-9 * extent(tgt):.3g}), "
          f"sum_d2 rel {rel(st[4], ref['sum_d2']):.3g}, sum_r2 rel {rel(st[5], ref['sum_r2']):.3g}")
    assert st[0] == ref["n"] and st[3] == 0.0 and st[6] == 0.0 and st[7] == 0.0
    assert rel(st[1], ref["fitness"]) <= 1e-12 and rel(st[2], ref["rmse"]) <= 1e-12
    assert rel(st[4], ref["sum_d2"]) <= 1e-12 and rel(st[5], ref["sum_r2"]) <= 1e-12
    assert err <= 1e-9 * extent(tgt)
    assert T[3].tolist() == [0.0, 0.0, 0.0, 1.0]
    dR = (T @ np.linalg.inv(T0))[:3, :3]
    # (T0 itself is orthonormal to 1e-16; the product with its inverse adds a few units of that)
    assert np.abs(dR @ dR.T - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(dR) - 1.0) <= 1e-14
    # from the identity dT is T itself: no inverse between the kernel's rotations and the check
    corr_id = RR.correspondences(RR.nearest(src, tgt, 6 * NR.SPACING))
    if (corr_id >= 0).sum() >= 6:
        Ti, sti = S.icp_update(dev(src), dev(tgt), dev(corr_id), None, target_normals=dev(nrm))
        if sti.tolist()[3] == 0.0:
            R = Ti.cpu().numpy()[:3, :3]
            assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(R) - 1.0) <= 1e-14


def test_update_status_one_leaves_T():
    src, tgt, nrm, T0, corr = NR.update_case(256, 0.0)
    keep = np.flatnonzero(corr >= 0)[:5]
    few = np.full_like(corr, -1)
    few[keep] = corr[keep]
    for c, n in ((few, 5), (np.full_like(corr, -1), 0), (np.full_like(corr, tgt.shape[0]), 0)):      # (a row the target lacks)
        T, stats = S.icp_update(dev(src), dev(tgt), dev(c), torch.from_numpy(T0), target_normals=dev(nrm))
        st = stats.tolist()
        assert np.array_equal(bits64(T), T0.view(np.uint64)) and st[0] == n and st[3] == 1.0 and st[1] == n / 256
        if n:
            ref = NR.plane_update(src, tgt, nrm, c, T0)
            assert rel(st[2], ref["rmse"]) <= 1e-12 and rel(st[5], ref["sum_r2"]) <= 1e-12


def test_update_status_two_on_a_single_exact_plane():
    rng = np.random.default_rng(3)
    tgt = np.concatenate([rng.integers(-128, 128, size=(500, 2)) / 64.0, np.full((500, 1), 0.25)], axis=1).astype(np.float32)
    nrm = np.tile(np.float32([0, 0, 1]), (500, 1))
    src = (tgt[rng.integers(0, 500, size=300)] + np.float32([0.0, 0.0, 0.125])).astype(np.float32)
    T0 = RR.rigid_about([0, 0, 0.25], [0, 0, 1], 0.0, [0.0, 0.0, 0.0])
    corr = RR.correspondences(RR.nearest(src, tgt))
    T, stats = S.icp_update(dev(src), dev(tgt), dev(corr), torch.from_numpy(T0), target_normals=dev(nrm))
    st = stats.tolist()
    assert st[0] == 300 and st[3] == 2.0 and np.array_equal(bits64(T), T0.view(np.uint64))
    assert rel(st[5], 300 * 0.125 ** 2) <= 1e-12 and rel(st[2], 0.125) <= 1e-12


def test_non_finite_normals_drop_their_rows_only():
    src, tgt, nrm, T0, corr = NR.update_case(257, 0.0)
    bad = nrm.copy()
    hit = np.unique(corr[corr >= 0])[::7]
    bad[hit[0::3], 0] = np.nan
    bad[hit[1::3], 1] = np.inf
    bad[hit[2::3]] = -np.inf
    ref = NR.plane_update(src, tgt, bad, corr, T0)
    full = NR.plane_update(src, tgt, nrm, corr, T0)
    assert 6 <= ref["n"] < full["n"] and ref["status"] == 0
    T, stats = S.icp_update(dev(src), dev(tgt), dev(corr), torch.from_numpy(T0), target_normals=dev(bad))
    st = stats.tolist()
    assert st[0] == ref["n"] and st[3] == 0.0 and rel(st[4], ref["sum_d2"]) <= 1e-12 and rel(st[5], ref["sum_r2"]) <= 1e-12
    assert NR.displacement(T.cpu().numpy(), ref["T"], src) <= 1e-9 * extent(tgt)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def e2e():
    """the scene of NR.E2E_SEED (tests/test_normals_cpu.py shows its preconditions and what the two reference runs reach)"""
    src, tgt, T, md = NR.e2e_planes()
    nrm = NR.estimate(tgt, NR.E2E_NORMAL_RADIUS, 30)[0].astype(np.float32)
    plane = NR.icp_plane(src, tgt, nrm, md, max_iteration=30)
    point = RR.icp(src, tgt, md, relative_fitness=0.0, relative_rmse=0.0, max_iteration=30)
    return src, tgt, T, md, nrm, plane, point


def test_point_to_plane_icp_follows_the_reference_iteration_by_iteration():
    src, tgt, T_true, md, nrm, ref, _ = e2e()
    s, t, nd = dev(src), dev(tgt), dev(nrm)
    bound = 1e-9 * extent(tgt)
    index = NeighborIndex(t)
    T = torch.eye(4, dtype=torch.float64, device="cuda")
    for k, h in enumerate(ref["history"]):
        assert NR.displacement(T.cpu().numpy(), h["T"], src) <= bound, k
        idx, _ = index.query(s, T, md)
        assert np.array_equal(idx.cpu().numpy(), h["corr"]), k
        T, stats = S.icp_update(s, t, idx, T, target_normals=nd)
        st = stats.tolist()
        assert st[0] == h["n"] and st[3] == 0.0 and rel(st[2], h["rmse"]) <= 1e-9, (k, st, h["rmse"])
    results = []
    for use_order in (True, False):
        res = S.registration_icp(s, t, md, index=index, use_order=use_order, estimation="point_to_plane", target_normals=nd)
        assert res.iterations == ref["iterations"] <= 10 and res.converged
        assert NR.displacement(res.transformation.cpu().numpy(), ref["T"], src) <= bound
        assert res.fitness == ref["fitness"] and rel(res.inlier_rmse, ref["rmse"]) <= 1e-9
        assert np.array_equal(res.correspondences.cpu().numpy(), ref["corr"])
        results.append(res)
    assert np.array_equal(bits64(results[0].transformation), bits64(results[1].transformation))
    assert results[0].inlier_rmse == results[1].inlier_rmse
    # the gain, without a timing: point-to-plane is at the motion, and ...
    assert NR.displacement(results[0].transformation.cpu().numpy(), T_true, src) < 1e-6
    # normals estimated inside give the bits of normals estimated outside and handed in
    own = S.estimate_normals(t, NR.E2E_NORMAL_RADIUS, 30)
    a = S.registration_icp(s, t, md, estimation="point_to_plane", target_normals=own)
    b = S.registration_icp(s, t, md, estimation="point_to_plane", normal_radius=NR.E2E_NORMAL_RADIUS, normal_max_nn=30)
    assert np.array_equal(bits64(a.transformation), bits64(b.transformation)) and a.iterations == b.iterations
    assert NR.displacement(a.transformation.cpu().numpy(), T_true, src) < 1e-6
    # no read-back inside the loop
    c = S.registration_icp(s, t, md, estimation="point_to_plane", target_normals=nd, max_iteration=ref["iterations"], check_every=0)
    assert c.iterations == ref["iterations"] and not c.converged
    assert np.array_equal(bits64(c.transformation), bits64(results[0].transformation))


def test_point_to_point_icp_on_the_same_scene_has_not_arrived_after_thirty():
    src, tgt, T_true, md, _, _, ref = e2e()
    s, t = dev(src), dev(tgt)
    res = S.registration_icp(s, t, md, relative_fitness=0.0, relative_rmse=0.0, max_iteration=30)
    assert res.iterations == ref["iterations"] == 30 and not res.converged
    err, bound = NR.displacement(res.transformation.cpu().numpy(), ref["T"], src), 2.0 ** -23 * float(np.abs(tgt).max())
    assert err <= bound, (err, bound)                           # (the point-to-point bound of tests/test_registration_gpu.py)
    assert np.array_equal(res.correspondences.cpu().numpy(), ref["corr"])
    assert NR.displacement(res.transformation.cpu().numpy(), T_true, src) > 1e-3
    # the defaults are point-to-point, bit for bit
    spelled = S.registration_icp(s, t, md, relative_fitness=0.0, relative_rmse=0.0, max_iteration=30, estimation="point_to_point")
    assert np.array_equal(bits64(spelled.transformation), bits64(res.transformation))
    assert spelled.inlier_rmse == res.inlier_rmse and torch.equal(spelled.correspondences, res.correspondences)


def test_register_and_merge_point_to_plane_is_the_composition():
    src, tgt, T_true, md, _, _, _ = e2e()
    v = 1.5 * NR.SPACING
    pts, cols, res = S.register_and_merge(dev(src), None, dev(tgt), None, voxel_size=v, estimation="point_to_plane")
    sd, _ = S.voxel_down_sample(dev(src), None, v)
    td, _ = S.voxel_down_sample(dev(tgt), None, v)
    nrm = S.estimate_normals(td, 2.0 * v, 30)
    want = S.registration_icp(sd, td, 5.0 * v, estimation="point_to_plane", target_normals=nrm)
    assert cols is None and res.iterations == want.iterations
    assert np.array_equal(bits64(res.transformation), bits64(want.transformation))
    assert torch.equal(pts, torch.cat([S.transform_points(dev(src), want.transformation), dev(tgt)]))
    # ... and against the references: the down-sampled clouds, their normals, the reference loop
    sdr = PR.voxel_down_sample_reference(src, None, v)["points"].astype(np.float32)
    tdr = PR.voxel_down_sample_reference(tgt, None, v)["points"].astype(np.float32)
    assert np.array_equal(sd.cpu().numpy(), sdr) and np.array_equal(td.cpu().numpy(), tdr)
    ref = NR.icp_plane(sdr, tdr, nrm.cpu().numpy(), 5.0 * v)
    assert res.iterations == ref["iterations"] and res.fitness == ref["fitness"]
    assert NR.displacement(res.transformation.cpu().numpy(), ref["T"], src) <= 1e-9 * extent(tgt)
    assert NR.displacement(res.transformation.cpu().numpy(), T_true, src) < 1e-3      # (voxel means of two samplings of a plane)


def test_align_map_point_to_plane_moves_the_model_as_transform_would():
    from test_transform_gpu import check_parameters, snapshot
    src, tgt, T_true, md, _, _, _ = e2e()
    P = src.shape[0]
    raw = S.make_gaussians(P, 1, seed=5)
    m = S.GaussianModel.from_raw(raw.to("cuda"))
    with torch.no_grad():
        m._xyz.copy_(dev(src))
    before, _ = snapshot(m)
    res = S.align_map(m, dev(tgt), md, estimation="point_to_plane", normal_radius=NR.E2E_NORMAL_RADIUS)
    want = S.registration_icp(dev(src), dev(tgt), md, estimation="point_to_plane", normal_radius=NR.E2E_NORMAL_RADIUS)
    assert np.array_equal(bits64(res.transformation), bits64(want.transformation)) and res.iterations <= 10
    assert NR.displacement(res.transformation.cpu().numpy(), T_true, src) < 1e-6
    moved = check_parameters(m, before, res.transformation.cpu().numpy()[None], None, "align_map point_to_plane")
    assert bool(moved.all())
