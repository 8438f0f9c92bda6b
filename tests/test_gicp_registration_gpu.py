"""registration_generalized_icp and register_scan_to_map on the device (scene_utils/gicp.py over csrc/gicp.hip) against the float64
loop of tests/gicp_reference.py, on the scene of tests/test_icp_plane_gpu.py: three exact patches and a motion that slides along
them, which point-to-point ICP has not undone after thirty iterations (test_point_to_point_icp_on_the_same_scene_has_not_arrived_
after_thirty there).

Bounds.  Correspondences and n: equal - tests/test_gicp_reference_cpu.py shows every neighbour clear of its runner-up by 1e-5
relative.  T: within 1e-9 x the cloud's extent of the reference's at every iteration (cond(J^T W J) <= 1e6 there).  The end-to-end
runs use epsilon = 1e-4 (gicp_reference.E2E_EPSILON says why): the float64 loop then settles 6.2e-7 from the true motion."""
import functools

import numpy as np
import pytest
import torch

import gicp_reference as G
import normals_reference as NR
import scene_utils as S
from scene_utils import NeighborIndex

pytestmark = pytest.mark.gpu
EPS = G.E2E_EPSILON


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def extent(points):
    return float(np.ptp(np.asarray(points, dtype=np.float64), axis=0).max())


def bits64(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint64)


def rel(a, b):
    return abs(a - b) / abs(b) if b else abs(a)


@functools.lru_cache(maxsize=None)
def e2e():
    src, scov, tgt, tcov, T, md = G.e2e_case()
    return src, scov, tgt, tcov, T, md, G.icp_generalized(src, scov, tgt, tcov, md)


def test_generalized_icp_follows_the_reference_iteration_by_iteration():
    src, scov, tgt, tcov, T_true, md, ref = e2e()
    s, sc, t, tc = dev(src), dev(scov), dev(tgt), dev(tcov)
    bound = 1e-9 * extent(tgt)
    index = NeighborIndex(t)
    T = torch.eye(4, dtype=torch.float64, device="cuda")
    for k, h in enumerate(ref["history"]):
        assert NR.displacement(T.cpu().numpy(), h["T"], src) <= bound, k
        idx, _ = index.query(s, T, md)
        assert np.array_equal(idx.cpu().numpy(), h["corr"]), k
        T, stats = S.gicp_update(s, sc, t, tc, idx, T)
        st = stats.tolist()
        assert st[0] == h["n"] and st[3] == 0.0 and rel(st[2], h["rmse"]) <= 1e-9, (k, st, h["rmse"])
    results = []
    for use_order in (True, False):
        res = S.registration_generalized_icp(s, t, md, index=index, use_order=use_order, source_covariances=sc,
                                             target_covariances=tc)
        assert res.iterations == ref["iterations"] <= 10 and res.converged
        assert NR.displacement(res.transformation.cpu().numpy(), ref["T"], src) <= bound
        assert res.fitness == ref["fitness"] and rel(res.inlier_rmse, ref["rmse"]) <= 1e-9
        assert np.array_equal(res.correspondences.cpu().numpy(), ref["corr"])
        results.append(res)
    assert np.array_equal(bits64(results[0].transformation), bits64(results[1].transformation))
    assert results[0].inlier_rmse == results[1].inlier_rmse
    # it is at the motion, where point-to-point ICP is still 1e-3 away after thirty iterations
    err = NR.displacement(results[0].transformation.cpu().numpy(), T_true, src)
    print(f"generalized ICP: {results[0].iterations} iterations, {err:.3g} from the true motion")
    assert err < 1e-6
    # the target given without an index, and the default order, are the same run
    plain = S.registration_generalized_icp(s, t, md, source_covariances=sc, target_covariances=tc)
    assert np.array_equal(bits64(plain.transformation), bits64(results[0].transformation))
    # no read-back inside the loop
    c = S.registration_generalized_icp(s, t, md, source_covariances=sc, target_covariances=tc, max_iteration=ref["iterations"],
                                       check_every=0)
    assert c.iterations == ref["iterations"] and not c.converged
    assert np.array_equal(bits64(c.transformation), bits64(results[0].transformation))
    assert torch.equal(c.correspondences, results[0].correspondences) and c.inlier_rmse == results[0].inlier_rmse


def test_covariances_estimated_inside_are_those_estimated_outside():
    src, _, tgt, _, T_true, md, ref = e2e()
    s, t = dev(src), dev(tgt)
    own_s = S.estimate_covariances(s, G.COVARIANCE_RADIUS, 20, EPS)
    own_t = S.estimate_covariances(t, G.COVARIANCE_RADIUS, 20, EPS)
    a = S.registration_generalized_icp(s, t, md, source_covariances=own_s, target_covariances=own_t)
    b = S.registration_generalized_icp(s, t, md, covariance_radius=G.COVARIANCE_RADIUS, covariance_max_nn=20, epsilon=EPS)
    c = S.registration_generalized_icp(s, t, md, source_covariances=own_s, covariance_radius=G.COVARIANCE_RADIUS,
                                       covariance_max_nn=20, epsilon=EPS)
    for r in (b, c):
        assert np.array_equal(bits64(a.transformation), bits64(r.transformation)) and a.iterations == r.iterations
        assert torch.equal(a.correspondences, r.correspondences) and a.inlier_rmse == r.inlier_rmse
    assert a.converged and NR.displacement(a.transformation.cpu().numpy(), T_true, src) < 1e-6
    # given covariances are used as given: epsilon plays no part then
    d = S.registration_generalized_icp(s, t, md, source_covariances=own_s, target_covariances=own_t, epsilon=0.5)
    assert np.array_equal(bits64(a.transformation), bits64(d.transformation))
    # ... and against the reference loop on the device's covariances
    own = G.icp_generalized(src, own_s.cpu().numpy(), tgt, own_t.cpu().numpy(), md)
    assert a.iterations == own["iterations"] and a.fitness == own["fitness"]
    assert NR.displacement(a.transformation.cpu().numpy(), own["T"], src) <= 1e-9 * extent(tgt)


def test_register_scan_to_map_uses_the_gaussians_own_shapes():
    src, _, tgt, _, T_true, md, _ = e2e()
    quats, scales, _ = G.map_gaussians(tgt)
    P = tgt.shape[0]
    raw = S.make_gaussians(P, 1, seed=5)
    m = S.GaussianModel.from_raw(raw.to("cuda"))
    with torch.no_grad():
        m._xyz.copy_(dev(tgt))
        m._rotation.copy_(dev(quats))
        m._scaling.copy_(torch.log(dev(scales)))
    names = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity")
    before = {k: getattr(m, k).detach().clone() for k in names}
    s = dev(src)
    res = S.register_scan_to_map(m, s, md, covariance_radius=G.COVARIANCE_RADIUS, epsilon=EPS)
    for k in names:
        assert torch.equal(getattr(m, k).detach().view(torch.int32), before[k].view(torch.int32)), k
    assert m._xyz.requires_grad and m._xyz.grad is None
    tcov = S.regularize_covariances(m.get_covariance().detach(), EPS)
    scov = S.estimate_covariances(s, G.COVARIANCE_RADIUS, 20, EPS)
    want = S.registration_generalized_icp(s, dev(tgt), md, source_covariances=scov, target_covariances=tcov)
    assert np.array_equal(bits64(res.transformation), bits64(want.transformation)) and res.iterations == want.iterations
    assert torch.equal(res.correspondences, want.correspondences) and res.inlier_rmse == want.inlier_rmse
    # the map's covariances are the patches': flat along each patch's normal
    flat = G.regularize(G.gaussian_covariances(quats, scales).astype(np.float32), EPS)["cov"]
    assert np.abs(tcov.cpu().numpy().astype(np.float64) - flat).max() <= 1e-5
    # against the reference loop on those covariances
    ref = G.icp_generalized(src, scov.cpu().numpy(), tgt, tcov.cpu().numpy(), md)
    assert res.iterations == ref["iterations"] <= 10 and res.converged and res.fitness == ref["fitness"]
    assert NR.displacement(res.transformation.cpu().numpy(), ref["T"], src) <= 1e-9 * extent(tgt)
    assert np.array_equal(res.correspondences.cpu().numpy(), ref["corr"])
    err = NR.displacement(res.transformation.cpu().numpy(), T_true, src)
    print(f"scan to map: {res.iterations} iterations, {err:.3g} from the true motion")
    assert err < 1e-6
    # a subset of the map by keyframe: the rows of the two anchors that are asked for
    anchor = torch.arange(P, dtype=torch.int32, device="cuda") % 3
    m._anchor = anchor
    sub = S.register_scan_to_map(m, s, md, ids=[0, 2], covariance_radius=G.COVARIANCE_RADIUS, epsilon=EPS)
    keep = anchor != 1
    want = S.registration_generalized_icp(s, dev(tgt)[keep], md, source_covariances=scov, target_covariances=tcov[keep])
    assert np.array_equal(bits64(sub.transformation), bits64(want.transformation)) and sub.iterations == want.iterations
