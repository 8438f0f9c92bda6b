"""Registration on the device (csrc/registration.hip) against the float64 restatements of tests/registration_reference.py.

Bounds.  A distance: the project's 1e-6 relative (0 where 0), as for gsr_knn_k - both sides start from the SAME float32 query,
because q = (float32)(R s + t) is bit-identical by construction (asserted below through transform_points).  A transform: the
largest displacement of a source row, max_i |T_got s_i - T_ref s_i| <= 2^-23 max|coordinate| - below one float32 ulp of the data,
the bound the voxel means are held to.  Sums: 1e-12 relative (float64 sums of <= 65 537 non-negative terms in a different order:
<= n 2^-53 relative)."""
import functools

import numpy as np
import pytest
import torch

import pointcloud_reference as PR
import registration_reference as RR
import scene_utils as S
from scene_utils import NeighborIndex

pytestmark = pytest.mark.gpu
U23 = 2.0 ** -23
PT_SIZES = [1, 2, 63, 64, 65, 4096, 4097, 5000]
PS_SIZES = [1, 255, 256, 257, 5000]


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def cloud(kind, P, seed):
    return {"uniform": PR.uniform_cloud, "clustered": PR.clustered_cloud, "duplicates": PR.duplicate_cloud}[kind](P, seed)


def assert_dist(got, want, label):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isinf(got), np.isinf(want)), label
    f = np.isfinite(want)
    err = np.abs(got[f] - want[f])
    bad = err > 1e-6 * np.abs(want[f])
    assert not bad.any(), (label, float((err / np.maximum(np.abs(want[f]), 1e-300))[bad].max()))


def transform_error(T_got, T_ref, source):
    s = np.asarray(source, dtype=np.float64)
    a = s @ np.asarray(T_got)[:3, :3].T + np.asarray(T_got)[:3, 3]
    b = s @ np.asarray(T_ref)[:3, :3].T + np.asarray(T_ref)[:3, 3]
    return float(np.linalg.norm(a - b, axis=1).max()), U23 * float(np.abs(b).max())


@functools.lru_cache(maxsize=None)
def search_case(kind, Pt):
    """target, 5000 queries near it (the smaller query sets are prefixes), one generic rigid T about the cloud's centre, and the
    reference's answers under the identity and under T"""
    tgt = cloud(kind, Pt, 20 + Pt)
    big = cloud(kind, 5000, 7)
    src = cloud(kind, 5000, 8)
    if kind == "duplicates":                                   # half the queries ARE target rows: exact ties at distance 0
        src[::2] = tgt[np.random.default_rng(9).integers(0, Pt, size=2500)]
    centre = big.astype(np.float64).mean(axis=0)
    T = RR.rigid_about(centre, [0.4, -0.7, 0.5], 0.3, [0.05, -0.02, 0.03])
    refs = {}
    for name, M in (("identity", None), ("rigid", T)):
        q = RR.apply_transform(M, src)
        refs[name] = (M, q, RR.nearest(q, tgt))
    return tgt, src, refs


def own_d2(q, tgt, idx):
    """float64 distance of every query to the row it was given"""
    e = q.astype(np.float64) - tgt.astype(np.float64)[idx]
    return (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]


@pytest.mark.parametrize("Pt", PT_SIZES)
@pytest.mark.parametrize("kind", ["uniform", "clustered", "duplicates"])
def test_search_against_brute_force(kind, Pt):
    tgt, src, refs = search_case(kind, Pt)
    index = NeighborIndex(dev(tgt))
    _, canon = np.unique(tgt, axis=0, return_inverse=True)
    canon = canon.reshape(-1)
    first_of = np.full(canon.max() + 1, Pt, dtype=np.int64)
    np.minimum.at(first_of, canon, np.arange(Pt))               # the smallest row among rows with identical coordinates
    for name, (M, q, ref) in refs.items():
        Md = None if M is None else torch.from_numpy(M)
        assert np.array_equal(S.transform_points(dev(src), Md).cpu().numpy().view(np.uint32), q.view(np.uint32)), (name, "q bits")
        for Ps in PS_SIZES:
            label = f"{kind} Pt={Pt} Ps={Ps} {name}"
            idx, d2 = index.query(dev(src[:Ps]), Md)
            idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
            assert idx.dtype == np.int32 and d2.dtype == np.float32 and idx.shape == d2.shape == (Ps,)
            assert (idx >= 0).all() and (idx < Pt).all(), label
            assert_dist(d2, ref["d2"][:Ps], label)
            assert_dist(own_d2(q[:Ps], tgt, idx), ref["d2"][:Ps], label + " (the returned row's own distance)")
            assert np.array_equal(idx, first_of[canon[idx]]), label + ": not the smallest row among equal points"
            if kind == "duplicates" and name == "identity":
                zero = ref["d2"][:Ps] == 0.0
                assert zero.sum() >= Ps // 2 and np.array_equal(idx[zero], ref["idx"][:Ps][zero]), label


def test_search_staging_loop_second_round():
    """Pt = 256 * 4096 + 1: the smallest target with 257 super-boxes, so the LDS staging loop runs twice"""
    Pt = 256 * 4096 + 1
    tgt, src = PR.uniform_cloud(Pt, 31), PR.uniform_cloud(300, 32)
    ref = RR.nearest(src, tgt, chunk=16)
    idx, d2 = S.nn_search(dev(src), dev(tgt))
    idx = idx.cpu().numpy()
    assert_dist(d2.cpu().numpy(), ref["d2"], "1M + 1")
    assert_dist(own_d2(src, tgt, idx), ref["d2"], "1M + 1 own")
    assert (idx == ref["idx"]).mean() > 0.99


def test_max_distance_validity():
    tgt, src = PR.uniform_cloud(5000, 11), PR.uniform_cloud(5000, 12)
    ref = RR.nearest(src, tgt)
    md = float(np.sqrt(np.median(ref["d2"])))
    thr = RR.max_dist2(md)
    band = np.abs(ref["d2"] - thr) <= 1e-5 * thr
    assert band.mean() < 0.01
    idx, d2 = NeighborIndex(dev(tgt)).query(dev(src), max_distance=md)
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    valid = idx >= 0
    assert np.array_equal(valid[~band], (ref["d2"] <= thr)[~band]) and 0.3 < valid.mean() < 0.7
    assert np.isinf(d2[~valid]).all() and (d2[valid] <= np.float32(thr)).all()
    assert_dist(d2[valid], ref["d2"][valid], "within max_distance")
    # max_distance 0 keeps exact hits only
    idx0, d20 = NeighborIndex(dev(tgt)).query(dev(np.concatenate([tgt[:3], src[:3]])), max_distance=0.0)
    assert idx0.tolist() == [0, 1, 2, -1, -1, -1] and d20[:3].tolist() == [0.0, 0.0, 0.0]


def test_non_finite_rows_change_no_other_row():
    tgt, src = PR.uniform_cloud(4097, 41), PR.uniform_cloud(1000, 42)
    T = torch.from_numpy(RR.rigid_about([0, 0, 0], [1, 1, 0], 0.2, [0.01, 0, 0]))
    idx, d2 = NeighborIndex(dev(tgt)).query(dev(src), T)
    junk = np.array([[np.nan, 0, 0], [0, np.inf, 0], [1, 2, -np.inf], [np.nan] * 3], dtype=np.float32)
    tgt2 = np.concatenate([tgt, np.repeat(junk, 40, axis=0)])     # rows behind the clean ones: their numbers stay
    src2 = np.concatenate([src, junk])
    idx2, d22 = NeighborIndex(dev(tgt2)).query(dev(src2), T)
    assert torch.equal(idx2[:1000], idx) and torch.equal(d22[:1000].view(torch.int32), d2.view(torch.int32))
    assert idx2[1000:].tolist() == [-1] * 4 and bool(torch.isinf(d22[1000:]).all())
    only = NeighborIndex(dev(junk)).query(dev(src[:10]))
    assert only[0].tolist() == [-1] * 10 and bool(torch.isinf(only[1]).all())


def test_runs_shuffles_and_order_agree_bit_for_bit():
    tgt, src = PR.duplicate_cloud(5000, 51), PR.clustered_cloud(3000, 52, offset=0.0) * 0.3
    T = torch.from_numpy(RR.rigid_about([0, 0, 0], [0, 1, 1], 0.4, [0.1, 0, -0.1]))
    index = NeighborIndex(dev(tgt))
    s = dev(src)
    a = index.query(s, T, 0.05)
    b = NeighborIndex(dev(tgt)).query(s, T, 0.05)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    perm = torch.randperm(3000, generator=torch.Generator().manual_seed(1)).cuda()
    c = index.query(s[perm], T, 0.05)
    assert torch.equal(c[0], a[0][perm]) and torch.equal(c[1].view(torch.int32), a[1][perm].view(torch.int32))
    morton = index.query_order(s, T)
    assert torch.equal(torch.sort(morton.long()).values, torch.arange(3000, device="cuda"))
    for order in (morton, perm.int()):
        d = index.query(s, T, 0.05, order=order)
        assert torch.equal(d[0], a[0]) and torch.equal(d[1].view(torch.int32), a[1].view(torch.int32))
    assert -1 in a[0].tolist() and int((a[0] >= 0).sum()) > 100


# ---- one update ---------------------------------------------------------------------------------------------------------------------
def update_case(Ps, offset, planar=False, seed=0):
    """a 500-point target; every source row is a target point moved back by a known motion, plus noise, so that the reference's
    neighbours under a nearby T leave some rows without a correspondence"""
    rng = np.random.default_rng(100 + Ps + seed)
    tgt = (offset + rng.uniform(-1, 1, size=(500, 3))).astype(np.float32)
    if planar:
        tgt[:, 2] = np.float32(offset + 0.25)
    truth = RR.rigid_about([offset] * 3, [0.3, 0.5, -0.8], 0.15, [0.04, -0.03, 0.02])
    noise = 0.01 * rng.standard_normal((Ps, 3))
    if planar:
        noise[:, 2] = 0.0
    p = tgt[rng.integers(0, 500, size=Ps)].astype(np.float64) + noise
    if planar:                                                 # a motion inside the plane: the source is exactly planar too
        truth = RR.rigid_about([offset] * 3, [0, 0, 1], 0.15, [0.04, -0.03, 0.0])
    inv = np.linalg.inv(truth)
    src = (p @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    if planar:
        src[:, 2] = np.float32(offset + 0.25)
    T0 = RR.rigid_about([offset] * 3, [0.1, 0.2, 0.9], 0.03, [0.01, 0.01, -0.01])
    corr = RR.correspondences(RR.nearest(RR.apply_transform(T0, src), tgt, 0.12))
    return src, tgt, T0, corr


@pytest.mark.parametrize("Ps", [3, 256, 257, 65537])
@pytest.mark.parametrize("offset", [0.0, 1000.0])
def test_update_against_kabsch(Ps, offset):
    src, tgt, T0, corr = update_case(Ps, offset)
    if Ps == 3:
        corr = RR.correspondences(RR.nearest(RR.apply_transform(T0, src), tgt))      # all three rows, or nothing to solve
    ref = RR.update(src, tgt, corr, T0)
    assert ref["status"] == 0 and (Ps == 3 or 0 < ref["n"] <= Ps)
    T, stats = S.icp_update(dev(src), dev(tgt), dev(corr), torch.from_numpy(T0))
    T, stats = T.cpu().numpy(), stats.tolist()
    assert stats[0] == ref["n"] and stats[3] == 0.0
    assert abs(stats[1] - ref["fitness"]) <= 1e-12 * ref["fitness"]
    assert abs(stats[2] - ref["rmse"]) <= 1e-12 * ref["rmse"] and abs(stats[4] - ref["sum_d2"]) <= 1e-12 * ref["sum_d2"]
    err, bound = transform_error(T, ref["T"], src)
    print(f"update Ps={Ps} offset={offset}: n={ref['n']} err {err:.3g} bound {bound:.3g}")
    assert err <= bound and T[3].tolist() == [0.0, 0.0, 0.0, 1.0]
    assert abs(np.linalg.det(T[:3, :3]) - 1.0) < 1e-12


@pytest.mark.parametrize("offset", [0.0, 1000.0])
def test_update_planar_cloud_gives_a_proper_rotation(offset):
    src, tgt, T0, corr = update_case(257, offset, planar=True)
    ref = RR.update(src, tgt, corr, T0)
    assert ref["n"] > 50
    T, stats = S.icp_update(dev(src), dev(tgt), dev(corr), torch.from_numpy(T0))
    T = T.cpu().numpy()
    assert stats.tolist()[3] == 0.0 and abs(np.linalg.det(T[:3, :3]) - 1.0) < 1e-12
    assert np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() < 1e-12
    err, bound = transform_error(T, ref["T"], src)
    assert err <= bound, (err, bound)


def test_update_with_fewer_than_three_rows_leaves_T():
    src, tgt, T0, corr = update_case(256, 0.0)
    keep = np.flatnonzero(corr >= 0)[:2]
    few = np.full_like(corr, -1)
    few[keep] = corr[keep]
    for c, n in ((few, 2), (np.full_like(corr, -1), 0), (np.full_like(corr, 500), 0)):      # (500: a row the target lacks)
        T, stats = S.icp_update(dev(src), dev(tgt), dev(c), torch.from_numpy(T0))
        assert np.array_equal(T.cpu().numpy().view(np.uint64), T0.view(np.uint64))
        st = stats.tolist()
        assert st[0] == n and st[3] == 1.0 and st[1] == n / 256
        if n == 2:
            assert abs(st[2] - RR.update(src, tgt, few, T0)["rmse"]) <= 1e-12 * st[2]


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def e2e(kind):
    """inputs of seed RR.E2E_SEED / RR.E2E_OVERLAP_SEED (tests/test_registration_cpu.py shows their preconditions)"""
    src, tgt, T, md = RR.e2e_full() if kind == "full" else RR.e2e_overlap()
    return src, tgt, T, md, RR.icp(src, tgt, md, max_iteration=30)


@pytest.mark.parametrize("kind", ["full", "overlap"])
def test_icp_agrees_with_the_reference_iteration_by_iteration(kind):
    src, tgt, T_true, md, ref = e2e(kind)
    s, t = dev(src), dev(tgt)
    index = NeighborIndex(t)
    T = torch.eye(4, dtype=torch.float64, device="cuda")
    for k, h in enumerate(ref["history"]):
        err, bound = transform_error(T.cpu().numpy(), h["T"], src)
        assert err <= bound, (k, err, bound)
        idx, _ = index.query(s, T, md)
        assert np.array_equal(idx.cpu().numpy(), h["corr"]), (k, int((idx.cpu().numpy() != h["corr"]).sum()))
        T, stats = S.icp_update(s, t, idx, T)
        st = stats.tolist()
        # (rmse: the two transforms differ in the last bits, so a q may round to the neighbouring float32 - a relative 2^-23 of
        # one term; 1e-6 relative holds whatever number of terms does so)
        assert st[1] == h["fitness"] and abs(st[2] - h["rmse"]) <= 1e-6 * h["rmse"] + 1e-12, (k, st, h["fitness"], h["rmse"])
    # the driver: the same stopping rule, the same number of updates, fitness and rmse of the returned transformation
    for use_order in (True, False):
        res = S.registration_icp(s, t, md, index=index, use_order=use_order)
        assert res.iterations == ref["iterations"] and res.converged == ref["converged"]
        err, bound = transform_error(res.transformation.cpu().numpy(), ref["T"], src)
        assert err <= bound, (err, bound)
        assert res.fitness == ref["fitness"], (res.fitness, ref["fitness"])
        assert abs(res.inlier_rmse - ref["rmse"]) <= 1e-6 * ref["rmse"] + 1e-12
        assert np.array_equal(res.correspondences.cpu().numpy(), ref["corr"])
    ev = S.evaluate_registration(s, None, md, res.transformation, index=index)
    assert ev.fitness == res.fitness and ev.inlier_rmse == res.inlier_rmse and ev.iterations == 0
    if kind == "full":
        err, bound = transform_error(res.transformation.cpu().numpy(), T_true, src)
        print(f"final T against the motion: err {err:.3g} bound {bound:.3g}")
        assert err <= bound
        moved = S.transform_points(s, res.transformation).cpu().numpy().astype(np.float64)
        want = tgt.astype(np.float64)[ref["corr"]]
        assert np.linalg.norm(moved - want, axis=1).max() <= 2 * bound      # (+ the rounding of q itself: one more ulp)


def test_hundred_iterations_without_read_back_stay_a_rigid_transform():
    src, tgt, T_true, md, ref = e2e("full")
    res = S.registration_icp(dev(src), dev(tgt), md, max_iteration=100, check_every=0)
    assert res.iterations == 100 and not res.converged
    T = res.transformation.cpu().numpy()
    S.validate_transforms(T)
    err, bound = transform_error(T, T_true, src)
    assert err <= bound and res.fitness == 1.0
    every3 = S.registration_icp(dev(src), dev(tgt), md, check_every=3)
    assert every3.converged and every3.iterations % 3 == 0 and ref["iterations"] <= every3.iterations < ref["iterations"] + 3


def test_register_and_merge_is_the_composition_of_the_references():
    rng = np.random.default_rng(5)
    src, tgt, T_true, md = RR.e2e_full()
    scol, tcol = rng.uniform(size=src.shape).astype(np.float32), rng.uniform(size=tgt.shape).astype(np.float32)
    v = 0.2
    pts, cols, res = S.register_and_merge(dev(src), dev(scol), dev(tgt), dev(tcol), voxel_size=v)
    sd = PR.voxel_down_sample_reference(src, None, v)["points"].astype(np.float32)
    td = PR.voxel_down_sample_reference(tgt, None, v)["points"].astype(np.float32)
    ref = RR.icp(sd, td, 5 * v)
    assert res.iterations == ref["iterations"] and res.fitness == ref["fitness"]
    err, bound = transform_error(res.transformation.cpu().numpy(), ref["T"], src)
    assert err <= bound, (err, bound)
    want = np.concatenate([RR.apply_transform(ref["T"], src), tgt]).astype(np.float64)
    got = pts.cpu().numpy().astype(np.float64)
    assert got.shape == want.shape and np.array_equal(got[5000:], want[5000:])
    assert np.linalg.norm(got - want, axis=1).max() <= 2 * bound
    assert np.array_equal(cols.cpu().numpy(), np.concatenate([scol, tcol]))
    # the merged cloud down-sampled again, and no colours
    mp, mc, _ = S.register_and_merge(dev(src), dev(scol), dev(tgt), dev(tcol), voxel_size=v, merge_voxel_size=0.1)
    wp, wc = S.voxel_down_sample(pts, cols, 0.1)
    assert torch.equal(mp, wp) and torch.equal(mc, wc) and mp.shape[0] < pts.shape[0]
    np_, nc, _ = S.register_and_merge(dev(src), None, dev(tgt), None, voxel_size=v, max_correspondence_distance=5 * v)
    assert nc is None and torch.equal(np_, pts)


def test_align_map_moves_the_model_as_transform_would():
    from gaussian_renderer import render, PipelineParams
    from test_transform_gpu import check_parameters, snapshot
    P = 2000
    raw = S.make_gaussians(P, 3, seed=5)
    m = S.GaussianModel.from_raw(raw.to("cuda"))
    cams = S.fibonacci_cameras(2, 64, 48, seed=3, device="cuda")
    image = torch.rand(3, 48, 64, generator=torch.Generator().manual_seed(1)).cuda()
    tr = S.Trainer(m, cams[:1], {0: image}, render, PipelineParams(), torch.zeros(3, device="cuda"), separate_sh=True)
    tr.step(0)
    tr.finish()
    xyz = m.get_xyz.detach().cpu().numpy()
    extent = xyz.max(axis=0) - xyz.min(axis=0)
    h = RR.mean_spacing(P, extent)
    motion = RR.rigid_about(xyz.mean(axis=0), [0.2, 0.9, -0.3], np.deg2rad(3.0), 0.2 * h * np.array([0.6, 0.0, 0.8]))
    tgt = RR.apply_transform(motion, xyz)[np.random.default_rng(2).permutation(P)]
    ref = RR.icp(xyz, tgt, 2.0 * h)
    err, bound = transform_error(ref["T"], motion, xyz)
    assert ref["converged"] and err <= bound                    # the reference itself finds the motion
    before, _ = snapshot(m)
    res = S.align_map(m, dev(tgt), 2.0 * h)
    assert res.iterations == ref["iterations"] and res.fitness == 1.0
    err, bound = transform_error(res.transformation.cpu().numpy(), ref["T"], xyz)
    assert err <= bound, (err, bound)
    moved = check_parameters(m, before, ref["T"][None], None, "align_map")
    assert bool(moved.all())
    tr.step(0)                                                  # the trainer goes on with the moved map
    tr.finish()
    # by anchor: only the rows of keyframe 1 are registered and moved
    m2 = S.GaussianModel.from_raw(raw.to("cuda"))
    anchors = (torch.arange(P) % 2).int()
    m2.set_anchors(anchors)
    before2, _ = snapshot(m2)
    mine = (anchors == 1).numpy()
    xyz2 = m2.get_xyz.detach().cpu().numpy()                   # (the first model's means have taken an optimizer step)
    tgt2 = RR.apply_transform(motion, xyz2)[np.random.default_rng(2).permutation(P)]
    ref2 = RR.icp(xyz2[mine], tgt2, 2.0 * h)
    S.align_map(m2, dev(tgt2), 2.0 * h, ids=[1])
    moved2 = check_parameters(m2, before2, ref2["T"][None], torch.where(anchors == 1, 0, -1), "align_map ids")
    assert torch.equal(moved2, anchors == 1)
