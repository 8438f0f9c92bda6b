"""Point-cloud conditioning on the device against the CPU restatements of pointcloud_reference.py.

knn_k: dist2 row-wise against the sorted float64 brute force, mean distance likewise - 1e-6 relative, exactly 0 where the
reference is 0 (the bar of test_knn_gpu.py: above the ~3e-7 that the three roundings of a difference-based float32 distance
allow; the sorted distances and their mean are continuous in which neighbour wins a tie, a missed neighbour is orders above).
voxel_down_sample: voxel set, order and counts EQUAL the float32 numpy lattice; means within 2^-23 max|value on the axis| of the
float64 mean (twice the half-ulp of the one final rounding).
statistical_outlier_mask: mu, sigma, threshold within 1e-6 relative; the mask equal except on rows whose reference mean distance
lies within 1e-5 relative of the threshold, at most max(1, P / 1000) of them."""
import functools
import math

import numpy as np
import pytest
import torch

import pointcloud_reference as PR

pytestmark = pytest.mark.gpu
REL = 1e-6
KS = (1, 3, 4, 5, 19, 32)           # the edges of the list sizes 4 / 8 / 16 / 32
CLOUDS = {"uniform": PR.uniform_cloud, "clustered": PR.clustered_cloud, "duplicates": PR.duplicate_cloud}


@functools.lru_cache(maxsize=None)
def cloud_and_reference(kind, P):
    """the cloud and its 32 nearest squared distances, computed once and shared (read-only) by every k"""
    pts = CLOUDS[kind](P, seed=100 + P)
    d2, _ = PR.knn_k_reference(pts, 32)
    d2.setflags(write=False)
    pts.setflags(write=False)
    return pts, d2


def assert_rel(got, want, label):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf), label
    zero = want == 0
    assert (got[zero] == 0).all(), label
    m = ~inf & ~zero
    err = float((np.abs(got[m] - want[m]) / want[m]).max()) if m.any() else 0.0
    print(f"{label}: max rel err {err:.3e} over {int(m.sum())} values, {int(zero.sum())} zeros, {int(inf.sum())} inf")
    assert err <= REL, (label, err)


@pytest.mark.parametrize("P", [1, 2, 5, 63, 65, 257, 4097, 5000])
@pytest.mark.parametrize("kind", ["uniform", "clustered", "duplicates"])
def test_knn_k_against_brute_force(kind, P):
    from simple_knn import knn_k
    pts, ref = cloud_and_reference(kind, P)
    dev = torch.from_numpy(np.array(pts)).cuda()
    for k in KS:
        d2, mean = knn_k(dev, k, return_dist2=True, return_mean=True)
        assert d2.shape == (P, k) and mean.shape == (P,) and d2.dtype == mean.dtype == torch.float32
        d2 = d2.cpu().numpy()
        assert_rel(d2, ref[:, :k], f"knn_k {kind} P={P} k={k} dist2")
        keff = min(k, P - 1)
        assert (np.diff(d2[:, :keff], axis=1) >= 0).all()                        # ascending
        assert np.isinf(d2[:, keff:]).all() and np.isfinite(d2[:, :keff]).all()  # k > P - 1: the +inf tail
        assert_rel(mean.cpu().numpy(), PR.knn_mean_from_dist2(ref, k), f"knn_k {kind} P={P} k={k} mean")
    if P == 1:
        assert knn_k(dev, 3, return_dist2=False, return_mean=True).tolist() == [0.0]


def test_knn_k_outputs_alone_and_runs_repeat_bit_for_bit():
    from simple_knn import knn_k
    pts = torch.from_numpy(np.array(cloud_and_reference("duplicates", 5000)[0])).cuda()
    for k in (3, 19):
        d2, mean = knn_k(pts, k, return_mean=True)
        d2b, meanb = knn_k(pts, k, return_mean=True)
        assert torch.equal(d2, d2b) and torch.equal(mean, meanb)
        assert torch.equal(knn_k(pts, k), d2)
        assert torch.equal(knn_k(pts, k, return_dist2=False, return_mean=True), mean)


@pytest.mark.parametrize("kind,P", [("uniform", 5000), ("clustered", 4097), ("duplicates", 5000), ("uniform", 2), ("uniform", 3),
                                    ("uniform", 5)])
def test_knn_k3_gives_the_values_knn_dist2_averages(kind, P):
    """the same search, the same float32 distances: the existing result is their mean after its own fadd / fdiv sequence"""
    from simple_knn import knn_dist2, knn_k
    pts = torch.from_numpy(np.array(cloud_and_reference(kind, P)[0])).cuda()
    d = knn_k(pts, 3).cpu().numpy()      # (numpy float32 on the host: IEEE add / divide, one rounding each, as __fadd_rn / __fdiv_rn)
    assert d.dtype == np.float32
    if P >= 4:
        mean = ((d[:, 0] + d[:, 1]) + d[:, 2]) / np.float32(3.0)
    elif P == 3:
        mean = (d[:, 0] + d[:, 1]) * np.float32(0.5)
    else:
        mean = d[:, 0]
    assert mean.dtype == np.float32 and np.array_equal(mean, knn_dist2(pts).cpu().numpy())


def test_knn_k_nan_rows_leave_the_finite_rows_alone():
    from simple_knn import knn_k
    pts = np.array(cloud_and_reference("uniform", 5000)[0])
    rng = np.random.default_rng(9)
    bad = rng.permutation(5000)[:60]
    dirty = pts.copy()
    dirty[bad[:20], 0] = np.nan
    dirty[bad[20:40], 1] = np.inf
    dirty[bad[40:], 2] = -np.inf
    ok = np.ones(5000, dtype=bool)
    ok[bad] = False
    for k in (3, 19):
        d2, mean = knn_k(torch.from_numpy(dirty).cuda(), k, return_mean=True)
        c2, cmean = knn_k(torch.from_numpy(pts[ok]).cuda(), k, return_mean=True)
        assert torch.equal(d2.cpu()[ok], c2.cpu()) and torch.equal(mean.cpu()[ok], cmean.cpu())      # as if the rows were absent
        assert torch.isinf(d2.cpu()[~ok]).all() and torch.isnan(mean.cpu()[~ok]).all()
    want, wmean = PR.knn_k_reference(dirty, 19)
    assert_rel(d2.cpu().numpy(), want, "knn_k with non-finite rows dist2")
    assert_rel(mean.cpu().numpy()[ok], wmean[ok], "knn_k with non-finite rows mean")


def test_knn_k_rejects_k_out_of_range():
    from simple_knn import knn_k
    pts = torch.rand(100, 3, device="cuda")
    for k in (0, 33):
        with pytest.raises(ValueError, match="k="):
            knn_k(pts, k)
    assert knn_k(torch.zeros(0, 3, device="cuda"), 5).shape == (0, 5)


# ---- voxel grid -----------------------------------------------------------------------------------------------------------------
def check_voxels(pts, cols, v, origin=None, label=""):
    from scene_utils import voxel_down_sample
    ref = PR.voxel_down_sample_reference(pts, cols, v, origin)
    dp = torch.from_numpy(np.ascontiguousarray(pts)).cuda()
    dc = torch.from_numpy(np.ascontiguousarray(cols)).cuda() if cols is not None else None
    out_p, out_c, out_n = voxel_down_sample(dp, dc, voxel_size=v, origin=origin, return_counts=True)
    V = ref["counts"].shape[0]
    assert out_p.shape == (V, 3) and out_n.shape == (V,) and out_n.dtype == torch.int32, (out_p.shape, V)
    assert np.array_equal(out_n.cpu().numpy().astype(np.int64), ref["counts"])      # the counts in order pin set and order ...
    got = out_p.cpu().numpy().astype(np.float64)
    kept = PR.finite_rows(pts)
    o = PR.voxel_origin_f32(pts, v, origin).astype(np.float64)
    if V:
        # ... and so does every mean lying in the reference's cell of that row (up to the rounding of the lattice itself)
        assert float(np.abs(got - (o + (ref["cells"] + 0.5) * v)).max()) <= v / 2 * (1 + 1e-5) + 1e-6 * np.abs(got).max()
        tol = 2.0 ** -23 * np.abs(np.asarray(pts, dtype=np.float64)[kept]).max(axis=0)
        err = np.abs(got - ref["points"]).max(axis=0)
        print(f"voxel {label}: P = {pts.shape[0]}, V = {V}, longest run {int(ref['counts'].max())}, mean err {err}, bound {tol}")
        assert (err <= tol).all(), (err, tol)
    if cols is None:
        assert out_c is None
    else:
        assert out_c.shape == (V, 3)
        if V:
            tolc = 2.0 ** -23 * np.abs(np.asarray(cols, dtype=np.float64)[kept]).max(axis=0)
            assert (np.abs(out_c.cpu().numpy().astype(np.float64) - ref["colors"]).max(axis=0) <= tolc).all()
    again = voxel_down_sample(dp, dc, voxel_size=v, origin=origin, return_counts=True)
    assert torch.equal(again[0], out_p) and torch.equal(again[2], out_n) and (cols is None or torch.equal(again[1], out_c))
    return out_p, out_c, out_n, ref


@pytest.mark.parametrize("P", [1, 63, 65, 4097, 5000])
@pytest.mark.parametrize("with_colors", [False, True])
def test_voxel_down_sample_matches_the_float32_lattice(P, with_colors):
    pts = PR.uniform_cloud(P, seed=200 + P)
    cols = np.random.default_rng(P).uniform(0, 1, size=(P, 3)).astype(np.float32) if with_colors else None
    check_voxels(pts, cols, 0.2, label=f"uniform colours={with_colors}")
    check_voxels(pts, cols, 0.05, origin=(0.013, -0.5, 0.25), label="explicit origin, negative indices")
    cells, _ = PR.voxel_cells_f32(pts, 0.05, (0.013, -0.5, 0.25))
    assert cells.min() < 0 < cells.max() or P == 1


def test_voxel_every_point_its_own_voxel():
    rng = np.random.default_rng(3)
    cells = rng.permutation(30 ** 3)[:5000]
    pts = ((np.stack([cells % 30, cells // 30 % 30, cells // 900], axis=1) + rng.uniform(0.2, 0.8, size=(5000, 3))) * 0.1)
    out_p, _, out_n, _ = check_voxels(pts.astype(np.float32), None, 0.1, origin=(0.0, 0.0, 0.0), label="own voxels")
    assert out_p.shape[0] == 5000 and int(out_n.max()) == 1
    order = np.lexsort((cells % 30, cells // 30 % 30, cells // 900))
    assert np.array_equal(out_p.cpu().numpy(), pts.astype(np.float32)[order])      # the mean of one point is the point


def test_voxel_long_runs_are_reduced_cooperatively():
    rng = np.random.default_rng(4)
    one = (5.0 + rng.uniform(0.001, 0.099, size=(5000, 3))).astype(np.float32)
    cols = rng.uniform(0, 1, size=(5000, 3)).astype(np.float32)
    _, _, out_n, _ = check_voxels(one, cols, 0.1, origin=(5.0, 5.0, 5.0), label="one voxel of 5000")
    assert out_n.tolist() == [5000]
    singles = rng.permutation(40 ** 3)[:2000] + 1
    sp = (np.stack([singles % 40, singles // 40 % 40, singles // 1600], axis=1) + rng.uniform(0.2, 0.8, size=(2000, 3))) * 0.1
    big = rng.uniform(0.001, 0.099, size=(3000, 3))                                # cell (0, 0, 0): not among the singles
    mixed = np.concatenate([sp, big])[rng.permutation(5000)].astype(np.float32)
    _, _, out_n, ref = check_voxels(mixed, cols, 0.1, origin=(0.0, 0.0, 0.0), label="3000 among 2000 singles")
    assert sorted(out_n.tolist())[-2:] == [1, 3000] and out_n.shape[0] == 2001
    # run lengths around the split (64 | 65 rows of one voxel)
    for n in (64, 65, 129):
        pts = np.concatenate([rng.uniform(0.001, 0.099, size=(n, 3)), 0.1 + rng.uniform(0.001, 0.099, size=(7, 3))])
        _, _, out_n, _ = check_voxels(pts.astype(np.float32), None, 0.1, origin=(0.0, 0.0, 0.0), label=f"run of {n}")
        assert out_n.tolist() == [n, 7]


def test_voxel_shared_origin_gives_one_lattice_and_non_finite_rows_are_dropped():
    from scene_utils import voxel_down_sample
    a, b = PR.uniform_cloud(3000, 11), PR.uniform_cloud(3000, 12) + np.float32(0.37)
    origin, v = (-2.0, -2.0, -2.0), 0.25
    outs = [check_voxels(x, None, v, origin=origin, label="shared origin")[3] for x in (a, b, np.concatenate([a, b]))]
    both = {tuple(c) for c in outs[2]["cells"]}
    assert {tuple(c) for c in outs[0]["cells"]} | {tuple(c) for c in outs[1]["cells"]} == both
    assert len({tuple(c) for c in outs[0]["cells"]} & {tuple(c) for c in outs[1]["cells"]}) > 100      # shared cells exist
    dirty = a.copy()
    dirty[5, 0], dirty[77, 1], dirty[2999, 2] = np.nan, np.inf, -np.inf
    _, _, out_n, _ = check_voxels(dirty, None, v, label="non-finite rows")
    assert int(out_n.sum()) == 2997
    nothing = np.full((70, 3), np.nan, dtype=np.float32)
    p, c, n = voxel_down_sample(torch.from_numpy(nothing).cuda(), return_counts=True)
    assert p.shape == (0, 3) and c is None and n.shape == (0,)
    p, c = voxel_down_sample(torch.zeros(0, 3, device="cuda"), torch.zeros(0, 3, device="cuda"))
    assert p.shape == (0, 3) and c.shape == (0, 3)


def test_voxel_capacity_guard_and_index_range():
    import ctypes as C
    from diff_gaussian_rasterization import _C
    from scene_utils import voxel_down_sample
    pts = torch.from_numpy(PR.uniform_cloud(4097, 5)).cuda()
    ref = PR.voxel_down_sample_reference(pts.cpu().numpy(), None, 0.2)
    V, cap = ref["counts"].shape[0], 100
    assert V > cap
    GUARD = 12345.0
    out_p = torch.full((cap + 1, 3), GUARD, device="cuda")
    out_c = torch.full((cap + 1, 3), GUARD, device="cuda")
    out_n = torch.full((cap + 1,), 777, dtype=torch.int32, device="cuda")
    count = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    lib = _C.lib()
    ws = torch.empty(lib.gsr_voxel_workspace_bytes(4097), dtype=torch.uint8, device="cuda")
    _C.check(lib.gsr_voxel_down_sample(4097, _C.ptr(pts), _C.ptr(pts), 0.2, None, _C.ptr(out_p), _C.ptr(out_c), _C.ptr(out_n), cap,
                                       _C.ptr(count), _C.ptr(ws), ws.numel(), _C._stream()))
    assert count.tolist() == [V, 0]                                           # the count is the cloud's, not the capacity's
    assert np.array_equal(out_n[:cap].cpu().numpy(), ref["counts"][:cap])
    assert float((out_p[:cap].cpu().double() - torch.from_numpy(ref["points"][:cap])).abs().max()) <= 2.0 ** -23 * 1.3
    assert torch.equal(out_p[:cap], out_c[:cap])
    assert (out_p[cap] == GUARD).all() and (out_c[cap] == GUARD).all() and int(out_n[cap]) == 777
    # an index outside [-2^20, 2^20): status through the ABI, ValueError through the wrapper
    far = pts.clone()
    far[17, 1] = 3.0e5
    cells, kept = PR.voxel_cells_f32(far.cpu().numpy(), 0.2)
    assert not PR.voxel_in_range(cells, kept)
    _C.check(lib.gsr_voxel_down_sample(4097, _C.ptr(far), None, 0.2, None, _C.ptr(out_p), None, None, cap, _C.ptr(count),
                                       _C.ptr(ws), ws.numel(), _C._stream()))
    assert int(count[1]) != 0
    with pytest.raises(ValueError, match="cell index"):
        voxel_down_sample(far, voxel_size=0.2)
    edge = torch.tensor([[0.0, 0.0, 0.0], [(2 ** 20 - 1) * 0.5, 0.0, -(2 ** 20) * 0.5]], device="cuda")      # the last cells in range
    p, _, n = voxel_down_sample(edge, voxel_size=0.5, origin=(0.0, 0.0, 0.0), return_counts=True)
    assert n.tolist() == [1, 1] and torch.equal(p, edge[[1, 0]])


# ---- statistical outlier filter ---------------------------------------------------------------------------------------------------
def check_filter(pts, nb, ratio, label=""):
    from scene_utils import statistical_outlier_mask
    ref = PR.statistical_outlier_reference(pts, nb, ratio)
    dev = torch.from_numpy(np.ascontiguousarray(pts)).cuda()
    keep, stats = statistical_outlier_mask(dev, nb_neighbors=nb, std_ratio=ratio, return_stats=True)
    keep2, stats2 = statistical_outlier_mask(dev, nb_neighbors=nb, std_ratio=ratio, return_stats=True)
    assert torch.equal(keep, keep2) and torch.equal(stats, stats2)
    assert torch.equal(statistical_outlier_mask(dev, nb, ratio), keep)
    assert keep.dtype == torch.bool and stats.dtype == torch.float64 and stats.is_cuda
    n, mu, sigma, thr = stats.tolist()
    print(f"filter {label}: n {n} / {ref['n_valid']}, mu {mu:.9g} / {ref['mu']:.9g}, sigma {sigma:.9g} / {ref['sigma']:.9g}, "
          f"threshold {thr:.9g} / {ref['threshold']:.9g}")
    assert n == ref["n_valid"]
    for got, want in ((mu, ref["mu"]), (sigma, ref["sigma"]), (thr, ref["threshold"])):
        assert abs(got - want) <= REL * abs(want), (got, want)
    P = pts.shape[0]
    with np.errstate(invalid="ignore"):
        near = np.abs(ref["dbar"] - ref["threshold"]) <= 1e-5 * abs(ref["threshold"])
    if P >= 21:
        assert int(near.sum()) <= max(1, P // 1000)
    else:
        # P = 1 / 2: sigma = 0 and every row sits ON the threshold whatever the points are - nothing is excluded there, the masks
        # must agree outright (the strict `<` drops the rows in both)
        near[:] = False
    got = keep.cpu().numpy()
    assert np.array_equal(got[~near], ref["keep"][~near]), int((got != ref["keep"]).sum())
    return got, ref


def test_filter_removes_planted_points_and_keeps_the_surface():
    pts, planted = PR.surface_with_outliers(0)
    got, ref = check_filter(pts, 20, 2.0, "surface + 30 far points")
    assert not got[planted].any() and not ref["keep"][planted].any()
    assert got[~planted].sum() >= 0.95 * 3000 and ref["keep"][~planted].sum() >= 0.95 * 3000
    from scene_utils import remove_statistical_outliers
    cols = torch.rand(3030, 3, device="cuda")
    p, c, idx = remove_statistical_outliers(torch.from_numpy(pts).cuda(), cols, 20, 2.0)
    assert torch.equal(idx.cpu(), torch.from_numpy(np.nonzero(got)[0])) and idx.dtype == torch.int64
    assert torch.equal(p.cpu(), torch.from_numpy(pts)[idx.cpu()]) and torch.equal(c, cols[idx])


def test_filter_drops_duplicates_and_non_finite_rows():
    pts, _ = PR.surface_with_outliers(1, n_surface=1500, n_far=10)
    pts = pts.copy()
    pts[100:125] = pts[100]                    # 25 copies: the 19 nearest are at distance 0 -> mean distance 0
    pts[7, 2] = np.nan
    pts[900, 0] = np.inf
    got, ref = check_filter(pts, 20, 2.0, "duplicates + non-finite rows")
    assert ref["n_valid"] == 1508 and not got[100:125].any() and not got[7] and not got[900]
    assert (ref["dbar"][100:125] == 0).all()


@pytest.mark.parametrize("P", [1, 2, 21])
@pytest.mark.parametrize("nb", [2, 20, 33])
def test_filter_small_sets_and_neighbour_counts(P, nb):
    check_filter(PR.uniform_cloud(P, seed=300 + P), nb, 1.0, f"P={P} nb={nb}")


@pytest.mark.parametrize("nb", [2, 33])
def test_filter_neighbour_count_edges_on_the_surface(nb):
    pts, planted = PR.surface_with_outliers(2, n_surface=2000, n_far=20)
    got, _ = check_filter(pts, nb, 2.0, f"nb={nb}")
    assert got[~planted].sum() >= 0.9 * 2000


def test_filter_empty_input():
    from scene_utils import remove_statistical_outliers, statistical_outlier_mask
    e = torch.zeros(0, 3, device="cuda")
    assert statistical_outlier_mask(e).shape == (0,)
    p, c, idx = remove_statistical_outliers(e, e)
    assert p.shape == (0, 3) and c.shape == (0, 3) and idx.shape == (0,)


# ---- the composition ----------------------------------------------------------------------------------------------------------------
def noisy_scan(seed, n=5000, n_far=25):
    pts, planted = PR.surface_with_outliers(seed, n_surface=n - n_far, n_far=n_far)
    cols = np.random.default_rng(seed).uniform(0, 1, size=(n, 3)).astype(np.float32)
    return pts, cols, planted


def test_condition_point_cloud_is_the_composition_of_the_references():
    from scene_utils import condition_point_cloud, voxel_down_sample
    pts, cols, _ = noisy_scan(5)
    v, nb, ratio = 0.03, 20, 2.0
    vox = PR.voxel_down_sample_reference(pts, cols, v)
    dp, dc = torch.from_numpy(pts).cuda(), torch.from_numpy(cols).cuda()
    mid_p, mid_c = voxel_down_sample(dp, dc, voxel_size=v)
    assert mid_p.shape[0] == vox["counts"].shape[0] < 5000
    tol = 2.0 ** -23 * np.abs(pts.astype(np.float64)).max(axis=0)
    assert (np.abs(mid_p.cpu().numpy().astype(np.float64) - vox["points"]).max(axis=0) <= tol).all()
    # the filter's reference on the product's down-sampled points (the float32 values it really sees), the rules of check_filter
    got, ref = check_filter(mid_p.cpu().numpy(), nb, ratio, "down-sampled scan")
    out_p, out_c = condition_point_cloud(dp, dc, voxel_size=v, nb_neighbors=nb, std_ratio=ratio)
    assert torch.equal(out_p, mid_p[torch.from_numpy(got).cuda()]) and torch.equal(out_c, mid_c[torch.from_numpy(got).cuda()])
    assert 0 < out_p.shape[0] < mid_p.shape[0]
    # either stage alone
    only_v = condition_point_cloud(dp, dc, voxel_size=v, nb_neighbors=None)
    assert torch.equal(only_v[0], mid_p) and torch.equal(only_v[1], mid_c)
    only_f = condition_point_cloud(mid_p, mid_c, voxel_size=None, nb_neighbors=nb, std_ratio=ratio)
    assert torch.equal(only_f[0], out_p)
    e = torch.zeros(0, 3, device="cuda")
    assert condition_point_cloud(e, e)[0].shape == (0, 3)


# ---- mapping hooks ------------------------------------------------------------------------------------------------------------------
def rgbd_frame(seed, W=96, H=72):
    import mapping_reference as MR
    from scene_utils import fibonacci_cameras
    cam = fibonacci_cameras(3, W, H, seed=seed, device="cuda")[0]
    depth = torch.from_numpy(MR.depth_sheet(H, W, seed=seed, base=2.0, amp=0.4)).cuda()
    image = torch.rand(3, H, W, generator=torch.Generator().manual_seed(seed)).cuda()
    return cam, image, depth


def params(m):
    from scene_utils.model import _PARAM_ATTRS
    return [getattr(m, a).detach().clone() for a in _PARAM_ATTRS]


def test_mapping_defaults_change_nothing():
    from scene_utils import GaussianModel
    pts, cols, _ = noisy_scan(6)
    dp, dc = torch.from_numpy(pts).cuda(), torch.from_numpy(cols).cuda()
    a = GaussianModel(2).create_from_pcd(dp, dc, spatial_lr_scale=1.5)
    b = GaussianModel(2).create_from_pcd(dp, dc, spatial_lr_scale=1.5, voxel_size=None, nb_neighbors=None, std_ratio=2.0)
    assert all(torch.equal(x, y) for x, y in zip(params(a), params(b))) and a._xyz.shape[0] == 5000
    cam, image, depth = rgbd_frame(7)
    na = a.add_from_rgbd(cam, image, depth, stride=2)
    nb = b.add_from_rgbd(cam, image, depth, stride=2, voxel_size=None, voxel_origin=None, nb_neighbors=None, std_ratio=2.0)
    assert na == nb > 0 and all(torch.equal(x, y) for x, y in zip(params(a), params(b)))


def test_create_from_pcd_conditions_the_cloud_first():
    from scene_utils import GaussianModel, condition_point_cloud
    from simple_knn import knn_dist2
    pts, cols, _ = noisy_scan(8)
    dp, dc = torch.from_numpy(pts).cuda(), torch.from_numpy(cols).cuda()
    m = GaussianModel(1).create_from_pcd(dp, dc, voxel_size=0.03, nb_neighbors=20, anchor=4)
    want_p, want_c = condition_point_cloud(dp, dc, 0.03, 20, 2.0)
    n = want_p.shape[0]
    assert 0 < n < 5000 and torch.equal(m._xyz.detach(), want_p)
    for attr, cols_ in (("_features_dc", (1, 3)), ("_features_rest", (3, 3)), ("_scaling", (3,)), ("_rotation", (4,)),
                        ("_opacity", (1,))):
        assert tuple(getattr(m, attr).shape) == (n,) + cols_
    assert m._anchor.shape == (n,) and int(m._anchor.min()) == 4 and m.max_radii2D.shape == (n,)
    # sized by the neighbour search on the CONDITIONED cloud
    want = torch.log(torch.sqrt(knn_dist2(want_p).clamp_min(1e-7)))
    assert torch.equal(m._scaling.detach()[:, 0], want)


def test_add_from_rgbd_conditions_the_new_points_and_a_trainer_steps():
    from gaussian_renderer import render, PipelineParams
    from scene_utils import GaussianModel, Trainer, make_gaussians, unproject_rgbd
    from scene_utils.model import _PARAM_ATTRS
    cam, image, depth = rgbd_frame(9)
    H, W = depth.shape
    fy, fx = 30, 40
    assert abs(float(depth[fy, fx]) - 2.0) < 0.6
    depth = depth.clone()
    depth[fy, fx] = 0.8                                        # a flying pixel: far in front of the sheet
    v = 0.08
    xyz, rgb = unproject_rgbd(cam, image, depth)
    assert xyz.shape[0] == H * W
    flying = xyz[fy * W + fx]
    ref = PR.voxel_down_sample_reference(xyz.cpu().numpy(), None, v)
    V = ref["counts"].shape[0]
    assert V < H * W // 2                                      # the lattice really merges pixels

    bg = torch.zeros(3, device="cuda")
    model = GaussianModel.from_raw(make_gaussians(1500, 1, seed=5, scale_factor=0.5).to("cuda"))
    cams = [cam]
    tr = Trainer(model, cams, {0: image}, render, PipelineParams(), bg, separate_sh=True)
    tr.step(0)
    tr.finish()
    P = model.get_xyz.shape[0]
    old = params(model)
    fired = []
    model._resize_hooks.append(fired.append)                   # behind the trainer's own hook
    n = model.add_from_rgbd(cam, image, depth, voxel_size=v, anchor=3)
    assert n == V and model.get_xyz.shape[0] == P + V          # one Gaussian per occupied voxel
    assert fired == ["before", "after"]
    new = model._xyz.detach()[P:]
    cells = torch.from_numpy(ref["cells"]).cuda().double()
    o = torch.from_numpy((xyz.cpu().numpy().min(axis=0) - np.float32(0.5) * np.float32(v)).astype(np.float64)).cuda()
    centre = o + (cells + 0.5) * v
    assert float((new.double() - centre).norm(dim=1).max()) <= v * math.sqrt(3) / 2 * (1 + 1e-5)
    assert float((new - flying).norm(dim=1).min()) <= v * math.sqrt(3)      # without the filter the flying pixel is in the map
    for a, o_ in zip(_PARAM_ATTRS, old):
        p = getattr(model, a)
        st = model.optimizer.state[p]
        assert p.shape[0] == P + V and torch.equal(p.detach()[:P], o_)
        assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape
        assert float(st["exp_avg"][P:].abs().max()) == 0.0
    assert model.xyz_gradient_accum.shape[0] == model.denom.shape[0] == model.max_radii2D.shape[0] == P + V
    assert model._anchor.shape == (P + V,) and bool((model._anchor[P:] == 3).all())
    out = tr.step(0)
    tr.finish()
    assert torch.isfinite(out["loss"])
    assert float(model.optimizer.state[model._xyz]["exp_avg"][P:].abs().max()) > 0

    # with the filter the flying pixel is gone; on a shared lattice (voxel_origin) the rows are the composition's
    m2 = GaussianModel(1)
    n2 = m2.add_from_rgbd(cam, image, depth, voxel_size=v, voxel_origin=(0.0, 0.0, 0.0), nb_neighbors=20, std_ratio=2.0)
    from scene_utils import condition_point_cloud
    want_p, _ = condition_point_cloud(xyz, rgb, v, 20, 2.0, origin=(0.0, 0.0, 0.0))
    assert 0 < n2 == want_p.shape[0] < H * W // 2 and torch.equal(m2._xyz.detach(), want_p)
    assert float((m2._xyz.detach() - flying).norm(dim=1).min()) > 0.5
    m3 = GaussianModel(1)
    m3.add_from_rgbd(cam, image, depth, voxel_size=v, voxel_origin=(0.0, 0.0, 0.0))
    assert float((m3._xyz.detach() - flying).norm(dim=1).min()) <= v * math.sqrt(3)
    with pytest.raises(ValueError, match="voxel_size"):
        m3.add_from_rgbd(cam, image, depth, voxel_size=-1.0)
