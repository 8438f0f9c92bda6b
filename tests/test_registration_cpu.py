"""Registration without a device: the C ABI's new symbols and size queries, argument validation (before any device work, so it
can be seen here), the no-CPU-path errors, the float64 reference on known motions, and the PRECONDITIONS of the GPU tests' inputs
shown on the reference alone: at every reference iteration of the end-to-end inputs the float64 gap between the best and the
second-best distance, and the distance of every best from the threshold, exceed 1e-5 relative - float32 distances then select
the rows and the validity float64 selects."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import pointcloud_reference as PR
import registration_reference as RR

NEW_SYMBOLS = ("gsr_nn_index_bytes", "gsr_nn_index_build", "gsr_nn_search", "gsr_nn_order_workspace_bytes", "gsr_nn_query_order",
               "gsr_transform_points", "gsr_icp_workspace_bytes", "gsr_icp_update")
MARGIN = 1e-5


def test_new_symbols_resolve_and_the_abi_version_stays():
    from diff_gaussian_rasterization import _C
    raw = ctypes.CDLL(_C.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert hasattr(raw, n), n
        assert n in _C.EXPORTS, n
    assert _C.lib().gsr_abi_version() == 7


def test_size_queries():
    from diff_gaussian_rasterization import _C
    lib = _C.lib()
    sizes = [lib.gsr_nn_index_bytes(P) for P in (0, 1, 63, 65, 4097, 307200, 1000000)]
    assert all(s > 0 and s % 256 == 0 for s in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert sizes[-1] >= 1000000 * 16
    assert lib.gsr_icp_workspace_bytes(1) == lib.gsr_icp_workspace_bytes(1000000) >= 256 * 17 * 8
    assert 0 < lib.gsr_nn_order_workspace_bytes(1) < lib.gsr_nn_order_workspace_bytes(1000000)


def test_entry_points_reject_bad_arguments_before_any_launch():
    from diff_gaussian_rasterization import _C
    lib = _C.lib()
    p = ctypes.c_void_p(4096)      # never dereferenced: every call below fails its argument check
    inf = float("inf")
    bad = _C.lib().gsr_nn_index_build
    assert bad(0, p, p, 1 << 30, None) == -1 and bad(1 << 30, p, p, 1 << 40, None) == -1 and bad(5, None, p, 1 << 30, None) == -1
    assert bad(5, p, None, 1 << 30, None) == -1
    assert bad(5, p, p, lib.gsr_nn_index_bytes(5) - 1, None) == -5 and "needed" in _C.last_error()
    s = lib.gsr_nn_search
    assert s(5, p, 0, p, None, inf, None, p, None, None) == -1 and s(0, p, 5, p, None, inf, None, p, None, None) == -1
    assert s(5, None, 5, p, None, inf, None, p, None, None) == -1 and s(5, p, 5, None, None, inf, None, p, None, None) == -1
    assert s(5, p, 5, p, None, inf, None, None, None, None) == -1
    assert s(5, p, 5, p, None, -1.0, None, p, None, None) == -1 and s(5, p, 5, p, None, float("nan"), None, p, None, None) == -1
    o = lib.gsr_nn_query_order
    assert o(5, p, 5, p, None, None, p, 1 << 30, None) == -1 and o(5, p, 5, p, None, p, p, 16, None) == -5
    assert lib.gsr_transform_points(0, p, None, p, None) == -1 and lib.gsr_transform_points(5, p, None, None, None) == -1
    u = lib.gsr_icp_update
    ws = lib.gsr_icp_workspace_bytes(5)
    assert u(5, p, 5, p, p, p, p, p, ws - 1, None) == -5
    assert u(0, p, 5, p, p, p, p, p, ws, None) == -1 and u(5, p, 1 << 30, p, p, p, p, p, ws, None) == -1
    for k in range(6):      # source, target, idx, T, stats, workspace
        args = [p] * 6
        args[k] = None
        assert u(5, args[0], 5, args[1], args[2], args[3], args[4], args[5], ws, None) == -1, k


def test_python_validation_comes_first_and_there_is_no_cpu_path():
    import scene_utils as S
    import simple_knn
    from diff_gaussian_rasterization import _C
    a, b = torch.rand(10, 3), torch.rand(12, 3)
    for call in (lambda: S.registration_icp(a, b, -1.0), lambda: S.registration_icp(a, b, float("nan")),
                 lambda: S.registration_icp(a, b, 0.5, max_iteration=0), lambda: S.registration_icp(a, b, 0.5, check_every=-1),
                 lambda: S.registration_icp(a, b, 0.5, relative_rmse=-1e-6), lambda: S.registration_icp(a, b, 0.5, init=torch.eye(3)),
                 lambda: S.evaluate_registration(a, b, 0.5, transformation=np.zeros((4, 3))),
                 lambda: S.nn_search(a, b, max_distance=-2.0), lambda: S.nn_search(a, b, transform=torch.eye(4, dtype=torch.int32)),
                 lambda: S.register_and_merge(a, None, b, None, voxel_size=0.0),
                 lambda: S.register_and_merge(a, a, b, None), lambda: S.register_and_merge(a, None, b, None, merge_voxel_size=-1.0)):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: S.registration_icp(a, b, "0.5"), lambda: S.registration_icp(a, b, 0.5, max_iteration=2.5),
                 lambda: S.registration_icp(a, b, 0.5, index="x"), lambda: S.register_and_merge(a, None, b, None, init=np.eye(4))):
        with pytest.raises(TypeError):
            call()
    for call in (lambda: S.registration_icp(a, b, 0.5), lambda: S.evaluate_registration(a, b, 0.5), lambda: S.NeighborIndex(b),
                 lambda: simple_knn.nn_search(a, b), lambda: S.register_and_merge(a, None, b, None),
                 lambda: S.transform_points(a, np.eye(4)), lambda: S.icp_update(a, b, torch.zeros(10, dtype=torch.int32), None),
                 lambda: S.align_map(S.GaussianModel.from_raw(S.make_gaussians(20, 1, seed=1)), b, 0.5)):
        with pytest.raises(_C.GsrError, match="no CPU path"):
            call()


# ---- the reference itself -----------------------------------------------------------------------------------------------------------
def test_apply_transform_is_the_documented_order_and_rounds_once():
    rng = np.random.default_rng(0)
    p = (rng.normal(size=(200, 3)) * 50).astype(np.float32)
    T = RR.rigid_about([3, -2, 1], [1, 2, 3], 0.7, [0.5, 0.25, -4])
    q = RR.apply_transform(T, p)
    for r in (0, 17, 199):
        x, y, z = (float(v) for v in p[r])
        for i in range(3):
            want = np.float32(((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3])
            assert q[r, i] == want and q.dtype == np.float32
    assert np.array_equal(RR.apply_transform(None, p), p)
    exact = p.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    assert np.abs(q - exact).max() <= 2.0 ** -24 * np.abs(exact).max() * 1.0001      # half an ulp: one rounding


def test_nearest_breaks_ties_by_row_and_drops_non_finite_rows():
    tgt = np.array([[1, 0, 0], [np.nan, 0, 0], [0, 1, 0], [1, 0, 0], [np.inf, 0, 0]], dtype=np.float32)
    q = np.array([[1, 0, 0], [0.5, 0.5, 0], [np.nan, 1, 1], [0, 0, 9]], dtype=np.float32)
    n = RR.nearest(q, tgt, max_distance=2.0)
    assert n["idx"].tolist() == [0, 0, -1, 0] and n["d2"][:2].tolist() == [0.0, 0.5] and n["second"][0] == 0.0
    assert n["valid"].tolist() == [True, True, False, False] and RR.correspondences(n).tolist() == [0, 0, -1, -1]


@pytest.mark.parametrize("offset", [0.0, 1000.0])
def test_kabsch_recovers_a_known_motion_and_never_reflects(offset):
    rng = np.random.default_rng(1)
    q = rng.normal(size=(300, 3)) + offset
    T = RR.rigid_about([offset] * 3, [0.2, 1, -0.4], 1.1, [0.3, -0.2, 0.1])
    p = q @ T[:3, :3].T + T[:3, 3]
    assert np.abs(RR.kabsch(q, p) - T).max() < 1e-9 * max(1.0, offset)
    q[:, 2] = offset                                           # a planar cloud: the third singular value is 0
    p = q @ T[:3, :3].T + T[:3, 3]
    got = RR.kabsch(q, p)
    assert abs(np.linalg.det(got[:3, :3]) - 1.0) < 1e-12 and np.abs(got - T).max() < 1e-9 * max(1.0, offset)
    mirrored = p * np.array([1, 1, -1])                         # no rigid motion fits: still a proper rotation
    assert abs(np.linalg.det(RR.kabsch(q + rng.normal(size=q.shape), mirrored)[:3, :3]) - 1.0) < 1e-12


@functools.lru_cache(maxsize=None)
def e2e(kind):
    src, tgt, T, md = RR.e2e_full() if kind == "full" else RR.e2e_overlap()
    return src, tgt, T, md, RR.icp(src, tgt, md, max_iteration=30)


def test_reference_icp_recovers_the_motion_of_a_rigid_copy():
    src, tgt, T, md, r = e2e("full")
    assert r["converged"] and 3 <= r["iterations"] <= 30 and r["fitness"] == 1.0
    got, want = RR.apply_transform(r["T"], src).astype(np.float64), RR.apply_transform(T, src).astype(np.float64)
    assert np.linalg.norm(got - want, axis=1).max() <= 2.0 ** -23 * np.abs(want).max()
    assert r["history"][0]["fitness"] == 1.0 and r["history"][0]["rmse"] > 10 * r["rmse"]


def test_reference_icp_on_a_partial_overlap():
    src, tgt, T, md, r = e2e("overlap")
    assert r["converged"] and 0.3 < r["fitness"] < 0.5
    # the shared slab fits: its rows land within the distance the threshold allows, and T is close to the motion
    assert np.abs(r["T"] - T).max() < 5e-3


@pytest.mark.parametrize("kind", ["full", "overlap"])
def test_preconditions_of_the_end_to_end_inputs(kind):
    """seeds RR.E2E_SEED / RR.E2E_OVERLAP_SEED: conditions, not measurements - a seed that fails here is replaced"""
    src, tgt, T, md, r = e2e(kind)
    ms = [h["margins"] for h in r["history"]] + [r["final_margins"]]
    print(kind, "iterations", r["iterations"], "smallest gap %.3g, smallest threshold distance %.3g" %
          (min(m[0] for m in ms), min(m[1] for m in ms)))
    assert all(m[0] > MARGIN and m[1] > MARGIN for m in ms)


def test_max_distance_inputs_keep_the_threshold_band_thin():
    """the inputs of the GPU test's max_distance case: under 1 % of the rows within 1e-5 relative of the threshold"""
    tgt, src = PR.uniform_cloud(5000, 11), PR.uniform_cloud(5000, 12)
    n = RR.nearest(src, tgt)
    md = float(np.sqrt(np.median(n["d2"])))
    thr = RR.max_dist2(md)
    band = np.abs(n["d2"] - thr) <= 1e-5 * thr
    assert band.mean() < 0.01 and 0.3 < (n["d2"] <= thr).mean() < 0.7
