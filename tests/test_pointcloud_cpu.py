"""Point-cloud conditioning without a device: the C ABI's new symbols and host-side size queries, argument validation (before any
device work, so it can be seen here), the no-CPU-path errors, and the test reference's own lattice against an independent one."""
import ctypes

import numpy as np
import pytest
import torch

import pointcloud_reference as PR

NEW_SYMBOLS = ("gsr_knn_k_workspace_bytes", "gsr_knn_k", "gsr_voxel_workspace_bytes", "gsr_voxel_down_sample",
               "gsr_outlier_workspace_bytes", "gsr_statistical_outliers")


def test_new_symbols_resolve_and_the_abi_version_stays():
    from diff_gaussian_rasterization import _C
    raw = ctypes.CDLL(_C.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert hasattr(raw, n), n
        assert n in _C.EXPORTS, n
    assert _C.lib().gsr_abi_version() == 7


@pytest.mark.parametrize("query", ["gsr_knn_k_workspace_bytes", "gsr_voxel_workspace_bytes", "gsr_outlier_workspace_bytes"])
def test_workspace_queries_are_positive_and_monotone(query):
    from diff_gaussian_rasterization import _C
    f = getattr(_C.lib(), query)
    sizes = [f(P) for P in (0, 1, 63, 65, 4097, 307200, 1000000, 5000000)]
    assert all(s > 0 and s % 256 == 0 for s in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[1] < sizes[-1]
    assert sizes[-1] >= 5000000 * 16      # at least the sorted points / the cell words and permutations


def test_outlier_workspace_holds_the_search():
    from diff_gaussian_rasterization import _C
    lib = _C.lib()
    for P in (1, 1000, 100000):
        assert lib.gsr_outlier_workspace_bytes(P) > lib.gsr_knn_k_workspace_bytes(P) >= lib.gsr_knn_workspace_bytes(P)


def test_c_abi_rejects_bad_arguments_before_any_device_work():
    """no device here: a call that launched anything could not return these codes"""
    from diff_gaussian_rasterization import _C
    lib = _C.lib()
    INVALID = -1
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    for k in (0, 33, -1):
        assert lib.gsr_knn_k(10, p, k, p, p, p, 1 << 30, None) == INVALID
        assert "knn_k" in _C.last_error()
    assert lib.gsr_knn_k(10, p, 3, None, None, p, 1 << 30, None) == INVALID
    for v in (0.0, -0.05, float("inf"), float("nan")):
        assert lib.gsr_voxel_down_sample(10, p, None, v, None, p, None, None, 10, p, p, 1 << 30, None) == INVALID
    bad_origin = (ctypes.c_float * 3)(0.0, float("nan"), 0.0)
    assert lib.gsr_voxel_down_sample(10, p, None, 0.05, bad_origin, p, None, None, 10, p, p, 1 << 30, None) == INVALID
    for nb in (1, 34):
        assert lib.gsr_statistical_outliers(10, p, nb, 2.0, p, None, None, p, 1 << 30, None) == INVALID
    assert lib.gsr_statistical_outliers(10, p, 20, float("nan"), p, None, None, p, 1 << 30, None) == INVALID
    # a workspace that is too small is refused before anything is launched, too
    TOO_SMALL = lib.gsr_knn_k(10, p, 3, p, p, p, 16, None)
    assert TOO_SMALL < 0 and TOO_SMALL != INVALID
    assert lib.gsr_voxel_down_sample(10, p, None, 0.05, None, p, None, None, 10, p, p, 16, None) == TOO_SMALL
    assert lib.gsr_statistical_outliers(10, p, 20, 2.0, p, None, None, p, 16, None) == TOO_SMALL


def test_scene_utils_imports_without_a_device_and_exports_the_surface():
    import scene_utils
    import simple_knn
    for n in ("voxel_down_sample", "statistical_outlier_mask", "remove_statistical_outliers", "condition_point_cloud"):
        assert callable(getattr(scene_utils, n)), n
    assert callable(simple_knn.knn_k)


def test_cpu_tensors_raise_gsr_error():
    from diff_gaussian_rasterization import _C
    from scene_utils import (GaussianModel, condition_point_cloud, remove_statistical_outliers, statistical_outlier_mask,
                             voxel_down_sample)
    from simple_knn import knn_k
    pts, cols = torch.rand(50, 3), torch.rand(50, 3)
    with pytest.raises(_C.GsrError, match="no CPU path"):
        knn_k(pts, 3)
    with pytest.raises(_C.GsrError, match="no CPU path"):
        voxel_down_sample(pts, cols)
    with pytest.raises(_C.GsrError, match="no CPU path"):
        statistical_outlier_mask(pts)
    with pytest.raises(_C.GsrError, match="no CPU path"):
        remove_statistical_outliers(pts, cols)
    with pytest.raises(_C.GsrError, match="no CPU path"):
        condition_point_cloud(pts, cols)
    with pytest.raises(_C.GsrError, match="no CPU path"):
        voxel_down_sample(pts.numpy())
    with pytest.raises(_C.GsrError):
        GaussianModel(0).create_from_pcd(pts, cols, voxel_size=0.05, nb_neighbors=20)


def test_argument_validation_comes_before_the_device_check():
    from scene_utils import condition_point_cloud, remove_statistical_outliers, statistical_outlier_mask, voxel_down_sample
    from simple_knn import knn_k
    pts, cols = torch.rand(50, 3), torch.rand(50, 3)      # CPU tensors: a GsrError would mean the values were not looked at first
    for v in (0, -0.05, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="voxel_size"):
            voxel_down_sample(pts, cols, voxel_size=v)
        with pytest.raises(ValueError, match="voxel_size"):
            condition_point_cloud(pts, cols, voxel_size=v)
    with pytest.raises(TypeError, match="voxel_size"):
        voxel_down_sample(pts, cols, voxel_size="0.05")
    for o in ((0.0, 1.0), (0.0, 1.0, float("nan")), (0.0, 1.0, 2.0, 3.0)):
        with pytest.raises(ValueError, match="origin"):
            voxel_down_sample(pts, cols, origin=o)
    for nb in (1, 0, 34):
        with pytest.raises(ValueError, match="nb_neighbors"):
            statistical_outlier_mask(pts, nb_neighbors=nb)
        with pytest.raises(ValueError, match="nb_neighbors"):
            remove_statistical_outliers(pts, cols, nb_neighbors=nb)
        with pytest.raises(ValueError, match="nb_neighbors"):
            condition_point_cloud(pts, cols, nb_neighbors=nb)
    with pytest.raises(TypeError, match="nb_neighbors"):
        statistical_outlier_mask(pts, nb_neighbors=20.0)
    with pytest.raises(ValueError, match="std_ratio"):
        statistical_outlier_mask(pts, std_ratio=float("nan"))
    with pytest.raises(TypeError, match="std_ratio"):
        statistical_outlier_mask(pts, std_ratio=None)
    for k in (0, 33, -3):
        with pytest.raises(ValueError, match="k="):
            knn_k(pts, k)
    with pytest.raises(TypeError, match="k="):
        knn_k(pts, 3.0)
    with pytest.raises(ValueError, match="nothing asked for"):
        knn_k(pts, 3, return_dist2=False, return_mean=False)


def test_reference_lattice_agrees_with_an_independent_float64_lattice():
    """points at least 1 % of a cell away from every face: the float32 operations cannot carry them across"""
    rng = np.random.default_rng(0)
    v = 0.05
    origin = np.array([-1.0, 0.5, 2.0])
    cells = rng.integers(-40, 40, size=(4000, 3))
    frac = rng.uniform(0.01, 0.99, size=(4000, 3))
    pts = (origin + (cells + frac) * v).astype(np.float32)
    got, kept = PR.voxel_cells_f32(pts, v, origin)
    assert kept.all() and np.array_equal(got, cells)
    assert np.array_equal(PR.voxel_cells_f64(pts, v, origin), cells)
    assert PR.voxel_in_range(got, kept)
    # the default origin is min - v / 2: the smallest coordinate of every axis sits in the middle of cell 0
    got0, _ = PR.voxel_cells_f32(pts, v)
    assert (got0.min(axis=0) == 0).all()
    out = PR.voxel_down_sample_reference(pts, None, v, origin)
    assert int(out["counts"].sum()) == 4000 and out["cells"].shape[0] == len({tuple(c) for c in cells})
    key = [tuple(c[::-1]) for c in out["cells"]]
    assert key == sorted(key)                                  # ascending (i_z, i_y, i_x)
    centre = origin + (out["cells"] + 0.5) * v
    assert float(np.abs(out["points"] - centre).max()) <= v / 2


def test_reference_filter_on_its_own_seeds():
    """the GPU test's cloud: the reference alone removes every planted point, keeps the surface, and has no row within 1e-5
    relative of its threshold (so the GPU comparison excludes nothing on the reference's account)"""
    pts, planted = PR.surface_with_outliers(0)
    so = PR.statistical_outlier_reference(pts, 20, 2.0)
    assert so["n_valid"] == 3030 and not (so["keep"] & planted).any()
    assert (so["keep"] & ~planted).sum() >= 0.95 * 3000
    near = np.abs(so["dbar"] - so["threshold"]) <= 1e-5 * so["threshold"]
    assert int(near.sum()) <= max(1, 3030 // 1000)
    d2, mean = PR.knn_k_reference(np.array([[0, 0, 0], [3, 4, 0], [0, 0, 1]], dtype=np.float32), 2)
    assert np.allclose(d2, [[1, 25], [25, 26], [1, 26]]) and np.allclose(mean, [(1 + 5) / 3, (5 + 26 ** 0.5) / 3, (1 + 26 ** 0.5) / 3])
