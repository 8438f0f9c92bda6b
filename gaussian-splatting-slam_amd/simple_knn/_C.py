"""The native surface of `simple_knn`: `distCUDA2(points)` as the reference calls it, and `knn_dist2(points, first_query)`,
the same search answered only for the rows from `first_query` on (new points against map + new points); `knn_k(points, k)`,
the search for k = 1 .. 32 neighbours (every squared distance and / or the mean distance an outlier filter thresholds);
`nn_search(query, target)`, the nearest row of ANOTHER cloud with its row number (csrc/registration.hip);
`estimate_normals(points, radius, max_nn)`, the normal of every row from its hybrid neighbourhood (csrc/normals.hip);
`compute_fpfh(points, normals, radius, max_nn)`, the 33-bin point feature histogram of every row (csrc/features.hip);
`estimate_color_gradients(points, colors, normals, radius, max_nn)`, the colour gradient of every row in its tangent plane
(csrc/colored.hip)."""
import math

import torch

from diff_gaussian_rasterization import _C as _gsr


def knn_dist2(points, first_query=0):
    """points [P,3] float on the HIP device -> float32 [P - first_query]: for every row i >= first_query the mean of the three
    smallest squared distances to the OTHER rows of `points` (exact neighbours; min(3, P-1) of them when P < 4, 0 for P == 1).
    Equal to `knn_dist2(points)[first_query:]` bit for bit."""
    if not isinstance(points, torch.Tensor) or not points.is_cuda:
        raise _gsr.GsrError("simple_knn needs a tensor on the HIP device (no CPU path)")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points: expected [P, 3], got {tuple(points.shape)}")
    pts = points.detach().float().contiguous()
    P, first = int(pts.shape[0]), int(first_query)
    if P == 0 and first == 0:
        return torch.empty(0, dtype=torch.float32, device=pts.device)
    if not 0 <= first < P:
        raise ValueError(f"first_query={first_query}: expected a row of the {P} points")
    lib = _gsr.lib()
    out = torch.empty(P - first, dtype=torch.float32, device=pts.device)
    with _gsr.on_device(pts.device):
        ws = torch.empty(lib.gsr_knn_workspace_bytes(P), dtype=torch.uint8, device=pts.device)
        _gsr.check(lib.gsr_knn_dist2(P, _gsr.ptr(pts), first, _gsr.ptr(out), _gsr.ptr(ws), ws.numel(), _gsr._stream()))
    return out


KNN_K_MAX = 32      # GSR_KNN_K_MAX of include/gsr.h


def knn_k(points, k, return_dist2=True, return_mean=False):
    """points [P,3] float on the HIP device, 1 <= k <= 32.  With k_eff = min(k, P - 1):
    dist2 [P,k] float32: per row the k_eff smallest squared distances to the OTHER rows, ascending, then +inf;
    mean [P] float32: (sum of their square roots) / (k_eff + 1) - the point itself counts at distance 0, as in a neighbour search
    that returns the query; root and sum in float64 on the device, rounded once.  P == 1 gives 0.
    Exact neighbours, the float32 distances of `knn_dist2` (k = 3: the three values whose mean it returns).  A row with a
    non-finite coordinate gets +inf / NaN and is nobody's neighbour.  Returns dist2, mean, or (dist2, mean) as asked."""
    from scene_utils._args import integer
    k = integer("k", k, 1, KNN_K_MAX)
    if not (return_dist2 or return_mean):
        raise ValueError("knn_k: nothing asked for (return_dist2 and return_mean both False)")
    if not isinstance(points, torch.Tensor) or not points.is_cuda:
        raise _gsr.GsrError("simple_knn needs a tensor on the HIP device (no CPU path)")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points: expected [P, 3], got {tuple(points.shape)}")
    pts = points.detach().float().contiguous()
    P = int(pts.shape[0])
    dist2 = torch.empty((P, k), dtype=torch.float32, device=pts.device) if return_dist2 else None
    mean = torch.empty(P, dtype=torch.float32, device=pts.device) if return_mean else None
    if P > 0:
        lib = _gsr.lib()
        with _gsr.on_device(pts.device):
            ws = torch.empty(lib.gsr_knn_k_workspace_bytes(P), dtype=torch.uint8, device=pts.device)
            _gsr.check(lib.gsr_knn_k(P, _gsr.ptr(pts), k, _gsr.ptr(dist2), _gsr.ptr(mean), _gsr.ptr(ws), ws.numel(),
                                     _gsr._stream()))
    if return_dist2 and return_mean:
        return dist2, mean
    return dist2 if return_dist2 else mean


def distCUDA2(points):
    """reference scene/gaussian_model.py:140: mean squared distance of every point to its three nearest neighbours."""
    return knn_dist2(points, 0)


def nn_search(query, target, transform=None, max_distance=math.inf):
    """-> (idx int32 [P], dist2 float32 [P]): for every row of `query` (moved by the [4,4] `transform`, None = identity) the row of
    its nearest point of `target` and the squared distance; -1 / +inf beyond `max_distance`.  `scene_utils.NeighborIndex` keeps
    the structure over `target` for repeated searches."""
    from scene_utils.registration import nn_search as _nn_search
    return _nn_search(query, target, transform, max_distance)


def estimate_normals(points, radius=0.1, max_nn=30, viewpoint=None, return_stats=False):
    """-> normals float32 [P,3] (with return_stats also count int32 [P] and eigenvalues float32 [P,3]): the covariance normal of
    the rows within `radius`, cut at the max_nn nearest - `scene_utils.estimate_normals`."""
    from scene_utils.pointcloud import estimate_normals as _estimate_normals
    return _estimate_normals(points, radius, max_nn, viewpoint, return_stats)


def compute_fpfh(points, normals, radius, max_nn=0, return_stats=False):
    """-> fpfh float32 [P,33] (with return_stats also spfh_counts int32 [P,33] and count int32 [P]): the fast point feature
    histogram of every row over the rows within `radius` (max_nn > 0: cut at the max_nn nearest) -
    `scene_utils.compute_fpfh_feature`."""
    from scene_utils.registration import compute_fpfh_feature as _compute_fpfh_feature
    return _compute_fpfh_feature(points, normals, radius, max_nn, return_stats)


def estimate_color_gradients(points, colors, normals, radius, max_nn=30, return_stats=False):
    """float32 [P,3]: per row the gradient of the intensity (r + g + b) / 3 over its tangent plane, from the neighbourhood of
    `estimate_normals` - `scene_utils.estimate_color_gradients`."""
    from scene_utils.pointcloud import estimate_color_gradients as _estimate_color_gradients
    return _estimate_color_gradients(points, colors, normals, radius, max_nn, return_stats)
