"""Conditioning of a sensor point cloud before it seeds Gaussians: voxel-grid down-sampling and the statistical outlier filter -
the reference's process_point_cloud (submodules/ros_workspace/src/gs_slam_msgs/scripts/pointcloud_pcd.py:163-209:
voxel_down_sample, then remove_statistical_outlier, both Open3D there) - and surface normals, the reference's estimate_normals
calls (convert_visual_merged_msg.py:181, :193-196, :348).  Everything runs in HIP (csrc/pointcloud.hip, csrc/normals.hip, the
neighbour search of csrc/knn.hip); there is no CPU path.  Arguments are validated before any device work."""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _args as A

NB_NEIGHBORS_MAX = 33      # GSR_KNN_K_MAX + 1: the point itself counts among its nb_neighbors


def _check_origin(origin):
    if origin is None:
        return None
    if isinstance(origin, torch.Tensor):
        origin = origin.detach().cpu().tolist()
    o = [float(v) for v in origin]
    if len(o) != 3 or not all(math.isfinite(v) for v in o):
        raise ValueError(f"origin={origin!r}: expected three finite values")
    return o


def _check_filter(nb_neighbors, std_ratio):
    return A.integer("nb_neighbors", nb_neighbors, 2, NB_NEIGHBORS_MAX), \
        A.number("std_ratio", std_ratio, math.isfinite, "a finite value")


def _check_normals(radius, max_nn, viewpoint=None):
    r, nn = A.neighbourhood(radius, max_nn, 3, NB_NEIGHBORS_MAX)
    if viewpoint is not None:
        if isinstance(viewpoint, torch.Tensor):
            viewpoint = viewpoint.detach().cpu().tolist()
        try:
            viewpoint = [float(c) for c in viewpoint]
        except TypeError:
            raise TypeError(f"viewpoint={viewpoint!r}: expected three numbers") from None
        if len(viewpoint) != 3 or not all(math.isfinite(c) for c in viewpoint):
            raise ValueError(f"viewpoint={viewpoint!r}: expected three finite values")
    return r, nn, viewpoint


def check_conditioning(voxel_size, origin, nb_neighbors, std_ratio):
    """the arguments of condition_point_cloud (None skips a stage), also for the mapping hooks that pass them through"""
    if voxel_size is not None:
        A.voxel_size(voxel_size)
        _check_origin(origin)
    if nb_neighbors is not None:
        _check_filter(nb_neighbors, std_ratio)


def voxel_down_sample(points, colors=None, voxel_size=0.05, origin=None, return_counts=False):
    """One averaged point per occupied voxel -> (points [V,3], colors [V,3] or None), with `return_counts` also the int32 [V]
    number of points of every voxel.  Rows in ascending (i_z, i_y, i_x).  The lattice starts at `origin` (three values: successive
    keyframes that pass the same origin share one world-anchored lattice) or, by default, at min - voxel_size / 2 of the cloud;
    the cell index floor((p - o) / voxel_size) is float32 arithmetic, one rounding per operation.  Rows with a non-finite
    coordinate are dropped.  A cell index outside [-2^20, 2^20) raises ValueError.  One read-back (the voxel count and status)."""
    v, o = A.voxel_size(voxel_size), _check_origin(origin)
    pts, col = A.cloud(points, colors, "voxel_down_sample")
    _C = A.gsr()
    P, dev = int(pts.shape[0]), pts.device
    out_p = torch.empty((P, 3), dtype=torch.float32, device=dev)
    out_c = torch.empty((P, 3), dtype=torch.float32, device=dev) if col is not None else None
    out_n = torch.empty(P, dtype=torch.int32, device=dev) if return_counts else None
    n = 0
    if P > 0:
        lib = _C.lib()
        count = torch.zeros(2, dtype=torch.int64, device=dev)
        org = (C.c_float * 3)(*o) if o is not None else None
        with _C.on_device(dev):
            ws = torch.empty(lib.gsr_voxel_workspace_bytes(P), dtype=torch.uint8, device=dev)
            _C.check(lib.gsr_voxel_down_sample(P, _C.ptr(pts), _C.ptr(col), v, org, _C.ptr(out_p), _C.ptr(out_c), _C.ptr(out_n), P,
                                               _C.ptr(count), _C.ptr(ws), ws.numel(), _C._stream()))
        n, status = (int(x) for x in count.tolist())
        if status != 0:
            raise ValueError(f"voxel_down_sample: a cell index leaves [-2^20, 2^20) with voxel_size={v} (origin={o})")
    res = (out_p[:n], out_c[:n] if out_c is not None else None)
    return res + (out_n[:n],) if return_counts else res


def statistical_outlier_mask(points, nb_neighbors=20, std_ratio=2.0, return_stats=False):
    """bool [P]: True for the rows a statistical outlier filter keeps.  Per row the mean distance to its nb_neighbors nearest
    rows, itself included at distance 0 (simple_knn.knn_k with k = nb_neighbors - 1, return_mean); kept iff that mean is > 0 and
    < mu + std_ratio sigma, mu and sigma (n - 1 in the divisor) taken over the rows with finite coordinates in float64 on the
    device.  Rows with a non-finite coordinate are not kept.  `return_stats`: also a float64 [4] device tensor
    (n_valid, mu, sigma, threshold) - no read-back happens here."""
    nb, ratio = _check_filter(nb_neighbors, std_ratio)
    pts, _ = A.cloud(points, None, "statistical_outlier_mask")
    _C = A.gsr()
    P, dev = int(pts.shape[0]), pts.device
    keep = torch.zeros(P, dtype=torch.uint8, device=dev)
    stats = torch.zeros(4, dtype=torch.float64, device=dev)
    if P > 0:
        lib = _C.lib()
        with _C.on_device(dev):
            ws = torch.empty(lib.gsr_outlier_workspace_bytes(P), dtype=torch.uint8, device=dev)
            _C.check(lib.gsr_statistical_outliers(P, _C.ptr(pts), nb, ratio, _C.ptr(keep), None, _C.ptr(stats), _C.ptr(ws),
                                                  ws.numel(), _C._stream()))
    return (keep.bool(), stats) if return_stats else keep.bool()


def remove_statistical_outliers(points, colors=None, nb_neighbors=20, std_ratio=2.0):
    """-> (points, colors or None, kept_index): the rows statistical_outlier_mask keeps, in their order, and their int64 row
    numbers."""
    nb, ratio = _check_filter(nb_neighbors, std_ratio)
    pts, col = A.cloud(points, colors, "remove_statistical_outliers")
    idx = torch.nonzero(statistical_outlier_mask(pts, nb, ratio)).view(-1)
    return pts[idx], (col[idx] if col is not None else None), idx


def condition_point_cloud(points, colors, voxel_size=0.05, nb_neighbors=20, std_ratio=2.0, origin=None):
    """The reference's process_point_cloud: voxel_down_sample, then remove_statistical_outliers -> (points, colors).
    voxel_size=None / nb_neighbors=None skips that stage."""
    check_conditioning(voxel_size, origin, nb_neighbors, std_ratio)
    pts, col = A.cloud(points, colors, "condition_point_cloud")
    if voxel_size is not None:
        pts, col = voxel_down_sample(pts, col, voxel_size, origin)
    if nb_neighbors is not None:
        pts, col, _ = remove_statistical_outliers(pts, col, nb_neighbors, std_ratio)
    return pts, col


def estimate_normals(points, radius=0.1, max_nn=30, viewpoint=None, return_stats=False):
    """float32 [P,3] on the device: per row the unit normal of the plane through its hybrid neighbourhood - the rows within
    `radius` (inf: no limit), cut at the max_nn nearest, the point itself counted (Open3D's KDTreeSearchParamHybrid; rows tied at
    the cut-off distance are all kept) - the eigenvector of the smallest eigenvalue of their covariance, in float64 on the device
    (include/gsr.h gsr_estimate_normals).  Sign: towards `viewpoint` (three values) or, without one, the component of largest
    magnitude positive.  Fewer than three rows in the neighbourhood: (0, 0, 1).  A row with a non-finite coordinate: NaN.
    `return_stats`: also (count int32 [P], the neighbourhood's size; eigenvalues float32 [P,3], ascending).  No read-back."""
    r, nn, v = _check_normals(radius, max_nn, viewpoint)
    pts, _ = A.cloud(points, None, "estimate_normals")
    _C = A.gsr()
    P, dev = int(pts.shape[0]), pts.device
    normals = torch.empty((P, 3), dtype=torch.float32, device=dev)
    count = torch.empty(P, dtype=torch.int32, device=dev) if return_stats else None
    eig = torch.empty((P, 3), dtype=torch.float32, device=dev) if return_stats else None
    if P > 0:
        lib = _C.lib()
        view = (C.c_float * 3)(*v) if v is not None else None
        with _C.on_device(dev):
            ws = torch.empty(lib.gsr_normals_workspace_bytes(P), dtype=torch.uint8, device=dev)
            _C.check(lib.gsr_estimate_normals(P, _C.ptr(pts), r, nn, view, _C.ptr(normals), _C.ptr(count), _C.ptr(eig), _C.ptr(ws),
                                              ws.numel(), _C._stream()))
    return (normals, count, eig) if return_stats else normals


GRADIENT_STATUS = ("solved", "fewer than four rows", "rejected pivot", "masked")      # status codes 0 .. 3 of gsr_color_gradient
ROW_PER_POINT = ", one row per point"      # how a ValueError for per-point normals, colours or gradients ends


def estimate_color_gradients(points, colors, normals, radius, max_nn=30, return_stats=False):
    """float32 [P,3] on the device: per row the gradient of the intensity (r + g + b) / 3 over the tangent plane of its normal -
    what Open3D's registration_colored_icp prepares on the target (include/gsr.h gsr_color_gradient).  The neighbourhood is
    estimate_normals' (radius, cut at the max_nn nearest, the point itself counted, ties all kept), max_nn 4 .. 33; the
    least-squares fit of the members' intensity differences over their tangential offsets, with the constraint that the gradient
    has no component along the normal, in float64 on the device.  Fewer than four rows, or a neighbourhood that does not fix the
    gradient (collinear rows): 0.  A row with a non-finite point, colour or normal: NaN, and nobody's neighbour.
    `return_stats`: also (count int32 [P], the neighbourhood's size; status uint8 [P]: 0 solved, 1 fewer than four rows, 2
    rejected pivot, 3 masked).  No read-back."""
    r, nn = A.neighbourhood(radius, max_nn, 4, NB_NEIGHBORS_MAX)      # (Open3D solves from four rows on)
    if colors is None:
        raise ValueError("colors: expected a floating-point tensor of shape (P, 3), one row per point")
    rows = A.rows(points)
    nrm = A.tensor(normals, "normals", ("P" if rows is None else rows, 3), ROW_PER_POINT)
    pts, col = A.cloud(points, colors, "estimate_color_gradients")
    _C = A.gsr()
    P, dev = int(pts.shape[0]), pts.device
    grad = torch.empty((P, 3), dtype=torch.float32, device=dev)
    count = torch.empty(P, dtype=torch.int32, device=dev) if return_stats else None
    status = torch.empty(P, dtype=torch.uint8, device=dev) if return_stats else None
    if P > 0:
        lib = _C.lib()
        nrm = nrm.to(dev)
        with _C.on_device(dev):
            ws = torch.empty(lib.gsr_color_gradient_workspace_bytes(P), dtype=torch.uint8, device=dev)
            _C.check(lib.gsr_color_gradient(P, _C.ptr(pts), _C.ptr(col), _C.ptr(nrm), r, nn, _C.ptr(grad), _C.ptr(count),
                                            _C.ptr(status), _C.ptr(ws), ws.numel(), _C._stream()))
    return (grad, count, status) if return_stats else grad
