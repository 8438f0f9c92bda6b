"""Conditioning of a sensor point cloud before it seeds Gaussians: voxel-grid down-sampling and the statistical outlier filter -
the reference's process_point_cloud (submodules/ros_workspace/src/gs_slam_msgs/scripts/pointcloud_pcd.py:163-209:
voxel_down_sample, then remove_statistical_outlier, both Open3D there) - and surface normals, the reference's estimate_normals
calls (convert_visual_merged_msg.py:181, :193-196, :348).  Everything runs in HIP (csrc/pointcloud.hip, csrc/normals.hip, the
neighbour search of csrc/knn.hip); there is no CPU path.  Arguments are validated before any device work."""
from __future__ import annotations

import ctypes as C
import math
import numbers

import torch

NB_NEIGHBORS_MAX = 33      # GSR_KNN_K_MAX + 1: the point itself counts among its nb_neighbors


def _gsr():
    from diff_gaussian_rasterization import _C
    return _C


def _check_voxel_size(voxel_size):
    if isinstance(voxel_size, bool) or not isinstance(voxel_size, numbers.Real):
        raise TypeError(f"voxel_size={voxel_size!r}: expected a number")
    if not (math.isfinite(voxel_size) and voxel_size > 0):
        raise ValueError(f"voxel_size={voxel_size}: expected a finite value > 0")
    return float(voxel_size)


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
    if isinstance(nb_neighbors, bool) or not isinstance(nb_neighbors, numbers.Integral):
        raise TypeError(f"nb_neighbors={nb_neighbors!r}: expected an int")
    if not 2 <= nb_neighbors <= NB_NEIGHBORS_MAX:
        raise ValueError(f"nb_neighbors={nb_neighbors}: expected 2 .. {NB_NEIGHBORS_MAX}")
    if isinstance(std_ratio, bool) or not isinstance(std_ratio, numbers.Real):
        raise TypeError(f"std_ratio={std_ratio!r}: expected a number")
    if not math.isfinite(std_ratio):
        raise ValueError(f"std_ratio={std_ratio}: expected a finite value")
    return int(nb_neighbors), float(std_ratio)


def _check_normals(radius, max_nn, viewpoint=None):
    if isinstance(radius, bool) or not isinstance(radius, numbers.Real):
        raise TypeError(f"radius={radius!r}: expected a number")
    if math.isnan(radius) or not radius > 0:
        raise ValueError(f"radius={radius}: expected a value > 0 (inf: limited by max_nn only)")
    if isinstance(max_nn, bool) or not isinstance(max_nn, numbers.Integral):
        raise TypeError(f"max_nn={max_nn!r}: expected an int")
    if not 3 <= max_nn <= NB_NEIGHBORS_MAX:
        raise ValueError(f"max_nn={max_nn}: expected 3 .. {NB_NEIGHBORS_MAX}")
    if viewpoint is not None:
        if isinstance(viewpoint, torch.Tensor):
            viewpoint = viewpoint.detach().cpu().tolist()
        try:
            viewpoint = [float(c) for c in viewpoint]
        except TypeError:
            raise TypeError(f"viewpoint={viewpoint!r}: expected three numbers") from None
        if len(viewpoint) != 3 or not all(math.isfinite(c) for c in viewpoint):
            raise ValueError(f"viewpoint={viewpoint!r}: expected three finite values")
    return float(radius), int(max_nn), viewpoint


def _check_conditioning(voxel_size, origin, nb_neighbors, std_ratio):
    """the arguments of condition_point_cloud (None skips a stage), also for the mapping hooks that pass them through"""
    if voxel_size is not None:
        _check_voxel_size(voxel_size)
        _check_origin(origin)
    if nb_neighbors is not None:
        _check_filter(nb_neighbors, std_ratio)


def _check_cloud(points, colors, who):
    if not isinstance(points, torch.Tensor) or not points.is_cuda:
        raise _gsr().GsrError(f"{who} needs points on the HIP device (no CPU path)")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points: expected [P, 3], got {tuple(points.shape)}")
    pts = points.detach().float().contiguous()
    col = None
    if colors is not None:
        if not isinstance(colors, torch.Tensor) or not colors.is_cuda:
            raise _gsr().GsrError(f"{who} needs colors on the HIP device (no CPU path)")
        if tuple(colors.shape) != tuple(points.shape):
            raise ValueError(f"colors: expected {tuple(points.shape)} like points, got {tuple(colors.shape)}")
        col = colors.detach().float().to(pts.device).contiguous()
    return pts, col


def voxel_down_sample(points, colors=None, voxel_size=0.05, origin=None, return_counts=False):
    """One averaged point per occupied voxel -> (points [V,3], colors [V,3] or None), with `return_counts` also the int32 [V]
    number of points of every voxel.  Rows in ascending (i_z, i_y, i_x).  The lattice starts at `origin` (three values: successive
    keyframes that pass the same origin share one world-anchored lattice) or, by default, at min - voxel_size / 2 of the cloud;
    the cell index floor((p - o) / voxel_size) is float32 arithmetic, one rounding per operation.  Rows with a non-finite
    coordinate are dropped.  A cell index outside [-2^20, 2^20) raises ValueError.  One read-back (the voxel count and status)."""
    v, o = _check_voxel_size(voxel_size), _check_origin(origin)
    pts, col = _check_cloud(points, colors, "voxel_down_sample")
    _C = _gsr()
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
    pts, _ = _check_cloud(points, None, "statistical_outlier_mask")
    _C = _gsr()
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
    pts, col = _check_cloud(points, colors, "remove_statistical_outliers")
    idx = torch.nonzero(statistical_outlier_mask(pts, nb, ratio)).view(-1)
    return pts[idx], (col[idx] if col is not None else None), idx


def condition_point_cloud(points, colors, voxel_size=0.05, nb_neighbors=20, std_ratio=2.0, origin=None):
    """The reference's process_point_cloud: voxel_down_sample, then remove_statistical_outliers -> (points, colors).
    voxel_size=None / nb_neighbors=None skips that stage."""
    _check_conditioning(voxel_size, origin, nb_neighbors, std_ratio)
    pts, col = _check_cloud(points, colors, "condition_point_cloud")
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
    pts, _ = _check_cloud(points, None, "estimate_normals")
    _C = _gsr()
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


def _check_gradient(radius, max_nn, names=("radius", "max_nn")):
    """the neighbourhood of estimate_color_gradients: _check_normals' rules with max_nn >= 4 (Open3D solves from four rows on)"""
    if isinstance(radius, bool) or not isinstance(radius, numbers.Real):
        raise TypeError(f"{names[0]}={radius!r}: expected a number")
    if math.isnan(radius) or not radius > 0:
        raise ValueError(f"{names[0]}={radius}: expected a value > 0 (inf: limited by {names[1]} only)")
    if isinstance(max_nn, bool) or not isinstance(max_nn, numbers.Integral):
        raise TypeError(f"{names[1]}={max_nn!r}: expected an int")
    if not 4 <= max_nn <= NB_NEIGHBORS_MAX:
        raise ValueError(f"{names[1]}={max_nn}: expected 4 .. {NB_NEIGHBORS_MAX}")
    return float(radius), int(max_nn)


def _check_rows3_shape(t, name, rows=None):
    if not isinstance(t, torch.Tensor) or not t.is_floating_point() or t.dim() != 2 or t.shape[1] != 3 or \
            (rows is not None and int(t.shape[0]) != rows):
        raise ValueError(f"{name}: expected a floating-point tensor of shape ({'P' if rows is None else rows}, 3), one row per point")


def _check_rows3(t, name, rows=None):
    """a floating-point [rows,3] tensor on the HIP device -> contiguous float32; type and shape first"""
    _check_rows3_shape(t, name, rows)
    if not t.is_cuda:
        raise _gsr().GsrError(f"{name} must live on the HIP device (no CPU path)")
    return t.detach().float().contiguous()


def estimate_color_gradients(points, colors, normals, radius, max_nn=30, return_stats=False):
    """float32 [P,3] on the device: per row the gradient of the intensity (r + g + b) / 3 over the tangent plane of its normal -
    what Open3D's registration_colored_icp prepares on the target (include/gsr.h gsr_color_gradient).  The neighbourhood is
    estimate_normals' (radius, cut at the max_nn nearest, the point itself counted, ties all kept), max_nn 4 .. 33; the
    least-squares fit of the members' intensity differences over their tangential offsets, with the constraint that the gradient
    has no component along the normal, in float64 on the device.  Fewer than four rows, or a neighbourhood that does not fix the
    gradient (collinear rows): 0.  A row with a non-finite point, colour or normal: NaN, and nobody's neighbour.
    `return_stats`: also (count int32 [P], the neighbourhood's size; status uint8 [P]: 0 solved, 1 fewer than four rows, 2
    rejected pivot, 3 masked).  No read-back."""
    r, nn = _check_gradient(radius, max_nn)
    rows = int(points.shape[0]) if isinstance(points, torch.Tensor) and points.dim() == 2 else None
    if colors is None:
        raise ValueError("colors: expected a floating-point tensor of shape (P, 3), one row per point")
    nrm = _check_rows3(normals, "normals", rows)
    pts, col = _check_cloud(points, colors, "estimate_color_gradients")
    _C = _gsr()
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
