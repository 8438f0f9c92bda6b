"""Generalized ICP (Segal, Haehnel, Thrun 2009; Open3D's registration_generalized_icp): a covariance per point on BOTH clouds,
every pair weighted by the inverse of M = Sigma_t + R Sigma_s R^T.  Flat covariances on both sides make it plane-to-plane;
isotropic ones make it point-to-point, so its 6 x 6 system stays solvable on a single plane, where point-to-plane's does not; the
covariances of a Gaussian map as the target's register a scan to the map with the map's own shapes (`register_scan_to_map`).
Everything runs in HIP (csrc/gicp.hip; the search, the loop and the stopping rule are registration_icp's); there is no CPU path.
Arguments are validated before any device work.

A covariance is six float32 per row - xx, xy, xz, yy, yz, zz - the layout of `GaussianModel.get_covariance`."""
from __future__ import annotations

import torch

from . import _args as A
from .pointcloud import NB_NEIGHBORS_MAX
from .registration import USE_QUERY_ORDER, NeighborIndex, RegistrationResult, _check_distance, _check_icp, _evaluate, prepare

EPSILON = 1e-3      # Open3D's default: the extent given to a surface along its normal, against 1 across it


def _check_epsilon(epsilon):
    return A.number("epsilon", epsilon, lambda v: 0.0 < v <= 1.0, "a value > 0 and <= 1")      # (false for NaN)


def _check_cov(cov, name, rows, convert=True):
    """A.tensor of [rows,6] (rows=None: any number)"""
    return A.tensor(cov, name, ("P" if rows is None else rows, 6), ", one row of xx, xy, xz, yy, yz, zz per point", convert=convert)


def _check_idx(idx, rows):
    if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int32 or tuple(idx.shape) != (rows,):
        raise ValueError(f"correspondences: expected an int32 tensor of shape ({rows},)")
    return idx


def estimate_covariances(points, radius, max_nn=20, epsilon=EPSILON, return_count=False):
    """float32 [P,6] on the device: per row the regularised covariance of its hybrid neighbourhood - estimate_normals' rows (within
    `radius`, cut at the max_nn nearest, the point itself counted, ties all kept), their covariance in float64, and with n its
    eigenvector of the smallest eigenvalue Sigma = I - (1 - epsilon) n n^T: extent `epsilon` along the normal, 1 across it (include/gsr.h
    gsr_estimate_covariances).  Fewer than three rows in the neighbourhood: I (the row then pulls as a point-to-point pair does).
    A row with a non-finite coordinate: NaN.  `return_count`: also count int32 [P], the neighbourhood's size.  No read-back."""
    r, nn = A.neighbourhood(radius, max_nn, 3, NB_NEIGHBORS_MAX)
    eps = _check_epsilon(epsilon)
    pts, _ = A.cloud(points, None, "estimate_covariances")
    _C = A.gsr()
    P, dev = int(pts.shape[0]), pts.device
    cov = torch.empty((P, 6), dtype=torch.float32, device=dev)
    count = torch.empty(P, dtype=torch.int32, device=dev) if return_count else None
    if P > 0:
        lib = _C.lib()
        with _C.on_device(dev):
            ws = torch.empty(lib.gsr_covariance_workspace_bytes(P), dtype=torch.uint8, device=dev)
            _C.check(lib.gsr_estimate_covariances(P, _C.ptr(pts), r, nn, eps, _C.ptr(cov), _C.ptr(count), _C.ptr(ws), ws.numel(),
                                                  _C._stream()))
    return (cov, count) if return_count else cov


def regularize_covariances(covariances, epsilon=EPSILON):
    """float32 [P,6] on the device: every given covariance keeps its direction of least extent n and becomes I - (1 - epsilon) n n^T
    (include/gsr.h gsr_regularize_covariances) - what makes the covariances of a Gaussian map comparable with estimated ones.  A
    multiple of the identity: I.  A row with a non-finite entry: NaN.  The input is not changed.  No read-back."""
    eps = _check_epsilon(epsilon)
    cov = _check_cov(covariances, "covariances", None)
    P = int(cov.shape[0])
    out = torch.empty_like(cov)
    if P > 0:
        _C = A.gsr()
        with _C.on_device(cov.device):
            _C.check(_C.lib().gsr_regularize_covariances(P, _C.ptr(cov), eps, _C.ptr(out), _C._stream()))
    return out


class _GeneralizedUpdater:
    """gsr_icp_update_generalized on fixed clouds and covariances: the workspace is allocated once (registration._Updater's
    pattern and call signature)"""

    def __init__(self, src, scov, tgt, tcov):
        _C = A.gsr()
        self.src, self.scov, self.tgt, self.tcov = src, scov, tgt, tcov
        with _C.on_device(src.device):
            self.ws = torch.empty(_C.lib().gsr_icp_generalized_workspace_bytes(int(src.shape[0])), dtype=torch.uint8,
                                  device=src.device)

    def __call__(self, idx, Td, stats):
        _C = A.gsr()
        with _C.on_device(self.src.device):
            _C.check(_C.lib().gsr_icp_update_generalized(int(self.src.shape[0]), _C.ptr(self.src), _C.ptr(self.scov),
                                                         int(self.tgt.shape[0]), _C.ptr(self.tgt), _C.ptr(self.tcov), _C.ptr(idx),
                                                         _C.ptr(Td), _C.ptr(stats), _C.ptr(self.ws), self.ws.numel(), _C._stream()))


def gicp_update(source, source_covariances, target, target_covariances, correspondences, transformation):
    """One generalized ICP update from given correspondences (int32 [Ps], -1 = none) -> (new transformation float64 [4,4] on the
    device, stats float64 [8] on the device: n, fitness, inlier_rmse (Euclidean), status, sum |d|^2, sum d^T W d, 0, 0; include/gsr.h
    gsr_icp_update_generalized).  The covariances ([Ps,6], [Pt,6]) are used as given.  A row with a non-finite covariance on either
    side, or whose combined covariance has no positive determinant, takes no part.  n, fitness and inlier_rmse describe the
    transformation that was passed in; status 1 below six rows, 2 when they do not fix all six unknowns.  No read-back."""
    T = A.transform(transformation)
    _check_cov(source_covariances, "source_covariances", A.rows(source), convert=False)      # (every shape before any device check)
    _check_cov(target_covariances, "target_covariances", A.rows(target), convert=False)
    scov = _check_cov(source_covariances, "source_covariances", A.rows(source))
    tcov = _check_cov(target_covariances, "target_covariances", A.rows(target))
    src, _ = A.cloud(source, None, "gicp_update")
    tgt, _ = A.cloud(target, None, "gicp_update")
    A.nonempty(src, "gicp_update", "source")
    A.nonempty(tgt, "gicp_update", "target")
    idx = _check_idx(correspondences, int(src.shape[0]))
    dev = src.device
    Td = A.device_T(T, dev)
    stats = torch.zeros(8, dtype=torch.float64, device=dev)
    _GeneralizedUpdater(src, scov.to(dev), tgt.to(dev), tcov.to(dev))(idx.to(dev).contiguous(), Td, stats)
    return Td, stats


def _check_sides(who, source_covariances, target_covariances, covariance_radius, covariance_max_nn):
    """each side brings its covariances or has them estimated: the radius serves the sides that bring none"""
    missing = [side for side, cov in (("source", source_covariances), ("target", target_covariances)) if cov is None]
    if missing and covariance_radius is None:
        raise ValueError(f"{who}: neither {missing[0]}_covariances nor covariance_radius given - pass the covariances or have them "
                         "estimated")
    if not missing and covariance_radius is not None:
        raise ValueError(f"{who}: source_covariances, target_covariances and covariance_radius all given - pass the covariances or "
                         "have them estimated")
    if covariance_radius is not None:
        A.neighbourhood(covariance_radius, covariance_max_nn, 3, NB_NEIGHBORS_MAX, ("covariance_radius", "covariance_max_nn"))


def registration_generalized_icp(source, target, max_correspondence_distance, init=None, source_covariances=None,
                                 target_covariances=None, covariance_radius=None, covariance_max_nn=20, epsilon=EPSILON,
                                 relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30, check_every=1, index=None,
                                 use_order=None):
    """Generalized ICP of `source` onto `target` (both [P,3] float on the HIP device) from `init` (None = identity) ->
    RegistrationResult.  The loop, the stopping rule, the closing search, `check_every`, `index` and `use_order` are
    registration_icp's; the update is gicp_update's.  Fitness and RMSE are the Euclidean ones.
    Each side either brings its covariances ([P,6]: used AS GIVEN, not regularised - regularize_covariances is the caller's to
    apply) or has them estimated once with estimate_covariances(covariance_radius, covariance_max_nn, epsilon); a side with both,
    or with neither, is a ValueError.  An iteration with fewer than six usable rows, or whose rows do not fix all six unknowns,
    leaves the transformation as it is."""
    who = "registration_generalized_icp"
    _check_icp(relative_fitness, relative_rmse, max_iteration, check_every)
    eps = _check_epsilon(epsilon)
    A.transform(init, "init")
    _check_sides(who, source_covariances, target_covariances, covariance_radius, covariance_max_nn)
    target_rows = index.size if isinstance(index, NeighborIndex) else A.rows(target)
    for cov, name, rows in ((source_covariances, "source_covariances", A.rows(source)),
                            (target_covariances, "target_covariances", target_rows)):      # (every shape before any device check)
        if cov is not None:
            _check_cov(cov, name, rows, convert=False)
    scov = None if source_covariances is None else _check_cov(source_covariances, "source_covariances", A.rows(source))
    tcov = None if target_covariances is None else _check_cov(target_covariances, "target_covariances", target_rows)
    src, index, md2, T = prepare(source, target, max_correspondence_distance, init, index, who)
    dev, P = src.device, int(src.shape[0])
    Td = A.device_T(T, dev)
    order = index.query_order(src, Td) if (USE_QUERY_ORDER if use_order is None else use_order) else None
    if scov is None:
        scov = estimate_covariances(src, covariance_radius, covariance_max_nn, eps)
    if tcov is None:
        tcov = estimate_covariances(index.points, covariance_radius, covariance_max_nn, eps)
    updater = _GeneralizedUpdater(src, scov.to(dev), index.points, tcov.to(dev))
    idx = torch.empty(P, dtype=torch.int32, device=dev)
    stats = torch.zeros((max_iteration, 8), dtype=torch.float64, device=dev)
    iterations, converged = 0, False
    for k in range(max_iteration):
        index._search(src, Td, md2, order, idx, None)
        updater(idx, Td, stats[k])
        iterations = k + 1
        if check_every and k >= 1 and (k + 1) % check_every == 0:
            prev, cur = stats[k - 1:k + 1, 1:3].tolist()
            if abs(cur[0] - prev[0]) < relative_fitness and abs(cur[1] - prev[1]) < relative_rmse:
                converged = True
                break
    fitness, rmse, idx = _evaluate(src, index, md2, Td, order, updater)
    return RegistrationResult(Td, fitness, rmse, iterations, converged, idx)


# what register_scan_to_map hands on; the covariances and the index are its own to decide
_SCAN_TO_MAP_PASSED_ON = ("covariance_max_nn", "relative_fitness", "relative_rmse", "max_iteration", "check_every", "use_order")


def register_scan_to_map(model, points, max_correspondence_distance, init=None, ids=None, covariance_radius=None, epsilon=EPSILON,
                         **icp):
    """Registers a scan (`points` [P,3] float on the HIP device) to a Gaussian map with the map's own shapes -> RegistrationResult
    with x_map ~ T x_scan: what corrects a GPS / IMU pose of the scan against the map.  The target is the model's means - with
    `ids`, the rows anchored to those keyframes; the target's covariances are regularize_covariances(model.get_covariance(),
    epsilon), each Gaussian's direction of least extent with the extents (epsilon, 1, 1); the source's are estimated on the scan
    with estimate_covariances(covariance_radius, epsilon=epsilon) (covariance_max_nn may be passed on).  Further keywords go to
    registration_generalized_icp.  The model is not changed: moving the map is align_map's business."""
    who = "register_scan_to_map"
    _check_distance("max_correspondence_distance", max_correspondence_distance, True)
    eps = _check_epsilon(epsilon)
    A.transform(init, "init")
    for k in icp:
        if k not in _SCAN_TO_MAP_PASSED_ON:
            raise TypeError(f"{who}: {k} is not accepted (passed on to registration_generalized_icp: "
                            f"{', '.join(_SCAN_TO_MAP_PASSED_ON)})")
    max_nn = icp.pop("covariance_max_nn", 20)
    _check_icp(icp.get("relative_fitness", 1e-6), icp.get("relative_rmse", 1e-6), icp.get("max_iteration", 30),
               icp.get("check_every", 1))
    if covariance_radius is None:
        raise ValueError(f"{who}: covariance_radius is needed to estimate the scan's covariances")
    A.neighbourhood(covariance_radius, max_nn, 3, NB_NEIGHBORS_MAX, ("covariance_radius", "covariance_max_nn"))
    xyz = getattr(model, "get_xyz", None)
    if not isinstance(xyz, torch.Tensor) or not xyz.is_cuda:
        raise A.gsr().GsrError(f"{who} runs in HIP kernels (no CPU path): the model must live on the HIP device")
    pts, _ = A.cloud(points, None, who)
    if ids is not None:
        ids = [int(i) for i in ids]
        if getattr(model, "_anchor", None) is None:
            raise ValueError(f"{who}: `ids` given but the model has no anchors (set_anchors, add_from_rgbd(anchor=...))")
    with torch.no_grad():
        tgt = xyz.detach()
        cov = model.get_covariance().detach()
        if ids is not None:
            keep = torch.isin(model._anchor.to(tgt.device), torch.tensor(ids, dtype=torch.int32, device=tgt.device))
            tgt, cov = tgt[keep], cov[keep]
        tgt = tgt.float().contiguous()
        tcov = regularize_covariances(cov, eps)
        scov = estimate_covariances(pts, covariance_radius, max_nn, eps)
    return registration_generalized_icp(pts, tgt, max_correspondence_distance, init=init, source_covariances=scov,
                                        target_covariances=tcov, epsilon=eps, **icp)
