"""Rigid registration of one point cloud to another: a nearest-neighbour index with row numbers and ICP, point-to-point (the
default), point-to-plane on the target's normals, or coloured (the plane residual joined with a photometric one: Park, Zhou,
Koltun 2017, Open3D's registration_colored_icp - for floors, walls and roads, where the texture stops the slide) - what the
reference's pointcloud_registeration / pointcloud_registration_gpu (convert_visual_merged_msg.py:187-249, :393-432) do with Open3D
before a message's cloud is merged into the accumulated one.  Everything runs in HIP (csrc/registration.hip over the structure of
csrc/knn.hip); there is no CPU path.  Arguments are validated before any device work.

The transformed point is q = (float32)(R s + t) evaluated in float64 in one fixed order (include/gsr.h), so a float64 restatement
reproduces every query bit for bit; the neighbour is the lexicographic minimum of (float32 d2, target row).

For clouds that are not roughly aligned: FPFH features, feature matching and RANSAC over the matches (csrc/features.hip) - the
lines the reference has commented out at :198-213 - whose result starts ICP (`register_and_merge(global_init=True)`)."""
from __future__ import annotations

import math
from typing import NamedTuple

import torch

from . import _args as A
from .pointcloud import NB_NEIGHBORS_MAX, ROW_PER_POINT, estimate_color_gradients, estimate_normals, voxel_down_sample

USE_QUERY_ORDER = True      # registration_icp Morton-sorts the queries once (profiles/README.md, registration_bench: measured)


class RegistrationResult(NamedTuple):
    transformation: torch.Tensor      # float64 [4,4] on the device: x_target ~ T x_source
    fitness: float                    # valid correspondences / source rows, under `transformation`
    inlier_rmse: float                # sqrt(mean squared distance of the valid correspondences), under `transformation`
    iterations: int                   # ICP updates applied
    converged: bool                   # the stopping rule fired (always False with check_every=0)
    correspondences: torch.Tensor     # int32 [Ps]: target row of every source row under `transformation`, -1 = none


def _check_distance(name, value, allow_inf):
    return A.number(name, value, lambda v: v >= 0 and (allow_inf or not math.isinf(v)),      # (false for NaN)
                    "a value >= 0" + ("" if allow_inf else ", finite"))


def _check_icp(relative_fitness, relative_rmse, max_iteration, check_every):
    for n, v in (("relative_fitness", relative_fitness), ("relative_rmse", relative_rmse)):
        A.number(n, v, lambda v: math.isfinite(v) and v >= 0, "a finite value >= 0")
    A.integer("max_iteration", max_iteration, 1)
    A.integer("check_every", check_every, 0)


ESTIMATIONS = ("point_to_point", "point_to_plane", "colored")
LAMBDA_GEOMETRIC = 0.968      # Open3D's default weight of the geometric residual in the coloured estimator


def _check_estimation(estimation):
    if not isinstance(estimation, str):
        raise TypeError(f"estimation={estimation!r}: expected one of {ESTIMATIONS}")
    if estimation not in ESTIMATIONS:
        raise ValueError(f"estimation={estimation!r}: expected one of {ESTIMATIONS}")
    return estimation


def check_lambda(lambda_geometric):
    return A.number("lambda_geometric", lambda_geometric, lambda v: 0.0 <= v <= 1.0, "0 .. 1")      # (false for NaN)


def _check_rows3(t, name, rows, convert=True):
    """colours or gradients, one row per point: A.tensor of [rows,3] (rows=None: any number)"""
    return A.tensor(t, name, ("P" if rows is None else rows, 3), ROW_PER_POINT, convert=convert)


def _check_target_normals(normals, rows):
    """None, or A.tensor of [rows,3] (rows=None: any number)"""
    return None if normals is None else A.tensor(normals, "target_normals", ("Pt" if rows is None else rows, 3),
                                                 ", one row per target row")


class NeighborIndex:
    """The search structure over a target cloud (points [Pt,3] float on the HIP device), built once.  `query` may then be called
    any number of times; the target's rows keep their numbers."""

    def __init__(self, target):
        pts, _ = A.cloud(target, None, "NeighborIndex")
        A.nonempty(pts, "NeighborIndex", "target")
        _C = A.gsr()
        lib = _C.lib()
        self.points = pts
        self.size = int(pts.shape[0])
        self.device = pts.device
        with _C.on_device(self.device):
            self.blob = torch.empty(lib.gsr_nn_index_bytes(self.size), dtype=torch.uint8, device=self.device)
            _C.check(lib.gsr_nn_index_build(self.size, _C.ptr(pts), _C.ptr(self.blob), self.blob.numel(), _C._stream()))

    def _source(self, points, who):
        pts, _ = A.cloud(points, None, who)
        if pts.device != self.device:
            raise ValueError(f"{who}: points on {pts.device}, the index on {self.device}")
        return pts

    def query_order(self, points, transform=None):
        """int32 [P]: the rows of `points` sorted by the Morton code of T p in the target's bounding box - handed to `query` as
        `order`, it gives the lanes of a wave neighbouring queries.  It never changes an answer."""
        T = A.transform(transform, "transform")
        pts = self._source(points, "NeighborIndex.query_order")
        P = int(pts.shape[0])
        order = torch.empty(P, dtype=torch.int32, device=self.device)
        if P:
            _C = A.gsr()
            lib = _C.lib()
            Td = None if T is None else A.device_T(T, self.device)
            with _C.on_device(self.device):
                ws = torch.empty(lib.gsr_nn_order_workspace_bytes(P), dtype=torch.uint8, device=self.device)
                _C.check(lib.gsr_nn_query_order(self.size, _C.ptr(self.blob), P, _C.ptr(pts), _C.ptr(Td), _C.ptr(order), _C.ptr(ws),
                                                ws.numel(), _C._stream()))
        return order

    def _search(self, pts, Td, max_dist2, order, idx, dist2):
        _C = A.gsr()
        with _C.on_device(self.device):
            _C.check(_C.lib().gsr_nn_search(self.size, _C.ptr(self.blob), int(pts.shape[0]), _C.ptr(pts), _C.ptr(Td), max_dist2,
                                            _C.ptr(order), _C.ptr(idx), _C.ptr(dist2), _C._stream()))

    def query(self, points, transform=None, max_distance=math.inf, order=None):
        """-> (idx int32 [P], dist2 float32 [P]): for every row of `points`, moved by `transform` ([4,4], None = identity), the
        row of its nearest target point and the squared distance; among equal float32 distances the smallest row.  idx = -1 and
        dist2 = +inf where the distance exceeds `max_distance` or the row is not finite."""
        md = _check_distance("max_distance", max_distance, True)
        T = A.transform(transform, "transform")
        pts = self._source(points, "NeighborIndex.query")
        P = int(pts.shape[0])
        if order is not None:
            if not isinstance(order, torch.Tensor) or order.dtype != torch.int32 or tuple(order.shape) != (P,):
                raise ValueError(f"order: expected an int32 tensor of shape ({P},)")
            order = order.to(self.device).contiguous()
        idx = torch.empty(P, dtype=torch.int32, device=self.device)
        dist2 = torch.empty(P, dtype=torch.float32, device=self.device)
        if P:
            self._search(pts, None if T is None else A.device_T(T, self.device), A.sq(md), order, idx, dist2)
        return idx, dist2


def nn_search(query, target, transform=None, max_distance=math.inf):
    """NeighborIndex(target).query(query, ...) in one call (also `simple_knn.nn_search`)."""
    md = _check_distance("max_distance", max_distance, True)
    T = A.transform(transform, "transform")
    return NeighborIndex(target).query(query, T, md)


def transform_points(points, transformation):
    """float32 [P,3]: every row moved by the [4,4] `transformation`, q = (float32)(R p + t) as the search evaluates it."""
    T = A.transform(transformation)
    pts, _ = A.cloud(points, None, "transform_points")
    out = torch.empty_like(pts)
    P = int(pts.shape[0])
    if P:
        _C = A.gsr()
        Td = None if T is None else A.device_T(T, pts.device)
        with _C.on_device(pts.device):
            _C.check(_C.lib().gsr_transform_points(P, _C.ptr(pts), _C.ptr(Td), _C.ptr(out), _C._stream()))
    return out


class _Updater:
    """gsr_icp_update - with the target's normals gsr_icp_update_plane, with `colored` = (source colours, target colours, target
    gradients, lambda_geometric) besides them gsr_icp_update_colored - on fixed clouds: the workspace is allocated once"""

    def __init__(self, src, tgt, normals=None, colored=None):
        _C = A.gsr()
        self.src, self.tgt, self.normals, self.colored = src, tgt, normals, colored
        size = _C.lib().gsr_icp_workspace_bytes if colored is None else _C.lib().gsr_icp_colored_workspace_bytes
        with _C.on_device(src.device):
            self.ws = torch.empty(size(int(src.shape[0])), dtype=torch.uint8, device=src.device)

    def __call__(self, idx, Td, stats):
        _C = A.gsr()
        with _C.on_device(self.src.device):
            if self.colored is not None:
                scol, tcol, grad, lam = self.colored
                _C.check(_C.lib().gsr_icp_update_colored(int(self.src.shape[0]), _C.ptr(self.src), _C.ptr(scol),
                                                         int(self.tgt.shape[0]), _C.ptr(self.tgt), _C.ptr(self.normals),
                                                         _C.ptr(tcol), _C.ptr(grad), _C.ptr(idx), lam, _C.ptr(Td), _C.ptr(stats),
                                                         _C.ptr(self.ws), self.ws.numel(), _C._stream()))
                return
            if self.normals is not None:
                _C.check(_C.lib().gsr_icp_update_plane(int(self.src.shape[0]), _C.ptr(self.src), int(self.tgt.shape[0]),
                                                       _C.ptr(self.tgt), _C.ptr(self.normals), _C.ptr(idx), _C.ptr(Td),
                                                       _C.ptr(stats), _C.ptr(self.ws), self.ws.numel(), _C._stream()))
                return
            _C.check(_C.lib().gsr_icp_update(int(self.src.shape[0]), _C.ptr(self.src), int(self.tgt.shape[0]), _C.ptr(self.tgt),
                                             _C.ptr(idx), _C.ptr(Td), _C.ptr(stats), _C.ptr(self.ws), self.ws.numel(),
                                             _C._stream()))


def icp_update(source, target, correspondences, transformation, target_normals=None, source_colors=None, target_colors=None,
               target_gradients=None, lambda_geometric=LAMBDA_GEOMETRIC):
    """One ICP update from given correspondences (int32 [Ps], -1 = none) -> (new transformation float64 [4,4] on the device,
    stats float64 [8] on the device: n, fitness, inlier_rmse, status, sum of squared distances, ...; include/gsr.h
    gsr_icp_update).  n, fitness and inlier_rmse describe the transformation that was passed in.  No read-back.
    target_normals ([Pt,3] float on the device): the point-to-plane update instead (gsr_icp_update_plane; stats[5] = the sum of
    the squared point-to-plane residuals, status 1 below six correspondences, 2 when they do not fix all six unknowns).
    source_colors ([Ps,3]), target_colors and target_gradients ([Pt,3]; estimate_color_gradients of the target) besides the
    normals: the coloured update (gsr_icp_update_colored; stats[5] and stats[6] = the sums of the squared geometric and
    photometric residuals, unweighted).  Some of the four without the others is a ValueError."""
    T = A.transform(transformation)
    lam = check_lambda(lambda_geometric)
    given = [a is not None for a in (source_colors, target_colors, target_gradients)]
    if any(given) and not (all(given) and target_normals is not None):
        raise ValueError("icp_update: the coloured update needs target_normals, source_colors, target_colors and target_gradients "
                         "together")
    if all(given):      # (every shape before any device check)
        for t, name, rows in ((source_colors, "source_colors", A.rows(source)), (target_colors, "target_colors", A.rows(target)),
                              (target_gradients, "target_gradients", A.rows(target))):
            _check_rows3(t, name, rows, convert=False)
    nrm = _check_target_normals(target_normals, A.rows(target))
    colored = None
    if all(given):
        colored = (_check_rows3(source_colors, "source_colors", A.rows(source)),
                   _check_rows3(target_colors, "target_colors", A.rows(target)),
                   _check_rows3(target_gradients, "target_gradients", A.rows(target)), lam)
    src, _ = A.cloud(source, None, "icp_update")
    tgt, _ = A.cloud(target, None, "icp_update")
    A.nonempty(src, "icp_update", "source")
    A.nonempty(tgt, "icp_update", "target")
    idx = correspondences
    if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int32 or tuple(idx.shape) != (int(src.shape[0]),):
        raise ValueError(f"correspondences: expected an int32 tensor of shape ({int(src.shape[0])},)")
    Td = A.device_T(T, src.device)
    stats = torch.zeros(8, dtype=torch.float64, device=src.device)
    if colored is not None:
        colored = tuple(c.to(src.device) for c in colored[:3]) + (lam,)
    _Updater(src, tgt.to(src.device), None if nrm is None else nrm.to(src.device), colored)(idx.to(src.device).contiguous(), Td,
                                                                                            stats)
    return Td, stats


def prepare(source, target, max_correspondence_distance, T, index, who):
    md = _check_distance("max_correspondence_distance", max_correspondence_distance, True)
    T = A.transform(T, "init" if who == "registration_icp" else "transformation")
    if index is not None and not isinstance(index, NeighborIndex):
        raise TypeError(f"index={index!r}: expected a NeighborIndex")
    src, _ = A.cloud(source, None, who)
    A.nonempty(src, who, "source")
    if index is None:
        index = NeighborIndex(target)
    elif target is not None:
        tgt, _ = A.cloud(target, None, who)
        if int(tgt.shape[0]) != index.size:
            raise ValueError(f"{who}: target has {int(tgt.shape[0])} rows, the index {index.size}")
    if src.device != index.device:
        raise ValueError(f"{who}: source on {src.device}, target on {index.device}")
    return src, index, A.sq(md), T


def _evaluate(src, index, md2, Td, order, updater):
    """closing search under Td -> (fitness, rmse, idx); Td is not changed.  One read-back."""
    P = int(src.shape[0])
    idx = torch.empty(P, dtype=torch.int32, device=src.device)
    index._search(src, Td, md2, order, idx, None)
    stats = torch.zeros(8, dtype=torch.float64, device=src.device)
    updater(idx, Td.clone(), stats)
    s = stats.tolist()
    return s[1], s[2], idx


def evaluate_registration(source, target, max_correspondence_distance, transformation=None, index=None):
    """Fitness and inlier RMSE of `transformation` (None = identity) as Open3D's evaluate_registration defines them:
    correspondences = nearest target point within max_correspondence_distance.  iterations = 0."""
    src, index, md2, T = prepare(source, target, max_correspondence_distance, transformation, index, "evaluate_registration")
    Td = A.device_T(T, src.device)
    fitness, rmse, idx = _evaluate(src, index, md2, Td, None, _Updater(src, index.points))
    return RegistrationResult(Td, fitness, rmse, 0, False, idx)


def registration_icp(source, target, max_correspondence_distance, init=None, relative_fitness=1e-6, relative_rmse=1e-6,
                     max_iteration=30, check_every=1, index=None, use_order=None, estimation="point_to_point",
                     target_normals=None, normal_radius=None, normal_max_nn=30, source_colors=None, target_colors=None,
                     lambda_geometric=LAMBDA_GEOMETRIC, target_gradients=None, gradient_radius=None, gradient_max_nn=30):
    """ICP of `source` onto `target` (both [P,3] float on the HIP device) from `init` (None = identity).

    Iteration k searches the neighbours under T_k, sums them and replaces T_k by T_{k+1} on the device; its fitness and RMSE
    describe T_k.  Every `check_every` iterations they are read back, and the loop stops - as Open3D's does - once both
    |fitness_k - fitness_{k-1}| < relative_fitness and |rmse_k - rmse_{k-1}| < relative_rmse; the update of iteration k has
    been applied by then, and the result's fitness, RMSE and correspondences come from one closing search under the returned
    transformation.  check_every=0 enqueues max_iteration iterations without a read-back and reads once at the end.
    index: a NeighborIndex of `target` to reuse (`target` may then be None).  use_order: Morton-sort the queries once, from
    `init` (None: the measured default, USE_QUERY_ORDER); no result bit depends on it.
    An iteration with fewer than three correspondences leaves the transformation as it is.
    estimation: "point_to_point" (Kabsch on the pairs) or "point_to_plane" (the residual along the target's normal: on floors,
    walls and road surfaces, where pairs slide along the plane, it needs far fewer iterations).  Point-to-plane takes
    `target_normals` ([Pt,3], one per target row) or estimates them once on the target with estimate_normals(normal_radius,
    normal_max_nn) - normal_radius is then required; both at once, or either with "point_to_point", is a ValueError.  An iteration with fewer than six correspondences, or with planes that do not
    fix all six unknowns, leaves the transformation as it is.  Fitness and RMSE are the Euclidean ones for every estimator.
    "colored": the point-to-plane residual, weighted lambda_geometric, joined with a photometric one, weighted 1 -
    lambda_geometric, measured in the target's tangent plane (include/gsr.h gsr_icp_update_colored) - on one plane, where
    point-to-plane pairs slide, the texture fixes the remaining three unknowns.  It takes `source_colors` ([Ps,3]) and
    `target_colors` ([Pt,3]), normals as point-to-plane does, and `target_gradients` ([Pt,3]) or `gradient_radius` to estimate
    them once on the target with estimate_color_gradients(gradient_radius, gradient_max_nn) from those normals - the rules of
    the normals: one of the two, and none of the colour arguments with another estimator."""
    _check_icp(relative_fitness, relative_rmse, max_iteration, check_every)
    est = _check_estimation(estimation)
    plane, colored = est != "point_to_point", est == "colored"
    if not plane and (target_normals is not None or normal_radius is not None):
        raise ValueError('registration_icp: target_normals / normal_radius given, but estimation="point_to_point" uses no normals')
    if not colored and (source_colors is not None or target_colors is not None or target_gradients is not None or
                        gradient_radius is not None):
        raise ValueError(f'registration_icp: colours / gradients given, but estimation="{est}" uses none')
    if target_normals is not None and normal_radius is not None:
        raise ValueError("registration_icp: target_normals and normal_radius both given - pass the normals or have them estimated")
    target_rows = index.size if isinstance(index, NeighborIndex) else A.rows(target)
    if colored:      # (every shape before any device check)
        for t, name, rows in ((source_colors, "source_colors", A.rows(source)), (target_colors, "target_colors", target_rows),
                              (target_gradients, "target_gradients", target_rows)):
            if t is not None:
                _check_rows3(t, name, rows, convert=False)
    nrm = _check_target_normals(target_normals, target_rows)
    if plane and nrm is None:
        if normal_radius is None:
            raise ValueError(f'registration_icp: estimation="{est}" needs target_normals, or normal_radius to estimate them')
        A.neighbourhood(normal_radius, normal_max_nn, 3, NB_NEIGHBORS_MAX)
    lam = check_lambda(lambda_geometric)
    scol = tcol = grd = None
    if colored:
        if source_colors is None or target_colors is None:
            raise ValueError('registration_icp: estimation="colored" needs source_colors and target_colors')
        if target_gradients is not None and gradient_radius is not None:
            raise ValueError("registration_icp: target_gradients and gradient_radius both given - pass the gradients or have "
                             "them estimated")
        if target_gradients is None:
            if gradient_radius is None:
                raise ValueError('registration_icp: estimation="colored" needs target_gradients, or gradient_radius to estimate '
                                 'them')
            A.neighbourhood(gradient_radius, gradient_max_nn, 4, NB_NEIGHBORS_MAX, ("gradient_radius", "gradient_max_nn"))
        scol = _check_rows3(source_colors, "source_colors", A.rows(source))
        tcol = _check_rows3(target_colors, "target_colors", target_rows)
        grd = None if target_gradients is None else _check_rows3(target_gradients, "target_gradients", target_rows)
    src, index, md2, T = prepare(source, target, max_correspondence_distance, init, index, "registration_icp")
    dev, P = src.device, int(src.shape[0])
    Td = A.device_T(T, dev)
    order = index.query_order(src, Td) if (USE_QUERY_ORDER if use_order is None else use_order) else None
    if plane and nrm is None:
        nrm = estimate_normals(index.points, normal_radius, normal_max_nn)
    if colored:
        tcol = tcol.to(dev)
        if grd is None:
            grd = estimate_color_gradients(index.points, tcol, nrm.to(dev), gradient_radius, gradient_max_nn)
    updater = _Updater(src, index.points, nrm.to(dev) if plane else None,
                       (scol.to(dev), tcol, grd.to(dev), lam) if colored else None)
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


# ---- global registration: FPFH features, matching, RANSAC (csrc/features.hip) ------------------------------------------------------
FPFH_WIDTH = 33


def _check_seed(seed):
    return A.integer("seed", seed, 0, 2 ** 64 - 1)


def _check_feature(feature, name, rows=None, convert=True):
    """A.tensor of [rows,33] (rows=None: any number)"""
    return A.tensor(feature, name, ("N" if rows is None else rows, FPFH_WIDTH), convert=convert)


def _check_ransac(max_correspondence_distance, ransac_n, edge_length_threshold, max_iteration, confidence, seed, batch):
    md = _check_distance("max_correspondence_distance", max_correspondence_distance, False)
    n = A.integer("ransac_n", ransac_n, 3, 8)
    for name, v in (("edge_length_threshold", edge_length_threshold), ("confidence", confidence)):
        A.number(name, v, lambda v: 0.0 <= v <= 1.0, "0 .. 1.0")      # (false for NaN)
    A.integer("max_iteration", max_iteration, 1)
    A.integer("batch", batch, 1, 1 << 20)
    return md, n, float(edge_length_threshold), float(confidence), _check_seed(seed)


def _check_pairs(pairs):
    if not isinstance(pairs, torch.Tensor) or pairs.dtype != torch.int32 or pairs.dim() != 2 or pairs.shape[1] != 2:
        raise ValueError("pairs: expected an int32 tensor of shape (M, 2): source row, target row")
    if not pairs.is_cuda:
        raise A.gsr().GsrError("pairs must live on the HIP device (no CPU path)")
    return pairs.contiguous()


def compute_fpfh_feature(points, normals, radius, max_nn=0, return_stats=False):
    """float32 [P,33] on the device: the fast point feature histogram of every row from its normals ([P,3]) - Open3D's
    compute_fpfh_feature, defined bin by bin in include/gsr.h (gsr_compute_fpfh).  The neighbourhood is estimate_normals' (radius,
    cut at the max_nn nearest, ties all kept), or with max_nn=0 the finite radius alone - how Open3D's (5 * voxel, 100) call is
    served: a ball of five voxel sizes on a voxel-sampled surface holds fewer than 100 rows.  Rows are features (Open3D stores the
    transpose).  A row with a non-finite point or normal: NaN, and nobody's neighbour.  `return_stats`: also (spfh_counts int32
    [P,33], count int32 [P] - the neighbourhood's size, the row included).  No read-back."""
    r, nn = A.neighbourhood(radius, max_nn, 3, NB_NEIGHBORS_MAX, radius_alone=True)
    nrm = _check_target_normals(normals, A.rows(points))
    pts, _ = A.cloud(points, None, "compute_fpfh_feature")
    if nrm is None:
        raise ValueError("normals: expected a floating-point tensor of shape (P, 3), one row per point")
    _C = A.gsr()
    P, dev = int(pts.shape[0]), pts.device
    out = torch.empty((P, FPFH_WIDTH), dtype=torch.float32, device=dev)
    counts = torch.empty((P, FPFH_WIDTH), dtype=torch.int32, device=dev) if return_stats else None
    count = torch.empty(P, dtype=torch.int32, device=dev) if return_stats else None
    if P > 0:
        lib = _C.lib()
        nrm = nrm.to(dev)
        with _C.on_device(dev):
            ws = torch.empty(lib.gsr_fpfh_workspace_bytes(P), dtype=torch.uint8, device=dev)
            _C.check(lib.gsr_compute_fpfh(P, _C.ptr(pts), _C.ptr(nrm), r, nn, _C.ptr(out), _C.ptr(counts), _C.ptr(count),
                                          _C.ptr(ws), ws.numel(), _C._stream()))
    return (out, counts, count) if return_stats else out


def feature_nn(query_feature, target_feature):
    """-> (idx int32 [Nq], dist2 float32 [Nq]): the target row nearest to every query row in the 33-dimensional feature space
    (float32 squared distance; among equal distances the smallest row).  A query with a NaN: -1 / NaN; target rows with a NaN
    never win."""
    _check_feature(query_feature, "query_feature", convert=False)
    _check_feature(target_feature, "target_feature", convert=False)
    q = _check_feature(query_feature, "query_feature")
    t = _check_feature(target_feature, "target_feature")
    if q.device != t.device:
        raise ValueError(f"feature_nn: query on {q.device}, target on {t.device}")
    Nq, Nt = int(q.shape[0]), int(t.shape[0])
    idx = torch.full((Nq,), -1, dtype=torch.int32, device=q.device)
    dist2 = torch.full((Nq,), math.inf, dtype=torch.float32, device=q.device)
    if Nq and Nt:
        _C = A.gsr()
        lib = _C.lib()
        with _C.on_device(q.device):
            ws = torch.empty(lib.gsr_feature_nn_workspace_bytes(Nq), dtype=torch.uint8, device=q.device)
            _C.check(lib.gsr_feature_nn(Nq, _C.ptr(q), Nt, _C.ptr(t), FPFH_WIDTH, _C.ptr(idx), _C.ptr(dist2), _C.ptr(ws),
                                        ws.numel(), _C._stream()))
    return idx, dist2


def match_features(source_feature, target_feature, mutual_filter=False):
    """int32 [M,2] on the device, ascending source row: (i, j) with j the target feature nearest to source feature i.
    mutual_filter: only the pairs whose target row j has i as ITS nearest source feature (a second search, roles swapped)."""
    if not isinstance(mutual_filter, bool):
        raise TypeError(f"mutual_filter={mutual_filter!r}: expected a bool")
    _check_feature(source_feature, "source_feature", convert=False)
    _check_feature(target_feature, "target_feature", convert=False)
    s = _check_feature(source_feature, "source_feature")
    t = _check_feature(target_feature, "target_feature")
    fwd, _ = feature_nn(s, t)
    rows = torch.arange(int(s.shape[0]), dtype=torch.int32, device=s.device)
    keep = fwd >= 0
    if mutual_filter and int(t.shape[0]):
        back, _ = feature_nn(t, s)
        keep = keep & (back[fwd.clamp(min=0).long()] == rows)
    return torch.stack([rows[keep], fwd[keep]], dim=1).contiguous()


def new_ransac_record(device):
    """a fresh gsr_ransac_best on `device` as int64 [20] (words 1 and 3 .. 18 hold float64 bits): count -1, sum_d2 +inf, trial -1,
    T = identity, trials_checked 0"""
    rec = torch.zeros(20, dtype=torch.float64)
    rec[1] = math.inf
    rec[3:19] = torch.eye(4, dtype=torch.float64).reshape(-1)
    rec = rec.view(torch.int64)
    rec[0] = -1
    rec[2] = -1
    return rec.to(device)


def read_ransac_record(record):
    """-> dict(count, sum_d2, trial, T float64 [4,4] (host), trials_checked) - one read-back"""
    r = record.cpu()
    f = r.view(torch.float64)
    return dict(count=int(r[0]), sum_d2=float(f[1]), trial=int(r[2]), T=f[3:19].reshape(4, 4).clone(), trials_checked=int(r[19]))


def ransac_trials(source, target, pairs, max_correspondence_distance, ransac_n, edge_length_threshold, seed, first_trial, trials,
                  record=None, debug=False):
    """Trials [first_trial, first_trial + trials) of gsr_ransac_feature_matching against `record` (new_ransac_record; updated in
    place and returned).  debug: also (samples int32 [trials,8], status int32 [trials], T float64 [trials,4,4]) of the
    hypothesis stage.  No read-back."""
    md, n, theta, _, sd = _check_ransac(max_correspondence_distance, ransac_n, edge_length_threshold, 1, 1.0, seed, 1)
    t0 = A.integer("first_trial", first_trial, 0)
    cnt = A.integer("trials", trials, 1, 1 << 20)
    prs = _check_pairs(pairs)
    src, _ = A.cloud(source, None, "ransac_trials")
    tgt, _ = A.cloud(target, None, "ransac_trials")
    A.nonempty(src, "ransac_trials", "source")
    A.nonempty(tgt, "ransac_trials", "target")
    M, dev = int(prs.shape[0]), src.device
    if M == 0:
        raise ValueError("ransac_trials: no pairs")
    if record is None:
        record = new_ransac_record(dev)
    _C = A.gsr()
    lib = _C.lib()
    dbg = None
    out = None
    if debug:
        out = (torch.empty((cnt, 8), dtype=torch.int32, device=dev), torch.empty(cnt, dtype=torch.int32, device=dev),
               torch.empty((cnt, 4, 4), dtype=torch.float64, device=dev))
        dbg = _C.gsr_ransac_debug(out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr())
    with _C.on_device(dev):
        ws = torch.empty(lib.gsr_ransac_workspace_bytes(M, cnt), dtype=torch.uint8, device=dev)
        _C.check(lib.gsr_ransac_feature_matching(int(src.shape[0]), _C.ptr(src), int(tgt.shape[0]), _C.ptr(tgt.to(dev)), M,
                                                 _C.ptr(prs.to(dev)), md, n, theta, sd, t0, cnt, _C.ptr(record), _C.ptr(ws),
                                                 ws.numel(), dbg, _C._stream()))
    return (record,) + out if debug else record


def _ransac_enough(done, inliers, M, ransac_n, confidence):
    """Open3D's rule: done >= log(1 - confidence) / log(1 - (inliers / M) ** ransac_n).  The denominator is log1p(-p): for a
    p below 1e-16 (eight samples at an inlier share of a thousandth) 1 - p rounds to 1 and its logarithm to 0; and where even
    log1p gives 0 (p = 0, or below the smallest float) no number of trials is enough: keep going."""
    ratio = max(inliers, 0) / M
    if ratio >= 1.0:
        return True
    den = math.log1p(-(ratio ** ransac_n))
    return den < 0.0 and done >= math.log(1.0 - confidence) / den


def registration_ransac_based_on_feature_matching(source, target, source_feature, target_feature, mutual_filter,
                                                  max_correspondence_distance, ransac_n=3, edge_length_threshold=0.9,
                                                  max_iteration=100000, confidence=0.999, seed=0, batch=16384, pairs=None):
    """Open3D's call of the same name -> RegistrationResult (iterations = trials run, converged = some trial survived).
    Correspondences: match_features(source_feature, target_feature, mutual_filter) - with fewer than ransac_n mutual pairs the
    unfiltered ones, as Open3D does - or `pairs` (int32 [M,2]; the features may then be None).  Trials of ransac_n sampled pairs
    each (a counter-based generator: trial t is a function of (seed, t) alone), checked by edge length (0 switches it off) and
    distance, scored by their inliers over all pairs; they run in batches of `batch`, and after each the best is read back and
    the loop stops once trials >= log(1 - confidence) / log(1 - (inliers / pairs) ** ransac_n).  confidence=1.0 runs
    max_iteration trials without a read-back.  The winner is the lexicographic best of (inliers max, sum of squared inlier
    distances min, trial min): the result depends on `batch` only through where the loop stops.  Fitness, RMSE and
    correspondences are evaluate_registration's under the winner; without a surviving trial the identity."""
    md, n, theta, conf, sd = _check_ransac(max_correspondence_distance, ransac_n, edge_length_threshold, max_iteration,
                                           confidence, seed, batch)
    if not isinstance(mutual_filter, bool):
        raise TypeError(f"mutual_filter={mutual_filter!r}: expected a bool")
    if pairs is None:
        _check_feature(source_feature, "source_feature", A.rows(source), convert=False)
        _check_feature(target_feature, "target_feature", A.rows(target), convert=False)
    elif not isinstance(pairs, torch.Tensor) or pairs.dtype != torch.int32 or pairs.dim() != 2 or pairs.shape[1] != 2:
        raise ValueError("pairs: expected an int32 tensor of shape (M, 2): source row, target row")
    src, _ = A.cloud(source, None, "registration_ransac_based_on_feature_matching")
    tgt, _ = A.cloud(target, None, "registration_ransac_based_on_feature_matching")
    A.nonempty(src, "registration_ransac_based_on_feature_matching", "source")
    A.nonempty(tgt, "registration_ransac_based_on_feature_matching", "target")
    dev = src.device
    if pairs is not None:
        pairs = _check_pairs(pairs)
    else:
        pairs = match_features(source_feature, target_feature, mutual_filter)
        if mutual_filter and int(pairs.shape[0]) < n:
            pairs = match_features(source_feature, target_feature, False)
    M = int(pairs.shape[0])
    record = new_ransac_record(dev)
    done = 0
    while M >= n and done < max_iteration:
        cnt = min(batch, max_iteration - done)
        ransac_trials(src, tgt, pairs, md, n, theta, sd, done, cnt, record)
        done += cnt
        if conf < 1.0 and _ransac_enough(done, int(record[0].item()), M, n, conf):
            break
    best = read_ransac_record(record)
    found = best["count"] >= 0
    res = evaluate_registration(src, tgt, md, best["T"] if found else None)
    return RegistrationResult(res.transformation, res.fitness, res.inlier_rmse, done, found, res.correspondences)


def global_registration(source, target, voxel_size, seed=0, **ransac):
    """The reference's commented pipeline on clouds that are already down-sampled at `voxel_size`: normals (radius 2 v, max_nn 30,
    towards the cloud's mean - a rule that turns with the cloud, which the default sign rule does not), FPFH (radius 5 v,
    radius-only), mutual matching, RANSAC (1.5 v, ransac_n 4, edge length 0.9) -> RegistrationResult."""
    v = A.voxel_size(voxel_size)
    _check_seed(seed)
    src, _ = A.cloud(source, None, "global_registration")
    tgt, _ = A.cloud(target, None, "global_registration")
    feats = []
    for pts in (src, tgt):
        ok = torch.isfinite(pts).all(dim=1)
        centre = pts[ok].double().mean(dim=0).tolist() if bool(ok.any()) else [0.0, 0.0, 0.0]
        nrm = estimate_normals(pts, 2.0 * v, 30, viewpoint=centre)
        feats.append(compute_fpfh_feature(pts, nrm, 5.0 * v))
    ransac = dict(dict(ransac_n=4, edge_length_threshold=0.9, seed=seed), **ransac)
    return registration_ransac_based_on_feature_matching(src, tgt, feats[0], feats[1], True, 1.5 * v, **ransac)


# what the drivers below decide themselves when they run the coloured (or the point-to-plane) estimator on clouds they down-sample
_COLORED_OWN = ("target_normals", "normal_radius", "normal_max_nn", "source_colors", "target_colors", "target_gradients",
                "gradient_radius", "gradient_max_nn")


def registration_colored_icp(source, source_colors, target, target_colors, max_correspondence_distance, init=None,
                             lambda_geometric=LAMBDA_GEOMETRIC, max_iteration=50, **icp):
    """Open3D's call of the same name: registration_icp(estimation="colored") with Open3D's argument order and its 50
    iterations.  The target's normals (`target_normals` or `normal_radius`) and colour gradients (`target_gradients` or
    `gradient_radius`) and every other keyword go to registration_icp.  -> RegistrationResult."""
    if "estimation" in icp:
        raise TypeError('registration_colored_icp: the estimation is "colored" (registration_icp takes the others)')
    return registration_icp(source, target, max_correspondence_distance, init=init, max_iteration=max_iteration,
                            estimation="colored", source_colors=source_colors, target_colors=target_colors,
                            lambda_geometric=lambda_geometric, **icp)


def registration_multiscale(source, source_colors, target, target_colors, voxel_sizes, max_iterations, estimation="colored",
                            init=None, lambda_geometric=LAMBDA_GEOMETRIC, **icp):
    """Coarse-to-fine registration, Open3D's coloured-registration recipe: for every (voxel_size, max_iteration) of the two equally
    long sequences, in the order given (coarse first), both clouds are down-sampled with voxel_down_sample (colours averaged),
    normals and colour gradients of the down-sampled target are estimated with radius = 2 * voxel_size and max_nn = 30, and
    registration_icp runs with max_correspondence_distance = voxel_size from the previous level's transformation (`init` for the
    first).  estimation: "colored" (colours required), "point_to_plane" or "point_to_point" (colours may be None).  Further
    keywords (relative_fitness, relative_rmse, check_every, use_order) go to every level.
    -> (the last level's RegistrationResult - its correspondences number the rows of that level's down-sampled clouds -, the list of
    every level's result)."""
    est = _check_estimation(estimation)
    lam = check_lambda(lambda_geometric)
    T = A.transform(init, "init")
    try:
        voxels, iterations = list(voxel_sizes), list(max_iterations)
    except TypeError:
        raise TypeError("registration_multiscale: voxel_sizes and max_iterations are sequences, one entry per level") from None
    if not voxels or len(voxels) != len(iterations):
        raise ValueError(f"registration_multiscale: {len(voxels)} voxel sizes and {len(iterations)} iteration counts: expected "
                         "as many of one as of the other, at least one")
    voxels = [A.voxel_size(v) for v in voxels]
    iterations = [A.integer("max_iterations", n, 1) for n in iterations]
    for k in ("index", "max_iteration", "estimation") + _COLORED_OWN:
        if k in icp:
            raise TypeError(f"registration_multiscale: {k} is decided per level, not accepted")
    if (source_colors is None) != (target_colors is None):
        raise ValueError("registration_multiscale: colours for both clouds or for neither")
    if est == "colored" and source_colors is None:
        raise ValueError('registration_multiscale: estimation="colored" needs the colours of both clouds')
    src, scol = A.cloud(source, source_colors, "registration_multiscale")
    tgt, tcol = A.cloud(target, target_colors, "registration_multiscale")
    results = []
    for v, n in zip(voxels, iterations):
        sd, sc = voxel_down_sample(src, scol, v)
        td, tc = voxel_down_sample(tgt, tcol, v)
        level = dict(icp)
        if est != "point_to_point":
            level.update(normal_radius=2.0 * v, normal_max_nn=30)
        if est == "colored":
            level.update(gradient_radius=2.0 * v, gradient_max_nn=30, source_colors=sc, target_colors=tc, lambda_geometric=lam)
        results.append(registration_icp(sd, td, v, init=T, max_iteration=n, estimation=est, **level))
        T = results[-1].transformation
    return results[-1], results


def register_and_merge(source, source_colors, target, target_colors, voxel_size=0.05, max_correspondence_distance=None,
                       merge_voxel_size=None, estimation="point_to_point", global_init=False, global_seed=0, **icp):
    """The reference's pointcloud_registeration: down-sample both clouds (voxel_down_sample, voxel_size), ICP of the down-sampled
    source onto the down-sampled target from the identity (max_correspondence_distance=None: 5 * voxel_size; further keywords
    go to registration_icp), move the FULL source by the result, concatenate it with the target (source rows first) and, with
    merge_voxel_size, down-sample the merged cloud.  Colours: both or neither.  -> (points, colors or None, result).
    estimation="point_to_plane": the down-sampled target's normals are estimated with radius = 2 * voxel_size, max_nn = 30 - the
    reference's estimate_normals calls at :193-196 - and the registration is point-to-plane.
    estimation="colored": both clouds are down-sampled WITH their colours (averaged per voxel), normals and colour gradients of
    the down-sampled target are estimated with radius = 2 * voxel_size, max_nn = 30, and the registration is the coloured one
    (`lambda_geometric` may be passed on); colours are then required.
    global_init=True: ICP starts from a global registration of the down-sampled clouds instead of the identity - the reference's
    commented pipeline at :198-213: normals (radius 2 * voxel_size, max_nn 30, oriented towards the cloud's mean so that they
    turn with the cloud), compute_fpfh_feature (radius 5 * voxel_size, radius-only), mutual matching and
    registration_ransac_based_on_feature_matching (1.5 * voxel_size, ransac_n 4, edge length 0.9, seed `global_seed`).  With
    False nothing of that runs and every output bit is what it was."""
    if not isinstance(global_init, bool):
        raise TypeError(f"global_init={global_init!r}: expected a bool")
    _check_seed(global_seed)
    v = A.voxel_size(voxel_size)
    est = _check_estimation(estimation)
    plane, colored = est == "point_to_plane", est == "colored"
    mv = None if merge_voxel_size is None else A.voxel_size(merge_voxel_size)
    md = 5.0 * v if max_correspondence_distance is None else _check_distance("max_correspondence_distance",
                                                                             max_correspondence_distance, True)
    if (source_colors is None) != (target_colors is None):
        raise ValueError("register_and_merge: colours for both clouds or for neither")
    if "init" in icp or "index" in icp:
        raise TypeError("register_and_merge: starts from the identity and builds its own index (init / index not accepted)")
    if plane and ("target_normals" in icp or "normal_radius" in icp or "normal_max_nn" in icp):
        raise TypeError("register_and_merge: estimates the down-sampled target's normals itself (radius 2 * voxel_size, max_nn 30)")
    if colored:
        if any(k in icp for k in _COLORED_OWN):
            raise TypeError("register_and_merge: the coloured registration takes the down-sampled clouds' colours and estimates "
                            "normals and gradients itself (radius 2 * voxel_size, max_nn 30)")
        if source_colors is None:
            raise ValueError('register_and_merge: estimation="colored" needs the colours of both clouds')
    src, scol = A.cloud(source, source_colors, "register_and_merge")
    tgt, tcol = A.cloud(target, target_colors, "register_and_merge")
    src_down, scol_down = voxel_down_sample(src, scol if colored else None, v)
    tgt_down, tcol_down = voxel_down_sample(tgt, tcol if colored else None, v)
    if colored:
        icp = dict(icp, estimation="colored", normal_radius=2.0 * v, normal_max_nn=30, gradient_radius=2.0 * v, gradient_max_nn=30,
                   source_colors=scol_down, target_colors=tcol_down)
    if plane:
        icp = dict(icp, estimation="point_to_plane", normal_radius=2.0 * v, normal_max_nn=30)
    if global_init:
        icp = dict(icp, init=global_registration(src_down, tgt_down, v, seed=global_seed).transformation)
    result = registration_icp(src_down, tgt_down, md, **icp)
    points = torch.cat([transform_points(src, result.transformation), tgt.to(src.device)])
    colors = None if scol is None else torch.cat([scol, tcol.to(src.device)])
    if mv is not None:
        points, colors = voxel_down_sample(points, colors, mv)
    return points, colors, result


def align_map(model, target_points, max_correspondence_distance, ids=None, voxel_size=None, **icp):
    """Registers the model's means - with `ids`, only the rows anchored to those keyframes - to `target_points` and moves the
    model by the result through `model.transform_(T, ids=ids)`: rotations, SH bands and moments follow as that call defines.
    voxel_size: down-sample the means first (the target is taken as given).  -> RegistrationResult."""
    md = _check_distance("max_correspondence_distance", max_correspondence_distance, True)
    v = None if voxel_size is None else A.voxel_size(voxel_size)
    xyz = model.get_xyz
    if not isinstance(xyz, torch.Tensor) or not xyz.is_cuda:
        raise A.gsr().GsrError("align_map runs in HIP kernels (no CPU path): the model must live on the HIP device")
    src = xyz.detach()
    if ids is not None:
        ids = [int(i) for i in ids]
        if getattr(model, "_anchor", None) is None:
            raise ValueError("align_map: `ids` given but the model has no anchors (set_anchors, add_from_rgbd(anchor=...))")
        wanted = torch.tensor(ids, dtype=torch.int32, device=src.device)
        src = src[torch.isin(model._anchor.to(src.device), wanted)]
    if v is not None:
        src, _ = voxel_down_sample(src, None, v)
    result = registration_icp(src, target_points, md, **icp)
    T = result.transformation
    model.transform_(T if ids is None else T.unsqueeze(0).expand(len(ids), 4, 4).contiguous(), ids=ids)
    return result
