"""Place recognition from LiDAR scans: the polar "scan context" descriptor of Kim & Kim (IROS 2018) - rings x sectors around the
sensor, the largest height per cell - the exhaustive search over all column shifts, which gives a distance and a yaw together,
and a keyframe database that says which old scans the current one resembles (csrc/scancontext.hip; the rules, stated exactly, are
in include/gsr.h).  A road driven the other way, a crossing entered from a side street, night against day: the images differ, the
360 degree scan hardly does.  scan_loop_closure_edge turns a hit into a loop-closure edge of a PoseGraph: the yaw starts the
registration that global_registration's RANSAC would have had to guess.  There is no CPU path."""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

from . import _args as A
from .gicp import registration_generalized_icp
from .posegraph import information_from_point_clouds
from .registration import registration_icp, _check_distance

MAX_RINGS = 40         # GSR_SCAN_CONTEXT_MAX_RINGS
MAX_SECTORS = 120      # GSR_SCAN_CONTEXT_MAX_SECTORS
MAX_ORIGINS = 16       # GSR_SCAN_CONTEXT_MAX_ORIGINS
SCAN_ESTIMATIONS = ("generalized", "point_to_plane", "point_to_point")


class ScanContext(NamedTuple):
    descriptor: torch.Tensor    # float32 [B,R,S] on the device: one grid per origin, variant 0 first
    norms: torch.Tensor         # float32 [B,S]: the Euclidean norm of every column
    rings: int
    sectors: int
    max_range: float
    height_offset: float


def _check_geometry(rings, sectors, max_range, height_offset):
    return (A.integer("rings", rings, 1, MAX_RINGS), A.integer("sectors", sectors, 1, MAX_SECTORS),
            A.number("max_range", max_range, lambda v: math.isfinite(v) and v > 0, "a finite value > 0"),
            A.number("height_offset", height_offset, math.isfinite, "a finite value"))


def _host_matrix(value, name, shapes, expected):
    """a finite float64 numpy array of one of `shapes` from a tensor, an array or nested lists (a device tensor is read back)"""
    if isinstance(value, torch.Tensor):
        value = value.detach().cpu().numpy()
    try:
        m = np.asarray(value, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: expected {expected}") from None
    if not any(m.ndim == len(s) and all(n is None or d == n for d, n in zip(m.shape, s)) for s in shapes):
        raise ValueError(f"{name}: expected {expected}, got shape {m.shape}")
    if not np.isfinite(m).all():
        raise ValueError(f"{name}: not finite")
    return m


def _check_frame(frame):
    """None, or the rows 0 .. 2 of a [3,4] / [4,4] matrix (cloud -> levelled sensor frame) as float64 numpy [3,4]"""
    if frame is None:
        return None
    return _host_matrix(frame, "frame", ((3, 4), (4, 4)), "a [3,4] or [4,4] matrix")[:3].copy()


def _check_origins(origins, name="origins"):
    """None, or float64 numpy [B,3], B = 1 .. 16"""
    if origins is None:
        return None
    o = _host_matrix(origins, name, ((None, 3),), "a [B,3] matrix")
    if not 1 <= o.shape[0] <= MAX_ORIGINS:
        raise ValueError(f"{name}: expected 1 .. {MAX_ORIGINS} rows, got {o.shape[0]}")
    return o


def _c_floats(m):
    _C = A.gsr()
    flat = np.ascontiguousarray(m, dtype=np.float32).reshape(-1)
    return (_C.C.c_float * flat.size)(*flat.tolist())


def scan_context(points, rings=20, sectors=60, max_range=80.0, height_offset=2.0, frame=None, origins=None):
    """gsr_scan_context: `points` [N,3] float on the HIP device -> ScanContext, one descriptor per origin.  frame: [3,4] or [4,4],
    cloud -> levelled sensor frame with z up (None: the cloud is in that frame already); origins: [B,3] in the levelled frame,
    B = 1 .. 16 (None: the sensor itself) - a scan described again as if taken a lane to the left or right is how a query
    becomes robust against a lateral offset.  Both are host data: given as a device tensor each is read back once.
    height_offset: added to z before the cut at 0, so roughly the sensor's height above the road.  N = 0 gives zeros.  All
    outputs stay on the device; with `frame` and `origins` on the host there is no read-back."""
    R, S, mr, ho = _check_geometry(rings, sectors, max_range, height_offset)
    F, O = _check_frame(frame), _check_origins(origins)
    A.tensor(points, "points", ("N", 3), convert=False)
    pts = A.tensor(points, "points", ("N", 3))
    _C = A.gsr()
    B, N = 1 if O is None else int(O.shape[0]), int(pts.shape[0])
    desc = torch.empty((B, R, S), dtype=torch.float32, device=pts.device)
    norms = torch.empty((B, S), dtype=torch.float32, device=pts.device)
    with _C.on_device(pts.device):
        _C.check(_C.lib().gsr_scan_context(N, _C.ptr(pts) if N else None, None if F is None else _c_floats(F), B,
                                           None if O is None else _c_floats(O), R, S, mr, ho, _C.ptr(desc), _C.ptr(norms),
                                           _C._stream()))
    return ScanContext(desc, norms, R, S, mr, ho)


def _check_context(context, name="context", convert=True):
    if not isinstance(context, ScanContext):
        raise TypeError(f"{name}: expected a ScanContext, got {type(context).__name__}")
    R, S = A.integer(f"{name}.rings", context.rings, 1, MAX_RINGS), A.integer(f"{name}.sectors", context.sectors, 1, MAX_SECTORS)
    d, n = context.descriptor, context.norms
    B = int(d.shape[0]) if isinstance(d, torch.Tensor) and d.dim() == 3 else 0
    if not 1 <= B <= MAX_ORIGINS:
        raise ValueError(f"{name}.descriptor: expected a floating-point tensor of shape (B, {R}, {S}), B = 1 .. {MAX_ORIGINS}")
    A.tensor(d, f"{name}.descriptor", (B, R, S), convert=False)
    A.tensor(n, f"{name}.norms", (B, S), convert=False)
    if not convert:
        return None
    return A.tensor(d, f"{name}.descriptor", (B, R, S)), A.tensor(n, f"{name}.norms", (B, S))


def _distance(qd, qn, R, S, dd, dn, K):
    """gsr_scan_context_distance of checked tensors against the first K rows of dd / dn"""
    dev = qd.device
    dist = torch.empty(K, dtype=torch.float32, device=dev)
    shift = torch.empty(K, dtype=torch.int32, device=dev)
    variant = torch.empty(K, dtype=torch.int32, device=dev)
    if K:
        _C = A.gsr()
        with _C.on_device(dev):
            _C.check(_C.lib().gsr_scan_context_distance(R, S, int(qd.shape[0]), _C.ptr(qd), _C.ptr(qn), K, _C.ptr(dd), _C.ptr(dn),
                                                        _C.ptr(dist), _C.ptr(shift), _C.ptr(variant), _C._stream()))
    return dist, shift, variant


def scan_context_distance(query, database_descriptors, database_norms):
    """gsr_scan_context_distance: the ScanContext `query` (all its variants) against K stored descriptors [K,R,S] with their norms
    [K,S] -> (dist float32 [K], shift int32 [K], variant int32 [K]): per row the smallest distance over all variants and column
    shifts, ties to the smallest variant, then the smallest shift; yaw = shift 2 pi / S, the query's points being about Rz(yaw)
    times the stored scan's.  K = 0 is legal.  No read-back."""
    _check_context(query, "query", convert=False)
    R, S = query.rings, query.sectors
    A.tensor(database_descriptors, "database_descriptors", ("K", R, S), convert=False)
    K = int(database_descriptors.shape[0])
    A.tensor(database_norms, "database_norms", (K, S), convert=False)
    qd, qn = _check_context(query, "query")
    dd = A.tensor(database_descriptors, "database_descriptors", ("K", R, S))
    dn = A.tensor(database_norms, "database_norms", (K, S))
    if dd.device != qd.device or dn.device != qd.device:
        raise ValueError(f"scan_context_distance: query on {qd.device}, database on {dd.device} / {dn.device}")
    return _distance(qd, qn, R, S, dd, dn, K)


# ---- the keyframe database ---------------------------------------------------------------------------------------------------------------
class ScanEntry(NamedTuple):
    kf_id: object
    context: ScanContext
    points: object              # the keyframe's scan [P,3] on the device (for scan_loop_closure_edge), or None


class ScanDatabase:
    """Variant 0 of the descriptor of every keyframe added so far, one behind the other in one device buffer (append-only; the
    buffer doubles when it is full).  query() runs gsr_scan_context_distance: one workgroup per keyframe, every column shift."""

    def __init__(self, device="cuda", rings=20, sectors=60, max_range=80.0, height_offset=2.0):
        self.rings, self.sectors, self.max_range, self.height_offset = _check_geometry(rings, sectors, max_range, height_offset)
        self.device = torch.device(device)
        self._desc = torch.zeros((0, self.rings, self.sectors), dtype=torch.float32, device=self.device)
        self._norms = torch.zeros((0, self.sectors), dtype=torch.float32, device=self.device)
        self._entries = []
        self._row_of = {}

    def __len__(self):
        return len(self._entries)

    def __getitem__(self, kf_id):
        return self._entries[self._row_of[kf_id]]

    def __contains__(self, kf_id):
        return kf_id in self._row_of

    def _same_geometry(self, context, who):
        have = (context.rings, context.sectors, float(context.max_range), float(context.height_offset))
        want = (self.rings, self.sectors, self.max_range, self.height_offset)
        if have != want:
            raise ValueError(f"{who}: the context's (rings, sectors, max_range, height_offset) = {have}, the database's {want}")

    def _grow(self, rows):
        cap = int(self._desc.shape[0])
        if rows <= cap:
            return
        cap = max(rows, 2 * cap, 64)
        d = torch.zeros((cap, self.rings, self.sectors), dtype=torch.float32, device=self.device)
        n = torch.zeros((cap, self.sectors), dtype=torch.float32, device=self.device)
        K = len(self._entries)
        d[:K], n[:K] = self._desc[:K], self._norms[:K]
        self._desc, self._norms = d, n

    def add(self, kf_id, context, points=None):
        """appends keyframe `kf_id` (any hashable id, not yet present) with variant 0 of `context`; `points`, the scan itself, is
        kept beside it for scan_loop_closure_edge"""
        _check_context(context, convert=False)
        self._same_geometry(context, "add")
        if kf_id in self._row_of:
            raise ValueError(f"add: keyframe {kf_id!r} is already in the database")
        if points is not None:
            A.tensor(points, "points", ("P", 3), convert=False)
        d, n = _check_context(context)
        if points is not None:
            points = A.tensor(points, "points", ("P", 3))
        K = len(self._entries)
        self._grow(K + 1)
        self._desc[K], self._norms[K] = d[0].to(self.device), n[0].to(self.device)
        self._row_of[kf_id] = K
        self._entries.append(ScanEntry(kf_id, context, points))

    def distances(self, context):
        """(dist float32 [K], shift int32 [K], variant int32 [K]) on the device, in insertion order.  No read-back."""
        _check_context(context, convert=False)
        self._same_geometry(context, "distances")
        qd, qn = _check_context(context)
        return _distance(qd.to(self.device), qn.to(self.device), self.rings, self.sectors, self._desc, self._norms,
                         len(self._entries))

    def query(self, context, exclude=(), top_k=5, max_distance=0.4):
        """-> [(kf_id, distance, yaw_radians, variant)]: the at most `top_k` keyframes within `max_distance`, none of `exclude`,
        ranked by distance, then by insertion order; yaw = shift 2 pi / sectors, the query scan's points being about Rz(yaw) times
        the keyframe's.  One read-back: the K rows."""
        k = A.integer("top_k", top_k, 1)
        md = A.number("max_distance", max_distance, lambda v: v >= 0, "a value >= 0")      # (false for NaN)
        skip = set(exclude)
        dist, shift, variant = self.distances(context)
        rows = torch.stack([dist.double(), shift.double(), variant.double()], dim=1).tolist()
        ranked = sorted((d, r) for r, (d, _, _) in enumerate(rows) if d <= md and self._entries[r].kf_id not in skip)
        return [(self._entries[r].kf_id, d, int(rows[r][1]) * 2.0 * math.pi / self.sectors, int(rows[r][2])) for d, r in ranked[:k]]


# ---- from a hit to a pose-graph edge ---------------------------------------------------------------------------------------------------
def _yaw_start_pose(yaw, offset=None, frame=None):
    """float64 numpy [4,4]: x_new ~ T x_old in the clouds' own frame for two scans whose levelled frames differ by Rz(yaw) and the
    translation `offset` (levelled frame; None: 0) - Rz about the levelled z axis, conjugated by `frame` (cloud -> levelled)."""
    c, s = math.cos(yaw), math.sin(yaw)
    L = np.eye(4)
    L[:3, :3] = [[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]
    if offset is not None:
        L[:3, 3] = offset
    if frame is None:
        return L
    F = np.eye(4)
    F[:3] = frame
    return np.linalg.inv(F) @ L @ F


def scan_loop_closure_edge(db_entry, points, context=None, max_correspondence_distance=1.0, min_fitness=0.3,
                           estimation="generalized", origin_of_variant=None, frame=None, **registration):
    """A loop-closure edge from the keyframe `db_entry` (a ScanEntry with its scan, e.g. db[kf_id]) to the scan `points` [P,3] on
    the HIP device (`context`: its ScanContext, computed here with the entry's geometry, `frame` and `origin_of_variant` when
    None).  The entry's descriptor against the context gives a column shift and a variant (one read-back); the start pose is
    Rz(shift 2 pi / S) about the levelled z axis, conjugated by `frame` (cloud -> levelled, the same for both scans) if one is
    given, plus the lateral offset of the winning variant (`origin_of_variant`: the [B,3] origins the context was computed with;
    None: no offset).  It goes as `init` into registration_generalized_icp ("generalized"; without covariances a
    covariance_radius of 2 max_correspondence_distance) or registration_icp ("point_to_plane"; without normals a normal_radius
    of 2 max_correspondence_distance; or "point_to_point") with the stored scan as source and the new one as target;
    `registration`: further keywords of that call.  None when the fitness stays below `min_fitness`; otherwise (transformation
    float64 [4,4], information float64 [6,6]), both on the device, taking coordinates of the keyframe's scan to those of
    `points`: PoseGraph.add_edge(kf_id, frame_id, transformation, information, uncertain=True)."""
    if not isinstance(db_entry, ScanEntry) or db_entry.points is None:
        raise ValueError("db_entry: expected a ScanEntry that holds its scan (ScanDatabase.add(..., points=...))")
    md = _check_distance("max_correspondence_distance", max_correspondence_distance, False)
    floor = A.number("min_fitness", min_fitness, lambda v: 0.0 <= v <= 1.0, "0 .. 1.0")      # (false for NaN)
    if not isinstance(estimation, str):
        raise TypeError(f"estimation={estimation!r}: expected one of {SCAN_ESTIMATIONS}")
    if estimation not in SCAN_ESTIMATIONS:
        raise ValueError(f"estimation={estimation!r}: expected one of {SCAN_ESTIMATIONS}")
    if "init" in registration:
        raise ValueError("scan_loop_closure_edge: init is the yaw start pose, not the caller's to give")
    F, O = _check_frame(frame), _check_origins(origin_of_variant, "origin_of_variant")
    A.tensor(points, "points", ("P", 3), convert=False)
    old = db_entry.context
    if context is not None:
        _check_context(context, convert=False)
        have = (context.rings, context.sectors, float(context.max_range), float(context.height_offset))
        want = (old.rings, old.sectors, float(old.max_range), float(old.height_offset))
        if have != want:
            raise ValueError(f"context: (rings, sectors, max_range, height_offset) = {have}, the entry's descriptor has {want}")
        B = int(context.descriptor.shape[0])
        if O is not None and int(O.shape[0]) != B:
            raise ValueError(f"origin_of_variant: {int(O.shape[0])} rows, the context has {B} variants")
    tgt = A.tensor(points, "points", ("P", 3))
    if context is None:
        context = scan_context(tgt, old.rings, old.sectors, old.max_range, old.height_offset, frame=F, origins=O)
    src = db_entry.points
    _, shift, variant = scan_context_distance(context, old.descriptor[:1].to(tgt.device), old.norms[:1].to(tgt.device))
    s, b = torch.stack([shift, variant]).reshape(-1).tolist()
    init = torch.from_numpy(_yaw_start_pose(s * 2.0 * math.pi / old.sectors, None if O is None else O[b], F))
    if estimation == "generalized":
        if not any(k in registration for k in ("source_covariances", "target_covariances", "covariance_radius")):
            registration["covariance_radius"] = 2.0 * md
        res = registration_generalized_icp(src, tgt, md, init=init, **registration)
    else:
        if estimation == "point_to_plane" and not any(k in registration for k in ("target_normals", "normal_radius")):
            registration["normal_radius"] = 2.0 * md
        res = registration_icp(src, tgt, md, init=init, estimation=estimation, **registration)
    if res.fitness < floor:
        return None
    return res.transformation, information_from_point_clouds(src, tgt, md, res.transformation)


__all__ = ["ScanContext", "ScanEntry", "ScanDatabase", "scan_context", "scan_context_distance", "scan_loop_closure_edge"]
