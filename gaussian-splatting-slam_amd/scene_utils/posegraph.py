"""Pose-graph optimisation on the device: edges in, corrections out.

`registration_icp`, `registration_colored_icp`, `global_registration` and `rgbd_odometry` each return the relative transformation
between two keyframes; `correct_keyframes` takes one 4x4 correction per keyframe.  `PoseGraph` joins the two: nodes are keyframe
poses (node frame to world), an edge carries the transformation that takes coordinates of its source node to coordinates of its
target node - exactly what `registration_icp(source, target)` returns - with a 6x6 information matrix
(`information_from_point_clouds`, Open3D's GetInformationMatrixFromPointClouds) and whether it is a loop closure that may be
false (`uncertain`).  `optimize` is Levenberg-Marquardt with a line process on the uncertain edges (Choi, Zhou, Koltun 2015, as
in Open3D's GlobalOptimization) and preconditioned conjugate gradients on the block-sparse normal equations, the whole loop in ONE
launch of one workgroup, float64, deterministic (csrc/posegraph.hip, include/gsr.h "pose graph").  There is no CPU path.

Matrices given on the host are validated (ValueError); device tensors are trusted, as in `GaussianModel.transform_`."""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple

import numpy as np
import torch

from . import _args as A
from .odometry import OdometryResult
from .registration import RegistrationResult, prepare
from .transform import validate_transforms

STATUS_NAMES = ("converged: step", "max_iteration", "solver failed", "converged: residual", "converged: zero residual", "lambda")
CONVERGED = (0, 3, 4)      # GSR_PG_CONVERGED_STEP, GSR_PG_CONVERGED_RESIDUAL, GSR_PG_ZERO_RESIDUAL
SYMMETRY_TOL = 1e-9        # |L - L^T| <= SYMMETRY_TOL max |L|


class PoseGraphResult(NamedTuple):
    status: int                       # GSR_PG_* of include/gsr.h (STATUS_NAMES[status])
    converged: bool                   # status is one of the three "converged" values
    iterations: int                   # linear solves
    accepted: int                     # accepted steps
    residual_start: float             # F before
    residual_end: float               # F after
    lam: float                        # the damping at the end
    cg_iterations: int                # matrix-vector products over all solves
    cg_worst_residual: float          # the largest achieved |r| / |b| of a solve
    weights: torch.Tensor             # float64 [E] on the device: the line-process weight of every edge (1 for a certain one)
    residuals: torch.Tensor           # float64 [E] on the device: r_k = e^T Lambda e at the returned poses
    pruned: list                      # (source id, target id) of the edges optimize(prune=True) dropped


def information_from_point_clouds(source, target, max_correspondence_distance, transformation, index=None):
    """float64 [6,6] on the device: the information matrix of `transformation` between two clouds, sum of G^T G over the
    correspondences (nearest target point within max_correspondence_distance of every source point moved by `transformation`),
    unknowns (alpha, beta, gamma, tx, ty, tz); entry [3,3] is the number of correspondences.  One NeighborIndex query (`index`:
    an index built over `target` earlier), then gsr_registration_information.  No read-back."""
    src, index, md2, T = prepare(source, target, max_correspondence_distance, transformation, index, "information_from_point_clouds")
    _C = A.gsr()
    lib = _C.lib()
    dev = src.device
    Ps = int(src.shape[0])
    idx = torch.empty(Ps, dtype=torch.int32, device=dev)
    index._search(src, A.device_T(T, dev), md2, None, idx, None)
    info = torch.empty(6, 6, dtype=torch.float64, device=dev)
    stats = torch.empty(4, dtype=torch.float64, device=dev)
    with _C.on_device(dev):
        ws = torch.empty(lib.gsr_information_workspace_bytes(Ps), dtype=torch.uint8, device=dev)
        _C.check(lib.gsr_registration_information(index.size, _C.ptr(index.points), Ps, _C.ptr(idx), _C.ptr(info), _C.ptr(stats),
                                                  _C.ptr(ws), ws.numel(), _C._stream()))
    return info


def _check_information(info):
    """-> float64 numpy [6,6]; symmetric within SYMMETRY_TOL max |L|, finite, diagonal >= 0 (a device tensor is read back)"""
    if isinstance(info, torch.Tensor):
        info = info.detach().cpu().numpy()
    L = np.asarray(info, dtype=np.float64)
    if L.shape != (6, 6):
        raise ValueError(f"information: expected a [6,6] matrix, got {L.shape}")
    if not np.isfinite(L).all():
        raise ValueError("information: not finite")
    if np.abs(L - L.T).max() > SYMMETRY_TOL * np.abs(L).max():
        raise ValueError(f"information: not symmetric (|L - L^T| = {np.abs(L - L.T).max():.3g})")
    if (np.diag(L) < 0).any():
        raise ValueError(f"information: negative diagonal {np.diag(L).tolist()}")
    return L


def _check_rigid(T, name):
    """a [4,4] matrix as _check_transform takes it; given on the host it is held to validate_transforms"""
    on_host = not (isinstance(T, torch.Tensor) and T.is_cuda)
    T = A.transform(T, name)
    if T is None:
        raise ValueError(f"{name}: expected a [4,4] matrix, got None")
    if on_host:
        try:
            validate_transforms(T.detach().cpu().numpy().astype(np.float64))
        except ValueError as e:
            raise ValueError(f"{name}: {e}") from None
    return T.detach().to(torch.float64)


def _check_positive(name, value):
    return A.number(name, value, lambda v: math.isfinite(v) and v > 0, "a finite value > 0")


def _check_nonnegative(name, value):
    return A.number(name, value, lambda v: math.isfinite(v) and v >= 0, "a finite value >= 0")


class PoseGraph:
    """Keyframe poses and the relative transformations measured between them.  Node ids may be any hashable keyframe id; rows keep
    insertion order."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self._ids, self._row = [], {}
        self._X = torch.empty(0, 4, 4, dtype=torch.float64, device=self.device)      # current poses
        self._X0 = torch.empty(0, 4, 4, dtype=torch.float64, device=self.device)     # poses at the last commit
        self._fixed = []
        self._edges = []            # (source row, target row, T [4,4] where it was given, Lambda numpy [6,6], uncertain)
        self._pairs = set()
        self._topo = None           # the device blob of gsr_posegraph_topology for the current nodes and edges
        self._weights = None        # of the last optimize, while the edges are the same

    # ---- building ----
    def add_node(self, pose, fixed=False, id=None):
        """-> the node's id (`id`, or its row number): `pose` [4,4] maps the keyframe's frame to the world"""
        X = _check_rigid(pose, "pose")
        if id is None:
            id = len(self._ids)
        if id in self._row:
            raise ValueError(f"add_node: id {id!r} is already in the graph")
        self._row[id] = len(self._ids)
        self._ids.append(id)
        self._fixed.append(bool(fixed))
        X = X.to(self.device).reshape(1, 4, 4)
        self._X = torch.cat([self._X, X])
        self._X0 = torch.cat([self._X0, X])
        self._topo = self._weights = None
        return id

    def add_edge(self, source, target, transformation, information=None, uncertain=False):
        """`transformation` takes coordinates of node `source` to coordinates of node `target`: a [4,4] matrix, or the
        RegistrationResult / OdometryResult of registering `source`'s data onto `target`'s.  `information`: [6,6], None = the
        identity (a device tensor is read back once, here).  `uncertain`: a loop closure the line process may switch off."""
        if isinstance(transformation, (RegistrationResult, OdometryResult)):
            transformation = transformation.transformation
        for n in (source, target):
            if n not in self._row:
                raise ValueError(f"add_edge: node {n!r} is not in the graph")
        s, t = self._row[source], self._row[target]
        if s == t:
            raise ValueError(f"add_edge: a self-loop at node {source!r}")
        if (s, t) in self._pairs or (t, s) in self._pairs:
            raise ValueError(f"add_edge: nodes {source!r} and {target!r} are already joined")
        T = _check_rigid(transformation, "transformation")
        L = np.eye(6) if information is None else _check_information(information)
        self._pairs.add((s, t))
        self._edges.append((s, t, T, L, bool(uncertain)))
        self._topo = self._weights = None

    # ---- reading ----
    @property
    def ids(self):
        return list(self._ids)

    @property
    def poses(self):
        """float64 [N,4,4] on the device, rows in insertion order"""
        return self._X

    @property
    def edges(self):
        """[(source id, target id, uncertain)] in edge order"""
        return [(self._ids[s], self._ids[t], u) for s, t, _, _, u in self._edges]

    def pose(self, id):
        return self._X[self._row[id]]

    def updates(self, ids=None):
        """{id: T} with T = X_now X_at_last_commit^-1, float64 [4,4] on the device: what `correct_keyframes` takes (its all-device
        branch).  A node that has not moved since the commit gets the identity exactly.  No read-back."""
        ids = self._ids if ids is None else list(ids)
        if not ids:
            return {}
        rows = torch.tensor([self._row[i] for i in ids], dtype=torch.long, device=self.device)
        X, X0 = self._X[rows], self._X0[rows]
        inv = torch.zeros_like(X0)
        Rt = X0[:, :3, :3].transpose(1, 2)
        inv[:, :3, :3] = Rt
        inv[:, :3, 3] = -(Rt @ X0[:, :3, 3:4]).squeeze(2)
        inv[:, 3, 3] = 1.0
        T = X @ inv
        T[:, 3, :3] = 0.0
        T[:, 3, 3] = 1.0
        same = (X == X0).flatten(1).all(dim=1)
        T = torch.where(same[:, None, None], torch.eye(4, dtype=torch.float64, device=self.device), T)
        return {i: T[k] for k, i in enumerate(ids)}

    def commit(self):
        """The current poses become the baseline of `updates` (call it once the map has been moved)."""
        self._X0 = self._X.clone()

    # ---- optimisation ----
    def _validate(self):
        N = len(self._ids)
        if N < 1:
            raise ValueError("PoseGraph: no nodes")
        parent = list(range(N))

        def find(a):
            while parent[a] != a:
                parent[a] = parent[parent[a]]
                a = parent[a]
            return a
        for s, t, _, _, _ in self._edges:
            parent[find(s)] = find(t)
        anchored = {find(i) for i in range(N) if self._fixed[i]}
        for i in range(N):
            if find(i) not in anchored:
                raise ValueError(f"PoseGraph: the component of node {self._ids[i]!r} holds no fixed node: its gauge is free "
                                 "(add_node(..., fixed=True) for one of its nodes)")

    def _default_mu(self, max_correspondence_distance, preference_loop_closure, line_process_weight):
        if line_process_weight is not None:
            return _check_positive("line_process_weight", line_process_weight)
        if not any(e[4] for e in self._edges):
            return 1.0      # (no uncertain edge reads it)
        if max_correspondence_distance is None:
            raise ValueError("optimize: the graph has uncertain edges: give max_correspondence_distance or line_process_weight")
        md = A.number("max_correspondence_distance", max_correspondence_distance, lambda v: v >= 0 and not math.isinf(v),
                      "a value >= 0, finite")      # (false for NaN; worded as registration's distances are)
        pref = _check_positive("preference_loop_closure", preference_loop_closure)
        mu = pref * md * md * float(np.mean([e[3][3, 3] for e in self._edges]))
        if not mu > 0:
            raise ValueError(f"optimize: line-process weight {mu} (preference_loop_closure max_correspondence_distance^2 mean "
                             "Lambda[3,3]): expected > 0")
        return mu

    def _build_topology(self):
        _C = A.gsr()
        lib = _C.lib()
        N, E = len(self._ids), len(self._edges)
        ends = np.ascontiguousarray(np.array([(s, t) for s, t, _, _, _ in self._edges], dtype=np.int32).reshape(E, 2))
        fixed = np.ascontiguousarray(np.array(self._fixed, dtype=np.uint8))
        with _C.on_device(self.device):
            topo = torch.empty(lib.gsr_posegraph_topology_bytes(N, E), dtype=torch.uint8, device=self.device)
            scratch = np.zeros(topo.numel() // 4, dtype=np.int32)      # the blob on the host: kept beside it (include/gsr.h)
            _C.check(lib.gsr_posegraph_topology(N, E, ends.ctypes.data_as(C.POINTER(C.c_int32)),
                                                fixed.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_void_p(scratch.ctypes.data),
                                                _C.ptr(topo), topo.numel(), _C._stream()))
            if E:
                T = torch.stack([e[2].to(self.device) for e in self._edges]).contiguous()
                L = torch.as_tensor(np.stack([e[3] for e in self._edges])).to(self.device).contiguous()
                unc = torch.as_tensor(np.array([e[4] for e in self._edges], dtype=np.uint8)).to(self.device)
            else:
                T = L = unc = None
        self._topo = (topo, T, L, unc, scratch)

    def optimize(self, max_correspondence_distance=None, preference_loop_closure=1.0, line_process_weight=None, max_iteration=100,
                 min_relative_increment=1e-6, min_relative_residual_increment=1e-6, cg_rtol=1e-12, cg_max_iteration=None,
                 prune=False, prune_threshold=0.25):
        """Moves the free nodes to the minimum of F (include/gsr.h) in one launch -> PoseGraphResult; one read-back (the 16
        statistics).  The line-process weight mu is `line_process_weight`, or preference_loop_closure x
        max_correspondence_distance^2 x the mean of Lambda[3,3] over the edges (the correspondence count where Lambda came from
        `information_from_point_clouds`).  `prune=True`: optimise, drop the uncertain edges whose weight ended below
        `prune_threshold`, optimise again (Open3D's two passes).  `cg_max_iteration` defaults to min(6 N, 1000): block-Jacobi
        conjugate gradients need on the order of the graph's diameter in products, so a chain of several hundred keyframes with
        few chords reaches the cap before `cg_rtol` - the approximate step is then judged by the gain test, and a run can stop
        early (`result.cg_worst_residual` far above `cg_rtol` says so): give such graphs a larger cap or a looser `cg_rtol`.  ValueError before any device work: a component without a fixed
        node, bad options.  A graph on the CPU raises GsrError: there is no CPU path."""
        _C = A.gsr()
        self._validate()
        mu = self._default_mu(max_correspondence_distance, preference_loop_closure, line_process_weight)
        if not A.is_integer(max_iteration) or max_iteration < 0:
            raise ValueError(f"max_iteration={max_iteration!r}: expected an int >= 0")
        N = len(self._ids)
        if cg_max_iteration is None:
            cg_max_iteration = min(6 * N, 1000)
        if not A.is_integer(cg_max_iteration) or cg_max_iteration < 1:
            raise ValueError(f"cg_max_iteration={cg_max_iteration!r}: expected an int >= 1")
        mri = _check_nonnegative("min_relative_increment", min_relative_increment)
        mrri = _check_nonnegative("min_relative_residual_increment", min_relative_residual_increment)
        rtol = _check_nonnegative("cg_rtol", cg_rtol)
        thr = _check_nonnegative("prune_threshold", prune_threshold)
        if self.device.type != "cuda":
            raise _C.GsrError("PoseGraph.optimize runs in HIP kernels (no CPU path): the graph must live on the HIP device")
        first = self._run(mu, int(max_iteration), mri, mrri, rtol, int(cg_max_iteration))
        if not prune:
            return first
        pruned = self.prune_edges(thr)
        if not pruned:
            return first
        second = self._run(mu, int(max_iteration), mri, mrri, rtol, int(cg_max_iteration))
        return second._replace(iterations=first.iterations + second.iterations, accepted=first.accepted + second.accepted,
                               residual_start=first.residual_start, cg_iterations=first.cg_iterations + second.cg_iterations,
                               cg_worst_residual=max(first.cg_worst_residual, second.cg_worst_residual), pruned=pruned)

    def _run(self, mu, max_iteration, mri, mrri, rtol, cg_max):
        _C = A.gsr()
        lib = _C.lib()
        if self._topo is None:
            self._build_topology()
        topo, T, L, unc, _ = self._topo
        N, E = len(self._ids), len(self._edges)
        dev = self.device
        X = self._X.contiguous().clone()
        w = torch.empty(E, dtype=torch.float64, device=dev)
        r = torch.empty(E, dtype=torch.float64, device=dev)
        stats = torch.empty(16, dtype=torch.float64, device=dev)
        with _C.on_device(dev):
            ws = torch.empty(lib.gsr_posegraph_workspace_bytes(N, E), dtype=torch.uint8, device=dev)
            _C.check(lib.gsr_posegraph_optimize(N, E, _C.ptr(topo), _C.ptr(X), _C.ptr(T), _C.ptr(L), _C.ptr(unc), mu, max_iteration,
                                                mri, mrri, rtol, cg_max, _C.ptr(w) if E else None, _C.ptr(r) if E else None,
                                                _C.ptr(stats), _C.ptr(ws), ws.numel(), _C._stream()))
        s = stats.tolist()
        self._X = X
        self._weights = w
        status = int(s[0])
        return PoseGraphResult(status, status in CONVERGED, int(s[1]), int(s[2]), s[3], s[4], s[5], int(s[6]), s[7], w, r, [])

    def prune_edges(self, threshold=0.25):
        """Drops the uncertain edges whose weight of the last `optimize` is below `threshold` -> [(source id, target id)] of the
        dropped edges.  One read-back (the weights)."""
        thr = _check_nonnegative("threshold", threshold)
        if self._weights is None:
            raise ValueError("prune_edges: no weights: call optimize first (and do not change the graph in between)")
        w = self._weights.cpu().tolist()
        keep, dropped = [], []
        for e, wk in zip(self._edges, w):
            if e[4] and wk < thr:
                dropped.append((self._ids[e[0]], self._ids[e[1]]))
                self._pairs.discard((e[0], e[1]))
            else:
                keep.append(e)
        if dropped:
            self._edges = keep
            self._topo = self._weights = None
        return dropped
