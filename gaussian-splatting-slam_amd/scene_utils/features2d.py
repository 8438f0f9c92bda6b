"""Sparse image features for place recognition: FAST-9 corners on the halving levels of a FramePyramid, a 256-bit BRIEF descriptor
steered by the intensity centroid, brute-force Hamming matching, and a keyframe database that says which old keyframes the
current frame resembles (csrc/orb.hip; the rules, stated exactly, are in include/gsr.h).  The 3-D lift from depth hands matched
pixels to registration_ransac_based_on_feature_matching(pairs=...), so a revisit becomes a loop-closure edge of a PoseGraph.
This is not OpenCV's ORB - the sampling pattern is the library's own - and its descriptors are not interchangeable with OpenCV's.
There is no CPU path."""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import _args as A
from .cameras import camera_intrinsics
from .frames import Frame, build_pyramid, MAX_LEVELS
from .posegraph import information_from_point_clouds
from .registration import RegistrationResult, registration_icp, registration_ransac_based_on_feature_matching, _check_distance, \
    evaluate_registration, icp_update, transform_points

BORDER = 17          # GSR_ORB_BORDER
PER_CELL_MAX = 16    # GSR_ORB_PER_CELL_MAX
WORDS = 8            # int32 words of a descriptor


class OrbFeatures(NamedTuple):
    xy: torch.Tensor            # float32 [M,2]: the keypoint in level-0 pixels (the centre of its pixel of its own level)
    level: torch.Tensor         # int32 [M]
    angle_bin: torch.Tensor     # int32 [M]: 0 .. 29, bins of 12 degrees of atan2(m01, m10)
    score: torch.Tensor         # int32 [M]: the FAST-9 score
    descriptors: torch.Tensor   # int32 [M,8]: bit b in word b // 32 at position b % 32


def _check_descriptors(d, name, convert=True):
    if not isinstance(d, torch.Tensor) or d.dtype != torch.int32 or d.dim() != 2 or d.shape[1] != WORDS:
        raise ValueError(f"{name}: expected an int32 tensor of shape (N, {WORDS})")
    if not convert:
        return None
    if not d.is_cuda:
        raise A.gsr().GsrError(f"{name} must live on the HIP device (no CPU path)")
    return d.contiguous()


def _descriptors_of(f, name, convert=True):
    return _check_descriptors(f.descriptors if isinstance(f, OrbFeatures) else f, name, convert)


def _check_match(max_distance, ratio):
    return (A.integer("max_distance", max_distance, 0, 256),
            A.number("ratio", ratio, lambda v: 0.0 <= v <= 1.0, "0 .. 1.0"))      # (false for NaN)


# ---- the three image kernels, one level ---------------------------------------------------------------------------------------------
def orb_prepare(image):
    """gsr_orb_prepare: `image` [3,H,W] (intensity ((r + g) + b) / 3) or [H,W] on the HIP device -> (u8 uint8 [H,W], box int16
    [H,W] holding the uint16 5 x 5 sums)."""
    A.tensor(image, "image", (3, "H", "W"), also=("H", "W"), convert=False)
    img = A.tensor(image, "image", (3, "H", "W"), also=("H", "W"))
    _C = A.gsr()
    H, W = int(img.shape[-2]), int(img.shape[-1])
    u8 = torch.empty((H, W), dtype=torch.uint8, device=img.device)
    box = torch.empty((H, W), dtype=torch.int16, device=img.device)
    with _C.on_device(img.device):
        _C.check(_C.lib().gsr_orb_prepare(W, H, _C.ptr(img), 3 if img.dim() == 3 else 1, _C.ptr(u8), _C.ptr(box), _C._stream()))
    return u8, box


def orb_detect(u8, threshold=20, per_cell=4, mask=None):
    """gsr_orb_detect -> slots int32 [cells, per_cell, 3] = (x, y, score), score 0 = empty: the per_cell best corners of every
    32 x 32 cell, by score descending then raster order.  No read-back."""
    thr = A.integer("threshold", threshold, 0, 254)
    pc = A.integer("per_cell", per_cell, 1, PER_CELL_MAX)
    if not isinstance(u8, torch.Tensor) or u8.dtype != torch.uint8 or u8.dim() != 2:
        raise ValueError("u8: expected a uint8 tensor of shape (H, W)")
    if not u8.is_cuda:
        raise A.gsr().GsrError("u8 must live on the HIP device (no CPU path)")
    H, W = int(u8.shape[0]), int(u8.shape[1])
    m = None if mask is None else A.tensor(mask, "mask", (H, W)).to(u8.device)
    _C = A.gsr()
    lib = _C.lib()
    u8 = u8.contiguous()
    slots = torch.empty((int(lib.gsr_orb_cells(W, H)), pc, 3), dtype=torch.int32, device=u8.device)
    with _C.on_device(u8.device):
        _C.check(lib.gsr_orb_detect(W, H, _C.ptr(u8), _C.ptr(m), thr, pc, _C.ptr(slots), _C._stream()))
    return slots


def orb_describe(u8, box, keypoints, return_moments=False):
    """gsr_orb_describe: keypoints int32 [M,3] = (x, y, score) -> (angle_bin int32 [M], descriptors int32 [M,8][, moments int32
    [M,2]]); a row with score <= 0 or inside the border of 17: bin -1 and a zero descriptor."""
    if not isinstance(keypoints, torch.Tensor) or keypoints.dtype != torch.int32 or keypoints.dim() != 2 or keypoints.shape[1] != 3:
        raise ValueError("keypoints: expected an int32 tensor of shape (M, 3): x, y, score")
    for t, n, dt in ((u8, "u8", torch.uint8), (box, "box", torch.int16)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt or t.dim() != 2:
            raise ValueError(f"{n}: expected a {str(dt).split('.')[-1]} tensor of shape (H, W)")
    if tuple(box.shape) != tuple(u8.shape):
        raise ValueError(f"box: expected {tuple(u8.shape)} like u8, got {tuple(box.shape)}")
    if not (u8.is_cuda and box.is_cuda and keypoints.is_cuda):
        raise A.gsr().GsrError("orb_describe needs its tensors on the HIP device (no CPU path)")
    _C = A.gsr()
    dev = u8.device
    H, W = int(u8.shape[0]), int(u8.shape[1])
    kp = keypoints.contiguous()
    M = int(kp.shape[0])
    bins = torch.empty(M, dtype=torch.int32, device=dev)
    desc = torch.empty((M, WORDS), dtype=torch.int32, device=dev)
    mom = torch.empty((M, 2), dtype=torch.int32, device=dev) if return_moments else None
    if M:
        with _C.on_device(dev):
            _C.check(_C.lib().gsr_orb_describe(W, H, _C.ptr(u8.contiguous()), _C.ptr(box.contiguous()), M, _C.ptr(kp), _C.ptr(bins),
                                               _C.ptr(mom), _C.ptr(desc), _C._stream()))
    return (bins, desc, mom) if return_moments else (bins, desc)


# ---- detection over the pyramid -------------------------------------------------------------------------------------------------------
def detect_orb(frame_or_image, levels=4, threshold=20, per_cell=4, max_keypoints=2000, mask=None):
    """-> OrbFeatures of a Frame (its validity mask applies, AND `mask`) or of an image [3,H,W] / [H,W] on the HIP device.
    `levels` pyramid levels (1 .. 4: FramePyramid's halving levels 0 .. levels - 1); a level too small for the border of 17
    contributes nothing.  Per level: prepare, detect (the `per_cell` best corners of every 32 x 32 cell above `threshold`),
    describe.  The final cut to `max_keypoints` is by score descending, then level, y, x ascending.  One read-back: the count."""
    n_levels = A.integer("levels", levels, 1, MAX_LEVELS + 1)
    A.integer("threshold", threshold, 0, 254)
    A.integer("per_cell", per_cell, 1, PER_CELL_MAX)
    cap = A.integer("max_keypoints", max_keypoints, 1)
    if isinstance(frame_or_image, Frame):
        image, fmask = frame_or_image.image, frame_or_image.mask
    else:
        image, fmask = frame_or_image, None
    A.tensor(image, "image", (3, "H", "W"), also=("H", "W"), convert=False)
    H, W = int(image.shape[-2]), int(image.shape[-1])
    if mask is not None:
        A.tensor(mask, "mask", (H, W), convert=False)
    img = A.tensor(image, "image", (3, "H", "W"), also=("H", "W"))
    dev = img.device
    grey = img.dim() == 2
    if mask is not None:
        mask = A.tensor(mask, "mask", (H, W)).to(dev)
        fmask = mask if fmask is None else ((fmask.to(dev) > 0) & (mask > 0)).float()
    while n_levels > 1 and min(W >> (n_levels - 1), H >> (n_levels - 1)) < 2 * BORDER + 1:      # (such a level has no keypoint)
        n_levels -= 1
    images, masks = [img], [fmask]
    if n_levels > 1:
        c, _, m = build_pyramid(img.expand(3, H, W) if grey else img, None, fmask, n_levels - 1)
        images += [t[0] if grey else t for t in c]
        masks += [None] * (n_levels - 1) if m is None else m
    xs, lv, bins, scores, descs = [], [], [], [], []
    for l in range(n_levels):
        h, w = int(images[l].shape[-2]), int(images[l].shape[-1])
        if w < 2 * BORDER + 1 or h < 2 * BORDER + 1:
            continue
        u8, box = orb_prepare(images[l])
        slots = orb_detect(u8, threshold, per_cell, masks[l]).reshape(-1, 3)
        b, d = orb_describe(u8, box, slots)
        xs.append(slots)
        lv.append(torch.full((int(slots.shape[0]),), l, dtype=torch.int32, device=dev))
        bins.append(b)
        descs.append(d)
    if not xs:
        z = torch.zeros(0, dtype=torch.int32, device=dev)
        return OrbFeatures(torch.zeros((0, 2), dtype=torch.float32, device=dev), z, z.clone(), z.clone(),
                           torch.zeros((0, WORDS), dtype=torch.int32, device=dev))
    slots, lv, bins, descs = torch.cat(xs), torch.cat(lv), torch.cat(bins), torch.cat(descs)
    x, y, s = slots[:, 0].long(), slots[:, 1].long(), slots[:, 2].long()
    key = ((255 - s) << 40) | (lv.long() << 36) | (y << 18) | x
    key = torch.where(s > 0, key, torch.full_like(key, 2 ** 62))
    order = torch.sort(key).indices
    count = min(int((s > 0).sum().item()), cap)
    keep = order[:count]
    scale = torch.pow(2.0, lv[keep].float()).unsqueeze(1)
    xy = (slots[keep, :2].float() + 0.5) * scale - 0.5
    return OrbFeatures(xy.contiguous(), lv[keep].contiguous(), bins[keep].contiguous(), slots[keep, 2].contiguous(),
                       descs[keep].contiguous())


# ---- matching ----------------------------------------------------------------------------------------------------------------------------
def hamming_match(query, database):
    """gsr_hamming_match -> (idx, best, second) int32 [Q]: the nearest database row of every query row (ties: the lowest row), its
    distance and the second smallest distance; -1 / 257 where there is none.  No read-back."""
    _check_descriptors(query, "query", convert=False)
    _check_descriptors(database, "database", convert=False)
    q, t = _check_descriptors(query, "query"), _check_descriptors(database, "database")
    if q.device != t.device:
        raise ValueError(f"hamming_match: query on {q.device}, database on {t.device}")
    Q, N = int(q.shape[0]), int(t.shape[0])
    out = [torch.empty(Q, dtype=torch.int32, device=q.device) for _ in range(3)]
    if Q:
        _C = A.gsr()
        with _C.on_device(q.device):
            _C.check(_C.lib().gsr_hamming_match(Q, _C.ptr(q), N, _C.ptr(t) if N else None, _C.ptr(out[0]), _C.ptr(out[1]),
                                                _C.ptr(out[2]), _C._stream()))
    return tuple(out)


def match_descriptors(a, b, max_distance=64, ratio=0.8, mutual=True):
    """int32 [m,2] on the device, ascending in the first column: (i, j) with j the row of `b` nearest to row i of `a` (OrbFeatures
    or int32 [N,8]), kept where the distance is <= max_distance and < ratio * the second smallest distance (float32).  mutual:
    only the pairs for which the same holds with the roles swapped and whose row j has i as ITS nearest row - a subset of the
    result without it, and the same pairs, flipped, as match_descriptors(b, a)."""
    md, rt = _check_match(max_distance, ratio)
    if not isinstance(mutual, bool):
        raise TypeError(f"mutual={mutual!r}: expected a bool")
    _descriptors_of(a, "a", convert=False)
    _descriptors_of(b, "b", convert=False)
    da, db = _descriptors_of(a, "a"), _descriptors_of(b, "b")

    def passing(q, t):
        idx, best, second = hamming_match(q, t)
        return idx, (idx >= 0) & (best <= md) & (best.float() < torch.tensor(rt, dtype=torch.float32) * second.float())
    fwd, keep = passing(da, db)
    rows = torch.arange(int(da.shape[0]), dtype=torch.int32, device=da.device)
    if mutual and int(db.shape[0]):
        back, ok = passing(db, da)
        j = fwd.clamp(min=0).long()
        keep = keep & ok[j] & (back[j] == rows)
    return torch.stack([rows[keep], fwd[keep]], dim=1).contiguous()


# ---- the lift to 3-D and the relative pose ----------------------------------------------------------------------------------------------
def _check_depth_range(min_depth, max_depth):
    lo = A.number("min_depth", min_depth, lambda v: v >= 0, "a value >= 0")      # (false for NaN)
    hi = A.number("max_depth", max_depth, lambda v: v > lo, f"a value > min_depth={min_depth}")
    return lo, hi


def keypoint_points(features, depth, camera, min_depth=0.0, max_depth=float("inf")):
    """-> (xyz float32 [M,3] in the camera frame, valid bool [M]): every keypoint lifted by the depth read at the nearest level-0
    pixel, x = (u - cx) d / fx, y = (v - cy) d / fy, z = d with (u, v) the keypoint; valid iff the pixel lies inside the image
    and min_depth < d <= max_depth, d finite (unproject_rgbd's rule); an invalid row is 0 0 0."""
    if not isinstance(features, OrbFeatures):
        raise TypeError(f"features: expected OrbFeatures, got {type(features).__name__}")
    lo, hi = _check_depth_range(min_depth, max_depth)
    W, H = int(camera.image_width), int(camera.image_height)
    A.tensor(depth, "depth", (H, W), also=(1, H, W), convert=False)
    d = A.tensor(depth, "depth", (H, W), also=(1, H, W)).reshape(H, W)
    fx, fy, cx, cy = camera_intrinsics(camera)
    xy = features.xy.to(d.device)
    px = torch.floor(xy + 0.5).long()
    inside = (px[:, 0] >= 0) & (px[:, 0] < W) & (px[:, 1] >= 0) & (px[:, 1] < H)
    z = d[px[:, 1].clamp(0, H - 1), px[:, 0].clamp(0, W - 1)]
    valid = inside & torch.isfinite(z) & (z > lo) & (z <= hi)
    z = torch.where(valid, z, torch.zeros_like(z))
    xyz = torch.stack([(xy[:, 0] - cx) / fx * z, (xy[:, 1] - cy) / fy * z, z], dim=1)
    return xyz.contiguous(), valid


def relative_pose_from_features(fa, depth_a, cam_a, fb, depth_b, cam_b, max_correspondence_distance, min_depth=0.0,
                                max_depth=float("inf"), max_distance=64, ratio=0.8, mutual=True, refit=True, **ransac):
    """The rigid transformation from camera frame a to camera frame b out of two frames' features: match_descriptors, both sides
    lifted by their depth, pairs with an invalid side dropped, then registration_ransac_based_on_feature_matching(pairs=...) over
    the lifted keypoints (`ransac`: its keywords) -> RegistrationResult whose fitness, RMSE and correspondences are measured on
    the valid keypoints of a against those of b.  refit: the winning trial, a fit to ransac_n pairs, is followed by one
    least-squares update over all pairs within the distance under it.  Fewer than ransac_n usable pairs: the identity,
    converged False."""
    if not isinstance(refit, bool):
        raise TypeError(f"refit={refit!r}: expected a bool")
    md = _check_distance("max_correspondence_distance", max_correspondence_distance, False)
    pairs = match_descriptors(fa, fb, max_distance, ratio, mutual)
    xa, va = keypoint_points(fa, depth_a, cam_a, min_depth, max_depth)
    xb, vb = keypoint_points(fb, depth_b, cam_b, min_depth, max_depth)
    pairs = pairs[va[pairs[:, 0].long()] & vb[pairs[:, 1].long()]]
    # the clouds RANSAC sees hold the valid keypoints only, so that its closing fitness counts no (0, 0, 0) row
    ia, ib = torch.cumsum(va.int(), 0, dtype=torch.int32) - 1, torch.cumsum(vb.int(), 0, dtype=torch.int32) - 1
    pairs = torch.stack([ia[pairs[:, 0].long()], ib[pairs[:, 1].long()]], dim=1).contiguous()
    src, tgt = xa[va], xb[vb]
    if int(src.shape[0]) == 0 or int(tgt.shape[0]) == 0:
        eye = torch.eye(4, dtype=torch.float64, device=xa.device)
        return RegistrationResult(eye, 0.0, 0.0, 0, False, torch.full((int(src.shape[0]),), -1, dtype=torch.int32, device=xa.device))
    res = registration_ransac_based_on_feature_matching(src, tgt, None, None, False, md, pairs=pairs, **ransac)
    if not (refit and res.converged):
        return res
    # the winning trial is a fit to ransac_n pairs: one Kabsch update (gsr_icp_update) over ALL pairs that lie within the distance
    # under it
    moved = transform_points(src, res.transformation)
    i, j = pairs[:, 0].long(), pairs[:, 1].long()
    inlier = ((moved[i] - tgt[j]) ** 2).sum(dim=1) <= A.sq(md)
    corr = torch.full((int(src.shape[0]),), -1, dtype=torch.int32, device=src.device)
    corr[i[inlier]] = pairs[:, 1][inlier]
    T, _ = icp_update(src, tgt, corr, res.transformation)
    fit = evaluate_registration(src, tgt, md, T)
    return RegistrationResult(fit.transformation, fit.fitness, fit.inlier_rmse, res.iterations, True, fit.correspondences)


# ---- the keyframe database ---------------------------------------------------------------------------------------------------------------
class PlaceEntry(NamedTuple):
    kf_id: object
    features: OrbFeatures
    frame: object               # the keyframe's Frame (depth and camera for loop_closure_edge), or None


class PlaceDatabase:
    """The descriptors of every keyframe added so far, one behind the other in one device buffer (append-only; the buffer doubles
    when it is full).  query() runs gsr_hamming_vote: one grid row per keyframe, one vote per query descriptor that finds a
    distinctive match inside that keyframe."""

    def __init__(self, device="cuda", max_distance=64, ratio=0.8):
        self.device = torch.device(device)
        self.max_distance, self.ratio = _check_match(max_distance, ratio)
        self._desc = torch.zeros((0, WORDS), dtype=torch.int32, device=self.device)
        self._rows = 0
        self._offsets = [0]
        self._segments = None       # device int32 [K+1], rebuilt after an add
        self._entries = []
        self._row_of = {}

    def __len__(self):
        return len(self._entries)

    def __getitem__(self, kf_id):
        return self._entries[self._row_of[kf_id]]

    def __contains__(self, kf_id):
        return kf_id in self._row_of

    def _grow(self, rows):
        cap = int(self._desc.shape[0])
        if rows <= cap:
            return
        t = torch.zeros((max(rows, 2 * cap, 1024), WORDS), dtype=torch.int32, device=self.device)
        t[:self._rows] = self._desc[:self._rows]
        self._desc = t

    def add(self, kf_id, features, frame=None):
        """appends keyframe `kf_id` (any hashable id, not yet present); `frame` is kept beside it for loop_closure_edge"""
        if not isinstance(features, OrbFeatures):
            raise TypeError(f"features: expected OrbFeatures, got {type(features).__name__}")
        if kf_id in self._row_of:
            raise ValueError(f"add: keyframe {kf_id!r} is already in the database")
        if len(self._entries) >= 65535:
            raise ValueError("add: the database holds 65535 keyframes")
        d = _check_descriptors(features.descriptors, "features.descriptors").to(self.device)
        n = int(d.shape[0])
        self._grow(self._rows + n)
        self._desc[self._rows:self._rows + n] = d
        self._rows += n
        self._offsets.append(self._rows)
        self._row_of[kf_id] = len(self._entries)
        self._entries.append(PlaceEntry(kf_id, features, frame))
        self._segments = None

    def votes(self, features):
        """int32 [K] on the device, in insertion order: gsr_hamming_vote of the query's descriptors.  No read-back."""
        q = _descriptors_of(features, "features").to(self.device)
        K = len(self._entries)
        out = torch.zeros(K, dtype=torch.int32, device=self.device)
        if K:
            if self._segments is None:
                self._segments = torch.tensor(self._offsets, dtype=torch.int32, device=self.device)
            _C = A.gsr()
            Q = int(q.shape[0])
            with _C.on_device(self.device):
                _C.check(_C.lib().gsr_hamming_vote(Q, _C.ptr(q) if Q else None, self._rows, _C.ptr(self._desc) if self._rows else None,
                                                   K, _C.ptr(self._segments), self.max_distance, self.ratio, _C.ptr(out),
                                                   _C._stream()))
        return out

    def query(self, features, exclude=(), top_k=5, min_votes=20):
        """-> [(kf_id, votes)]: the at most `top_k` keyframes with at least `min_votes` votes, none of `exclude`, ranked by votes
        descending, then by insertion order.  One read-back: the K counts."""
        k = A.integer("top_k", top_k, 1)
        mv = A.integer("min_votes", min_votes, 0)
        skip = set(exclude)
        counts = self.votes(features).tolist()
        ranked = sorted((-v, r) for r, v in enumerate(counts) if v >= mv and self._entries[r].kf_id not in skip)
        return [(self._entries[r].kf_id, -nv) for nv, r in ranked[:k]]


def _frame_cloud(frame, stride, min_depth, max_depth):
    """the valid pixels of every stride-th row and column, lifted into the camera frame: float32 [P,3]"""
    H, W = int(frame.depth.shape[-2]), int(frame.depth.shape[-1])
    d = frame.depth.reshape(H, W)[::stride, ::stride]
    dev = d.device
    fx, fy, cx, cy = camera_intrinsics(frame.camera)
    v, u = torch.meshgrid(torch.arange(0, H, stride, device=dev, dtype=torch.float32),
                          torch.arange(0, W, stride, device=dev, dtype=torch.float32), indexing="ij")
    ok = torch.isfinite(d) & (d > min_depth) & (d <= max_depth)
    if frame.mask is not None:
        ok &= frame.mask.reshape(H, W)[::stride, ::stride] > 0
    return torch.stack([(u - cx) / fx * d, (v - cy) / fy * d, d], dim=-1)[ok].contiguous()


def loop_closure_edge(db_entry, frame, features=None, max_correspondence_distance=0.05, min_fitness=0.3, icp_distance=None,
                      stride=4, min_depth=0.0, max_depth=float("inf"), icp=None, **pose):
    """A loop-closure edge from the keyframe `db_entry` (a PlaceEntry with its frame, e.g. db[kf_id]) to `frame` (`features`: its
    OrbFeatures, detected here when None): relative_pose_from_features (`pose`: its keywords), None when its fitness is below
    `min_fitness` or no trial survived; refined by registration_icp on the two frames' clouds (every `stride`-th pixel, within
    `icp_distance`, default max_correspondence_distance; `icp`: a dict of its keywords), then information_from_point_clouds ->
    (transformation float64 [4,4], information float64 [6,6]), both on the device, taking coordinates of the keyframe's camera to
    those of `frame`'s: PoseGraph.add_edge(kf_id, frame_id, transformation, information, uncertain=True)."""
    if not isinstance(db_entry, PlaceEntry) or db_entry.frame is None or db_entry.frame.depth is None:
        raise ValueError("db_entry: expected a PlaceEntry that holds its frame with depth (PlaceDatabase.add(..., frame=...))")
    if not isinstance(frame, Frame) or frame.depth is None:
        raise ValueError("frame: expected a Frame with depth")
    md = _check_distance("max_correspondence_distance", max_correspondence_distance, False)
    floor = A.number("min_fitness", min_fitness, lambda v: 0.0 <= v <= 1.0, "0 .. 1.0")
    st = A.integer("stride", stride, 1)
    fine = md if icp_distance is None else _check_distance("icp_distance", icp_distance, False)
    lo, hi = _check_depth_range(min_depth, max_depth)
    if features is None:
        features = detect_orb(frame)
    old = db_entry.frame
    coarse = relative_pose_from_features(db_entry.features, old.depth, old.camera, features, frame.depth, frame.camera, md,
                                         min_depth=lo, max_depth=hi, **pose)
    if not coarse.converged or coarse.fitness < floor:
        return None
    src, tgt = _frame_cloud(old, st, lo, hi), _frame_cloud(frame, st, lo, hi)
    if int(src.shape[0]) == 0 or int(tgt.shape[0]) == 0:
        return None
    res = registration_icp(src, tgt, fine, init=coarse.transformation, **(icp or {}))
    return res.transformation, information_from_point_clouds(src, tgt, fine, res.transformation)


__all__ = ["OrbFeatures", "PlaceEntry", "PlaceDatabase", "detect_orb", "match_descriptors", "hamming_match", "keypoint_points",
           "relative_pose_from_features", "loop_closure_edge", "orb_prepare", "orb_detect", "orb_describe"]
