"""Keyframe covisibility for a SLAM back end, from the rasterizer's per-Gaussian visibility counts (`render(...,
n_touched=True)`: for every Gaussian the number of pixels that blend it while still less than `touched_T_min` occluded).
Three decisions hang on "which Gaussians did this frame SEE": whether a tracked frame becomes a keyframe (its overlap with the
last one), which old keyframe leaves the mapping window (the one that shares least with the newest) and which freshly inserted
Gaussians are spurious (seen from too few keyframes).  `radii > 0` cannot answer them: it ignores occlusion.

Pure torch, works on CPU tensors.  Every threshold here is an argument with a default taken from common practice in
Gaussian-splatting SLAM systems: they are POLICY KNOBS, not optima measured on this code base."""
from __future__ import annotations

import torch


def _as_mask(v, min_pixels=1, name="n_touched"):
    """bool [P] of a counts vector (count >= min_pixels) or of a bool mask (taken as it is)."""
    if not isinstance(v, torch.Tensor) or v.dim() != 1:
        raise ValueError(f"{name}: expected a 1-D tensor of counts or a bool mask")
    return v if v.dtype == torch.bool else v >= int(min_pixels)


def covisibility(a, b, min_pixels=1):
    """-> (iou, overlap) of two frames' visible sets A, B.  `a`, `b`: their n_touched vectors (a row is visible when its count
    is >= min_pixels) or bool masks, of EQUAL length (anything else raises: the vectors index the same map).
    iou = |A n B| / |A u B|; overlap = |A n B| / min(|A|, |B|), the overlap coefficient; both 0.0 when a set is empty.
    `min_pixels` is a policy knob (1 = any pixel at all), not a measured optimum."""
    A, B = _as_mask(a, min_pixels, "a"), _as_mask(b, min_pixels, "b")
    if A.shape[0] != B.shape[0]:
        raise ValueError(f"covisibility: lengths differ ({A.shape[0]} and {B.shape[0]}): both must index the same map")
    B = B.to(A.device)
    inter = int((A & B).sum().item())
    na, nb = int(A.sum().item()), int(B.sum().item())
    union = na + nb - inter
    if inter == 0 or min(na, nb) == 0:
        return 0.0, 0.0
    return inter / union, inter / min(na, nb)


class KeyframeWindow:
    """The mapping window: at most `size` keyframes, each a caller-supplied id and the bool visibility row of its frame over the
    map's P Gaussians.  All rows have the same length; after the map changes size call `resized` (prune_unobserved does)."""

    def __init__(self, size, min_pixels=1):
        if int(size) < 1:
            raise ValueError(f"size={size}: expected at least 1")
        self.size = int(size)
        self.min_pixels = int(min_pixels)     # a row is visible in a frame when its count is >= this (policy knob)
        self.ids = []                         # oldest first
        self.rows = []                        # bool [P] each

    def __len__(self):
        return len(self.ids)

    def _row(self, n_touched):
        row = _as_mask(n_touched, self.min_pixels)
        if self.rows and row.shape[0] != self.rows[-1].shape[0]:
            raise ValueError(f"n_touched has {row.shape[0]} rows, the window's keyframes {self.rows[-1].shape[0]}: call "
                             "resized() after the map changed size")
        return row

    def is_keyframe(self, n_touched, iou_below=0.9):
        """True when the window is empty or the IoU of this frame's visible set with the NEWEST keyframe's is below
        `iou_below` (a policy knob, not a measured optimum: lower = fewer keyframes)."""
        row = self._row(n_touched)
        if not self.rows:
            return True
        return covisibility(row, self.rows[-1])[0] < float(iou_below)

    def add(self, kf_id, n_touched, overlap_cutoff=0.4):
        """Appends the keyframe and returns the list of evicted ids: first every OLDER keyframe whose overlap coefficient with
        the new one is <= `overlap_cutoff` (it no longer looks at what is being mapped) - except the newest two of the window,
        which the cutoff never evicts - then, while the window holds more than `size`, the oldest.  `overlap_cutoff` is a policy
        knob, not a measured optimum."""
        row = self._row(n_touched).clone()
        self.ids.append(kf_id)
        self.rows.append(row)
        evicted = []
        keep_ids, keep_rows = [], []
        n = len(self.ids)
        for i, (k, r) in enumerate(zip(self.ids, self.rows)):
            if i < n - 2 and covisibility(r, row)[1] <= float(overlap_cutoff):
                evicted.append(k)
            else:
                keep_ids.append(k)
                keep_rows.append(r)
        while len(keep_ids) > self.size:
            evicted.append(keep_ids.pop(0))
            keep_rows.pop(0)
        self.ids, self.rows = keep_ids, keep_rows
        return evicted

    def observations(self):
        """int32 [P]: how many of the window's keyframes see each row (an empty window: an empty tensor)."""
        if not self.rows:
            return torch.zeros(0, dtype=torch.int32)
        return torch.stack(self.rows, dim=0).sum(dim=0, dtype=torch.int32)

    def resized(self, new_P, keep=None):
        """Follows a change of the map.  After an insertion (keep=None): every row is padded with False up to `new_P` (a new
        Gaussian has been seen by no earlier keyframe).  After a prune: `keep` (bool [old P], = ~mask of prune_points) selects
        the surviving rows, which must be `new_P`.  A length that does not fit raises, nothing is broadcast.  Returns self."""
        new_P = int(new_P)
        out = []
        for r in self.rows:
            if keep is None:
                if new_P < r.shape[0]:
                    raise ValueError(f"resized: new_P={new_P} is smaller than the rows ({r.shape[0]}): pass keep= after a prune")
                out.append(torch.cat([r, torch.zeros(new_P - r.shape[0], dtype=torch.bool, device=r.device)]))
            else:
                if not isinstance(keep, torch.Tensor) or keep.dtype != torch.bool or tuple(keep.shape) != (r.shape[0],):
                    raise ValueError(f"resized: keep must be a bool mask over the {r.shape[0]} old rows")
                k = r[keep.to(r.device)]
                if k.shape[0] != new_P:
                    raise ValueError(f"resized: keep selects {k.shape[0]} rows, new_P={new_P}")
                out.append(k)
        self.rows = out
        return self


def prune_unobserved(model, window, candidates, min_keyframes=3):
    """Removes the `candidates` (bool [P], typically the rows inserted since some keyframe) that fewer than `min_keyframes` of
    the window's keyframes see - a Gaussian born from a depth outlier is seen by the frame that made it and hardly any other -
    through `model.prune_points`, then brings the window's rows in line (`window.resized`).  Returns how many were removed.
    `min_keyframes` is a policy knob, not a measured optimum; with fewer keyframes in the window than that nothing is pruned
    (no candidate could pass)."""
    P = int(model.get_xyz.shape[0])
    if not isinstance(candidates, torch.Tensor) or candidates.dtype != torch.bool or tuple(candidates.shape) != (P,):
        raise ValueError(f"prune_unobserved: candidates must be a bool mask over the model's {P} rows")
    if len(window) < int(min_keyframes):
        return 0
    obs = window.observations()
    if obs.shape[0] != P:
        raise ValueError(f"prune_unobserved: the window's rows have {obs.shape[0]} entries, the model {P}: call resized() first")
    dev = model.get_xyz.device
    mask = candidates.to(dev) & (obs.to(dev) < int(min_keyframes))
    n = model.prune_points(mask)
    if n:
        window.resized(P - n, keep=~mask)
    return n
