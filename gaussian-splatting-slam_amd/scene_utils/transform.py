"""The map follows pose corrections: Gaussians that are already in the model move into a corrected world frame.

A loop closure or a pose-graph update moves keyframes, an alignment to another frame (GPS, a second sub-map) moves everything,
possibly with a scale factor.  A correction is a similarity x' = s R x + t given as a float64 4x4 matrix [[s R, t], [0, 1]].
`GaussianModel.transform_` applies one to every row, or one per keyframe to the rows that keyframe created (`model._anchor`),
in ONE pass of HIP kernels (csrc/transform.hip, gsr_transform_gaussians): positions in float64, rotations composed, log-scales
shifted by ln s, the view-dependent SH bands of `_features_rest` rotated with their real-SH rotation matrices, the Adam moments
of the moved rows zeroed.  There is no CPU path.  `transform_camera` gives the camera that sees the moved map as the old camera
saw the old one; `correct_keyframes` is the loop-closure call that does both."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _args as A
from .cameras import MiniCam, camera_projection
from .model import GaussianModel

_MOVED_GROUPS = ("_xyz", "_rotation", "_scaling", "_features_rest")      # the order of gsr_transform_gaussians' moments8
ORTHO_TOL = 1e-6       # max |R R^T - I|, |s - 1| and the bottom row's deviation a validated matrix may show


def _as_stack(T):
    """-> (float64 tensor [K,4,4] where T lives, whether T was given on the host)"""
    if not isinstance(T, torch.Tensor):
        T = torch.as_tensor(np.asarray(T, dtype=np.float64))
    if T.dim() == 2:
        T = T.unsqueeze(0)
    if T.dim() != 3 or tuple(T.shape[1:]) != (4, 4):
        raise ValueError(f"transform: expected [4,4] or [K,4,4], got {tuple(T.shape)}")
    if not T.is_floating_point():
        raise ValueError(f"transform: expected a floating-point matrix, got {T.dtype}")
    return T.detach().to(torch.float64), not T.is_cuda


def decompose(T):
    """One 4x4 similarity (anything np.asarray takes) -> (s, R [3,3], t [3]) in float64: s = det(s R)^(1/3)."""
    T = np.asarray(T, dtype=np.float64)
    M = T[:3, :3]
    s = float(np.cbrt(np.linalg.det(M)))
    return s, M / s, T[:3, 3].copy()


def validate_transforms(T, allow_scale=False):
    """Raises ValueError unless every T[k] is [[s R, t], [0 0 0 1]] with R a proper rotation and s > 0 (s == 1 unless
    `allow_scale`), all within ORTHO_TOL."""
    T = np.asarray(T, dtype=np.float64).reshape(-1, 4, 4)
    for k, Tk in enumerate(T):
        if not np.isfinite(Tk).all():
            raise ValueError(f"transform {k}: not finite")
        if np.abs(Tk[3] - np.array([0.0, 0.0, 0.0, 1.0])).max() > ORTHO_TOL:
            raise ValueError(f"transform {k}: bottom row {Tk[3].tolist()}, expected (0, 0, 0, 1)")
        det = float(np.linalg.det(Tk[:3, :3]))
        if not det > 0.0:
            raise ValueError(f"transform {k}: det = {det:.3g} <= 0 (a reflection or a singular matrix)")
        s, R, _ = decompose(Tk)
        err = float(np.abs(R @ R.T - np.eye(3)).max())
        if err > ORTHO_TOL:
            raise ValueError(f"transform {k}: upper-left block is not s R with R a rotation (|R R^T - I| = {err:.3g})")
        if not allow_scale and abs(s - 1.0) > ORTHO_TOL:
            raise ValueError(f"transform {k}: scale factor {s:.9g}; pass allow_scale=True to apply a similarity")


def quat_from_matrix(R):
    """Unit quaternion (w, x, y, z) of a rotation matrix, float64 - Shepperd's method with the sign convention of the table
    kernel: the largest of (trace, R00, R11, R22) picks the component formed from a square root, which is positive."""
    R = np.asarray(R, dtype=np.float64)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr >= R[0, 0] and tr >= R[1, 1] and tr >= R[2, 2]:
        r = np.sqrt(1.0 + tr)
        q = [0.5 * r, (R[2, 1] - R[1, 2]) * 0.5 / r, (R[0, 2] - R[2, 0]) * 0.5 / r, (R[1, 0] - R[0, 1]) * 0.5 / r]
    elif R[0, 0] >= R[1, 1] and R[0, 0] >= R[2, 2]:
        r = np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2])
        q = [(R[2, 1] - R[1, 2]) * 0.5 / r, 0.5 * r, (R[0, 1] + R[1, 0]) * 0.5 / r, (R[0, 2] + R[2, 0]) * 0.5 / r]
    elif R[1, 1] >= R[2, 2]:
        r = np.sqrt(1.0 - R[0, 0] + R[1, 1] - R[2, 2])
        q = [(R[0, 2] - R[2, 0]) * 0.5 / r, (R[0, 1] + R[1, 0]) * 0.5 / r, 0.5 * r, (R[1, 2] + R[2, 1]) * 0.5 / r]
    else:
        r = np.sqrt(1.0 - R[0, 0] - R[1, 1] + R[2, 2])
        q = [(R[1, 0] - R[0, 1]) * 0.5 / r, (R[0, 2] + R[2, 0]) * 0.5 / r, (R[1, 2] + R[2, 1]) * 0.5 / r, 0.5 * r]
    q = np.asarray(q, dtype=np.float64)
    return q / np.linalg.norm(q)


def set_anchors(self, anchors):
    """Labels every row with the id of the keyframe it belongs to: an int (all rows) or an integer tensor [P] (-1 = none).
    `model._anchor` (int32 [P] where the parameters live) is then kept through add_from_rgbd / create_from_pcd (`anchor=`),
    densify_and_prune (children inherit), prune_points and checkpoints; None (the default) costs nothing anywhere."""
    P, dev = int(self._xyz.shape[0]), self._xyz.device
    if isinstance(anchors, torch.Tensor):
        if anchors.is_floating_point() or tuple(anchors.shape) != (P,):
            raise ValueError(f"set_anchors: expected an integer tensor of shape ({P},), got {anchors.dtype} {tuple(anchors.shape)}")
        self._anchor = anchors.detach().to(device=dev, dtype=torch.int32).contiguous().clone()
    else:
        self._anchor = torch.full((P,), int(anchors), dtype=torch.int32, device=dev)
    return self


def extend_anchors(model, old_rows, new_rows, anchor, device):
    """Bookkeeping of a row insertion: `new_rows` rows appended behind `old_rows`.  With `anchor` they get it (and a model
    without anchors so far labels its old rows -1); without, they get -1 if the model has anchors and nothing happens otherwise."""
    cur = getattr(model, "_anchor", None)
    if anchor is None and cur is None:
        return
    if cur is None:
        cur = torch.full((old_rows,), -1, dtype=torch.int32, device=device)
    new = torch.full((new_rows,), -1 if anchor is None else int(anchor), dtype=torch.int32, device=device)
    model._anchor = torch.cat([cur.to(device), new])


def _transform_index(anchor, ids):
    """int32 [P]: the position in `ids` of every row's anchor, -1 where it is not among them (index bookkeeping on [P] integers;
    `ids` that already are 0 .. K-1 need none: the anchors are the indices)."""
    K = len(ids)
    if list(ids) == list(range(K)):
        return anchor
    ids_t = torch.tensor(list(ids), dtype=torch.int32, device=anchor.device)
    order = torch.argsort(ids_t)
    sorted_ids = ids_t[order]
    pos = torch.searchsorted(sorted_ids, anchor).clamp_(max=K - 1)
    hit = sorted_ids[pos] == anchor
    return torch.where(hit, order[pos].to(torch.int32), torch.full_like(anchor, -1)).contiguous()


def transform_(self, T, ids=None, moments="reset", check=None, allow_scale=False, count=True):
    """Moves rows of the model by x' = s R x + t, in place; returns how many rows moved (one read-back; `count=False`: None).

    T: [4,4] or [K,4,4] float64 [[s R, t], [0, 1]], on the host (validated: bottom row, |R R^T - I|, det > 0, and s == 1 unless
    `allow_scale=True`; ValueError otherwise) or on the device (trusted; `check=True` validates it at the price of one read-back,
    `check=False` skips the validation of a host matrix too).
    ids: None - K must be 1 and every row moves; or K keyframe ids - a row moves by T[k] when model._anchor[row] == ids[k], every
    other row stays bit for bit.
    moments: "reset" zeroes the moved rows' Adam moments of xyz, rotation, scaling and f_rest (they describe gradients in the
    old frame; f_dc and opacity are invariant and keep theirs), as reset_opacity does for its group; "keep" leaves them.
    The model's resize hooks are called around the move, so a Trainer in flight settles first and relearns its tile cut-offs
    (under exchange="sharded" its hook raises, as for prune_points).  Runs in HIP kernels: a CPU model raises GsrError."""
    _C = A.gsr()
    if moments not in ("reset", "keep"):
        raise ValueError(f"moments={moments!r}: expected 'reset' or 'keep'")
    T, on_host = _as_stack(T)
    K = int(T.shape[0])
    if (check is None and on_host) or check:
        validate_transforms(T.cpu().numpy(), allow_scale=allow_scale)
    if ids is None:
        if K != 1:
            raise ValueError(f"transform_: {K} transforms without `ids`: which rows move by which?")
    else:
        ids = [int(i) for i in ids]
        if len(ids) != K:
            raise ValueError(f"transform_: {K} transforms for {len(ids)} ids")
        if len(set(ids)) != K:
            raise ValueError("transform_: duplicate ids")
        if getattr(self, "_anchor", None) is None:
            raise ValueError("transform_: `ids` given but the model has no anchors (set_anchors, add_from_rgbd(anchor=...))")
    if self._xyz is None or not self._xyz.is_cuda:
        raise _C.GsrError("transform_ runs in HIP kernels (no CPU path): the model must live on the HIP device")
    dev = self._xyz.device
    P = int(self._xyz.shape[0])
    if P == 0 or K == 0:
        return 0 if count else None
    rest = int(self._features_rest.shape[1])
    if rest not in (0, 3, 8, 15):
        raise ValueError(f"transform_: features_rest holds {rest} coefficients; SH degrees 0..3 can be rotated")
    if ids is not None and int(self._anchor.shape[0]) != P:
        raise ValueError(f"transform_: model._anchor has {int(self._anchor.shape[0])} entries for {P} rows")
    with torch.no_grad():
        for hook in getattr(self, "_resize_hooks", ()):
            hook("before")
        index = None
        if ids is not None:
            index = _transform_index(self._anchor.to(device=dev, dtype=torch.int32).contiguous(), ids)
        params = [getattr(self, a).data for a in _MOVED_GROUPS]
        mom = [None] * 8
        opt = getattr(self, "optimizer", None)
        if moments == "reset" and opt is not None:
            for g, a in enumerate(_MOVED_GROUPS):
                st = opt.state.get(getattr(self, a), None)
                if st and "exp_avg" in st:
                    mom[2 * g], mom[2 * g + 1] = st["exp_avg"], st["exp_avg_sq"]
        for t in params + [m for m in mom if m is not None]:
            if not t.is_contiguous() or t.dtype != torch.float32 or t.device != dev:
                raise _C.GsrError("transform_: parameters and moments must be contiguous float32 tensors on the model's device")
        Td = T.to(dev).contiguous()
        lib = _C.lib()
        mom8 = (C.c_void_p * 8)(*[None if (m is None or m.numel() == 0) else m.data_ptr() for m in mom])
        with _C.on_device(dev):
            ws = torch.empty(lib.gsr_transform_workspace_bytes(K), dtype=torch.uint8, device=dev)
            _C.check(lib.gsr_transform_gaussians(P, _C.ptr(index), K, _C.ptr(Td), _C.ptr(ws), ws.numel(), _C.ptr(params[0]),
                                                 _C.ptr(params[1]), _C.ptr(params[2]), _C.ptr(params[3]) if rest else None, rest,
                                                 mom8, _C._stream()))
        for hook in getattr(self, "_resize_hooks", ()):
            hook("after")
        if not count:
            return None
        return P if index is None else int(((index >= 0) & (index < K)).sum().item())


def transform_camera(cam, T) -> MiniCam:
    """The camera that sees the map moved by T (x' = s R x + t) as `cam` saw the old one: R_c' = R_c R^T, centre c' = s R c + t.
    The world-to-camera matrix stays rigid, so a point's view-space coordinates - its depth too - come out s times the old ones
    and its pixel is the same.  Intrinsics (the principal point too), image size, znear / zfar and the construction of
    full_proj_transform are those of scene_utils.cameras.camera_from_RT.  Computed in float64 on the host; the result has `cam`'s dtype and device."""
    if isinstance(T, torch.Tensor):
        T = T.detach().cpu().numpy()
    s, R, t = decompose(np.asarray(T, dtype=np.float64).reshape(4, 4))
    wv = cam.world_view_transform
    w2c = wv.detach().cpu().double().numpy().T
    Rc, tc = w2c[:3, :3], w2c[:3, 3]
    c = -Rc.T @ tc
    Rc2 = Rc @ R.T
    c2 = s * (R @ c) + t
    new = np.eye(4)
    new[:3, :3], new[:3, 3] = Rc2, -Rc2 @ c2
    wv2 = torch.tensor(new, dtype=torch.float64).to(wv.dtype).transpose(0, 1)
    proj = camera_projection(cam).to(wv.dtype).transpose(0, 1)
    full = wv2.unsqueeze(0).bmm(proj.unsqueeze(0)).squeeze(0)
    out = MiniCam(cam.image_width, cam.image_height, cam.FoVy, cam.FoVx, cam.znear, cam.zfar, wv2.to(wv.device),
                  full.to(wv.device), cam.image_name, ox=float(getattr(cam, "ox", 0.0)), oy=float(getattr(cam, "oy", 0.0)))
    if hasattr(cam, "fx"):
        out.fx, out.fy, out.cx, out.cy = cam.fx, cam.fy, cam.cx, cam.cy
    return out


def correct_keyframes(model, cams, corrections, **kw):
    """The loop-closure call.  cams: {keyframe id: camera}; corrections: {keyframe id: T [4,4]} for the keyframes that moved.
    One transform_ moves the Gaussians anchored to every corrected keyframe by its correction (keywords go to transform_);
    -> {id: camera} with the corrected cameras (cameras without a correction are returned as they are)."""
    ids = list(corrections)
    if ids:
        mats = [corrections[i] for i in ids]
        if all(isinstance(m, torch.Tensor) and m.is_cuda for m in mats):
            T = torch.stack([m.double() for m in mats])
        else:
            T = torch.as_tensor(np.stack([m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else np.asarray(m)
                                          for m in mats]).astype(np.float64))
        model.transform_(T, ids=ids, **kw)
    return {i: (transform_camera(cam, corrections[i]) if i in corrections else cam) for i, cam in cams.items()}


GaussianModel.transform_ = transform_
GaussianModel.set_anchors = set_anchors
