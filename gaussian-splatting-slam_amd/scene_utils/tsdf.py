"""TSDF fusion: depth frames into a block-sparse truncated signed distance volume on the HIP device, out as an oriented cloud and
a triangle mesh (csrc/tsdf.hip; the volume is defined in include/gsr.h).  Per pixel and per voxel work
is four HIP kernels - touch, integrate, extract points, extract triangles; what torch does here is plumbing on the device: unique
and merge of the int64 block keys, growing the row storage, welding the triangle soup.  There is no CPU path."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _args as A
from .cameras import camera_intrinsics

BLOCK = 8
BLOCK_VOXELS = 512
_BIAS = 1 << 20


def block_keys(coords):
    """int64 keys of integer block coordinates [...,3] (x highest, 21 bits per axis after the bias 2^20)."""
    c = coords.to(torch.int64) + _BIAS
    return (c[..., 0] << 42) | (c[..., 1] << 21) | c[..., 2]


def key_coords(keys):
    """the inverse of block_keys: int64 [B] -> int64 [B,3]"""
    m = (1 << 21) - 1
    return torch.stack(((keys >> 42) & m, (keys >> 21) & m, keys & m), dim=-1) - _BIAS


def _w2c64(camera, w2c):
    """the world-to-camera matrix as float64 numpy [4,4]: `w2c` when given (a pose kept in float64), else the camera's float32
    world_view_transform (stored transposed)"""
    if w2c is not None:
        T = A.transform(w2c, "w2c")
        return np.asarray(T.detach().cpu().numpy(), dtype=np.float64)
    return np.asarray(camera.world_view_transform.detach().cpu().numpy(), dtype=np.float64).T.copy()


class TSDFVolume:
    """A block-sparse TSDF volume.  `voxel_size` <= `sdf_trunc` <= 8 `voxel_size`; readings beyond `depth_trunc` are ignored;
    `origin` is the world position of the corner of voxel (0, 0, 0) (float64: choose it near the scene when the world frame is far
    from it); `max_weight` caps a voxel's weight (None: no cap).  Storage: `tsdf`, `weight` [B,512], `color` [B,512,3] in allocation
    order, append-only; `keys_sorted` [B] int64 ascending with `row_of_sorted` [B] int32."""

    def __init__(self, voxel_size, sdf_trunc, depth_trunc=10.0, origin=(0.0, 0.0, 0.0), max_weight=None, device="cuda"):
        self.voxel_size = A.voxel_size(voxel_size)
        self.sdf_trunc = A.number("sdf_trunc", sdf_trunc, lambda v: self.voxel_size <= v <= 8 * self.voxel_size,
                                  "voxel_size .. 8 voxel_size")
        self.depth_trunc = A.number("depth_trunc", depth_trunc, lambda v: v > 0 and math.isfinite(v), "a finite value > 0")
        self.max_weight = None if max_weight is None else A.number("max_weight", max_weight, lambda v: v >= 1, "a value >= 1")
        o = np.asarray(origin, dtype=np.float64).reshape(-1)
        if o.shape != (3,) or not np.all(np.isfinite(o)):
            raise ValueError(f"origin={origin!r}: expected three finite numbers")
        self.origin = tuple(float(v) for v in o)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise A.gsr().GsrError("TSDFVolume lives on the HIP device (no CPU path)")
        self._count_guess = {"points": 0, "triangles": 0}
        self.reset()

    # ---- state -------------------------------------------------------------------------------------------------------------------
    def reset(self):
        dev = self.device
        self._rows = 0                 # rows in use; the tensors below may hold more (capacity grows by doubling)
        self._tsdf = torch.zeros((0, BLOCK_VOXELS), dtype=torch.float32, device=dev)
        self._weight = torch.zeros((0, BLOCK_VOXELS), dtype=torch.float32, device=dev)
        self._color = torch.zeros((0, BLOCK_VOXELS, 3), dtype=torch.float32, device=dev)
        self.keys_sorted = torch.zeros((0,), dtype=torch.int64, device=dev)
        self.row_of_sorted = torch.zeros((0,), dtype=torch.int32, device=dev)

    @property
    def num_blocks(self):
        return self._rows

    @property
    def tsdf(self):
        return self._tsdf[:self._rows]

    @property
    def weight(self):
        return self._weight[:self._rows]

    @property
    def color(self):
        return self._color[:self._rows]

    def block_coords(self):
        """int64 [B,3]: the block coordinates, in key order (row i of the storage: block_coords()[argsort(row_of_sorted)][i])."""
        return key_coords(self.keys_sorted)

    def load(self, keys, tsdf, weight, color):
        """Replaces the content: `keys` int64 [B] (any order, distinct) with rows tsdf / weight [B,512], color [B,512,3] in the same
        order - a volume computed elsewhere, or saved earlier."""
        dev = self.device
        keys = torch.as_tensor(keys, dtype=torch.int64).to(dev).reshape(-1)
        B = int(keys.shape[0])
        if B > A.gsr().TSDF_MAX_BLOCKS or int(torch.unique(keys).shape[0]) != B:
            raise ValueError(f"load: {B} keys: expected at most {A.gsr().TSDF_MAX_BLOCKS} distinct ones")
        self.reset()
        self._tsdf = torch.as_tensor(tsdf, dtype=torch.float32).to(dev).reshape(B, BLOCK_VOXELS).contiguous().clone()
        self._weight = torch.as_tensor(weight, dtype=torch.float32).to(dev).reshape(B, BLOCK_VOXELS).contiguous().clone()
        self._color = torch.as_tensor(color, dtype=torch.float32).to(dev).reshape(B, BLOCK_VOXELS, 3).contiguous().clone()
        self._rows = B
        self.keys_sorted, order = torch.sort(keys)
        self.row_of_sorted = order.to(torch.int32)

    def _vol(self):
        _C = A.gsr()
        mw = 3.0e38 if self.max_weight is None else self.max_weight
        return _C.gsr_tsdf_volume((C.c_double * 3)(*self.origin), self.voxel_size, self.sdf_trunc, self.depth_trunc, mw, 0.0)

    def _grow(self, rows):
        cap = int(self._tsdf.shape[0])
        if rows <= cap:
            return
        new_cap = max(rows, 2 * cap, 64)
        for name in ("_tsdf", "_weight", "_color"):
            old = getattr(self, name)
            t = torch.zeros((new_cap,) + tuple(old.shape[1:]), dtype=torch.float32, device=self.device)
            t[:self._rows] = old[:self._rows]
            setattr(self, name, t)

    # ---- integration -------------------------------------------------------------------------------------------------------------
    def touch(self, depth, camera, mask=None, w2c=None):
        """The sorted unique keys of the blocks the frame touches (int64 [n]); allocates nothing."""
        fr, keep = self._frame(None, depth, camera, mask, w2c)
        return self._touch(fr, keep)

    def _touch(self, fr, keep):
        _C = A.gsr()
        n = fr.width * fr.height
        cand = torch.empty((_C.TSDF_TOUCH_SLOTS, n), dtype=torch.int64, device=self.device)
        with _C.on_device(self.device):
            _C.check(_C.lib().gsr_tsdf_touch(C.byref(self._vol()), C.byref(fr), _C.ptr(cand), _C._stream()))
        keys = torch.unique(cand)
        return keys[keys != _C.TSDF_NO_KEY]

    def _frame(self, image, depth, camera, mask, w2c):
        _C = A.gsr()
        for name, t in (("image", image), ("depth", depth), ("mask", mask)):
            if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda):
                raise _C.GsrError(f"TSDFVolume: {name} must live on the HIP device (no CPU path)")
        if depth is None:
            raise ValueError("TSDFVolume: the frame has no depth")
        W, H = int(camera.image_width), int(camera.image_height)
        A.tensor(depth, "depth", (H, W), also=(1, H, W))
        d = depth.detach().float().contiguous()
        m = None
        if mask is not None:
            if not isinstance(mask, torch.Tensor) or mask.numel() != H * W:
                raise ValueError(f"mask: expected {H} x {W} values")
            m = mask.detach().float().contiguous()
        img = None
        if image is not None:
            A.tensor(image, "image", (3, H, W))
            img = image.detach().float().contiguous()
        T = _w2c64(camera, w2c)
        K = [float(np.float32(v)) for v in camera_intrinsics(camera)]
        fr = _C.gsr_tsdf_frame(W, H, (C.c_float * 4)(*K), (C.c_double * 12)(*[float(v) for v in T[:3].reshape(-1)]),
                               d.data_ptr(), None if m is None else m.data_ptr(), None if img is None else img.data_ptr())
        return fr, (d, m, img)

    def integrate(self, frame_or_image, depth=None, camera=None, mask=None, w2c=None):
        """integrate(frame) with a `Frame` (image, depth, mask, camera), or integrate(image, depth, camera, mask=None); `image`
        [3,H,W] or None (colours then stay as they are), `depth` [H,W] view-space z, `mask` [H,W] (0 = ignore the pixel).  `w2c`: the
        pose as a float64 [4,4] world-to-camera matrix where the camera's float32 one is too coarse (a world frame kilometres from
        its origin).  Returns the number of blocks the frame touched."""
        if hasattr(frame_or_image, "camera") and depth is None and camera is None:
            f = frame_or_image
            image, depth, mask, camera = f.image, f.depth, (f.mask if mask is None else mask), f.camera
        else:
            image = frame_or_image
        if camera is None:
            raise ValueError("TSDFVolume.integrate: no camera")
        _C = A.gsr()
        fr, keep = self._frame(image, depth, camera, mask, w2c)
        touched = self._touch(fr, keep)
        n = int(touched.shape[0])
        if n == 0:
            return 0
        # merge: which touched keys are new, rows for them, one sort of the union
        pos = torch.searchsorted(self.keys_sorted, touched)
        known = torch.zeros(n, dtype=torch.bool, device=self.device)
        if self._rows:
            inside = pos < self._rows
            known[inside] = self.keys_sorted[pos[inside]] == touched[inside]
        new_keys = touched[~known]
        n_new = int(new_keys.shape[0])
        if self._rows + n_new > _C.TSDF_MAX_BLOCKS:
            raise _C.GsrError(f"TSDFVolume: {self._rows + n_new} blocks exceed the limit of {_C.TSDF_MAX_BLOCKS}")
        if n_new:
            self._grow(self._rows + n_new)
            new_rows = torch.arange(self._rows, self._rows + n_new, dtype=torch.int32, device=self.device)
            keys = torch.cat((self.keys_sorted, new_keys))
            rows = torch.cat((self.row_of_sorted, new_rows))
            self.keys_sorted, order = torch.sort(keys)
            self.row_of_sorted = rows[order].contiguous()
            self._rows += n_new
        rows_touched = self.row_of_sorted[torch.searchsorted(self.keys_sorted, touched)].contiguous()
        with _C.on_device(self.device):
            _C.check(_C.lib().gsr_tsdf_integrate(C.byref(self._vol()), C.byref(fr), n, _C.ptr(touched), _C.ptr(rows_touched),
                                                 self._rows, _C.ptr(self._tsdf), _C.ptr(self._weight), _C.ptr(self._color),
                                                 _C._stream()))
        return n

    # ---- extraction --------------------------------------------------------------------------------------------------------------
    def _extract(self, kind, min_weight, widths):
        """The verified-capacity idiom: outputs sized from the last count of this kind (a count-only call the first time), the
        call reports the count it needed, one repeat when that exceeds the capacity."""
        _C = A.gsr()
        min_weight = A.number("min_weight", min_weight, lambda v: v >= 0, "a value >= 0")
        dev, B = self.device, self._rows
        l = _C.lib()
        fn = l.gsr_tsdf_extract_points if kind == "points" else l.gsr_tsdf_extract_triangles
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        ws = torch.empty(l.gsr_tsdf_extract_workspace_bytes(B), dtype=torch.uint8, device=dev)
        vol = self._vol()

        def call(cap, outs):
            with _C.on_device(dev):
                _C.check(fn(C.byref(vol), B, _C.ptr(self.keys_sorted), _C.ptr(self.row_of_sorted), _C.ptr(self._tsdf),
                            _C.ptr(self._weight), _C.ptr(self._color), min_weight, cap, *[_C.ptr(o) for o in outs], _C.ptr(count),
                            _C.ptr(ws), ws.numel(), _C._stream()))
            return int(count.item())
        cap = self._count_guess[kind]
        if cap == 0:
            cap = call(0, [None] * len(widths))
        while True:
            outs = [torch.empty((cap,) + w, dtype=torch.float32, device=dev) for w in widths]
            need = call(cap, outs) if cap else call(0, [None] * len(widths))
            if need <= cap:
                break
            cap = need
        self._count_guess[kind] = need
        return [o[:need] for o in outs]

    def extract_point_cloud(self, min_weight=0):
        """-> (points [N,3], normals [N,3], colors [N,3]): one point per sign-change edge between observed voxels (weight >
        min_weight), normals toward positive tsdf; blocks in key order, voxels in linear order, axes x, y, z."""
        return tuple(self._extract("points", min_weight, [(3,), (3,), (3,)]))

    def extract_triangle_mesh(self, min_weight=0, weld=True):
        """Marching tetrahedra.  weld=True -> (vertices [V,3], triangles [T,3] int64, colors [V,3]): vertices with the same bits are
        one, triangles with two equal indices are dropped; weld=False -> the soup (positions [T,3,3], None, colors [T,3,3])."""
        pos, col = self._extract("triangles", min_weight, [(3, 3), (3, 3)])
        if not weld:
            return pos, None, col
        return weld_triangles(pos, col)


def weld_triangles(positions, colors):
    """Triangle soup [T,3,3] -> (vertices, triangles, colors): exact-bits unique of the vertices, degenerate triangles dropped.
    The colour of a vertex is that of its first occurrence in the soup (equal positions carry equal colours: both are functions
    of the same edge)."""
    T = int(positions.shape[0])
    dev = positions.device
    if T == 0:
        return (torch.zeros((0, 3), dtype=torch.float32, device=dev), torch.zeros((0, 3), dtype=torch.int64, device=dev),
                torch.zeros((0, 3), dtype=torch.float32, device=dev))
    flat = positions.reshape(-1, 3)
    bits = flat.contiguous().view(torch.int32)           # (-0.0 and 0.0 stay apart: exact bits)
    uniq, inverse = torch.unique(bits, dim=0, return_inverse=True)
    V = int(uniq.shape[0])
    first = torch.full((V,), flat.shape[0], dtype=torch.int64, device=dev)
    first.scatter_reduce_(0, inverse, torch.arange(flat.shape[0], device=dev), reduce="amin")
    tri = inverse.reshape(T, 3)
    keep = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])
    return uniq.view(torch.float32), tri[keep].contiguous(), colors.reshape(-1, 3)[first]


def fuse_views(model, cameras, pipe, bg, volume, alpha_min=0.5):
    """From map to mesh: every camera renders the model (colour, z-depth, accumulated opacity) and the result is integrated into
    `volume`.  The mask is alpha > alpha_min; the z channel is the opacity-weighted sum of depths, so the metric depth of a pixel
    is that sum over alpha.  Returns the volume."""
    from gaussian_renderer import render
    alpha_min = A.number("alpha_min", alpha_min, lambda v: 0 <= v < 1, "a value in [0, 1)")
    with torch.no_grad():
        for cam in cameras:
            pkg = render(cam, model, pipe, bg, depth="z", alpha=True)
            alpha = pkg["alpha"].reshape(cam.image_height, cam.image_width)
            mask = (alpha > alpha_min).float()
            depth = pkg["depth"].reshape(cam.image_height, cam.image_width) / alpha.clamp_min(1e-6) * mask
            volume.integrate(pkg["render"].clamp(0.0, 1.0), depth, cam, mask=mask)
    return volume


__all__ = ["TSDFVolume", "fuse_views", "weld_triangles", "block_keys", "key_coords"]
