"""One frame through the C ABI with everything the replay tests read back (tests/test_compositing_replay_gpu.py,
tests/test_projection_replay_gpu.py): gsr_forward_async_ex on fresh states, the debug views of the geometry, binning and image
states, gsr_backward / gsr_backward_ex with a scratch buffer made here (its first 48 R bytes are the gradient records by slot)."""
import contextlib
import ctypes as C
import math
import os

import numpy as np
import torch

import compositing_reference as CR

DEV = "cuda"
CAP = 1 << 20


@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


class _Scene:
    """Settings and Gaussians of one case as the C ABI takes them (the tensors are kept alive here).  _Scene(name): a case of
    compositing_reference in the activated `shs` call form.  _Scene.of(...): any call form (tests/projection_reference.case_inputs)."""

    def __init__(self, name):
        from helpers import leaf_inputs
        raw, cam, deg, W, H, bg = CR.case_scene(name)
        inp = leaf_inputs(raw, torch.float32, DEV, "sh")
        t = {k: v.detach().contiguous() for k, v in inp.items()}
        self._setup(W, H, bg, cam, deg, dict(means3D=t["means3D"], dc=None, shs=t["shs"], colors=None, opacities=t["opacities"],
                                             scales=t["scales"], rotations=t["rotations"], cov3D=None))
        self.t = t

    @classmethod
    def of(cls, W, H, bg, cam, deg, tensors, raw=False, scale_modifier=1.0, antialiasing=False):
        self = cls.__new__(cls)
        self._setup(W, H, bg, cam, deg, {k: (None if v is None else v.to(DEV).contiguous()) for k, v in tensors.items()}, raw,
                    scale_modifier, antialiasing)
        return self

    def _setup(self, W, H, bg, cam, deg, x, raw=False, scale_modifier=1.0, antialiasing=False):
        from diff_gaussian_rasterization import GaussianRasterizationSettings, _settings_struct, _gauss_struct
        self.W, self.H, self.bg = W, H, np.asarray(bg, dtype=np.float32)
        self.x = x
        self.t = x
        self.P = int(x["means3D"].shape[0])
        rs = GaussianRasterizationSettings(H, W, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), torch.from_numpy(self.bg).to(DEV),
                                           float(scale_modifier), cam.world_view_transform.to(DEV), cam.full_proj_transform.to(DEV), deg,
                                           cam.camera_center.to(DEV), False, False, bool(antialiasing))
        self.s, self.keep = _settings_struct(rs, DEV)
        self.g = _gauss_struct(self.P, x["means3D"], x["dc"], x["shs"], x["colors"], x["opacities"], x["scales"], x["rotations"],
                               x["cov3D"], raw)


class _FrameRun:
    """One forward (for_backward = 1) on fresh states; the states stay alive for the backward calls."""

    def __init__(self, sc, tlo=1, depth_z=False, defer_color=0, allow_empty=False):
        from diff_gaussian_rasterization import _C, _stream
        from helpers import _view
        lib = _C.lib()
        P, W, H = sc.P, sc.W, sc.H
        self.sc, self.depth_kind = sc, 1 if depth_z else 0
        self.geom = torch.zeros(max(4096, lib.gsr_geometry_state_bytes(P)), dtype=torch.uint8, device=DEV)
        self.img = torch.zeros(lib.gsr_image_state_bytes(W, H), dtype=torch.uint8, device=DEV)
        self.binning = torch.zeros(lib.gsr_binning_state_bytes(P, W, H, CAP), dtype=torch.uint8, device=DEV)
        self.radii = torch.zeros(max(P, 1), dtype=torch.int32, device=DEV)
        self.color = torch.full((3, H, W), 12345.0, device=DEV)
        self.invd = torch.full((1, H, W), 12345.0, device=DEV)
        self.alpha = torch.full((H, W), 12345.0, device=DEV)
        status = torch.zeros(8, dtype=torch.int64).pin_memory()
        ex = _C.gsr_render_extras(self.depth_kind, self.alpha.data_ptr(), None)
        _C.check(lib.gsr_forward_async_ex(C.byref(sc.s), C.byref(sc.g), _C.ptr(self.geom), self.geom.numel(), _C.ptr(self.radii),
                                          _C.ptr(self.binning), self.binning.numel(), CAP, _C.ptr(self.img), self.img.numel(),
                                          _C.ptr(self.color), _C.ptr(self.invd), 1, int(defer_color), None,
                                          C.c_void_p(status.data_ptr()), tlo, _stream(), None, C.byref(ex)))
        torch.cuda.synchronize()
        self.R = int(status[1])
        assert (0 <= self.R if allow_empty else 0 < self.R) and self.R <= CAP and int(status[0]) & 1 == 0
        tiles = math.prod(CR.R.tile_grid(W, H))
        pi = [C.c_void_p() for _ in range(2)]
        lib.gsr_debug_image_views(_C.ptr(self.img), W, H, C.byref(pi[0]), C.byref(pi[1]))
        pv = [C.c_void_p() for _ in range(7)]
        lib.gsr_debug_geometry_views(_C.ptr(self.geom), P, *[C.byref(p) for p in pv])
        pb = [C.c_void_p() for _ in range(3)]
        lib.gsr_debug_binning_views(_C.ptr(self.binning), W, H, CAP, C.byref(pb[0]), C.byref(pb[1]))
        lib.gsr_debug_slot_views(_C.ptr(self.binning), W, H, CAP, C.byref(pb[2]))
        self.out = dict(color=self.color.cpu().numpy().reshape(3, -1), depth=self.invd.cpu().numpy().reshape(-1),
                        alpha=self.alpha.cpu().numpy().reshape(-1),
                        fT=_view(self.img, pi[0].value, W * H, torch.float32).numpy(),
                        nc=_view(self.img, pi[1].value, W * H, torch.int32).numpy().astype(np.int64))
        self.rec = _view(self.geom, pv[0].value, P * 12, torch.float32).view(P, 12).numpy()
        # (tile-local binning has no depth sort: the keys are still per Gaussian, in index order)
        self.depth_key = _view(self.geom, pv[1].value, P, torch.int32).numpy().view(np.uint32)
        self.tiles_touched = _view(self.geom, pv[3].value, P, torch.int32).numpy().view(np.uint32).astype(np.int64)
        self.rect = _view(self.geom, pv[4].value, P * 4, torch.int16).numpy().view(np.uint16).astype(np.int64).reshape(P, 4)
        self.clamped = _view(self.geom, pv[6].value, P, torch.uint8).numpy()
        self.radii_host = self.radii[:P].cpu().numpy().astype(np.int64)
        self.point_list = _view(self.binning, pb[0].value, self.R, torch.int32).numpy().view(np.uint32)
        self.ranges = _view(self.binning, pb[1].value, tiles * 2, torch.int32).numpy().view(np.uint32).reshape(tiles, 2)
        self.slot = _view(self.binning, pb[2].value, self.R, torch.int32).numpy().view(np.uint32).astype(np.int64)
        self.frame = CR.Frame(self.rec, self.ranges, self.point_list, sc.bg, W, H)
        # the lists are contiguous, in tile order, from position 0: list order = position order
        lens = self.frame.ranges[:, 1] - self.frame.ranges[:, 0]
        assert int(lens.sum()) == self.R
        assert np.array_equal(self.frame.ranges[lens > 0, 0], (np.cumsum(lens) - lens)[lens > 0])
        # the slots are a permutation, and the slots of one Gaussian are contiguous (k_preprocess_bwd streams them)
        assert np.array_equal(np.sort(self.slot), np.arange(self.R))
        gid_of_slot = np.empty(self.R, dtype=np.int64)
        gid_of_slot[self.slot] = self.point_list
        self.gid_of_slot = gid_of_slot
        real = gid_of_slot[gid_of_slot != CR.NO_ID]
        assert len(np.unique(real)) == (1 + int((np.diff(real) != 0).sum()) if len(real) else 0)

    def backward(self, extras, depth_only=False):
        """gsr_backward (extras: gsr_backward_ex with dL/d(depth plane) and dL/d(alpha plane); depth_only: dL/d(depth plane) alone)
        with a scratch buffer made here, pre-filled with a pattern.
        -> (records [R, 12] float32 by SLOT, validity flags [R] uint8, dL_dmeans2D [P, 3], {gradient name: array})"""
        from diff_gaussian_rasterization import _C, _stream
        lib = _C.lib()
        sc = self.sc
        P, W, H = sc.P, sc.W, sc.H
        gp, gd, gA = (torch.from_numpy(x).to(DEV) for x in CR.upstream(W, H))
        nbytes = lib.gsr_backward_scratch_bytes(P, CAP)
        assert nbytes >= 48 * CAP + CAP
        scratch = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=DEV)
        x = sc.x
        shapes = dict(m3=(P, 3), m2=(P, 3), op=(P, 1))
        for k, src in (("dc", "dc"), ("sh", "shs"), ("col", "colors"), ("sc", "scales"), ("ro", "rotations"), ("cov", "cov3D")):
            if x[src] is not None:
                shapes[k] = tuple(x[src].shape)
        d = {k: torch.full(shape, 7.0, device=DEV) for k, shape in shapes.items()}
        gr = _C.gsr_grads(*[None if d.get(k) is None else d[k].data_ptr() for k in
                            ("m3", "m2", "dc", "sh", "col", "op", "sc", "ro", "cov")])
        with_depth = extras or depth_only
        args = (C.byref(sc.s), C.byref(sc.g), _C.ptr(self.radii), _C.ptr(self.geom), _C.ptr(self.binning), _C.ptr(self.img), CAP,
                _C.ptr(gp), _C.ptr(gd) if with_depth else None, _C.ptr(scratch), scratch.numel(), C.byref(gr), _stream())
        if extras:
            ex = _C.gsr_render_extras(self.depth_kind, None, gA.data_ptr())
            _C.check(lib.gsr_backward_ex(*args, C.byref(ex)))
        elif self.depth_kind:
            ex = _C.gsr_render_extras(self.depth_kind, None, None)
            _C.check(lib.gsr_backward_ex(*args, C.byref(ex)))
        else:
            _C.check(lib.gsr_backward(*args))
        torch.cuda.synchronize()
        recs = scratch[:48 * self.R].clone().view(torch.float32).view(self.R, 12).cpu().numpy()
        flags = scratch[48 * CAP:48 * CAP + self.R].cpu().numpy()
        return recs, flags, d["m2"].cpu().numpy(), {k: v.cpu().numpy() for k, v in d.items()}
