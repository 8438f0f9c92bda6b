"""Every exported forward and backward entry point of the rasterizer and every host-side route behind them, bit for bit what the
commit before the host path of csrc/api.hip was rebuilt around one frame view and two call records computed.

tests/golden/frame_paths_parent.npz was recorded on the MI355X from a build of that commit by `cases()` below (each case run twice
and kept only because both runs agreed): every output as raw 32-bit words, and a float64 checksum of every input array.  The
rasterizer is bitwise reproducible, so there is no tolerance, and no case is left out.  Scene and case table:
tests/frame_paths_cases.py.  Equal outputs are stored once: `pack` / `gold` are the fixture's format."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import frame_paths_cases as F
from diff_gaussian_rasterization import _C

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_paths_parent.npz")
DEV = "cuda"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def words(t):
    """raw bits of a tensor of 4-byte elements (or of a Python int as int64) as uint32"""
    if isinstance(t, int):
        return np.array([t], dtype=np.int64).view(np.uint32).copy()
    return t.detach().cpu().contiguous().numpy().view(np.uint32).ravel().copy()


def zeros(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype, device=DEV)


def stream():
    return C.c_void_p(_C.raw_stream())


def call(name, variant, *args, extras=None):
    """entry point `name`, or its _ex twin with `extras` (variant "ex") or NULL (variant "exnull") as the last argument"""
    lib = _C.lib()
    if variant == "plain":
        return _C.check(getattr(lib, name)(*args))
    return _C.check(getattr(lib, name + "_ex")(*args, C.byref(extras) if variant == "ex" else None))


class Scene:
    """the device copies of one case's inputs and the two structs that point at them"""

    def __init__(self, P, camera="front", debug=0):
        self.P = P
        self.t = {k: dev(v) for k, v in F.scene().items()}
        self.cam = {k: dev(v) for k, v in F.camera(camera).items()}
        self.s = _C.gsr_settings(F.H, F.W, F.TANFOV, F.TANFOV, self.t["bg"].data_ptr(), 1.0, self.cam["viewmatrix"].data_ptr(),
                                 self.cam["projmatrix"].data_ptr(), F.SH_DEGREE, self.cam["campos"].data_ptr(), 0, debug, 0)
        self.g = self.gaussians(self.t)

    def gaussians(self, t):
        return _C.gsr_gaussians(self.P, F.SH_REST, t["means3D"].data_ptr(), t["dc"].data_ptr(), t["shs"].data_ptr(), None,
                                t["opacities"].data_ptr(), t["scales"].data_ptr(), t["rotations"].data_ptr(), None, 1)


def _forward(name):
    """one forward case -> (frame: what a backward needs, outputs {key: uint32 words})"""
    spec = F.FORWARD_CASES[name]
    lib, v, fb = _C.lib(), spec["variant"], spec["fb"]
    P = spec.get("P", F.P)
    sc = Scene(P, spec.get("camera", "front"), spec.get("debug", 0))
    s, g = C.byref(sc.s), C.byref(sc.g)
    rows = max(P, 1)
    geom = zeros(lib.gsr_geometry_state_bytes(P), dtype=torch.uint8)
    img = zeros(lib.gsr_image_state_bytes(F.W, F.H), dtype=torch.uint8)
    radii = zeros(rows, dtype=torch.int32)
    color, depth = zeros(3, F.H, F.W), zeros(1, F.H, F.W)
    alpha = zeros(F.H, F.W)
    touched = torch.full((rows,), -1, dtype=torch.int32, device=DEV)       # (the library owns the zeroing)
    ex = _C.gsr_render_extras(_C.DEPTH_KINDS["z"], alpha.data_ptr(), None, touched.data_ptr(), F.TOUCHED_T_MIN)
    out = {}

    def binning_for(cap):
        b = zeros(lib.gsr_binning_state_bytes(P, F.W, F.H, cap), dtype=torch.uint8)
        return b, _C.ptr(b), b.numel()

    def status_slot(kind):
        if kind == "null":
            return None, None
        st = torch.zeros(8, dtype=torch.int32)
        st = st.pin_memory() if kind == "pinned" else st
        return st, C.c_void_p(st.data_ptr())

    images = (_C.ptr(img), img.numel(), _C.ptr(color), _C.ptr(depth), fb)
    if spec["path"] == "blocking":
        prepare = "gsr_forward_prepare" if spec["shade"] == "fused" else "gsr_forward_prepare_geometry"
        R = call(prepare, v, s, g, _C.ptr(geom), geom.numel(), _C.ptr(radii), stream(), extras=ex)
        binning, bp, bn = binning_for(R)
        if spec["shade"] == "call":
            _C.check(lib.gsr_forward_shade(s, g, _C.ptr(geom), stream()))
        if spec["shade"] == "late":
            event = None
            if spec["event"]:
                event = torch.cuda.Event()
                event.record()
            call("gsr_forward_render_shade", v, s, g, _C.ptr(geom), bp, bn, R, *images,
                 C.c_void_p(event.cuda_event) if event is not None else None, stream(), extras=ex)
        else:
            call("gsr_forward_render", v, s, g, _C.ptr(geom), bp, bn, R, *images, stream(), extras=ex)
        out["count"] = words(int(R))
    else:
        tlo = spec.get("tlo", 1)
        status, sp = status_slot(spec.get("status", "pinned"))
        count = C.c_int64(-1)
        cp = C.byref(count) if spec.get("count", spec["path"] == "rerender") else None
        R = F.SMALL_CAPACITY if spec["path"] == "rerender" else F.CAPACITY
        binning, bp, bn = binning_for(R)
        head = (s, g, _C.ptr(geom), geom.numel(), _C.ptr(radii), bp, bn, R, *images, spec.get("defer", 0), None, sp, tlo)
        old = os.environ.get("GSR_SHADE_STREAM")
        os.environ["GSR_SHADE_STREAM"] = str(spec.get("aside", 0))          # (the library reads it per call)
        try:
            if spec["path"] == "culled":
                cutoff = torch.full((F.TILES,), -1, dtype=torch.int32, device=DEV)
                for apply in (0, 1):           # the second frame is cut by what the first one left
                    call("gsr_forward_async_culled", v, *head, stream(), cp, _C.ptr(cutoff), apply, extras=ex)
                    torch.cuda.synchronize()
                    out[f"cutoff_after_apply{apply}"] = words(cutoff)
                    out[f"color_after_apply{apply}"] = words(color)
                    out[f"status_after_apply{apply}"] = words(status)
            else:
                call("gsr_forward_async", v, *head, stream(), cp, extras=ex)
        finally:
            if old is None:
                del os.environ["GSR_SHADE_STREAM"]
            else:
                os.environ["GSR_SHADE_STREAM"] = old
        torch.cuda.synchronize()
        if cp is not None:
            out["count"] = words(count.value)
        if spec["path"] == "rerender":
            assert count.value > R                           # the frame was composited from a truncated list
            out["first_status"], out["first_radii"] = words(status), words(radii)
            R = count.value + 17
            binning, bp, bn = binning_for(R)
            call("gsr_forward_rerender", v, s, g, _C.ptr(geom), bp, bn, R, *images, tlo, sp, stream(), extras=ex)
        if status is not None:
            torch.cuda.synchronize()
            out["status"] = words(status)
    torch.cuda.synchronize()
    out.update(color=words(color), depth=words(depth), radii=words(radii))
    if v == "ex":
        out.update(alpha=words(alpha), n_touched=words(touched))
    return dict(scene=sc, geom=geom, binning=binning, img=img, radii=radii, R=int(R)), out


@functools.lru_cache(maxsize=None)
def frame(name):
    """the state a forward case leaves, for the backward cases that share it: none of them writes to it"""
    return _forward(name)[0]


def adam_struct(m, v, sparse):
    """-> gsr_fused_adam over the moment tensors of the six groups (None: no moments, gsr_adam_set_dynamic reads none)"""
    six = C.c_void_p * 6
    return _C.gsr_fused_adam(six(*[t.data_ptr() for t in m]) if m else six(), six(*[t.data_ptr() for t in v]) if v else six(),
                             (C.c_float * 6)(*F.ADAM_LR), (C.c_int64 * 6)(*F.ADAM_STEP), F.ADAM_BETA1, F.ADAM_BETA2, F.ADAM_EPS,
                             sparse, None)


def _backward(name):
    spec = F.BACKWARD_CASES[name]
    lib, v, form = _C.lib(), spec["variant"], spec["form"]
    fr = frame(spec["frame"])
    sc, P, R = fr["scene"], fr["scene"].P, fr["R"]
    rows = max(P, 1)
    t = {k: dev(a) for k, a in F.scene().items()}            # fresh copies: the folded forms update the parameters in place
    g = sc.gaussians(t)
    ex = _C.gsr_render_extras(_C.DEPTH_KINDS["z"], None, t["dL_dalpha"].data_ptr(), None, 0.0)
    gr = {k: zeros(rows, n) for k, n in (("dL_dmeans3D", 3), ("dL_dmeans2D", 3), ("dL_ddc", 3), ("dL_dshs", 3 * F.SH_REST),
                                         ("dL_dopacities", 1), ("dL_dscales", 3), ("dL_drotations", 4),
                                         ("xyz_gradient_accum", 1), ("denom", 1), ("max_radii2D", 1))}
    grads = _C.gsr_grads(*[gr[k].data_ptr() if k in gr else None for k, _ in _C.gsr_grads._fields_])
    scratch = zeros(lib.gsr_backward_scratch_bytes(P, R), dtype=torch.uint8)
    head = (C.byref(sc.s), C.byref(g), _C.ptr(fr["radii"]), _C.ptr(fr["geom"]), _C.ptr(fr["binning"]), _C.ptr(fr["img"]), R,
            _C.ptr(t["dL_dcolor"]), _C.ptr(t["dL_ddepth"]), _C.ptr(scratch), scratch.numel())
    cg = dict(dL_dviewmatrix=zeros(16), dL_dprojmatrix=zeros(16), dL_dcampos=zeros(3))
    cam_scratch = zeros(lib.gsr_camera_grad_scratch_bytes(P), dtype=torch.uint8)
    camera = (C.byref(_C.gsr_camera_grads(*[x.data_ptr() for x in cg.values()])), _C.ptr(cam_scratch), cam_scratch.numel())
    out = {}
    if form == "plain":
        call("gsr_backward", v, *head, C.byref(grads), stream(), extras=ex)
    elif form == "camera":
        call("gsr_backward_camera", v, *head, C.byref(grads), *camera, stream(), extras=ex)
    elif form == "camera_only":
        call("gsr_backward_camera_only", v, *head, *camera, stream(), extras=ex)
    else:
        sparse = int(form[len("adam_sparse")])
        m = [dev(F.scene()["m_" + k]) for k, _ in F.ADAM_GROUPS]
        vv = [dev(F.scene()["v_" + k]) for k, _ in F.ADAM_GROUPS]
        opt = adam_struct(m, vv, sparse)
        call("gsr_backward_adam", v, *head, C.byref(grads), C.byref(opt), stream(), extras=ex)
        if sparse == 2:
            _C.check(lib.gsr_adam_step_culled_rows(C.byref(g), _C.ptr(fr["geom"]), R, C.byref(opt), stream()))
        for i, (k, param) in enumerate(F.ADAM_GROUPS):
            out.update({"p_" + k: words(t[param]), "m_" + k: words(m[i]), "v_" + k: words(vv[i])})
    torch.cuda.synchronize()
    if form != "camera_only":
        out.update({k: words(x) for k, x in gr.items()})
    if form in ("camera", "camera_only"):
        out.update({k: words(x) for k, x in cg.items()})
    return out


def _dynamic(name):
    dyn = zeros(_C.ADAM_DYNAMIC_FLOATS)
    _C.check(_C.lib().gsr_adam_set_dynamic(C.byref(adam_struct(None, None, F.DYNAMIC_CASES[name])), _C.ptr(dyn), stream()))
    torch.cuda.synchronize()
    return {"dynamic": words(dyn)}


def run(name):
    """one case through the C ABI -> {key: uint32 words}"""
    if name in F.FORWARD_CASES:
        return _forward(name)[1]
    return _backward(name) if name in F.BACKWARD_CASES else _dynamic(name)


def cases():
    """{name: {key: words}} of every case: what the fixture holds"""
    return {name: run(name) for name in F.NAMES}


def pack(outputs, sums):
    """the fixture's arrays: keys "case/output", for each the index of its words among the distinct word arrays, those arrays end
    to end with their offsets, and the input checksums"""
    keys, which, blobs, seen = [], [], [], {}
    for name in F.NAMES:
        for k in sorted(outputs[name]):
            w = outputs[name][k]
            assert w.dtype == np.uint32 and w.ndim == 1
            keys.append(f"{name}/{k}")
            which.append(seen.setdefault(w.tobytes(), len(blobs)))
            if which[-1] == len(blobs):
                blobs.append(w)
    offsets = np.cumsum([0] + [len(b) for b in blobs]).astype(np.int64)
    return dict(keys=np.array(keys), which=np.array(which, dtype=np.int32), offsets=offsets, words=np.concatenate(blobs),
                sum_keys=np.array(sorted(sums)), sums=np.array([sums[k] for k in sorted(sums)], dtype=np.float64))


@functools.lru_cache(maxsize=None)
def gold():
    """-> ({name: {key: words}}, {key: checksum}) of the fixture"""
    g = np.load(GOLDEN)
    assert g["words"].dtype == np.uint32
    out = {}
    for key, i in zip(g["keys"], g["which"]):
        name, k = str(key).split("/")
        out.setdefault(name, {})[k] = g["words"][g["offsets"][i]:g["offsets"][i + 1]]
    return out, {str(k): float(v) for k, v in zip(g["sum_keys"], g["sums"])}


def test_the_inputs_are_the_recorded_ones():
    outputs, sums = gold()
    assert sums == F.input_checksums()
    assert sorted(outputs) == sorted(F.NAMES)


def test_the_scene_is_what_the_cases_need():
    out = gold()[0]["prepare_render_fb1_ex"]
    R = int(out["count"].view(np.int64)[0])
    radii = out["radii"].view(np.int32)
    assert F.SMALL_CAPACITY < R < F.CAPACITY
    assert (radii > 0).sum() >= 20 and (radii == 0).sum() >= 20             # some on screen, some behind or beside it
    assert out["n_touched"].any() and out["alpha"].view(np.float32).max() > 0.5
    culled = gold()[0]["culled_plain"]                                        # the cut-offs of the first frame shorten the second
    assert (culled["cutoff_after_apply0"] != 0xFFFFFFFF).any()
    assert 0 < culled["status_after_apply1"][2] < culled["status_after_apply0"][2] == R
    for name in ("sees_nothing_blocking_plain", "no_gaussians_blocking_plain"):
        assert int(gold()[0][name]["count"].view(np.int64)[0]) == 0


@pytest.mark.parametrize("name", F.NAMES)
def test_case_is_bit_for_bit_what_it_was(name):
    want, got = gold()[0][name], run(name)
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        assert got[k].dtype == np.uint32 and np.array_equal(got[k], want[k]), (name, k, got[k][:8], want[k][:8])
