"""The projection kernels (csrc/preprocess.hip: k_preprocess_fwd staged and unstaged, k_shade, k_preprocess_bwd) held to the float64
replay of tests/projection_reference.py ON THEIR OWN INPUTS, Gaussian by Gaussian: the float32 call arguments in, the 48-byte record,
radius, tile rectangle, tile count, depth key and clamp bits out; the kernel's own gradient records (caller-made scratch buffer of
gsr_backward, by slot) summed per Gaussian in float64 in, every gradient row out.
  A  forward: every continuous record value of every visible Gaussian within its bound; every discrete value inside the (lo, hi)
     pair of the reference (decided: exact; undecided: one of the two neighbours); invisible Gaussians have radius 0, tile count 0
     and depth key 0xFFFFFFFF; word 11 of the record carries the bits of the depth key; the tile count is zero exactly where the
     first-stage box or every row interval is empty.
  B  backward: every gradient row of every Gaussian with instances within its bound, with and without dL/d(depth plane); rows of
     Gaussians without instances are exact zeros.
  C  two runs give identical bits.
BOUNDS.  |kernel - float64 replay| / S <= max(2^-24, 4 x the float32 numpy replay's largest figure over all cases)
(projection_reference.YARDSTICK, measured on the CPU; tests/test_projection_reference_cpu.py recomputes it).  The factor covers a
different order of the same sums and the hardware's expf / logf; this file is compiled without contraction and without fast-math
(csrc/Makefile, `#pragma clang fp contract(off)`), so division and sqrt are correctly rounded as in numpy.  Nothing was measured
against the kernels; profiles/projection_replay.txt records their figures.
The folded-Adam, camera and camera-only instantiations of k_preprocess_bwd are not repeated here: tests/test_loss_adam_gpu.py,
tests/test_camera_grad_gpu.py and tests/test_camera_only_gpu.py hold them bit for bit to the gradients checked here."""
import functools

import numpy as np
import pytest
import torch

import compositing_reference as CR
import projection_reference as PR
from frame_run import _env, _FrameRun, _Scene

pytestmark = pytest.mark.gpu

BOUNDS = PR.bounds()
_UNSET = dict(GSR_BWD_FORM=None, GSR_BWD_LPT=None, GSR_BWD_MASK=None, GSR_BWD_REDUCE=None, GSR_BWD_PRIO=None, GSR_FWD_MASK=None,
              GSR_BINNING=None, GSR_SHADE_STREAM=None)
DEGS = PR.DEG_FORMS                                                       # active degree below the stored 3: the unstaged kernels
EDGE_FORMS = list(PR.FORMS) + list(DEGS)
FORWARD = ([(n, "base") for n in CR.CASES] + [("edge", f) for f in EDGE_FORMS] + [(f"tail_{n}", "base") for n in PR.TAIL_SIZES]
           + [("regular", f) for f in ("dc", "raw-aa-mod2.3", "cov-aa", "colors", "mod0.5", "raw-mod2.3", "z")]
           + [("needles", "raw-aa-mod2.3"), ("needles", "cov")])
BACKWARD = ([(n, "base") for n in CR.CASES] + [("edge", f) for f in EDGE_FORMS] + [(f"tail_{n}", "base") for n in PR.TAIL_SIZES]
            + [("regular", f) for f in ("dc", "raw-aa-mod2.3", "cov-aa", "colors", "mod0.5", "raw-mod2.3", "z")]
            + [("needles", "raw-aa-mod2.3"), ("needles", "cov")])
DEFERRED = [("edge", "base"), ("edge", "dc"), ("edge", "deg1"), ("edge", "dc-deg2"), ("regular", "base"), ("regular", "raw-aa-mod2.3"),
            ("tail_257", "base")]


@functools.lru_cache(maxsize=None)
def _case(name, form):
    inp, t, cam, f = PR.case_inputs(name, form, torch_out=True)
    sc = _Scene.of(inp["W"], inp["H"], np.array([0.3, 0.2, 0.1], dtype=np.float32), cam, inp["deg"],
                   dict(means3D=t["means3D"], dc=t["dc"], shs=t["shs"], colors=t["colors"], opacities=t["opacities"],
                        scales=t["scales"], rotations=t["rotations"], cov3D=t["cov3D"]),
                   raw=inp["raw"], scale_modifier=float(inp["scale_modifier"]), antialiasing=inp["antialiasing"])
    return inp, sc, PR.forward(inp, np.float64)


@functools.lru_cache(maxsize=None)
def _run(name, form, defer=0):
    inp, sc, _ = _case(name, form)
    with _env(**_UNSET):
        return _FrameRun(sc, 1, inp["depth_z"], defer_color=defer, allow_empty=True)


def _hold(what, fig):
    bad = {k: (v, BOUNDS[k]) for k, v in fig.items() if not v <= BOUNDS[k]}
    assert not bad, f"{what}: beyond the bound (figure, bound): {bad}"


def _between(got, pair, rows):
    lo, hi = (np.asarray(x).astype(np.int64) for x in pair)
    got = np.asarray(got).astype(np.int64)
    ok = (lo <= got) & (got <= hi)
    return bool(ok[rows].all())


def _check_forward(name, form, fr):
    inp, _, ref = _case(name, form)
    P = inp["means3D"].shape[0]
    radii, tt = fr.radii_host, fr.tiles_touched
    vis = radii > 0
    und = PR.undecided(ref)
    everyone = np.ones(P, dtype=bool)
    assert _between(vis, ref["visible"], everyone), "visibility outside the reference's (lo, hi)"
    assert not tt[~vis].any() and (fr.depth_key[~vis] == 0xFFFFFFFF).all()
    assert _between(radii, ref["radius"], vis), "radius"
    assert np.array_equal(fr.rec[vis, 11].view(np.uint32), fr.depth_key[vis])
    rows = vis & PR.continuous_ok(ref)
    fig = {}
    for j, k in enumerate(PR.RECORD):
        if k not in ("r", "g", "b"):
            fig[k] = PR.figures(fr.rec[:, j], ref["rec"][:, j], ref["S"][:, j], rows)
    if inp["colors"] is not None:
        for c, k in enumerate(("r", "g", "b")):
            fig[k] = PR.figures(fr.rec[:, 7 + c], ref["rec"][:, 7 + c], ref["S"][:, 7 + c], rows)
        assert not fr.clamped[vis].any()
    else:
        shaded = vis & (tt > 0)
        bits = ((fr.clamped[:, None] >> np.arange(3)[None, :]) & 1).astype(bool)
        assert _between(bits, ref["clamp"], shaded), "colour clamp bits"
        assert not fr.rec[:, 7:10][shaded[:, None] & bits].any(), "a clamped colour is not 0"
        assert not fr.rec[vis & (tt == 0), 7:10].any() and not fr.clamped[vis & (tt == 0)].any()
        for c, k in enumerate(("r", "g", "b")):
            fig[k] = PR.figures(fr.rec[:, 7 + c], np.maximum(ref["rgb_pre"][:, c], 0.0), ref["S_rgb_pre"][:, c], rows & shaded)
    # the tile rectangle `rect` holds: the first-stage box where the Gaussian keeps a tile, zeros where it keeps none
    kept = vis & (tt > 0)
    assert _between(fr.rect, ref["box"], kept), "first-stage box"
    assert not fr.rect[vis & (tt == 0)].any()
    # ... inside the published 3-sigma rectangle, which the radii imply
    rlo, rhi = ref["rect"]
    assert ((fr.rect[kept][:, :2] >= rlo[kept][:, :2]) & (fr.rect[kept][:, 2:] <= rhi[kept][:, 2:])).all()
    surely_empty, maybe_empty = ref["box_empty"]
    assert not tt[vis & surely_empty].any(), "tiles kept in an empty box"
    blo, bhi = ref["box"]
    for i in np.nonzero(vis)[0]:
        if tt[i] > 0:
            assert PR.row_interval_tiles(fr.rec[i], fr.rect[i], 1e-3) > 0, (i, "tiles kept although every row interval is empty")
        elif not maybe_empty[i]:
            widest = (blo[i, 0], blo[i, 1], bhi[i, 2], bhi[i, 3])
            assert PR.row_interval_tiles(fr.rec[i], widest, -1e-3) == 0, (i, "no tile kept although a row interval is not empty")
    counts = {k: int((u & vis).sum()) for k, u in und.items()}
    print(f"\n[A] {name} / {form}: visible {int(vis.sum())}, with tiles {int(kept.sum())}, undecided {counts} | "
          + " ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    _hold(f"forward {name} / {form}", fig)
    return fig


@pytest.mark.parametrize("name,form", FORWARD)
def test_forward_is_the_replay_of_its_inputs(name, form):
    """A, the fused colour path (k_preprocess_fwd: staged where the active degree is the stored one, unstaged below it)."""
    _check_forward(name, form, _run(name, form))


@pytest.mark.parametrize("name,form", DEFERRED)
def test_deferred_colour_is_the_same_replay(name, form):
    """A with the colour left to k_shade (defer_color = 1): the same bounds, and the very bits of the fused path."""
    a, b = _run(name, form), _run(name, form, 1)
    _check_forward(name, form, b)
    assert np.array_equal(a.rec.view(np.uint32), b.rec.view(np.uint32)) and np.array_equal(a.clamped, b.clamped)
    assert np.array_equal(a.rect, b.rect) and np.array_equal(a.tiles_touched, b.tiles_touched)


@pytest.mark.parametrize("name,form", [("edge", "raw-aa-mod2.3"), ("needles", "base"), ("tail_513", "base")])
def test_two_forwards_give_identical_bits(name, form):
    """C, forward: fresh states, the same bits in every view."""
    inp, sc, _ = _case(name, form)
    with _env(**_UNSET):
        a, b = _FrameRun(sc, 1, inp["depth_z"], allow_empty=True), _FrameRun(sc, 1, inp["depth_z"], allow_empty=True)
    for k in ("rec", "depth_key", "tiles_touched", "rect", "clamped", "radii_host"):
        x, y = getattr(a, k), getattr(b, k)
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y), k


def _grad_arrays(inp, d):
    P = inp["means3D"].shape[0]
    out = dict(means2D=d["m2"][:, :2], means3D=d["m3"], opacities=d["op"].reshape(P, 1))
    if "sc" in d:
        out.update(scales=d["sc"], rotations=d["ro"])
    if "cov" in d:
        out["cov3D"] = d["cov"]
    if "col" in d:
        out["colors"] = d["col"]
    else:
        sh = d["sh"].reshape(P, -1)
        out["shs"] = np.concatenate([d["dc"].reshape(P, -1), sh], axis=1) if "dc" in d else sh
    return out


def _check_backward(name, form, extras, defer=0):
    from diff_gaussian_rasterization import _C
    inp, _, ref = _case(name, form)
    fr = _run(name, form, defer)
    P = inp["means3D"].shape[0]
    lib = _C.lib()
    prev = lib.gsr_debug_set_flags_min_r(0xFFFFFFFF)          # every slot holds a record (zeros behind the walks)
    try:
        with _env(**_UNSET):
            recs, _, _, d = fr.backward(False, depth_only=extras)
            recs2, _, _, d2 = fr.backward(False, depth_only=extras)
    finally:
        lib.gsr_debug_set_flags_min_r(prev)
    assert np.array_equal(recs.view(np.uint32), recs2.view(np.uint32))
    for k in d:
        assert np.array_equal(d[k].view(np.uint32), d2[k].view(np.uint32)), f"C: {k} differs between two runs"
    sums, mag = PR.slot_order_sums(recs, fr.gid_of_slot, P)
    active = fr.tiles_touched > 0
    bits = ((fr.clamped[:, None] >> np.arange(3)[None, :]) & 1).astype(bool)
    b = PR.backward(inp, sums, mag, bits, active, np.float64)
    got = _grad_arrays(inp, d)
    assert not d["m2"][:, 2].any()
    rows = active & PR.continuous_ok(ref)
    fig = {}
    for k, g in got.items():
        g = g.reshape(P, -1)
        assert not g[~active].any(), f"{k}: a row of a Gaussian without instances is not zero"
        fig[k] = PR.figures(g, b["grads"][k], b["S"][k], rows)
    if not extras:
        assert not recs[:, 9].any()
    print(f"\n[B{', depth gradient' if extras else ''}] {name} / {form}: with instances {int(active.sum())}, compared {int(rows.sum())} | "
          + " ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    if name.startswith("needles"):     # (recorded in profiles/projection_replay.txt beside the float32 replay's per-stage table)
        rl2 = {k: float(np.linalg.norm((g.reshape(P, -1) - b["grads"][k])[rows]) / np.linalg.norm(b["grads"][k][rows])) for k, g in got.items()}
        kind = "depth gradient" if extras else "bare"
        print(f"[B, {kind}] {name} / {form}: kernel rel-L2 against the float64 replay | " + " ".join(f"{k} {v:.2e}" for k, v in rl2.items()))
        table, n = PR.stage_table(inp, PR.slot_order_sums_f32(recs, fr.gid_of_slot, P), sums, mag, bits)
        print(f"[stage table] {name} / {form}, {kind}\n" + "\n".join(PR.format_stage_table(table, n, f"{name} / {form}, own records, {kind}")))
    _hold(f"backward {name} / {form}", fig)


@pytest.mark.parametrize("extras", [False, True], ids=["bare", "depth"])
@pytest.mark.parametrize("name,form", BACKWARD)
def test_backward_is_the_replay_of_its_sums(name, form, extras):
    """B + C."""
    _check_backward(name, form, extras)


@pytest.mark.parametrize("name,form", DEFERRED)
def test_backward_after_deferred_colour(name, form):
    """B on a frame whose colours and clamp bits k_shade wrote (defer_color = 1), with dL/d(depth plane)."""
    _check_backward(name, form, True, defer=1)
