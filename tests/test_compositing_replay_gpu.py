"""The compositing kernels (csrc/render.hip: k_render_fwd, k_render_bwd, k_render_bwd_tile with and without sub-block masks, the
opt-in k_render_bwd_tile_mx) held to the float64 replay of tests/compositing_reference.py ON THEIR OWN FRAME: the float32
records, sorted lists and tile ranges the debug views expose, n_contrib and final_T from the image state, the gradient records from
the caller-made scratch buffer of gsr_backward (record index = gsr_debug_slot_views' slot of the list position).  Nothing upstream
of the records (projection, conic inversion) enters, so the bound holds on anisotropic scenes too.
  A  forward: n_contrib exact, colour / depth plane (both forms) / final_T / alpha plane within the bound on every pixel of every
     tile not left out; pixels outside the image never written; tile-local and global binning give identical bits.
  B  backward: every record of a walked instance within the bound, every record behind a walk all zeros (or flagged invalid with
     the validity flags forced on); every form, with and without dL/d(depth plane) and dL/d(alpha plane); the kernel's own records
     summed per Gaussian in float64 and mapped to dL/dmean2D against the dL_dmeans2D gsr_backward returns.
  C  two runs give identical bits.
BOUNDS.  |kernel - float64 replay| / S (S = the float64 sum of the magnitudes of the value's terms) <= 4 x the largest figure of
the float32 numpy replay over all cases, floor 2^-24: compositing_reference.YARDSTICK, measured on the CPU (`measure()` reprints it;
tests/test_compositing_reference_cpu.py recomputes it).  profiles/compositing_replay.txt holds these figures and the kernels'.
FOUND AND FIXED.  k_render_fwd, k_render_bwd and k_render_bwd_tile (masks on and off) held every bound from the start, the anisotropic
scenes included.  The opt-in matrix-pipe form (`mfma`: k_render_bwd_tile_mx, GSR_BWD_REDUCE=mfma) missed the bound of the SECOND MOMENTS,
6.36e-5: `sparse` h_dx2 8.2e-4 and h_dy2 1.1e-3, `needles` h_dy2 6.1e-4, `needles_08` h_dy2 9.2e-4.  It took the moments of h about the
TILE CENTRE and mapped them to d = mean - pixel after the sum; for a splat a pixel or two wide the three terms of that map are a few
hundred times the result.  It now forms each lane's terms about the mean, as the other forms do, and uses the matrix pipe for the
sums over the wave only: 5.9e-6 on `needles`, 6.4e-7 on `sparse`."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import compositing_reference as CR
from frame_run import CAP, DEV, _env, _FrameRun, _Scene

pytestmark = pytest.mark.gpu

BOUNDS = CR.bounds(CR.YARDSTICK)
RANDOM_CASES = list(CR.CASES)
STACK_CASES = [n for n in CR.all_case_names() if n not in CR.CASES]
_UNSET = dict(GSR_BWD_FORM=None, GSR_BWD_LPT=None, GSR_BWD_MASK=None, GSR_BWD_REDUCE=None, GSR_BWD_PRIO=None, GSR_FWD_MASK=None,
              GSR_BINNING=None)
FORMS = {"quad": dict(GSR_BWD_FORM="quad"), "tile": dict(GSR_BWD_FORM="tile", GSR_BWD_MASK="1"),
         "tile-mask0": dict(GSR_BWD_FORM="tile", GSR_BWD_MASK="0"), "mfma": dict(GSR_BWD_FORM="tile", GSR_BWD_REDUCE="mfma")}


def measure():
    """Reprints the float32 replay's figures (CPU, about two minutes): the constants of compositing_reference.YARDSTICK."""
    worst = {}
    for name in CR.all_case_names():
        fig, _, _ = CR.yardstick(name, verbose=True)
        worst = {k: max(worst.get(k, 0.0), v) for k, v in fig.items()}
    for k in CR.CLASSES:
        print(f"{k}: yardstick {worst[k]:.4e}, bound {max(CR.FLOOR, CR.FACTOR * worst[k]):.4e}")


@functools.lru_cache(maxsize=None)
def _scene(name):
    return _Scene(name)


@functools.lru_cache(maxsize=None)
def _run(name, tlo=1, depth_z=False):
    with _env(**_UNSET):
        return _FrameRun(_scene(name), tlo, depth_z)


@functools.lru_cache(maxsize=None)
def _forward_ref(name, depth_z=False):
    return CR.forward_reference(_run(name, 1, depth_z).frame)


@functools.lru_cache(maxsize=None)
def _backward_ref(name, extras):
    fr = _run(name)
    gp, gd, gA = CR.upstream(fr.sc.W, fr.sc.H)
    return CR.backward_reference(fr.frame, fr.out["nc"], fr.out["fT"], (gp, gd if extras else None, gA if extras else None))


def _report(what, name, fig, ref_left, tiles):
    print(f"\n[{what}] {name}: tiles {tiles}, left out {ref_left} | " + " ".join(f"{k} {v:.2e}" for k, v in fig.items()))


def _hold(what, name, fig):
    bad = {k: (v, BOUNDS[k]) for k, v in fig.items() if not v <= BOUNDS[k]}
    assert not bad, f"{what}, {name}: beyond the bound (figure, bound): {bad}"


@pytest.mark.parametrize("depth_z", [False, True], ids=["inverse", "z"])
@pytest.mark.parametrize("name", RANDOM_CASES + STACK_CASES)
def test_forward_is_the_replay_of_its_frame(name, depth_z):
    """A: both depth-plane forms.  (The stack cases put a list end on either side of FWD_BATCH = 256 and the pixels' stops on
    either side of entries 64, 128, 256.)"""
    fr, ref = _run(name, 1, depth_z), _forward_ref(name, depth_z)
    tiles = fr.frame.tiles
    left = int(ref["left_out"].sum())
    fig, bad_nc = CR.forward_errors(ref, fr.out)
    _report(f"A, depth {'z' if depth_z else 'inverse'}", name, fig, left, tiles)
    assert left <= CR.LEFT_OUT_CAP * tiles, (left, tiles)
    assert bad_nc == 0, f"{name}: n_contrib of {bad_nc} pixels matches no assignment of their doubtful tests"
    _hold("forward", name, fig)
    assert np.array_equal(fr.out["alpha"], np.float32(1.0) - fr.out["fT"])
    if depth_z:      # colour, final_T and n_contrib do not depend on the depth kind
        a = _run(name, 1, False)
        assert all(np.array_equal(fr.out[k], a.out[k]) for k in ("color", "fT", "nc", "alpha"))
        seen = np.unique(fr.point_list[fr.point_list != CR.NO_ID])
        assert np.array_equal(fr.rec[seen, 10], fr.rec[seen, 11])


@pytest.mark.parametrize("name", ["partial_tiles", "single_tile"])
def test_pixels_outside_the_image_are_never_written(name):
    """A: the five planes lie back to back inside a larger pre-filled buffer, the image state inside a larger pre-filled one.  A
    pixel below the image (a partial tile's rows) would land in the next plane or behind the last one, one right of it on the next
    row: after the forward everything around the planes and around the state still holds the pattern, and the planes are, bit for
    bit, those of the run on separate buffers (which the replay holds pixel by pixel)."""
    from diff_gaussian_rasterization import _C, _stream
    lib = _C.lib()
    sc = _scene(name)
    P, W, H = sc.P, sc.W, sc.H
    N = W * H
    pad = 16 * (W + 16)
    buf = torch.full((5 * N + 2 * pad,), 12345.0, device=DEV)
    state = lib.gsr_image_state_bytes(W, H)
    img = torch.full((state + 2 * 4096,), 0x5A, dtype=torch.uint8, device=DEV)
    geom = torch.zeros(max(4096, lib.gsr_geometry_state_bytes(P)), dtype=torch.uint8, device=DEV)
    binning = torch.zeros(lib.gsr_binning_state_bytes(P, W, H, CAP), dtype=torch.uint8, device=DEV)
    radii = torch.zeros(P, dtype=torch.int32, device=DEV)
    status = torch.zeros(8, dtype=torch.int64).pin_memory()
    body = buf[pad:pad + 5 * N]
    ex = _C.gsr_render_extras(0, body[4 * N:].data_ptr(), None)
    with _env(**_UNSET):
        _C.check(lib.gsr_forward_async_ex(C.byref(sc.s), C.byref(sc.g), _C.ptr(geom), geom.numel(), _C.ptr(radii), _C.ptr(binning),
                                          binning.numel(), CAP, C.c_void_p(img.data_ptr() + 4096), state, _C.ptr(body),
                                          C.c_void_p(body[3 * N:].data_ptr()), 1, 0, None, C.c_void_p(status.data_ptr()), 1,
                                          _stream(), None, C.byref(ex)))
    torch.cuda.synchronize()
    assert bool((buf[:pad] == 12345.0).all()) and bool((buf[pad + 5 * N:] == 12345.0).all())
    assert bool((img[:4096] == 0x5A).all()) and bool((img[4096 + state:] == 0x5A).all())
    ref = _run(name)
    got = body.cpu().numpy()
    assert np.array_equal(got[:3 * N], ref.out["color"].reshape(-1)) and np.array_equal(got[3 * N:4 * N], ref.out["depth"])
    assert np.array_equal(got[4 * N:], ref.out["alpha"])


@pytest.mark.parametrize("name", RANDOM_CASES + ["stack_a_257", "stop_128"])
def test_both_binning_forms_give_identical_bits(name):
    """A: tile-local binning against the global form (tile_local_sort = 0, what GSR_BINNING=global makes the Python workspace
    pass): records, lists, images, image state."""
    a, b = _run(name), _run(name, 0)
    assert np.array_equal(a.point_list, b.point_list) and np.array_equal(a.ranges, b.ranges)
    assert np.array_equal(a.rec.view(np.uint32), b.rec.view(np.uint32))
    for k in ("color", "depth", "alpha", "fT", "nc"):
        assert np.array_equal(a.out[k].view(np.uint32) if a.out[k].dtype == np.float32 else a.out[k],
                              b.out[k].view(np.uint32) if b.out[k].dtype == np.float32 else b.out[k]), k


def _backward_check(name, form, extras, flags_forced):
    from diff_gaussian_rasterization import _C
    fr, ref = _run(name), _backward_ref(name, extras)
    lib = _C.lib()
    prev = lib.gsr_debug_set_flags_min_r(0 if flags_forced else 0xFFFFFFFF)
    try:
        with _env(**{**_UNSET, **FORMS[form]}):
            recs, flags, m2, _ = fr.backward(extras)
            recs2, flags2, m2b, _ = fr.backward(extras)
    finally:
        lib.gsr_debug_set_flags_min_r(prev)
    # C: reproducible bit for bit (where the flags say "no record" the record bytes are not the kernel's)
    valid = flags != 0 if flags_forced else np.ones(fr.R, dtype=bool)
    assert np.array_equal(recs[valid].view(np.uint32), recs2[valid].view(np.uint32)) and np.array_equal(m2.view(np.uint32), m2b.view(np.uint32))
    if flags_forced:
        assert np.array_equal(flags, flags2) and set(np.unique(flags)) <= {0, 1}
    tile, pos, _ = CR.instances(fr.frame)
    walk = np.array([r["walk"] for r in ref])
    walked = pos < walk[tile]
    by_pos = recs[fr.slot]                                                  # list order
    # behind the walk: all zeros, or flagged invalid; inside it: a record (flag set)
    if flags_forced:
        assert np.array_equal(flags[fr.slot] != 0, walked), "validity flags are not exactly the walked instances"
    else:
        assert not by_pos[~walked][:, :10].any(), "a record behind its tile's walk is not all zeros"
    by_pos = np.where(walked[:, None], by_pos, np.float32(0.0))
    base = fr.frame.ranges[:, 0]
    got = [by_pos[base[t]:base[t] + walk[t], :10] for t in range(fr.frame.tiles)]
    fig, chosen = CR.backward_errors(ref, got)
    left = sum(r["left_out"] for r in ref)
    # the per-Gaussian sums in slot order and the moment-to-mean map, from the kernel's OWN records (stages ii and iii, for the mean)
    fig["mean2D"] = CR.mean2d_error(fr.frame, by_pos[:, :10], fr.slot, m2)
    _report(f"B, {form}{', depth + alpha gradients' if extras else ''}{', flags' if flags_forced else ''}", name, fig, left,
            fr.frame.tiles)
    assert left <= CR.LEFT_OUT_CAP * fr.frame.tiles
    if not extras:
        fig.pop("d_depth")
        assert not by_pos[:, 9].any()                                       # no gradient on the depth plane: the tenth value stays zero
    _hold(f"backward {form}", name, fig)
    assert not m2[:, 2].any()


@pytest.mark.parametrize("extras", [False, True], ids=["bare", "depth+alpha"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", RANDOM_CASES)
def test_backward_records_are_the_replay_of_their_frame(name, form, extras):
    """B + C on the random frames, zero records behind the walks."""
    _backward_check(name, form, extras, flags_forced=False)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", STACK_CASES)
def test_backward_records_at_the_batch_ends(name, form):
    """B + C on the stacks: lists of 1 .. 513 entries around BWD1_BATCH = 64, BWD_BATCH = 128 (and a fifth batch), walks that end
    on either side of a batch end; with the depth-plane and alpha-plane gradients."""
    _backward_check(name, form, True, flags_forced=False)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", ["saturating", "needles", "stop_128"])
def test_backward_records_with_validity_flags(name, form):
    """B with gsr_debug_set_flags_min_r(0): no zero records, one validity byte per slot - set exactly for the walked instances."""
    _backward_check(name, form, False, flags_forced=True)
