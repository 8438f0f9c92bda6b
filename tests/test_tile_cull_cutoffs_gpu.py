"""WHICH depth cut-off the compositing forward learns per tile (csrc/render.hip k_render_fwd; gsr_forward_async_culled), held to
the float64 reconstruction of tests/tile_cull_reference.py bit for bit.  tests/test_tile_cull_gpu.py shows that training with
truncated lists ends where training without ends, and that most tiles get SOME finite cut-off; a cut-off that is too loose only
costs time and one that is too tight is caught by the CULL_MISS re-run, so neither shows there.  Here, through the C ABI:
  (a) the learnt value of every non-ambiguous tile, tile-local binning form, with and without a backward to follow;
  (b) the boundary k == len (all ones) against k == len - 1 (the last entry's key);
  (c) the global binning form learns the same values as the tile-local form (both forms produce bit-identical lists);
  (d) learn, apply, apply again: the cut-offs and the frame are a fixed point, and a hand-made tighter cut-off is kept;
  (e) soundness independent of the margin: nothing a tile needed lies behind its cut-off, and emission keeps exactly key <= cut-off;
  (f) P == 0 and R == 0 leave the tensor as it was.
Every frame has at most 4000 Gaussians and 208 x 144 pixels."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import tile_cull_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
ALL = R.ALL
FRAME_CASES = ["saturating", "sparse", "partial_tiles", "single_tile", "small", "three"]


class _Scene:
    """Settings and Gaussians of one view as the C ABI takes them (the tensors are kept alive here)."""

    def __init__(self, raw, cam, deg, W, H):
        from diff_gaussian_rasterization import GaussianRasterizationSettings, _settings_struct, _gauss_struct
        from helpers import leaf_inputs
        self.W, self.H = W, H
        inp = leaf_inputs(raw, torch.float32, DEV, "sh")
        self.t = {k: v.detach().contiguous() for k, v in inp.items()}
        self.P = int(self.t["means3D"].shape[0])
        rs = GaussianRasterizationSettings(H, W, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), torch.zeros(3, device=DEV),
                                           1.0, cam.world_view_transform.to(DEV), cam.full_proj_transform.to(DEV), deg,
                                           cam.camera_center.to(DEV), False, False, False)
        self.s, self.keep = _settings_struct(rs, DEV)
        t = self.t
        self.g = _gauss_struct(self.P, t["means3D"], None, t["shs"], None, t["opacities"], t["scales"], t["rotations"], None)


def _new_cut(sc, fill=-1):
    import diff_gaussian_rasterization as dgr
    cut = dgr.new_tile_cull(sc.H, sc.W, DEV)          # (the library's tile grid sizes it: partial tiles count)
    assert cut.numel() == math.prod(R.tile_grid(sc.W, sc.H))
    return cut.fill_(fill)


def _u32(t):
    return t.detach().cpu().numpy().view(np.uint32).copy()


def _frame(sc, cut, apply, tlo=1, for_backward=1, cap=1 << 20):
    """One gsr_forward_async_culled call (unverified) on fresh states -> images, status, the frame's records, keys and lists."""
    from diff_gaussian_rasterization import _C, _stream
    from helpers import _view
    lib = _C.lib()
    P, W, H = sc.P, sc.W, sc.H
    geom = torch.zeros(max(4096, lib.gsr_geometry_state_bytes(P)), dtype=torch.uint8, device=DEV)
    img = torch.zeros(lib.gsr_image_state_bytes(W, H), dtype=torch.uint8, device=DEV)
    binning = torch.zeros(lib.gsr_binning_state_bytes(P, W, H, cap), dtype=torch.uint8, device=DEV)
    radii = torch.zeros(max(P, 1), dtype=torch.int32, device=DEV)
    color, invd = torch.empty(3, H, W, device=DEV), torch.empty(1, H, W, device=DEV)
    status = torch.zeros(4, dtype=torch.int64).pin_memory()
    _C.check(lib.gsr_forward_async_culled(C.byref(sc.s), C.byref(sc.g), _C.ptr(geom), geom.numel(), _C.ptr(radii), _C.ptr(binning),
                                          binning.numel(), cap, _C.ptr(img), img.numel(), _C.ptr(color), _C.ptr(invd),
                                          for_backward, 0, None, C.c_void_p(status.data_ptr()), tlo, _stream(), None,
                                          _C.ptr(cut), 1 if apply else 0))
    torch.cuda.synchronize()
    tiles = cut.numel()
    out = dict(color=color.cpu(), invd=invd.cpu(), cut=_u32(cut), R=int(status[1]), flags=int(status[0]) & 0xFFFFFFFF,
               miss=int(status[3]) & 0xFFFFFFFF)
    pi = [C.c_void_p() for _ in range(2)]
    lib.gsr_debug_image_views(_C.ptr(img), W, H, C.byref(pi[0]), C.byref(pi[1]))
    out["fT"] = _view(img, pi[0].value, W * H, torch.float32)
    out["nc"] = _view(img, pi[1].value, W * H, torch.int32)
    if P == 0:
        return out
    assert out["R"] <= cap and out["flags"] & 1 == 0
    pv = [C.c_void_p() for _ in range(6)]
    lib.gsr_debug_geometry_views(_C.ptr(geom), P, *[C.byref(p) for p in pv], None)
    out["rec"] = _view(geom, pv[0].value, P * 12, torch.float32).view(P, 12).numpy()
    out["keys"] = _view(geom, pv[1].value, P, torch.int32).numpy().view(np.uint32)     # (unsorted in the tile-local form only)
    pb = [C.c_void_p() for _ in range(2)]
    lib.gsr_debug_binning_views(_C.ptr(binning), W, H, cap, C.byref(pb[0]), C.byref(pb[1]))
    out["point_list"] = _view(binning, pb[0].value, max(out["R"], 1), torch.int32).numpy().view(np.uint32)[:out["R"]]
    out["ranges"] = _view(binning, pb[1].value, tiles * 2, torch.int32).numpy().view(np.uint32).reshape(tiles, 2)
    return out


def _expect(sc, fr, q8=R.MARGIN_Q8, add=R.MARGIN_ADD):
    """The reference on the frame's OWN float32 records (promoted), lists and keys."""
    return R.expected_cutoffs(fr["rec"].astype(np.float64), fr["ranges"], fr["point_list"], fr["keys"], sc.W, sc.H, q8, add)


@functools.lru_cache(maxsize=None)
def _scene(name):
    return _Scene(*R.case_scene(name))


@functools.lru_cache(maxsize=None)
def _learnt(name, tlo, for_backward):
    """Frame 1 of a view: apply = 0, cut-offs all ones before.  Cached: (a), (c), (d) and (e) share these frames unchanged."""
    sc = _scene(name)
    return _frame(sc, _new_cut(sc), apply=False, tlo=tlo, for_backward=for_backward)


@functools.lru_cache(maxsize=None)
def _reference(name):
    return _expect(_scene(name), _learnt(name, 1, 1))


def _hold(name, got, exp, what):
    """got == exp on every non-ambiguous tile; prints the counts; -> number of finite expected values compared"""
    amb = exp["ambiguous"]
    tiles = len(amb)
    fin = int(((exp["cutoff"] != ALL) & ~amb).sum())
    ones = int(((exp["cutoff"] == ALL) & ~amb).sum())
    print(f"\n[{what}] {name}: tiles {tiles}, compared {tiles - int(amb.sum())} (finite {fin}, all ones {ones}), "
          f"ambiguous (left out) {int(amb.sum())}")
    assert amb.sum() <= R.AMBIGUOUS_CAP * tiles, (name, int(amb.sum()), tiles)
    bad = np.nonzero((got != exp["cutoff"]) & ~amb)[0]
    assert bad.size == 0, (f"{what} {name}: {bad.size} tiles differ; first tile {int(bad[0])}: written 0x{int(got[bad[0]]):08X}, "
                           f"expected 0x{int(exp['cutoff'][bad[0]]):08X} (need {int(exp['need'][bad[0]])}, k {int(exp['k'][bad[0]])}, "
                           f"len {int(exp['len'][bad[0]])})")
    return fin


@pytest.mark.parametrize("for_backward", [0, 1])
@pytest.mark.parametrize("name", FRAME_CASES)
def test_learnt_cutoffs_equal_the_float64_reconstruction(name, for_backward):
    """(a) tile-local form, apply = 0: per tile the key of the entry at 0-based index k = 1.75 need + 48, all ones where the list
    is shorter or a pixel never saturated.  192 x 128 saturating and sparse, 200 x 120 (partial tiles right and bottom), one tile,
    40 x 24, and P = 3 (every list shorter than the margin)."""
    sc, fr = _scene(name), _learnt(name, 1, for_backward)
    ref = _learnt(name, 1, 1)
    same = all(np.array_equal(fr[k], ref[k]) for k in ("rec", "keys", "point_list", "ranges"))
    exp = _reference(name) if same else _expect(sc, fr)
    assert fr["miss"] == 0
    fin = _hold(name, fr["cut"], exp, f"a, for_backward={for_backward}")
    if name == "saturating":
        assert fin >= len(fr["cut"]) // 2, fin
    if name == "three":
        assert (fr["cut"] == ALL).all() and (exp["len"] <= 3).all()


@pytest.mark.parametrize("for_backward", [0, 1])
@pytest.mark.parametrize("name", FRAME_CASES)
def test_global_form_learns_what_the_tile_local_form_learns(name, for_backward):
    """(c) tile_local_sort = 0: the depth keys were radix-sorted in place by then (api.hip forward_geometry), so the kernel must
    not index them by Gaussian id.  It takes the key from the record's depth word, which holds the same bits."""
    a = _learnt(name, 1, for_backward)
    b = _learnt(name, 0, for_backward)
    assert np.array_equal(a["point_list"], b["point_list"]) and np.array_equal(a["ranges"], b["ranges"])
    assert torch.equal(a["color"], b["color"]) and torch.equal(a["fT"], b["fT"])
    bad = np.nonzero(a["cut"] != b["cut"])[0]
    print(f"\n[c, for_backward={for_backward}] {name}: tiles {len(a['cut'])}, finite {int((a['cut'] != ALL).sum())}, differing {bad.size}")
    assert bad.size == 0, (f"global form, {name}: {bad.size} tiles differ; first tile {int(bad[0])}: written 0x{int(b['cut'][bad[0]]):08X}, "
                           f"expected 0x{int(a['cut'][bad[0]]):08X}")


def test_record_depth_word_is_the_depth_key():
    """What (c)'s fix rests on: for every Gaussian that reaches a list, word 11 of its record holds the bits of its sort key."""
    fr = _learnt("saturating", 1, 1)
    ids = np.unique(fr["point_list"])
    ids = ids[ids != R.NO_ID]
    assert ids.size > 1000
    assert np.array_equal(fr["rec"][:, 11].copy().view(np.uint32)[ids], fr["keys"][ids])


def test_boundary_k_equals_len(monkeypatch):
    """(b) one tile, a stack of N identical wide splats, margin "256,3" (k = need + 3; the launcher reads GSR_CULL_MARGIN on every
    call).  N = k_ref: the margin reaches exactly past the list, all ones.  N = k_ref + 1: index k is the last entry."""
    add = 3
    monkeypatch.setenv("GSR_CULL_MARGIN", f"256,{add}")
    sc = _Scene(*R.stack_scene(24))
    probe = _frame(sc, _new_cut(sc), apply=False)
    e = _expect(sc, probe, 256, add)
    assert not e["ambiguous"][0] and e["need"][0] != ALL and e["len"][0] == 24
    k_ref = int(e["k"][0])
    assert k_ref == int(e["need"][0]) + add and 6 + add <= k_ref < 23
    for n, last in ((k_ref, False), (k_ref + 1, True)):
        sc = _Scene(*R.stack_scene(n))
        fr = _frame(sc, _new_cut(sc), apply=False)
        e = _expect(sc, fr, 256, add)
        assert not e["ambiguous"][0] and int(e["k"][0]) == k_ref and int(e["len"][0]) == n
        print(f"\n[b] N {n}: need {int(e['need'][0])}, k {k_ref}, len {n}, written 0x{int(fr['cut'][0]):08X}")
        want = int(fr["keys"][fr["point_list"][n - 1]]) if last else ALL
        assert int(e["cutoff"][0]) == want and int(fr["cut"][0]) == want, (n, hex(int(fr["cut"][0])), hex(want))
        if last:
            assert want == int(fr["keys"].max()) != ALL


@pytest.mark.parametrize("name", ["saturating", "partial_tiles"])
def test_learn_apply_apply_is_a_fixed_point(name):
    """(d) + (e).  Frame 1 learns, frames 2 and 3 apply: the tensor stays what frame 1 left (a truncated list is a prefix that
    still holds index k), the frames are frame 1 bit for bit, word 6 stays clear.  And, whatever the margin: every entry up to
    `need` of the untruncated list has key <= cut-off, and the truncated frame's list of every tile holds exactly the entries
    with key <= cut-off."""
    sc, f1, exp = _scene(name), _learnt(name, 1, 1), _reference(name)
    cut = torch.from_numpy(f1["cut"].view(np.int32).copy()).to(DEV)
    keys, pl = f1["keys"], f1["point_list"]
    finite = f1["cut"] != ALL
    assert finite.sum() > len(finite) // 2
    for n in (2, 3):
        f = _frame(sc, cut, apply=True)
        assert f["miss"] == 0 and f["flags"] & 2 == 0, n
        assert np.array_equal(f["cut"], f1["cut"]), (n, np.nonzero(f["cut"] != f1["cut"])[0][:4])
        for k in ("color", "invd", "fT", "nc"):
            assert torch.equal(f[k], f1[k]), (n, k)
        assert f["R"] < f1["R"]
        for t in range(len(finite)):
            lo, hi = int(f1["ranges"][t, 0]), int(f1["ranges"][t, 1])
            tk = keys[pl[lo:hi]]
            assert int((tk <= f1["cut"][t]).sum()) == int(f["ranges"][t, 1]) - int(f["ranges"][t, 0]), (n, t)
            if finite[t] and not exp["ambiguous"][t]:
                assert exp["need"][t] != ALL and (tk[:int(exp["need"][t])] <= f1["cut"][t]).all(), (n, t)
    print(f"\n[d, e] {name}: R {f1['R']} -> {f['R']}, finite tiles {int(finite.sum())} of {len(finite)}")


def test_a_tighter_cutoff_that_still_holds_is_kept():
    """The "keep the wider cut-off" branch: a frame truncated right behind what each tile needs (the key at 0-based index `need`)
    still saturates everywhere, but index k now lies past its lists: the kernel must leave those words alone.  Where equal keys
    make the truncated list reach index k after all, it writes the key found there."""
    name = "saturating"
    sc, f1, exp = _scene(name), _learnt(name, 1, 1), _reference(name)
    keys, pl, rg = f1["keys"], f1["point_list"], f1["ranges"].astype(np.int64)
    tight = np.full(len(exp["need"]), ALL, dtype=np.uint32)
    want = tight.copy()
    sure = ~exp["ambiguous"]
    for t in range(len(tight)):
        tk = keys[pl[rg[t, 0]:rg[t, 1]]]
        if exp["need"][t] != ALL and exp["need"][t] < len(tk) and sure[t]:
            tight[t] = tk[int(exp["need"][t])]
        kept = tk[tk <= tight[t]]
        if exp["need"][t] != ALL and exp["k"][t] < len(kept):
            want[t] = kept[int(exp["k"][t])]
        elif exp["need"][t] != ALL and len(kept) < len(tk):
            want[t] = tight[t]                                # truncated, and the margin reaches past the list: kept
    assert (tight != ALL).sum() > len(tight) // 2 and (want == tight)[tight != ALL].sum() > len(tight) // 2
    f = _frame(sc, torch.from_numpy(tight.view(np.int32).copy()).to(DEV), apply=True)
    assert f["miss"] == 0 and f["R"] < f1["R"]
    for k in ("color", "invd", "fT", "nc"):
        assert torch.equal(f[k], f1[k]), k
    bad = np.nonzero((f["cut"] != want) & sure)[0]
    assert bad.size == 0, (bad[:4], [hex(int(f["cut"][b])) for b in bad[:4]], [hex(int(want[b])) for b in bad[:4]])


@pytest.mark.parametrize("tlo", [0, 1])
def test_a_frame_without_gaussians_leaves_the_tensor_alone(tlo):
    """(f) P == 0: no cut-off pointer reaches the kernel, a tensor pre-filled with a pattern comes back unchanged.  P == 3 with
    every Gaussian behind the camera (a binning state with room, but empty lists): no pixel saturates, every word is all ones."""
    from scene_utils.synthetic import RawGaussians
    raw, cam, deg, W, H = R.case_scene("three")
    pattern = 0x1234567
    empty = RawGaussians(*(t[:0] for t in raw.tensors()), raw.sh_degree)
    behind = RawGaussians(cam.camera_center.cpu()[None, :] * torch.tensor([[2.0], [2.5], [3.0]]), *raw.tensors()[1:], raw.sh_degree)
    for what, scene, want in (("P == 0", empty, pattern), ("all behind the camera", behind, ALL)):
        sc = _Scene(scene, cam, deg, W, H)
        cut = _new_cut(sc, pattern)
        fr = _frame(sc, cut, apply=False, tlo=tlo)
        assert fr["R"] == 0 and float(fr["fT"].min()) == 1.0 and fr["miss"] == 0, what
        assert (fr["cut"] == want).all(), what
