"""Keyframe covisibility (scene_utils.keyframes), GaussianModel.prune_points bookkeeping and the ctypes layout of
gsr_render_extras - everything here runs on CPU tensors (prune_points is plain torch indexing, so it does too)."""
import ctypes as C

import pytest
import torch

from scene_utils import GaussianModel, make_gaussians, covisibility, KeyframeWindow, prune_unobserved
from scene_utils.model import _PARAM_ATTRS


def _mask(P, idx):
    m = torch.zeros(P, dtype=torch.bool)
    m[list(idx)] = True
    return m


# ---- covisibility -------------------------------------------------------------------------------------------------------------
def test_covisibility_on_hand_made_masks():
    a, b = _mask(10, range(0, 6)), _mask(10, range(4, 8))           # |A| = 6, |B| = 4, |A n B| = 2, |A u B| = 8
    assert covisibility(a, b) == (2 / 8, 2 / 4)
    assert covisibility(b, a) == (2 / 8, 2 / 4)
    assert covisibility(a, a) == (1.0, 1.0)
    assert covisibility(_mask(10, range(3)), _mask(10, range(6))) == (3 / 6, 1.0)      # a subset: overlap coefficient 1
    e = _mask(10, ())
    assert covisibility(e, e) == (0.0, 0.0) and covisibility(a, e) == (0.0, 0.0) and covisibility(e, a) == (0.0, 0.0)
    assert covisibility(_mask(10, (0, 1)), _mask(10, (2, 3))) == (0.0, 0.0)


def test_covisibility_takes_counts_and_a_pixel_threshold():
    a = torch.tensor([0, 1, 5, 9, 0], dtype=torch.int32)
    b = torch.tensor([3, 0, 2, 9, 0], dtype=torch.int32)
    assert covisibility(a, b) == (2 / 4, 2 / 3)
    assert covisibility(a, b, min_pixels=3) == (1 / 3, 1 / 2)       # A = {2, 3}, B = {0, 3}
    assert covisibility(a, b > 0) == (2 / 4, 2 / 3)                 # counts against a mask


def test_covisibility_refuses_unequal_lengths():
    with pytest.raises(ValueError, match="lengths"):
        covisibility(_mask(10, (1,)), _mask(11, (1,)))
    with pytest.raises(ValueError):
        covisibility(torch.zeros(2, 3), torch.zeros(2, 3))


# ---- KeyframeWindow -----------------------------------------------------------------------------------------------------------
def test_window_keyframe_decision():
    w = KeyframeWindow(3)
    a = _mask(100, range(0, 50))
    assert w.is_keyframe(a)                                          # an empty window takes anything
    assert w.add("a", a) == []
    assert not w.is_keyframe(_mask(100, range(0, 48)))               # IoU 0.96
    assert w.is_keyframe(_mask(100, range(10, 50)))                  # IoU 0.8 < 0.9
    assert not w.is_keyframe(_mask(100, range(10, 50)), iou_below=0.7)
    w.add("b", _mask(100, range(50, 100)), overlap_cutoff=0.0)
    assert w.is_keyframe(a)                                          # compared with the NEWEST keyframe, not with any


def test_window_eviction_order_and_the_protected_newest_two():
    w = KeyframeWindow(3)
    assert w.add(0, _mask(100, range(0, 40))) == []
    assert w.add(1, _mask(100, range(30, 70))) == []                 # overlap with 0: 10 / 40 = 0.25, but 0 is one of the newest two
    assert w.ids == [0, 1]
    # keyframe 2 shares nothing with 1 (protected: newest two are 1, 2) and 10 / 40 <= 0.4 with ... 0 shares 0 with it: evicted
    assert w.add(2, _mask(100, range(70, 100))) == [0]
    assert w.ids == [1, 2]
    assert w.add(3, _mask(100, range(60, 100)), overlap_cutoff=0.2) == []      # 1 shares 10 / 40 = 0.25 > 0.2: stays
    assert w.ids == [1, 2, 3]
    # over the size: the oldest goes, after the cutoff had its say (cutoff 0.0 evicts only what shares nothing)
    assert w.add(4, _mask(100, range(55, 100)), overlap_cutoff=0.0) == [1]
    assert w.ids == [2, 3, 4]
    # the cutoff looks at every keyframe but the newest two (4 and the new one): 2 shares nothing, 3 shares 10 / 30 <= 0.4
    assert w.add(5, _mask(100, range(40, 70)), overlap_cutoff=0.4) == [2, 3]
    assert w.ids == [4, 5]                                           # 4 shares 15 / 30 and is protected anyway
    # both kinds in one call, the cutoff first, then the oldest while over the size
    w3 = KeyframeWindow(2)
    w3.add("p", _mask(100, range(0, 10)))
    w3.add("q", _mask(100, range(0, 50)))
    assert w3.add("r", _mask(100, range(5, 50))) == ["p"] and w3.ids == ["q", "r"]          # p shares 5 / 10: over the size
    assert w3.add("s", _mask(100, range(60, 70))) == ["q"] and w3.ids == ["r", "s"]          # q shares nothing: the cutoff
    w2 = KeyframeWindow(1)
    assert w2.add("x", _mask(5, (0,))) == [] and w2.add("y", _mask(5, (0,))) == ["x"] and w2.ids == ["y"]


def test_window_observations_and_resized():
    w = KeyframeWindow(4)
    assert w.observations().numel() == 0
    w.add("a", torch.tensor([1, 0, 3, 0, 2], dtype=torch.int32), overlap_cutoff=0.0)
    w.add("b", torch.tensor([0, 0, 1, 7, 2], dtype=torch.int32), overlap_cutoff=0.0)
    w.add("c", torch.tensor([1, 0, 1, 1, 0], dtype=torch.int32), overlap_cutoff=0.0)
    obs = w.observations()
    assert obs.dtype == torch.int32 and obs.tolist() == [2, 0, 3, 2, 2]
    with pytest.raises(ValueError):
        w.add("d", torch.zeros(6, dtype=torch.int32))                # the map grew: resized() first
    with pytest.raises(ValueError):
        w.is_keyframe(torch.zeros(4, dtype=torch.int32))
    w.resized(7)                                                     # after an insertion: padded with False
    assert w.observations().tolist() == [2, 0, 3, 2, 2, 0, 0]
    with pytest.raises(ValueError):
        w.resized(6)                                                 # shrinking needs keep=
    keep = torch.tensor([True, False, True, True, False, True, True])
    with pytest.raises(ValueError):
        w.resized(4, keep=keep)                                      # keep selects 5 rows
    with pytest.raises(ValueError):
        w.resized(5, keep=keep[:6])
    assert w.observations().tolist() == [2, 0, 3, 2, 2, 0, 0]        # a refused call changed nothing
    w.resized(5, keep=keep)                                          # after a prune
    assert w.observations().tolist() == [2, 3, 2, 0, 0] and w.ids == ["a", "b", "c"]


# ---- prune_points -------------------------------------------------------------------------------------------------------------
def _live_model(P=40):
    model = GaussianModel.from_raw(make_gaussians(P, 1, seed=3))
    opt = model.training_setup(optimizer="torch")
    gen = torch.Generator().manual_seed(5)
    for _ in range(2):
        for p in model.parameters():
            p.grad = torch.randn(p.shape, generator=gen)
        opt.step()
    model.xyz_gradient_accum += torch.rand(P, 1, generator=gen)
    model.denom += 1
    model.max_radii2D += torch.rand(P, generator=gen)
    return model, opt


def test_prune_points_keeps_the_survivors_bit_for_bit_and_calls_the_hooks():
    model, opt = _live_model()
    P = 40
    calls = []
    model._resize_hooks.append(calls.append)
    mask = _mask(P, (0, 7, 8, 39))
    keep = ~mask
    old = [getattr(model, a).detach().clone() for a in _PARAM_ATTRS]
    old_m = [(opt.state[getattr(model, a)]["exp_avg"].clone(), opt.state[getattr(model, a)]["exp_avg_sq"].clone(),
              opt.state[getattr(model, a)]["step"]) for a in _PARAM_ATTRS]
    assert all(float(m[0].abs().max()) > 0 for m in old_m)
    stats = [model.xyz_gradient_accum.clone(), model.denom.clone(), model.max_radii2D.clone()]
    ids = [id(getattr(model, a)) for a in _PARAM_ATTRS]
    assert model.prune_points(torch.zeros(P, dtype=torch.bool)) == 0      # all False: nothing changes, no hook
    assert calls == [] and ids == [id(getattr(model, a)) for a in _PARAM_ATTRS]
    assert model.prune_points(mask) == 4
    assert calls == ["before", "after"]
    groups = {g["name"]: g for g in opt.param_groups}
    for a, name, o, (m1, m2, step) in zip(_PARAM_ATTRS, ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"), old, old_m):
        p = getattr(model, a)
        assert p.shape[0] == P - 4 and p.requires_grad and p.is_contiguous() and torch.equal(p.detach(), o[keep])
        assert groups[name]["params"][0] is p
        st = opt.state[p]
        assert torch.equal(st["exp_avg"], m1[keep]) and torch.equal(st["exp_avg_sq"], m2[keep]) and st["step"] == step
    assert len(opt.state) == 6
    for t, o in zip((model.xyz_gradient_accum, model.denom, model.max_radii2D), stats):
        assert torch.equal(t, o[keep])
    for p in model.parameters():                                       # the optimizer steps the pruned tensors
        p.grad = torch.ones_like(p)
    opt.step()
    with pytest.raises(ValueError):
        model.prune_points(torch.zeros(P, dtype=torch.bool))           # the old length
    with pytest.raises(ValueError):
        model.prune_points(torch.zeros(P - 4, dtype=torch.int32))


def test_prune_points_without_an_optimizer():
    model = GaussianModel.from_raw(make_gaussians(10, 1, seed=3))
    xyz = model.get_xyz.detach().clone()
    assert model.prune_points(_mask(10, (1, 2))) == 2
    assert torch.equal(model.get_xyz.detach(), xyz[~_mask(10, (1, 2))])


def test_prune_unobserved_prunes_candidates_seen_too_rarely_and_resizes_the_window():
    model, opt = _live_model(P=8)
    w = KeyframeWindow(4)
    #                     row: 0  1  2  3  4  5  6  7
    w.add("a", torch.tensor([1, 1, 1, 1, 1, 0, 1, 0], dtype=torch.int32), overlap_cutoff=0.0)
    w.add("b", torch.tensor([1, 0, 1, 1, 1, 0, 0, 0], dtype=torch.int32), overlap_cutoff=0.0)
    cand = _mask(8, (3, 4, 5, 6, 7))
    assert prune_unobserved(model, w, cand, min_keyframes=3) == 0     # two keyframes cannot show three observations: nothing
    w.add("c", torch.tensor([1, 0, 0, 1, 0, 0, 1, 9], dtype=torch.int32), overlap_cutoff=0.0)
    # observations: [3, 1, 2, 3, 2, 0, 2, 1]; candidates below 3: rows 4, 5, 6, 7 (rows 1, 2 are no candidates)
    xyz = model.get_xyz.detach().clone()
    assert prune_unobserved(model, w, cand, min_keyframes=3) == 4
    assert torch.equal(model.get_xyz.detach(), xyz[:4])
    assert w.observations().tolist() == [3, 1, 2, 3]
    assert prune_unobserved(model, w, _mask(4, (3,)), min_keyframes=3) == 0
    with pytest.raises(ValueError):
        prune_unobserved(model, w, _mask(8, (3,)))


# ---- ctypes layout of gsr_render_extras ---------------------------------------------------------------------------------------
def test_render_extras_layout():
    from diff_gaussian_rasterization import _C
    ex = _C.gsr_render_extras(1, 0x1000, 0x2000)                       # the three positional values of existing callers
    assert ex.depth_kind == 1 and ex.out_alpha == 0x1000 and ex.dL_dalpha == 0x2000
    assert ex.n_touched is None and ex.touched_T_min == 0.0            # the new fields default to NULL / 0
    z = _C.gsr_render_extras()
    assert z.n_touched is None and z.touched_T_min == 0.0 and z.out_alpha is None
    names = [f[0] for f in _C.gsr_render_extras._fields_]
    assert names == ["depth_kind", "out_alpha", "dL_dalpha", "n_touched", "touched_T_min"]       # the new ones sit at the end
    E = _C.gsr_render_extras
    assert (E.depth_kind.offset, E.out_alpha.offset, E.dL_dalpha.offset) == (0, 8, 16)           # the old part did not move
    assert E.n_touched.offset == 24 and E.touched_T_min.offset == 32 and C.sizeof(E) == 40
    ex = E(0, None, None, 0x3000, 0.25)
    assert ex.n_touched == 0x3000 and ex.touched_T_min == 0.25
