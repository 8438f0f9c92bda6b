"""tests/compositing_reference.py against the float64 oracle, on the oracle's own records (no GPU): its images are the oracle's
render, its gradient records summed per Gaussian are the oracle's dL/dmean2D and dL/dopacity, no case leaves out more than 2 % of
its tiles, the stack cases have the properties tests/test_compositing_replay_gpu.py relies on, and the float32 replay's error
figures - from which that test's bounds are derived - are the constants it imports."""
import functools

import numpy as np
import pytest
import torch

import compositing_reference as CR
import tile_cull_reference as R

ORACLE_CASES = ["single_tile", "partial_tiles", "needles", "stop_64"]


@functools.lru_cache(maxsize=None)
def _yardstick(name):
    return CR.yardstick(name)


def _oracle_render(name, bg, gp, gd, gA):
    """The oracle's render of a case and its gradients under sum gp colour + gd depth + gA (1 - final_T), final_T taken from the
    difference of two composites (bg and black: colour_0 = C_0 + final_T bg_0)."""
    from oracle import gs_oracle as O
    from helpers import leaf_inputs, settings_for
    raw, cam, deg, W, H, _ = CR.case_scene(name)
    inp = leaf_inputs(raw, torch.float64, "cpu", "sh")
    s = settings_for(cam, deg, torch.from_numpy(bg.astype(np.float64)))
    pre = O.preprocess(inp["means3D"], inp["means2D"], inp["opacities"], s, shs=inp["shs"], scales=inp["scales"],
                       rotations=inp["rotations"])
    point_list, ranges, _ = O.bin_instances(pre, W, H)
    color, invd, fT, nc = O.composite(pre, point_list, ranges, s.bg, W, H)
    black, _, _, _ = O.composite(pre, point_list, ranges, torch.zeros(3, dtype=torch.float64), W, H)
    T = (color[0] - black[0]) / float(bg[0])
    loss = (color * torch.from_numpy(gp).double()).sum() + (invd[0] * torch.from_numpy(gd).double()).sum() \
        + ((1.0 - T) * torch.from_numpy(gA).double()).sum()
    loss.backward()
    return dict(color=color.detach().numpy(), invd=invd.detach().numpy()[0], fT=fT.numpy(), nc=nc.numpy(),
                d_means2D=inp["means2D"].grad.numpy(), d_opacity=inp["opacities"].grad.numpy().reshape(-1))


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_replay_is_the_oracle(name):
    """Published constants, the oracle's float64 records: images to 1e-12, and the records - summed per Gaussian, pushed through the
    moment-to-mean map - are the oracle's dL/dmean2D and dL/dopacity to 1e-10 of their largest magnitude."""
    raw, cam, deg, W, H, bg = CR.case_scene(name)
    bg = np.array([0.4, 0.25, 0.6], dtype=np.float32)                      # (every channel non-zero: final_T = difference / bg_0)
    rec, ranges, point_list, _ = CR.oracle_frame(raw, cam, deg, W, H)
    frame = CR.Frame(rec, ranges, point_list, bg, W, H)
    gp, gd, gA = CR.upstream(W, H)
    o = _oracle_render(name, bg, gp, gd, gA)
    ref = CR.forward_reference(frame, published=True)
    assert np.array_equal(ref["nc"].reshape(H, W), o["nc"])
    assert np.abs(ref["color"].reshape(3, H, W) - o["color"]).max() <= 1e-12
    assert np.abs(ref["depth"].reshape(H, W) - o["invd"]).max() <= 1e-12
    assert np.abs(ref["fT"].reshape(H, W) - o["fT"]).max() <= 1e-12
    assert np.abs(ref["alpha"].reshape(H, W) - (1.0 - o["fT"])).max() <= 1e-12
    # the depth plane's other form: the same sums with the depth itself as the record's value
    rec_z = CR.oracle_frame(raw, cam, deg, W, H, depth_z=True)[0]
    seen = np.unique(point_list)
    assert np.array_equal(rec_z[seen, 10], rec_z[seen, 11]) and np.array_equal(rec[seen, 10], 1.0 / rec[seen, 11])
    frame_z = CR.Frame(rec_z, ranges, point_list, bg, W, H)
    wz = CR.forward_reference(frame_z, published=True)["depth"]
    assert (wz[ref["nc"] > 0] > 0.2).all() and np.array_equal(wz == 0.0, ref["nc"] == 0)
    bref = CR.backward_reference(frame, ref["nc"], ref["fT"], (gp, gd, gA), published=True)
    recs = CR.records_in_list_order(frame, CR.natural_records(bref))
    gm, _, acc = CR.mean2d_from_records(frame, recs, CR.oracle_slots(frame), np.float64)
    for got, want in ((gm, o["d_means2D"][:, :2]), (acc[:, 5], o["d_opacity"])):
        assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max(), (name, np.abs(got - want).max(), np.abs(want).max())


@pytest.mark.parametrize("name", CR.all_case_names())
def test_left_out_cap_and_yardstick(name):
    """At most 2 % of a case's tiles are left out, in the forward and in either backward; the float32 replay's figures stay
    below the constants the bounds are derived from (and the largest of them IS the constant: test_yardstick_constants)."""
    fig, left, tiles = _yardstick(name)
    for stage, n in left.items():
        assert n <= CR.LEFT_OUT_CAP * tiles, (name, stage, n, tiles)
    for k, v in fig.items():
        assert v <= CR.YARDSTICK[k] * (1 + 1e-3), (name, k, v, CR.YARDSTICK[k])


def test_yardstick_constants():
    """Recomputed over all cases, the float32 replay's largest figures equal the constants (to their printed digits)."""
    worst = {k: max(_yardstick(n)[0][k] for n in CR.all_case_names()) for k in CR.CLASSES}
    for k in CR.CLASSES:
        assert abs(worst[k] - CR.YARDSTICK[k]) <= 1e-3 * CR.YARDSTICK[k], (k, worst[k], CR.YARDSTICK[k])
        assert CR.bounds(CR.YARDSTICK)[k] == max(2.0 ** -24, 4.0 * CR.YARDSTICK[k])


def _stack_frame(name):
    raw, cam, deg, W, H, bg = CR.case_scene(name)
    rec, ranges, point_list, _ = CR.oracle_frame(raw, cam, deg, W, H)
    frame = CR.Frame(rec, ranges, point_list, bg, W, H)
    ids, px, py, _ = frame.tile(0)
    return frame, ids, CR._geometry(rec, ids, px, py, np.float64)


@pytest.mark.parametrize("n", CR.STACK_A_SIZES)
def test_stack_a_never_saturates(n):
    """(a) one list of exactly n entries on one tile; every entry is blended by every pixel, alpha far from 1/255, no pixel
    stops: (1 - alpha)^513 > 1e-4 over the whole tile."""
    frame, ids, g = _stack_frame(f"stack_a_{n}")
    assert frame.tiles == 1 and len(ids) == n and g["ok"].all()
    assert g["alpha"].min() > 2.5 / 255.0 and g["alpha"].max() < 0.0125
    assert (1.0 - g["alpha"].max()) ** 513 > 1.0e-4
    ref = CR.forward_reference(frame)
    assert (ref["nc"] == n).all() and ref["doubt"][0] == 0 and ref["fT"].min() > 1.0e-4


@pytest.mark.parametrize("name", list(CR.STACK_B))
def test_stack_b_stops_straddle_the_batch_end(name):
    """(b) the pixels of the tile stop on both sides of entry k = 64, 128, 256: some at k - 1 or before, some at k + 1 or later."""
    k = CR.STACK_B[name]["k"]
    frame, ids, _ = _stack_frame(name)
    _, _, stop_at = R.composite_tile(frame.rec, ids, 0, 0, 16, 16)
    assert len(ids) == CR.STACK_B[name]["n"] and stop_at.min() >= 1
    assert stop_at.min() <= k - 1 and stop_at.max() >= k + 1 and stop_at.max() < len(ids), (stop_at.min(), stop_at.max())
    ref = CR.forward_reference(frame)
    assert ref["nc"].min() <= k - 2 and ref["nc"].max() >= k
