"""tests/tile_cull_reference.py on its own (no GPU): the `need` of hand-built tiles worked out on paper, the cut-off rule from
`need`, the ambiguity test, and - on the oracle's float64 records and lists - that every seeded case of the GPU test leaves out
at most 2 % of its tiles."""
import numpy as np
import pytest

import tile_cull_reference as R


def _flat_stack(n, opacity, conic=0.0, centre=8.0):
    rec = np.zeros((n, 12))
    rec[:, 0] = rec[:, 1] = centre
    rec[:, 2] = rec[:, 4] = conic
    rec[:, 5] = opacity
    return rec


def test_need_of_a_hand_built_tile():
    """Identical splats of alpha = 0.8 at the centre pixel: T = 0.2^j after j blends, test_T of entry 6 is 0.2^6 = 6.4e-5 < 1e-4
    while entry 5 leaves 3.2e-4: the pixel stops at entry 6.  Flat splats (conic 0): every pixel does.  With A' = C' = -1/128 the
    corner pixel (0, 0), 128 squared pixels from the mean, sees alpha = 0.8 / 2 = 0.4: 0.6^18 = 1.0156e-4, 0.6^19 = 6.09e-5, it
    stops at entry 19 and no pixel lies farther out."""
    ids = np.arange(30)
    need, amb, stop_at = R.composite_tile(_flat_stack(30, 0.8), ids, 0, 0, 16, 16)
    assert need == 6 and not amb and (stop_at == 6).all()
    need, amb, stop_at = R.composite_tile(_flat_stack(30, 0.8, -1.0 / 128.0), ids, 0, 0, 16, 16)
    assert stop_at.reshape(16, 16)[8, 8] == 6 and stop_at.reshape(16, 16)[0, 0] == 19
    assert need == 19 and not amb
    # a list that ends before the corner pixel saturates: all ones; and pixels outside the image add nothing (9 x 9 image: the
    # farthest inside pixel is (0, 0) still; 12 x 12 with the tile at the origin cut to the pixels near the mean: need 6)
    need, amb, _ = R.composite_tile(_flat_stack(18, 0.8, -1.0 / 128.0), ids[:18], 0, 0, 16, 16)
    assert need == R.ALL and not amb
    need, _, stop_at = R.composite_tile(_flat_stack(30, 0.8, -1.0 / 128.0, centre=8.0), ids, 0, 0, 9, 9)
    assert need == 19 and stop_at.size == 81
    # padding slots count as list positions and are never blended
    pad = np.array([0, R.NO_ID, 1, 2, R.NO_ID, 3, 4, 5, 6, 7])
    need, amb, _ = R.composite_tile(_flat_stack(30, 0.8), pad, 0, 0, 16, 16)
    assert need == 8 and not amb
    assert R.composite_tile(_flat_stack(30, 0.8), ids[:0], 0, 0, 16, 16)[0] == R.ALL


def test_skip_rules():
    """alpha < 1/255 and power > 0 are skipped; alpha is capped at 0.99 (two entries of opacity 1 leave T = 1e-4, not < 1e-4:
    the pixel stops at the third)."""
    rec = _flat_stack(6, 1.0)
    assert R.composite_tile(rec, np.arange(6), 0, 0, 16, 16)[0] == 3
    rec = _flat_stack(12, 0.8)
    rec[1, 5] = 0.9 / 255.0            # skipped: costs a position, blends nothing
    rec[3, 2] = rec[3, 4] = 1.0        # power > 0 away from the mean, 0 at it
    need, amb, stop_at = R.composite_tile(rec, np.arange(12), 0, 0, 16, 16)
    assert stop_at.reshape(16, 16)[8, 8] == 7 and stop_at.reshape(16, 16)[3, 3] == 8 and need == 8 and not amb


def test_doubt_is_followed_through_to_need():
    """A doubtful comparison makes a tile ambiguous only where it can move the tile's maximum."""
    ids = np.arange(30)
    # entry 2 sits on the 1/255 threshold: blended or not, the sixth 0.8-splat (entry 7) stops the pixel -> not ambiguous
    rec = _flat_stack(30, 0.8)
    rec[1, 5] = (1.0 + 0.5 * R.BAND) / 255.0
    need, amb, _ = R.composite_tile(rec, ids, 0, 0, 16, 16)
    assert need == 7 and not amb       # (T changes by 0.4 %: 0.2^5 (1 - 1/255) = 3.19e-4 stays above 1e-4 either way)
    # ... but right at a stop it decides: five blends of 0.8 and one of alpha* leave 1e-4 x (1 +- 1e-5)
    for sign, want in ((-1.0, 6), (1.0, 7)):
        rec = _flat_stack(30, 0.8)
        rec[5, 5] = 1.0 - (1.0e-4 * (1.0 + sign * 1.0e-5)) / 0.2 ** 5
        need, amb, _ = R.composite_tile(rec, ids, 0, 0, 16, 16)
        assert need == want and amb
    # a doubtful skip test behind the pixel's stop is never looked at
    rec = _flat_stack(30, 0.8)
    rec[9, 5] = 1.0 / 255.0
    assert R.composite_tile(rec, ids, 0, 0, 16, 16)[1] is False


def test_cutoff_from_need():
    """k = ((need q8) >> 8) + add; the key at 0-based index k, all ones from k == len on."""
    W = H = 16
    keys = (1000 + 10 * np.arange(400)).astype(np.uint32)
    for n, q8, add, want_k in ((200, 448, 48, 58), (59, 448, 48, 58), (58, 448, 48, 58), (30, 256, 3, 9), (10, 256, 3, 9),
                               (9, 256, 3, 9), (30, 300, 0, 7)):
        e = R.expected_cutoffs(_flat_stack(400, 0.8), np.array([[0, n]]), np.arange(n), keys, W, H, q8, add)
        assert e["need"][0] == 6 and e["k"][0] == want_k and e["len"][0] == n
        assert e["cutoff"][0] == (keys[want_k] if want_k < n else R.ALL), (n, q8, add)
    e = R.expected_cutoffs(_flat_stack(400, 0.8), np.array([[0, 5]]), np.arange(5), keys, W, H)
    assert e["need"][0] == R.ALL and e["k"][0] == -1 and e["cutoff"][0] == R.ALL


@pytest.mark.parametrize("name", list(R.CASES))
def test_seeded_cases_leave_out_at_most_two_percent(name):
    raw, cam, deg, W, H = R.case_scene(name)
    rec, ranges, point_list, keys = R.oracle_frame(raw, cam, deg, W, H)
    e = R.expected_cutoffs(rec, ranges, point_list, keys, W, H)
    tiles = len(e["need"])
    assert tiles == np.prod(R.tile_grid(W, H))
    print(f"\n{name}: tiles {tiles}, ambiguous {int(e['ambiguous'].sum())}, finite {int((e['cutoff'] != R.ALL).sum())}")
    assert e["ambiguous"].sum() <= R.AMBIGUOUS_CAP * tiles
    if name == "saturating":
        assert ((e["cutoff"] != R.ALL) & ~e["ambiguous"]).sum() >= tiles // 2
    if name == "three":
        assert (e["len"] <= 3).all() and (e["cutoff"] == R.ALL).all()


def test_the_boundary_stack_is_unambiguous_on_the_oracle():
    raw, cam, deg, W, H = R.stack_scene(24)
    rec, ranges, point_list, keys = R.oracle_frame(raw, cam, deg, W, H)
    e = R.expected_cutoffs(rec, ranges, point_list, keys, W, H, 256, 3)
    assert not e["ambiguous"][0] and e["len"][0] == 24 and 9 <= e["k"][0] < 23
    assert (np.diff(keys.astype(np.int64)) > 0).all()          # depth-ordered, no equal keys
