"""gsr_feature_nn and match_features on the device (csrc/features.hip) against the float64 brute force of
tests/global_registration_reference.py.

Bounds.  The device's distance is 33 float32 differences and fused multiply-adds: its relative error against float64 is below
34 x 2^-24 = 2e-6 in the worst case and a few 1e-7 in practice; the issue's bar is 1e-6 relative, for dist2 itself and for the
float64 distance of the returned row against the brute-force minimum.  The row itself is compared where the reference's best and
second best are more than 1e-5 relative apart (test_global_registration_cpu.py shows that this is every row of the mutual case)."""
import numpy as np
import pytest
import torch

import global_registration_reference as G
import scene_utils as S

pytestmark = pytest.mark.gpu
TILE = 128              # GSR_FEATURE_NN_TILE: target rows per LDS tile
WORKGROUPS = 512        # GSR_FEATURE_NN_WORKGROUPS: the target range is split until the grid has that many
REL = 1e-6


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def tiles_per_split(Nq, Nt):
    """the library's rule, restated"""
    qblk, ntiles = -(-Nq // 256), -(-Nt // TILE)
    splits = min(-(-WORKGROUPS // qblk), ntiles, 65535)
    return -(-ntiles // splits)


def check(q, t, label):
    idx, d2 = (x.cpu().numpy() for x in S.feature_nn(dev(q), dev(t)))
    ref = G.feature_nn(q, t)
    has = ref["idx"] >= 0
    assert np.array_equal(idx >= 0, has), label
    assert np.isnan(d2[np.isnan(ref["d2"])]).all() and (d2[~has & ~np.isnan(ref["d2"])] == np.inf).all(), label
    own = ((q[has].astype(np.float64) - t[idx[has]].astype(np.float64)) ** 2).sum(axis=1)
    best = ref["d2"][has]
    scale = np.maximum(best, 1e-300)
    e_row, e_d2 = (np.abs(own - best) / scale).max(initial=0.0), (np.abs(d2[has].astype(np.float64) - best) / scale).max(initial=0.0)
    print(f"{label}: rows {int(has.sum())}, returned row off the minimum by {e_row:.3g}, dist2 by {e_d2:.3g}")
    assert e_row <= REL and e_d2 <= REL, (label, e_row, e_d2)
    with np.errstate(invalid="ignore", divide="ignore"):
        clear = has & ((ref["second"] - ref["d2"]) / ref["second"] > 1e-5)
    assert np.array_equal(idx[clear], ref["idx"][clear]), label
    return idx, d2


def run_boundaries(Nq, runs):
    """Nt one below / at / one above the end of run number `runs` of the grid split, and one row beyond two further runs - with the
    run length the library uses AT that Nt (it is recomputed per call): None where the queries alone fill the grid"""
    for ntiles in range(2, 4096):
        if tiles_per_split(Nq, ntiles * TILE) >= 2:
            tps = tiles_per_split(Nq, ntiles * TILE)
            end = max(runs, -(-ntiles // tps)) * tps * TILE      # a whole number of runs, at least as many tiles as found
            sizes = [end - 1, end, end + 1, end + 2 * tps * TILE + 1]
            return [Nt for Nt in sizes if tiles_per_split(Nq, Nt) == tps], tps
    return [], 1


@pytest.mark.parametrize("Nq", [1, 63, 64, 65, 257, 5000])
def test_matching_against_brute_force(Nq):
    from diff_gaussian_rasterization import _C
    lib = _C.lib()
    q = G.features(Nq, 10 + Nq)
    # the LDS tile: one below / at / one above (runs of one tile: every tile is a split of its own); beyond two splits: 257
    sizes = [1, 2, 5000, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]
    # runs of SEVERAL tiles exist where the tiles outnumber the splits: from 27 tiles on at Nq = 5000 (20 query blocks, 26 splits)
    # and from 513 tiles on at Nq = 1; in between (one or two query blocks) likewise, but a float64 brute force of 65 or 257
    # queries against 65 537 targets is left to the two ends
    long_runs, tps = run_boundaries(Nq, 20) if Nq in (1, 5000) else ([], 1)
    assert (Nq not in (1, 5000)) or (tps >= 2 and len(long_runs) >= 3), (Nq, tps, long_runs)
    for Nt in sorted(set(sizes + long_runs)):
        assert lib.gsr_feature_nn_tiles_per_split(Nq, Nt) == tiles_per_split(Nq, Nt)
        check(q, G.features(Nt, 1000 + Nt), f"Nq={Nq} Nt={Nt} (runs of {tiles_per_split(Nq, Nt)} tiles)")


def test_identical_rows_nan_rows_and_repeat_runs():
    q = G.features(300, 1)
    t = G.features(700, 2)
    t[[5, 300, 699]] = q[17]                  # three copies of one query: the smallest row wins, at distance 0
    t[[131, 400]] = q[200]                    # two copies in different tiles
    t[3, 7] = np.nan                          # a NaN target row never wins
    t[4] = q[17]
    t[4, 0] = np.nan
    q[9, 32] = np.nan                         # a NaN query: -1 / NaN
    idx, d2 = check(q, t, "ties and NaN")
    assert idx[17] == 5 and d2[17] == 0 and idx[200] == 131 and d2[200] == 0 and idx[9] == -1 and np.isnan(d2[9])
    assert not np.isin(idx, [3, 4]).any()
    a = S.feature_nn(dev(q), dev(t))
    b = S.feature_nn(dev(q), dev(t))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    none = np.full((3, 33), np.nan, dtype=np.float32)
    idx, d2 = (x.cpu().numpy() for x in S.feature_nn(dev(q[:20]), dev(none)))
    assert (idx == -1).all() and np.isnan(d2[9]) and (np.delete(d2, 9) == np.inf).all()


def test_no_bit_depends_on_how_the_target_range_is_split():
    # the same targets searched by 1 query block (many splits) and, inside 5000 queries, by 20 blocks (runs of two tiles)
    t = dev(G.features(5000, 7, copies=400))
    q = G.features(5000, 8)
    whole = S.feature_nn(dev(q), t)
    for lo, hi in ((0, 1), (100, 165), (4743, 5000)):
        part = S.feature_nn(dev(q[lo:hi]), t)
        assert torch.equal(part[0], whole[0][lo:hi]) and torch.equal(part[1].view(torch.int32), whole[1][lo:hi].view(torch.int32))


@pytest.mark.parametrize("n,m,seed", [(5000, 5000, 1), (257, 129, 2)])
def test_mutual_filter_equals_the_reference_set(n, m, seed):
    a, b = G.features(n, seed), G.features(m, seed + 100)
    for mutual in (False, True):
        got = S.match_features(dev(a), dev(b), mutual).cpu().numpy()
        assert got.dtype == np.int32 and np.array_equal(got, G.match(a, b, mutual)), mutual
        assert (np.diff(got[:, 0]) > 0).all()
