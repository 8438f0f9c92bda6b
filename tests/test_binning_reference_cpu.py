"""tests/binning_reference.py (the numpy references the GPU tests of the scan, the tile sort and the per-tile depth ordering
compare against) held to brute-force Python loops on a few dozen elements."""
import numpy as np
import pytest

import binning_reference as BR


@pytest.mark.parametrize("inclusive", [False, True])
@pytest.mark.parametrize("gather", [False, True])
def test_scan_reference_matches_a_loop(inclusive, gather):
    rng = np.random.default_rng(11 + 2 * inclusive + gather)
    n = 37
    src = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)      # (the total passes 2^32 several times)
    idx = rng.permutation(n).astype(np.uint32) if gather else None
    want, run = [], 0
    for i in range(n):
        v = int(src[int(idx[i])] if gather else src[i])
        if inclusive:
            run = (run + v) % (1 << 32)
            want.append(run)
        else:
            want.append(run)
            run = (run + v) % (1 << 32)
    got = BR.scan_u32(src, idx, inclusive)
    assert got.dtype == np.uint32 and got.tolist() == want
    assert max(want) > 0 and sum(int(x) for x in src) > (1 << 32)
    assert BR.scan_u32(np.zeros(0, dtype=np.uint32)).size == 0


@pytest.mark.parametrize("bits", [1, 3, 9, 17, 24])
def test_stable_sort_reference_matches_an_insertion_sort(bits):
    rng = np.random.default_rng(bits)
    n = 48
    keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    keys[::3] = keys[1]                                                      # ties
    v, w = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32), np.arange(n, dtype=np.uint32) * 7 + 3
    mask = (1 << bits) - 1
    rows = []                                                                # stable insertion sort by the low bits
    for i in range(n):
        k = int(keys[i]) & mask
        j = len(rows)
        while j > 0 and rows[j - 1][0] > k:
            j -= 1
        rows.insert(j, (k, int(v[i]), int(w[i]), i))
    ks, (vs, ws), order = BR.stable_sort_pairs(keys, bits, v, w)
    assert ks.tolist() == [r[0] for r in rows] and vs.tolist() == [r[1] for r in rows] and ws.tolist() == [r[2] for r in rows]
    assert order.tolist() == [r[3] for r in rows]


def test_encoded_ranges_reference_matches_a_loop():
    rng = np.random.default_rng(5)
    tiles = 32
    keys = np.sort(rng.choice(np.array([0, 3, 4, 17, 31]), 40)).astype(np.uint32)
    want = [[0, 0] for _ in range(tiles)]
    for t in range(tiles):
        hits = [i for i in range(keys.size) if int(keys[i]) == t]
        if hits:
            want[t] = [(~hits[0]) & 0xFFFFFFFF, hits[-1] + 1]
    enc = BR.encoded_ranges(keys, tiles)
    assert enc.dtype == np.uint32 and enc.tolist() == want
    assert int(enc[0, 0]) == 0xFFFFFFFF                                      # tile 0 starts at position 0
    dec = BR.decode_ranges(enc)
    for t in range(tiles):
        hits = [i for i in range(keys.size) if int(keys[i]) == t]
        assert dec[t].tolist() == ([hits[0], hits[-1] + 1] if hits else [0, 0])
    assert not BR.encoded_ranges(np.zeros(0, dtype=np.uint32), 4).any()


@pytest.mark.parametrize("dual", [False, True])
def test_tile_depth_order_reference_matches_a_loop(dual):
    rng = np.random.default_rng(9 + dual)
    P = 20
    depth = rng.integers(0, 4, P, dtype=np.uint64).astype(np.uint32) * np.uint32(0x01000001)      # heavy ties
    lens = [0, 1, 5, 0, 12, 2, 9]
    pl, ranges, at = [], [], 3
    pl += [777] * at                                                         # words in front of, between and behind the lists
    for n in lens:
        ids = rng.permutation(P)[:n].tolist()
        if n >= 9:
            ids[2] = BR.PAD_ID
            ids[7] = BR.PAD_ID
        ranges.append([at, at + n])
        pl += ids + [888]
        at += n + 1
    pl = np.array(pl, dtype=np.uint32)
    slots = rng.integers(0, 1 << 32, pl.size, dtype=np.uint64).astype(np.uint32)
    want_pl, want_sl = pl.copy(), slots.copy()
    for s, e in ranges:
        rows = sorted(range(s, e), key=lambda p: (0xFFFFFFFF if int(pl[p]) == BR.PAD_ID else int(depth[int(pl[p])]), p))
        for i, p in enumerate(rows):
            want_pl[s + i], want_sl[s + i] = pl[p], slots[p]
    got_pl, got_sl = BR.tile_depth_order(np.array(ranges, dtype=np.uint32), pl, depth, slots if dual else None)
    assert got_pl.tolist() == want_pl.tolist()
    assert (got_sl is None) if not dual else (got_sl.tolist() == want_sl.tolist())
    assert (got_pl != pl).any()
