"""The tile-local binning's per-tile ordering (k_tile_depth_sort, binning.hip) through its test hook, bit-exact against numpy
(tests/binning_reference.py).  One call orders many synthetic tiles, list lengths at every edge of the kernel: 1 / 2 (nothing to
do), 1024 / 1025 (the first launch against the `_long` launch), 2048 / 2049 (from where meta[4] reports the longest list),
4096 / 4097 (stable LSD radix sort in LDS against the bitonic network in memory with virtual padding); depth keys that make
passes skip, that make every pass skip, that tie heavily; padding ids; the second payload; encoded ranges decoded on the way."""
import numpy as np
import pytest
import torch

import binning_reference as BR

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 5000, 8192, 8193]
P = 20_000                   # Gaussians the lists draw their ids from
GUARD = 64                   # words in front of and behind [0, R) of every buffer
PATTERN = 0x3C3CC3C3
GARBAGE = 0x7EADBEEF
KEY_PATTERNS = ("random32", "low20", "all_equal", "all_equal_pads", "top_byte", "eight_values")


def _layout(lengths, seed, pads=True):
    """Lists back to back in point_list, an empty tile after every second list; pads: three padding ids in every list of 64
    entries or more.  -> (ranges uint32 [tiles, 2], point_list uint32 [R])"""
    rng = np.random.default_rng(seed)
    ranges, lists, at = [], [], 0
    for i, n in enumerate(lengths):
        ids = rng.permutation(P)[:n].astype(np.uint32)           # distinct ids, in no particular order
        if pads and n >= 64:
            ids[rng.choice(n, 3, replace=False)] = BR.PAD_ID
        ranges.append((at, at + n))
        lists.append(ids)
        at += n
        if i % 2 == 1:
            ranges.append((at, at))
    return np.array(ranges, dtype=np.uint32), np.concatenate(lists)


def _depth_keys(pattern, seed):
    rng = np.random.default_rng(seed)
    if pattern == "random32":
        k = rng.integers(0, 1 << 32, P, dtype=np.uint64)
    elif pattern == "low20":                                     # a common top: the two upper passes are skipped
        k = rng.integers(0, 1 << 20, P, dtype=np.uint64) | 0x40300000
    elif pattern in ("all_equal", "all_equal_pads"):             # without padding ids no pass runs: the order must stay
        k = np.full(P, 0x3F800000, dtype=np.uint64)
    elif pattern == "top_byte":
        k = (rng.integers(0, 256, P, dtype=np.uint64) << 24) | 0x00123456
    elif pattern == "eight_values":                              # heavy ties -> input order
        k = rng.integers(0, 8, P, dtype=np.uint64) * 0x01010101 + 0x3F000000
    else:
        raise ValueError(pattern)
    return k.astype(np.uint32)


def _guarded(a, dev="cuda"):
    """Device buffer [GUARD | a | GUARD] as int32, and the view of its middle."""
    buf = torch.full((a.size + 2 * GUARD,), PATTERN, dtype=torch.int32, device=dev)
    mid = buf[GUARD:GUARD + a.size]
    mid.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)))
    return buf, mid


def _guards_ok(buf, n):
    return bool((buf[:GUARD] == PATTERN).all()) and bool((buf[GUARD + n:] == PATTERN).all())


def _run(lengths, pattern, dual, encoded, seed):
    from diff_gaussian_rasterization import _C
    lib = _C.lib()
    ranges, pl = _layout(lengths, seed, pads=pattern != "all_equal")      # (a padding id is a second key value)
    tiles, R = ranges.shape[0], pl.size
    depth = _depth_keys(pattern, seed + 1)
    slots = np.random.default_rng(seed + 2).integers(0, 1 << 32, R, dtype=np.uint64).astype(np.uint32)
    want_pl, want_sl = BR.tile_depth_order(ranges, pl, depth, slots)
    dev = "cuda"
    pl_buf, pl_d = _guarded(pl)
    sl_buf, sl_d = _guarded(slots)
    free = [_guarded(np.full(R, GARBAGE, dtype=np.uint32)) for _ in range(3)]
    dk_buf, dk_d = _guarded(depth)
    meta = torch.zeros(8, dtype=torch.int32, device=dev)
    if encoded:      # ranges as the tile sort's last pass leaves them; `ranges` itself arrives as garbage and leaves decoded
        n = ranges[:, 1].astype(np.int64) - ranges[:, 0]
        enc = np.zeros_like(ranges)
        enc[n > 0, 0] = ~ranges[n > 0, 0]
        enc[n > 0, 1] = ranges[n > 0, 1]
        assert (BR.decode_ranges(enc)[n > 0] == ranges[n > 0]).all()
        want_rg = np.where((n > 0)[:, None], ranges, 0).astype(np.uint32)
        enc_buf, enc_d = _guarded(enc.reshape(-1))
        rg_buf, rg_d = _guarded(np.full(2 * tiles, GARBAGE, dtype=np.uint32))
    else:
        want_rg = ranges
        enc_buf = enc_d = None
        rg_buf, rg_d = _guarded(ranges.reshape(-1))
    _C.check(lib.gsr_debug_tile_depth_sort(tiles, 1 if dual else 0, _C.ptr(rg_d), _C.ptr(enc_d), _C.ptr(pl_d),
                                           _C.ptr(sl_d) if dual else None, _C.ptr(dk_d), _C.ptr(free[0][1]), _C.ptr(free[1][1]),
                                           _C.ptr(free[2][1]), _C.ptr(meta), _C._stream()))
    torch.cuda.synchronize()
    u32 = lambda t: t.cpu().numpy().view(np.uint32)
    got_pl, got_sl, got_rg = u32(pl_d), u32(sl_d), u32(rg_d).reshape(tiles, 2)
    what = (pattern, dual, encoded)
    for t, (s, e) in enumerate(ranges.astype(np.int64)):         # per tile, so that a failure names the list length
        assert (got_pl[s:e] == want_pl[s:e]).all(), what + ("point_list", int(e - s))
        assert (got_sl[s:e] == (want_sl if dual else slots)[s:e]).all(), what + ("slot_of_pos", int(e - s))
    assert (got_rg == want_rg).all(), what
    assert _guards_ok(pl_buf, R) and _guards_ok(sl_buf, R) and _guards_ok(rg_buf, 2 * tiles) and _guards_ok(dk_buf, P), what
    assert all(_guards_ok(b, R) for b, _ in free), what
    assert enc_buf is None or (_guards_ok(enc_buf, 2 * tiles) and (u32(enc_d).reshape(tiles, 2) == enc).all()), what
    assert (u32(dk_d) == depth).all(), what
    longest = max(lengths)
    m = u32(meta)
    assert int(m[4]) == (longest if longest > 2048 else 0) and not m[[0, 1, 2, 3, 5, 6, 7]].any(), (what, m.tolist())
    return got_pl, pl


@pytest.mark.parametrize("encoded", [False, True])
@pytest.mark.parametrize("dual", [False, True])
@pytest.mark.parametrize("pattern", KEY_PATTERNS)
def test_tile_depth_sort_matches_reference_at_every_list_length(pattern, dual, encoded):
    got_pl, pl = _run(LENGTHS, pattern, dual, encoded, seed=7 + KEY_PATTERNS.index(pattern))
    if pattern == "all_equal":
        assert (got_pl == pl).all()                              # equal keys everywhere: every list keeps its order


@pytest.mark.parametrize("longest", [2048, 2049])
def test_tile_depth_sort_reports_only_lists_beyond_2048(longest):
    """meta[4] stays 0 while no list passes 2048 entries (asserted in _run), and holds the longest list from 2049 on."""
    _run([n for n in LENGTHS if n <= longest], "low20", True, True, seed=40 + longest)
