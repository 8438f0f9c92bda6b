"""Plain numpy statements (uint64 arithmetic) of the binning stage's integer building blocks - the prefix sum, the stable
tile sort with its encoded tile ranges, the per-tile depth ordering - for bit-exact comparison with the HIP kernels
(sort_scan.hip, binning.hip).  tests/test_binning_reference_cpu.py holds each of them to a brute-force loop."""
import numpy as np

PAD_ID = 0xFFFFFFFF          # padding entry of a tile list: ordered as depth key 0xFFFFFFFF, whatever depth_key holds
M32 = np.uint64(0xFFFFFFFF)


def scan_u32(src, idx=None, inclusive=False):
    """out[i] = sum over j < i (inclusive: j <= i) of src[idx[j]] (idx None: src[j]), modulo 2^32.  -> uint32 [n]"""
    v = np.asarray(src, dtype=np.uint32)
    if idx is not None:
        v = v[np.asarray(idx).astype(np.int64)]
    v = v.astype(np.uint64)
    c = np.cumsum(v, dtype=np.uint64)          # (below 2^56 for any array that fits in memory: no uint64 wrap)
    if not inclusive:
        c = c - v
    return (c & M32).astype(np.uint32)


def stable_order(keys, bits):
    """Permutation that sorts `keys` by their low `bits` bits, equal keys keeping their input order.  -> int64 [n]"""
    k = np.asarray(keys, dtype=np.uint32).astype(np.uint64) & np.uint64((1 << bits) - 1)
    # (a 16-bit view takes numpy's radix sort: the same stable order, much faster on millions of keys)
    return np.argsort(k.astype(np.uint16) if bits <= 16 else k, kind="stable")


def stable_sort_pairs(keys, bits, *payloads):
    """-> (sorted low-bits keys uint32, [payload[order] ...], order)"""
    order = stable_order(keys, bits)
    k = (np.asarray(keys, dtype=np.uint32).astype(np.uint64) & np.uint64((1 << bits) - 1)).astype(np.uint32)
    return k[order], [np.asarray(p)[order] for p in payloads], order


def encoded_ranges_sparse(sorted_keys):
    """The tiles that occur in `sorted_keys`, ascending, and for each (~first, last + 1) of its run of sorted positions.
    -> (tiles int64 [m], pairs uint32 [m, 2])"""
    k = np.asarray(sorted_keys, dtype=np.uint32).astype(np.int64)
    if k.size == 0:
        return np.zeros(0, dtype=np.int64), np.zeros((0, 2), dtype=np.uint32)
    present, first, count = np.unique(k, return_index=True, return_counts=True)
    first = first.astype(np.uint64)
    last = first + count.astype(np.uint64) - np.uint64(1)
    pairs = np.stack([(~first) & M32, (last + np.uint64(1)) & M32], axis=1).astype(np.uint32)
    return present, pairs


def encoded_ranges(sorted_keys, tiles):
    """What the tile sort's last pass leaves per tile t < tiles: (~first, last + 1) of t's run of sorted positions, (0, 0)
    where t does not occur.  -> uint32 [tiles, 2]"""
    present, pairs = encoded_ranges_sparse(sorted_keys)
    out = np.zeros((tiles, 2), dtype=np.uint32)
    out[present] = pairs
    return out


def decode_ranges(enc):
    """(~first, last + 1) -> [start, end); (0, 0) stays (0, 0).  -> uint32 [tiles, 2]"""
    enc = np.asarray(enc, dtype=np.uint32)
    out = enc.copy()
    out[:, 0] = np.where(enc[:, 1] != 0, ~enc[:, 0], 0).astype(np.uint32)
    return out


def tile_depth_order(ranges, point_list, depth_key, slot_of_pos=None):
    """Every tile's list point_list[start:end] ordered by (depth_key[id] - 0xFFFFFFFF for id 0xFFFFFFFF -, input position);
    slot_of_pos permuted along.  Positions outside every range keep their contents.  The ranges must not overlap.
    -> (point_list, slot_of_pos or None), new arrays"""
    ranges = np.asarray(ranges, dtype=np.uint32).astype(np.int64)
    pl = np.asarray(point_list, dtype=np.uint32)
    dk = np.asarray(depth_key, dtype=np.uint32)
    n = ranges[:, 1] - ranges[:, 0]
    tile = np.repeat(np.arange(ranges.shape[0], dtype=np.int64), n)
    start = np.repeat(ranges[:, 0], n)
    first = np.cumsum(n) - n
    pos = start + (np.arange(tile.size, dtype=np.int64) - np.repeat(first, n))       # list positions, tile by tile
    assert np.unique(pos).size == pos.size, "overlapping ranges"
    ids = pl[pos]
    key = np.where(ids == PAD_ID, np.uint32(PAD_ID), dk[np.where(ids == PAD_ID, 0, ids).astype(np.int64)]).astype(np.uint64)
    comp = (tile.astype(np.uint64) << np.uint64(32)) | key
    order = np.argsort(comp, kind="stable")        # stable + positions ascending inside a tile: ties keep the input order
    out_pl = pl.copy()
    out_pl[pos] = ids[order]
    out_slot = None
    if slot_of_pos is not None:
        sl = np.asarray(slot_of_pos, dtype=np.uint32)
        out_slot = sl.copy()
        out_slot[pos] = sl[pos][order]
    return out_pl, out_slot
