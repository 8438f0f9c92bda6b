"""The library's stable LSD radix sort (one kernel per pass: ticketed chunks + decoupled look-back, sort_scan.hip) through the
C ABI test hook, bit-exact against numpy's stable argsort: sizes around the chunk boundaries, every pass count, the dual
payload, a device-side count smaller than the capacity, a uniform digit (identity-pass shortcut), heavy duplicates.

The form the tile-local binning runs (gsr_debug_tile_sort: histograms counted ahead and summed over their replicas, every pass
clearing the next one's look-back table, the last pass leaving encoded tile ranges instead of keys) has tests of its own below:
one to three passes, tile runs that span chunks, every key in one tile (each pass an identity pass), the switch from 2048- to
4096-key chunks at 2^21 keys."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _sort(keys, bits, dual=False, n_dev=None, vals=None):
    from diff_gaussian_rasterization import _C
    lib = _C.lib()
    n = keys.numel()
    dev = "cuda"
    k0 = keys.to(dev).contiguous()
    k1 = torch.empty_like(k0)
    v0 = torch.empty(n, dtype=torch.int32, device=dev) if vals is None else vals.to(dev).contiguous()
    v1 = torch.empty(n, dtype=torch.int32, device=dev)
    w0 = (torch.arange(n, dtype=torch.int32, device=dev) * 7 + 3) if dual else None
    w1 = torch.empty(n, dtype=torch.int32, device=dev) if dual else None
    tmp = torch.empty(lib.gsr_debug_radix_tmp_bytes(n), dtype=torch.uint8, device=dev)
    nd = None
    if n_dev is not None:
        nd = torch.tensor([n_dev, 0], dtype=torch.int32, device=dev)
    where = _C.check(lib.gsr_debug_radix_sort(_C.ptr(k0), _C.ptr(v0), _C.ptr(k1), _C.ptr(v1), _C.ptr(w0), _C.ptr(w1), n, bits,
                                              1 if vals is None else 0, _C.ptr(nd), _C.ptr(tmp), _C._stream()))
    torch.cuda.synchronize()
    ks, vs, ws = (k1, v1, w1) if where else (k0, v0, w0)
    return ks.cpu().numpy().view(np.uint32), vs.cpu().numpy().view(np.uint32), None if ws is None else ws.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("n,bits", [(1, 32), (63, 8), (2047, 13), (2048, 13), (2049, 16), (4096, 32), (40_001, 24),
                                    (300_000, 32), (2_200_000, 13), (3_000_001, 15),
                                    (2_097_151, 13), (2_097_152, 13), (2_097_153, 13)])     # 2048- / 4096-key chunks
def test_radix_sort_matches_numpy_stable_sort(n, bits):
    rng = np.random.default_rng(n + bits)
    kn = rng.integers(0, 1 << bits, n, dtype=np.uint64).astype(np.uint32)
    keys = torch.from_numpy(kn.view(np.int32).copy())
    order = np.argsort(kn, kind="stable")
    ks, vs, ws = _sort(keys, bits, dual=(n % 2 == 1))
    assert (ks == kn[order]).all() and (vs == order.astype(np.uint32)).all()
    if ws is not None:
        assert (ws == (order.astype(np.uint32) * 7 + 3)).all()


def test_radix_sort_duplicates_uniform_digit_and_device_count():
    gen = torch.Generator().manual_seed(5)
    n = 123_457
    # (a) every key has the same top byte (identity-pass shortcut) and few distinct values overall
    keys = (torch.randint(0, 37, (n,), generator=gen, dtype=torch.int64) * 4099 + 0x40000000).to(torch.int32)
    kn = keys.numpy().view(np.uint32)
    order = np.argsort(kn, kind="stable")
    ks, vs, _ = _sort(keys, 32)
    assert (ks == kn[order]).all() and (vs == order.astype(np.uint32)).all()
    # (b) given values instead of the index, and a device-side count below the capacity: only the first m keys are sorted
    vals = torch.randint(0, 2**31 - 1, (n,), generator=gen, dtype=torch.int64).to(torch.int32)
    m = 77_777
    ks, vs, ws = _sort(keys, 32, dual=True, n_dev=m, vals=vals)
    order_m = np.argsort(kn[:m], kind="stable")
    assert (ks[:m] == kn[:m][order_m]).all() and (vs[:m] == vals.numpy().view(np.uint32)[:m][order_m]).all()
    assert (ws[:m] == (order_m.astype(np.uint32) * 7 + 3)).all()


def test_lookback_timeout_reaches_the_host():
    """A look-back wait that times out (a broken inter-workgroup hand-off) used to leave a mark only the device could see
    (VERDICT r3): the pass goes on with a wrong base and the frame is silently mis-sorted.  The kernel now also raises bit 0 of
    the frame's first status word.  GSR_TEST_FORCE_LOOKBACK_TIMEOUT=1 makes chunk 0 of the last pass behave as if its wait had
    timed out (mark + status bit; the sort's result is left alone): the frame's status then raises GsrError when it is looked at
    (the next call on the device, or call_stats), in every forward mode, and with debug=True the failing call itself returns
    GSR_ERR_HIP - the reference's failure contract (README.md:168-171: raise, and with --debug dump the inputs)."""
    import os
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _C
    from helpers import run_hip
    from scene_utils import make_gaussians, fibonacci_cameras
    raw = make_gaussians(4000, 1, seed=31, scale_factor=0.8)
    cam = fibonacci_cameras(2, 160, 96, seed=32)[0]
    bg = torch.zeros(3)
    ok = run_hip(raw, cam, 1, bg)                    # a clean frame first (and the shape's capacity)
    dgr.call_stats()
    os.environ["GSR_TEST_FORCE_LOOKBACK_TIMEOUT"] = "1"
    try:
        for mode in ("exact", "async"):
            out = run_hip(raw, cam, 1, bg, forward_mode=mode)          # fire-and-forget: the call itself returns
            with pytest.raises(_C.GsrError, match="look-back"):
                dgr.call_stats()                                       # ... its status does not
            assert torch.equal(out["color"], ok["color"])              # (the hook leaves the sort's result alone)
        with pytest.raises(_C.GsrError, match="look-back"):
            run_hip(raw, cam, 1, bg, debug=True)                       # debug: the failing call raises (and dumps snapshot_fw.dump)
    finally:
        os.environ.pop("GSR_TEST_FORCE_LOOKBACK_TIMEOUT", None)
        for f in ("snapshot_fw.dump",):
            if os.path.exists(f):
                os.remove(f)
    dgr.call_stats()                                                    # nothing is left pending
    again = run_hip(raw, cam, 1, bg)
    dgr.call_stats()
    assert torch.equal(again["color"], ok["color"])


# ---- the tile sort's own form (gsr_debug_tile_sort) ----
TILE_BITS = [1, 5, 8, 9, 13, 16, 17, 24]                 # 1, 2 and 3 passes
TILE_N = [1, 2047, 2048, 2049, 4097, 40_001]
PATTERNS = ("uniform", "one_tile_0", "one_tile_last", "alternate", "sorted_long_run", "sparse", "n_dev")


def _tile_keys(pattern, n, bits, rng):
    """-> (keys uint32 [n], all below 2^bits; number of keys present)"""
    T = 1 << bits
    m = n
    if pattern in ("uniform", "n_dev"):
        keys = rng.integers(0, T, n, dtype=np.uint64)
        if pattern == "n_dev":
            m = (3 * n) // 5                              # a device-side count of 3/5 of the capacity
    elif pattern == "one_tile_0":
        keys = np.zeros(n, dtype=np.uint64)
    elif pattern == "one_tile_last":
        keys = np.full(n, T - 1, dtype=np.uint64)
    elif pattern == "alternate":                          # two tiles in turn, the larger one first
        keys = np.where(np.arange(n) % 2 == 0, T - 1, (T - 1) // 3).astype(np.uint64)
    elif pattern == "sorted_long_run":
        # sorted input; tile r owns a run of three chunks and a bit between smaller and larger tiles - where n has room for
        # that (40,001 and the sizes around 2^21); below, r owns the middle half, which still crosses a chunk boundary at 4097
        chunk = 2048 if n < (2 << 20) else 4096
        r = T // 2
        run = 3 * chunk + 37 if n > 3 * chunk + 39 else max(1, n // 2)
        below = (n - run) // 2
        above = n - run - below if r + 1 < T else 0
        run = n - below - above
        keys = np.concatenate([np.sort(rng.integers(0, r, below, dtype=np.uint64)), np.full(run, r, dtype=np.uint64),
                               np.sort(rng.integers(r + 1, T, above, dtype=np.uint64)) if above else np.zeros(0, dtype=np.uint64)])
    elif pattern == "sparse":                             # 90 % of the tiles empty
        present = rng.choice(T, max(1, T // 10), replace=False).astype(np.uint64)
        keys = present[rng.integers(0, present.size, n)]
    else:
        raise ValueError(pattern)
    keys = keys.astype(np.uint32)
    assert keys.size == n and int(keys.max()) < T         # (the last pass indexes ranges_enc[2^bits] by the key)
    return keys, m


def _tile_sort(keys, m, bits, dual, iota, vals, wals):
    """One gsr_debug_tile_sort call -> (values, second payload or None, ranges_enc as a device tensor [2^bits, 2])"""
    from diff_gaussian_rasterization import _C
    lib = _C.lib()
    n = keys.size
    dev = "cuda"
    t = lambda a: torch.from_numpy(a.view(np.int32)).to(dev)
    k0, k1 = t(keys), torch.empty(n, dtype=torch.int32, device=dev)
    v0 = torch.full((n,), -1, dtype=torch.int32, device=dev) if iota else t(vals)
    v1 = torch.empty(n, dtype=torch.int32, device=dev)
    w0 = t(wals) if dual else None
    w1 = torch.empty(n, dtype=torch.int32, device=dev) if dual else None
    enc = torch.zeros((1 << bits, 2), dtype=torch.int32, device=dev)
    # (dirty scratch: the look-back words of the second and third pass are zero only if the pass before cleared them)
    tmp = torch.full((lib.gsr_debug_radix_tmp_bytes(n),), 0xFF, dtype=torch.uint8, device=dev)
    nd = None if m == n else torch.tensor([m, 0], dtype=torch.int32, device=dev)
    where = _C.check(lib.gsr_debug_tile_sort(_C.ptr(k0), _C.ptr(v0), _C.ptr(k1), _C.ptr(v1), _C.ptr(w0), _C.ptr(w1), n, bits,
                                             1 if iota else 0, _C.ptr(nd), _C.ptr(enc), _C.ptr(tmp), _C._stream()))
    torch.cuda.synchronize()
    assert where == ((bits + 7) // 8) & 1
    vs, ws = (v1, w1) if where else (v0, w0)
    return vs.cpu().numpy().view(np.uint32), None if ws is None else ws.cpu().numpy().view(np.uint32), enc


def _check_tile_sort(n, bits, seed):
    import binning_reference as BR
    rng = np.random.default_rng(seed)
    vals = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    wals = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    for pattern in PATTERNS:
        keys, m = _tile_keys(pattern, n, bits, rng)
        ks, _, order = BR.stable_sort_pairs(keys[:m], bits)                   # one reference per pattern, shared by the four forms
        present, pairs = BR.encoded_ranges_sparse(ks)                         # (dense on the device: 2^24 pairs are 134 MB)
        want_enc = torch.zeros((1 << bits, 2), dtype=torch.int32, device="cuda")
        want_enc[torch.from_numpy(present).cuda()] = torch.from_numpy(pairs.view(np.int32)).cuda()
        for dual in (False, True):
            for iota in (False, True):
                vs, ws, enc = _tile_sort(keys, m, bits, dual, iota, vals, wals)
                what = (pattern, n, bits, dual, iota)
                assert (vs[:m] == (order.astype(np.uint32) if iota else vals[:m][order])).all(), what
                if dual:
                    assert (ws[:m] == wals[:m][order]).all(), what
                assert torch.equal(enc, want_enc), what                       # every one of the 2^bits tiles


@pytest.mark.parametrize("bits", TILE_BITS)
@pytest.mark.parametrize("n", TILE_N)
def test_tile_sort_form_matches_stable_reference(n, bits):
    """Payloads equal the stable reference and ranges_enc the encoded reference, for every key pattern, single and dual payload,
    values given and values = index.  (The sorted keys are not asserted: the last pass does not write them.)"""
    _check_tile_sort(n, bits, seed=1000 * bits + n)


@pytest.mark.parametrize("n", [2_097_151, 2_097_152, 2_097_153])
def test_tile_sort_form_at_the_chunk_size_switch(n):
    _check_tile_sort(n, 13, seed=n)
