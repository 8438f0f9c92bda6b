"""The library's device-wide prefix sum (gsr_scan_u32, sort_scan.hip) through its test hook, bit-exact against numpy
(tests/binning_reference.py): every size at which it changes path - one k_scan_apply workgroup up to 2048 elements,
k_scan_single up to 8192, reduce -> scan of the chunk sums -> apply beyond, with 2048 / 2049 chunk sums (4,194,304 / 4,194,305
elements) and a second recursion level from 8193 chunk sums (16,777,217 elements) - exclusive and inclusive, through a gather,
in place, with sums that wrap 2^32; and nothing written outside the n output words."""
import numpy as np
import pytest
import torch

import binning_reference as BR

pytestmark = pytest.mark.gpu

SMALL = [1, 255, 256, 257, 2047, 2048, 2049, 4096, 8191, 8192, 8193, 10241]
LARGE = [4_194_304, 4_194_305, 16_777_216, 16_777_217]
PAD = 64                     # guard words on either side of the output
PATTERN = 0x5A5AA5A5


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32))


def _scan(src, idx, inclusive, inplace=False):
    """src (numpy uint32), idx (numpy uint32 or None) -> the hook's output as numpy uint32; asserts the guard words."""
    from diff_gaussian_rasterization import _C
    lib = _C.lib()
    n = src.size
    dev = "cuda"
    buf = torch.full((n + 2 * PAD,), PATTERN, dtype=torch.int32, device=dev)
    out = buf[PAD:PAD + n]
    if inplace:
        out.copy_(_i32(src))
        s = out
    else:
        s = _i32(src).to(dev)
    ix = None if idx is None else _i32(idx).to(dev)
    tmp = torch.empty(lib.gsr_debug_scan_tmp_bytes(n), dtype=torch.uint8, device=dev)
    _C.check(lib.gsr_debug_scan_u32(_C.ptr(s), _C.ptr(ix), _C.ptr(out), n, 1 if inclusive else 0, _C.ptr(tmp), _C._stream()))
    torch.cuda.synchronize()
    assert bool((buf[:PAD] == PATTERN).all()) and bool((buf[PAD + n:] == PATTERN).all()), "guard words overwritten"
    if not inplace:
        assert torch.equal(s.cpu(), _i32(src)), "the source was modified"
    return out.cpu().numpy().view(np.uint32)


def _check(src, idx=None, inplace=False):
    for inclusive in (False, True):
        got = _scan(src, idx, inclusive, inplace)
        want = BR.scan_u32(src, idx, inclusive)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (src.size, inclusive, int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))


@pytest.mark.parametrize("n", SMALL + LARGE)
def test_scan_matches_numpy_exclusive_and_inclusive(n):
    rng = np.random.default_rng(n)
    _check(rng.integers(0, 4, n, dtype=np.uint32))


@pytest.mark.parametrize("n", SMALL + [4_194_305])
def test_scan_through_a_gather(n):
    """The forward's tile-count scan: out[i] = scan of src[idx[i]], idx a permutation."""
    rng = np.random.default_rng(n + 1)
    _check(rng.integers(0, 4, n, dtype=np.uint32), idx=rng.permutation(n).astype(np.uint32))


@pytest.mark.parametrize("n", [2049, 8193, 4_194_305])
def test_scan_in_place(n):
    """src == out, as the library scans its own chunk sums: the single-workgroup chain and the three-launch form."""
    rng = np.random.default_rng(n + 2)
    _check(rng.integers(0, 4, n, dtype=np.uint32), inplace=True)


def test_scan_of_ones_counts():
    n = 4_194_305
    src = np.ones(n, dtype=np.uint32)
    assert (_scan(src, None, False) == np.arange(n, dtype=np.uint32)).all()
    assert (_scan(src, None, True) == np.arange(1, n + 1, dtype=np.uint32)).all()


@pytest.mark.parametrize("n", [2048, 8192, 10241])
def test_scan_wraps_modulo_2_32(n):
    """Full-range 32-bit values: the running total passes 2^32 thousands of times and must wrap like the reference."""
    rng = np.random.default_rng(n + 3)
    src = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    assert int(src.astype(np.uint64).sum()) > (1 << 32)
    _check(src)
