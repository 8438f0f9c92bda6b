"""gsr_hamming_match / gsr_hamming_vote and match_descriptors against numpy: every size around the tile and wave boundaries, ties
and duplicates, segments of length 0, 1 and 300 in one call, the mutual filter."""
import numpy as np
import pytest
import torch

import orb_reference as R

pytestmark = pytest.mark.gpu
SIZES = [0, 1, 63, 64, 65, 257, 1000]


def _words(n, seed, base=None, flips=40):
    """n descriptors: copies of a few base words with some bits flipped, so that distances are small and ties are common"""
    rng = np.random.RandomState(seed)
    if base is None:
        base = rng.randint(0, 256, size=(12, 32)).astype(np.uint8)
    rows = base[rng.randint(0, len(base), size=n)].copy()
    bits = np.unpackbits(rows, axis=1)
    for r in range(n):
        bits[r, rng.randint(0, 256, size=rng.randint(0, flips))] ^= 1
    return np.packbits(bits, axis=1).view(np.int32).reshape(n, 8), base


@pytest.fixture(scope="module")
def data():
    q, base = _words(1000, 1)
    t, _ = _words(1000, 2, base)
    return q, t, R.hamming_matrix(q, t)


def _match(q, t):
    import scene_utils as su
    out = su.hamming_match(torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda())
    return [o.cpu().numpy() for o in out]


def _ref_from(D):
    Q, N = D.shape
    idx, best, second = np.full(Q, -1, np.int32), np.full(Q, R.NONE, np.int32), np.full(Q, R.NONE, np.int32)
    if N:
        idx = D.argmin(axis=1).astype(np.int32)
        best = D[np.arange(Q), idx].astype(np.int32)
    if N > 1:
        second = np.partition(D, 1, axis=1)[:, 1].astype(np.int32)
    return idx, best, second


@pytest.mark.parametrize("Q", SIZES)
def test_match_at_every_size(Q, data):
    q, t, D = data
    for N in SIZES:
        idx, best, second = _match(q[:Q], t[:N])
        r_idx, r_best, r_second = _ref_from(D[:Q, :N])
        assert np.array_equal(idx, r_idx), (Q, N)
        assert np.array_equal(best, r_best) and np.array_equal(second, r_second), (Q, N)
    if Q == 1000:
        assert (np.sort(D, axis=1)[:, 0] == np.sort(D, axis=1)[:, 1]).mean() > 0.05      # the data has tied minima


def test_duplicated_rows_tie_to_the_lowest_index():
    q, base = _words(130, 3)
    t = np.concatenate([q[::-1], q[::-1], q[:7]])      # every query row three or two times, far apart and across tiles
    idx, best, second = _match(q, t)
    assert (best == 0).all() and (second == 0).all()
    first = np.array([min(j for j in range(len(t)) if (t[j] == q[i]).all()) for i in range(len(q))])
    assert np.array_equal(idx, first)
    assert np.array_equal(idx, R.hamming_ref(q, t)[0])


def _vote(q, t, seg, md, ratio):
    from diff_gaussian_rasterization import _C
    qd, td = torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()
    sd = torch.tensor(seg, dtype=torch.int32, device="cuda")
    votes = torch.full((len(seg) - 1,), -7, dtype=torch.int32, device="cuda")
    _C.check(_C.lib().gsr_hamming_vote(len(q), _C.ptr(qd) if len(q) else None, len(t), _C.ptr(td), len(seg) - 1, _C.ptr(sd), md, ratio,
                                       _C.ptr(votes), _C._stream()))
    return votes.cpu().numpy()


def test_vote_over_segments_of_length_0_1_and_300(data):
    q, t, _ = data
    seg = [0, 0, 1, 301, 301, 601, 602]
    db = t[:602].copy()
    db[301:601] = q[100:400]      # a frame that holds 300 of the query rows themselves
    for md, ratio in ((64, 0.8), (20, 1.0), (256, 0.5)):
        votes = _vote(q[:500], db, seg, md, ratio)
        ref = R.vote_ref(q[:500], db, seg, md, ratio)
        assert np.array_equal(votes, ref), (md, ratio)
        assert votes[0] == 0 and votes[3] == 0
    assert _vote(q[:500], db, seg, 64, 0.8)[4] >= 150
    assert np.array_equal(_vote(q[:500], db, seg, 64, 0.8), _vote(q[:500], db, seg, 64, 0.8))
    assert not _vote(q[:0], db, seg, 64, 0.8).any()      # no query rows: the counts are cleared
    # offsets beyond the database are clamped: nothing is read past it
    assert np.array_equal(_vote(q[:70], db, [0, 300, 5000], 64, 0.8), R.vote_ref(q[:70], db, [0, 300, 602], 64, 0.8))


def test_mutual_matches_are_a_symmetric_subset(data):
    import scene_utils as su
    q, t, D = data
    a, b = torch.from_numpy(q[:300]).cuda(), torch.from_numpy(t[:257]).cuda()
    one = su.match_descriptors(a, b, max_distance=64, ratio=0.9, mutual=False).cpu().numpy()
    both = su.match_descriptors(a, b, max_distance=64, ratio=0.9, mutual=True).cpu().numpy()
    back = su.match_descriptors(b, a, max_distance=64, ratio=0.9, mutual=True).cpu().numpy()
    assert len(both) and len(one) > len(both)
    assert (np.diff(one[:, 0]) > 0).all() and (np.diff(both[:, 0]) > 0).all() and both.dtype == np.int32
    assert {tuple(p) for p in both} <= {tuple(p) for p in one}
    assert {tuple(p) for p in both} == {(int(i), int(j)) for j, i in back}
    # the one-way result is the rule itself
    idx, best, second = _ref_from(D[:300, :257])
    keep = (best <= 64) & (best.astype(np.float32) < np.float32(0.9) * second.astype(np.float32))
    assert np.array_equal(one, np.stack([np.nonzero(keep)[0], idx[keep]], axis=1))
    empty = su.match_descriptors(a, b[:0]).cpu().numpy()
    assert empty.shape == (0, 2)
