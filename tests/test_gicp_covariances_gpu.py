"""gsr_estimate_covariances and gsr_regularize_covariances on the device (csrc/gicp.hip) against the float64 restatement of
tests/gicp_reference.py, on the clouds, sizes and neighbourhoods of tests/test_normals_gpu.py (whose analyses are shared).

Bounds.  count: exact (tests/test_normals_cpu.py shows that the float32 membership is the float64 one on every row).  Sigma = I -
(1 - epsilon) n n^T: the normals' own bound, 1e-6 max-abs on n where (l1 - l0) / l2 >= NR.GAP, carried through the product -
|d(n_a n_b)| <= 2 x 1e-6 for a unit n - plus the float32 rounding of an entry of magnitude <= 1, 2^-24 (2^-23 allowed): 2 (1 -
epsilon) 1e-6 + 2^-23.  Symmetric by construction: six values are stored.  Trace = 3 - (1 - epsilon) |n|^2 = 2 + epsilon to 1e-6
on every row with a neighbourhood of three or more, whatever its shape."""
import numpy as np
import pytest
import torch

import gicp_reference as G
import normals_reference as NR
import scene_utils as S
from test_normals_gpu import case

pytestmark = pytest.mark.gpu
I6 = np.float32([1, 0, 0, 1, 0, 1])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.contiguous().view(torch.int32)


def bound(epsilon):
    return 2.0 * (1.0 - epsilon) * 1e-6 + 2.0 ** -23


def check(a, got, epsilon, label):
    cov, count = (t.cpu().numpy() for t in got)
    P = a["count"].shape[0]
    assert cov.dtype == np.float32 and cov.shape == (P, 6) and count.dtype == np.int32 and count.shape == (P,), label
    assert np.array_equal(count, a["count"]), (label, int((count != a["count"]).sum()))
    finite, few = a["finite"], a["finite"] & (a["count"] < 3)
    full = a["finite"] & (a["count"] >= 3)
    assert np.isnan(cov[~finite]).all(), label
    assert np.array_equal(cov[few], np.tile(I6, (int(few.sum()), 1))), label
    trace = np.abs(cov[full][:, [0, 3, 5]].astype(np.float64).sum(axis=1) - (2.0 + epsilon)).max(initial=0.0)
    assert trace <= 1e-6, (label, trace)
    with np.errstate(invalid="ignore"):
        shaped = full & (a["gap"] >= NR.GAP)
    want = G.covariances(None, None, None, epsilon, analysis=a)["cov"]
    err = np.abs(cov[shaped].astype(np.float64) - want[shaped]).max(initial=0.0)
    print(f"{label}: rows {int(full.sum())}, compared {int(shaped.sum())}, err {err:.3g} (bound {bound(epsilon):.3g}), "
          f"trace err {trace:.3g}")
    assert err <= bound(epsilon), (label, err)


@pytest.mark.parametrize("P", NR.SIZES)
@pytest.mark.parametrize("kind", list(NR.CLOUDS))
def test_covariances_against_the_reference(kind, P):
    pts, refs = case(kind, P)
    d = dev(pts)
    for (radius, nn), a in zip(NR.combos(kind), refs):
        check(a, S.estimate_covariances(d, radius, nn, return_count=True), G.EPSILON, f"{kind} P={P} radius={radius:.4g} max_nn={nn}")
    radius, nn = NR.combos(kind)[-1]
    for eps in (1.0, 0.25):
        check(refs[-1], S.estimate_covariances(d, radius, nn, epsilon=eps, return_count=True), eps, f"{kind} P={P} epsilon={eps}")
    only = S.estimate_covariances(d, radius, nn)
    assert torch.equal(bits(only), bits(S.estimate_covariances(d, radius, nn, return_count=True)[0]))


def test_one_and_two_rows_are_isotropic():
    for P in (1, 2):
        cov, count = S.estimate_covariances(torch.rand(P, 3).cuda(), NR.INF, 3, return_count=True)
        assert cov.tolist() == [I6.tolist()] * P and count.tolist() == [P] * P


def test_runs_are_bit_identical_and_simple_knn_is_the_same_call():
    import simple_knn
    for kind, radius, nn in (("duplicates", NR.RADIUS, 30), ("clusters", NR.RADIUS, 3), ("sphere", NR.INF, 4),
                             ("lattice", NR.INF, 9), ("lattice", NR.INF, 17)):
        pts = dev(NR.cloud(kind, 5000))
        a = S.estimate_covariances(pts, radius, nn, return_count=True)
        b = simple_knn.estimate_covariances(pts, radius, nn, return_count=True)
        for x, y in zip(a, b):
            assert torch.equal(bits(x), bits(y)), (kind, nn)
        assert torch.equal(bits(simple_knn.regularize_covariances(a[0])), bits(S.regularize_covariances(a[0])))


def test_non_finite_rows_get_nan_and_change_no_other_row():
    pts = NR.cloud("plane", 4097)
    junk = np.array([[np.nan, 0, 0], [0.3, np.inf, 0.1], [0.3, -0.2, -np.inf], [np.nan] * 3], dtype=np.float32)
    both = np.concatenate([pts, np.repeat(junk, 10, axis=0)])
    for radius, nn in ((NR.INF, 30), (NR.RADIUS, 33), (NR.RADIUS, 3), (NR.INF, 4)):
        clean = S.estimate_covariances(dev(pts), radius, nn, return_count=True)
        cov, count = S.estimate_covariances(dev(both), radius, nn, return_count=True)
        for x, y in zip(clean, (cov, count)):
            assert torch.equal(bits(x), bits(y[:4097]))
        assert bool(torch.isnan(cov[4097:]).all()) and count[4097:].tolist() == [0] * 40
    cov, count = S.estimate_covariances(dev(junk), NR.INF, 3, return_count=True)
    assert bool(torch.isnan(cov).all()) and count.tolist() == [0] * 4


def test_the_covariance_is_flat_along_the_normal_of_estimate_normals():
    pts = dev(NR.cloud("sphere", 5000))
    n = S.estimate_normals(pts, NR.RADIUS, 20).double()
    cov6, count = S.estimate_covariances(pts, NR.RADIUS, 20, return_count=True)
    cov = torch.from_numpy(G.full(cov6.cpu().numpy())).cuda()
    along = torch.einsum("pa,pab,pb->p", n, cov, n)
    full = count >= 3                                           # (below three rows: the normal is (0, 0, 1) and Sigma is I)
    assert 4900 <= int(full.sum()) < 5000
    # n^T Sigma n = epsilon for the normal the same kernels' arithmetic gave (float32 n: 1e-6)
    assert float((along[full] - G.EPSILON).abs().max()) <= 1e-5
    assert float((along[~full] - 1.0).abs().max()) == 0.0


# ---- gsr_regularize_covariances -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 255, 256, 257, 65537])
def test_regularize_against_the_reference(P):
    given = G.random_spd(P, 70 + P)
    given[::5] *= np.float32(1e-6)                              # (a map's Gaussians: centimetres squared)
    ref = G.regularize(given)
    assert np.nanmin(ref["gap"]) >= 1e-3
    got = S.regularize_covariances(dev(given)).cpu().numpy()
    err = np.abs(got.astype(np.float64) - ref["cov"]).max()
    print(f"regularize P={P}: err {err:.3g} (bound {bound(G.EPSILON):.3g}), least gap {np.nanmin(ref['gap']):.3g}")
    assert got.dtype == np.float32 and got.shape == (P, 6) and err <= bound(G.EPSILON)
    assert np.abs(got[:, [0, 3, 5]].astype(np.float64).sum(axis=1) - (2.0 + G.EPSILON)).max() <= 1e-6
    half = S.regularize_covariances(dev(given), 0.5).cpu().numpy()
    assert np.abs(half.astype(np.float64) - G.regularize(given, 0.5)["cov"]).max() <= bound(0.5)


def test_regularize_isotropic_nan_and_in_place_rows():
    rng = np.random.default_rng(8)
    given = G.random_spd(1000, 9)
    iso = rng.integers(0, 1000, size=100)
    given[iso] = I6[None, :] * (10.0 ** rng.uniform(-6, 2, size=(100, 1))).astype(np.float32)
    bad = np.setdiff1d(rng.integers(0, 1000, size=60), iso)
    for k, r in enumerate(bad):
        given[r, k % 6] = (np.nan, np.inf, -np.inf)[k % 3]
    d = dev(given)
    keep = d.clone()
    out = S.regularize_covariances(d)
    assert torch.equal(bits(d), bits(keep))                     # (the call leaves its input alone)
    got = out.cpu().numpy()
    assert np.array_equal(got[iso], np.tile(I6, (100, 1)))
    assert np.isnan(got[bad]).all() and np.isfinite(np.delete(got, bad, axis=0)).all()
    ref = G.regularize(given)["cov"]
    rest = np.setdiff1d(np.arange(1000), np.concatenate([iso, bad]))
    assert np.abs(got[rest].astype(np.float64) - ref[rest]).max() <= bound(G.EPSILON)
    # in place: the C entry with cov_out = cov_in gives the bits of the out-of-place call
    from diff_gaussian_rasterization import _C
    with _C.on_device(d.device):
        _C.check(_C.lib().gsr_regularize_covariances(1000, _C.ptr(d), G.EPSILON, _C.ptr(d), _C._stream()))
    assert torch.equal(bits(d), bits(out))
    # regularising twice changes nothing but rounding: Sigma's least direction is the one it was built about
    again = S.regularize_covariances(out).cpu().numpy()
    assert np.abs(again[rest].astype(np.float64) - got[rest]).max() <= bound(G.EPSILON)
