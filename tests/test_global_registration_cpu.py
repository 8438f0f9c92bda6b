"""Global registration without a device: the new symbols, argument validation (before any device work, so it can be seen here),
self-checks of the float64 reference (tests/global_registration_reference.py) and the PRECONDITIONS of the GPU tests' inputs,
shown on the reference alone for the seeds used:
  - FPFH: on every pair of every neighbourhood, each scaled pair feature lies >= 1e-9 from an integer (the bin is the same in
    any float64 arithmetic), | |a1| - |a2| | >= 1e-9 or exactly 0, |v| >= 1e-9 d or exactly 0; membership gaps as in
    test_normals_cpu.py (coordinates are multiples of 2^-10, the lattice's of 1 / 8);
  - matching: best and second-best feature distance more than 1e-5 relative apart on the rows the mutual-filter test compares;
  - the end-to-end scene: the reference pipeline recovers the planted motion, ICP from the identity does not."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import global_registration_reference as G
import normals_reference as NR
import registration_reference as RR

NEW_SYMBOLS = ("gsr_fpfh_workspace_bytes", "gsr_compute_fpfh", "gsr_feature_nn_workspace_bytes", "gsr_feature_nn_tiles_per_split",
               "gsr_feature_nn", "gsr_ransac_workspace_bytes", "gsr_ransac_feature_matching")
MARGIN = 1e-5
EXACT = 1e-9


def test_new_symbols_resolve_and_the_abi_version_stays():
    from diff_gaussian_rasterization import _C
    raw = ctypes.CDLL(_C.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert hasattr(raw, n) and n in _C.EXPORTS, n
    lib = _C.lib()
    assert lib.gsr_abi_version() == 7
    for f in (lib.gsr_fpfh_workspace_bytes, lib.gsr_feature_nn_workspace_bytes, lambda P: lib.gsr_ransac_workspace_bytes(P, 16384),
              lambda n: lib.gsr_ransac_workspace_bytes(5000, n)):
        sizes = [f(P) for P in (0, 1, 65, 4097, 307200, 1000000)]
        assert all(s > 0 and s % 256 == 0 for s in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:]))
    # the split of the matching kernel's target range: whole tiles, never more runs than tiles, one run once the queries fill the CUs
    assert lib.gsr_feature_nn_tiles_per_split(1, 1) == 1 and lib.gsr_feature_nn_tiles_per_split(1, 5000) == 1
    assert lib.gsr_feature_nn_tiles_per_split(5000, 5000) == 2 and lib.gsr_feature_nn_tiles_per_split(1 << 20, 5000) == 40


def test_entry_points_reject_bad_arguments_before_any_launch():
    from diff_gaussian_rasterization import _C
    lib = _C.lib()
    p = ctypes.c_void_p(4096)      # never dereferenced: every call below fails its argument check
    inf, nan, big = float("inf"), float("nan"), 1 << 40
    f = lib.gsr_compute_fpfh
    for args in ((0, p, p, 0.1, 0, p, None, None, p, big), (1 << 30, p, p, 0.1, 0, p, None, None, p, big),
                 (5, None, p, 0.1, 0, p, None, None, p, big), (5, p, None, 0.1, 0, p, None, None, p, big),
                 (5, p, p, 0.1, 0, None, None, None, p, big), (5, p, p, 0.1, 0, p, None, None, None, big),
                 (5, p, p, 0.0, 0, p, None, None, p, big), (5, p, p, nan, 30, p, None, None, p, big),
                 (5, p, p, 0.1, 1, p, None, None, p, big), (5, p, p, 0.1, 2, p, None, None, p, big),
                 (5, p, p, 0.1, 34, p, None, None, p, big), (5, p, p, 0.1, -1, p, None, None, p, big),
                 (5, p, p, inf, 0, p, None, None, p, big)):
        assert f(*args, None) == -1, args
    assert f(5, p, p, inf, 33, p, None, None, p, lib.gsr_fpfh_workspace_bytes(5) - 1, None) == -5
    assert "needed" in _C.last_error()
    m = lib.gsr_feature_nn
    for args in ((0, p, 5, p, 33, p, None, p, big), (5, p, 0, p, 33, p, None, p, big), (5, None, 5, p, 33, p, None, p, big),
                 (5, p, 5, None, 33, p, None, p, big), (5, p, 5, p, 33, None, None, p, big), (5, p, 5, p, 33, p, None, None, big),
                 (5, p, 5, p, 32, p, None, p, big), (5, p, 5, p, 34, p, None, p, big)):
        assert m(*args, None) == -1, args
    assert m(5, p, 5, p, 33, p, None, p, lib.gsr_feature_nn_workspace_bytes(5) - 1, None) == -5
    r = lib.gsr_ransac_feature_matching
    ws = lib.gsr_ransac_workspace_bytes(10, 64)
    good = [5, p, 5, p, 10, p, 0.1, 3, 0.9, 1, 0, 64, p, p, ws, None]
    assert r(*good[:14], ws - 1, None, None) == -5
    for k, v in ((0, 0), (1, None), (2, 1 << 30), (3, None), (4, 0), (5, None), (6, -1.0), (6, nan), (6, inf), (7, 2), (7, 9),
                 (8, -0.1), (8, 1.5), (8, nan), (10, -1), (11, 0), (11, (1 << 20) + 1), (12, None), (13, None)):
        args = list(good)
        args[k] = v
        assert r(*args, None) == -1, (k, v)


def test_python_validation_comes_first_and_there_is_no_cpu_path():
    import scene_utils as S
    import simple_knn
    from diff_gaussian_rasterization import _C
    a, b, n = torch.rand(10, 3), torch.rand(12, 3), torch.rand(10, 3)
    fa, fb = torch.rand(10, 33), torch.rand(12, 33)
    pairs = torch.zeros((5, 2), dtype=torch.int32)
    R = S.registration_ransac_based_on_feature_matching
    for call in (lambda: S.compute_fpfh_feature(a, n, 0.0), lambda: S.compute_fpfh_feature(a, n, float("nan")),
                 lambda: S.compute_fpfh_feature(a, n, 0.1, 2), lambda: S.compute_fpfh_feature(a, n, 0.1, 34),
                 lambda: S.compute_fpfh_feature(a, n, float("inf"), 0), lambda: S.compute_fpfh_feature(a, b, 0.1),
                 lambda: simple_knn.compute_fpfh(a, n, 0.1, 1), lambda: S.match_features(torch.rand(10, 32), fb),
                 lambda: S.match_features(fa, torch.rand(12, 34)), lambda: S.feature_nn(fa, torch.rand(33)),
                 lambda: R(a, b, fa, fb, True, 0.1, ransac_n=2), lambda: R(a, b, fa, fb, True, 0.1, ransac_n=9),
                 lambda: R(a, b, fa, fb, True, 0.1, edge_length_threshold=1.5), lambda: R(a, b, fa, fb, True, -0.1),
                 lambda: R(a, b, fa, fb, True, float("inf")), lambda: R(a, b, fa, fb, True, 0.1, confidence=1.5),
                 lambda: R(a, b, fa, fb, True, 0.1, max_iteration=0), lambda: R(a, b, fa, fb, True, 0.1, batch=0),
                 lambda: R(a, b, fa, fb, True, 0.1, seed=-1), lambda: R(a, b, fb, fa, True, 0.1),
                 lambda: R(a, b, None, None, True, 0.1, pairs=torch.zeros((5, 3), dtype=torch.int32)),
                 lambda: S.register_and_merge(a, None, b, None, global_init=True, global_seed=-1)):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: S.compute_fpfh_feature(a, n, "0.1"), lambda: S.compute_fpfh_feature(a, n, 0.1, 30.0),
                 lambda: S.match_features(fa, fb, mutual_filter=1), lambda: R(a, b, fa, fb, 1, 0.1),
                 lambda: R(a, b, fa, fb, True, 0.1, ransac_n=3.0), lambda: R(a, b, fa, fb, True, 0.1, seed=1.5),
                 lambda: S.register_and_merge(a, None, b, None, global_init=1),
                 lambda: S.register_and_merge(a, None, b, None, global_init=True, init=torch.eye(4))):
        with pytest.raises(TypeError):
            call()
    for call in (lambda: S.compute_fpfh_feature(a, n, 0.1), lambda: simple_knn.compute_fpfh(a, n, 0.1, 30, return_stats=True),
                 lambda: S.match_features(fa, fb), lambda: S.feature_nn(fa, fb), lambda: R(a, b, fa, fb, True, 0.1),
                 lambda: R(a, b, None, None, False, 0.1, pairs=pairs), lambda: S.ransac_trials(a, b, pairs, 0.1, 3, 0.9, 0, 0, 10),
                 lambda: S.global_registration(a, b, 0.05), lambda: S.register_and_merge(a, None, b, None, global_init=True)):
        with pytest.raises(_C.GsrError, match="no CPU path"):
            call()
    assert callable(simple_knn.compute_fpfh) and "compute_fpfh" in simple_knn.__all__


# ---- the reference itself -----------------------------------------------------------------------------------------------------------
def test_reference_generator_equals_a_hand_computed_vector():
    # mix(0x9E3779B97F4A7C15) is the first output of splitmix64 seeded with 0, a published constant; the sample rows below were
    # computed with unbounded integers reduced mod 2^64 by hand of the formula in include/gsr.h
    assert int(G.mix(np.uint64(0x9E3779B97F4A7C15))) == 0xE220A8397B1DCDAF and int(G.mix(np.uint64(1))) == 0x5692161D100B05E5
    assert G.samples(12345, 0, 2, 4, 5000).tolist() == [[665, 1024, 597, 880], [2398, 4337, 923, 1901]]
    assert G.samples(12345, 2 ** 40 + 7, 1, 4, 5000).tolist() == [[1103, 2985, 846, 4956]]
    m64 = (1 << 64) - 1

    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m64
        return z ^ (z >> 31)

    for seed, t0, rn, M in ((0, 0, 8, 3), (2 ** 64 - 1, 2 ** 50, 3, 2 ** 30 - 1), (977, 4097, 5, 257)):      # (wrap-around included)
        want = [[((mix((seed + (8 * (t0 + k) + s + 1) * 0x9E3779B97F4A7C15) & m64) >> 32) * M) >> 32 for s in range(rn)]
                for k in range(64)]
        assert G.samples(seed, t0, 64, rn, M).tolist() == want, (seed, t0)


def test_reference_pair_feature_of_a_hand_made_pair():
    # p_i at the origin with normal +z, p_j at (1, 0, 0) with normal +x: a1 = 0, a2 = 1 -> swapped: n1 = +x, delta = (-1, 0, 0)
    # parallel to n1 -> |v| = 0 -> the zero feature.  With n_j = (0, 1, 0): a1 = a2 = 0, no swap, v = delta x z = (0, -1, 0),
    # w = z x v = (1, 0, 0), f1 = v.n_j = -1, f0 = atan2(w.n_j, n_i.n_j) = atan2(0, 0) = 0, f2 = 0
    d = np.array([[1.0, 0.0, 0.0]] * 2)
    f = G.pair_features(d, np.array([[0.0, 0.0, 1.0]] * 2), np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]))["f"]
    assert f.tolist() == [[0.0, 0.0, 0.0], [0.0, -1.0, 0.0]]
    assert np.floor(G.scaled(f)).tolist() == [[5, 5, 5], [5, 0, 5]]
    # a duplicate: the zero feature, counted in SPFH, skipped in the weighted sum; one block of a non-empty row sums to 200
    pts = np.float32([[0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 1, 0]])
    a = G.analyse(pts, np.tile(np.float32([0, 0, 1]), (4, 1)), [(2.0, 0)])[0]
    assert a["m"].tolist() == [3, 3, 3, 3] and a["counts"][0, 5] == 3 and a["counts"].sum(axis=1).tolist() == [9] * 4
    assert np.abs(a["fpfh"].reshape(4, 3, 11).sum(axis=2) - 200).max() < 1e-12


# ---- preconditions --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fpfh_case(kind, P):
    pts, nrm = G.cloud(kind, P)
    return pts, nrm, G.analyse(pts, nrm, G.combos(kind))


@pytest.mark.parametrize("kind", list(G.CLOUDS))
def test_preconditions_of_the_fpfh_clouds(kind):
    seen = set()
    for P in G.SIZES:
        pts, nrm, refs = fpfh_case(kind, P)
        unit = 8 if kind == "lattice" else 1 / NR.QUANTUM
        assert np.array_equal(pts.astype(np.float64) * unit, np.round(pts.astype(np.float64) * unit))
        for (radius, nn), a in zip(G.combos(kind), refs):
            label = f"{kind} P={P} radius={radius} max_nn={nn}"
            assert NR.set_margin(a) > MARGIN, (label, NR.set_margin(a))
            assert a["bin_margin"] >= EXACT and a["swap_gap_min"] >= EXACT and a["v_rel_min"] >= EXACT, \
                (label, a["bin_margin"], a["swap_gap_min"], a["v_rel_min"])
            seen |= set(np.minimum(a["m"], 3).tolist())
            live = a["m"] > 0
            assert np.abs(a["fpfh"][live].reshape(-1, 3, 11).sum(axis=2) - 200).max(initial=0) < 1e-9, label
    assert seen == {0, 1, 2, 3} or kind == "lattice", (kind, seen)      # the radii leave rows with m = 0, 1 and 2
    if kind == "edge":      # exact |a1| = |a2| ties (rows of one plane), and pairs that are not
        pts, nrm, _ = fpfh_case(kind, 5000)
        same = (nrm[:200, None, :] == nrm[None, :200, :]).all(axis=2)
        assert same.any() and not same.all()
    if kind == "lattice":   # delta parallel to n: |v| = 0 exactly
        pts, nrm, refs = fpfh_case(kind, 5000)
        assert (refs[0]["counts"][:, [5, 16, 27]].min(axis=1) > 0).any()
    if kind == "twice":
        assert np.unique(fpfh_case(kind, 5000)[0], axis=0).shape[0] == 4500


def test_preconditions_of_the_matching_features():
    for n, m, seed in ((5000, 5000, 1), (257, 129, 2)):
        near = G.feature_nn(G.features(n, seed), G.features(m, seed + 100))
        gap = (near["second"] - near["d2"]) / near["second"]
        assert (gap > MARGIN).all(), gap.min()
        back = G.feature_nn(G.features(m, seed + 100), G.features(n, seed))
        assert ((back["second"] - back["d2"]) / back["second"] > MARGIN).all()
        assert 0 < G.match(G.features(n, seed), G.features(m, seed + 100), True).shape[0] < n


def test_the_confidence_rule_survives_a_tiny_inlier_share():
    from scene_utils.registration import _ransac_enough
    for f in (G.enough, _ransac_enough):
        # (8 / 5000) ** 8 = 4e-23: 1 - p rounds to 1, log(1 - p) to 0 - a division by zero, or numpy's -inf and an early stop
        assert f(16384, 8, 5000, 8, 0.999) is False and f(10 ** 9, 8, 5000, 8, 0.999) is False
        assert f(10 ** 30, 8, 5000, 8, 0.999) is True                       # 6.9 / 4.3e-23 = 1.6e23 trials would do
        assert f(10 ** 12, 1, 10 ** 6, 8, 0.999) is False and f(1, 0, 5000, 3, 0.999) is False and f(1, -1, 5000, 3, 0.999) is False
        assert f(1, 5000, 5000, 8, 0.999) is True and f(34, 2500, 5000, 4, 0.999) is False and f(108, 2500, 5000, 4, 0.999) is True
        assert f(1, 10, 10 ** 6, 8, 0.0) is True                           # confidence 0: log 1 = 0 trials needed


def test_reference_ransac_finds_the_planted_motion():
    src, tgt, pairs, T, md = G.ransac_case(256, 5)
    r = G.ransac(src, tgt, pairs, md, 3, 0.9, seed=3, max_iteration=4000, confidence=1.0, batch=1000)
    assert r["trial"] >= 0 and r["count"] >= 0.4 * 256 and NR.displacement(r["T"], T, src) < md
    one = G.ransac(src, tgt, pairs, md, 3, 0.9, seed=3, max_iteration=4000, confidence=1.0, batch=4000)
    assert one["trial"] == r["trial"] and one["count"] == r["count"] and one["sum_d2"] == r["sum_d2"]


@functools.lru_cache(maxsize=None)
def e2e():
    src, tgt, T, v = G.e2e()
    return src, tgt, T, v, G.pipeline(src, tgt, v)


def test_reference_pipeline_recovers_the_planted_motion_and_icp_from_the_identity_does_not():
    src, tgt, T, v, p = e2e()
    assert 1700 <= p["src_down"].shape[0] <= 2300 and 1700 <= p["tgt_down"].shape[0] <= 2300
    angle = np.degrees(np.arccos((np.trace(T[:3, :3]) - 1) / 2))
    extent = np.ptp(tgt.astype(np.float64), axis=0).max()
    assert angle > 90 and np.linalg.norm(T[:3, 3]) > 2 * extent
    assert p["ransac"]["trial"] >= 0 and NR.displacement(p["ransac"]["T"], T, p["src_down"]) < 1.5 * v
    reached = NR.displacement(p["icp"]["T"], T, p["src_down"])
    print(f"reference: pairs {p['pairs'].shape[0]}, inliers {p['ransac']['count']}, trial {p['ransac']['trial']}, after RANSAC "
          f"{NR.displacement(p['ransac']['T'], T, p['src_down']):.4g}, after ICP {reached:.4g}")
    assert abs(reached - G.E2E_REFERENCE_AFTER_ICP) <= 0.01 * G.E2E_REFERENCE_AFTER_ICP, reached      # the GPU test's bound is twice this
    plain = RR.icp(p["src_down"], p["tgt_down"], 5 * v)
    assert NR.displacement(plain["T"], T, p["src_down"]) > extent
