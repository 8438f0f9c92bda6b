"""One update each of the point-to-point, point-to-plane and coloured ICP and of the dense odometry, bit for bit what the commit
before the three 6-unknown updates were folded into one final kernel computed (csrc/solve6_common.h k_gn6_final).

tests/golden/gn_updates_parent.npz was recorded on the MI355X from a build of that commit by `cases()` below: for every case the 16
float64 of T and the 8 float64 of the stats as uint64, and a float64 checksum of every input array.  No tolerance, no case left
out.  The cases (tests/gn_updates_cases.py) are the smallest that reach each branch of the shared code;
tests/test_gn_updates_cpu.py shows on the float64 references that none of them pins a pivot that could fall either way."""
import functools
import os

import numpy as np
import pytest
import torch

import gn_updates_cases as G
import scene_utils as S

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gn_updates_parent.npz")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits64(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint64).ravel().copy()


@functools.lru_cache(maxsize=None)
def icp_device(Ps, variant):
    return {k: (v if k == "T0" else dev(v)) for k, v in G.icp_inputs(Ps, variant).items()}


@functools.lru_cache(maxsize=None)
def odometry_levels(name):
    c = G.odometry_case(name)
    K, w, h = tuple(c["K"]), c["w"], c["h"]
    return (S.OdometryLevel(dev(c["src_I"]), dev(c["src_D"]), None, K, w, h),
            S.OdometryLevel(dev(c["tgt_I"]), dev(c["tgt_D"]), dev(c["tgt_grad"]), K, w, h))


def run(name):
    """one case through the public call -> (T bits uint64 [16], stats bits uint64 [8])"""
    if name in G.ICP_CASES:
        est, Ps, variant, lam = G.ICP_CASES[name]
        a = icp_device(Ps, variant)
        kw = {}
        if est != "point":
            kw["target_normals"] = a["nrm"]
        if est == "colored":
            kw.update(source_colors=a["scol"], target_colors=a["tcol"], target_gradients=a["grd"], lambda_geometric=lam)
        T, stats = S.icp_update(a["src"], a["tgt"], a["corr"], torch.from_numpy(a["T0"]), **kw)
    else:
        case, lam, apply = G.ODOMETRY_CASES[name]
        c = G.odometry_case(case)
        src, tgt = odometry_levels(case)
        T, stats = S.odometry_update(src, tgt, torch.from_numpy(np.asarray(c["T"], dtype=np.float64)), lam, c["depth_diff_max"],
                                     apply=apply)
    return bits64(T), bits64(stats)


def cases():
    """{name: (T bits, stats bits)} of every case: what the fixture holds"""
    return {name: run(name) for name in G.NAMES}


@functools.lru_cache(maxsize=None)
def gold():
    """-> ({name: (T bits, stats bits)}, {key: checksum}) of the fixture: names [N], T uint64 [N,16], S uint64 [N,8], sum_keys, sums"""
    g = np.load(GOLDEN)
    assert g["T"].dtype == np.uint64 and g["S"].dtype == np.uint64
    return ({str(n): (g["T"][i], g["S"][i]) for i, n in enumerate(g["names"])},
            {str(k): float(v) for k, v in zip(g["sum_keys"], g["sums"])})


def test_the_inputs_are_the_recorded_ones():
    outputs, sums = gold()
    assert sums == G.input_checksums()
    assert sorted(outputs) == sorted(G.NAMES)


@pytest.mark.parametrize("name", G.NAMES)
def test_update_is_bit_for_bit_what_it_was(name):
    T_gold, stats_gold = gold()[0][name]
    T, stats = run(name)
    assert T.dtype == np.uint64 and T.shape == (16,) and stats.dtype == np.uint64 and stats.shape == (8,)
    st = stats.view(np.float64)
    if name in G.ICP_CASES:
        est, Ps, variant, _ = G.ICP_CASES[name]
        assert st[3] == G.icp_expected_status(name)
        if Ps in G.ICP_EXACT_N:
            assert st[0] == G.ICP_EXACT_N[Ps]                                  # (5 and 6: on either side of the n < 6 rule)
        start = G.icp_inputs(Ps, variant)["T0"]
        applied = True
    else:
        case, _, applied = G.ODOMETRY_CASES[name]
        assert st[3] == G.odometry_case(case)["status"]
        start = np.asarray(G.odometry_case(case)["T"], dtype=np.float64)
    if st[3] != 0.0 or not applied:                                            # T as it came, bit for bit
        assert np.array_equal(T, np.ascontiguousarray(start).view(np.uint64).ravel()), name
    assert np.array_equal(T, T_gold), (name, T.view(np.float64), T_gold.view(np.float64))
    assert np.array_equal(stats, stats_gold), (name, st, stats_gold.view(np.float64))
