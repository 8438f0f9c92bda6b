"""The preconditions of tests/test_gn_updates_pinned_gpu.py, on the float64 references alone: every case the fixture pins has the
status it is there for, and where a step is taken cond(J^T J) <= 1e6 - the bound the GPU tests of the three families use - so the
fixture never pins a pivot that another summation order could turn."""
import numpy as np
import pytest

import gn_updates_cases as G
import odometry_reference as OR


@pytest.mark.parametrize("name", G.ICP_CASES)
def test_icp_case_has_what_it_is_there_for(name):
    est, Ps, variant, lam = G.ICP_CASES[name]
    r = G.icp_reference(name)
    print(f"{name}: n={r['n']} status={r['status']} cond={r.get('cond', float('nan')):.3g}")
    assert r["status"] == G.icp_expected_status(name)
    if Ps in G.ICP_EXACT_N:
        assert r["n"] == G.ICP_EXACT_N[Ps]
    if r["status"] == 0 and est != "point":
        assert r["cond"] <= 1e6
    if r["status"] != 0:
        assert np.array_equal(r["T"], G.icp_inputs(Ps, variant)["T0"])


def test_icp_inputs_are_the_handmade_ones():
    for Ps in G.ICP_SIZES:
        a = G.icp_inputs(Ps)
        Pt, corr = a["tgt"].shape[0], a["corr"]
        assert Pt == min(Ps, G.ICP_PT_MAX) and (corr[6::7] == -1).all() and int((corr >= Pt).sum()) == (1 if Ps > 7 else 0)
        ok = (corr >= 0) & (corr < Pt)
        assert np.array_equal(corr[ok], (np.arange(Ps) % Pt)[ok])
    assert (256 * 256 < np.array(G.ICP_SIZES)).sum() == 1 and 256 * 256 in G.ICP_SIZES      # the cap, and one row beyond it
    assert np.count_nonzero(G.icp_inputs(G.VARIANT_PS, "full_T")["T0"][:3]) == 12
    assert G.icp_inputs(G.VARIANT_PS, "offset")["tgt"].min() > 998.0


@pytest.mark.parametrize("name", sorted({c[0] for c in G.ODOMETRY_CASES.values()}))
def test_odometry_case_has_what_it_is_there_for(name):
    c = G.odometry_case(name)
    for lam in c["lambdas"]:
        r = OR.run_update(c, lam)
        print(f"{name} lambda={lam}: n={r['n']} status={r['status']} cond={r['cond']:.3g}")
        assert r["status"] == c["status"], (name, lam, r["status"])
        if r["status"] == 0:
            assert r["cond"] <= 1e6, (name, lam, r["cond"])
    if name == "size_16x16":
        assert c["w"] * c["h"] == 256
