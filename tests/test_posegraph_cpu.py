"""The pose-graph reference (tests/posegraph_reference.py) on its own, the shared cases, and the host validation of
scene_utils.PoseGraph - no GPU.

Jacobian bound away from D = I.  The Jacobian is Open3D's linearisation: exact for vec6 at D = I, and for a residual e it differs
from the derivative of vec6 by terms of first order in |e| (the Euler-angle chart is not the exponential chart): per entry at most
|e| x the size of the column.  The test holds central differences to  2 |e|_2 max(1, |J|_max)  for the cases with |e| <= 0.1."""
import numpy as np
import pytest

import posegraph_reference as PR


def test_compose_and_vec6_are_inverse():
    rng = np.random.default_rng(0)
    for _ in range(50):
        d = np.concatenate([rng.uniform(-1.2, 1.2, 3), rng.uniform(-3, 3, 3)])
        assert np.abs(PR.vec6(PR.compose(d)) - d).max() <= 1e-14
    # the gimbal branch: sy <= 1e-6 gives gamma = 0 and still reproduces the matrix
    M = PR.compose([0.3, np.pi / 2, 0.2, 1, 2, 3])
    e = PR.vec6(M)
    assert e[2] == 0.0 and np.abs(PR.compose(e) - M).max() <= 1e-9


def _numeric_jacobian(Xs, Xt, T, h=1e-6):
    """central differences of e over delta_s (left product)"""
    J = np.zeros((6, 6))
    for j in range(6):
        d = np.zeros(6)
        d[j] = h
        J[:, j] = (PR.residual(PR.compose(d) @ Xs, Xt, T) - PR.residual(PR.compose(-d) @ Xs, Xt, T)) / (2 * h)
    return J


def test_jacobian_at_identity_matches_central_differences():
    G = PR.random_graph()
    worst = 0.0
    for k in range(0, G.E, 37):
        Xs, Xt = G.truth[G.s[k]], G.truth[G.t[k]]
        T = PR.relative(Xt, Xs)      # D = I
        worst = max(worst, np.abs(PR.jacobian(Xs, Xt, T) - _numeric_jacobian(Xs, Xt, T)).max())
        # delta_t enters with -J
        d = np.zeros(6)
        d[4] = 1e-6
        dt = (PR.residual(Xs, PR.compose(d) @ Xt, T) - PR.residual(Xs, PR.compose(-d) @ Xt, T)) / 2e-6
        assert np.abs(dt + PR.jacobian(Xs, Xt, T)[:, 4]).max() <= 1e-7
    print("jacobian at D = I: worst |J - central differences| =", worst)
    assert worst <= 1e-7


def test_jacobian_away_from_identity_is_within_the_second_order_term():
    n = 0
    for G in PR.linearize_cases():
        for k in range(G.E):
            Xs, Xt, T = G.poses[G.s[k]], G.poses[G.t[k]], G.T[k]
            e = PR.residual(Xs, Xt, T)
            if np.linalg.norm(e) > 0.1 or np.abs(Xs[:3, 3]).max() > 100:      # (far from the origin h = 1e-6 differences are too coarse)
                continue
            J = PR.jacobian(Xs, Xt, T)
            err = np.abs(J - _numeric_jacobian(Xs, Xt, T)).max()
            assert err <= 2 * np.linalg.norm(e) * max(1.0, np.abs(J).max()) + 1e-7, (G.name, k, err, np.linalg.norm(e))
            n += 1
    assert n > 100


def test_information_equals_the_row_by_row_sum():
    rng = np.random.default_rng(1)
    tgt = rng.normal(size=(40, 3)).astype(np.float32)
    tgt[5] = np.nan
    idx = rng.integers(-1, 40, 200)
    A, n = PR.information(tgt, idx)
    B, m = np.zeros((6, 6)), 0
    for i in idx:
        if i < 0 or not np.isfinite(tgt[i]).all():
            continue
        x, y, z = tgt[i].astype(np.float64)
        Gm = np.array([[0, z, -y, 1, 0, 0], [-z, 0, x, 0, 1, 0], [y, -x, 0, 0, 0, 1]])
        B += Gm.T @ Gm
        m += 1
    assert n == m and A[3, 3] == n and np.abs(A - B).max() <= 1e-12 * np.abs(B).max() and np.array_equal(A, A.T)
    assert PR.information(tgt, [-1, 5])[1] == 0 and not PR.information(tgt, [-1, 5])[0].any()


@pytest.mark.parametrize("G", PR.solve_cases(), ids=lambda G: G.name)
def test_solve_cases_are_well_conditioned(G):
    lin = PR.linearize(G, G.poses, G.mu)
    A, rhs, _ = PR.dense_matrix(G, lin, 1e-5 * lin["maxdiag"])
    cond = np.linalg.cond(A)
    print(G.name, "cond(H + lambda I) =", cond)
    assert cond <= 1e6
    # the reference's own PCG meets its stopping rule and the dense answer
    d0 = PR.solve(G, lin, 1e-5 * lin["maxdiag"])[0]
    d1, it, rel, st = PR.solve(G, lin, 1e-5 * lin["maxdiag"], solver="pcg")
    free = ~G.fixed
    true = [np.linalg.norm(A @ d[free].reshape(-1) - rhs) / np.linalg.norm(rhs) for d in (d0, d1)]      # not the recurrence's figure
    assert st == 0 and rel <= 1e-12 and true[1] <= 2e-12
    assert np.linalg.norm(d1 - d0) <= cond * (true[0] + true[1] + np.finfo(float).eps) * np.linalg.norm(d0)
    assert not d0[G.fixed].any() and not d1[G.fixed].any()


@pytest.fixture(scope="module")
def end_to_end():
    return {G.name: (G, PR.optimize(G)) for G in PR.end_to_end_cases()}


def test_reference_converges_on_every_end_to_end_case(end_to_end):
    for name, (G, res) in end_to_end.items():
        print(name, "status", res["status"], "iterations", res["iterations"], "F", res["F_start"], "->", res["F_end"])
        assert res["status"] != PR.ST_MAX_ITERATION and res["status"] in PR.CONVERGED, name
        assert res["F_end"] <= res["F_start"]
        assert np.array_equal(res["poses"][G.fixed], G.poses[G.fixed])


def _scipy_minimum(opt, G):
    """F at the minimum scipy.optimize.least_squares finds from the graph's start (an independent minimiser: its own Jacobian by
    finite differences, its own trust region)"""
    free = np.flatnonzero(~G.fixed)
    chol = [np.linalg.cholesky(G.L[k]).T for k in range(G.E)]      # |C e|^2 = e^T L e

    def fun(x):
        X = G.poses.copy()
        for a, i in enumerate(free):
            X[i] = PR.compose(x[6 * a:6 * a + 6]) @ G.poses[i]
        out = []
        for k in range(G.E):
            ce = chol[k] @ PR.residual(X[G.s[k]], X[G.t[k]], G.T[k])
            if G.uncertain[k]:      # mu r / (mu + r), split over the six components
                ce = ce * np.sqrt(G.mu / (G.mu + ce @ ce))
            out.append(ce)
        return np.concatenate(out)
    sol = opt.least_squares(fun, np.zeros(6 * free.size), xtol=1e-15, ftol=1e-15, gtol=1e-15)
    return float(np.sum(sol.fun ** 2))


TIGHT = dict(min_relative_increment=1e-12, min_relative_residual_increment=1e-14)      # below the 1e-6 that is compared


@pytest.mark.parametrize("G", [PR.false_loop_ring(), PR.two_fixed(), PR.quiet_ring()], ids=lambda G: G.name)
def test_scipy_least_squares_reaches_the_same_minimum(G):
    """The same F from the same start, within 1e-6 relative.  (random257 is not run here: finite differences over 1536 unknowns take
    minutes.  The case 10 km from the origin is not run either: there the optimiser stops at its first solve by the
    relative-increment rule - a documented limit, see test_posegraph_gpu.py - and there is no minimum to compare.)"""
    opt = pytest.importorskip("scipy.optimize")
    F, ref = _scipy_minimum(opt, G), PR.optimize(G, **TIGHT)
    print(G.name, "scipy F", F, "reference F", ref["F_end"], "relative", abs(F - ref["F_end"]) / F)
    assert ref["status"] in PR.CONVERGED
    assert abs(F - ref["F_end"]) <= 1e-6 * F


@pytest.mark.parametrize("G", [PR.two_nodes(), PR.exact_ring()], ids=lambda G: G.name)
def test_scipy_least_squares_agrees_that_exact_measurements_reach_zero(G):
    """F -> 0: a relative figure means nothing; both minimisers end below 1e-18 of F at the start (the bound of the exact ring in
    test_posegraph_gpu.py)"""
    opt = pytest.importorskip("scipy.optimize")
    F, ref = _scipy_minimum(opt, G), PR.optimize(G, **TIGHT)
    print(G.name, "scipy F", F, "reference F", ref["F_end"], "F at the start", ref["F_start"])
    assert ref["status"] in PR.CONVERGED and max(F, ref["F_end"]) <= 1e-18 * ref["F_start"]


def test_scipy_least_squares_on_the_noisy_ring_shows_the_bias_of_the_linearisation():
    """DEVIATION from the issue's 1e-6, stated here where it is asserted.  The iteration uses Open3D's Jacobian, exact only at D = I:
    per entry it is off by O(|e|) (test_jacobian_away_from_identity...), so the iteration's fixed point J~^T Lambda e = 0 is not the
    stationary point of F, and F there exceeds the minimum by O(|e|^2) relative.  On the ring of 16 at the issue's noise (1 cm,
    0.5 degrees) the reference ends 1.79e-6 above scipy (0.025991642 against 0.025991596); at half the noise (quiet_ring16, above)
    the gap is under 1e-6, as the second-order argument says.  Asserted: the reference is never BELOW the true minimum (beyond
    1e-9, scipy's own stopping), and the gap is within max_k |e_k|^2 at the solution - the second-order term itself, from the
    case's own residuals, not from the figure observed."""
    opt = pytest.importorskip("scipy.optimize")
    G = PR.noisy_ring()
    F, ref = _scipy_minimum(opt, G), PR.optimize(G, **TIGHT)
    X = ref["poses"]
    e2 = max(float(np.sum(PR.residual(X[G.s[k]], X[G.t[k]], G.T[k]) ** 2)) for k in range(G.E))
    gap = (ref["F_end"] - F) / F
    print("noisy_ring16: scipy F", F, "reference F", ref["F_end"], "relative gap", gap, "max |e|^2", e2)
    assert ref["status"] in PR.CONVERGED
    assert -1e-9 <= gap <= e2


def test_false_loop_is_switched_off_and_true_edges_are_kept(end_to_end):
    G, res = end_to_end["false_loop_ring16"]
    assert (G.s[-1], G.t[-1]) == PR.FALSE_EDGE and G.uncertain[-1]
    print("false edge w =", res["w"][-1], "smallest true w =", res["w"][:-1].min())
    assert res["w"][-1] < 0.01 and (res["w"][:-1] > 0.5).all()


def test_unconstrained_node_is_a_solver_failure():
    G = PR.zero_information()
    res = PR.optimize(G)
    assert res["status"] == PR.ST_SOLVER and np.array_equal(res["poses"], G.poses)
    res = PR.optimize(PR.no_edges())
    assert res["status"] == PR.ST_ZERO and res["iterations"] == 0


def test_random_graph_has_the_shapes_it_promises():
    G = PR.random_graph()
    ptr, adj = G.csr()
    deg = np.diff(ptr)
    assert G.N == 257 and G.E == 1300 and deg.max() > 64 and (deg == 1).sum() >= 3 and G.N % 64 and G.E % 256
    for i in range(G.N):      # ascending edge index per node, one bit for the end
        ks = adj[ptr[i]:ptr[i + 1]]
        assert (np.diff(ks >> 1) > 0).all()
        assert all((G.t if c & 1 else G.s)[c >> 1] == i for c in ks)


# ---- host validation of the Python surface -------------------------------------------------------------------------------------
def _graph():
    from scene_utils import PoseGraph
    g = PoseGraph(device="cpu")
    g.add_node(np.eye(4), fixed=True, id="a")
    g.add_node(np.eye(4), id="b")
    return g


def test_pose_and_transformation_must_be_rigid():
    g = _graph()
    bad = np.eye(4)
    bad[0, 0] = 2.0
    with pytest.raises(ValueError):
        g.add_node(bad)
    with pytest.raises(ValueError):
        g.add_node(np.eye(3))
    with pytest.raises(ValueError):
        g.add_edge("a", "b", bad)
    refl = np.diag([1.0, 1.0, -1.0, 1.0])
    with pytest.raises(ValueError):
        g.add_edge("a", "b", refl)
    with pytest.raises(ValueError):
        g.add_node(np.eye(4), id="a")      # a duplicate id


def test_information_must_be_symmetric_finite_and_nonnegative():
    g = _graph()
    L = np.eye(6)
    L[0, 1] = 1e-3
    with pytest.raises(ValueError, match="symmetric"):
        g.add_edge("a", "b", np.eye(4), L)
    L = np.eye(6)
    L[2, 2] = np.nan
    with pytest.raises(ValueError, match="finite"):
        g.add_edge("a", "b", np.eye(4), L)
    L = np.eye(6)
    L[4, 4] = -1.0
    with pytest.raises(ValueError, match="diagonal"):
        g.add_edge("a", "b", np.eye(4), L)
    with pytest.raises(ValueError):
        g.add_edge("a", "b", np.eye(4), np.eye(5))
    L = np.eye(6)
    L[0, 1], L[1, 0] = 1e-3, 1e-3 + 1e-13      # within 1e-9 max |L|
    g.add_edge("a", "b", np.eye(4), L)


def test_duplicates_self_loops_and_unknown_nodes_are_rejected():
    g = _graph()
    g.add_edge("a", "b", np.eye(4))
    with pytest.raises(ValueError, match="already joined"):
        g.add_edge("a", "b", np.eye(4))
    with pytest.raises(ValueError, match="already joined"):
        g.add_edge("b", "a", np.eye(4))
    with pytest.raises(ValueError, match="self-loop"):
        g.add_edge("a", "a", np.eye(4))
    with pytest.raises(ValueError, match="not in the graph"):
        g.add_edge("a", "c", np.eye(4))


def test_every_component_needs_a_fixed_node():
    g = _graph()
    g.add_edge("a", "b", np.eye(4))
    g.add_node(np.eye(4), id="c")
    g.add_node(np.eye(4), id="d")
    g.add_edge("c", "d", np.eye(4))
    with pytest.raises(ValueError, match="'c'"):
        g.optimize()
    from scene_utils import PoseGraph
    with pytest.raises(ValueError, match="no nodes"):
        PoseGraph(device="cpu").optimize()


def test_options_and_the_default_line_process_weight():
    g = _graph()
    g.add_edge("a", "b", np.eye(4), 100.0 * np.eye(6), uncertain=True)
    with pytest.raises(ValueError, match="max_correspondence_distance"):
        g.optimize()
    assert g._default_mu(0.05, 1.0, None) == pytest.approx(0.25)      # 1.0 x 0.05^2 x mean Lambda[3,3]
    assert g._default_mu(None, 1.0, 0.5) == 0.5
    with pytest.raises(ValueError):
        g.optimize(0.05, max_iteration=-1)
    with pytest.raises(ValueError):
        g.optimize(0.05, cg_rtol=float("nan"))
    with pytest.raises(ValueError):
        g.optimize(0.05, preference_loop_closure=0.0)


def test_a_cpu_graph_has_no_path():
    from diff_gaussian_rasterization import _C
    g = _graph()
    g.add_edge("a", "b", np.eye(4))
    with pytest.raises(_C.GsrError, match="no CPU path"):
        g.optimize()
    # updates and commit are plain tensor algebra and work anywhere
    assert all(np.array_equal(T.numpy(), np.eye(4)) for T in g.updates().values())
