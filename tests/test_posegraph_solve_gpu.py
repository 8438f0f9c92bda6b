"""gsr_posegraph_solve on the device: from the reference's linearisation and a given lambda.

|(H + lambda I) delta + b| <= 2 cg_rtol |b|, evaluated on the host in float64 from the reference's matrix (the factor 2: the
recurrence's residual against the true one).  |delta - delta*| <= cond (achieved relative residual) |delta*| with delta* the dense
solve and cond from numpy; "achieved" is the TRUE relative residual of the kernel's delta, evaluated on the host, plus that of
delta* itself and one rounding of the evaluation - the recurrence's own figure can lie below float64's floor.  Rows of fixed
nodes are exactly 0."""
import numpy as np
import pytest
import torch

import posegraph_reference as PR
from diff_gaussian_rasterization import _C
from test_posegraph_linearize_gpu import dev, topology

pytestmark = pytest.mark.gpu
RTOL = 1e-12


def solve(G, lin, lam, cg_max, rtol=RTOL):
    lib = _C.lib()
    topo = topology(G)
    er = dev(PR.edge_records(lin)) if G.E else None
    nr = dev(PR.node_records(lin))
    delta = torch.full((G.N, 6), 7.0, dtype=torch.float64, device="cuda")
    stats = torch.zeros(4, dtype=torch.float64, device="cuda")
    ws = torch.empty(lib.gsr_posegraph_workspace_bytes(G.N, G.E), dtype=torch.uint8, device="cuda")
    _C.check(lib.gsr_posegraph_solve(G.N, G.E, _C.ptr(topo), _C.ptr(er), _C.ptr(nr), lam, rtol, cg_max, _C.ptr(delta), _C.ptr(stats),
                                     _C.ptr(ws), ws.numel(), None))
    return delta.cpu().numpy(), stats.tolist()


@pytest.mark.parametrize("G", PR.solve_cases(), ids=lambda G: G.name)
def test_solve_against_the_dense_solve(G):
    lin = PR.linearize(G, G.poses, G.mu)
    lam = 1e-5 * lin["maxdiag"]
    A, rhs, free = PR.dense_matrix(G, lin, lam)
    delta, st = solve(G, lin, lam, min(6 * G.N, 1000))
    x = delta[free].reshape(-1)
    bn = np.linalg.norm(rhs)
    true = np.linalg.norm(A @ x - rhs) / bn
    xs = np.linalg.solve(A, rhs)
    true_ref = np.linalg.norm(A @ xs - rhs) / bn
    cond = np.linalg.cond(A)
    err = np.linalg.norm(x - xs)
    bound = cond * (true + true_ref + np.finfo(float).eps) * np.linalg.norm(xs)
    print(f"{G.name}: products {st[0]:.0f}, reported |r|/|b| {st[1]:.3g}, true {true:.3g}, cond {cond:.3g}, |delta - delta*| {err:.3g} "
          f"(bound {bound:.3g})")
    assert st[2] == 0.0 and st[1] <= RTOL and st[3] == 0.0 and 1 <= st[0] <= min(6 * G.N, 1000)
    assert true <= 2 * RTOL
    assert err <= bound
    assert not delta[G.fixed].any()
    delta2, st2 = solve(G, lin, lam, min(6 * G.N, 1000))
    assert np.array_equal(delta.view(np.uint64), delta2.view(np.uint64)) and st == st2


def test_unconstrained_node_is_status_2():
    G = PR.zero_information()
    lin = PR.linearize(G, G.poses, G.mu)
    delta, st = solve(G, lin, 1e-5 * lin["maxdiag"], 18)
    assert st[2] == 2.0 and not delta.any()


def test_cg_max_iteration_of_one():
    G = PR.noisy_ring()
    lin = PR.linearize(G, G.poses, G.mu)
    delta, st = solve(G, lin, 1e-5 * lin["maxdiag"], 1)
    ref = PR.solve(G, lin, 1e-5 * lin["maxdiag"], solver="pcg", cg_max_iteration=1)
    print("one product: |r|/|b| =", st[1], "reference", ref[2])
    assert st[0] == 1.0 and st[2] == 1.0 and st[1] > RTOL
    assert abs(st[1] - ref[2]) <= 1e-9 * ref[2] and np.abs(delta - ref[0]).max() <= 1e-9 * np.abs(ref[0]).max()


def test_zero_right_hand_side_and_no_edges():
    G = PR.exact_ring()
    X = G.truth.copy()      # exact measurements at the truth: b = 0
    lin = PR.linearize(G, X, G.mu)
    lin["b"][:] = 0.0
    delta, st = solve(G, lin, 1e-3, 48)
    assert st[:3] == [0.0, 0.0, 0.0] and not delta.any()
