"""gsr_posegraph_linearize and gsr_registration_information on the device against tests/posegraph_reference.py.

Bound: 1e-12 relative to the largest magnitude of each quantity in the case.  Every value is a few dozen float64 operations in
another order plus device atan2 / sincos within a couple of ulp (the argument of tests/test_odometry_update_gpu.py); the sums of
the information matrix are float64 sums of at most 65 537 terms in another order.  n is exact.  Two runs give identical bits."""
import ctypes as C

import numpy as np
import pytest
import torch

import posegraph_reference as PR
from diff_gaussian_rasterization import _C

pytestmark = pytest.mark.gpu


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))).cuda()


def topology(G):
    lib = _C.lib()
    ends = np.ascontiguousarray(np.stack([G.s, G.t], 1).astype(np.int32).reshape(G.E, 2))
    fixed = np.ascontiguousarray(G.fixed.astype(np.uint8))
    topo = torch.empty(lib.gsr_posegraph_topology_bytes(G.N, G.E), dtype=torch.uint8, device="cuda")
    scratch = np.zeros(topo.numel() // 4, np.int32)
    _C.check(lib.gsr_posegraph_topology(G.N, G.E, ends.ctypes.data_as(C.POINTER(C.c_int32)), fixed.ctypes.data_as(C.POINTER(C.c_uint8)),
                                        C.c_void_p(scratch.ctypes.data), _C.ptr(topo), topo.numel(), None))
    torch.cuda.synchronize()      # (the scratch must outlive the copy)
    return topo


def linearize(G, topo=None):
    lib = _C.lib()
    topo = topology(G) if topo is None else topo
    X, T, L, unc = dev(G.poses), dev(G.T), dev(G.L), dev(G.uncertain, np.uint8)
    edge = torch.zeros(max(G.E, 1), PR.EDGE_STRIDE, dtype=torch.float64, device="cuda")
    node = torch.zeros(G.N, PR.NODE_STRIDE, dtype=torch.float64, device="cuda")
    sc = torch.zeros(2, dtype=torch.float64, device="cuda")
    _C.check(lib.gsr_posegraph_linearize(G.N, G.E, _C.ptr(topo), _C.ptr(X), _C.ptr(T) if G.E else None, _C.ptr(L) if G.E else None,
                                         _C.ptr(unc) if G.E else None, G.mu, _C.ptr(edge) if G.E else None, _C.ptr(node), _C.ptr(sc),
                                         None))
    return edge[:G.E].cpu().numpy(), node.cpu().numpy(), sc.cpu().numpy()


def close(got, ref, what):
    assert got.shape == ref.shape
    if not ref.size:
        return
    scale, err = np.abs(ref).max(), np.abs(got - ref).max()
    print(f"  {what}: max |diff| {err:.3g}, scale {scale:.3g}")
    assert err <= 1e-12 * scale, (what, err, scale)


@pytest.mark.parametrize("G", PR.linearize_cases() + [PR.no_edges()], ids=lambda G: G.name)
def test_linearize_against_the_reference(G):
    edge, node, sc = linearize(G)
    lin = PR.linearize(G, G.poses, G.mu)
    re, rn = PR.edge_records(lin), PR.node_records(lin)
    print(G.name, "N", G.N, "E", G.E)
    for what, sl in (("e", slice(0, 6)), ("r", slice(6, 7)), ("w", slice(7, 8)), ("W", slice(8, 29)), ("g", slice(29, 35))):
        close(edge[:, sl], re[:, sl], what)
    close(node[:, :21], rn[:, :21], "H_ii")
    close(node[:, 21:], rn[:, 21:], "b")
    close(sc[:1], np.array([lin["F"]]), "F")
    close(sc[1:], np.array([lin["maxdiag"]]), "max diag(H)")
    assert not node[G.fixed].any()
    edge2, node2, sc2 = linearize(G)
    for a, b in ((edge, edge2), (node, node2), (sc, sc2)):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_linearize_rejects_bad_arguments():
    lib = _C.lib()
    G = PR.two_nodes()
    fixed = np.zeros(2, np.uint8)
    topo = torch.empty(lib.gsr_posegraph_topology_bytes(2, 1), dtype=torch.uint8, device="cuda")
    scratch = np.zeros(topo.numel() // 4, np.int32)
    hs = C.c_void_p(scratch.ctypes.data)
    for ends in ([0, 0], [0, 2], [-1, 1]):
        e = np.array(ends, np.int32)
        assert lib.gsr_posegraph_topology(2, 1, e.ctypes.data_as(C.POINTER(C.c_int32)), fixed.ctypes.data_as(C.POINTER(C.c_uint8)),
                                          hs, _C.ptr(topo), topo.numel(), None) == -1
    e = np.array([0, 1], np.int32)
    args = (e.ctypes.data_as(C.POINTER(C.c_int32)), fixed.ctypes.data_as(C.POINTER(C.c_uint8)), hs, _C.ptr(topo))
    assert lib.gsr_posegraph_topology(0, 1, *args, topo.numel(), None) == -1
    assert lib.gsr_posegraph_topology(2, -1, *args, topo.numel(), None) == -1
    assert lib.gsr_posegraph_topology(2, 1, *args, 16, None) == -5
    assert lib.gsr_posegraph_topology(2, 1, *args, topo.numel(), None) == 0
    torch.cuda.synchronize()
    ws = torch.empty(64, dtype=torch.uint8, device="cuda")
    d = torch.zeros(64, dtype=torch.float64, device="cuda")
    assert lib.gsr_posegraph_solve(2, 1, _C.ptr(topo), _C.ptr(d), _C.ptr(d), 1.0, 1e-12, 10, _C.ptr(d), _C.ptr(d), _C.ptr(ws), 64,
                                   None) == -5
    assert lib.gsr_posegraph_optimize(2, 1, _C.ptr(topo), None, _C.ptr(d), _C.ptr(d), _C.ptr(ws), 1.0, 10, 1e-6, 1e-6, 1e-12, 10,
                                      _C.ptr(d), _C.ptr(d), _C.ptr(d), _C.ptr(ws), 64, None) == -1


@pytest.fixture(scope="module")
def cloud():
    rng = np.random.default_rng(3)
    tgt = (rng.normal(size=(5000, 3)) * [4.0, 2.0, 1.0] + [1.0, -2.0, 0.5]).astype(np.float32)
    tgt[::97] = np.nan
    tgt[5, 1] = np.inf
    return tgt


@pytest.mark.parametrize("Ps", [1, 255, 256, 257, 65537])
def test_information_matrix(cloud, Ps):
    lib = _C.lib()
    rng = np.random.default_rng(Ps)
    idx = rng.integers(0, cloud.shape[0], Ps).astype(np.int32)
    if Ps > 1:
        idx[rng.random(Ps) < 0.2] = -1
        idx[1] = cloud.shape[0]      # past the end: no part
        idx[2] = 5                   # a non-finite target row
    ref, n = PR.information(cloud, idx)
    tgt, di = dev(cloud), dev(idx)
    out = []
    for _ in range(2):
        info = torch.full((6, 6), 7.0, dtype=torch.float64, device="cuda")
        stats = torch.full((4,), 7.0, dtype=torch.float64, device="cuda")
        ws = torch.empty(lib.gsr_information_workspace_bytes(Ps), dtype=torch.uint8, device="cuda")
        _C.check(lib.gsr_registration_information(cloud.shape[0], _C.ptr(tgt), Ps, _C.ptr(di), _C.ptr(info), _C.ptr(stats), _C.ptr(ws),
                                                  ws.numel(), None))
        out.append((info.cpu().numpy(), stats.cpu().numpy()))
    info, stats = out[0]
    print(f"Ps {Ps}: n {n}, max |diff| {np.abs(info - ref).max():.3g}, scale {np.abs(ref).max():.3g}")
    assert stats.tolist() == [float(n), 0.0, 0.0, 0.0] and info[3, 3] == n
    assert np.abs(info - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1.0) and np.array_equal(info, info.T)
    assert np.array_equal(info.view(np.uint64), out[1][0].view(np.uint64))


def test_information_with_no_correspondence_is_zero(cloud):
    lib = _C.lib()
    tgt, di = dev(cloud), dev(np.full(300, -1, np.int32))
    info = torch.full((6, 6), 7.0, dtype=torch.float64, device="cuda")
    stats = torch.full((4,), 7.0, dtype=torch.float64, device="cuda")
    ws = torch.empty(lib.gsr_information_workspace_bytes(300), dtype=torch.uint8, device="cuda")
    _C.check(lib.gsr_registration_information(cloud.shape[0], _C.ptr(tgt), 300, _C.ptr(di), _C.ptr(info), _C.ptr(stats), _C.ptr(ws),
                                              ws.numel(), None))
    assert not info.cpu().numpy().any() and not stats.cpu().numpy().any()
    assert lib.gsr_registration_information(cloud.shape[0], _C.ptr(tgt), 300, _C.ptr(di), _C.ptr(info), _C.ptr(stats), _C.ptr(ws), 8,
                                            None) == -5
    assert lib.gsr_registration_information(cloud.shape[0], None, 300, _C.ptr(di), _C.ptr(info), _C.ptr(stats), _C.ptr(ws),
                                            ws.numel(), None) == -1
