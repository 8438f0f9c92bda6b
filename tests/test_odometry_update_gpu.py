"""gsr_odometry_update on the device against the float64 restatement of tests/odometry_reference.py, on the cases
tests/test_odometry_cpu.py checks on the reference alone.

Bounds (those of tests/test_icp_plane_gpu.py).  n exact: the association is the same sequence of separately rounded float64
operations on both sides.  Sums, fitness and RMSE: 1e-12 relative - float64 sums of at most 66 049 non-negative terms in another
order.  Transform: the largest displacement of an unprojected source pixel between the kernel's T and the reference's <= 1e-9 x the
extent of those points; tests/test_odometry_cpu.py shows cond(J^T J) <= 1e6 for every case, so two float64 solves of it agree to
1e-10.  dR: orthonormal to 1e-14 (a product of three exact rotations); row 3 exact."""
import numpy as np
import pytest
import torch

import odometry_reference as OR
import scene_utils as S
from diff_gaussian_rasterization import _C

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits64(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint64)


def rel(a, b):
    return abs(a - b) / abs(b) if b else abs(a)


def levels(c):
    K, w, h = tuple(c["K"]), c["w"], c["h"]
    return (S.OdometryLevel(dev(c["src_I"]), dev(c["src_D"]), None, K, w, h),
            S.OdometryLevel(dev(c["tgt_I"]), dev(c["tgt_D"]), dev(c["tgt_grad"]), K, w, h))


def check_step(c, ref, T, stats, what):
    """the kernel's (T, stats) of one step against the reference's, to the bounds of the module docstring"""
    T, st = T.cpu().numpy(), stats.tolist()
    print(f"{what}: n={ref['n']} status={ref['status']} sum_rD2 rel {rel(st[4], ref['sum_rD2']):.3g} sum_rI2 rel "
          f"{rel(st[5], ref['sum_rI2']):.3g}", end="")
    assert st[0] == ref["n"] and st[3] == ref["status"] and st[6] == 0.0 and st[7] == 0.0, (what, st, ref["n"], ref["status"])
    assert rel(st[1], ref["fitness"]) <= 1e-12 and rel(st[2], ref["rmse"]) <= 1e-12, (what, st)
    assert rel(st[4], ref["sum_rD2"]) <= 1e-12 and rel(st[5], ref["sum_rI2"]) <= 1e-12, (what, st)
    assert T[3].tolist() == [0.0, 0.0, 0.0, 1.0]
    if ref["status"] != 0:
        print()
        assert np.array_equal(T.view(np.uint64), np.asarray(c["T"], dtype=np.float64).view(np.uint64)), what
        return
    points = OR.unproject(c["src_D"], c["K"])
    err, bound = OR.displacement(T, ref["T"], points), 1e-9 * OR.extent(c)
    print(f" displacement {err:.3g} (bound {bound:.3g})")
    assert err <= bound, (what, err, bound)
    dR = (T @ np.linalg.inv(c["T"]))[:3, :3]
    assert np.abs(dR @ dR.T - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(dR) - 1.0) <= 1e-14, what


@pytest.mark.parametrize("name", OR.UPDATE_CASES)
def test_update_against_the_reference(name):
    c = OR.update_case(name)
    src, tgt = levels(c)
    T0 = torch.from_numpy(np.asarray(c["T"], dtype=np.float64))
    for lam in c["lambdas"]:
        ref = OR.run_update(c, lam)
        assert ref["status"] == c["status"]
        T, stats = S.odometry_update(src, tgt, T0, lam, c["depth_diff_max"])
        check_step(c, ref, T, stats, f"{name} lambda={lam}")
        # apply=False: the same stats and status, T bit for bit as it came
        Tn, stats_n = S.odometry_update(src, tgt, T0, lam, c["depth_diff_max"], apply=False)
        assert np.array_equal(bits64(Tn), bits64(T0)) and np.array_equal(bits64(stats_n), bits64(stats)), (name, lam)
        # two runs: identical bits
        T2, stats2 = S.odometry_update(src, tgt, T0, lam, c["depth_diff_max"])
        assert np.array_equal(bits64(T2), bits64(T)) and np.array_equal(bits64(stats2), bits64(stats)), (name, lam)
        if ref["status"] != 0:
            assert np.array_equal(bits64(T), bits64(T0)), (name, lam)


def test_a_step_from_a_transformation_that_is_not_the_identity():
    """T <- [dR, t] T with a T that has every entry set: the product, not only dT"""
    c = dict(OR.update_case("size_64x64"))
    c["T"] = OR.rigid((0.2, 0.5, -0.4), 0.3, (0.004, 0.003, -0.005))
    src, tgt = levels(c)
    ref = OR.run_update(c, OR.LAMBDA)
    assert ref["status"] == 0 and ref["cond"] <= 1e6
    T, stats = S.odometry_update(src, tgt, torch.from_numpy(c["T"]), OR.LAMBDA, c["depth_diff_max"])
    check_step(c, ref, T, stats, "size_64x64 from a small motion")


def test_planes_of_another_dtype_or_layout_are_copied_not_misread():
    """float64 planes, and views with a stride, give the bits of contiguous float32 planes; a level with one plane left on the
    host is refused before any launch"""
    c = OR.update_case("size_20x13")
    src, tgt = levels(c)
    T0 = torch.eye(4, dtype=torch.float64)
    T, stats = S.odometry_update(src, tgt, T0, OR.LAMBDA, c["depth_diff_max"])
    wide = torch.zeros(13, 32, device="cuda")
    wide[:, :20] = src.depth
    grad_t = tgt.grad.permute(1, 2, 0).contiguous().permute(2, 0, 1)                # [4,13,20] with the plane index innermost
    assert not wide[:, :20].is_contiguous() and not grad_t.is_contiguous()
    odd_s = src._replace(intensity=src.intensity.double(), depth=wide[:, :20])
    odd_t = tgt._replace(depth=tgt.depth.double(), grad=grad_t)
    T2, stats2 = S.odometry_update(odd_s, odd_t, T0, OR.LAMBDA, c["depth_diff_max"])
    assert np.array_equal(bits64(T2), bits64(T)) and np.array_equal(bits64(stats2), bits64(stats))
    for bad_s, bad_t in ((src._replace(depth=src.depth.cpu()), tgt), (src, tgt._replace(grad=tgt.grad.cpu())),
                         (src, tgt._replace(intensity=tgt.intensity.cpu()))):
        with pytest.raises(_C.GsrError, match="no CPU path"):
            S.odometry_update(bad_s, bad_t, T0)
    with pytest.raises(ValueError, match="target_level.grad"):
        S.odometry_update(src, tgt._replace(grad=tgt.grad[:3]), T0)
    with pytest.raises(ValueError, match="source_level.depth"):
        S.odometry_update(src._replace(depth=src.depth[:12]), tgt, T0)


def test_error_codes():
    lib = _C.lib()
    c = OR.update_case("size_20x13")
    src, tgt = levels(c)
    T, st = torch.eye(4, dtype=torch.float64, device="cuda"), torch.zeros(8, dtype=torch.float64, device="cuda")
    need = lib.gsr_odometry_workspace_bytes(20, 13)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    import ctypes as C
    p = _C.ptr

    def call(w=20, h=13, K=c["K"], planes=(src.intensity, src.depth, tgt.intensity, tgt.depth, tgt.grad), lam=0.968, ddm=0.03, T=T, st=st,
             ws=ws, nbytes=need):
        Kc = None if K is None else (C.c_double * 4)(*K)
        return lib.gsr_odometry_update(w, h, Kc, *[p(t) for t in planes], lam, ddm, 1, p(T), p(st), p(ws), nbytes, _C._stream())
    nan, inf = float("nan"), float("inf")
    bad = [dict(K=None), dict(T=None), dict(st=None), dict(ws=None), dict(w=0), dict(h=-3), dict(w=1 << 15, h=1 << 15),
           dict(K=(0.0, 17.5, 9.7, 5.8)), dict(K=(17.5, -1.0, 9.7, 5.8)), dict(K=(17.5, 17.5, nan, 5.8)), dict(K=(17.5, 17.5, 9.7, inf)),
           dict(K=(inf, 17.5, 9.7, 5.8)), dict(lam=-0.01), dict(lam=1.01), dict(lam=nan), dict(ddm=0.0), dict(ddm=-1.0), dict(ddm=nan)]
    for k in range(5):
        planes = [src.intensity, src.depth, tgt.intensity, tgt.depth, tgt.grad]
        planes[k] = None
        bad.append(dict(planes=tuple(planes)))
    for kw in bad:
        assert call(**kw) == -1, kw                    # GSR_ERR_INVALID_ARGUMENT, before any launch
        assert "odometry_update" in _C.last_error()
    assert call(nbytes=need - 1) == -5                 # GSR_ERR_STATE_TOO_SMALL
    torch.cuda.synchronize()
    assert torch.equal(T.cpu(), torch.eye(4, dtype=torch.float64)) and float(st.abs().sum()) == 0.0
    assert call() == 0
    assert st.tolist()[0] == OR.run_update(c, 0.968)["n"]
