"""The coloured update and its drivers on the device (csrc/registration.hip gsr_icp_update_colored, csrc/colored.hip) against the
float64 restatement of tests/colored_reference.py.

Bounds of one update: those of tests/test_icp_plane_gpu.py, taken from it.  n exact.  Sums (sum |q - p|^2, the two residual sums,
RMSE and fitness): 1e-12 relative - float64 sums of at most 65 537 non-negative terms in another order.  Transform: the largest
displacement of a source row between the kernel's T and the reference's <= 1e-9 x the cloud's extent; tests/test_colored_cpu.py
shows cond(J^T J) <= 1e6 for every case, as that file requires of the plane update's.
End to end: the flat textured plane of colored_reference.plane_scene, whose conditions tests/test_colored_cpu.py establishes with
the reference alone."""
import functools
import os

import numpy as np
import pytest
import torch

import colored_reference as CR
import normals_reference as NR
import scene_utils as S
from test_icp_plane_gpu import bits64, dev, extent, rel

pytestmark = pytest.mark.gpu
H = NR.SPACING
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "register_and_merge_default.npz")


def colored_update(case, corr=None, T0=None, lam=CR.LAMBDA, **swap):
    src, scol, tgt, nrm, tcol, grd, T, c = case
    a = dict(src=src, scol=scol, tgt=tgt, nrm=nrm, tcol=tcol, grd=grd)
    a.update(swap)
    T = T if T0 is None else T0
    c = c if corr is None else corr
    got = S.icp_update(dev(a["src"]), dev(a["tgt"]), dev(c), torch.from_numpy(T), target_normals=dev(a["nrm"]),
                       source_colors=dev(a["scol"]), target_colors=dev(a["tcol"]), target_gradients=dev(a["grd"]),
                       lambda_geometric=lam)
    ref = CR.colored_update(a["src"], a["scol"], a["tgt"], a["nrm"], a["tcol"], a["grd"], c, T, lam)
    return got[0].cpu().numpy(), got[1].tolist(), ref


def check_stats(st, ref, status):
    assert st[0] == ref["n"] and st[3] == status and st[7] == 0.0
    assert rel(st[1], ref["fitness"]) <= 1e-12 and rel(st[2], ref["rmse"]) <= 1e-12
    assert rel(st[4], ref["sum_d2"]) <= 1e-12 and rel(st[5], ref["sum_rg2"]) <= 1e-12 and rel(st[6], ref["sum_ri2"]) <= 1e-12


@pytest.mark.parametrize("offset", [0.0, 1000.0])
@pytest.mark.parametrize("Ps", [6, 256, 257, 65537])
def test_update_against_the_reference(Ps, offset):
    case = CR.update_case(Ps, offset)
    src, tgt, T0 = case[0], case[2], case[6]
    for lam in (CR.LAMBDA, 0.5, 0.0):
        if lam == 0.0 and Ps == 6:
            continue                                             # (six photometric residuals alone do not fix six unknowns)
        T, st, ref = colored_update(case, lam=lam)
        assert ref["status"] == 0 and ref["cond"] <= 1e6
        err = NR.displacement(T, ref["T"], src)
        print(f"coloured update Ps={Ps} offset={offset} lambda={lam}: n={ref['n']} displacement {err:.3g} (bound "
              f"{1e-9 * extent(tgt):.3g}), sums rel {rel(st[4], ref['sum_d2']):.3g} {rel(st[5], ref['sum_rg2']):.3g} "
              f"{rel(st[6], ref['sum_ri2']):.3g}")
        check_stats(st, ref, 0.0)
        assert err <= 1e-9 * extent(tgt)
        assert T[3].tolist() == [0.0, 0.0, 0.0, 1.0]
        dR = (T @ np.linalg.inv(T0))[:3, :3]
        assert np.abs(dR @ dR.T - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(dR) - 1.0) <= 1e-14


@pytest.mark.parametrize("offset", [0.0, 1000.0])
@pytest.mark.parametrize("Ps", [6, 257, 65537])
def test_lambda_one_is_the_plane_update(Ps, offset):
    src, scol, tgt, nrm, tcol, grd, T0, corr = CR.update_case(Ps, offset)
    T, st, _ = colored_update(CR.update_case(Ps, offset), lam=1.0)
    Tp, sp = S.icp_update(dev(src), dev(tgt), dev(corr), torch.from_numpy(T0), target_normals=dev(nrm))
    Tp, sp = Tp.cpu().numpy(), sp.tolist()
    assert st[3] == sp[3] == 0.0 and st[6] == 0.0
    for a, b in zip(st[:6], sp[:6]):
        assert rel(a, b) <= 1e-12
    assert (np.abs(T - Tp) <= 1e-12 * np.maximum(np.abs(Tp), 1.0)).all(), np.abs(T - Tp).max()


def test_update_status_one_leaves_T():
    case = CR.update_case(256, 0.0)
    tgt, T0, corr = case[2], case[6], case[7]
    keep = np.flatnonzero(corr >= 0)[:5]
    few = np.full_like(corr, -1)
    few[keep] = corr[keep]
    for c, n in ((few, 5), (np.full_like(corr, -1), 0), (np.full_like(corr, tgt.shape[0]), 0)):      # (a row the target lacks)
        T, st, ref = colored_update(case, corr=c)
        assert np.array_equal(T.view(np.uint64), T0.view(np.uint64)) and ref["status"] == 1 and ref["n"] == n
        check_stats(st, ref, 1.0)


def test_update_status_two_on_one_untextured_plane():
    """one exact plane of one colour: the normals fix three unknowns and nothing fixes the others - the gradient is zero"""
    rng = np.random.default_rng(3)
    tgt = np.concatenate([rng.integers(-128, 128, size=(500, 2)) / 64.0, np.full((500, 1), 0.25)], axis=1).astype(np.float32)
    nrm = np.tile(np.float32([0, 0, 1]), (500, 1))
    tcol = np.full((500, 3), 0.5, np.float32)
    grd = S.estimate_color_gradients(dev(tgt), dev(tcol), dev(nrm), 0.2, 30).cpu().numpy()
    assert (grd == 0).all()
    src = (tgt[rng.integers(0, 500, size=300)] + np.float32([0.0, 0.0, 0.125])).astype(np.float32)
    scol = np.full((300, 3), 0.75, np.float32)
    corr = CR.RR.correspondences(CR.RR.nearest(src, tgt))
    T0 = np.eye(4)
    T, st, ref = colored_update((src, scol, tgt, nrm, tcol, grd, T0, corr))
    assert ref["status"] == 2 and np.array_equal(T.view(np.uint64), T0.view(np.uint64))
    check_stats(st, ref, 2.0)
    assert rel(st[5], 300 * 0.125 ** 2) <= 1e-12 and rel(st[6], 300 * 0.25 ** 2) <= 1e-12 and rel(st[2], 0.125) <= 1e-12


def test_rows_without_a_pair_or_with_non_finite_values_drop_out():
    case = CR.update_case(257, 0.0)
    src, scol, tgt, nrm, tcol, grd, T0, corr = case
    hit = np.unique(corr[corr >= 0])
    scol2, tcol2, grd2, nrm2, corr2 = scol.copy(), tcol.copy(), grd.copy(), nrm.copy(), corr.copy()
    scol2[0:200:9, 1] = np.nan
    scol2[4] = np.inf
    tcol2[hit[0::11], 2] = -np.inf
    grd2[hit[1::11]] = np.nan
    nrm2[hit[2::11], 0] = np.inf
    corr2[5:250:13] = -1
    T, st, ref = colored_update(case, corr=corr2, scol=scol2, tcol=tcol2, grd=grd2, nrm=nrm2)
    full = CR.colored_update(src, scol, tgt, nrm, tcol, grd, corr, T0)
    assert 6 <= ref["n"] < full["n"] - 40 and ref["status"] == 0
    check_stats(st, ref, 0.0)
    assert NR.displacement(T, ref["T"], src) <= 1e-9 * extent(tgt)


def test_a_workspace_one_byte_short_is_refused():
    from diff_gaussian_rasterization import _C
    lib = _C.lib()
    src, scol, tgt, nrm, tcol, grd, T0, corr = (dev(x) for x in CR.update_case(256, 0.0))
    stats = torch.zeros(8, dtype=torch.float64, device="cuda")
    need = lib.gsr_icp_colored_workspace_bytes(256)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    args = (256, _C.ptr(src), _C.ptr(scol), tgt.shape[0], _C.ptr(tgt), _C.ptr(nrm), _C.ptr(tcol), _C.ptr(grd), _C.ptr(corr), 0.968)
    before = T0.clone()
    assert lib.gsr_icp_update_colored(*args, _C.ptr(T0), _C.ptr(stats), _C.ptr(ws), need - 1, _C._stream()) == -5
    assert lib.gsr_icp_update_colored(*args, _C.ptr(T0), _C.ptr(stats), _C.ptr(ws), lib.gsr_icp_workspace_bytes(256),
                                      _C._stream()) == -5       # (the other two updates' size does not serve)
    assert torch.equal(T0, before) and stats.tolist() == [0.0] * 8
    assert lib.gsr_icp_update_colored(*args, _C.ptr(T0), _C.ptr(stats), _C.ptr(ws), need, _C._stream()) == 0
    assert stats.tolist()[3] == 0.0 and not torch.equal(T0, before)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene():
    src, scol, tgt, tcol, T, md = CR.plane_scene()
    nrm = NR.estimate(tgt, CR.PLANE_RADIUS, 30)[0].astype(np.float32)
    grd = CR.gradient(tgt, tcol, nrm, CR.PLANE_RADIUS, 30)["gradient"].astype(np.float32)
    ref = CR.icp_colored(src, scol, tgt, nrm, tcol, grd, md)
    return src, scol, tgt, tcol, T, md, nrm, grd, ref


def test_colored_icp_ends_where_the_reference_ends():
    src, scol, tgt, tcol, T_true, md, nrm, grd, ref = scene()
    s, sc, t, tc = dev(src), dev(scol), dev(tgt), dev(tcol)
    assert NR.displacement(ref["T"], T_true, src) <= 0.25 * H
    given = S.registration_colored_icp(s, sc, t, tc, md, target_normals=dev(nrm), target_gradients=dev(grd))
    own = S.registration_colored_icp(s, sc, t, tc, md, normal_radius=CR.PLANE_RADIUS, gradient_radius=CR.PLANE_RADIUS)
    for name, res in (("given", given), ("estimated", own)):
        err = NR.displacement(res.transformation.cpu().numpy(), ref["T"], src)
        print(f"coloured ICP ({name} normals and gradients): {res.iterations} iterations (reference {ref['iterations']}), "
              f"{err / H:.3g} spacings from the reference, {NR.displacement(res.transformation.cpu().numpy(), T_true, src) / H:.3g} "
              f"from the truth, fitness {res.fitness}, rmse {res.inlier_rmse:.3g}")
        assert res.converged and err <= 0.1 * H
        assert res.fitness == ref["fitness"] and rel(res.inlier_rmse, ref["rmse"]) <= 0.05      # (Euclidean, as every estimator's)
    # the pieces, estimated outside and handed in, give the bits of the run that estimates them inside
    n_dev = S.estimate_normals(t, CR.PLANE_RADIUS, 30)
    g_dev = S.estimate_color_gradients(t, tc, n_dev, CR.PLANE_RADIUS, 30)
    again = S.registration_icp(s, t, md, estimation="colored", source_colors=sc, target_colors=tc, target_normals=n_dev,
                               target_gradients=g_dev, max_iteration=50)
    assert np.array_equal(bits64(again.transformation), bits64(own.transformation)) and again.iterations == own.iterations
    # use_order changes no bit; check_every=0 runs the iterations asked for without a read-back
    plain = S.registration_colored_icp(s, sc, t, tc, md, target_normals=dev(nrm), target_gradients=dev(grd), use_order=False)
    assert np.array_equal(bits64(plain.transformation), bits64(given.transformation))
    blind = S.registration_colored_icp(s, sc, t, tc, md, target_normals=dev(nrm), target_gradients=dev(grd),
                                       max_iteration=given.iterations, check_every=0)
    assert blind.iterations == given.iterations and not blind.converged
    assert np.array_equal(bits64(blind.transformation), bits64(given.transformation))


def test_point_to_plane_icp_stays_away_on_the_same_scene():
    src, _, tgt, _, T_true, md, nrm, _, _ = scene()
    res = S.registration_icp(dev(src), dev(tgt), md, estimation="point_to_plane", target_normals=dev(nrm))
    err = NR.displacement(res.transformation.cpu().numpy(), T_true, src)
    print(f"point-to-plane ICP on the textured plane: {res.iterations} iterations, {err / H:.3g} spacings from the truth")
    assert err > H


def test_multiscale_reaches_the_truth():
    src, scol, tgt, tcol, T_true, _, _, _, _ = scene()
    last, levels = S.registration_multiscale(dev(src), dev(scol), dev(tgt), dev(tcol), list(CR.MULTISCALE_VOXELS),
                                             list(CR.MULTISCALE_ITERATIONS))
    errs = [NR.displacement(r.transformation.cpu().numpy(), T_true, src) / H for r in levels]
    print(f"multiscale: iterations {[r.iterations for r in levels]}, spacings from the truth {[round(e, 4) for e in errs]}")
    assert len(levels) == 2 and levels[-1] is last and errs[-1] <= 0.25
    # each level starts where the previous one ended: the second level alone from the first level's result is the same run
    v = CR.MULTISCALE_VOXELS[1]
    sd, sc = S.voxel_down_sample(dev(src), dev(scol), v)
    td, tc = S.voxel_down_sample(dev(tgt), dev(tcol), v)
    alone = S.registration_icp(sd, td, v, init=levels[0].transformation, max_iteration=CR.MULTISCALE_ITERATIONS[1],
                               estimation="colored", source_colors=sc, target_colors=tc, normal_radius=2 * v, gradient_radius=2 * v)
    assert np.array_equal(bits64(alone.transformation), bits64(last.transformation))
    # the other estimators pass through it too (the plane alone does not hold point-to-plane: it stays where it starts)
    for est in ("point_to_point", "point_to_plane"):
        res, lv = S.registration_multiscale(dev(src), None, dev(tgt), None, [2 * H], [5], estimation=est)
        assert len(lv) == 1 and res.iterations >= 1 and tuple(res.transformation.shape) == (4, 4)


def test_register_and_merge_colored_is_the_composition():
    src, scol, tgt, tcol, T_true, _, _, _, _ = scene()
    v = 1.5 * H
    pts, cols, res = S.register_and_merge(dev(src), dev(scol), dev(tgt), dev(tcol), voxel_size=v, estimation="colored")
    sd, sc = S.voxel_down_sample(dev(src), dev(scol), v)
    td, tc = S.voxel_down_sample(dev(tgt), dev(tcol), v)
    want = S.registration_icp(sd, td, 5.0 * v, estimation="colored", source_colors=sc, target_colors=tc, normal_radius=2.0 * v,
                              gradient_radius=2.0 * v)
    assert res.iterations == want.iterations and np.array_equal(bits64(res.transformation), bits64(want.transformation))
    assert torch.equal(pts, torch.cat([S.transform_points(dev(src), want.transformation), dev(tgt)]))
    assert torch.equal(cols, torch.cat([dev(scol), dev(tcol)]))
    err = NR.displacement(res.transformation.cpu().numpy(), T_true, src)
    print(f"register_and_merge coloured: {res.iterations} iterations, {err / H:.3g} spacings from the truth")
    assert err <= 0.25 * H
    merged, mcols, res2 = S.register_and_merge(dev(src), dev(scol), dev(tgt), dev(tcol), voxel_size=v, estimation="colored",
                                               merge_voxel_size=2 * H, lambda_geometric=0.9)
    assert merged.shape[0] < pts.shape[0] and mcols.shape == merged.shape and res2.iterations >= 1


def test_register_and_merge_default_is_what_it_was():
    """the fixture was written by the commit before the coloured estimator existed: same inputs, every output bit"""
    gold = np.load(GOLDEN)
    src, tgt, _, _ = NR.e2e_planes()
    rng = np.random.default_rng(77)
    scol = rng.random(src.shape, dtype=np.float32)
    tcol = rng.random(tgt.shape, dtype=np.float32)
    assert float(src.astype(np.float64).sum()) == float(gold["source_sum"]) and \
        float(tgt.astype(np.float64).sum()) == float(gold["target_sum"]) and \
        float(scol.astype(np.float64).sum() + tcol.astype(np.float64).sum()) == float(gold["color_sum"])      # the same inputs
    v = 1.5 * H
    Ns = src.shape[0]
    for kw in ({}, {"estimation": "point_to_point"}):
        pts, cols, res = S.register_and_merge(dev(src), dev(scol), dev(tgt), dev(tcol), voxel_size=v, **kw)
        assert np.array_equal(res.transformation.cpu().numpy().view(np.uint64), gold["transformation"].view(np.uint64))
        assert res.iterations == int(gold["iterations"]) and res.converged == bool(gold["converged"])
        assert res.fitness == float(gold["fitness"]) and res.inlier_rmse == float(gold["inlier_rmse"])
        assert np.array_equal(res.correspondences.cpu().numpy(), gold["correspondences"])
        assert np.array_equal(pts[:Ns].cpu().numpy().view(np.uint32), gold["moved"].view(np.uint32))
        assert torch.equal(pts[Ns:], dev(tgt)) and torch.equal(cols, torch.cat([dev(scol), dev(tcol)]))
    pts, cols, _ = S.register_and_merge(dev(src), dev(scol), dev(tgt), dev(tcol), voxel_size=v, merge_voxel_size=4 * H)
    assert np.array_equal(pts.cpu().numpy().view(np.uint32), gold["merged_points"].view(np.uint32))
    assert np.array_equal(cols.cpu().numpy().view(np.uint32), gold["merged_colors"].view(np.uint32))
