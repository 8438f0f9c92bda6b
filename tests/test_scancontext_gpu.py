"""GPU tests of csrc/scancontext.hip and scene_utils.scancontext against the float64 restatement in tests/scancontext_reference.py:
descriptors bit for bit on clouds whose points lie strictly inside their cells, the distance within 1e-5 and the shift exactly on
fixtures with one clear best shift (checked on the CPU in test_scancontext_reference_cpu.py), exact ties, the database, and one
end-to-end revisit: eight stored scans, the query turned by 137 degrees, to a pose-graph edge."""
import functools
import math

import numpy as np
import pytest
import torch

import scancontext_reference as SR
import scene_utils as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
MR, HO = SR.MAX_RANGE, SR.HEIGHT_OFFSET
GEOMETRIES = [(20, 60), (1, 1), (3, 7), (40, 120)]


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a.astype(np.float32)).view(np.uint32)


def _describe(points, R, S_, **kw):
    return S.scan_context(_dev(np.asarray(points, dtype=np.float32).reshape(-1, 3)), R, S_, MR, HO, **kw)


def _check_norms(ctx, R):
    """within R 2^-23 relative of the float64 norms of the kernel's own descriptor: R squares and adds and one square root"""
    got = ctx.norms.cpu().numpy().astype(np.float64)
    want = SR.norms(ctx.descriptor.cpu().numpy())
    assert (np.abs(got - want) <= R * 2.0 ** -23 * want).all(), np.abs(got - want).max()


# ---- the descriptor ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 257, 5000])
@pytest.mark.parametrize("R,S_", GEOMETRIES)
def test_descriptor_is_bit_identical_to_the_reference(R, S_, N):
    pts = SR.make_cloud(17 + N, N, R, S_, MR)
    ctx = _describe(pts, R, S_)
    assert tuple(ctx.descriptor.shape) == (1, R, S_) and tuple(ctx.norms.shape) == (1, S_)
    assert (ctx.rings, ctx.sectors, ctx.max_range, ctx.height_offset) == (R, S_, MR, HO)
    want = SR.descriptor(pts, R, S_, MR, HO)
    print(f"R={R} S={S_} N={N}: {np.count_nonzero(want)} cells, bits differ in {(_bits(ctx.descriptor[0]) != _bits(want)).sum()}")
    assert np.array_equal(_bits(ctx.descriptor[0]), _bits(want))
    if N == 0:
        assert not ctx.descriptor.any() and not ctx.norms.any()
    _check_norms(ctx, R)


def test_skipped_rows_and_clamped_heights():
    nan, inf = np.nan, np.inf
    pts = np.array([[1, 1, 5], [nan, 1, 9], [1, inf, 9], [1, 1, nan], [-inf, 2, 9], [0, 0, 9], [90, 0, 9], [80, 0, 9], [0, -80.5, 9],
                    [-3, 0.5, -7], [1, 1, 2], [20, -30, -2], [-40, 0.1, -0.0]], dtype=np.float32)
    ctx = _describe(pts, 20, 60)
    want = SR.descriptor(pts, 20, 60, MR, HO)
    assert np.array_equal(_bits(ctx.descriptor[0]), _bits(want))
    got = ctx.descriptor[0].cpu().numpy()
    assert np.count_nonzero(got) == 2 and got.max() == 7.0 and got[got > 0].min() == 2.0      # (1,1,5) and (-40,0.1,-0)
    _, ring, sector = SR.bins(pts, 20, 60, MR)
    assert got[ring[9], sector[9]] == 0.0 and got[ring[11], sector[11]] == 0.0      # negative heights clamp to 0: as empty
    _check_norms(ctx, 20)


def test_many_points_in_one_cell_give_the_max_whatever_the_order():
    R, S_ = 20, 60
    rng = np.random.default_rng(8)
    draw = SR.polar_draw(rng, 6000, R, S_)
    draw["ring"][:3000], draw["sector"][:3000] = 5, 7      # half of the points in ONE cell, over three workgroups
    draw["fr"][:3000] = 0.1 + 0.8 * rng.random(3000)
    pts = SR.polar_points(draw, R, S_, MR)
    a = _describe(pts, R, S_)
    b = _describe(pts[rng.permutation(len(pts))], R, S_)
    c = _describe(pts, R, S_)
    assert torch.equal(a.descriptor.view(torch.int32), b.descriptor.view(torch.int32))
    assert torch.equal(a.descriptor.view(torch.int32), c.descriptor.view(torch.int32))
    assert torch.equal(a.norms.view(torch.int32), b.norms.view(torch.int32))
    assert np.array_equal(_bits(a.descriptor[0]), _bits(SR.descriptor(pts, R, S_, MR, HO)))
    assert float(a.descriptor[0, 5, 7]) == float(np.float32(draw["z"][:3000].max().astype(np.float32) + np.float32(HO)))


def test_three_origins_in_one_launch_equal_three_launches():
    R, S_ = 20, 60
    pts = SR.make_cloud(9, 5000, R, S_, MR)
    origins = np.array([[0, 0, 0], [0, 1.5, 0], [0.7, -1.5, 0.2]], dtype=np.float32)
    frame = SR.tilted_frame()
    for kw in ({}, {"frame": frame}):
        together = _describe(pts, R, S_, origins=origins, **kw)
        assert tuple(together.descriptor.shape) == (3, R, S_)
        for b in range(3):
            alone = _describe(pts, R, S_, origins=origins[b:b + 1], **kw)
            assert torch.equal(together.descriptor[b].view(torch.int32), alone.descriptor[0].view(torch.int32)), b
            assert torch.equal(together.norms[b].view(torch.int32), alone.norms[0].view(torch.int32)), b
        assert not torch.equal(together.descriptor[0], together.descriptor[1])
    # origin 0 0 0 given explicitly is the NULL origin: the same bits as the reference
    assert np.array_equal(_bits(_describe(pts, R, S_, origins=origins[:1]).descriptor[0]), _bits(SR.descriptor(pts, R, S_, MR, HO)))


@pytest.mark.parametrize("R,S_", [(20, 60), (40, 120)])
def test_frame_gives_the_reference_bins_and_heights_within_rounding(R, S_):
    frame = SR.tilted_frame()
    levelled = SR.make_cloud(10, 5000, R, S_, MR)
    cloud = SR.to_cloud_frame(levelled, frame)
    ctx = _describe(cloud, R, S_, frame=frame)
    got = ctx.descriptor[0].cpu().numpy().astype(np.float64)
    want = SR.descriptor(cloud, R, S_, MR, HO, frame=frame)
    _, ring, sector = SR.bins(cloud, R, S_, MR, frame=frame)
    _, ring0, sector0 = SR.bins(levelled, R, S_, MR)
    assert np.array_equal(ring, ring0) and np.array_equal(sector, sector0)      # the round trip through the frame moved no point
    # 4 ulp of the largest |coordinate| plus |height_offset|: a 3-term float32 dot product and one add
    tol = 4.0 * float(np.spacing(np.float32(max(np.abs(cloud).max(), np.abs(levelled).max()) + abs(HO))))
    print(f"R={R} S={S_}: max |height - reference| = {np.abs(got - want).max():.3g}, allowed {tol:.3g}")
    assert np.array_equal(got > 0, want > 0)
    assert np.abs(got - want).max() <= tol
    _check_norms(ctx, R)


# ---- the distance ------------------------------------------------------------------------------------------------------------------------
def _context_of(desc):
    d = _dev(desc)
    return S.ScanContext(d, torch.sqrt((d * d).sum(dim=1)), int(d.shape[1]), int(d.shape[2]), MR, HO)


def _gpu_distance(q, db):
    d = _dev(db).reshape(len(db), q.shape[1], q.shape[2])
    out = S.scan_context_distance(_context_of(q), d, torch.sqrt((d * d).sum(dim=1)))
    return [t.cpu().numpy() for t in out], out


@functools.lru_cache(maxsize=None)
def _fixture(R, S_, K, B):
    q, db, shifts, variants = SR.distance_fixture(R, S_, K, B)
    return q, db, SR.distance(q, db)


@pytest.mark.parametrize("R,S_,K,B", SR.DISTANCE_CASES)
def test_distance_against_the_reference(R, S_, K, B):
    q, db, (dist, shift, variant, margin) = _fixture(R, S_, K, B)
    (gd, gs, gv), raw = _gpu_distance(q, db)
    assert gd.dtype == np.float32 and gs.dtype == np.int32 and gv.dtype == np.int32 and gd.shape == (K,)
    print(f"R={R} S={S_} K={K} B={B}: max |dist - reference| = {np.abs(gd - dist).max():.3g}, smallest margin {margin.min():.3g}")
    assert np.abs(gd.astype(np.float64) - dist).max() <= 1e-5
    clear = margin > 2e-5
    assert clear.all()
    assert np.array_equal(gs[clear], shift[clear]) and np.array_equal(gv[clear], variant[clear])
    again = _gpu_distance(q, db)[1]
    for a, b in zip(raw, again):      # two runs: identical bits
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_distance_with_an_empty_database():
    q = SR.distance_fixture(20, 60, 1, 2)[0]
    (gd, gs, gv), _ = _gpu_distance(q, np.zeros((0, 20, 60), dtype=np.float32))
    assert gd.shape == gs.shape == gv.shape == (0,)


@pytest.mark.parametrize("R,S_,period,turn", [(4, 12, 3, 1), (40, 120, 3, 1), (40, 120, 3, 65), (20, 60, 4, 2), (20, 64, 4, 63)])
def test_exact_ties_go_to_the_smallest_variant_then_the_smallest_shift(R, S_, period, turn):
    d = SR.one_hot_columns(R, S_, period)
    q = np.stack([np.roll(d, turn, axis=1)] * 2)
    table = SR.distance_table(q, d)
    want = SR.best_of(table)
    assert want[:3] == (0.0, turn % period, 0) and (table == 0).sum() == 2 * S_ // period      # the tie is real
    (gd, gs, gv), _ = _gpu_distance(q, d[None])
    assert (float(gd[0]), int(gs[0]), int(gv[0])) == (0.0, turn % period, 0)
    # a later variant wins where it is strictly better: variant 0 with one column's height moved to the next ring never reaches 0
    q2 = q.copy()
    q2[0, :, 0] = np.roll(q2[0, :, 0], 1)
    w2 = SR.best_of(SR.distance_table(q2, d))
    assert w2[:3] == (0.0, turn % period, 1)
    (gd, gs, gv), _ = _gpu_distance(q2, d[None])
    assert (float(gd[0]), int(gs[0]), int(gv[0])) == (0.0, turn % period, 1)


def test_zero_descriptors_and_zero_columns():
    R, S_ = 4, 12
    d = SR.one_hot_columns(R, S_, 3)
    zero = np.zeros((2, R, S_), dtype=np.float32)
    (gd, gs, gv), _ = _gpu_distance(zero, np.stack([d, zero[0]]))      # an all-zero query: distance exactly 1, variant 0, shift 0
    assert gd.tolist() == [1.0, 1.0] and gs.tolist() == [0, 0] and gv.tolist() == [0, 0]
    (gd, gs, gv), _ = _gpu_distance(d[None], zero[:1])                 # an all-zero database row
    assert gd.tolist() == [1.0] and gs.tolist() == [0] and gv.tolist() == [0]
    half = d.copy()
    half[:, ::2] = 0      # all-zero columns are left out of n: the others still match exactly
    (gd, gs, gv), _ = _gpu_distance(half[None], half[None])
    assert (float(gd[0]), int(gs[0]), int(gv[0])) == SR.best_of(SR.distance_table(half[None], half))[:3] == (0.0, 0, 0)
    # ... and counted nowhere else: against the full descriptor only the six shared columns are averaged
    (gd, _, _), _ = _gpu_distance(half[None], d[None])
    assert float(gd[0]) == 0.0


@pytest.mark.parametrize("R,S_", [(20, 60), (40, 120), (3, 7)])
def test_every_rotation_is_recovered_from_a_rotated_cloud(R, S_):
    draw = SR.polar_draw(np.random.default_rng(12), 6 * R * S_, R, S_)
    base = _describe(SR.polar_points(draw, R, S_, MR), R, S_)
    for k in (0, 1, S_ // 2, S_ - 1):
        turned = _describe(SR.polar_points(draw, R, S_, MR, shift=k), R, S_)
        dist, shift, variant = S.scan_context_distance(turned, base.descriptor, base.norms)
        assert int(shift[0]) == k and int(variant[0]) == 0 and abs(float(dist[0])) <= 1e-5, (k, int(shift[0]), float(dist[0]))


# ---- the database ------------------------------------------------------------------------------------------------------------------------
def test_scan_database_ranks_like_the_kernel_and_grows():
    R, S_, K, B = 20, 60, 65, 2
    q, rows, (dist, shift, variant, _) = _fixture(R, S_, K, B)
    db = S.ScanDatabase(DEV, R, S_, MR, HO)
    pts = torch.zeros(4, 3, device=DEV)
    for k in range(K):      # (65 rows: the buffer of 64 doubles once)
        db.add(f"kf{k}", _context_of(rows[k:k + 1]), points=pts if k == 3 else None)
    assert len(db) == K and "kf64" in db and "kf65" not in db and db["kf3"].points.data_ptr() == pts.data_ptr() and db["kf4"].points is None
    with pytest.raises(ValueError, match="already"):
        db.add("kf0", _context_of(rows[:1]))
    query = _context_of(q)
    gd, gs, gv = [t.cpu().numpy() for t in db.distances(query)]
    (kd, ks, kv), _ = _gpu_distance(q, rows)
    assert np.array_equal(_bits(gd), _bits(kd)) and np.array_equal(gs, ks) and np.array_equal(gv, kv)
    order = sorted(range(K), key=lambda r: (float(gd[r]), r))
    hits = db.query(query, top_k=4, max_distance=1.0)
    assert [h[0] for h in hits] == [f"kf{r}" for r in order[:4]]
    for (kf, d, yaw, var), r in zip(hits, order):
        assert d == float(gd[r]) and var == int(variant[r]) and yaw == int(shift[r]) * 2.0 * math.pi / S_
    skipped = db.query(query, exclude=(f"kf{order[0]}",), top_k=2, max_distance=1.0)
    assert [h[0] for h in skipped] == [f"kf{r}" for r in order[1:3]]
    cut = float(gd[order[1]])
    assert [h[0] for h in db.query(query, top_k=K, max_distance=cut)] == [f"kf{r}" for r in order if gd[r] <= cut]
    assert S.ScanDatabase(DEV, R, S_, MR, HO).query(query) == []


# ---- a revisit, end to end --------------------------------------------------------------------------------------------------------------
def test_revisit_turned_by_137_degrees_becomes_a_pose_graph_edge():
    """Eight scans of about 4000 points at eight places of a levelled scene of walls, boxes and poles; the query stands at place 5,
    turned by 137 degrees and 0.5 m to the side.  The yardstick of the edge is the existing registration: what the same
    generalized-ICP call reaches from the ground-truth pose (measured: fitness and RMSE are printed; DESIGN.md section 4 item 42
    records them), with 10 % allowed for the different entry into the basin; from the identity the same call must stay below."""
    scene = SR.make_scene()
    R, S_, mr, md, place = 20, 60, 40.0, 1.0, 5
    db = S.ScanDatabase(DEV, R, S_, mr, SR.SENSOR_HEIGHT)
    for i in range(8):
        pts = _dev(SR.take_scan(scene, SR.sensor_pose(i), 100 + i))
        db.add(i, S.scan_context(pts, R, S_, mr, SR.SENSOR_HEIGHT), points=pts)
    X_old, X_new = SR.sensor_pose(place), SR.sensor_pose(place, math.radians(-137.0), 0.5)
    T_gt = np.linalg.inv(X_new) @ X_old      # coordinates of the stored scan -> coordinates of the query: Rz(137 degrees), 0.5 m
    assert abs(math.degrees(math.atan2(T_gt[1, 0], T_gt[0, 0])) - 137.0) < 1e-9
    tgt = _dev(SR.take_scan(scene, X_new, 200))
    origins = np.array([[0, 0, 0], [0, -0.5, 0], [0, 0.5, 0]], dtype=np.float32)
    ctx = S.scan_context(tgt, R, S_, mr, SR.SENSOR_HEIGHT, origins=origins)
    hits = db.query(ctx, top_k=3)
    print("hits:", hits)
    assert hits[0][0] == place
    assert abs(math.degrees(hits[0][2]) - 137.0) <= 360.0 / S_

    src = db[place].points
    gt = S.registration_generalized_icp(src, tgt, md, init=T_gt, covariance_radius=2.0 * md)
    edge = S.scan_loop_closure_edge(db[place], tgt, context=ctx, max_correspondence_distance=md, origin_of_variant=origins)
    assert edge is not None
    T, info = edge
    assert T.dtype == torch.float64 and info.dtype == torch.float64 and T.is_cuda and info.is_cuda
    assert tuple(T.shape) == (4, 4) and tuple(info.shape) == (6, 6)
    got = S.evaluate_registration(src, tgt, md, T)
    none = S.registration_generalized_icp(src, tgt, md, init=None, covariance_radius=2.0 * md)
    print(f"from the ground truth: fitness {gt.fitness:.4f} rmse {gt.inlier_rmse:.4f}; from the yaw hint: fitness {got.fitness:.4f} "
          f"rmse {got.inlier_rmse:.4f}; from the identity: fitness {none.fitness:.4f} rmse {none.inlier_rmse:.4f}")
    assert got.fitness >= 0.9 * gt.fitness and got.inlier_rmse <= 1.1 * gt.inlier_rmse
    assert none.fitness < 0.9 * gt.fitness      # without the yaw hint the same call does not get there
    # the edge computed without a ready context takes the same way
    T2, _ = S.scan_loop_closure_edge(db[place], tgt, max_correspondence_distance=md, origin_of_variant=origins)
    assert torch.equal(T2, T)
    assert S.scan_loop_closure_edge(db[place], tgt, context=ctx, max_correspondence_distance=md, min_fitness=1.0,
                                    origin_of_variant=origins) is None

    graph = S.PoseGraph(DEV)
    graph.add_node(torch.from_numpy(X_old), fixed=True, id=place)
    graph.add_node(torch.from_numpy(X_new), id="query")
    graph.add_edge(place, "query", T, info, uncertain=True)
    assert len(graph.edges) == 1
