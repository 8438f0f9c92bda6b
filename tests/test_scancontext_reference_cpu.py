"""CPU tests of the scan-context layer (scene_utils.scancontext, csrc/scancontext.hip): the new symbols resolve and the ABI version
stays; the numpy restatement of the two rules (tests/scancontext_reference.py), which the GPU tests compare against, is consistent
with itself; the fixtures the GPU tests use have the margins those tests rely on; and every bad argument is refused by the
library and by the Python layer without a device - which shows that the refusal comes before any device work."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import scancontext_reference as SR
import scene_utils as S
from scene_utils.scancontext import _yaw_start_pose
from diff_gaussian_rasterization import _C as GSR

INVALID = -1
MR, HO = SR.MAX_RANGE, SR.HEIGHT_OFFSET


# ---- the library ------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_resolve_and_abi_stays_7():
    lib = GSR.lib()
    for name in ("gsr_scan_context", "gsr_scan_context_distance"):
        assert name in GSR.EXPORTS and getattr(lib, name) is not None
    assert lib.gsr_abi_version() == 7 and GSR.ABI_VERSION == 7
    assert (GSR.SCAN_CONTEXT_MAX_RINGS, GSR.SCAN_CONTEXT_MAX_SECTORS, GSR.SCAN_CONTEXT_MAX_ORIGINS) == (40, 120, 16)


def _describe(N=4, points=256, frame=None, B=1, origins=None, rings=20, sectors=60, max_range=80.0, height_offset=2.0, desc=256,
              norms=256):
    """the call on fake device pointers (never dereferenced: every call made with them fails a check)"""
    f = None if frame is None else (C.c_float * 12)(*frame)
    o = None if origins is None else (C.c_float * len(origins))(*origins)
    p = [None if v is None else C.c_void_p(v) for v in (points, desc, norms)]
    return GSR.lib().gsr_scan_context(N, p[0], f, B, o, rings, sectors, max_range, height_offset, p[1], p[2], None)


def test_scan_context_rejects_bad_arguments_before_any_launch():
    nan, inf = math.nan, math.inf
    ident = (1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    bad = [dict(rings=0), dict(rings=41), dict(sectors=0), dict(sectors=121), dict(B=0, origins=(0,) * 3), dict(B=17, origins=(0,) * 51),
           dict(B=2), dict(N=-1), dict(N=1 << 30), dict(points=None), dict(desc=None), dict(norms=None),
           dict(max_range=0.0), dict(max_range=-1.0), dict(max_range=nan), dict(max_range=inf),
           dict(height_offset=nan), dict(height_offset=inf),
           dict(frame=(nan,) + ident[1:]), dict(frame=ident[:11] + (inf,)), dict(B=2, origins=(0, 0, 0, 0, nan, 0))]
    for kw in bad:
        assert _describe(**kw) == INVALID, kw
        assert GSR.last_error().startswith("scan_context:"), kw


def test_scan_context_distance_rejects_bad_arguments_before_any_launch():
    lib, fake = GSR.lib(), C.c_void_p(256)

    def call(rings=20, sectors=60, B=1, q=fake, qn=fake, K=3, db=fake, dn=fake, dist=fake, shift=fake, variant=fake):
        return lib.gsr_scan_context_distance(rings, sectors, B, q, qn, K, db, dn, dist, shift, variant, None)
    bad = [dict(rings=0), dict(rings=41), dict(sectors=0), dict(sectors=121), dict(B=0), dict(B=17), dict(K=-1), dict(K=1 << 30),
           dict(q=None), dict(qn=None), dict(db=None), dict(dn=None), dict(dist=None), dict(shift=None), dict(variant=None)]
    for kw in bad:
        assert call(**kw) == INVALID, kw
        assert GSR.last_error().startswith("scan_context_distance:"), kw
    assert call(K=0, db=None, dn=None, dist=None, shift=None, variant=None) == 0      # K = 0 is legal, nothing is launched


# ---- the reference is consistent with itself ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,S", [(20, 60), (1, 1), (3, 7), (40, 120)])
def test_generated_points_lie_in_the_cells_they_were_drawn_for(R, S):
    draw = SR.polar_draw(np.random.default_rng(3), 5000, R, S)
    for shift in (0, 1, S - 1):
        pts = SR.polar_points(draw, R, S, MR, shift)
        p, ring, sector = SR.bins(pts, R, S, MR)
        assert (ring == draw["ring"]).all() and (sector == (draw["sector"] + shift) % S).all()
        rho = np.hypot(p[:, 0], p[:, 1])
        assert rho.max() < 0.99 * MR and rho.min() > 0
        # no decision within 1e-3 of a cell of a boundary: float32 rounding (1e-7 relative) cannot change a bin
        fr, fs = rho * R / MR - ring, (np.arctan2(p[:, 1], p[:, 0]) % SR.TWO_PI) * S / SR.TWO_PI - sector
        assert fr.min() > 0.099 and fr.max() < 0.901 and fs.min() > 0.099 and fs.max() < 0.901


@pytest.mark.parametrize("R,S", [(20, 60), (3, 7), (40, 120)])
def test_rotating_a_cloud_by_k_sectors_shifts_the_columns_by_k(R, S):
    draw = SR.polar_draw(np.random.default_rng(4), 2000, R, S)
    base = SR.descriptor(SR.polar_points(draw, R, S, MR), R, S, MR, HO)
    assert (base > 0).any() and not np.array_equal(base, np.roll(base, 1, axis=1))
    for k in (0, 1, S // 2, S - 1):
        turned = SR.descriptor(SR.polar_points(draw, R, S, MR, shift=k), R, S, MR, HO)
        assert np.array_equal(turned, np.roll(base, k, axis=1)), k


def test_distance_of_a_descriptor_to_its_shifted_self_is_zero_at_that_shift():
    R, S = 20, 60
    base = SR.descriptor(SR.make_cloud(6, 3000, R, S, MR), R, S, MR, HO)
    for k in (0, 1, S // 2, S - 1):
        table = SR.distance_table(np.roll(base, k, axis=1)[None], base)
        d, shift, variant, margin = SR.best_of(table)
        assert abs(d) < 1e-12 and shift == k and variant == 0 and margin > 0.05, (k, d, shift, margin)


def test_reference_skips_what_the_rule_skips_and_clamps_heights():
    pts = np.array([[1, 1, 5], [np.nan, 1, 9], [1, np.inf, 9], [0, 0, 9], [90, 0, 9], [80, 0, 9], [-3, 0.5, -7], [1, 1, 2]], dtype=np.float32)
    _, ring, sector = SR.bins(pts, 20, 60, MR)
    assert (ring >= 0).tolist() == [True, False, False, False, False, False, True, True]
    d = SR.descriptor(pts, 20, 60, MR, HO)
    assert d[ring[0], sector[0]] == 7.0 and d[ring[6], sector[6]] == 0.0 and np.count_nonzero(d) == 1
    assert SR.norms(d)[sector[0]] == 7.0


def test_ties_go_to_the_smallest_variant_then_the_smallest_shift():
    R, S, period = 4, 12, 3
    d = SR.one_hot_columns(R, S, period)
    table = SR.distance_table(np.stack([np.roll(d, 1, axis=1), np.roll(d, 1, axis=1)]), d)
    assert set(np.unique(table)) == {0.0, 1.0}      # every cosine is exactly 0 or 1
    assert SR.best_of(table)[:3] == (0.0, 1, 0)     # shifts 1, 4, 7, 10 of both variants tie
    zero = SR.distance_table(np.zeros((2, R, S)), d)
    assert (zero == 1.0).all() and SR.best_of(zero)[:3] == (1.0, 0, 0)
    half = d.copy()
    half[:, ::2] = 0      # all-zero columns are left out of n: the remaining columns still match exactly
    assert SR.best_of(SR.distance_table(half[None], half))[:3] == (0.0, 0, 0)


@pytest.mark.parametrize("R,S,K,B", SR.DISTANCE_CASES)
def test_distance_fixtures_have_one_clear_best_shift_per_row(R, S, K, B):
    """what the GPU test relies on when it demands the reference's shift: best and second best differ by more than 2e-5"""
    q, db, shifts, variants = SR.distance_fixture(R, S, K, B)
    dist, shift, variant, margin = SR.distance(q, db)
    assert (margin > 2e-5).all(), margin.min()
    assert (shift == shifts).all() and (variant == variants).all()


def test_scene_ranks_the_true_place_first_in_the_reference():
    """the end-to-end fixture, judged by the reference alone: eight places, the query at place 5 turned by 137 degrees and moved
    0.5 m sideways"""
    scene = SR.make_scene()
    R, S, mr = 20, 60, 40.0
    db = np.stack([SR.descriptor(SR.take_scan(scene, SR.sensor_pose(i), 100 + i), R, S, mr, SR.SENSOR_HEIGHT) for i in range(8)])
    query = SR.take_scan(scene, SR.sensor_pose(5, math.radians(-137.0), 0.5), 200)
    assert 3500 <= len(query) <= 4000
    dist, shift, _, _ = SR.distance(SR.descriptor(query, R, S, mr, SR.SENSOR_HEIGHT)[None], db)
    assert int(np.argmin(dist)) == 5 and dist[5] < 0.4 and np.delete(dist, 5).min() > dist[5] + 0.1, dist
    assert abs(shift[5] * 360.0 / S - 137.0) <= 360.0 / S, shift[5]


# ---- the Python layer refuses bad arguments without a device ---------------------------------------------------------------------------
ScanContext = S.ScanContext


def _context(B=1, R=20, S=60, device="cpu", **kw):
    args = dict(descriptor=torch.zeros(B, R, S, device=device), norms=torch.zeros(B, S, device=device), rings=R, sectors=S,
                max_range=80.0, height_offset=2.0)
    args.update(kw)
    return ScanContext(**args)


def test_scan_context_argument_checks():
    pts = torch.zeros(5, 3)
    for kw, exc in ((dict(rings=0), ValueError), (dict(rings=41), ValueError), (dict(rings=2.0), TypeError), (dict(rings=True), TypeError),
                    (dict(sectors=0), ValueError), (dict(sectors=121), ValueError), (dict(sectors="60"), TypeError),
                    (dict(max_range=0.0), ValueError), (dict(max_range=math.inf), ValueError), (dict(max_range=math.nan), ValueError),
                    (dict(max_range="80"), TypeError), (dict(height_offset=math.nan), ValueError), (dict(height_offset=None), TypeError),
                    (dict(frame=np.eye(3)), ValueError), (dict(frame=np.full((3, 4), np.nan)), ValueError), (dict(frame="x"), ValueError),
                    (dict(origins=np.zeros((0, 3))), ValueError), (dict(origins=np.zeros((17, 3))), ValueError),
                    (dict(origins=np.zeros((2, 2))), ValueError), (dict(origins=[[0.0, math.inf, 0.0]]), ValueError)):
        with pytest.raises(exc):
            S.scan_context(pts, **kw)
    for bad in (torch.zeros(5, 2), torch.zeros(5, 3, dtype=torch.int32), np.zeros((5, 3)), None):
        with pytest.raises(ValueError, match="points"):
            S.scan_context(bad)
    with pytest.raises(GSR.GsrError, match="HIP device"):
        S.scan_context(pts, frame=np.eye(4), origins=[[0, 0.5, 0]])


def test_scan_context_distance_argument_checks():
    q = _context()
    with pytest.raises(TypeError, match="ScanContext"):
        S.scan_context_distance(torch.zeros(1, 20, 60), torch.zeros(2, 20, 60), torch.zeros(2, 60))
    for db, dn in ((torch.zeros(2, 20, 61), torch.zeros(2, 61)), (torch.zeros(2, 20, 60), torch.zeros(3, 60)),
                   (torch.zeros(20, 60), torch.zeros(60)), (torch.zeros(2, 20, 60, dtype=torch.int32), torch.zeros(2, 60))):
        with pytest.raises(ValueError):
            S.scan_context_distance(q, db, dn)
    for broken in (_context(descriptor=torch.zeros(1, 20, 59)), _context(norms=torch.zeros(2, 60)), _context(B=17),
                   _context(descriptor=torch.zeros(20, 60)), _context(rings=0), _context(sectors=121)):
        with pytest.raises(ValueError):
            S.scan_context_distance(broken, torch.zeros(2, 20, 60), torch.zeros(2, 60))
    with pytest.raises(TypeError):
        S.scan_context_distance(_context(rings=20.0), torch.zeros(2, 20, 60), torch.zeros(2, 60))
    with pytest.raises(GSR.GsrError, match="HIP device"):
        S.scan_context_distance(q, torch.zeros(2, 20, 60), torch.zeros(2, 60))


def test_scan_database_argument_checks():
    for kw, exc in ((dict(rings=0), ValueError), (dict(sectors=1.5), TypeError), (dict(max_range=-1.0), ValueError),
                    (dict(height_offset=math.inf), ValueError)):
        with pytest.raises(exc):
            S.ScanDatabase("cpu", **kw)
    db = S.ScanDatabase("cpu")
    assert len(db) == 0 and 3 not in db
    with pytest.raises(TypeError, match="ScanContext"):
        db.add(0, torch.zeros(1, 20, 60))
    for other in (_context(S=59), _context(R=19), _context(max_range=79.0), _context(height_offset=1.0)):
        with pytest.raises(ValueError, match="database's"):
            db.add(0, other)
        with pytest.raises(ValueError, match="database's"):
            db.distances(other)
    with pytest.raises(ValueError, match="points"):
        db.add(0, _context(), points=torch.zeros(4, 2))
    with pytest.raises(GSR.GsrError, match="HIP device"):
        db.add(0, _context())
    for kw, exc in ((dict(top_k=0), ValueError), (dict(top_k=1.0), TypeError), (dict(max_distance=-0.1), ValueError),
                    (dict(max_distance=math.nan), ValueError), (dict(max_distance="x"), TypeError)):
        with pytest.raises(exc):
            db.query(_context(), **kw)
    with pytest.raises(KeyError):
        db[0]


def test_scan_loop_closure_edge_argument_checks():
    entry = S.ScanEntry(0, _context(), torch.zeros(5, 3))
    pts = torch.zeros(5, 3)
    with pytest.raises(ValueError, match="ScanEntry"):
        S.scan_loop_closure_edge(S.ScanEntry(0, _context(), None), pts)
    with pytest.raises(ValueError, match="ScanEntry"):
        S.scan_loop_closure_edge((0, _context(), pts), pts)
    for kw, exc in ((dict(max_correspondence_distance=-1.0), ValueError), (dict(max_correspondence_distance=math.inf), ValueError),
                    (dict(max_correspondence_distance="1"), TypeError), (dict(min_fitness=1.5), ValueError),
                    (dict(min_fitness=math.nan), ValueError), (dict(min_fitness=None), TypeError), (dict(estimation="colored"), ValueError),
                    (dict(estimation=3), TypeError), (dict(init=np.eye(4)), ValueError), (dict(frame=np.eye(2)), ValueError),
                    (dict(origin_of_variant=np.zeros((3, 2))), ValueError),
                    (dict(context=_context(B=2), origin_of_variant=np.zeros((3, 3))), ValueError),
                    (dict(context=_context(S=59)), ValueError), (dict(context=_context(max_range=79.0)), ValueError),
                    (dict(context=_context(height_offset=1.0)), ValueError), (dict(context=torch.zeros(1, 20, 60)), TypeError)):
        with pytest.raises(exc):
            S.scan_loop_closure_edge(entry, pts, **kw)
    with pytest.raises(ValueError, match="points"):
        S.scan_loop_closure_edge(entry, torch.zeros(5, 2))
    with pytest.raises(GSR.GsrError, match="HIP device"):
        S.scan_loop_closure_edge(entry, pts, context=_context())


def test_yaw_start_pose_is_the_rotation_about_the_levelled_axis():
    yaw, off = math.radians(137.0), np.array([0.0, 0.5, 0.0])
    L = _yaw_start_pose(yaw, off)
    assert np.allclose(L[:3, :3] @ [1, 0, 0], [math.cos(yaw), math.sin(yaw), 0]) and np.allclose(L[:3, 3], off)
    F = np.eye(4)
    F[:3] = SR.tilted_frame()
    T = _yaw_start_pose(yaw, off, SR.tilted_frame())
    x = np.array([3.0, -2.0, 0.7, 1.0])
    assert np.allclose(F @ T @ x, L @ F @ x, atol=1e-12)      # levelled(new) = L levelled(old)
    assert np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-6)
