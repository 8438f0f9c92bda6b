"""PointCloud2 decode on the device (csrc/pointcloud2.hip, scene_utils.messages) against the numpy restatement of
tests/pointcloud2_reference.py.  Every comparison of decoded values is BIT-EXACT: each rule is a fixed sequence of correctly rounded
operations (include/gsr.h, gsr_pc2_decode), so no tolerance has to be measured.

Sizes: 1, 2, around the wave (63 .. 65), around the kernel's chunk of PC2_CHUNK = 256 points (255 .. 257) and around two chunks
(511 .. 513); 307 200 once, as 640 x 480 with padded rows.  gsr_scan_u32 over the chunk counts (csrc/sort_scan.hip) has three
forms: one k_scan_apply up to GSR_SCAN_CHUNK = 2 048 counts, the one-workgroup k_scan_single up to GSR_SCAN_SINGLE_MAX = 8 192,
and beyond that k_scan_reduce -> a scan of the chunk sums -> k_scan_apply, the only form with a second level and the only one
that touches the decode's scan workspace.  One size each: 2 049 chunks (524 289 points) and 8 193 chunks (2 097 153 points; the
one size above 307 200 that a level of the scan needs).  Layouts: pointcloud2_reference.LAYOUTS - (a) .. (f) of the issue,
g1 / g2 for the remaining datatypes, h64 / h65 on either side of the staging buffer's size, `wide` whose chunks never fit it."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import pointcloud2_reference as P2
import registration_reference as RR
import scene_utils as S
from diff_gaussian_rasterization import _C as GSR
from scene_utils.messages import PointCloud2

pytestmark = pytest.mark.gpu
CHUNK = GSR.PC2_CHUNK        # points per workgroup of the decode
BOUNDARY = [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1]
SIZES = [1, 2, 63, 64, 65] + BOUNDARY
WIDE_SIZES = [3, 255, 258, 768, 771]
LAYOUTS = ["a", "b", "c", "d", "e", "f", "g1", "g2", "h64", "h65"]
SCAN_SINGLE = 2048 * CHUNK + 1       # GSR_SCAN_CHUNK + 1 chunk counts: k_scan_single instead of one k_scan_apply
SCAN_LEVELS = 8192 * CHUNK + 1       # GSR_SCAN_SINGLE_MAX + 1 chunk counts: reduce, scan of the sums (second level), apply


def _C():
    return GSR


def test_boundary_layouts_sit_on_either_side_of_the_staging_buffer():
    """h64: a full chunk stages with any misalignment of its first address; h65: a full chunk does not, a shorter one does"""
    assert SIZES == [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513]
    step64, step65 = P2.LAYOUTS["h64"][1], P2.LAYOUTS["h65"][1]
    assert CHUNK * step64 + 3 <= GSR.PC2_LDS_BYTES < CHUNK * step65
    assert (CHUNK - 4) * step65 + 3 <= GSR.PC2_LDS_BYTES


@functools.lru_cache(maxsize=None)
def message(name, N, seed=0, special=True):
    return P2.build_message(name, N, seed=seed + 7 * N, special=special)


def run(msg, **kw):
    p, c, i = S.decode_pointcloud2(msg, return_index=True, **kw)
    assert p.is_cuda and p.dtype == torch.float32 and i.dtype == torch.int32
    return p.cpu().numpy(), (None if c is None else c.cpu().numpy()), i.cpu().numpy()


def assert_same(got, want, label):
    gp, gc, gi = got
    wp, wc, wi = want
    assert gi.shape == wi.shape, (label, gi.shape, wi.shape)
    assert np.array_equal(gi, wi), label
    assert np.array_equal(P2.bits(gp), P2.bits(wp)), label
    assert (gc is None) == (wc is None), label
    if wc is not None:
        assert np.array_equal(P2.bits(gc), P2.bits(wc)), label


def check(msg, label, T=None, **kw):
    assert_same(run(msg, transform=T, **kw), P2.decode(msg, T=T, **kw), label)


# ---- decode only -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LAYOUTS)
@pytest.mark.parametrize("N", SIZES)
def test_decode_only(name, N):
    msg = message(name, N)
    got = run(msg, skip_nans=False)
    assert got[0].shape[0] == msg.n                                       # NaN and +-inf rows pass, with their bits
    assert_same(got, P2.decode(msg, skip_nans=False), (name, N))


@pytest.mark.parametrize("N", WIDE_SIZES)
def test_decode_only_rows_that_never_stage(N):
    check(message("wide", N), ("wide", N), skip_nans=False)
    check(message("wide", N), ("wide", N, "crop"), min_y=0.0, max_range=4.0)


@functools.lru_cache(maxsize=None)
def full_frame():
    return P2.build_message("f", 0, seed=11, shape=(480, 640))


def test_full_frame_640x480_padded_rows():
    msg = full_frame()
    assert msg.n == 307200 and msg.row_step == 640 * 20 + 7
    check(msg, "frame", skip_nans=False)
    T = RR.rigid_about([1000.0, 0.0, 0.0], [0.2, 0.9, -0.1], 0.4, [0.3, -0.1, 0.2])
    check(msg, "frame, all stages", T=T, min_y=-0.1, max_range=4.0)


# ---- skip_nans ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "c", "d"])
def test_skip_nans_drops_only_nan_rows(name):
    f32, nan, inf = np.float32, np.nan, np.inf
    vals = {"x": np.array([nan, 1, 1, 1, inf, 1, -inf, 1], dtype=f32), "y": np.array([1, nan, 1, 1, 1, 1, 1, 1], dtype=f32),
            "z": np.array([1, 1, nan, 1, 1, inf, -inf, 1], dtype=f32),
            "rgb": np.array([0, 0, 0, P2.NAN_WORD, 0x112233, 0x445566, 0x778899, 0xFFFFFF], dtype=np.uint32)}
    msg = P2.build_message(name, 8, values=vals)
    _, _, idx = run(msg)
    float_color = P2.field_of(msg, "rgb")[2] == P2.FLOAT32
    assert list(idx) == ([4, 5, 6, 7] if float_color else [3, 4, 5, 6, 7])      # the same word in a UINT32 field is a colour
    check(msg, name)
    check(msg, name, skip_nans=False)
    assert run(msg, skip_nans=False)[2].shape[0] == 8


# ---- crop boundaries ---------------------------------------------------------------------------------------------------------------
def test_crop_boundaries():
    f32 = np.float32
    edge = f32(-0.1)                                                      # lies below the double -0.1
    assert float(edge) < -0.1 < float(np.nextafter(edge, f32(0)))
    vals = {"x": np.array([0, 0, 3, 3, np.inf, 0], dtype=f32),
            "y": np.array([edge, np.nextafter(edge, f32(0)), 4, np.nextafter(f32(4), f32(np.inf)), 0, 0], dtype=f32),
            "z": np.array([0, 0, 0, 0, 0, -np.inf], dtype=f32), "rgb": np.zeros(6, dtype=np.uint32)}
    msg = P2.build_message("a", 6, values=vals)
    assert list(run(msg, min_y=-0.1)[2]) == [1, 2, 3, 4, 5]
    assert list(run(msg, max_range=5.0)[2]) == [0, 1, 2]
    assert list(run(msg, max_range=1e30)[2]) == [0, 1, 2, 3]             # an inf row is dropped by any finite range
    assert list(run(msg, max_range=None)[2]) == [0, 1, 2, 3, 4, 5]
    assert list(run(msg, max_range=math.inf)[2]) == [0, 1, 2, 3, 4, 5]
    assert list(run(msg, min_y=-0.1, max_range=5.0)[2]) == [1, 2]
    for kw in (dict(min_y=-0.1), dict(max_range=5.0), dict(min_y=-0.1, max_range=5.0)):
        check(msg, kw, **kw)


# ---- order and index ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "c", "f"])
@pytest.mark.parametrize("N", SIZES)
def test_random_keep_pattern(name, N):
    msg = message(name, N, seed=1)
    all_p, all_c, _ = run(msg, skip_nans=False)
    p, c, idx = run(msg, min_y=0.0, max_range=6.0)
    want = P2.decode(msg, min_y=0.0, max_range=6.0)
    assert idx.shape[0] == want[2].shape[0]
    assert (np.diff(idx) > 0).all()
    assert np.array_equal(P2.bits(p), P2.bits(all_p[idx])) and np.array_equal(P2.bits(c), P2.bits(all_c[idx]))
    assert_same((p, c, idx), want, (name, N))


@pytest.mark.parametrize("N", [SCAN_SINGLE, SCAN_LEVELS], ids=["one_workgroup_scan", "second_level"])
def test_chunk_count_scan_forms(N):
    msg = P2.build_message("e", N, seed=2)      # (not cached: 6 and 23 MB)
    check(msg, N, min_y=0.0)


@pytest.mark.parametrize("pattern", ["all", "none", "first", "last"])
@pytest.mark.parametrize("N", BOUNDARY)
def test_hand_placed_keep_patterns(N, pattern):
    y = np.full(N, 1.0 if pattern == "all" else -1.0, dtype=np.float32)
    if pattern == "first":
        y[0] = 1.0
    if pattern == "last":
        y[-1] = 1.0
    msg = P2.build_message("c", N, values={"y": y}, seed=N, special=False)
    p, c, idx = run(msg, min_y=0.0)
    want = {"all": np.arange(N), "none": np.arange(0), "first": np.array([0]), "last": np.array([N - 1])}[pattern]
    assert np.array_equal(idx, want.astype(np.int32))
    assert p.shape == (want.shape[0], 3) and c.shape == (want.shape[0], 3)
    assert_same((p, c, idx), P2.decode(msg, min_y=0.0), (N, pattern))


# ---- pose --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, N", [("a", 257), ("c", 513), ("e", 65), ("f", 256)])
def test_pose_equals_transform_points(name, N):
    msg = message(name, N, seed=3)
    T = RR.rigid_about([1000.0, 0.0, 0.0], [0.4, -0.7, 0.5], 0.3, [0.05, -0.02, 0.03])
    kw = dict(min_y=-1.0, max_range=8.0)
    plain, _, idx0 = S.decode_pointcloud2(msg, return_index=True, **kw)
    posed, _, idx1 = S.decode_pointcloud2(msg, transform=T, return_index=True, **kw)
    assert torch.equal(idx0, idx1)                                         # the crop acts before the pose
    moved = S.transform_points(plain, torch.from_numpy(T))
    assert torch.equal(posed.view(torch.int32), moved.view(torch.int32))
    check(msg, (name, N), T=T, **kw)


# ---- the two load paths ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, N", [("a", 257), ("a", 5000), ("c", 257), ("c", 5000), ("f", 257), ("f", 1000), ("h65", 513)])
def test_paths_agree(name, N):
    msg = message(name, N, seed=4)
    lib = _C().lib()
    kw = dict(min_y=-2.0, max_range=7.0)
    staged = run(msg, **kw)
    assert lib.gsr_debug_pc2_force_direct(1) == 0
    try:
        direct = run(msg, **kw)
    finally:
        assert lib.gsr_debug_pc2_force_direct(0) == 1
    assert_same(direct, staged, (name, N))
    assert_same(direct, P2.decode(msg, **kw), (name, N))


@pytest.mark.parametrize("shift", [1, 2, 3])
@pytest.mark.parametrize("name", ["a", "c"])
def test_unaligned_device_buffer(name, shift):
    """data that starts `shift` bytes behind a dword and ends with the tensor: the staging loop's first and last dword are
    assembled from guarded byte loads"""
    msg = message(name, 300, seed=5)
    raw = np.frombuffer(msg.data, dtype=np.uint8)
    buf = torch.full((raw.size + shift,), 255, dtype=torch.uint8, device="cuda")
    buf[shift:] = torch.from_numpy(raw.copy()).cuda()
    dev_msg = P2.Msg(msg.height, msg.width, msg.fields, msg.is_bigendian, msg.point_step, msg.row_step, buf[shift:])
    assert dev_msg.data.data_ptr() % 4 == shift
    assert_same(run(dev_msg, skip_nans=False), P2.decode(msg, skip_nans=False), (name, shift))


def test_device_data_is_used_in_place_and_numpy_data_uploads():
    msg = message("b", 100)
    want = P2.decode(msg)
    raw = np.frombuffer(msg.data, dtype=np.uint8)
    for data in (torch.from_numpy(raw.copy()).cuda(), raw, bytearray(msg.data)):
        rec = PointCloud2(msg.height, msg.width, [S.PointField(*f) for f in msg.fields], False, msg.point_step, msg.row_step, data)
        assert_same(run(rec), want, type(data).__name__)


def test_empty_and_fully_cropped_messages():
    empty = P2.Msg(1, 0, P2.LAYOUTS["a"][0], False, 20, 0, b"")
    p, c, i = S.decode_pointcloud2(empty, return_index=True)
    assert tuple(p.shape) == (0, 3) and tuple(c.shape) == (0, 3) and tuple(i.shape) == (0,) and p.is_cuda
    p, c = S.decode_pointcloud2(message("e", 64), max_range=0.0, min_y=1e9)
    assert tuple(p.shape) == (0, 3) and c is None


def test_color_field_by_name():
    msg = message("g1", 65)                                               # its colour field is called rgba
    by_default, named = run(msg), run(msg, color_field="rgba")
    assert_same(named, by_default, "rgba")
    assert_same(named, P2.decode(msg), "rgba")


# ---- the C entry: capacity and errors ----------------------------------------------------------------------------------------------
def c_decode(msg, cap, rows=None, with_colors=True, data_bytes=None, ws_bytes=None, min_y=-math.inf):
    _c = _C()
    lib = _c.lib()
    f = {x[0]: x for x in msg.fields}
    col = f.get("rgb") or f.get("rgba")
    L = _c.gsr_pc2_layout(msg.width, msg.height, msg.point_step, msg.row_step, int(msg.is_bigendian),
                          (C.c_int32 * 3)(*[f[a][1] for a in "xyz"]), (C.c_int32 * 3)(*[f[a][2] for a in "xyz"]),
                          col[1] if col else -1, col[2] if col else 0)
    data = torch.from_numpy(np.frombuffer(msg.data, dtype=np.uint8).copy()).cuda()
    rows = cap + 1 if rows is None else rows
    out_p = torch.full((rows, 3), -7.0, device="cuda")
    out_c = torch.full((rows, 3), -7.0, device="cuda") if with_colors else None
    out_i = torch.full((rows,), -7, dtype=torch.int32, device="cuda")
    count = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    ws = torch.empty(lib.gsr_pc2_decode_workspace_bytes(msg.n) if ws_bytes is None else ws_bytes, dtype=torch.uint8, device="cuda")
    rc = lib.gsr_pc2_decode(C.byref(L), _c.ptr(data), data.numel() if data_bytes is None else data_bytes, None, min_y, math.inf, 1,
                            _c.ptr(out_p), _c.ptr(out_c), _c.ptr(out_i), cap, _c.ptr(count), _c.ptr(ws), ws.numel(), _c._stream())
    torch.cuda.synchronize()
    return rc, out_p.cpu().numpy(), (out_c.cpu().numpy() if with_colors else None), out_i.cpu().numpy(), count.tolist()


@pytest.mark.parametrize("N, cap", [(257, 100), (513, 256), (513, 1)])
def test_capacity(N, cap):
    msg = message("a", N, seed=6)
    wp, wc, wi = P2.decode(msg, min_y=-3.0)
    assert wi.shape[0] > cap
    rc, p, c, i, count = c_decode(msg, cap, min_y=-3.0)
    assert rc == 0 and count == [wi.shape[0], 1]                          # the true count, status 1
    assert_same((p[:cap], c[:cap], i[:cap]), (wp[:cap], wc[:cap], wi[:cap]), (N, cap))
    assert (p[cap] == -7.0).all() and (c[cap] == -7.0).all() and i[cap] == -7      # the guard row behind `cap`
    rc, p, c, i, count = c_decode(msg, wi.shape[0], min_y=-3.0)
    assert rc == 0 and count == [wi.shape[0], 0] and (p[-1] == -7.0).all()


def test_c_entry_errors_come_before_any_launch():
    _c = _C()
    msg = message("a", 64)
    need = msg.n * msg.point_step
    for kw in (dict(data_bytes=need - 1), dict(cap=-1)):
        kw.setdefault("cap", 64)
        rc, p, _, _, count = c_decode(msg, rows=65, **kw)
        assert rc == -1 and count == [-1, -1] and (p == -7.0).all(), kw      # GSR_ERR_INVALID_ARGUMENT, nothing written
    rc, _, _, _, count = c_decode(msg, 64, ws_bytes=8)
    assert rc == -5 and count == [-1, -1]                                 # GSR_ERR_STATE_TOO_SMALL
    rc, _, _, _, _ = c_decode(message("e", 64), 64, with_colors=True)     # out_colors, but no colour field
    assert rc == -1 and "colour" in _c.last_error()
    bad = P2.Msg(1, 64, [("x", 0, 7, 1), ("y", 4, 9, 1), ("z", 8, 7, 1)], False, 20, 1280, msg.data)
    assert c_decode(bad, 64, with_colors=False)[0] == -1
    bad = P2.Msg(1, 64, [("x", 0, 7, 1), ("y", 4, 7, 1), ("z", 17, 7, 1)], False, 20, 1280, msg.data)
    assert c_decode(bad, 64, with_colors=False)[0] == -1
    bad = P2.Msg(1, 64, P2.LAYOUTS["a"][0], False, 20, 1279, msg.data)
    assert c_decode(bad, 64)[0] == -1


# ---- encode ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 255, 256, 257, 5000])
def test_round_trip(N):
    rng = np.random.default_rng(N)
    p = rng.normal(0, 5, size=(N, 3)).astype(np.float32)
    if N > 8:
        p[3, 0], p[5, 1], p[7, 2] = np.inf, -np.inf, -0.0
    c = rng.random((N, 3)).astype(np.float32)
    msg = S.encode_pointcloud2(torch.from_numpy(p).cuda(), torch.from_numpy(c).cuda())
    assert (msg.height, msg.width, msg.point_step, msg.row_step, bool(msg.is_bigendian)) == (1, N, 16, 16 * N, False)
    assert msg.data.is_cuda and msg.data.dtype == torch.uint8 and msg.data.numel() == 16 * N
    gp, gc, gi = run(msg)
    assert np.array_equal(gi, np.arange(N)) and np.array_equal(P2.bits(gp), P2.bits(p))
    want = P2.encode_bytes(c).astype(np.float32) / np.float32(255.0)      # round(c * 255) / 255
    assert np.array_equal(P2.bits(gc), P2.bits(want))
    assert np.abs(gc.astype(np.float64) - c.astype(np.float64)).max() <= 0.5 / 255 + 1e-7
    host = P2.Msg(1, N, [(f.name, f.offset, f.datatype, f.count) for f in msg.fields], False, 16, 16 * N,
                  msg.data.cpu().numpy().tobytes())
    assert_same((gp, gc, gi), P2.decode(host), N)                         # the bytes are a well-formed little-endian message


def test_encode_clamps_and_maps_nan_to_zero():
    p = torch.zeros(2, 3, device="cuda")
    c = torch.tensor([[-0.5, 1.5, math.nan], [0.0, 1.0, 0.5]], device="cuda")
    raw = S.encode_pointcloud2(p, c).data.cpu().numpy()
    assert list(raw[12:16]) == [0, 255, 0, 0]                             # b, g, r, the unused byte: bytes 0 / 255 / 0
    assert list(raw[28:32]) == [128, 255, 0, 0]
    plain = S.encode_pointcloud2(p)
    assert not plain.data.cpu().numpy().any()
    gp, gc = S.decode_pointcloud2(plain)
    assert gp.shape[0] == 2 and not gc.any()


# ---- the pipeline ------------------------------------------------------------------------------------------------------------------
def wall_and_floor(n, seed, pose=None):
    """n points of a floor (y = 0), a back wall (z = 3) and a side wall (x = 1) with colours, seen from `pose` (world <- sensor)"""
    rng = np.random.default_rng(seed)
    k = n // 3
    floor = np.stack([rng.uniform(-1, 1, k), np.zeros(k), rng.uniform(1, 3, k)], axis=1)
    back = np.stack([rng.uniform(-1, 1, k), rng.uniform(0, 1.5, k), np.full(k, 3.0)], axis=1)
    side = np.stack([np.ones(n - 2 * k), rng.uniform(0, 1.5, n - 2 * k), rng.uniform(1, 3, n - 2 * k)], axis=1)
    world = np.concatenate([floor, back, side]) + rng.normal(0, 0.002, size=(n, 3))
    if pose is not None:
        world = (world - pose[:3, 3]) @ pose[:3, :3]                      # R^T (w - t)
    vals = {"x": world[:, 0].astype(np.float32), "y": world[:, 1].astype(np.float32), "z": world[:, 2].astype(np.float32),
            "rgb": rng.integers(0, 1 << 24, size=n).astype(np.uint32)}
    vals["x"][::97] = np.nan                                              # a sensor's invalid returns
    return P2.build_message("a", n, values=vals, seed=seed, special=False)


def test_process_pointcloud_equals_the_three_calls():
    msg = wall_and_floor(4096, 1)
    q, t = (0.0, math.sin(0.05), 0.0, math.cos(0.05)), (0.2, 0.0, -0.1)
    pts, col, nrm = S.process_pointcloud(msg, t, q)
    p0, c0 = S.decode_pointcloud2(msg, transform=S.pose_matrix(q, t), min_y=-0.1, max_range=10.0)
    p1, c1 = S.voxel_down_sample(p0, c0, 0.05)
    n1 = S.estimate_normals(p1, 0.1, 30)
    assert 0 < p1.shape[0] < p0.shape[0] < 4096
    assert torch.equal(pts, p1) and torch.equal(col, c1) and torch.equal(nrm, n1)
    pts, col, nrm = S.process_pointcloud(msg, t, q, voxel_size=None, normal_radius=None)
    assert torch.equal(pts, p0) and torch.equal(col, c0) and nrm is None


def test_accumulate_pointclouds_equals_the_hand_run_sequence():
    quats = [(0.0, 0.0, 0.0, 1.0), (0.0, math.sin(0.01), 0.0, math.cos(0.01)), (0.0, math.sin(-0.008), 0.0, math.cos(-0.008))]
    offsets = [(0.0, 0.0, 0.0), (0.03, 0.0, 0.02), (-0.02, 0.0, 0.04)]
    msgs = [wall_and_floor(4096, 10 + i, S.pose_matrix(q, o).numpy()) for i, (q, o) in enumerate(zip(quats, offsets))]
    reported = [(o[0] + 0.01, o[1], o[2] - 0.01) for o in offsets]       # the poses a tracker would hand over: a centimetre off
    pts, col, results = S.accumulate_pointclouds(msgs, reported, quats)
    first = S.process_pointcloud(msgs[0], reported[0], quats[0])
    assert len(results) == 2 and pts.shape[0] >= first[0].shape[0] and col.shape == pts.shape
    m_p, m_c = first[0], first[1]
    for k in (1, 2):
        s_p, s_c, _ = S.process_pointcloud(msgs[k], reported[k], quats[k])
        m_p, m_c, want = S.register_and_merge(s_p, s_c, m_p, m_c)
        got = results[k - 1]
        moved_a = S.transform_points(s_p, got.transformation).double()
        moved_b = S.transform_points(s_p, want.transformation).double()
        assert float((moved_a - moved_b).norm(dim=1).max()) <= want.inlier_rmse
        assert got.fitness > 0.5
    assert pts.shape == m_p.shape
