"""CPU tests of the PointCloud2 layer: the numpy restatement (tests/pointcloud2_reference.py) against an independent per-point
struct.unpack_from, pose_matrix against a quaternion -> matrix written out by hand, and every validation error of
scene_utils.messages on host data - which shows that it fires before any device work (there is no device here)."""
import math

import numpy as np
import pytest
import torch

import pointcloud2_reference as P2
import scene_utils as S
from scene_utils import PointField
from scene_utils.messages import PointCloud2


# ---- the reference module against struct.unpack_from --------------------------------------------------------------------------------
def _all_types_message(big, n=37):
    """all 8 datatypes in one point, every multi-byte field at an odd offset"""
    fields = [("x", 1, P2.FLOAT32, 1), ("y", 5, P2.FLOAT64, 1), ("z", 13, P2.INT16, 1), ("a", 0, P2.INT8, 1),
              ("b", 15, P2.UINT8, 1), ("c", 17, P2.UINT16, 1), ("d", 19, P2.INT32, 1), ("e", 23, P2.UINT32, 1),
              ("rgb", 27, P2.FLOAT32, 1)]
    P2.LAYOUTS["_all"] = (fields, 33, big, 3, 5)
    try:
        return P2.build_message("_all", n, seed=5 + int(big))
    finally:
        del P2.LAYOUTS["_all"]


@pytest.mark.parametrize("big", [False, True])
def test_reference_decode_matches_struct_unpack(big):
    msg = _all_types_message(big)
    assert msg.height == 3 and msg.row_step == msg.width * 33 + 5
    for name, _, dt, _ in msg.fields:
        if name == "rgb":
            continue
        got = P2.field_view(msg, name)
        want = np.array([P2.unpack_point(msg, n, name) for n in range(msg.n)], dtype=P2.NP_KIND[dt])
        if dt in (P2.FLOAT32, P2.FLOAT64):
            assert np.array_equal(got.view("u%d" % P2.SIZE[dt]), want.view("u%d" % P2.SIZE[dt])), name
        else:
            assert np.array_equal(got, want), name
    words = P2.field_view(msg, "rgb", as_words=True)
    _, off, _, _ = P2.field_of(msg, "rgb")
    raw = bytes(msg.data)
    for n in range(msg.n):
        v, u = divmod(n, msg.width)
        at = v * msg.row_step + u * msg.point_step + off
        assert int(words[n]) == int.from_bytes(raw[at:at + 4], "big" if big else "little")


@pytest.mark.parametrize("name", sorted(P2.LAYOUTS))
def test_reference_decode_of_every_layout(name):
    msg = P2.build_message(name, 66, seed=3)
    x, y, z, w = P2.fields_f32(msg)
    for axis, got in zip("xyz", (x, y, z)):
        with np.errstate(over="ignore", invalid="ignore"):
            want = np.array([P2.unpack_point(msg, n, axis) for n in range(msg.n)]).astype(np.float32)
        assert np.array_equal(P2.bits(got), P2.bits(want)), (name, axis)
    pts, col, idx = P2.decode(msg, skip_nans=False)
    assert pts.shape == (msg.n, 3) and np.array_equal(idx, np.arange(msg.n))
    assert (col is None) == (P2.color_name(msg) is None)
    if col is not None:
        assert np.array_equal(np.round(col.astype(np.float64) * 255).astype(np.uint32),
                              np.stack([(w >> 16) & 255, (w >> 8) & 255, w & 255], axis=1))


def test_reference_crop_and_nan_rules():
    f32 = np.float32
    y_edge = f32(-0.1)
    vals = {"x": np.array([0, 0, 3, 3, np.nan, 1, np.inf, 1], dtype=f32),
            "y": np.array([y_edge, np.nextafter(y_edge, f32(0)), 4, np.nextafter(f32(4), f32(np.inf)), 0, 0, 0, 0], dtype=f32),
            "z": np.zeros(8, dtype=f32),
            "rgb": np.array([0, 0, 0, 0, 0, P2.NAN_WORD, 0, 0x00FF8001], dtype=np.uint32)}
    msg = P2.build_message("a", 8, values=vals)
    assert list(P2.keep_mask(msg, min_y=-0.1, max_range=5.0)) == [False, True, True, False, False, False, False, True]
    assert list(P2.keep_mask(msg, skip_nans=False)) == [True] * 8
    assert list(P2.keep_mask(msg)) == [True, True, True, True, False, False, True, True]
    _, col, _ = P2.decode(msg)
    assert np.array_equal(col[-1], np.array([1.0, f32(128) / f32(255), f32(1) / f32(255)], dtype=f32))


# ---- pose_matrix ---------------------------------------------------------------------------------------------------------------------
def _by_hand(q, t):
    x, y, z, w = (c / math.sqrt(sum(v * v for v in q)) for c in q)
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y), t[0]],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x), t[1]],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z, t[2]],
                     [0, 0, 0, 1]], dtype=np.float64)


@pytest.mark.parametrize("q", [(0.0, 0.0, math.sin(0.35), math.cos(0.35)), (0.5, -0.5, 0.5, 0.5), (0.1, 0.7, -0.2, 0.4)])
def test_pose_matrix_matches_hand_written(q):
    t = (1.5, -2.25, 1000.0)
    M = S.pose_matrix(q, t)
    assert M.dtype == torch.float64 and tuple(M.shape) == (4, 4) and not M.is_cuda
    assert np.abs(M.numpy() - _by_hand(q, t)).max() <= 1e-15
    R = M.numpy()[:3, :3]
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-15 and abs(np.linalg.det(R) - 1) <= 1e-15
    scaled = S.pose_matrix([7.5 * c for c in q], t)                       # normalised
    assert np.abs(scaled.numpy() - M.numpy()).max() <= 1e-15

    class Q:
        x, y, z, w = q

    class T:
        x, y, z = t
    assert torch.equal(S.pose_matrix(Q(), T()), M)                        # objects with .x .y .z .w, as ROS hands them over


def test_pose_matrix_z_rotation_values():
    a = 0.35
    M = S.pose_matrix((0, 0, math.sin(a / 2), math.cos(a / 2)), (0, 0, 0)).numpy()
    want = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    assert np.abs(M[:3, :3] - want).max() <= 1e-15


@pytest.mark.parametrize("q, t, exc", [
    ((0, 0, 0, 0), (0, 0, 0), ValueError), ((0, 0, math.nan, 1), (0, 0, 0), ValueError), ((0, 0, math.inf, 1), (0, 0, 0), ValueError),
    ((0, 0, 1), (0, 0, 0), ValueError), ((0, 0, 0, 1), (0, 0), ValueError), ((0, 0, 0, 1), (0, math.inf, 0), ValueError),
    (("a", 0, 0, 1), (0, 0, 0), TypeError), (5, (0, 0, 0), TypeError), ((0, 0, 0, 1), None, TypeError)])
def test_pose_matrix_errors(q, t, exc):
    with pytest.raises(exc):
        S.pose_matrix(q, t)


# ---- validation of decode_pointcloud2, all on host data --------------------------------------------------------------------------------
def _msg(**over):
    m = P2.build_message("a", 8, special=False)
    rec = PointCloud2(m.height, m.width, [PointField(*f) for f in m.fields], m.is_bigendian, m.point_step, m.row_step, m.data)
    for k, v in over.items():
        setattr(rec, k, v)
    return rec


def _fields(**change):
    """layout (a)'s fields with one of them replaced (None: removed)"""
    out = []
    for f in P2.LAYOUTS["a"][0]:
        if f[0] in change:
            if change[f[0]] is not None:
                out.append(change[f[0]])
        else:
            out.append(f)
    return out


BAD_MESSAGES = [
    ("no x", dict(fields=_fields(x=None)), ValueError),
    ("no z", dict(fields=_fields(z=None)), ValueError),
    ("count 2", dict(fields=_fields(y=("y", 4, 7, 2))), ValueError),
    ("datatype 9", dict(fields=_fields(y=("y", 4, 9, 1))), ValueError),
    ("datatype 0", dict(fields=_fields(x=("x", 0, 0, 1))), ValueError),
    ("datatype str", dict(fields=_fields(x=("x", 0, "7", 1))), TypeError),
    ("field outside point_step", dict(fields=_fields(z=("z", 17, 7, 1))), ValueError),
    ("float64 outside point_step", dict(fields=_fields(z=("z", 13, 8, 1))), ValueError),
    ("negative offset", dict(fields=_fields(z=("z", -1, 7, 1))), ValueError),
    ("colour outside point_step", dict(fields=_fields(rgb=("rgb", 18, 7, 1))), ValueError),
    ("colour datatype", dict(fields=_fields(rgb=("rgb", 16, 8, 1))), ValueError),
    ("field tuple", dict(fields=[("x", 0, 7)]), TypeError),
    ("short data", dict(data=b"\0" * 159), ValueError),
    ("data type", dict(data=[0] * 160), TypeError),
    ("data dtype", dict(data=np.zeros(160, dtype=np.int8)), TypeError),
    ("tensor dtype", dict(data=torch.zeros(160, dtype=torch.int8)), TypeError),
    ("row_step", dict(row_step=159), ValueError),
    ("width type", dict(width=8.0), TypeError),
    ("negative height", dict(height=-1), ValueError),
    ("too many points", dict(height=1 << 15, width=1 << 15, row_step=20 << 15), ValueError),
    ("row_step beyond uint32", dict(row_step=(1 << 32) + 160), ValueError),      # would wrap to 160 on its way into the C struct
    ("point_step beyond uint32", dict(point_step=1 << 32, row_step=1 << 35), ValueError),
    ("memoryview data", dict(data=memoryview(b"\0" * 160)), TypeError),
]


@pytest.mark.parametrize("label, over, exc", BAD_MESSAGES, ids=[b[0] for b in BAD_MESSAGES])
def test_decode_rejects_bad_message(label, over, exc):
    with pytest.raises(exc):
        S.decode_pointcloud2(_msg(**over))


BAD_ARGUMENTS = [
    (dict(max_range=math.nan), ValueError), (dict(max_range=-1.0), ValueError), (dict(max_range="5"), TypeError),
    (dict(min_y=math.nan), ValueError), (dict(min_y="0"), TypeError), (dict(min_y=True), TypeError),
    (dict(transform=np.eye(3)), ValueError), (dict(transform=torch.eye(4)[:3]), ValueError),
    (dict(transform=torch.eye(4, dtype=torch.int32)), ValueError),
    (dict(color_field="intensity"), ValueError), (dict(color_field=3), TypeError),
]


@pytest.mark.parametrize("kw, exc", BAD_ARGUMENTS)
def test_decode_rejects_bad_argument(kw, exc):
    with pytest.raises(exc):
        S.decode_pointcloud2(_msg(), **kw)


def test_decode_rejects_what_is_no_message():
    with pytest.raises(TypeError):
        S.decode_pointcloud2(b"\0" * 160)


def test_cpu_tensor_data_is_refused_last():
    from diff_gaussian_rasterization import _C
    with pytest.raises(_C.GsrError):
        S.decode_pointcloud2(_msg(data=torch.zeros(160, dtype=torch.uint8)))
    with pytest.raises(ValueError):                                       # the value errors come first
        S.decode_pointcloud2(_msg(data=torch.zeros(160, dtype=torch.uint8)), max_range=-1.0)
    with pytest.raises(_C.GsrError):
        S.encode_pointcloud2(torch.zeros(4, 3))


def test_pipeline_arguments_are_checked_before_the_decode():
    m, q, t = _msg(), (0, 0, 0, 1), (0, 0, 0)
    for kw, exc in ((dict(voxel_size=0.0), ValueError), (dict(voxel_size="a"), TypeError), (dict(normal_radius=-1.0), ValueError),
                    (dict(normal_max_nn=2), ValueError), (dict(distance_threshold=-1.0), ValueError),
                    (dict(min_y=math.nan), ValueError)):
        with pytest.raises(exc):
            S.process_pointcloud(m, t, q, **kw)
    with pytest.raises(ValueError):
        S.process_pointcloud(m, t, (0, 0, 0, 0))
    with pytest.raises(ValueError):
        S.accumulate_pointclouds([m, m], [t], [q, q])
    with pytest.raises(ValueError):
        S.accumulate_pointclouds([], [], [])
    with pytest.raises(ValueError):
        S.accumulate_pointclouds([m, m], [t, t], [q, (0, 0, 0, 0)])       # the second pose, before the first decode


def test_datatype_constants():
    assert [PointField.INT8, PointField.UINT8, PointField.INT16, PointField.UINT16, PointField.INT32, PointField.UINT32,
            PointField.FLOAT32, PointField.FLOAT64] == list(range(1, 9))
