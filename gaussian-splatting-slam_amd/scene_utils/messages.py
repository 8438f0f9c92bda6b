"""sensor_msgs/PointCloud2 on the device: the byte buffer of a message - a /Visual_Merged Local_Map, /camera/depth/color/points -
decoded, cropped, posed and compacted in HIP (csrc/pointcloud2.hip), which is what the reference's process_pointcloud
(convert_visual_merged_msg.py:115-185) and read_pointcloud / read_points_with_color (:251-326, pointcloud_pcd.py:13-85) do point by
point with `struct` in a Python loop; then the conditioning and registration of scene_utils.pointcloud / scene_utils.registration,
so that the reference's map-building loop (main, :549-555) runs on the device from message bytes to the merged cloud.  ROS is not
imported: any object with the attributes of sensor_msgs.msg.PointCloud2 is a message.  There is no CPU path; arguments are
validated before any device work.

The exact rules (include/gsr.h, gsr_pc2_decode): coordinates become float32 as numpy.astype(float32) makes them; skip_nans drops a
row with a NaN coordinate or a FLOAT32 colour word whose bits are a NaN; the crop acts on the sensor-frame values before the pose -
dropped iff (double)y < min_y, dropped iff ((double)x*x + (double)y*y) + (double)z*z > (double)max_range * (double)max_range;
the pose is q = (float32)(R s + t) of scene_utils.registration; colour channels are byte / 255 from the packed 0x00RRGGBB word,
read by its BITS (pointcloud_pcd.py:99-107 takes int(rgb) of the packed float, which truncates the float's value instead: a
defect of the reference that is not followed)."""
from __future__ import annotations

import ctypes as C
import math
import numbers
import warnings

import torch

from .pointcloud import _check_cloud, _check_normals, _check_voxel_size, estimate_normals, voxel_down_sample
from .registration import _check_transform, _device_T, register_and_merge


def _gsr():
    from diff_gaussian_rasterization import _C
    return _C


class PointField:
    """A field of a PointCloud2 point (sensor_msgs/PointField) and the eight datatype codes."""
    INT8, UINT8, INT16, UINT16, INT32, UINT32, FLOAT32, FLOAT64 = 1, 2, 3, 4, 5, 6, 7, 8
    __slots__ = ("name", "offset", "datatype", "count")

    def __init__(self, name, offset, datatype, count=1):
        self.name, self.offset, self.datatype, self.count = name, offset, datatype, count

    def __repr__(self):
        return f"PointField(name={self.name!r}, offset={self.offset}, datatype={self.datatype}, count={self.count})"


DATATYPE_SIZES = {PointField.INT8: 1, PointField.UINT8: 1, PointField.INT16: 2, PointField.UINT16: 2, PointField.INT32: 4,
                  PointField.UINT32: 4, PointField.FLOAT32: 4, PointField.FLOAT64: 8}
COLOR_DATATYPES = (PointField.FLOAT32, PointField.UINT32, PointField.INT32)
MAX_POINTS = (1 << 30) - 1


class PointCloud2:
    """A plain record with the attributes of sensor_msgs/PointCloud2.  fields: PointField objects or (name, offset, datatype,
    count) tuples; data: bytes, bytearray, a numpy uint8 array or a uint8 tensor on the HIP device."""
    __slots__ = ("height", "width", "fields", "is_bigendian", "point_step", "row_step", "data", "is_dense")

    def __init__(self, height, width, fields, is_bigendian, point_step, row_step, data, is_dense=False):
        self.height, self.width, self.fields, self.is_bigendian = height, width, fields, is_bigendian
        self.point_step, self.row_step, self.data, self.is_dense = point_step, row_step, data, is_dense


def _check_size(name, value):
    if isinstance(value, bool) or not isinstance(value, numbers.Integral):
        raise TypeError(f"{name}={value!r}: expected an int")
    if not 0 <= value <= 0xFFFFFFFF:      # (uint32 in the message and in gsr_pc2_layout)
        raise ValueError(f"{name}={value}: expected a value in [0, 2^32 - 1]")
    return int(value)


def _field_record(f):
    if isinstance(f, (tuple, list)):
        if len(f) != 4:
            raise TypeError(f"field {f!r}: expected (name, offset, datatype, count)")
        return tuple(f)
    try:
        return f.name, f.offset, f.datatype, f.count
    except AttributeError:
        raise TypeError(f"field {f!r}: expected an object with name, offset, datatype and count, or such a tuple") from None


def _check_field(name, offset, datatype, count, point_step, datatypes=None):
    for what, v in (("offset", offset), ("datatype", datatype), ("count", count)):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise TypeError(f"field {name!r}: {what}={v!r}: expected an int")
    if count != 1:
        raise ValueError(f"field {name!r}: count={count}: expected 1")
    if datatype not in DATATYPE_SIZES:
        raise ValueError(f"field {name!r}: datatype={datatype}: expected a PointField code 1 .. 8")
    if datatypes is not None and datatype not in datatypes:
        raise ValueError(f"field {name!r}: datatype={datatype}: a packed colour is FLOAT32, UINT32 or INT32")
    if offset < 0 or offset > 0x7FFFFFFF or offset + DATATYPE_SIZES[datatype] > point_step:      # (int32 in gsr_pc2_layout)
        raise ValueError(f"field {name!r}: offset={offset} with {DATATYPE_SIZES[datatype]} bytes leaves point_step={point_step}")
    return int(offset), int(datatype)


def _check_layout(msg, color_field):
    """the message's header -> (gsr_pc2_layout values as a dict, bytes the layout needs); type before value, no device work"""
    try:
        height, width, point_step, row_step = msg.height, msg.width, msg.point_step, msg.row_step
        fields, big, _ = msg.fields, msg.is_bigendian, msg.data
    except AttributeError as e:
        raise TypeError(f"msg: expected a PointCloud2 (height, width, fields, is_bigendian, point_step, row_step, data): {e}") \
            from None
    height, width = _check_size("height", height), _check_size("width", width)
    point_step, row_step = _check_size("point_step", point_step), _check_size("row_step", row_step)
    if color_field is not None and not isinstance(color_field, str):
        raise TypeError(f"color_field={color_field!r}: expected a field's name or None")
    named = {}
    for f in fields:
        rec = _field_record(f)
        named.setdefault(rec[0], rec)
    lay = {"height": height, "width": width, "point_step": point_step, "row_step": row_step, "is_bigendian": 1 if big else 0,
           "offset": [], "datatype": [], "color_offset": -1, "color_datatype": 0}
    for axis in "xyz":
        if axis not in named:
            raise ValueError(f"msg.fields: no field {axis!r} (fields: {sorted(str(k) for k in named)})")
        o, d = _check_field(*named[axis], point_step)
        lay["offset"].append(o)
        lay["datatype"].append(d)
    if color_field is None:
        color_field = "rgb" if "rgb" in named else "rgba" if "rgba" in named else None
    elif color_field not in named:
        raise ValueError(f"color_field={color_field!r}: no such field (fields: {sorted(str(k) for k in named)})")
    if color_field is not None:
        lay["color_offset"], lay["color_datatype"] = _check_field(*named[color_field], point_step, COLOR_DATATYPES)
    if row_step < width * point_step:
        raise ValueError(f"row_step={row_step}: below width * point_step = {width * point_step}")
    if width * height > MAX_POINTS:
        raise ValueError(f"width * height = {width * height}: at most 2^30 - 1 points")
    need = (height - 1) * row_step + width * point_step if width * height else 0
    return lay, need


def _check_crop(min_y, max_range):
    for name, v in (("min_y", min_y), ("max_range", max_range)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, numbers.Real)):
            raise TypeError(f"{name}={v!r}: expected a number or None")
    if min_y is not None and math.isnan(min_y):
        raise ValueError("min_y is NaN")
    if max_range is not None and (math.isnan(max_range) or max_range < 0):
        raise ValueError(f"max_range={max_range}: expected a value >= 0")
    lo = -math.inf if min_y is None else float(min_y)
    r = math.inf if max_range is None else float(max_range)
    return lo, r * r      # (the kernel compares the squared range: (double)r * (double)r)


def _check_data(data, need):
    """type and length of msg.data -> ('device', tensor) or ('host', numpy uint8 view); a CPU tensor raises GsrError, last"""
    import numpy as np
    if isinstance(data, torch.Tensor):
        if data.dtype != torch.uint8:
            raise TypeError(f"msg.data: expected a uint8 tensor, got {data.dtype}")
        n = data.numel()
    elif isinstance(data, np.ndarray):
        if data.dtype != np.uint8:
            raise TypeError(f"msg.data: expected a uint8 array, got {data.dtype}")
        n = data.size
    elif isinstance(data, (bytes, bytearray)):
        n = len(data)
    else:
        raise TypeError(f"msg.data: expected bytes, a bytearray, a numpy uint8 array or a uint8 tensor, got {type(data).__name__}")
    if n < need:
        raise ValueError(f"msg.data: {n} bytes, the layout needs {need}")
    if isinstance(data, torch.Tensor):
        if not data.is_cuda:
            raise _gsr().GsrError("decode_pointcloud2: a tensor msg.data must live on the HIP device (host data: bytes or numpy)")
        return "device", data.detach().reshape(-1).contiguous()
    if isinstance(data, np.ndarray):
        return "host", np.ascontiguousarray(data).reshape(-1)
    return "host", np.frombuffer(data, dtype=np.uint8)


def _upload(arr):
    with warnings.catch_warnings():      # (a read-only buffer - bytes - is only read: it goes to the device at once)
        warnings.simplefilter("ignore")
        t = torch.from_numpy(arr)
    return t.to(torch.device("cuda", torch.cuda.current_device()))


def decode_pointcloud2(msg, transform=None, min_y=None, max_range=None, skip_nans=True, color_field=None, return_index=False):
    """-> (points float32 [n,3], colors float32 [n,3] or None[, index int32 [n]]) on the HIP device: the rows of the message that
    survive skip_nans and the crop (min_y, max_range: None = off; both act on the sensor-frame values), moved by `transform` ([4,4],
    None = not moved), in message order; `index` = each kept row's number v * width + u.  color_field=None takes `rgb`, else
    `rgba`, if the message has one; a string names the field.  Host data is uploaded once, a device uint8 tensor is used in place.
    One read-back (count and status).  An empty message returns empty tensors without a launch."""
    lay, need = _check_layout(msg, color_field)
    T = _check_transform(transform, "transform")
    lo, r2 = _check_crop(min_y, max_range)
    where, data = _check_data(msg.data, need)
    _C = _gsr()
    if where == "host":
        data = _upload(data) if lay["width"] * lay["height"] else None
    dev = data.device if data is not None else torch.device("cuda", torch.cuda.current_device())
    N = lay["width"] * lay["height"]
    has_color = lay["color_offset"] >= 0
    out_p = torch.empty((N, 3), dtype=torch.float32, device=dev)
    out_c = torch.empty((N, 3), dtype=torch.float32, device=dev) if has_color else None
    out_i = torch.empty(N, dtype=torch.int32, device=dev) if return_index else None
    n = 0
    if N > 0:
        lib = _C.lib()
        L = _C.gsr_pc2_layout(lay["width"], lay["height"], lay["point_step"], lay["row_step"], lay["is_bigendian"],
                              (C.c_int32 * 3)(*lay["offset"]), (C.c_int32 * 3)(*lay["datatype"]), lay["color_offset"],
                              lay["color_datatype"])
        Td = None if T is None else _device_T(T, dev)
        count = torch.empty(2, dtype=torch.int64, device=dev)
        with _C.on_device(dev):
            ws = torch.empty(lib.gsr_pc2_decode_workspace_bytes(N), dtype=torch.uint8, device=dev)
            _C.check(lib.gsr_pc2_decode(C.byref(L), _C.ptr(data), data.numel(), _C.ptr(Td), lo, r2, 1 if skip_nans else 0,
                                        _C.ptr(out_p), _C.ptr(out_c), _C.ptr(out_i), N, _C.ptr(count), _C.ptr(ws), ws.numel(),
                                        _C._stream()))
        n, status = (int(x) for x in count.tolist())
        if status != 0 or n > N:
            raise _C.GsrError(f"decode_pointcloud2: {n} rows kept of {N}")      # (cap = N: cannot happen)
    res = (out_p[:n], out_c[:n] if out_c is not None else None)
    return res + (out_i[:n],) if return_index else res


def _xyz(v, name, with_w):
    """three (four) floats of a sequence, a tensor, or an object with .x .y .z (.w)"""
    names = ("x", "y", "z", "w") if with_w else ("x", "y", "z")
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().tolist()
    if all(hasattr(v, a) for a in names) and not hasattr(v, "__len__"):
        v = [getattr(v, a) for a in names]
    try:
        vals = list(v)
    except TypeError:
        raise TypeError(f"{name}={v!r}: expected {len(names)} numbers or an object with {' '.join('.' + a for a in names)}") from None
    for c in vals:
        if isinstance(c, bool) or not isinstance(c, numbers.Real):
            raise TypeError(f"{name}={v!r}: expected {len(names)} numbers")
    if len(vals) != len(names):
        raise ValueError(f"{name}: expected {len(names)} values, got {len(vals)}")
    return [float(c) for c in vals]


def pose_matrix(quaternion_xyzw, translation):
    """float64 [4,4] (host): rotation of the quaternion (x, y, z, w; normalised here, as scipy's Rotation.from_quat does) and the
    translation - the matrix the reference builds at convert_visual_merged_msg.py:130-136.  Both arguments: sequences or objects
    with .x .y .z (.w).  A zero or non-finite quaternion, a non-finite translation: ValueError."""
    q = _xyz(quaternion_xyzw, "quaternion_xyzw", True)
    t = _xyz(translation, "translation", False)
    norm = math.sqrt(sum(c * c for c in q)) if all(math.isfinite(c) for c in q) else math.nan
    if not (math.isfinite(norm) and norm > 0.0):
        raise ValueError(f"quaternion_xyzw={q}: expected a finite, non-zero quaternion")
    if not all(math.isfinite(c) for c in t):
        raise ValueError(f"translation={t}: expected three finite values")
    x, y, z, w = (c / norm for c in q)
    return torch.tensor([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w), t[0]],
                         [2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w), t[1]],
                         [2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y), t[2]],
                         [0.0, 0.0, 0.0, 1.0]], dtype=torch.float64)


def _check_process(voxel_size, normal_radius, normal_max_nn):
    if voxel_size is not None:
        _check_voxel_size(voxel_size)
    if normal_radius is not None:
        _check_normals(normal_radius, normal_max_nn)


def process_pointcloud(msg, xyz_offset, quaternion, distance_threshold=10.0, min_y=-0.1, voxel_size=0.05, normal_radius=0.1,
                       normal_max_nn=30):
    """The reference's process_pointcloud (convert_visual_merged_msg.py:115-185) -> (points, colors or None, normals or None):
    decode_pointcloud2 with skip_nans, the height and range crop (`min_y`, `distance_threshold`; None = off) and the pose
    pose_matrix(quaternion, xyz_offset); voxel_down_sample(voxel_size); estimate_normals(normal_radius, normal_max_nn).
    voxel_size=None / normal_radius=None skips that stage (no normals: None)."""
    T = pose_matrix(quaternion, xyz_offset)
    _check_crop(min_y, distance_threshold)
    _check_process(voxel_size, normal_radius, normal_max_nn)
    points, colors = decode_pointcloud2(msg, transform=T, min_y=min_y, max_range=distance_threshold, skip_nans=True)
    if voxel_size is not None:
        points, colors = voxel_down_sample(points, colors, voxel_size)
    normals = estimate_normals(points, normal_radius, normal_max_nn) if normal_radius is not None else None
    return points, colors, normals


def accumulate_pointclouds(messages, offsets, quaternions, **register):
    """The reference's map-building loop (convert_visual_merged_msg.py:549-555) -> (points, colors or None,
    [RegistrationResult, ...]): the first message's processed cloud (process_pointcloud with its defaults; the normals, which
    the loop never reads, are not estimated) is the map; every further one is the `source` of
    register_and_merge(source, source_colors, map, map_colors, **register), whose merged cloud is the next map.  One result per
    further message.  The reference adds `source` to the merged cloud a second time, unmoved, at :555 - every row of every
    message twice, one copy misplaced.  That is a defect of the reference and is not reproduced."""
    messages, offsets, quaternions = list(messages), list(offsets), list(quaternions)
    if not messages or len(offsets) != len(messages) or len(quaternions) != len(messages):
        raise ValueError(f"accumulate_pointclouds: {len(messages)} messages, {len(offsets)} offsets, {len(quaternions)} "
                         "quaternions: expected one offset and one quaternion per message, at least one message")
    for o, q in zip(offsets, quaternions):
        pose_matrix(q, o)      # (every pose is checked before the first message is decoded)
    points, colors, _ = process_pointcloud(messages[0], offsets[0], quaternions[0], normal_radius=None)
    results = []
    for msg, o, q in zip(messages[1:], offsets[1:], quaternions[1:]):
        src, scol, _ = process_pointcloud(msg, o, q, normal_radius=None)
        points, colors, result = register_and_merge(src, scol, points, colors, **register)
        results.append(result)
    return points, colors, results


def encode_pointcloud2(points, colors=None):
    """-> PointCloud2 in the canonical layout (little-endian, x / y / z FLOAT32 at 0 / 4 / 8, packed `rgb` FLOAT32 at 12,
    point_step 16, height 1) whose data is a uint8 tensor on the HIP device: what pointcloud_aligner.py:13-44 builds to publish a
    moved cloud.  Coordinates keep their bits; a colour channel becomes the byte (int)(min(max(c, 0), 1) * 255 + 0.5), NaN -> 0;
    without colours the rgb word is 0."""
    pts, col = _check_cloud(points, colors, "encode_pointcloud2")
    P, dev = int(pts.shape[0]), pts.device
    data = torch.empty(16 * P, dtype=torch.uint8, device=dev)
    if P > 0:
        _C = _gsr()
        with _C.on_device(dev):
            _C.check(_C.lib().gsr_pc2_encode(P, _C.ptr(pts), _C.ptr(col), _C.ptr(data), _C._stream()))
    fields = [PointField("x", 0, PointField.FLOAT32, 1), PointField("y", 4, PointField.FLOAT32, 1),
              PointField("z", 8, PointField.FLOAT32, 1), PointField("rgb", 12, PointField.FLOAT32, 1)]
    return PointCloud2(1, P, fields, False, 16, 16 * P, data, False)
