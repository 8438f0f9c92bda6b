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
import warnings

import torch

from . import _args as A
from .pointcloud import NB_NEIGHBORS_MAX, estimate_normals, voxel_down_sample
from .registration import register_and_merge


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
    return A.integer(name, value, 0, 0xFFFFFFFF, "a value in [0, 2^32 - 1]")      # (uint32 in the message and in gsr_pc2_layout)


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
        if not A.is_integer(v):
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
        if v is not None and not A.is_number(v):
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
            raise A.gsr().GsrError("decode_pointcloud2: a tensor msg.data must live on the HIP device (host data: bytes or numpy)")
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
    T = A.transform(transform, "transform")
    lo, r2 = _check_crop(min_y, max_range)
    where, data = _check_data(msg.data, need)
    _C = A.gsr()
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
        Td = None if T is None else A.device_T(T, dev)
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
        if not A.is_number(c):
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
        A.voxel_size(voxel_size)
    if normal_radius is not None:
        A.neighbourhood(normal_radius, normal_max_nn, 3, NB_NEIGHBORS_MAX)


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
    pts, col = A.cloud(points, colors, "encode_pointcloud2")
    P, dev = int(pts.shape[0]), pts.device
    data = torch.empty(16 * P, dtype=torch.uint8, device=dev)
    if P > 0:
        _C = A.gsr()
        with _C.on_device(dev):
            _C.check(_C.lib().gsr_pc2_encode(P, _C.ptr(pts), _C.ptr(col), _C.ptr(data), _C._stream()))
    fields = [PointField("x", 0, PointField.FLOAT32, 1), PointField("y", 4, PointField.FLOAT32, 1),
              PointField("z", 8, PointField.FLOAT32, 1), PointField("rgb", 12, PointField.FLOAT32, 1)]
    return PointCloud2(1, P, fields, False, 16, 16 * P, data, False)


# ---- sensor_msgs/Image, CameraInfo, TransformStamped: the other three members of a /Visual_Merged message -----------------------------
# What the reference's imgmsg_to_pli (scene/dataset_readers.py:278-309) does on the host for rgb8 / bgr8 / mono8 - ignoring `step`
# (a padded row breaks its reshape) and `is_bigendian`, and passing every frame through a JPEG on disk: three defects that are
# not followed - here in HIP (csrc/image.hip; the rules: include/gsr.h, gsr_image_decode) for the colour, Bayer and depth
# encodings, followed by the registration of a depth image into the colour camera and Frame.from_sensor.

# name -> bytes per pixel; the names of sensor_msgs/image_encodings.h
IMAGE_BYTES_PER_PIXEL = {"rgb8": 3, "bgr8": 3, "rgba8": 4, "bgra8": 4, "mono8": 1, "rgb16": 6, "bgr16": 6, "rgba16": 8, "bgra16": 8,
                         "mono16": 2, "bayer_rggb8": 1, "bayer_bggr8": 1, "bayer_gbrg8": 1, "bayer_grbg8": 1, "bayer_rggb16": 2,
                         "bayer_bggr16": 2, "bayer_gbrg16": 2, "bayer_grbg16": 2, "16UC1": 2, "32FC1": 4}
DEPTH_ENCODINGS = ("16UC1", "32FC1")      # depth unless as_depth=False; mono16 is depth where the caller says so
MAX_FOCAL_RATIO = 4.0                     # register_depth: fx_c <= 4 fx_d keeps every footprint inside the kernel's 8 x 8


class Image:
    """A plain record with the attributes of sensor_msgs/Image.  data: what PointCloud2.data takes."""
    __slots__ = ("height", "width", "encoding", "is_bigendian", "step", "data")

    def __init__(self, height, width, encoding, is_bigendian, step, data):
        self.height, self.width, self.encoding, self.is_bigendian, self.step, self.data = height, width, encoding, is_bigendian, \
            step, data


class CameraInfo:
    """A plain record with the attributes of sensor_msgs/CameraInfo that camera_info_intrinsics reads.  K: 9 values, row-major."""
    __slots__ = ("height", "width", "distortion_model", "D", "K", "R", "P")

    def __init__(self, height, width, distortion_model, D, K, R=None, P=None):
        self.height, self.width, self.distortion_model, self.D, self.K, self.R, self.P = height, width, distortion_model, D, K, R, P


def _check_image(msg, what="msg"):
    """the message's header -> (dict of gsr_image_layout values + name and bpp, bytes the layout needs); type before value"""
    try:
        height, width, encoding, step, big, _ = msg.height, msg.width, msg.encoding, msg.step, msg.is_bigendian, msg.data
    except AttributeError as e:
        raise TypeError(f"{what}: expected an Image (height, width, encoding, is_bigendian, step, data): {e}") from None
    height, width, step = _check_size("height", height), _check_size("width", width), _check_size("step", step)
    if not isinstance(encoding, str):
        raise TypeError(f"{what}.encoding={encoding!r}: expected a string")
    if encoding not in IMAGE_BYTES_PER_PIXEL:
        raise ValueError(f"{what}.encoding={encoding!r}: supported are {', '.join(IMAGE_BYTES_PER_PIXEL)}")
    bpp = IMAGE_BYTES_PER_PIXEL[encoding]
    if step < width * bpp:
        raise ValueError(f"step={step}: below width * bytes per pixel = {width * bpp}")
    if width * height > MAX_POINTS:
        raise ValueError(f"width * height = {width * height}: at most 2^30 - 1 pixels")
    if encoding.startswith("bayer_") and (width < 2 or height < 2):
        raise ValueError(f"a Bayer image of {width} x {height}: at least 2 x 2")
    lay = {"height": height, "width": width, "step": step, "encoding": encoding, "bpp": bpp, "is_bigendian": 1 if big else 0}
    return lay, ((height - 1) * step + width * bpp if width * height else 0)


def _check_depth_options(encoding, depth_scale, depth_range, as_depth):
    """-> (is depth, scale, lo, hi); type before value"""
    if as_depth is not None and not isinstance(as_depth, bool):
        raise TypeError(f"as_depth={as_depth!r}: expected True, False or None")
    if depth_scale is not None and not A.is_number(depth_scale):
        raise TypeError(f"depth_scale={depth_scale!r}: expected a number or None")
    lo = hi = None
    if depth_range is not None:
        try:
            lo, hi = depth_range
        except (TypeError, ValueError):
            raise TypeError(f"depth_range={depth_range!r}: expected (lo, hi), either may be None") from None
        for v in (lo, hi):
            if v is not None and not A.is_number(v):
                raise TypeError(f"depth_range={depth_range!r}: expected numbers or None")
    can_depth = encoding in DEPTH_ENCODINGS or encoding == "mono16"
    if as_depth is True and not can_depth:
        raise ValueError(f"as_depth=True: {encoding!r} holds no depth (16UC1, 32FC1 and mono16 do)")
    if as_depth is False and encoding in DEPTH_ENCODINGS:
        raise ValueError(f"as_depth=False: {encoding!r} holds nothing but depth")
    is_depth = encoding in DEPTH_ENCODINGS if as_depth is None else as_depth
    if not is_depth:
        if depth_scale is not None or depth_range is not None:
            raise ValueError(f"depth_scale / depth_range given, but {encoding!r} is decoded as colour")
        return False, 1.0, -math.inf, math.inf
    scale = (1.0 if encoding == "32FC1" else 0.001) if depth_scale is None else float(depth_scale)
    if not (math.isfinite(scale) and scale > 0.0):
        raise ValueError(f"depth_scale={depth_scale}: expected a finite value > 0")
    lo = -math.inf if lo is None else float(lo)
    hi = math.inf if hi is None else float(hi)
    if math.isnan(lo) or math.isnan(hi) or lo > hi:
        raise ValueError(f"depth_range={depth_range}: expected lo <= hi, no NaN")
    return True, scale, lo, hi


def decode_image(msg, depth_scale=None, depth_range=None, as_depth=None):
    """-> float32 [3,H,W] (colour, Bayer: channels in [0, 1]) or [H,W] (depth in metres, 0 = no reading) on the HIP device.
    as_depth=None: depth for 16UC1 and 32FC1, colour for everything else; as_depth=True reads a mono16 image as depth.
    depth_scale=None: 0.001 for the 16-bit forms (millimetres), 1.0 for 32FC1; depth_range=(lo, hi) zeroes what lies outside after
    the scaling (None: that bound is off).  The scale and the bounds act as float32.  Host data is uploaded once, a device uint8
    tensor is used in place, at any alignment.  One launch, no read-back.  An image of zero pixels returns an empty tensor."""
    lay, need = _check_image(msg)
    is_depth, scale, lo, hi = _check_depth_options(lay["encoding"], depth_scale, depth_range, as_depth)
    where, data = _check_data(msg.data, need)
    _C = A.gsr()
    W, H = lay["width"], lay["height"]
    if where == "host":
        data = _upload(data) if W * H else None
    dev = data.device if data is not None else torch.device("cuda", torch.cuda.current_device())
    out = torch.empty((H, W) if is_depth else (3, H, W), dtype=torch.float32, device=dev)
    if W * H > 0:
        code = _C.IMAGE_ENCODINGS["16UC1" if is_depth and lay["encoding"] == "mono16" else lay["encoding"]]
        L = _C.gsr_image_layout(W, H, lay["step"], code, lay["is_bigendian"])
        with _C.on_device(dev):
            _C.check(_C.lib().gsr_image_decode(C.byref(L), _C.ptr(data), data.numel(), scale, lo, hi, _C.ptr(out), _C._stream()))
    return out


def encode_image(image):
    """-> Image in rgb8 (step = 3 W, little-endian) whose data is a uint8 tensor on the HIP device: what the reference sends to its
    viewer (train.py:80).  `image`: float32 [3,H,W] on the device; a byte is (uint8)(min(max(c, 0), 1) * 255) - truncated, as
    .byte() does there - and 0 for a NaN."""
    if not isinstance(image, torch.Tensor):
        raise TypeError(f"image: expected a tensor, got {type(image).__name__}")
    if image.dtype != torch.float32:
        raise TypeError(f"image: expected float32, got {image.dtype}")
    if image.dim() != 3 or image.shape[0] != 3:
        raise ValueError(f"image: expected [3,H,W], got {tuple(image.shape)}")
    H, W = int(image.shape[1]), int(image.shape[2])
    if W * H > MAX_POINTS:
        raise ValueError(f"image: {W} x {H}: at most 2^30 - 1 pixels")
    _C = A.gsr()
    if not image.is_cuda:
        raise _C.GsrError("encode_image needs the image on the HIP device (no CPU path)")
    src = image.detach().contiguous()
    data = torch.empty(3 * W * H, dtype=torch.uint8, device=src.device)
    if W * H > 0:
        with _C.on_device(src.device):
            _C.check(_C.lib().gsr_image_encode_rgb8(W, H, _C.ptr(src), _C.ptr(data), _C._stream()))
    return Image(H, W, "rgb8", False, 3 * W, data)


def _numbers(v, name):
    """a flat list of floats from a sequence, an array or a tensor"""
    import numpy as np
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    try:
        arr = np.asarray(v)
    except Exception:
        raise TypeError(f"{name}={v!r}: expected numbers") from None
    if arr.dtype == object or arr.dtype.kind not in "fiu":
        raise TypeError(f"{name}={v!r}: expected numbers")
    return [float(c) for c in arr.reshape(-1)]


def camera_info_intrinsics(info):
    """sensor_msgs/CameraInfo -> (K float64 [3,3] (numpy), dist (k1, k2, p1, p2, k3) or None, (W, H)): what Frame.from_sensor
    takes - the step the reference has commented out (dataset_readers.py:313-320) in favour of hard-coded intrinsics.
    distortion_model: `plumb_bob` with up to 5 coefficients; `rational_polynomial` only if coefficients 5 and later are all
    zero (gsr_frame_undistort has five); an empty model, or an all-zero D, gives None.  fx and fy must be positive."""
    import numpy as np
    try:
        height, width, model, D, K = info.height, info.width, info.distortion_model, info.D, info.K
    except AttributeError as e:
        raise TypeError(f"info: expected a CameraInfo (height, width, distortion_model, D, K): {e}") from None
    height, width = _check_size("height", height), _check_size("width", width)
    if not isinstance(model, str):
        raise TypeError(f"distortion_model={model!r}: expected a string")
    k = _numbers(K, "K")
    d = _numbers(D, "D") if D is not None else []
    if len(k) != 9:
        raise ValueError(f"K: expected 9 values (row-major 3 x 3), got {len(k)}")
    if not all(math.isfinite(c) for c in k + d):
        raise ValueError("K / D: expected finite values")
    if not (k[0] > 0.0 and k[4] > 0.0):
        raise ValueError(f"K: fx = {k[0]}, fy = {k[4]}: expected positive focal lengths")
    if model not in ("", "plumb_bob", "rational_polynomial"):
        raise ValueError(f"distortion_model={model!r}: expected plumb_bob, rational_polynomial (with zero higher terms) or none")
    if model == "plumb_bob" and len(d) > 5:
        raise ValueError(f"D: plumb_bob has at most 5 coefficients, got {len(d)}")
    if model == "rational_polynomial" and any(c != 0.0 for c in d[5:]):
        raise ValueError("D: rational_polynomial with a non-zero k4, k5 or k6: the undistortion has (k1, k2, p1, p2, k3) only")
    dist = None
    if model != "" and any(c != 0.0 for c in d[:5]):
        dist = tuple((d[:5] + [0.0] * 5)[:5])
    return np.array(k, dtype=np.float64).reshape(3, 3), dist, (width, height)


def pose_from_transform(tf, convention="w2c"):
    """geometry_msgs/TransformStamped (anything with .transform.rotation and .transform.translation), or a (quaternion_xyzw,
    translation) pair -> float64 [4,4] world-to-camera matrix on the host.  convention="w2c": the message IS the COLMAP
    world-to-camera pose, the reading of initCameraExtrinsics / initSceneInfo (dataset_readers.py:333-338, 365-366);
    "c2w": the message is the camera's pose in the world and is inverted."""
    if not isinstance(convention, str):
        raise TypeError(f"convention={convention!r}: expected 'w2c' or 'c2w'")
    if hasattr(tf, "transform"):
        try:
            q, t = tf.transform.rotation, tf.transform.translation
        except AttributeError as e:
            raise TypeError(f"tf: expected .transform.rotation and .transform.translation: {e}") from None
    else:
        try:
            q, t = tf
        except (TypeError, ValueError):
            raise TypeError(f"tf={tf!r}: expected a TransformStamped or a (quaternion_xyzw, translation) pair") from None
    if convention not in ("w2c", "c2w"):
        raise ValueError(f"convention={convention!r}: expected 'w2c' or 'c2w'")
    M = pose_matrix(q, t)
    if convention == "c2w":      # the rigid inverse: (R^T, -R^T t)
        Rt = M[:3, :3].t().contiguous()
        M = torch.eye(4, dtype=torch.float64)
        M[:3, :3] = Rt
        M[:3, 3] = -(Rt @ pose_matrix(q, t)[:3, 3])
    return M


def _check_t34(T, name):
    """None (identity) or a [4,4] / [3,4] matrix -> 12 floats, rows 0 .. 2"""
    if T is None:
        return [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    if not isinstance(T, torch.Tensor):
        try:
            T = torch.as_tensor(T, dtype=torch.float64)
        except Exception:
            raise TypeError(f"{name}={T!r}: expected a [4,4] or [3,4] matrix") from None
    if tuple(T.shape) not in ((4, 4), (3, 4)) or not T.is_floating_point():
        raise ValueError(f"{name}: expected a floating-point [4,4] or [3,4] matrix, got {T.dtype} {tuple(T.shape)}")
    vals = [float(v) for v in T.detach().cpu().double()[:3].reshape(-1)]
    if not all(math.isfinite(v) for v in vals):
        raise ValueError(f"{name}: expected finite values")
    return vals


def _check_wh(size, name):
    try:
        W, H = size
    except (TypeError, ValueError):
        raise TypeError(f"{name}={size!r}: expected (W, H)") from None
    W, H = _check_size(f"{name}[0]", W), _check_size(f"{name}[1]", H)
    if W < 1 or H < 1 or W * H > MAX_POINTS:
        raise ValueError(f"{name}={size}: expected sides >= 1 and at most 2^30 - 1 pixels")
    return W, H


def register_depth(depth, K_depth, K_color, depth_to_color=None, size=None):
    """gsr_depth_register: `depth` float32 [Hd,Wd] (metres, 0 = no reading) of the depth camera `K_depth` on the HIP device ->
    [Hc,Wc] as the colour camera `K_color` of `size` = (Wc, Hc) (default: the depth image's) sees it - "aligned depth to
    colour", which track_pose(gt_depth=...) and add_from_rgbd assume.  depth_to_color: [4,4] or [3,4], depth-camera frame ->
    colour-camera frame (None: the identity).  Every reading covers the rectangle between its two projected pixel corners; the
    nearest reading wins; a pixel none reaches is 0.  Both cameras are ideal pinholes.  fx_c > 4 fx_d or fy_c > 4 fy_d: ValueError
    (a footprint would exceed the kernel's 8 x 8).  One read-back (the status word)."""
    if not isinstance(depth, torch.Tensor):
        raise TypeError(f"depth: expected a tensor, got {type(depth).__name__}")
    if depth.dtype != torch.float32:
        raise TypeError(f"depth: expected float32, got {depth.dtype}")
    T = _check_t34(depth_to_color, "depth_to_color")
    if depth.dim() == 3 and depth.shape[0] == 1:
        depth = depth[0]
    if depth.dim() != 2 or depth.numel() < 1 or depth.numel() > MAX_POINTS:
        raise ValueError(f"depth: expected [H,W] with 1 .. 2^30 - 1 pixels, got {tuple(depth.shape)}")
    Hd, Wd = int(depth.shape[0]), int(depth.shape[1])
    Wc, Hc = (Wd, Hd) if size is None else _check_wh(size, "size")
    kd, kc = A.k4(K_depth, "K_depth"), A.k4(K_color, "K_color")
    for name, k in (("K_depth", kd), ("K_color", kc)):
        if not all(math.isfinite(v) for v in k) or not (k[0] > 0.0 and k[1] > 0.0):
            raise ValueError(f"{name}: (fx, fy, cx, cy) = {k}: expected finite values, fx and fy positive")
    if kc[0] > MAX_FOCAL_RATIO * kd[0] or kc[1] > MAX_FOCAL_RATIO * kd[1]:
        raise ValueError(f"K_color: focal lengths ({kc[0]}, {kc[1]}) above {MAX_FOCAL_RATIO:g} x K_depth's ({kd[0]}, {kd[1]}): a "
                         "reading's footprint would exceed 8 x 8 colour pixels")
    _C = A.gsr()
    if not depth.is_cuda:
        raise _C.GsrError("register_depth needs the depth image on the HIP device (no CPU path)")
    src = depth.detach().contiguous()
    dev = src.device
    out = torch.empty((Hc, Wc), dtype=torch.float32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    lib = _C.lib()
    with _C.on_device(dev):
        ws = torch.empty(lib.gsr_depth_register_workspace_bytes(Wc, Hc), dtype=torch.uint8, device=dev)
        _C.check(lib.gsr_depth_register(Wd, Hd, _C.ptr(src), (C.c_float * 4)(*kd), (C.c_float * 4)(*kc), (C.c_double * 12)(*T),
                                        Wc, Hc, _C.ptr(out), _C.ptr(status), _C.ptr(ws), ws.numel(), _C._stream()))
    if int(status.item()) & 1:
        raise _C.GsrError("register_depth: a reading's footprint exceeded 8 x 8 colour pixels and was cut")
    return out


def frame_from_messages(image, camera_info, transform=None, depth=None, depth_info=None, depth_to_color=None, size=None,
                        new_K=None, depth_range=None, convention="w2c", name=""):
    """Message bytes in, a Frame on the device out: decode_image(image); with `depth` (an Image in 16UC1, 32FC1 or mono16)
    decode_image(depth, depth_range=..., as_depth=True) and - if `depth_info` (the depth camera's CameraInfo) or `depth_to_color`
    is given - register_depth into the colour camera (missing depth_info: the colour camera's intrinsics; missing depth_to_color:
    the identity); a depth that is already aligned (neither given) must have the image's size and skips that step.  Then
    Frame.from_sensor with camera_info's K and distortion, pose_from_transform(transform, convention) (None: the identity),
    `size` and `new_K`.  Everything is validated before the first launch.  Registration takes both cameras as ideal pinholes: a
    distorted camera on either side of it raises ValueError."""
    from .frames import Frame
    lay, _ = _check_image(image, "image")
    if not isinstance(convention, str):
        raise TypeError(f"convention={convention!r}: expected 'w2c' or 'c2w'")
    if _check_depth_options(lay["encoding"], None, None, None)[0]:
        raise ValueError(f"image.encoding={lay['encoding']!r}: a depth encoding where the colour image is expected")
    K, dist, wh = camera_info_intrinsics(camera_info)
    if wh != (lay["width"], lay["height"]):
        raise ValueError(f"camera_info is {wh[0]} x {wh[1]}, the image {lay['width']} x {lay['height']}")
    if lay["width"] * lay["height"] < 1:
        raise ValueError("image: no pixels")
    pose = None if transform is None else pose_from_transform(transform, convention)
    if size is not None:
        _check_wh(size, "size")
    register = depth is not None and (depth_info is not None or depth_to_color is not None)
    if depth is None and (depth_info is not None or depth_to_color is not None or depth_range is not None):
        raise ValueError("depth_info / depth_to_color / depth_range given without a depth image")
    if depth is not None:
        dlay, _ = _check_image(depth, "depth")
        _check_depth_options(dlay["encoding"], None, depth_range, True)
        dwh = (dlay["width"], dlay["height"])
        Kd = K
        if depth_info is not None:
            Kd, ddist, iwh = camera_info_intrinsics(depth_info)
            if iwh != dwh:
                raise ValueError(f"depth_info is {iwh[0]} x {iwh[1]}, the depth image {dwh[0]} x {dwh[1]}")
            if ddist is not None:
                raise ValueError("depth_info: a distorted depth camera: register_depth takes ideal pinholes")
        elif dwh != wh:
            raise ValueError(f"depth is {dwh[0]} x {dwh[1]}, the image {wh[0]} x {wh[1]}: pass depth_info to register it")
        if register:
            if dist is not None:
                raise ValueError("camera_info: a distorted colour camera: register_depth takes ideal pinholes")
            _check_t34(depth_to_color, "depth_to_color")
            if K[0, 0] > MAX_FOCAL_RATIO * Kd[0, 0] or K[1, 1] > MAX_FOCAL_RATIO * Kd[1, 1]:
                raise ValueError(f"camera_info: focal lengths above {MAX_FOCAL_RATIO:g} x the depth camera's")
    img = decode_image(image)
    d = None
    if depth is not None:
        d = decode_image(depth, depth_range=depth_range, as_depth=True)
        if register:
            d = register_depth(d, Kd, K, depth_to_color, wh)
    return Frame.from_sensor(img, d, K, dist, pose=pose, size=size, new_K=new_K, name=name)


def frame_from_visual_merged(msg, **kw):
    """gs_slam_msgs/visual_merged_msg (anything with .Image, .CameraInfo and .CameraPose, the names read at
    dataset_readers.py:333, 359) -> frame_from_messages(msg.Image, msg.CameraInfo, msg.CameraPose, **kw)."""
    try:
        image, info, pose = msg.Image, msg.CameraInfo, msg.CameraPose
    except AttributeError as e:
        raise TypeError(f"msg: expected .Image, .CameraInfo and .CameraPose: {e}") from None
    return frame_from_messages(image, info, pose, **kw)
