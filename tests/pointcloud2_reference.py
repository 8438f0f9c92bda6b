"""Float64 / numpy restatement of the PointCloud2 decode (include/gsr.h, gsr_pc2_decode) and generators of test messages.

Everything is vectorised numpy over views of the message's byte buffer: a field is an (unaligned) strided ndarray view
(height, width) with strides (row_step, point_step) in the message's byte order.  Every rule is a fixed sequence of correctly
rounded operations, so the product is compared with this bit for bit:
  coordinates  field.astype(float32) - FLOAT32 keeps its bits, FLOAT64 / 32-bit integers round to nearest even once;
  skip_nans    drops NaN x / y / z and a FLOAT32 colour word whose bits are a NaN;
  crop         dropped iff float64(y) < min_y; dropped iff (x*x + y*y) + z*z > r*r, all float64 (the squares of float32 values are
               exact in float64, numpy does not fuse);
  pose         ((T[i,0] x + T[i,1] y) + T[i,2] z) + T[i,3] in float64, rounded to float32 once;
  colour       byte.astype(float32) / float32(255)."""
import struct

import numpy as np

INT8, UINT8, INT16, UINT16, INT32, UINT32, FLOAT32, FLOAT64 = range(1, 9)
NP_KIND = {INT8: "i1", UINT8: "u1", INT16: "i2", UINT16: "u2", INT32: "i4", UINT32: "u4", FLOAT32: "f4", FLOAT64: "f8"}
STRUCT_KIND = {INT8: "b", UINT8: "B", INT16: "h", UINT16: "H", INT32: "i", UINT32: "I", FLOAT32: "f", FLOAT64: "d"}
SIZE = {k: np.dtype(v).itemsize for k, v in NP_KIND.items()}
NAN_WORD = 0x7FC00001      # a float32 NaN pattern with a payload


class Msg:
    """the attributes of sensor_msgs/PointCloud2 and nothing else (the product takes it by duck typing); fields are tuples"""

    def __init__(self, height, width, fields, is_bigendian, point_step, row_step, data):
        self.height, self.width, self.fields, self.is_bigendian = height, width, fields, is_bigendian
        self.point_step, self.row_step, self.data = point_step, row_step, data

    @property
    def n(self):
        return self.height * self.width


def np_dtype(datatype, big):
    return np.dtype((">" if big else "<") + NP_KIND[datatype])


def field_of(msg, name):
    for f in msg.fields:
        if f[0] == name:
            return f
    return None


def color_name(msg):
    return "rgb" if field_of(msg, "rgb") else "rgba" if field_of(msg, "rgba") else None


def field_view(msg, name, as_words=False):
    """(height * width,) copy of a field in native byte order; as_words: a 4-byte field as its uint32 bits"""
    _, off, dt, _ = field_of(msg, name)
    t = np.dtype((">" if msg.is_bigendian else "<") + "u4") if as_words else np_dtype(dt, msg.is_bigendian)
    buf = np.frombuffer(bytes(msg.data), dtype=np.uint8)
    v = np.ndarray(shape=(msg.height, msg.width), dtype=t, buffer=buf, offset=off, strides=(msg.row_step, msg.point_step))
    return v.astype(t.newbyteorder("=")).reshape(-1)


def fields_f32(msg):
    """x, y, z as float32 [N] each, colour words uint32 [N] or None"""
    with np.errstate(over="ignore", invalid="ignore"):
        xyz = [field_view(msg, a).astype(np.float32) for a in "xyz"]
    c = color_name(msg)
    return xyz[0], xyz[1], xyz[2], (field_view(msg, c, as_words=True) if c else None)


def apply_pose(T, pts):
    T = np.asarray(T, dtype=np.float64)
    p = pts.astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3] for i in range(3)], axis=1).astype(np.float32)


def colors_of(words):
    w = words.astype(np.uint32)
    b = np.stack([(w >> 16) & 255, (w >> 8) & 255, w & 255], axis=1)
    return b.astype(np.float32) / np.float32(255.0)


def keep_mask(msg, min_y=None, max_range=None, skip_nans=True):
    x, y, z, w = fields_f32(msg)
    keep = np.ones(x.shape[0], dtype=bool)
    if skip_nans:
        keep &= ~(np.isnan(x) | np.isnan(y) | np.isnan(z))
        c = color_name(msg)
        if c and field_of(msg, c)[2] == FLOAT32:
            keep &= ~((w & 0x7FFFFFFF) > 0x7F800000)
    X, Y, Z = x.astype(np.float64), y.astype(np.float64), z.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if min_y is not None:
            keep &= ~(Y < float(min_y))
        if max_range is not None:
            d2 = (X * X + Y * Y) + Z * Z
            keep &= ~(d2 > float(max_range) * float(max_range))
    return keep


def decode(msg, T=None, min_y=None, max_range=None, skip_nans=True):
    """-> points float32 [n,3], colors float32 [n,3] or None, index int32 [n]"""
    x, y, z, w = fields_f32(msg)
    keep = keep_mask(msg, min_y, max_range, skip_nans)
    idx = np.nonzero(keep)[0].astype(np.int32)
    pts = np.stack([x, y, z], axis=1)[idx]
    if T is not None:
        pts = apply_pose(T, pts)
    return pts, (colors_of(w[idx]) if w is not None else None), idx


def encode_bytes(colors):
    """the colour bytes of gsr_pc2_encode: (int)(min(max(c, 0), 1) * 255.0f + 0.5f) in float32, NaN -> 0"""
    c = np.asarray(colors, dtype=np.float32)
    c = np.where(np.isnan(c), np.float32(0), np.minimum(np.maximum(c, np.float32(0)), np.float32(1)))
    return ((c * np.float32(255.0)).astype(np.float32) + np.float32(0.5)).astype(np.float32).astype(np.int32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def unpack_point(msg, n, name):
    """independent of everything above: one field of one point through struct.unpack_from"""
    _, off, dt, _ = field_of(msg, name)
    v, u = divmod(n, msg.width)
    return struct.unpack_from((">" if msg.is_bigendian else "<") + STRUCT_KIND[dt], bytes(msg.data),
                              v * msg.row_step + u * msg.point_step + off)[0]


# ---- layouts ---------------------------------------------------------------------------------------------------------------------
def _f(name, off, dt):
    return (name, off, dt, 1)


XYZ_F32 = [_f("x", 0, FLOAT32), _f("y", 4, FLOAT32), _f("z", 8, FLOAT32)]
LAYOUTS = {
    # name: (fields, point_step, big-endian, rows (None: unorganised), row padding)
    "a": (XYZ_F32 + [_f("rgb", 16, FLOAT32)], 20, False, None, 0),
    "b": (XYZ_F32 + [_f("rgb", 16, FLOAT32)], 32, False, None, 0),
    "c": ([_f("x", 1, FLOAT32), _f("y", 5, FLOAT32), _f("z", 9, FLOAT32), _f("rgb", 13, UINT32)], 19, False, None, 0),
    "d": (XYZ_F32 + [_f("rgb", 16, FLOAT32)], 20, True, None, 0),
    "e": ([_f("x", 0, FLOAT64), _f("y", 8, INT16), _f("z", 10, UINT8)], 11, False, None, 0),
    "f": (XYZ_F32 + [_f("rgb", 16, FLOAT32)], 20, False, 5, 7),
    "g1": ([_f("x", 0, INT8), _f("y", 1, UINT16), _f("z", 3, INT32), _f("rgba", 7, INT32)], 11, False, None, 0),
    "g2": ([_f("x", 2, UINT32), _f("y", 6, FLOAT64), _f("z", 14, UINT16), _f("rgb", 17, FLOAT32)], 21, True, None, 0),
    # the staging buffer's edge: point_step 64 is the largest that always stages; with 65 a full chunk of 256 points is read
    # directly and a shorter last chunk is staged - both paths in one launch
    "h64": (XYZ_F32 + [_f("rgb", 60, FLOAT32)], 64, False, None, 0),
    "h65": ([_f("x", 1, FLOAT32), _f("y", 5, FLOAT32), _f("z", 9, FLOAT32), _f("rgb", 61, FLOAT32)], 65, False, None, 0),
    # rows of three points 1000 bytes apart: a chunk's span never fits the staging buffer
    "wide": (XYZ_F32 + [_f("rgb", 12, UINT32)], 16, False, -3, 952),
}


def shape_of(name, N):
    """(height, width) of layout `name` with N points per row (organised: `rows` rows of N) or N points in all"""
    rows = LAYOUTS[name][3]
    if rows is None:
        return 1, N
    if rows < 0:                 # rows of -rows points, as many rows as it takes (N a multiple)
        assert N % -rows == 0
        return N // -rows, -rows
    return rows, N


def random_values(fields, n, rng, special=True):
    """name -> array [n] in the field's own type: floats with some NaN / +-inf (special), integers over their whole range"""
    out = {}
    for name, _, dt, _ in fields:
        if name in ("rgb", "rgba"):
            out[name] = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        elif dt in (FLOAT32, FLOAT64):
            v = rng.normal(0.0, 3.0, size=n)
            if dt == FLOAT32:
                v = v.astype(np.float32)
            if special and n >= 8:
                k = rng.integers(0, n, size=max(3, n // 16))
                v[k] = rng.choice(np.array([np.nan, np.inf, -np.inf, 0.0, -0.0]), size=k.shape[0]).astype(v.dtype)
            out[name] = v
        else:
            info = np.iinfo(NP_KIND[dt])
            out[name] = rng.integers(info.min, int(info.max) + 1, size=n, dtype=np.int64).astype(NP_KIND[dt])
    return out


def build_message(name, N, values=None, seed=0, special=True, shape=None):
    """a message of layout `name`; `values` (name -> [height * width]) overrides the random field values; the bytes between the
    fields and in the row padding are random"""
    fields, step, big, _, pad = LAYOUTS[name]
    height, width = shape if shape is not None else shape_of(name, N)
    n = height * width
    rng = np.random.default_rng(seed)
    vals = random_values(fields, n, rng, special)
    vals.update(values or {})
    row_step = width * step + pad
    buf = rng.integers(0, 256, size=height * row_step, dtype=np.uint8)
    rec = np.dtype({"names": [f[0] for f in fields],
                    "formats": [np.dtype(">u4" if big else "<u4") if f[0] in ("rgb", "rgba") else np_dtype(f[2], big) for f in fields],
                    "offsets": [f[1] for f in fields], "itemsize": step})
    for v in range(height):
        row = buf[v * row_step: v * row_step + width * step].view(rec)
        for f in fields:
            row[f[0]] = np.asarray(vals[f[0]])[v * width:(v + 1) * width]
    return Msg(height, width, list(fields), big, step, row_step, buf.tobytes())
