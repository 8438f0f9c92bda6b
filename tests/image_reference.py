"""A vectorised numpy restatement of the rules of include/gsr.h for gsr_image_decode, gsr_image_encode_rgb8 and
gsr_depth_register - float32 scalar and array operations in the stated order (numpy rounds each one correctly and fuses none),
integer Bayer sums, np.minimum.at on the bit patterns - and a builder of sensor_msgs/Image messages that plants the extreme
values.  The GPU tests compare against it bit for bit; tests/test_image_messages_cpu.py checks it against values written out by
hand."""
import numpy as np

from scene_utils.messages import Image

F32 = np.float32
COLOR = {"rgb": (3, (0, 1, 2)), "bgr": (3, (2, 1, 0)), "rgba": (4, (0, 1, 2)), "bgra": (4, (2, 1, 0)), "mono": (1, (0, 0, 0))}
# the parity (x, y) of the red site: the name spells (0,0), (1,0) of row 0, then (0,1), (1,1) of row 1
BAYER_RED = {"rggb": (0, 0), "bggr": (1, 1), "gbrg": (0, 1), "grbg": (1, 0)}
COLOR_ENCODINGS = [k + b for b in ("8", "16") for k in COLOR]
BAYER_ENCODINGS = ["bayer_" + k + b for b in ("8", "16") for k in BAYER_RED]
DEPTH_ENCODINGS = ["16UC1", "32FC1"]
ENCODINGS = COLOR_ENCODINGS + BAYER_ENCODINGS + DEPTH_ENCODINGS
PLANT_LO_RAW, PLANT_HI_RAW = 500, 4000                   # 16-bit depth: raw readings planted at and beside these
PLANT_LO, PLANT_HI = F32(0.5), F32(4.0)                  # 32FC1: values planted at and beside these
UNTOUCHED = np.uint32(0xFFFFFFFF)
FOOTPRINT_CAP = 8


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def describe(encoding):
    """-> (kind, channels, bytes per channel, extra): extra = the r, g, b channel numbers / the red site's parity / None"""
    if encoding in DEPTH_ENCODINGS:
        return "depth", 1, 2 if encoding == "16UC1" else 4, None
    if encoding.startswith("bayer_"):
        name = encoding[6:10]
        return "bayer", 1, int(encoding[10:]) // 8, BAYER_RED[name]
    name = encoding.rstrip("0123456789")
    nchan, order = COLOR[name]
    return "color", nchan, int(encoding[len(name):]) // 8, order


def bytes_per_pixel(encoding):
    _, nchan, bpc, _ = describe(encoding)
    return nchan * bpc


class Message(Image):
    """an Image with host (numpy) data, and the offset from an aligned address at which a test places it on the device"""

    def __init__(self, height, width, encoding, is_bigendian, step, data, offset=0):
        super().__init__(height, width, encoding, is_bigendian, step, data)
        self.offset = offset


def samples(msg):
    """[H,W,channels] uint32: every sample (the 32FC1 float by its bits), `step` and the byte order honoured"""
    _, nchan, bpc, _ = describe(msg.encoding)
    H, W, bpp = msg.height, msg.width, nchan * bpc
    raw = np.frombuffer(bytes(msg.data), dtype=np.uint8) if isinstance(msg.data, (bytes, bytearray)) else np.asarray(msg.data)
    assert raw.size >= ((H - 1) * msg.step + W * bpp if W * H else 0)
    if W * H == 0:
        return np.zeros((H, W, nchan), dtype=np.uint32)
    rows = np.lib.stride_tricks.as_strided(raw, (H, W * bpp), (msg.step, 1)).reshape(H, W, nchan, bpc).astype(np.uint32)
    if msg.is_bigendian:
        rows = rows[..., ::-1]
    out = np.zeros((H, W, nchan), dtype=np.uint32)
    for k in range(bpc):
        out |= rows[..., k] << np.uint32(8 * k)
    return out


def decode_color(msg):
    _, _, bpc, order = describe(msg.encoding)
    s = samples(msg)
    full = F32(255.0) if bpc == 1 else F32(65535.0)
    return np.stack([s[..., c].astype(F32) / full for c in order])


def bayer_sums(s):
    """[H,W] integer samples -> (own, horizontal pair, vertical pair, four diagonals), taps reflected without repeating the edge"""
    p = np.pad(s.astype(np.int64), 1, mode="reflect")
    own = p[1:-1, 1:-1]
    horiz = p[1:-1, :-2] + p[1:-1, 2:]
    vert = p[:-2, 1:-1] + p[2:, 1:-1]
    diag = p[:-2, :-2] + p[:-2, 2:] + p[2:, :-2] + p[2:, 2:]
    return own, horiz, vert, diag


def decode_bayer(msg):
    _, _, bpc, (rx, ry) = describe(msg.encoding)
    H, W = msg.height, msg.width
    assert W >= 2 and H >= 2
    own, horiz, vert, diag = bayer_sums(samples(msg)[..., 0])
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    red_col, red_row = (x & 1) == rx, (y & 1) == ry
    red, blue = red_col & red_row, ~red_col & ~red_row
    full = 255 if bpc == 1 else 65535

    def plane(site, other, in_row):
        """a colour whose own sites are `site`, that sits diagonally of `other` and left / right of the greens of rows `in_row`"""
        total = np.where(site, own, np.where(other, diag, np.where(in_row, horiz, vert)))
        n = np.where(site, 1, np.where(other, 4, 2))
        return total.astype(F32) / (n * full).astype(F32)
    green = np.where(red | blue, horiz + vert, own).astype(F32) / (np.where(red | blue, 4, 1) * full).astype(F32)
    return np.stack([plane(red, blue, red_row), green, plane(blue, red, ~red_row)])


def decode_depth(msg, depth_scale=None, depth_range=None):
    bpc = 4 if msg.encoding == "32FC1" else 2
    scale = F32((1.0 if bpc == 4 else 0.001) if depth_scale is None else depth_scale)
    lo, hi = (None, None) if depth_range is None else depth_range
    lo, hi = F32(-np.inf if lo is None else lo), F32(np.inf if hi is None else hi)
    s = samples(msg)[..., 0]
    with np.errstate(all="ignore"):
        if bpc == 2:
            d = s.astype(F32) * scale
        else:
            f = s.view(np.float32)
            d = f * scale
            d = np.where((f > 0) & (f < np.inf), d, F32(0))
        d = np.where((d > 0) & (d < np.inf), d, F32(0))
        d = np.where((d < lo) | (d > hi), F32(0), d)
    return d.astype(F32)


def decode(msg, depth_scale=None, depth_range=None, as_depth=None):
    """what scene_utils.decode_image returns, on the host"""
    kind = describe(msg.encoding)[0]
    if as_depth is None:
        as_depth = kind == "depth"
    if as_depth:
        assert msg.encoding in ("16UC1", "32FC1", "mono16")
        return decode_depth(msg, depth_scale, depth_range)
    return decode_bayer(msg) if kind == "bayer" else decode_color(msg)


def encode_rgb8(image):
    """[3,H,W] float32 -> [H,W,3] uint8: (uint8)(min(max(c, 0), 1) * 255), truncated; NaN -> 0"""
    c = np.asarray(image, dtype=np.float32)
    with np.errstate(all="ignore"):
        v = np.where(np.isnan(c), F32(0), np.minimum(np.maximum(c, F32(0)), F32(1))).astype(F32)
        return np.ascontiguousarray(np.moveaxis((v * F32(255.0)).astype(np.int32).astype(np.uint8), 0, 2))


# ---- depth registration ---------------------------------------------------------------------------------------------------------------
def _project(uc, vc, d, Kd, Kc, T):
    fxd, fyd, cxd, cyd = (F32(v) for v in Kd)
    fxc, fyc, cxc, cyc = (F32(v) for v in Kc)
    x = ((uc - cxd) / fxd) * d
    y = ((vc - cyd) / fyd) * d
    x64, y64, z64 = x.astype(np.float64), y.astype(np.float64), d.astype(np.float64)
    q = [(((T[i, 0] * x64 + T[i, 1] * y64) + T[i, 2] * z64) + T[i, 3]).astype(F32) for i in range(3)]
    return fxc * (q[0] / q[2]) + cxc, fyc * (q[1] / q[2]) + cyc, q[2]


def register_depth(depth, Kd, Kc, T=None, size=None):
    """-> ([Hc,Wc] float32, cut flag).  Kd, Kc: (fx, fy, cx, cy); T: [3,4] or [4,4] float64, depth frame -> colour frame."""
    depth = np.asarray(depth, dtype=np.float32)
    Hd, Wd = depth.shape
    Wc, Hc = (Wd, Hd) if size is None else size
    T = np.eye(4)[:3] if T is None else np.asarray(T, dtype=np.float64)[:3]
    buf = np.full(Wc * Hc, UNTOUCHED, dtype=np.uint32)
    v, u = np.nonzero(depth > 0)
    d = depth[v, u]
    fu, fv, half = u.astype(F32), v.astype(F32), F32(0.5)
    with np.errstate(all="ignore"):
        _, _, cz = _project(fu, fv, d, Kd, Kc, T)
        ax, ay, _ = _project(fu - half, fv - half, d, Kd, Kc, T)
        bx, by, _ = _project(fu + half, fv + half, d, Kd, Kc, T)
        ok = (cz > 0) & np.isfinite(cz) & np.isfinite(ax) & np.isfinite(ay) & np.isfinite(bx) & np.isfinite(by)
        cz, ax, ay, bx, by = cz[ok], ax[ok], ay[ok], bx[ok], by[ok]

        def rnd(p, S):
            return np.clip(np.floor(p + half), F32(-1), F32(S)).astype(np.int64)
        ax, bx, ay, by = rnd(ax, Wc), rnd(bx, Wc), rnd(ay, Hc), rnd(by, Hc)
    x0, x1 = np.maximum(np.minimum(ax, bx), 0), np.minimum(np.maximum(ax, bx), Wc - 1)
    y0, y1 = np.maximum(np.minimum(ay, by), 0), np.minimum(np.maximum(ay, by), Hc - 1)
    inside = (x0 <= x1) & (y0 <= y1)
    x0, x1, y0, y1, zb = x0[inside], x1[inside], y0[inside], y1[inside], cz[inside].view(np.uint32)
    cut = bool(np.any((x1 - x0 >= FOOTPRINT_CAP) | (y1 - y0 >= FOOTPRINT_CAP)))
    x1, y1 = np.minimum(x1, x0 + FOOTPRINT_CAP - 1), np.minimum(y1, y0 + FOOTPRINT_CAP - 1)
    for dy in range(FOOTPRINT_CAP):
        for dx in range(FOOTPRINT_CAP):
            m = (x0 + dx <= x1) & (y0 + dy <= y1)
            if m.any():
                np.minimum.at(buf, (y0[m] + dy) * Wc + x0[m] + dx, zb[m])
    out = np.where(buf == UNTOUCHED, np.uint32(0), buf).view(np.float32)
    return out.reshape(Hc, Wc), cut


# ---- messages -------------------------------------------------------------------------------------------------------------------------
def pack(encoding, values, pad=0, offset=0, bigendian=False, seed=0):
    """[H,W,channels] sample values (uint; 32FC1: float32) -> Message: rows of `step` = W * bpp + pad bytes, padding filled with
    random bytes, exactly (H - 1) * step + W * bpp bytes of data"""
    _, nchan, bpc, _ = describe(encoding)
    values = np.asarray(values)
    if values.ndim == 2:
        values = values[..., None]
    H, W = values.shape[:2]
    assert values.shape[2] == nchan
    word = values.astype(np.float32).view(np.uint32) if encoding == "32FC1" else values.astype(np.uint32)
    by = np.stack([(word >> np.uint32(8 * k)) & np.uint32(255) for k in range(bpc)], axis=-1).astype(np.uint8)
    if bigendian:
        by = by[..., ::-1]
    row_bytes = W * nchan * bpc
    step = row_bytes + pad
    rows = np.random.default_rng(seed + 1000).integers(0, 256, size=(H, step), dtype=np.uint8)
    rows[:, :row_bytes] = by.reshape(H, row_bytes)
    need = (H - 1) * step + row_bytes if W * H else 0
    return Message(H, W, encoding, bool(bigendian), step, np.ascontiguousarray(rows.reshape(-1)[:need]), offset)


def depth_specials_32f():
    tiny = np.array([1, 0x80000001, 0x007FFFFF], dtype=np.uint32).view(np.float32)      # denormals of both signs
    lo, hi, inf = PLANT_LO, PLANT_HI, F32(np.inf)
    return np.concatenate([np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, -1.5, np.nextafter(lo, -inf), lo, np.nextafter(lo, inf),
                                     np.nextafter(hi, -inf), hi, np.nextafter(hi, inf), 3.0e38], dtype=np.float32), tiny])


def build_image(encoding, W, H, pad=0, offset=0, bigendian=False, seed=0):
    """A random message of the encoding with the extreme values planted (as many as it has room for): 0 and 255 / 65535; raw
    depth readings at and beside PLANT_LO_RAW / PLANT_HI_RAW; for 32FC1 NaN, +-inf, -0.0, denormals, a negative value, a value
    that overflows when scaled up, and values on either side of PLANT_LO and PLANT_HI."""
    kind, nchan, bpc, _ = describe(encoding)
    rng = np.random.default_rng(seed)
    n = W * H * nchan
    if encoding == "32FC1":
        vals = rng.uniform(0.2, 6.0, size=n).astype(np.float32)
        special = depth_specials_32f()
    else:
        full = 255 if bpc == 1 else 65535
        vals = rng.integers(0, 6000 if kind == "depth" else full + 1, size=n).astype(np.uint32)
        special = np.array([0, full], dtype=np.uint32)
        if kind == "depth":
            special = np.array([0, full, PLANT_LO_RAW - 1, PLANT_LO_RAW, PLANT_LO_RAW + 1, PLANT_HI_RAW - 1, PLANT_HI_RAW,
                                PLANT_HI_RAW + 1], dtype=np.uint32)
    k = min(n, special.size)
    if k:
        vals[rng.permutation(n)[:k]] = special[:k]
    return pack(encoding, vals.reshape(H, W, nchan), pad, offset, bigendian, seed)
