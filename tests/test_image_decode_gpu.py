"""sensor_msgs/Image decode on the device (csrc/image.hip, scene_utils.messages) against the numpy restatement of
tests/image_reference.py.  Every comparison is BIT-EXACT: each rule is a fixed sequence of correctly rounded float32 operations
(include/gsr.h, gsr_image_decode), so no tolerance has to be measured.

Widths: 1, 2, 3, around the wave (63 .. 65), around the kernel's row tile IMG_TILE_W = 256 (255 .. 257) and around two tiles
(511 .. 513) - at 257 and 513 the last tile holds one pixel, whose Bayer halo lies in the tile before it.  Heights 1, 2, 3: the
kernel does not tile rows (IMG_TILE_H = 1), 2 is "one above".  Row padding 0, 1, 7; the data at offsets 0 .. 3 from an aligned
address; both byte orders for the 16-bit and 32FC1 forms.  Every message is exactly as long as its layout needs, so the last
staged dword of the last row straddles the end of the buffer.  640 x 480 once for rgb8 (padded rows, odd address) and once for
bayer_rggb8."""
import functools
import itertools

import numpy as np
import pytest
import torch

import image_reference as IR
import scene_utils as S
from diff_gaussian_rasterization import _C as GSR
from scene_utils.messages import CameraInfo, Image

pytestmark = pytest.mark.gpu
TILE = GSR.IMG_TILE_W
WIDTHS = [1, 2, 3, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1]
HEIGHTS = [1, 2, 3]
PADS = [0, 1, 7]
OFFSETS = [0, 1, 2, 3]
CASES = [(enc, big) for enc in IR.ENCODINGS for big in ((False, True) if IR.describe(enc)[2] > 1 else (False,))]
DEPTH16_RANGE = (float(np.float32(IR.PLANT_LO_RAW) * np.float32(0.001)), float(np.float32(IR.PLANT_HI_RAW) * np.float32(0.001)))
DEPTH32_RANGE = (float(IR.PLANT_LO), float(IR.PLANT_HI))


def to_device(msg):
    """the message with its bytes on the device, msg.offset bytes behind an aligned address"""
    raw = torch.from_numpy(np.asarray(msg.data)).cuda()
    base = torch.zeros(msg.offset + raw.numel(), dtype=torch.uint8, device="cuda")
    base[msg.offset:] = raw
    data = base[msg.offset:]
    assert base.data_ptr() % 256 == 0 and data.data_ptr() == base.data_ptr() + msg.offset
    return Image(msg.height, msg.width, msg.encoding, msg.is_bigendian, msg.step, data)


def check(msg, label, **kw):
    want = IR.decode(msg, **kw)
    got = S.decode_image(to_device(msg), **kw)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == want.shape, label
    got = got.cpu().numpy()
    assert np.array_equal(IR.bits(got), IR.bits(want)), (label, int((IR.bits(got) != IR.bits(want)).sum()))


def test_sizes_sit_around_the_row_tile():
    assert TILE == 256 and GSR.IMG_TILE_H == 1
    assert WIDTHS == [1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513]


@pytest.mark.parametrize("encoding, big", CASES)
def test_decode_every_width_and_offset(encoding, big):
    """every width at every data offset; the height and the row padding cycle through their values along the way"""
    bayer = IR.describe(encoding)[0] == "bayer"
    for i, (W, offset) in enumerate(itertools.product(WIDTHS, OFFSETS)):
        H, pad = HEIGHTS[(i + i // 4) % 3], PADS[i % 3]
        if bayer and (W < 2 or H < 2):
            W, H = max(W, 2), max(H, 2)
        check(IR.build_image(encoding, W, H, pad, offset, big, seed=i), (encoding, big, W, H, pad, offset))


@pytest.mark.parametrize("encoding, big", [("rgb8", False), ("bgra16", True), ("mono8", False), ("bayer_grbg16", True),
                                           ("bayer_bggr8", False), ("16UC1", True), ("32FC1", False)])
@pytest.mark.parametrize("W", [3, TILE + 1])
def test_decode_every_height_padding_and_offset(encoding, big, W):
    for i, (H, pad, offset) in enumerate(itertools.product(HEIGHTS, PADS, OFFSETS)):
        if IR.describe(encoding)[0] == "bayer" and H < 2:
            continue
        check(IR.build_image(encoding, W, H, pad, offset, big, seed=100 + i), (encoding, big, W, H, pad, offset))


@pytest.mark.parametrize("pattern", sorted(IR.BAYER_RED))
@pytest.mark.parametrize("bits", [8, 16])
def test_bayer_smallest_images_and_tile_edges(pattern, bits):
    enc = f"bayer_{pattern}{bits}"
    for i, (W, H) in enumerate([(2, 2), (2, 3), (3, 2), (3, 3), (TILE, 4), (TILE + 1, 4), (TILE + 2, 5), (2 * TILE + 1, 3)]):
        for big in (False, True):
            check(IR.build_image(enc, W, H, pad=i % 3, offset=i % 4, bigendian=big, seed=200 + i), (enc, W, H, big))
    flat = IR.pack(enc, np.full((5, TILE + 3), 77 if bits == 8 else 30000))      # a constant mosaic decodes to a constant image
    got = S.decode_image(to_device(flat)).cpu().numpy()
    assert np.unique(IR.bits(got)).size == 1


@pytest.mark.parametrize("encoding, big", [("16UC1", False), ("16UC1", True), ("mono16", False), ("mono16", True), ("32FC1", False),
                                           ("32FC1", True)])
def test_depth_range_and_scale(encoding, big):
    rng16 = encoding != "32FC1"
    bounds = DEPTH16_RANGE if rng16 else DEPTH32_RANGE
    for i, (W, H) in enumerate([(5, 5), (65, 3), (TILE + 1, 2)]):
        # mono16 is built as 16UC1 so that the planted raw readings sit at and beside the bounds, then renamed
        msg = IR.build_image("16UC1" if rng16 else "32FC1", W, H, pad=i, offset=i + 1, bigendian=big, seed=300 + i)
        msg.encoding = encoding
        kw = dict(as_depth=True) if encoding == "mono16" else {}
        check(msg, (encoding, "off"), **kw)
        check(msg, (encoding, "on"), depth_range=bounds, **kw)
        check(msg, (encoding, "lo only"), depth_range=(bounds[0], None), **kw)
        check(msg, (encoding, "hi only"), depth_range=(None, bounds[1]), **kw)
        check(msg, (encoding, "scale"), depth_scale=0.00025 if rng16 else 10.0, depth_range=(0.3, 2.5), **kw)      # 3e38 * 10 overflows
        want = IR.decode(msg, depth_range=bounds, **kw)
        raw = IR.samples(msg)[..., 0]
        lo_hi = (raw == IR.PLANT_LO_RAW) | (raw == IR.PLANT_HI_RAW) if rng16 else \
            (raw == IR.bits(IR.PLANT_LO)) | (raw == IR.bits(IR.PLANT_HI))
        assert lo_hi.sum() >= 2 and np.all(want[lo_hi] > 0)                  # the values at the bounds stay ...
        assert (want == 0).sum() > (IR.decode(msg, **kw) == 0).sum()          # ... and their neighbours outside go
    if encoding == "mono16":
        check(msg, "mono16 as colour")


def test_host_data_and_device_data_agree():
    msg = IR.build_image("rgba8", 70, 3, pad=2, seed=9)
    want = IR.bits(IR.decode(msg))
    for data in (bytes(msg.data), bytearray(msg.data), msg.data):
        got = S.decode_image(Image(msg.height, msg.width, msg.encoding, False, msg.step, data))
        assert np.array_equal(IR.bits(got.cpu().numpy()), want)
    empty = S.decode_image(Image(0, 5, "rgb8", False, 15, b""))
    assert tuple(empty.shape) == (3, 0, 5) and empty.is_cuda
    assert tuple(S.decode_image(Image(4, 0, "16UC1", False, 0, b"")).shape) == (4, 0)


@functools.lru_cache(maxsize=None)
def full_frame(encoding, pad, offset):
    return IR.build_image(encoding, 640, 480, pad=pad, offset=offset, seed=11)


def test_full_frame_rgb8_640x480_padded_rows():
    msg = full_frame("rgb8", 7, 1)
    assert msg.step == 640 * 3 + 7
    check(msg, "rgb8 frame")


def test_full_frame_bayer_rggb8_640x480():
    check(full_frame("bayer_rggb8", 0, 0), "bayer frame")


# ---- encode ----------------------------------------------------------------------------------------------------------------------------
def encode_values():
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    inf = np.float32(np.inf)
    special = np.array([np.nan, -1.0, -0.0, 0.0, 1.0, 1.5, np.inf, -np.inf, 1e-45, 0.999999, 1e30], dtype=np.float32)
    return np.concatenate([special, k, np.nextafter(k, -inf), np.nextafter(k, inf)])


@pytest.mark.parametrize("W, H", [(1, 1), (4, 1), (37, 7), (37, 9), (3, 87), (640, 480)])
def test_encode_rgb8_truncates_and_round_trips(W, H):
    vals = encode_values()
    n = 3 * W * H
    x = np.resize(vals, n).astype(np.float32) if n <= 4000 else \
        np.random.default_rng(5).uniform(-0.1, 1.1, size=n).astype(np.float32)
    x[:min(n, vals.size)] = vals[:min(n, vals.size)]
    x = np.random.default_rng(6).permutation(x).reshape(3, H, W)
    want = IR.encode_rgb8(x)
    msg = S.encode_image(torch.from_numpy(x).cuda())
    assert (msg.height, msg.width, msg.encoding, msg.step, bool(msg.is_bigendian)) == (H, W, "rgb8", 3 * W, False)
    assert msg.data.is_cuda and msg.data.dtype == torch.uint8 and msg.data.numel() == n
    assert np.array_equal(msg.data.cpu().numpy().reshape(H, W, 3), want)
    back = S.decode_image(msg).cpu().numpy()
    assert np.array_equal(IR.bits(back), IR.bits(np.moveaxis(want, 2, 0).astype(np.float32) / np.float32(255)))


def test_encode_covers_every_byte_boundary():
    vals = encode_values()
    assert vals.size <= 3 * 37 * 9 and vals.size <= 3 * 3 * 87      # two of the shapes hold every planted value
    got = IR.encode_rgb8(vals[11:].reshape(3, 1, 256))
    assert np.array_equal(np.unique(got), np.arange(256))


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def _same_frame(a, b):
    for name in ("image", "depth", "mask"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), name
        if x is not None:
            assert x.is_cuda and torch.equal(x.view(torch.int32), y.view(torch.int32)), name
    for name in ("world_view_transform", "full_proj_transform", "camera_center"):
        assert torch.equal(getattr(a.camera, name), getattr(b.camera, name)), name
    assert (a.camera.image_width, a.camera.image_height) == (b.camera.image_width, b.camera.image_height)


def test_frame_from_messages_matches_from_sensor_on_the_restatement():
    W, H, Wd, Hd = 96, 72, 64, 48
    image = IR.build_image("bgr8", W, H, pad=3, offset=1, seed=21)
    rng = np.random.default_rng(22)
    raw = (1500 + 600 * np.sin(np.arange(Wd) / 9.0)[None, :] + 300 * np.cos(np.arange(Hd) / 7.0)[:, None]).astype(np.uint32)
    raw[rng.random((Hd, Wd)) < 0.05] = 0
    depth = IR.pack("16UC1", raw, pad=1, offset=2, bigendian=True, seed=23)
    K = (110.0, 0, 47.25, 0, 111.0, 35.5, 0, 0, 1)
    Kd = (75.0, 0, 31.5, 0, 74.0, 23.75, 0, 0, 1)
    info, dinfo = CameraInfo(H, W, "plumb_bob", [0.0] * 5, K), CameraInfo(Hd, Wd, "plumb_bob", [], Kd)
    T = np.eye(4)
    T[:3, 3] = (0.015, -0.002, 0.001)
    tf = ((0.05, -0.1, 0.02, 0.99), (0.3, -0.2, 1.5))
    frame = S.frame_from_messages(to_device(image), info, tf, depth=to_device(depth), depth_info=dinfo, depth_to_color=T,
                                  depth_range=(0.9, 2.2), convention="c2w", name="f0")
    k4, kd4 = (K[0], K[4], K[2], K[5]), (Kd[0], Kd[4], Kd[2], Kd[5])
    reg, cut = IR.register_depth(IR.decode(depth, depth_range=(0.9, 2.2)), kd4, k4, T, (W, H))
    assert not cut and (reg > 0).mean() > 0.5
    want = S.Frame.from_sensor(torch.from_numpy(IR.decode(image)).cuda(), torch.from_numpy(reg).cuda(), np.array(K).reshape(3, 3),
                               None, pose=S.pose_from_transform(tf, "c2w"), name="f0")
    _same_frame(frame, want)

    # a depth that is already aligned: no registration; a distorted colour camera; the message as one object
    aligned = IR.build_image("32FC1", W, H, pad=0, offset=3, seed=24)
    dist = (0.08, -0.03, 0.001, -0.002, 0.01)

    class Merged:
        Image, CameraInfo, CameraPose = to_device(image), CameraInfo(H, W, "plumb_bob", list(dist), K), tf
    frame = S.frame_from_visual_merged(Merged(), depth=to_device(aligned), size=(80, 60), new_K=(100.0, 100.0, 39.5, 29.5))
    want = S.Frame.from_sensor(torch.from_numpy(IR.decode(image)).cuda(), torch.from_numpy(IR.decode(aligned)).cuda(),
                               np.array(K).reshape(3, 3), dist, pose=S.pose_from_transform(tf), size=(80, 60),
                               new_K=(100.0, 100.0, 39.5, 29.5))
    _same_frame(frame, want)
