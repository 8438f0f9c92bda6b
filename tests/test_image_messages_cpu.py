"""CPU tests of the Image / CameraInfo / TransformStamped layer (scene_utils.messages, csrc/image.hip): the new symbols resolve and
the ABI version stays; every validation error is raised on host data without a device - which shows that it fires before any
device work (there is no device here); the numpy restatement (tests/image_reference.py) against values written out by hand;
camera_info_intrinsics and pose_from_transform against scene_utils.cameras."""
import math

import numpy as np
import pytest
import torch

import image_reference as IR
import scene_utils as S
from diff_gaussian_rasterization import _C as GSR
from scene_utils.cameras import qvec2rotmat, world_to_view
from scene_utils.messages import CameraInfo, Image

F32 = np.float32


# ---- the library ------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_resolve_and_abi_stays_7():
    lib = GSR.lib()
    for name in ("gsr_image_decode", "gsr_image_encode_rgb8", "gsr_depth_register", "gsr_depth_register_workspace_bytes"):
        assert name in GSR.EXPORTS and getattr(lib, name) is not None
    assert lib.gsr_abi_version() == 7 and GSR.ABI_VERSION == 7
    assert GSR.IMG_TILE_W == 256 and GSR.IMG_TILE_H == 1
    assert sorted(GSR.IMAGE_ENCODINGS) == sorted(IR.ENCODINGS) and sorted(GSR.IMAGE_ENCODINGS) == sorted(S.messages.IMAGE_BYTES_PER_PIXEL)
    assert sorted(GSR.IMAGE_ENCODINGS.values()) == list(range(1, 21))
    for name in IR.ENCODINGS:
        assert S.messages.IMAGE_BYTES_PER_PIXEL[name] == IR.bytes_per_pixel(name), name
    assert lib.gsr_depth_register_workspace_bytes(640, 480) >= 640 * 480 * 4


def test_c_abi_rejects_bad_arguments_before_any_launch():
    """NULL pointers come first, so none of these reaches a device"""
    import ctypes as C
    lib = GSR.lib()
    L = GSR.gsr_image_layout(4, 4, 12, GSR.IMAGE_ENCODINGS["rgb8"], 0)
    inf = math.inf
    assert lib.gsr_image_decode(None, None, 0, 1.0, -inf, inf, None, None) == -1
    assert lib.gsr_image_decode(C.byref(L), None, 48, 1.0, -inf, inf, None, None) == -1
    assert "NULL" in GSR.last_error()
    fake = C.c_void_p(256)      # never dereferenced: every call below fails a check of the layout
    for lay in (GSR.gsr_image_layout(4, 4, 12, 0, 0), GSR.gsr_image_layout(4, 4, 12, 21, 0),             # unknown codes
                GSR.gsr_image_layout(4, 4, 11, 1, 0),                                                     # step too small
                GSR.gsr_image_layout(4, 4, 12, 1, 0),                                                     # data too short (47 bytes)
                GSR.gsr_image_layout(1 << 15, 1 << 15, 3 << 15, 1, 0),                                    # 2^30 pixels
                GSR.gsr_image_layout(1, 4, 1, GSR.IMAGE_ENCODINGS["bayer_rggb8"], 0),                     # Bayer below 2 x 2
                GSR.gsr_image_layout(4, 1, 4, GSR.IMAGE_ENCODINGS["bayer_grbg16"], 0)):
        assert lib.gsr_image_decode(C.byref(lay), fake, 47, 1.0, -inf, inf, fake, None) == -1, lay.encoding
    depth = GSR.gsr_image_layout(4, 4, 8, GSR.IMAGE_ENCODINGS["16UC1"], 0)
    for scale, lo, hi in ((0.0, -inf, inf), (-1.0, -inf, inf), (inf, -inf, inf), (math.nan, -inf, inf), (1.0, math.nan, inf),
                          (1.0, -inf, math.nan)):
        assert lib.gsr_image_decode(C.byref(depth), fake, 32, scale, lo, hi, fake, None) == -1
    empty = GSR.gsr_image_layout(0, 7, 0, 1, 0)
    assert lib.gsr_image_decode(C.byref(empty), fake, 0, 1.0, -inf, inf, fake, None) == 0      # zero pixels: no launch
    assert lib.gsr_image_encode_rgb8(0, 4, fake, fake, None) == -1
    assert lib.gsr_image_encode_rgb8(4, 4, None, fake, None) == -1
    assert lib.gsr_image_encode_rgb8(4, 4, fake, C.c_void_p(258), None) == -1                     # misaligned output
    K, T = (C.c_float * 4)(8, 8, 1.5, 1.5), (C.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    assert lib.gsr_depth_register(4, 4, None, K, K, T, 4, 4, fake, fake, fake, 1 << 20, None) == -1
    assert lib.gsr_depth_register(0, 4, fake, K, K, T, 4, 4, fake, fake, fake, 1 << 20, None) == -1
    assert lib.gsr_depth_register(4, 4, fake, (C.c_float * 4)(0, 8, 1.5, 1.5), K, T, 4, 4, fake, fake, fake, 1 << 20, None) == -1
    assert lib.gsr_depth_register(4, 4, fake, K, K, (C.c_double * 12)(math.nan), 4, 4, fake, fake, fake, 1 << 20, None) == -1
    assert lib.gsr_depth_register(4, 4, fake, K, K, T, 4, 4, fake, fake, fake, 63, None) == -5      # workspace too small


# ---- validation in Python ---------------------------------------------------------------------------------------------------------------
def _rgb(**kw):
    a = dict(height=2, width=3, encoding="rgb8", is_bigendian=False, step=9, data=bytes(18))
    a.update(kw)
    return Image(**a)


@pytest.mark.parametrize("msg, kw, exc", [
    (object(), {}, TypeError), (_rgb(height=2.0), {}, TypeError), (_rgb(width=True), {}, TypeError), (_rgb(step="9"), {}, TypeError),
    (_rgb(encoding=8), {}, TypeError), (_rgb(data=[0] * 18), {}, TypeError), (_rgb(data=np.zeros(18, dtype=np.int8)), {}, TypeError),
    (_rgb(data=torch.zeros(18, dtype=torch.int8)), {}, TypeError), (_rgb(), dict(as_depth=1), TypeError),
    (_rgb(encoding="16UC1", step=6, data=bytes(12)), dict(depth_scale="1"), TypeError),
    (_rgb(encoding="16UC1", step=6, data=bytes(12)), dict(depth_range=5), TypeError),
    (_rgb(encoding="16UC1", step=6, data=bytes(12)), dict(depth_range=("a", None)), TypeError),
    (_rgb(encoding="yuv422"), {}, ValueError), (_rgb(encoding="8UC3"), {}, ValueError), (_rgb(height=-1), {}, ValueError),
    (_rgb(step=8), {}, ValueError), (_rgb(data=bytes(17)), {}, ValueError), (_rgb(width=1 << 16, height=1 << 14, step=3 << 16), {}, ValueError),
    (_rgb(encoding="bayer_rggb8", width=1, step=1), {}, ValueError), (_rgb(encoding="bayer_gbrg16", height=1, step=6), {}, ValueError),
    (_rgb(), dict(as_depth=True), ValueError), (_rgb(encoding="32FC1", step=12, data=bytes(24)), dict(as_depth=False), ValueError),
    (_rgb(), dict(depth_scale=0.001), ValueError), (_rgb(), dict(depth_range=(0, 1)), ValueError),
    (_rgb(encoding="16UC1", step=6, data=bytes(12)), dict(depth_scale=0.0), ValueError),
    (_rgb(encoding="16UC1", step=6, data=bytes(12)), dict(depth_scale=math.inf), ValueError),
    (_rgb(encoding="mono16", step=6, data=bytes(12)), dict(as_depth=True, depth_range=(2.0, 1.0)), ValueError),
    (_rgb(encoding="16UC1", step=6, data=bytes(12)), dict(depth_range=(math.nan, None)), ValueError),
    (_rgb(data=torch.zeros(18, dtype=torch.uint8)), {}, GSR.GsrError)])
def test_decode_image_validation(msg, kw, exc):
    with pytest.raises(exc):
        S.decode_image(msg, **kw)


def test_unknown_encoding_names_the_supported_ones():
    with pytest.raises(ValueError) as e:
        S.decode_image(_rgb(encoding="yuv422"))
    assert all(name in str(e.value) for name in IR.ENCODINGS)


def test_encode_image_and_register_depth_validation():
    with pytest.raises(TypeError):
        S.encode_image(np.zeros((3, 2, 2), dtype=np.float32))
    with pytest.raises(TypeError):
        S.encode_image(torch.zeros(3, 2, 2, dtype=torch.float64))
    with pytest.raises(ValueError):
        S.encode_image(torch.zeros(2, 2))
    with pytest.raises(GSR.GsrError):
        S.encode_image(torch.zeros(3, 2, 2))
    d, K = torch.ones(4, 4), (8.0, 8.0, 1.5, 1.5)
    with pytest.raises(TypeError):
        S.register_depth(d.numpy(), K, K)
    with pytest.raises(TypeError):
        S.register_depth(d.double(), K, K)
    with pytest.raises(TypeError):
        S.register_depth(d, K, K, size=4)
    with pytest.raises(ValueError):
        S.register_depth(d, K, K, depth_to_color=np.eye(3))
    with pytest.raises(ValueError):
        S.register_depth(torch.ones(4), K, K)
    with pytest.raises(ValueError):
        S.register_depth(d, (0.0, 8.0, 1.5, 1.5), K)
    with pytest.raises(ValueError):
        S.register_depth(d, K, K, size=(0, 4))
    with pytest.raises(ValueError):      # fx_c = 16 fx_d: refused before any launch (the depth is not even on a device)
        S.register_depth(d, K, (128.0, 8.0, 1.5, 1.5))
    with pytest.raises(ValueError):
        S.register_depth(d, K, (8.0, 32.5, 1.5, 1.5))
    with pytest.raises(GSR.GsrError):
        S.register_depth(d, K, (32.0, 32.0, 1.5, 1.5))


def _info(W=3, H=2, model="plumb_bob", D=(0, 0, 0, 0, 0), K=(500, 0, 1.5, 0, 510, 1.0, 0, 0, 1)):
    return CameraInfo(H, W, model, list(D), list(K))


def test_frame_from_messages_validation():
    tf = ((0, 0, 0, 1), (0, 0, 0))
    d16 = _rgb(encoding="16UC1", step=6, data=bytes(12))
    cases = [(dict(image=object(), camera_info=_info()), TypeError),
             (dict(image=_rgb(), camera_info=object()), TypeError),
             (dict(image=_rgb(), camera_info=_info(), transform=5), TypeError),
             (dict(image=_rgb(), camera_info=_info(), convention=1), TypeError),
             (dict(image=_rgb(), camera_info=_info(W=4)), ValueError),                                    # size mismatch
             (dict(image=d16, camera_info=_info()), ValueError),                                          # depth as the image
             (dict(image=_rgb(), camera_info=_info(), transform=tf, convention="cam"), ValueError),
             (dict(image=_rgb(), camera_info=_info(), depth=_rgb()), ValueError),                         # a colour image as depth
             (dict(image=_rgb(), camera_info=_info(), depth_info=_info()), ValueError),                   # no depth image
             (dict(image=_rgb(), camera_info=_info(), depth=_rgb(encoding="16UC1", width=2, step=4, data=bytes(8))), ValueError),
             (dict(image=_rgb(), camera_info=_info(), depth=d16, depth_info=_info(W=4)), ValueError),
             (dict(image=_rgb(), camera_info=_info(), depth=d16, depth_info=_info(D=(0.1, 0, 0, 0, 0))), ValueError),
             (dict(image=_rgb(), camera_info=_info(D=(0.1, 0, 0, 0, 0)), depth=d16, depth_info=_info()), ValueError),
             (dict(image=_rgb(), camera_info=_info(), depth=d16, depth_info=_info(K=(100, 0, 1.5, 0, 510, 1, 0, 0, 1))), ValueError),
             (dict(image=_rgb(), camera_info=_info(), depth=d16, depth_to_color=np.eye(2)), ValueError),
             (dict(image=_rgb(), camera_info=_info(), depth=d16, depth_range=(3, 1)), ValueError),
             (dict(image=_rgb(), camera_info=_info(), size=(0, 2)), ValueError)]
    for kw, exc in cases:
        with pytest.raises(exc):
            S.frame_from_messages(**kw)
    with pytest.raises(TypeError):
        S.frame_from_visual_merged(object())


# ---- the restatement against values written out by hand ----------------------------------------------------------------------------------
def _q(num, den):
    return F32(num) / F32(den)


def _planes(rows):
    return np.array([[[_q(*c) for c in r] for r in p] for p in rows], dtype=np.float32)


A, Bq, Cq = (10, 255), (40, 255), (100, 1020)      # 2 x 2 of 10 20 / 30 40: every tap of a colour is its one site
BAYER_2X2 = {
    "rggb": [[[A, A], [A, A]], [[Cq, (20, 255)], [(30, 255), Cq]], [[Bq, Bq], [Bq, Bq]]],
    "bggr": [[[Bq, Bq], [Bq, Bq]], [[Cq, (20, 255)], [(30, 255), Cq]], [[A, A], [A, A]]],
    "gbrg": [[[(30, 255)] * 2] * 2, [[A, Cq], [Cq, Bq]], [[(20, 255)] * 2] * 2],
    "grbg": [[[(20, 255)] * 2] * 2, [[A, Cq], [Cq, Bq]], [[(30, 255)] * 2] * 2],
}
# 3 x 3 of 1 2 3 / 4 5 6 / 7 8 9.  With the reflection: horizontal pairs 4 4 4 / 10 10 10 / 16 16 16, vertical pairs 8 10 12 in
# every row, the four diagonals 20 everywhere.
_RGGB_R = [[(1, 255), (4, 510), (3, 255)], [(8, 510), (20, 1020), (12, 510)], [(7, 255), (16, 510), (9, 255)]]
_RGGB_G = [[(12, 1020), (2, 255), (16, 1020)], [(4, 255), (20, 1020), (6, 255)], [(24, 1020), (8, 255), (28, 1020)]]
_RGGB_B = [[(20, 1020), (10, 510), (20, 1020)], [(10, 510), (5, 255), (10, 510)], [(20, 1020), (10, 510), (20, 1020)]]
_GRBG_R = [[(4, 510), (2, 255), (4, 510)], [(20, 1020), (10, 510), (20, 1020)], [(16, 510), (8, 255), (16, 510)]]
_GRBG_G = [[(1, 255), (14, 1020), (3, 255)], [(18, 1020), (5, 255), (22, 1020)], [(7, 255), (26, 1020), (9, 255)]]
_GRBG_B = [[(8, 510), (20, 1020), (12, 510)], [(4, 255), (10, 510), (6, 255)], [(8, 510), (20, 1020), (12, 510)]]
BAYER_3X3 = {"rggb": [_RGGB_R, _RGGB_G, _RGGB_B], "bggr": [_RGGB_B, _RGGB_G, _RGGB_R],
             "grbg": [_GRBG_R, _GRBG_G, _GRBG_B], "gbrg": [_GRBG_B, _GRBG_G, _GRBG_R]}


@pytest.mark.parametrize("pattern", sorted(IR.BAYER_RED))
def test_reference_bayer_2x2_and_3x3_by_hand(pattern):
    got = IR.decode(IR.pack(f"bayer_{pattern}8", np.array([[10, 20], [30, 40]]), pad=3))
    assert np.array_equal(IR.bits(got), IR.bits(_planes(BAYER_2X2[pattern]))), pattern
    got = IR.decode(IR.pack(f"bayer_{pattern}8", np.arange(1, 10).reshape(3, 3), pad=1))
    assert np.array_equal(IR.bits(got), IR.bits(_planes(BAYER_3X3[pattern]))), pattern
    # the 16-bit form: the same sums over n * 65535, in either byte order
    for big in (False, True):
        got = IR.decode(IR.pack(f"bayer_{pattern}16", np.arange(1, 10).reshape(3, 3) * 257, bigendian=big))
        want = _planes([[[(c[0] * 257, c[1] * 257) for c in r] for r in p] for p in BAYER_3X3[pattern]])
        assert np.array_equal(IR.bits(got), IR.bits(want)), (pattern, big)


def test_reference_colour_and_big_endian_depth_by_hand():
    msg = Image(1, 2, "bgra8", False, 9, bytes([0, 128, 255, 7, 51, 102, 153, 9, 77]))
    want = np.array([[[_q(255, 255), _q(153, 255)]], [[_q(128, 255), _q(102, 255)]], [[_q(0, 255), _q(51, 255)]]])
    assert np.array_equal(IR.bits(IR.decode(msg)), IR.bits(want))
    msg = Image(2, 2, "16UC1", True, 5, bytes([0x03, 0xE8, 0x00, 0x00, 0xAA, 0xFF, 0xFF, 0x01, 0xF4]))      # 1000, 0 / 65535, 500
    d = IR.decode(msg)
    mm = F32(0.001)
    assert np.array_equal(IR.bits(d), IR.bits(np.array([[F32(1000) * mm, 0], [F32(65535) * mm, F32(500) * mm]])))
    assert float(d[0, 0]) == 1.0 and float(d[1, 1]) == 0.5
    d = IR.decode(msg, depth_range=(0.5, 1.0))                      # the bounds themselves stay
    assert d.tolist() == [[1.0, 0.0], [0.0, 0.5]]
    assert IR.decode(msg, depth_range=(0.6, None)).tolist() == [[1.0, 0.0], [float(F32(65535) * mm), 0.0]]
    little = Image(2, 2, "16UC1", False, 5, msg.data)
    assert float(IR.decode(little)[0, 0]) == float(F32(0xE803) * mm)
    f = np.array([[np.nan, -0.0, 2.5], [np.inf, -3.0, 1e-40]], dtype=np.float32)
    assert IR.bits(IR.decode(IR.pack("32FC1", f, bigendian=True))).tolist() == IR.bits(np.array([[0, 0, 2.5], [0, 0, 1e-40]])).tolist()
    assert IR.decode(IR.pack("32FC1", f), depth_scale=0.5, depth_range=(0.1, 1.0)).tolist() == [[0, 0, 0], [0, 0, 0]]


def test_reference_encode_truncates():
    c = np.array([np.nan, -0.5, 0.0, 0.999, 1.0, 7.0, 0.5, 128 / 255], dtype=np.float32)
    img = np.stack([c, c, c]).reshape(3, 1, 8)
    assert IR.encode_rgb8(img)[0, :, 0].tolist() == [0, 0, 0, 254, 255, 255, 127, 128]


def test_reference_register_depth_splat_and_occlusion_by_hand():
    K = (8.0, 8.0, 1.5, 1.5)
    d = np.zeros((4, 4), dtype=np.float32)
    d[1, 1] = 2.0      # corners (0.5, 0.5) and (1.5, 1.5) project onto themselves, round to 1 and 2: the 2 x 2 splat
    out, cut = IR.register_depth(d, K, K)
    assert not cut and out.tolist() == [[0, 0, 0, 0], [0, 2, 2, 0], [0, 2, 2, 0], [0, 0, 0, 0]]
    d[1, 2] = 1.0      # covers columns 2 .. 3: the nearer reading wins where both land
    out, _ = IR.register_depth(d, K, K)
    assert out.tolist() == [[0, 0, 0, 0], [0, 2, 1, 1], [0, 2, 1, 1], [0, 0, 0, 0]]
    T = np.eye(4)
    T[0, 3] = 0.25     # a baseline of 0.25 at depth 2 and fx = 8: one pixel to the right; at depth 1: two pixels
    out, _ = IR.register_depth(d, K, K, T)
    assert out.tolist() == [[0, 0, 0, 0], [0, 0, 2, 2], [0, 0, 2, 2], [0, 0, 0, 0]]
    out, cut = IR.register_depth(d, K, (128.0, 128.0, 1.5, 1.5), size=(64, 64))
    assert cut and float(out.max()) == 2.0
    T[2, 3] = -5.0     # everything ends behind the colour camera
    assert not IR.register_depth(d, K, K, T)[0].any()


# ---- CameraInfo and TransformStamped ------------------------------------------------------------------------------------------------------
def test_camera_info_intrinsics():
    K, dist, wh = S.camera_info_intrinsics(_info(W=640, H=480, K=(615.5, 0, 329.5, 0, 615.75, 241.5, 0, 0, 1)))
    assert K.dtype == np.float64 and K.tolist() == [[615.5, 0, 329.5], [0, 615.75, 241.5], [0, 0, 1]]
    assert dist is None and wh == (640, 480)
    assert S.camera_info_intrinsics(_info(D=(0.1, -0.2, 0.001)))[1] == (0.1, -0.2, 0.001, 0.0, 0.0)
    assert S.camera_info_intrinsics(_info(D=(0.1, -0.2, 0.001, 0.002, 0.03)))[1] == (0.1, -0.2, 0.001, 0.002, 0.03)
    assert S.camera_info_intrinsics(_info(model="", D=(0.1, 0, 0, 0, 0)))[1] is None
    assert S.camera_info_intrinsics(_info(model="plumb_bob", D=()))[1] is None
    assert S.camera_info_intrinsics(_info(model="rational_polynomial", D=(0.1, 0, 0, 0, 0.2, 0, 0, 0)))[1] == (0.1, 0, 0, 0, 0.2)
    assert S.camera_info_intrinsics(_info(K=np.array([[500, 0, 1.5], [0, 510, 1.0], [0, 0, 1.0]])))[0][1, 1] == 510
    for bad, exc in ((_info(model="rational_polynomial", D=(0.1, 0, 0, 0, 0, 0.3, 0, 0)), ValueError),
                     (_info(model="plumb_bob", D=(0, 0, 0, 0, 0, 0)), ValueError), (_info(model="equidistant"), ValueError),
                     (_info(K=(0, 0, 1, 0, 5, 1, 0, 0, 1)), ValueError), (_info(K=(5, 0, 1, 0, -5, 1, 0, 0, 1)), ValueError),
                     (_info(K=(5, 0, 1, 0, 5, 1)), ValueError), (_info(K=(5, 0, math.nan, 0, 5, 1, 0, 0, 1)), ValueError),
                     (_info(model=None), TypeError), (_info(K="K"), TypeError), (_info(W=1.5), TypeError), (object(), TypeError)):
        with pytest.raises(exc):
            S.camera_info_intrinsics(bad)


QUATERNIONS = [(0.0, 0.0, math.sin(0.35), math.cos(0.35)), (0.5, -0.5, 0.5, 0.5), (0.1, 0.7, -0.2, 0.4), (0.0, 0.0, 0.0, 1.0)]


@pytest.mark.parametrize("q", QUATERNIONS)
def test_pose_from_transform(q):
    t = (1.5, -2.25, 10.0)
    n = math.sqrt(sum(c * c for c in q))
    x, y, z, w = (c / n for c in q)

    class V:
        def __init__(self, **kw):
            self.__dict__.update(kw)
    tf = V(transform=V(rotation=V(x=q[0], y=q[1], z=q[2], w=q[3]), translation=V(x=t[0], y=t[1], z=t[2])))
    M = S.pose_from_transform(tf)
    assert M.dtype == torch.float64 and tuple(M.shape) == (4, 4) and not M.is_cuda
    assert torch.equal(M, S.pose_from_transform((q, t), "w2c")) and torch.equal(M, S.pose_matrix(q, t))
    # the reference's reading (dataset_readers.py:333-338, 365-366): R = qvec2rotmat(w, x, y, z)^T and T = t give this view matrix
    want = world_to_view(qvec2rotmat((w, x, y, z)).T, np.array(t))      # (float32)
    assert np.abs(M.numpy() - want.astype(np.float64)).max() <= 2e-6   # 10 * 2^-24 * a few roundings of the float32 inverse
    inv = S.pose_from_transform(tf, "c2w")
    assert np.abs(np.linalg.inv(inv.numpy()) - M.numpy()).max() <= 1e-14
    assert np.abs(inv.numpy() @ M.numpy() - np.eye(4)).max() <= 1e-14
    for bad, exc in (((q, t, 1), TypeError), (5, TypeError), (V(transform=V(rotation=1)), TypeError), ((q[:3], t), ValueError)):
        with pytest.raises(exc):
            S.pose_from_transform(bad)
    with pytest.raises(ValueError):
        S.pose_from_transform(tf, "view")


def test_build_image_is_fast_and_plants_the_extremes():
    import time
    t0 = time.perf_counter()
    msg = IR.build_image("bayer_rggb8", 640, 480, pad=5, seed=1)
    out = IR.decode(msg)
    assert time.perf_counter() - t0 < 1.0 and out.shape == (3, 480, 640)
    s = IR.samples(msg)
    assert s.min() == 0 and s.max() == 255 and msg.step == 645 and len(msg.data) == 479 * 645 + 640
    f = IR.samples(IR.build_image("32FC1", 9, 7, bigendian=True, seed=2)).view(np.float32)
    assert np.isnan(f).any() and np.isinf(f).sum() == 2 and (f == IR.PLANT_LO).any() and (f == IR.PLANT_HI).any()
    assert ((f != 0) & (np.abs(f) < np.finfo(np.float32).tiny)).sum() == 3
    raw = IR.samples(IR.build_image("16UC1", 5, 5, seed=3))
    assert all((raw == v).any() for v in (0, 65535, 499, 500, 501, 3999, 4000, 4001))
