"""gsr_depth_register (csrc/image.hip, scene_utils.register_depth) against the numpy restatement of tests/image_reference.py,
BIT-EXACT and with no pixel left out: both sides do the same correctly rounded float32 operations (the point transform in float64,
rounded once), and the minimum is taken on the bit patterns, so neither the order of arrival nor a rounding boundary can make
them differ.  Depth sizes 1 x 1, 2 x 1, 64 x 1, 65 x 3 and 131 x 67 (one lane, a partial wave, a full wave, more than a wave,
more than one workgroup in both kernels), and 848 x 480 -> 640 x 480 once."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import image_reference as IR
import scene_utils as S
from diff_gaussian_rasterization import _C as GSR

pytestmark = pytest.mark.gpu
SIZES = [(1, 1), (2, 1), (64, 1), (65, 3), (131, 67)]


def intrinsics(W, H, f=0.9):
    """a camera whose principal point sits a little off the centre and whose focal lengths differ"""
    return (f * W + 0.3, f * W - 0.45, 0.5 * W - 0.2, 0.5 * H + 0.15)


@functools.lru_cache(maxsize=None)
def scene(W, H, seed=0, holes=0.1):
    """a slanted plane with noise, a share of the readings missing"""
    rng = np.random.default_rng(seed + 31 * W + H)
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = (2.0 + 0.004 * x - 0.003 * y + 0.05 * rng.standard_normal((H, W))).astype(np.float32)
    d[rng.random((H, W)) < holes] = 0
    d.setflags(write=False)
    return d


def rigid(axis, angle, t):
    a = np.asarray(axis, dtype=np.float64)
    a /= np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx
    T[:3, 3] = t
    return T


def check(depth, Kd, Kc, T=None, size=None, label=""):
    want, cut = IR.register_depth(depth, Kd, Kc, T, size)
    assert not cut, label
    got = S.register_depth(torch.from_numpy(np.array(depth)).cuda(), Kd, Kc, T, size)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == want.shape, label
    got = got.cpu().numpy()
    assert np.array_equal(IR.bits(got), IR.bits(want)), (label, int((IR.bits(got) != IR.bits(want)).sum()))
    return want


@pytest.mark.parametrize("W, H", SIZES)
def test_equal_cameras_identity(W, H):
    d = scene(W, H)
    K = intrinsics(W, H)
    want = check(d, K, K, label=(W, H))
    v, u = np.nonzero(d)
    assert np.all(want[v, u] > 0) and np.all(want[v, u] <= d[v, u])      # every reading lands at least on its own pixel
    check(d, K, K, np.eye(4)[:3], (W, H), label=(W, H, "[3,4]"))
    got = S.register_depth(torch.from_numpy(np.array(d)).cuda()[None], np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]]), K)
    assert np.array_equal(IR.bits(got.cpu().numpy()), IR.bits(want))     # [1,H,W] and a 3 x 3 K


@pytest.mark.parametrize("W, H", SIZES)
def test_rotation_translation_and_zeros(W, H):
    d, K = scene(W, H, seed=1, holes=0.3), intrinsics(W, H)
    check(d, K, K, rigid((0.2, 1.0, -0.1), 0.03, (0.02, -0.01, 0.005)), label=(W, H, "small rotation"))
    check(d, K, K, rigid((0, 0, 1), 3.0, (0.0, 0.0, 0.0)), label=(W, H, "roll: the corners change order"))
    check(d, K, K, rigid((0, 1, 0), 0.0, (1.5, -0.8, 0.0)), label=(W, H, "most readings leave the image"))
    # two layers, about 1 m and about 3 m; the colour camera sits 1.5 m ahead: the near layer ends at z' <= 0, the far one
    # arrives magnified less than 3 times
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    layers = np.where(d > 0, np.where((x + y) % 3 == 0, d - 1.3, d + 1.0), 0).astype(np.float32)
    behind = check(layers, K, K, rigid((1, 0, 0), 0.0, (0.0, 0.0, -1.5)), label=(W, H, "z' <= 0 for the near layer"))
    assert not behind.any() or behind[behind > 0].min() > 0.5         # (only the far layer arrives)
    assert not check(d, K, K, rigid((1, 0, 0), 0.0, (0.0, 0.0, -9.0)), label=(W, H, "everything behind")).any()
    zero = check(np.zeros((H, W), dtype=np.float32), K, K, label=(W, H, "all zero"))
    assert not zero.any()


@pytest.mark.parametrize("W, H", SIZES)
def test_other_resolutions(W, H):
    d, K = scene(W, H, seed=2), intrinsics(W, H)
    T = rigid((0, 1, 0), 0.01, (0.015, 0.0, 0.0))
    for s, (Wc, Hc) in ((2.0, (2 * W, 2 * H)), (0.5, ((W + 1) // 2, (H + 1) // 2)), (4.0, (4 * W - 1, 3 * H))):
        Kc = (s * K[0], s * K[1], s * K[2], s * K[3])
        check(d, K, Kc, None, (Wc, Hc), label=(W, H, s))
        check(d, K, Kc, T, (Wc, Hc), label=(W, H, s, "moved"))


def test_near_patch_occludes_the_far_plane():
    W, H = 131, 67
    K = intrinsics(W, H)
    far, near = np.full((H, W), 3.0, dtype=np.float32), np.zeros((H, W), dtype=np.float32)
    near[20:45, 50:80] = 1.0
    both = np.where(near > 0, near, far)
    T = rigid((0, 1, 0), 0.0, (0.06, 0.0, 0.0))      # a pure baseline: the patch moves ~6.5 pixels, the plane ~2.2
    only_far, _ = IR.register_depth(np.where(near > 0, 0, far).astype(np.float32), K, K, T)
    only_near, _ = IR.register_depth(near, K, K, T)
    want = check(both, K, K, T, label="occlusion")
    contested = (only_far > 0) & (only_near > 0)
    assert contested.sum() >= 1                       # the reference itself has pixels on which both land ...
    assert np.array_equal(want[contested], only_near[contested]) and np.all(want[contested] == 1.0)      # ... and the near one wins


def test_realsense_848x480_into_640x480():
    d = scene(848, 480, seed=3)
    Kd, Kc = (424.5, 424.9, 421.3, 239.2), (615.66, 615.77, 329.57, 241.67)
    want = check(d, Kd, Kc, rigid((0.1, 1.0, 0.3), 0.004, (0.0148, 0.0003, -0.0002)), (640, 480), label="848x480")
    assert (want > 0).mean() > 0.8


def test_two_runs_give_identical_bits():
    d = torch.from_numpy(np.array(scene(131, 67, seed=4))).cuda()
    K, T = intrinsics(131, 67), rigid((0, 1, 0), 0.02, (0.05, 0.0, 0.0))
    a, b = S.register_depth(d, K, K, T), S.register_depth(d, K, K, T)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_cut_footprint_sets_the_status_bit():
    """fx_c = 16 fx_d: a footprint is 17 pixels wide.  Python refuses the ratio before any launch; the C ABI cuts the footprint
    to 8 x 8, says so in the status word and returns normally - the same pixels as the restatement's cut."""
    W, H = 65, 3
    d, Kd = scene(W, H, seed=5), intrinsics(W, H)
    Kc = (16 * Kd[0], 16 * Kd[1], Kd[2], Kd[3])
    with pytest.raises(ValueError):
        S.register_depth(torch.from_numpy(np.array(d)).cuda(), Kd, Kc)
    want, cut = IR.register_depth(d, Kd, Kc)
    assert cut
    lib = GSR.lib()
    src = torch.from_numpy(np.array(d)).cuda()
    out = torch.full((H, W), -1.0, device="cuda")
    ws = torch.empty(lib.gsr_depth_register_workspace_bytes(W, H), dtype=torch.uint8, device="cuda")
    T = (C.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    for first in (7, 0):      # the call clears the word itself
        status = torch.full((1,), first, dtype=torch.int32, device="cuda")
        rc = lib.gsr_depth_register(W, H, GSR.ptr(src), (C.c_float * 4)(*Kd), (C.c_float * 4)(*Kc), T, W, H, GSR.ptr(out),
                                    GSR.ptr(status), GSR.ptr(ws), ws.numel(), GSR._stream())
        assert rc == 0 and int(status.item()) == 1
        assert np.array_equal(IR.bits(out.cpu().numpy()), IR.bits(want))
    status.fill_(7)           # and an uncut call leaves it at 0
    assert lib.gsr_depth_register(W, H, GSR.ptr(src), (C.c_float * 4)(*Kd), (C.c_float * 4)(*Kd), T, W, H, GSR.ptr(out),
                                  GSR.ptr(status), GSR.ptr(ws), ws.numel(), GSR._stream()) == 0
    assert int(status.item()) == 0
