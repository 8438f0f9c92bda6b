"""gsr_cloud_project on the device against tests/cloud_image_reference.py, bit for bit and element for element: depth, index,
pixel, z, visible, colours and the two counts - at image sizes of one lane, a partial wave, a full wave, more than a wave and
several workgroups, the same for the row count, every footprint class, and inputs that sit on the corners of the rule."""
import ctypes as C

import numpy as np
import pytest
import torch

import cloud_image_reference as CR
from diff_gaussian_rasterization import _C as GSR

pytestmark = pytest.mark.gpu
F32 = np.float32
DEV = "cuda:0"
Z_NEAR, Z_FAR = 0.5, 10.0
SCALE = CR.occlusion_scale(0.05)


def intrinsics(W, H):
    f = 0.9 * max(W, H, 4)
    return tuple(float(F32(v)) for v in (f, 1.1 * f, 0.5 * (W - 1) + 0.3, 0.5 * (H - 1) - 0.2))


def pose():
    """a cloud frame that is neither aligned with the camera nor near it"""
    a, b = 0.31, -0.17
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    T = np.eye(4)
    T[:3, :3] = Ry @ Rx
    T[:3, 3] = (0.4, -0.25, 1.5)
    return T


def make_points(N, W, H, K, T, r, seed):
    """N rows in the cloud frame whose camera-space images are spread over the image and a margin of r + 3 pixels around it, z
    from below z_near to above z_far; planted among them (as many as there is room for): NaN and Inf rows, rows behind the
    camera, duplicates of other rows, rows that share a ray (one hides the other)"""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = K
    m = r + 3
    px, py = rng.uniform(-m, W - 1 + m, N), rng.uniform(-m, H - 1 + m, N)
    z = rng.uniform(0.3, 11.0, N)
    z[rng.random(N) < 0.5] = rng.uniform(1.9, 2.1)                     # a near sheet that hides the rest
    cam = np.stack([(px - cx) / fx * z, (py - cy) / fy * z, z, np.ones(N)], axis=1)
    pts = (np.linalg.inv(T) @ cam.T).T[:, :3].astype(np.float32)
    special = [(np.nan, 0, 1), (0, np.inf, 1), (1, 1, -np.inf), (np.nan, np.nan, np.nan)]
    behind = (np.linalg.inv(T) @ np.array([0.1, 0.1, -2.0, 1.0]))[:3]
    special += [tuple(behind)] * 2
    slots = rng.permutation(N)
    k = min(len(special), N // 2)
    for s, row in zip(slots[:k], special[:k]):
        pts[s] = row
    rest = slots[k:]
    ndup = len(rest) // 8                                              # duplicate rows: equal z on one pixel
    if ndup:
        pts[rest[:ndup]] = pts[rest[ndup:2 * ndup]]
    return pts


def run(points, W, H, K, T, r, scale=SCALE, z_near=Z_NEAR, z_far=Z_FAR, image=None, mask=None, colors=None):
    """the C entry point on device tensors -> dict of numpy arrays and the two counts"""
    lib = GSR.lib()
    pts = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)).to(DEV)
    N = int(pts.shape[0])
    img = None if image is None else torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32)).to(DEV)
    msk = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask, dtype=np.float32)).to(DEV)
    col = None
    if image is not None:
        col = torch.zeros((N, 3), device=DEV) if colors is None else torch.from_numpy(np.array(colors, dtype=np.float32)).to(DEV)
    depth = torch.full((H, W), -7.0, device=DEV)
    index = torch.full((H, W), -7, dtype=torch.int32, device=DEV)
    pixel = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    z = torch.full((N,), -7.0, device=DEV)
    visible = torch.full((N,), 7, dtype=torch.uint8, device=DEV)
    count = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    cam = GSR.gsr_cloud_camera(W, H, (C.c_float * 4)(*K), (C.c_double * 12)(*np.asarray(T, dtype=np.float64)[:3].reshape(-1)),
                               z_near, z_far, r, float(scale))
    ws = torch.empty(lib.gsr_cloud_project_workspace_bytes(W, H), dtype=torch.uint8, device=DEV)
    with torch.cuda.device(0):
        GSR.check(lib.gsr_cloud_project(C.byref(cam), N, GSR.ptr(pts), GSR.ptr(img), GSR.ptr(msk), GSR.ptr(depth), GSR.ptr(index),
                                        GSR.ptr(pixel), GSR.ptr(z), GSR.ptr(visible), GSR.ptr(col), GSR.ptr(count), GSR.ptr(ws),
                                        ws.numel(), GSR._stream()))
    nv, nc = count.tolist()
    return dict(depth=depth.cpu().numpy(), index=index.cpu().numpy(), pixel=pixel.cpu().numpy(), z=z.cpu().numpy(),
                visible=visible.cpu().numpy(), colors=None if col is None else col.cpu().numpy(), n_visible=nv, n_candidates=nc)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check(got, ref, what=""):
    """every element of every output, bit for bit"""
    for name in ("depth", "z"):
        bad = bits(got[name]) != bits(getattr(ref, name))
        assert not bad.any(), f"{what}: {name} differs in {int(bad.sum())} of {bad.size} elements, first at {np.argwhere(bad)[0]}"
    for name in ("index", "pixel"):
        bad = got[name] != getattr(ref, name)
        assert not bad.any(), f"{what}: {name} differs in {int(bad.sum())} of {bad.size} elements, first at {np.argwhere(bad)[0]}"
    assert np.array_equal(got["visible"], ref.visible.astype(np.uint8)), f"{what}: visible"
    assert (got["n_visible"], got["n_candidates"]) == (ref.n_visible, ref.n_candidates), what
    if ref.colors is not None:
        bad = bits(got["colors"]) != bits(ref.colors)
        assert not bad.any(), f"{what}: colors differ in {int(bad.sum())} of {bad.size} elements, first at {np.argwhere(bad)[0]}"


def make_image(W, H, seed=3):
    return np.random.default_rng(seed).random((3, H, W), dtype=np.float32)


@pytest.mark.parametrize("r", [0, 1, 4])
@pytest.mark.parametrize("N", [1, 2, 64, 65, 257, 20011])
@pytest.mark.parametrize("W, H", [(1, 1), (2, 1), (64, 1), (65, 3), (131, 67)])
def test_bit_exact_across_sizes(W, H, N, r):
    K, T = intrinsics(W, H), pose()
    pts = make_points(N, W, H, K, T, r, seed=W * 1000 + N + r)
    image = make_image(W, H)
    before = np.random.default_rng(1).random((N, 3), dtype=np.float32)
    ref = CR.project(pts, W, H, K, T, r, SCALE, Z_NEAR, Z_FAR, image=image, colors=before)
    got = run(pts, W, H, K, T, r, image=image, colors=before)
    check(got, ref, f"{W}x{H} N={N} r={r}")
    # invisible colour rows keep the bits they had
    assert np.array_equal(bits(got["colors"][~ref.visible]), bits(before[~ref.visible]))
    # index >= 0 exactly where some visible row has pixel == p
    seen = np.zeros(W * H, bool)
    seen[got["pixel"][got["visible"] == 1]] = True
    assert np.array_equal(got["index"].reshape(-1) >= 0, seen)
    if N >= 257 and W >= 65:
        assert 0 < ref.n_visible < ref.n_candidates < N      # the case is not degenerate: hidden rows and rows outside exist


def test_corners_of_the_rule():
    """identity pose, so q is the row itself: z exactly z_near and z_far and one ulp outside; px + 0.5 exactly an integer; centres
    outside the image whose footprint reaches in, and centres more than r outside; equal z on one pixel"""
    W, H, r = 64, 48, 2
    K = (64.0, 64.0, 10.5, 7.5)
    zn, zf = F32(Z_NEAR), F32(Z_FAR)
    def at(px, py, z):      # exact in float32 for z a power of two and px, py multiples of 1/2
        return ((px - 10.5) / 64.0 * z, (py - 7.5) / 64.0 * z, z)
    rows = [(0, 0, zn), (0, 0, zf), (0, 0, np.nextafter(zn, F32(0))), (0, 0, np.nextafter(zf, F32(np.inf))),
            (0, 0, 1.0), (1 / 64.0, 0, 1.0), at(26.5, 15.5, 2.0), at(26.5, 15.5, 2.0), at(26.5, 15.5, 1.0)]
    for k in range(-r - 3, r + 4):      # centres from r + 3 pixels outside the left / top edge to inside, and the same at the far edges
        rows += [at(k, 20, 2.0), at(40, k, 2.0), at(W - 1 + k, 30, 4.0), at(50, H - 1 + k, 4.0), at(k - 0.5, k - 0.5, 8.0)]
    rows += [(3.0e38, 0, 0.6), (-3.0e38, 3.0e38, 0.6), (0, 0, np.inf), (0, 0, -0.0), (0, 0, 0.0)]      # px overflows to inf
    pts = np.array(rows, dtype=np.float32)
    for rr in (0, 1, r, 4):
        ref = CR.project(pts, W, H, K, np.eye(4), rr, SCALE, Z_NEAR, Z_FAR, image=make_image(W, H))
        assert ref.takes_part[:4].tolist() == [True, True, False, False] and ref.pixel[4] == 8 * W + 11      # 10.5 + 0.5 rounds up
        # rows 6 and 7 tie on pixel (27, 16) at z = 2, row 8 lies on their ray at z = 1 and hides both
        assert ref.pixel[6:9].tolist() == [16 * W + 27] * 3 and ref.index[16, 27] == 8 and ref.visible[6:9].tolist() == [False, False, True]
        check(run(pts, W, H, K, np.eye(4), rr, image=make_image(W, H)), ref, f"corners r={rr}")
    assert ref.n_candidates < ref.takes_part.sum()      # some centres lie outside and still take part


def test_mask_with_holes_and_no_image():
    W, H, N, r = 65, 33, 3000, 1
    K, T = intrinsics(W, H), pose()
    pts = make_points(N, W, H, K, T, r, seed=8)
    mask = (np.random.default_rng(2).random((H, W)) > 0.4).astype(np.float32)
    mask[5, 7] = np.nan                                   # mask != 0 holds for a NaN
    ref = CR.project(pts, W, H, K, T, r, SCALE, Z_NEAR, Z_FAR, mask=mask)
    got = run(pts, W, H, K, T, r, mask=mask)
    check(got, ref, "mask")
    assert got["colors"] is None
    unmasked = CR.project(pts, W, H, K, T, r, SCALE, Z_NEAR, Z_FAR)
    assert ref.n_candidates < unmasked.n_candidates and (got["index"][mask == 0] == -1).all()
    # with an image and a mask at once
    image = make_image(W, H)
    check(run(pts, W, H, K, T, r, image=image, mask=mask), CR.project(pts, W, H, K, T, r, SCALE, Z_NEAR, Z_FAR, image=image, mask=mask),
          "mask + image")


def test_no_rows():
    W, H = 65, 3
    got = run(np.zeros((0, 3), np.float32), W, H, intrinsics(W, H), pose(), 2)
    assert (got["depth"] == 0).all() and (got["index"] == -1).all() and (got["n_visible"], got["n_candidates"]) == (0, 0)
    lib = GSR.lib()      # the per-row outputs may be NULL then
    depth, index = torch.full((H, W), 5.0, device=DEV), torch.zeros((H, W), dtype=torch.int32, device=DEV)
    count = torch.full((2,), 9, dtype=torch.int64, device=DEV)
    ws = torch.empty(lib.gsr_cloud_project_workspace_bytes(W, H), dtype=torch.uint8, device=DEV)
    cam = GSR.gsr_cloud_camera(W, H, (C.c_float * 4)(*intrinsics(W, H)), (C.c_double * 12)(*pose()[:3].reshape(-1)), 0.5, 10.0, 2, 1.05)
    GSR.check(lib.gsr_cloud_project(C.byref(cam), 0, None, None, None, GSR.ptr(depth), GSR.ptr(index), None, None, None, None,
                                    GSR.ptr(count), GSR.ptr(ws), ws.numel(), GSR._stream()))
    assert not depth.any().item() and (index == -1).all().item() and count.tolist() == [0, 0]


def test_permutation_and_repeat():
    W, H, N, r = 131, 67, 20011, 2
    K, T = intrinsics(W, H), pose()
    pts = make_points(N, W, H, K, T, r, seed=11)
    a = run(pts, W, H, K, T, r)
    b = run(pts, W, H, K, T, r)
    for name in ("depth", "z"):
        assert np.array_equal(bits(a[name]), bits(b[name])), name
    for name in ("index", "pixel", "visible"):
        assert np.array_equal(a[name], b[name]), name
    perm = np.random.default_rng(4).permutation(N)
    c = run(pts[perm], W, H, K, T, r)
    assert np.array_equal(bits(c["depth"]), bits(a["depth"]))
    assert np.array_equal(c["visible"], a["visible"][perm]) and np.array_equal(c["pixel"], a["pixel"][perm])
    assert np.array_equal(bits(c["z"]), bits(a["z"][perm]))
    assert (c["n_visible"], c["n_candidates"]) == (a["n_visible"], a["n_candidates"])
    # the winner's row may differ where rows tie in z on one pixel; the pixel and the depth it names may not
    seen = a["index"] >= 0
    assert np.array_equal(seen, c["index"] >= 0)
    for out in (a, c):
        rows = out["index"][seen]
        assert np.array_equal(bits(out["z"][rows]), bits(out["depth"][seen])) and (out["visible"][rows] == 1).all()
        assert np.array_equal(out["pixel"][rows], np.flatnonzero(seen.reshape(-1)))


def test_working_size():
    """120 000 rows into 1280 x 720"""
    W, H, N, r = 1280, 720, 120000, 2
    K, T = intrinsics(W, H), pose()
    pts = make_points(N, W, H, K, T, r, seed=12)
    image = make_image(W, H)
    ref = CR.project(pts, W, H, K, T, r, SCALE, Z_NEAR, Z_FAR, image=image)
    check(run(pts, W, H, K, T, r, image=image), ref, "working size")
    assert ref.n_visible > 10000
