"""The float64 TSDF reference alone (tests/tsdf_reference.py), on the CPU: it reproduces analytic answers, its mesh of a sphere is
a closed surface, and every scene the GPU tests integrate meets the conditions those tests rely on.  Also the mesh PLY round trip and
the argument checks of scene_utils.tsdf, which need no device."""
import functools
import itertools

import numpy as np
import pytest
import torch

import tsdf_reference as R


@functools.lru_cache(maxsize=None)
def scene(name):
    args, frames = R.scenes()[name]
    return R.run_scene(args, frames)


def test_fronto_parallel_plane_gives_the_analytic_tsdf():
    W, H, vs, trunc, d0 = 64, 48, 0.05, 0.15, 1.0
    fr = R.plane_frames(W, H, [np.eye(4)], (0.0, 0.0, 1.0), d0)[0]
    vol = R.RefVolume(vs, trunc)
    vol.integrate(fr)
    b = R.key_block(vol.keys)
    g = 8 * b[:, None, :] + R.local_coords()[None]
    c = (g + 0.5) * vs
    x, y, z = c[..., 0], c[..., 1], c[..., 2]
    fx, fy, cx, cy = (float(k) for k in fr.K)
    u, v = np.floor(fx * x / z + cx + 0.5), np.floor(fy * y / z + cy + 0.5)
    seen = (z > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
    sdf = (d0 - z) * np.sqrt(1 + (x / z) ** 2 + (y / z) ** 2)
    expect = np.where(seen & (sdf > -trunc), np.minimum(1.0, sdf / trunc), 0.0)
    sure = ~vol.undecided
    assert sure.mean() > 0.99
    assert np.abs(vol.tsdf - expect)[sure].max() < 1e-6          # (the depth image is float32)
    assert np.array_equal(vol.weight[sure], (seen & (sdf > -trunc))[sure].astype(float))
    assert (vol.weight > 0).sum() > 1000


def test_kuhn_tetrahedra_tile_the_cube_and_agree_on_shared_faces():
    corner = lambda c: np.array([c & 1, (c >> 1) & 1, c >> 2], float)
    vol, faces = 0.0, set()
    for a, b, c in R.KUHN:
        path = [0, 1 << a, (1 << a) | (1 << b), 7]
        p = np.array([corner(k) for k in path])
        vol += abs(np.linalg.det(p[1:] - p[0])) / 6.0
        for e in itertools.combinations(path, 2):
            d = corner(e[1]) - corner(e[0])
            if d.sum() == 2:                                   # a face diagonal
                faces.add(e)
    assert abs(vol - 1.0) < 1e-12
    # a random interior point lies in exactly one tetrahedron (the one that orders its coordinates)
    rng = np.random.default_rng(0)
    for q in rng.uniform(size=(200, 3)):
        inside = 0
        for a, b, c in R.KUHN:
            inside += q[a] >= q[b] >= q[c]
        assert inside == 1
    # six faces, one diagonal each, from the face's lowest to its highest corner; opposite faces carry the translated diagonal
    assert len(faces) == 6
    for lo, hi in faces:
        assert lo & hi == lo
    for axis in range(3):
        bit = 1 << axis
        near = {(lo, hi) for lo, hi in faces if not (lo | hi) & bit}
        far = {(lo ^ bit, hi ^ bit) for lo, hi in faces if lo & hi & bit}
        assert near == far and len(near) == 1


def test_winding_follows_the_gradient_on_linear_fields():
    rng = np.random.default_rng(5)
    keys = R.block_key(np.array([[0, 0, 0]]))
    g = R.local_coords().astype(float)
    for _ in range(6):
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        f = ((g + 0.5) @ n - 4.0 * n.sum() + 0.123) / 8.0
        D = R.Dense(keys, f[None], np.ones((1, 512)))
        tri = R.extract_triangles(D, 1.0, (0.0, 0.0, 0.0))["positions"]
        assert len(tri) > 20
        nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        assert np.all(nrm @ n > 0)
        pts = R.extract_points(D, 1.0, (0.0, 0.0, 0.0))
        assert np.all(pts["normals"] @ n > 0.999)


def sphere_mesh():
    vol = scene("sphere")
    D = R.Dense(vol.keys, vol.tsdf.astype(np.float32), vol.weight, color=vol.color)
    soup = R.extract_triangles(D, R.SPHERE["voxel_size"], (0.0, 0.0, 0.0))["positions"]
    return R.weld(soup)


def test_sphere_mesh_is_a_closed_surface():
    v, t = sphere_mesh()
    st = R.mesh_stats(v, t)
    assert st["closed"], st
    assert st["euler"] == 2
    assert st["volume"] > 0
    r = np.linalg.norm(v.astype(np.float64) - np.array(R.SPHERE["centre"]), axis=1)
    e_ref = np.abs(r - R.SPHERE["radius"]).max()
    print(f"sphere: {len(v)} vertices, {len(t)} triangles, volume {st['volume']:.5f}, E_ref {e_ref:.3e}")
    assert e_ref < R.SPHERE["voxel_size"]          # the surface lies inside the cubes whose corners change sign
    assert abs(st["volume"] / (4.0 / 3.0 * np.pi * R.SPHERE["radius"] ** 3) - 1.0) < 0.05


@pytest.mark.parametrize("name", sorted(R.scenes()))
def test_scene_conditions(name):
    """What the GPU tests rely on, for the scenes they use: few undecided voxels, no sign change on a value below its bound, no
    exact zero among the observed values."""
    vol = scene(name)
    assert len(vol.keys) >= 1
    assert vol.undecided.mean() <= 0.01, vol.undecided.mean()
    seen = vol.weight > 0
    assert not np.any(vol.tsdf[seen] == 0.0)
    D = R.Dense(vol.keys, vol.tsdf, vol.weight, err=vol.err, flag=vol.undecided)
    pts = R.extract_points(D, vol.vs, vol.origin)
    e = pts["edges"]
    idx = e[:, :3] - D.base
    jdx = idx + np.eye(3, dtype=np.int64)[e[:, 3]]
    for i in (idx, jdx):
        f, err = D.F[i[:, 0], i[:, 1], i[:, 2]], D.E[i[:, 0], i[:, 1], i[:, 2]]
        assert np.all(np.abs(f) > err)
    # every observed value next to a sign change, not only the two ends of an edge: |tsdf| above its bound wherever it is small
    small = seen & (np.abs(vol.tsdf) < 1e-4)
    assert np.all(np.abs(vol.tsdf[small]) > vol.err[small])
    print(f"{name}: {len(vol.keys)} blocks, undecided {vol.undecided.mean():.2e}, max bound {vol.err.max():.2e}, "
          f"{len(e)} edges, {int(pts['undecided'].sum())} of them on an undecided voxel")


def test_touch_sets_are_nested():
    args, frames = R.scenes()["plane"]
    vol = R.RefVolume(**args)
    must, may, nominal = vol.touch(frames[0])
    assert set(must) <= set(nominal) <= set(may)
    assert len(must) > 10
    b = R.key_block(nominal)
    assert (b.min(axis=0) < 0).all()                 # negative block coordinates on every axis
    assert np.array_equal(R.block_key(b), nominal)


def test_shifted_scene_keeps_its_bounds():
    args, frames = R.scenes()["plane"]
    a = R.run_scene(args, frames[:2])
    b = R.run_scene(args, frames[:2], shift=R.FAR_SHIFT)
    assert np.array_equal(a.keys, b.keys)
    sure = ~(a.undecided | b.undecided)
    assert np.abs(a.tsdf - b.tsdf)[sure].max() < 1e-8         # the same volume, up to float64 cancellation at 10 km
    assert b.err.max() <= 1.001 * a.err.max() + 1e-12        # the bound does not grow with the distance from the origin


def test_mesh_ply_round_trip(tmp_path):
    from scene_utils import save_mesh_ply, read_mesh_ply
    v, t = sphere_mesh()
    col = np.random.default_rng(1).uniform(size=v.shape)
    nrm = v / np.linalg.norm(v, axis=1, keepdims=True)
    p = str(tmp_path / "mesh.ply")
    save_mesh_ply(p, torch.from_numpy(v), torch.from_numpy(t), colors=col, normals=nrm)
    m = read_mesh_ply(p)
    assert np.array_equal(m["vertices"], v) and np.array_equal(m["triangles"], t)
    assert np.abs(m["colors"] - col).max() <= 0.5 / 255 + 1e-6
    assert np.array_equal(m["normals"], nrm.astype(np.float32))
    assert open(p, "rb").read(40).startswith(b"ply\nformat binary_little_endian 1.0\n")
    # no faces: a point cloud with normals
    save_mesh_ply(p, v, None, normals=nrm)
    m = read_mesh_ply(p)
    assert m["triangles"].shape == (0, 3) and m["colors"] is None and np.array_equal(m["normals"], nrm.astype(np.float32))
    with pytest.raises(ValueError):
        save_mesh_ply(p, v, np.array([[0, 1, len(v)]]))
    with pytest.raises(ValueError):
        save_mesh_ply(p, v, t, colors=col[:-1])


def test_argument_validation():
    from diff_gaussian_rasterization._C import GsrError
    from scene_utils import TSDFVolume, fibonacci_cameras
    with pytest.raises(TypeError):
        TSDFVolume("0.1", 0.3)
    with pytest.raises(ValueError):
        TSDFVolume(0.0, 0.3)
    with pytest.raises(ValueError):
        TSDFVolume(0.1, 0.05)                        # sdf_trunc < voxel_size
    with pytest.raises(ValueError):
        TSDFVolume(0.1, 0.81)                        # sdf_trunc > 8 voxel_size
    with pytest.raises(ValueError):
        TSDFVolume(0.1, 0.3, depth_trunc=0.0)
    with pytest.raises(ValueError):
        TSDFVolume(0.1, 0.3, max_weight=0.5)
    with pytest.raises(ValueError):
        TSDFVolume(0.1, 0.3, origin=(0.0, float("nan"), 0.0))
    with pytest.raises(GsrError, match="no CPU path"):
        TSDFVolume(0.1, 0.3, device="cpu")
    if torch.cuda.is_available():
        return
    # without a device the class cannot be built; its frame checks still refuse CPU tensors first
    vol = TSDFVolume.__new__(TSDFVolume)
    cam = fibonacci_cameras(1, 16, 12)[0]
    with pytest.raises(GsrError, match="no CPU path"):
        vol._frame(None, torch.zeros(12, 16), cam, None, None)
