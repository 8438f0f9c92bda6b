"""gsr_tsdf_extract_points and gsr_tsdf_extract_triangles against the float64 reference (tests/tsdf_reference.py): on a volume
uploaded from the reference (the same float32 values on both sides: only the extraction's float32 arithmetic separates them) and
on the device's own volume (bounds propagated from the tsdf bounds)."""
import functools

import numpy as np
import pytest
import torch

import tsdf_reference as R

pytestmark = pytest.mark.gpu
EPS = R.EPS


def H():
    import tsdf_gpu_helpers
    return tsdf_gpu_helpers


def point_bounds(ref_pts, vs):
    """float32 arithmetic of one point: t (a difference, a quotient), the edge vector, a product and a sum; colours alike on
    values <= 1; the normal from gradient components <= 2 (differences, the interpolation), the squared length, root, quotient"""
    p = EPS * (np.abs(ref_pts["points"]).max(axis=1, initial=0) + 5 * vs)
    c = 6 * EPS
    n = 1.01 * (2 * np.sqrt(3.0) * 20 * EPS / np.maximum(ref_pts["normal_length"], 1e-30) + 4 * EPS)
    return p, c, n


def compare_points(vol, D, vs, origin, what):
    ref = R.extract_points(D, vs, origin)
    p, n, c = (t.cpu().numpy().astype(np.float64) for t in vol.extract_point_cloud())
    assert len(p) == len(ref["points"]), what                 # count and, through the positions below, the same edges in the same order
    bp, bc, bn = point_bounds(ref, vs)
    ep = np.abs(p - ref["points"]).max(axis=1, initial=0)
    ec = np.abs(c - ref["colors"]).max(axis=1, initial=0)
    en = np.abs(n - ref["normals"]).max(axis=1, initial=0)
    print(f"{what}: {len(p)} points, error / bound: position {np.max(ep / bp, initial=0):.3f}, colour {np.max(ec / bc, initial=0):.3f}, "
          f"normal {np.max(en / bn, initial=0):.3f}")
    assert np.all(ep <= bp) and np.all(ec <= bc) and np.all(en <= bn), what
    # each point lies on its own edge: between the two centres along the axis, on them across it
    g, ax = ref["edges"][:, :3], ref["edges"][:, 3]
    lo = R.centre32(origin, vs, g).astype(np.float64)
    hi = R.centre32(origin, vs, g + np.eye(3, dtype=np.int64)[ax]).astype(np.float64)
    assert np.all(p >= lo - bp[:, None]) and np.all(p <= hi + bp[:, None])
    ln = np.linalg.norm(n, axis=1)
    assert np.all((np.abs(ln - 1) < 1e-5) | (ln == 0))
    return ref, p, n, c


def compare_triangles(vol, D, vs, origin, what):
    ref = R.extract_triangles(D, vs, origin)
    pos, _, col = vol.extract_triangle_mesh(weld=False)
    pos, col = pos.cpu().numpy(), col.cpu().numpy()
    assert len(pos) == len(ref["positions"]), what
    bp = EPS * (np.abs(ref["positions"]).max(axis=(1, 2), initial=0) + 5 * vs)
    ep = np.abs(pos - ref["positions"]).max(axis=(1, 2), initial=0)
    ec = np.abs(col - ref["colors"]).max(initial=0)
    print(f"{what}: {len(pos)} triangles, error / bound: position {np.max(ep / bp, initial=0):.3f}, colour {ec / (6 * EPS):.3f}")
    assert np.all(ep <= bp) and ec <= 6 * EPS, what
    return ref, pos


@functools.lru_cache(maxsize=None)
def uploaded(name):
    args, _ = R.scenes()[name]
    _, ref = H().scene_pair(name)
    vol = H().uploaded(ref, args)
    D = R.Dense(ref.keys, ref.tsdf.astype(np.float32), ref.weight, color=ref.color.astype(np.float32))
    return vol, D, args


@pytest.mark.parametrize("name", ["sphere", "plane", "near", "one_block"])
def test_points_of_an_uploaded_volume(name):
    vol, D, args = uploaded(name)
    compare_points(vol, D, args["voxel_size"], args.get("origin", (0.0, 0.0, 0.0)), name)


@pytest.mark.parametrize("name", ["sphere", "plane", "near", "one_block"])
def test_triangles_of_an_uploaded_volume(name):
    vol, D, args = uploaded(name)
    compare_triangles(vol, D, args["voxel_size"], args.get("origin", (0.0, 0.0, 0.0)), name)


def test_sphere_crosses_three_blocks_per_axis():
    _, D, _ = uploaded("sphere")
    pts = R.extract_points(D, R.SPHERE["voxel_size"], (0.0, 0.0, 0.0))
    blocks = np.unique(pts["edges"][:, :3] >> 3, axis=0)
    assert all(len(np.unique(blocks[:, a])) >= 3 for a in range(3))
    # and edges run across block faces in every direction: i at local 7 with j in the next block
    l, ax = pts["edges"][:, :3] & 7, pts["edges"][:, 3]
    assert all(np.any((ax == a) & (l[:, a] == 7)) for a in range(3))


def test_own_volume_points_against_the_reference_volume():
    """The device's own volume: its edges are the reference's except where an undecided voxel takes part, and on the common edges
    the points lie within the bound propagated from the tsdf bounds."""
    args, _ = R.scenes()["sphere"]
    vs = args["voxel_size"]
    vol, ref = H().scene_pair("sphere")
    t, w, c = H().device_rows(vol, ref.keys)
    D_dev = R.Dense(ref.keys, t, w, color=c)
    own, p, n, col = compare_points(vol, D_dev, vs, (0.0, 0.0, 0.0), "sphere, own volume")
    D_ref = R.Dense(ref.keys, ref.tsdf, ref.weight, color=ref.color, err=ref.err, flag=ref.undecided)
    want = R.extract_points(D_ref, vs, (0.0, 0.0, 0.0))
    as_set = lambda e: {tuple(r) for r in e.tolist()}
    got_e, want_e = as_set(own["edges"]), as_set(want["edges"])
    und = ref.undecided
    g_und = (8 * R.key_block(ref.keys)[:, None, :] + R.local_coords()[None])[und]
    near_und = set()
    for g in g_und.tolist():
        for a in range(3):
            near_und.add((g[0], g[1], g[2], a))
            h = list(g)
            h[a] -= 1
            near_und.add((h[0], h[1], h[2], a))
    assert (got_e ^ want_e) <= near_und
    index = {tuple(r): i for i, r in enumerate(want["edges"].tolist())}
    pick = np.array([index.get(tuple(r), -1) for r in own["edges"].tolist()])
    both = (pick >= 0) & np.array([tuple(r) not in near_und for r in own["edges"].tolist()])
    wi = pick[both]
    bound = vs * want["dt"][wi] + EPS * (np.abs(want["points"][wi]).max(axis=1) + 5 * vs)
    err = np.abs(p[both] - want["points"][wi]).max(axis=1)
    print(f"own volume: {both.sum()} common edges, position error / propagated bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound)
    # normals against the true radial direction: what the reference achieves, the device achieves
    radial = lambda q: (q - np.array(R.SPHERE["centre"])) / np.linalg.norm(q - np.array(R.SPHERE["centre"]), axis=1, keepdims=True)
    dot_dev = (n[both] * radial(p[both])).sum(axis=1)
    dot_ref = (want["normals"][wi] * radial(want["points"][wi])).sum(axis=1)
    print(f"normal . radial: device min {dot_dev.min():.4f} mean {dot_dev.mean():.4f}; reference min {dot_ref.min():.4f} "
          f"mean {dot_ref.mean():.4f}")
    assert dot_dev.min() >= dot_ref.min() - 1e-3 and dot_dev.mean() >= dot_ref.mean() - 1e-4


def test_sphere_mesh_from_the_device_volume():
    args, _ = R.scenes()["sphere"]
    vs = args["voxel_size"]
    vol, ref = H().scene_pair("sphere")
    D_ref = R.Dense(ref.keys, ref.tsdf.astype(np.float32), ref.weight, flag=ref.undecided)
    want = R.extract_triangles(D_ref, vs, (0.0, 0.0, 0.0))["positions"]
    v, t, c = vol.extract_triangle_mesh()
    soup, _, _ = vol.extract_triangle_mesh(weld=False)
    # cubes with an undecided corner may triangulate differently (at most 12 triangles each)
    U = D_ref.U
    n_und = int(sum(U[a:U.shape[0] - 1 + a, b:U.shape[1] - 1 + b, cc:U.shape[2] - 1 + cc] for a in (0, 1) for b in (0, 1)
                    for cc in (0, 1)).astype(bool).sum())
    print(f"sphere mesh: {len(soup)} triangles (reference {len(want)}), {len(v)} vertices, {n_und} cubes on an undecided voxel")
    assert abs(len(soup) - len(want)) <= 12 * n_und
    st = R.mesh_stats(v.cpu().numpy(), t.cpu().numpy())
    assert st["closed"] and st["euler"] == 2 and st["volume"] > 0, st
    assert c.shape == v.shape and float(c.min()) >= 0 and float(c.max()) <= 1
    centre = np.array(R.SPHERE["centre"])
    e_dev = np.abs(np.linalg.norm(v.cpu().numpy().astype(np.float64) - centre, axis=1) - R.SPHERE["radius"]).max()
    rv, _ = R.weld(want)
    e_ref = np.abs(np.linalg.norm(rv.astype(np.float64) - centre, axis=1) - R.SPHERE["radius"]).max()
    print(f"distance to the true sphere: device {e_dev:.4e}, reference {e_ref:.4e}")
    assert e_dev <= 1.1 * e_ref
    if n_und == 0:
        assert len(soup) == len(want)


def test_a_lone_block_with_holes():
    """One block, no neighbours, a tenth of its voxels unobserved: the one-sided and the zero gradient components, cubes that are
    not used."""
    rng = np.random.default_rng(11)
    g = R.local_coords().astype(np.float64)
    f = ((g + 0.5) @ np.array([0.3, -0.5, 0.8]) - 2.3) / 4.0 + 0.02 * np.sin(g[:, 0] + 2 * g[:, 1])
    f = np.clip(f, -1, 1).astype(np.float32)
    w = (rng.uniform(size=512) > 0.1).astype(np.float32) * 2.0
    col = rng.uniform(size=(512, 3)).astype(np.float32)
    args = dict(voxel_size=0.02, sdf_trunc=0.06, origin=(0.3, -1.7, 2.9))
    keys = R.block_key(np.array([[-3, 2, 0]]))
    vol = H().new_volume(args)
    vol.load(keys, f[None], w[None], col[None])
    for mw in (0.0, 1.0, 2.0):
        D = R.Dense(keys, f[None], w[None], min_weight=mw, color=col[None])
        vol_pts = vol.extract_point_cloud(min_weight=mw)
        ref = R.extract_points(D, 0.02, args["origin"])
        assert len(vol_pts[0]) == len(ref["points"])
        if mw == 2.0:
            assert len(ref["points"]) == 0
            continue
        bp, bc, bn = point_bounds(ref, 0.02)
        assert np.all(np.abs(vol_pts[0].cpu().numpy() - ref["points"]).max(axis=1) <= bp)
        assert np.all(np.abs(vol_pts[1].cpu().numpy() - ref["normals"]).max(axis=1) <= bn)
        tri = R.extract_triangles(D, 0.02, args["origin"])["positions"]
        soup, _, _ = vol.extract_triangle_mesh(min_weight=mw, weld=False)
        assert len(soup) == len(tri) and len(tri) > 10
        assert np.abs(soup.cpu().numpy() - tri).max() <= EPS * (3.0 + 0.1)


def test_repeats_are_bit_identical():
    vol, _, _ = uploaded("sphere")
    a, b = vol.extract_point_cloud(), vol.extract_point_cloud()
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    s1, s2 = vol.extract_triangle_mesh(weld=False), vol.extract_triangle_mesh(weld=False)
    assert torch.equal(s1[0].view(torch.int32), s2[0].view(torch.int32)) and torch.equal(s1[2].view(torch.int32), s2[2].view(torch.int32))
    m1, m2 = vol.extract_triangle_mesh(), vol.extract_triangle_mesh()
    assert all(torch.equal(x, y) for x, y in zip(m1, m2))
