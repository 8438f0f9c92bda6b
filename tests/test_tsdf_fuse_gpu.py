"""From map to mesh: a small synthetic model rendered through fuse_views into a TSDF volume; the extracted surface lies on the
model, and the extracted cloud with its normals is taken by point-to-plane ICP and by create_from_pcd."""
import functools
import math

import numpy as np
import pytest
import torch

import tsdf_reference as R

pytestmark = pytest.mark.gpu
# 1000 centres on a unit sphere lie about 0.11 apart: a voxel of that size resolves the model as finely as it is sampled
RADIUS, VOXEL = 1.0, 0.1


@functools.lru_cache(maxsize=None)
def fused():
    import scene_utils as S
    from gaussian_renderer import PipelineParams
    raw = S.make_gaussians(1000, 0, seed=7)
    gen = torch.Generator().manual_seed(3)
    d = torch.nn.functional.normalize(torch.randn(1000, 3, generator=gen), dim=1)
    raw.xyz = RADIUS * d
    # discs tangent to the sphere that overlap their neighbours, thin along the normal: an opaque surface whose rendered depth
    # is that of the disc centres (the quaternion turns the local z axis onto the radial direction)
    raw.scaling = torch.tensor([math.log(0.1), math.log(0.1), math.log(0.01)]).repeat(1000, 1)
    raw.rotation = torch.nn.functional.normalize(torch.stack((1.0 + d[:, 2], -d[:, 1], d[:, 0], torch.zeros(1000)), dim=1), dim=1)
    raw.opacity = torch.full((1000, 1), 4.0)
    model = S.GaussianModel.from_raw(raw.to("cuda"), requires_grad=False)
    cams = S.fibonacci_cameras(8, 96, 72, radius=4.0, seed=1, device="cuda")
    vol = S.TSDFVolume(VOXEL, 3 * VOXEL, depth_trunc=8.0, device="cuda:0")
    S.fuse_views(model, cams, PipelineParams(), torch.zeros(3, device="cuda"), vol, alpha_min=0.95)   # (pixels on the limb blend the near and the far side)
    return model, vol


def test_fuse_views_gives_a_surface_on_the_model():
    model, vol = fused()
    assert vol.num_blocks > 8
    pts, nrm, col = vol.extract_point_cloud(min_weight=1)
    assert len(pts) > 500
    centres = model.get_xyz.detach()
    d = torch.cdist(pts, centres).min(dim=1).values
    print(f"fused: {vol.num_blocks} blocks, {len(pts)} points, distance to the nearest Gaussian centre max {float(d.max()):.3f}, "
          f"median {float(d.median()):.3f}, radius {float(pts.norm(dim=1).min()):.3f} .. {float(pts.norm(dim=1).max()):.3f}")
    assert float(d.max()) <= 2 * VOXEL
    # the front surface only: the model is a shell, the cameras are outside, normals point outward
    out = (torch.nn.functional.normalize(pts, dim=1) * nrm).sum(dim=1)
    assert float((out > 0).float().mean()) > 0.95
    v, t, c = vol.extract_triangle_mesh(min_weight=1)
    assert len(t) > 500 and int(t.max()) < len(v)
    st = R.mesh_stats(v.cpu().numpy(), t.cpu().numpy())
    print(f"fused mesh: {len(v)} vertices, {len(t)} triangles, {st}")
    assert st["non_manifold_edges"] == 0 and st["volume"] > 0
    # closed, or a surface bounded by rims rather than fragments: a manifold (no edge in three triangles) most of whose edges -
    # about 1.5 per triangle - are shared by two triangles; eight views and min_weight = 1 leave rims where one view alone saw
    assert st["closed"] or st["boundary_edges"] < 0.5 * len(t)


def test_fused_cloud_feeds_plane_icp_and_seeding():
    import scene_utils as S
    model, vol = fused()
    pts, nrm, col = vol.extract_point_cloud(min_weight=1)
    T = S.se3_exp(torch.tensor([0.02, -0.01, 0.015, 0.01, -0.02, 0.015], dtype=torch.float64))
    src = S.transform_points(pts, torch.linalg.inv(T).to(pts.device))
    res = S.registration_icp(src, pts, 3 * VOXEL, estimation="point_to_plane", target_normals=nrm, max_iteration=30)
    err = (res.transformation.cpu().double() @ torch.linalg.inv(T) - torch.eye(4, dtype=torch.float64)).abs().max()
    print(f"plane ICP on the fused cloud: fitness {res.fitness:.3f}, rmse {res.inlier_rmse:.2e}, pose error {float(err):.2e}")
    assert res.fitness > 0.9 and float(err) < 5e-3
    seeded = S.GaussianModel(0)
    seeded.create_from_pcd(pts, col.clamp(0, 1))
    assert seeded.get_xyz.shape[0] == len(pts)
