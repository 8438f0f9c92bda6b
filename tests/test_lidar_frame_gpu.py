"""From message bytes to a Frame with depth and a coloured cloud (scene_utils.lidar): a synthetic wall with a box in front of it,
sampled on scan rings, encoded as the members of a visual_merged_msg and taken through frame_from_visual_merged_map; the result
against the pieces it is made of, bit for bit, and into the consumers of Frame.depth."""
import numpy as np
import pytest
import torch

import cloud_image_reference as CR
import scene_utils as S
from scene_utils.messages import CameraInfo

pytestmark = pytest.mark.gpu
W, H = 160, 120
K = (140.0, 140.0, 79.5, 59.5)


def bits(t):
    return t.contiguous().view(torch.int32)


class Msg:
    pass


@pytest.fixture(scope="module")
def scene():
    """the message, and what went into it: the world -> camera pose, the cloud in its own frame, cloud frame -> world"""
    g = torch.Generator().manual_seed(3)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    image = torch.stack([xx / W, yy / H, 0.5 + 0.25 * torch.rand((H, W), generator=g)]).cuda()
    image = S.decode_image(S.encode_image(image))                        # what the bytes hold
    cam_pts = CR.scan_rings(W, H, K, beams=32, per_ring=400).astype(np.float64)
    w2c = np.eye(4)
    a = 0.2
    w2c[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    w2c[:3, 3] = (0.3, -0.1, 0.5)
    cloud_to_world = np.eye(4)
    cloud_to_world[:3, 3] = (1.0, 2.0, -0.5)
    to_cloud = np.linalg.inv(w2c @ cloud_to_world)                       # camera frame -> cloud frame
    cloud = (cam_pts @ to_cloud[:3, :3].T + to_cloud[:3, 3]).astype(np.float32)
    msg = Msg()
    msg.Image = S.encode_image(image)
    msg.CameraInfo = CameraInfo(H, W, "plumb_bob", [0.0] * 5, [K[0], 0, K[2], 0, K[1], K[3], 0, 0, 1])
    R = torch.tensor(w2c[:3, :3])
    qw = float(torch.sqrt(1.0 + R.trace()) / 2)
    quat = ((R[2, 1] - R[1, 2]) / (4 * qw), (R[0, 2] - R[2, 0]) / (4 * qw), (R[1, 0] - R[0, 1]) / (4 * qw), qw)
    msg.CameraPose = ([float(v) for v in quat], [float(v) for v in w2c[:3, 3]])
    msg.Local_Map = S.encode_pointcloud2(torch.from_numpy(cloud).cuda())
    return msg, torch.from_numpy(cloud_to_world), cloud


def test_message_bytes_to_frame_and_coloured_cloud(scene):
    msg, c2w, cloud = scene
    frame, points, colors = S.frame_from_visual_merged_map(msg, cloud_to_world=c2w)
    assert frame.image.shape == (3, H, W) and frame.depth.shape == (H, W) and frame.depth.is_cuda
    assert torch.equal(bits(points), bits(torch.from_numpy(cloud).cuda()))
    plain = S.frame_from_visual_merged(msg)
    assert plain.depth is None and torch.equal(plain.image, frame.image)
    # the frame's depth is densify_depth(project_cloud(...).depth), bit for bit
    T = torch.from_numpy(np.asarray(plain.camera.world_view_transform.cpu().numpy(), dtype=np.float64).T.copy() @ c2w.numpy())
    proj = S.project_cloud(points, plain.camera, w2c=T, image=plain.image, mask=plain.mask)
    dense, valid = S.densify_depth(proj.depth)
    assert torch.equal(bits(frame.depth), bits(dense))
    assert proj.n_visible > 2000 and proj.n_visible == int(proj.visible.sum()) and proj.n_candidates == int((proj.pixel >= 0).sum())
    # 32 rings, each about a pixel thick, on 120 rows: about a quarter of the pixels hold a reading; the fill reaches the rest
    assert float((proj.depth > 0).float().mean()) < 0.35 and float(valid.mean()) > 0.9
    # two surfaces, nothing in between: every depth is the box's or the wall's
    d = frame.depth[frame.depth > 0]
    assert bool((((d > 1.9) & (d < 2.1)) | ((d > 5.8) & (d < 6.2))).all())
    # the painted colours are colorize_cloud's, and project_cloud's where the row is visible
    painted, visible = S.colorize_cloud(points, plain, cloud_to_world=c2w)
    assert torch.equal(bits(colors), bits(painted)) and torch.equal(visible, proj.visible)
    assert torch.equal(bits(colors[visible]), bits(proj.colors[visible])) and not colors[~visible].any().item()
    # the red channel is x / W (to the 8 bits of the message): a row's colour tells its column
    u = (proj.pixel[visible] % W).float()
    assert float((colors[visible][:, 0] - u / W).abs().max()) < 1.5 / W + 1 / 255
    # colours already there survive where the camera does not look
    base = torch.full_like(colors, 0.25)
    again, _ = S.colorize_cloud(points, plain, colors=base, cloud_to_world=c2w)
    assert torch.equal(bits(again[visible]), bits(colors[visible])) and bool((again[~visible] == 0.25).all())
    # densify=False and options reach both stages
    sparse_frame, p2 = S.lidar_frame(plain, points, c2w, densify=False, footprint=1)
    assert torch.equal(bits(sparse_frame.depth), bits(S.project_cloud(points, plain.camera, w2c=T, mask=plain.mask, footprint=1).depth))
    f3, _, _ = S.frame_from_visual_merged_map(msg, cloud_to_world=c2w, radius=2, footprint=1, name="kf")
    assert torch.equal(bits(f3.depth), bits(S.densify_depth(sparse_frame.depth, radius=2)[0])) and f3.camera.image_name == "kf"


def test_the_frame_feeds_tsdf_and_mapping(scene):
    msg, c2w, _ = scene
    frame, points, colors = S.frame_from_visual_merged_map(msg, cloud_to_world=c2w)
    vol = S.TSDFVolume(voxel_size=0.05, sdf_trunc=0.15, depth_trunc=8.0)
    assert vol.integrate(frame) > 0
    pts, _, _ = vol.extract_point_cloud()
    assert pts.shape[0] > 0
    model = S.GaussianModel(1)
    assert model.add_from_rgbd(frame.camera, frame.image, frame.depth, stride=2) > 0
