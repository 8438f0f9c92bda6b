"""Host side of the map transform (scene_utils.transform, scene_utils.sh_rotation): the SH-rotation arithmetic in float64, the
constants csrc/transform.hip bakes in, transform_camera, argument validation and the anchor bookkeeping.  No GPU."""
import math
import os
import re

import numpy as np
import pytest
import torch

import transform_reference as TR
from scene_utils import GaussianModel, fibonacci_cameras, make_gaussians, transform_camera, correct_keyframes, MiniCam
from scene_utils import sh_rotation as SR
from scene_utils.sh import eval_sh, sh_basis
from scene_utils.transform import quat_from_matrix, validate_transforms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rot(seed, angle=1.0):
    return TR.random_rotation(np.random.default_rng(seed), angle)


@pytest.mark.parametrize("deg", [1, 2, 3])
def test_rotated_coefficients_give_the_same_colour_along_rotated_directions(deg):
    R = torch.tensor(_rot(1))
    gen = torch.Generator().manual_seed(deg)
    n = (deg + 1) ** 2
    c = torch.randn(50, 3, n, generator=gen, dtype=torch.float64)            # eval_sh layout [..., C, K]
    d = torch.nn.functional.normalize(torch.randn(50, 3, generator=gen, dtype=torch.float64), dim=1)
    M = TR.sh_rotation(R, deg)
    c2 = c @ M.T
    err = (eval_sh(deg, c2, d @ R.T) - eval_sh(deg, c, d)).abs().max()
    assert float(err) < 1e-12, float(err)


def test_band_matrices_compose_are_block_diagonal_and_orthogonal():
    R1, R2 = _rot(2), _rot(3, 0.7)
    M1, M2, M12 = TR.sh_rotation(R1), TR.sh_rotation(R2), TR.sh_rotation(R1 @ R2)
    assert float((M12 - M1 @ M2).abs().max()) < 1e-12
    assert float((M1 @ M1.T - torch.eye(16, dtype=torch.float64)).abs().max()) < 1e-12
    off = M1.clone()
    for l in range(4):
        off[l * l:(l + 1) ** 2, l * l:(l + 1) ** 2] = 0.0
    assert float(off.abs().max()) < 1e-12
    assert abs(float(M1[0, 0]) - 1.0) < 1e-12                                  # band 0 (features_dc) is invariant


def _baked_constants():
    """{name: array} parsed from csrc/transform_constants.inc - what the kernel is compiled with."""
    txt = open(os.path.join(ROOT, "gaussian-splatting-slam_amd", "csrc", "transform_constants.inc")).read()
    out = {}
    for name, rows, cols, body in re.findall(r"XF_CONST double (\w+)\[(\d+)\]\[(\d+)\] = \{(.*?)\};", txt, flags=re.S):
        vals = [float(v) for v in re.findall(r"-?\d+\.\d+(?:e[-+]?\d+)?", body)]
        out[name] = np.array(vals).reshape(int(rows), int(cols))
    return out


@pytest.mark.parametrize("l", [1, 2, 3])
def test_sample_constants_invert_and_reproduce_the_fit(l):
    n = 2 * l + 1
    A, Ainv = SR.sample_matrix(l), SR.sample_inverse(l)
    assert np.abs(A @ Ainv - np.eye(n)).max() < 1e-12
    assert np.linalg.cond(A) < 4.0
    baked = _baked_constants()
    dirs, ainv = baked[f"XF_DIRS{l}"], baked[f"XF_AINV{l}"]
    assert dirs.shape == (n, 3) and ainv.shape == (n, n)
    assert np.abs(np.linalg.norm(dirs, axis=1) - 1.0).max() < 1e-15
    assert np.abs(dirs - SR.sample_dirs(l)).max() < 1e-15                     # the committed file is the generator's output
    assert np.abs(SR.band_basis(l, dirs) @ ainv - np.eye(n)).max() < 1e-12
    # the table kernel's route (2 l + 1 samples) and the least-squares fit over 96 directions give the same matrix
    R = _rot(4 + l)
    D = ainv @ SR.band_basis(l, dirs @ R)
    assert np.abs(D - SR.band_rotation_from_samples(l, R)).max() < 1e-13
    assert float((torch.tensor(D) - TR.band(TR.sh_rotation(R), l)).abs().max()) < 1e-12


def test_quaternion_of_a_rotation_matches_the_reference_and_the_models_convention():
    from scene_utils.model import _build_rotation
    for seed, angle in ((1, 1.0), (2, 2.5), (3, 3.0), (4, 0.3)):
        R = _rot(seed, angle)
        q = quat_from_matrix(R)
        assert np.abs(q - TR.quat_of(R)).max() < 1e-12
        assert float((_build_rotation(torch.tensor(q)[None])[0] - torch.tensor(R)).abs().max()) < 1e-12
    # R(q_T (x) q) = R(q_T) R(q): the Hamilton product composes rotations on the left
    qa, qb = quat_from_matrix(_rot(5)), torch.tensor(quat_from_matrix(_rot(6, 0.8)))[None]
    prod, _ = TR.hamilton(qa, qb)
    assert float((_build_rotation(prod)[0] - torch.tensor(_rot(5) @ _rot(6, 0.8))).abs().max()) < 1e-12


def _cam64(cam):
    """The same camera with float64 matrices: the float32 rotation made orthogonal to float64 precision (a rigid pose is what
    transform_camera's round trip can return exactly) and full_proj_transform rebuilt as a float64 product."""
    wv = cam.world_view_transform.double()
    u, _, vt = np.linalg.svd(wv[:3, :3].numpy())
    wv[:3, :3] = torch.tensor(u @ vt)
    from scene_utils import projection_matrix
    full = wv @ projection_matrix(cam.znear, cam.zfar, cam.FoVx, cam.FoVy).double().T
    return MiniCam(cam.image_width, cam.image_height, cam.FoVy, cam.FoVx, cam.znear, cam.zfar, wv, full, cam.image_name)


@pytest.mark.parametrize("s", [1.0, 1.5])
def test_transform_camera_round_trip_and_pixels(s):
    cam = _cam64(fibonacci_cameras(3, 80, 48, seed=2)[1])
    T = TR.make_T(_rot(7), [0.3, -1.1, 0.6], s)
    cam2 = transform_camera(cam, T)
    assert cam2.world_view_transform.dtype == torch.float64
    assert (cam2.image_width, cam2.image_height, cam2.FoVx, cam2.FoVy) == (80, 48, cam.FoVx, cam.FoVy)
    back = transform_camera(cam2, np.linalg.inv(T))
    assert float((back.world_view_transform - cam.world_view_transform).abs().max()) < 1e-12
    assert float((back.full_proj_transform - cam.full_proj_transform).abs().max()) < 1e-12
    w2c = cam2.world_view_transform.T
    assert float((w2c[:3, :3] @ w2c[:3, :3].T - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-12     # stays rigid
    # a moved point through the moved camera: the same pixel, the view-space depth s times the old one
    x = torch.tensor(np.random.default_rng(0).uniform(-1.3, 1.3, size=(64, 3)))
    x2 = x @ torch.tensor(T[:3, :3]).T + torch.tensor(T[:3, 3])

    def project(c, p):
        h = torch.cat([p, torch.ones(len(p), 1, dtype=torch.float64)], dim=1) @ c.full_proj_transform
        z = (torch.cat([p, torch.ones(len(p), 1, dtype=torch.float64)], dim=1) @ c.world_view_transform)[:, 2]
        return h[:, :2] / h[:, 3:4], z
    (ndc, z), (ndc2, z2) = project(cam, x), project(cam2, x2)
    assert float((ndc - ndc2).abs().max()) < 1e-12
    assert float((z2 - s * z).abs().max()) < 1e-12 and float(z.min()) > 0.2


def test_transform_camera_keeps_float32_cameras_float32():
    cam = fibonacci_cameras(2, 64, 40, seed=1)[0]
    cam2 = transform_camera(cam, torch.tensor(TR.make_T(_rot(8), [1.0, 2.0, 3.0])))
    assert cam2.world_view_transform.dtype == torch.float32 and cam2.image_name == cam.image_name
    c = cam.camera_center.double().numpy()
    assert np.abs(cam2.camera_center.double().numpy() - (_rot(8) @ c + [1.0, 2.0, 3.0])).max() < 1e-5


def _cpu_model(P=40, deg=3):
    return GaussianModel.from_raw(make_gaussians(P, deg, seed=3))


def test_validation_errors():
    m = _cpu_model()
    R = _rot(9)
    good = TR.make_T(R, [0.1, 0.2, 0.3])
    with pytest.raises(ValueError, match="expected \\[4,4\\] or \\[K,4,4\\]"):
        m.transform_(np.eye(3))
    with pytest.raises(ValueError, match="expected \\[4,4\\] or \\[K,4,4\\]"):
        m.transform_(np.zeros((2, 2, 4, 4)))
    with pytest.raises(ValueError, match="reflection"):
        m.transform_(TR.make_T(R @ np.diag([1.0, 1.0, -1.0]), [0, 0, 0]))
    shear = good.copy()
    shear[0, 1] += 0.1
    with pytest.raises(ValueError, match="not s R"):
        m.transform_(shear)
    bottom = good.copy()
    bottom[3, 0] = 0.01
    with pytest.raises(ValueError, match="bottom row"):
        m.transform_(bottom)
    with pytest.raises(ValueError, match="allow_scale"):
        m.transform_(TR.make_T(R, [0, 0, 0], 1.5))
    with pytest.raises(ValueError, match="without `ids`"):
        m.transform_(np.stack([good, good]))
    with pytest.raises(ValueError, match="no anchors"):
        m.transform_(good, ids=[3])
    with pytest.raises(ValueError, match="2 transforms for 1 ids"):
        m.set_anchors(0).transform_(np.stack([good, good]), ids=[0])
    with pytest.raises(ValueError, match="duplicate"):
        m.transform_(np.stack([good, good]), ids=[1, 1])
    with pytest.raises(ValueError, match="moments"):
        m.transform_(good, moments="zero")
    validate_transforms(TR.make_T(R, [0, 0, 0], 1.5), allow_scale=True)


def test_cpu_model_raises_no_cpu_path():
    from diff_gaussian_rasterization import _C
    m = _cpu_model()
    before = [t.detach().clone() for t in m.parameters()]
    with pytest.raises(_C.GsrError, match="no CPU path"):
        m.transform_(TR.make_T(_rot(10), [0.1, 0.2, 0.3]))
    with pytest.raises(_C.GsrError, match="no CPU path"):
        correct_keyframes(m.set_anchors(2), {2: fibonacci_cameras(1, 32, 32)[0]}, {2: TR.make_T(_rot(10), [0, 0, 1])})
    assert all(torch.equal(a, b) for a, b in zip(before, m.parameters()))


def test_anchor_bookkeeping_on_cpu_tensors():
    m = _cpu_model(P=30)
    assert m._anchor is None
    m.prune_points(torch.arange(30) % 7 == 0)                    # without anchors: as before
    assert m._anchor is None and m.get_xyz.shape[0] == 25
    labels = torch.arange(25) % 4 - 1
    m.set_anchors(labels)
    assert m._anchor.dtype == torch.int32 and torch.equal(m._anchor.long(), labels)
    mask = torch.arange(25) % 3 == 0
    xyz = m.get_xyz.detach().clone()
    assert m.prune_points(mask) == int(mask.sum())
    assert m._anchor.shape[0] == m.get_xyz.shape[0] == 25 - int(mask.sum())
    assert torch.equal(m._anchor.long(), labels[~mask]) and torch.equal(m.get_xyz.detach(), xyz[~mask])
    assert torch.equal(_cpu_model(P=5).set_anchors(7)._anchor, torch.full((5,), 7, dtype=torch.int32))
    with pytest.raises(ValueError, match="set_anchors"):
        m.set_anchors(torch.zeros(3, dtype=torch.int64))


def test_checkpoint_carries_anchors():
    from scene_utils import capture, restore
    m = _cpu_model(P=12)
    m.training_setup(optimizer="torch")
    assert len(capture(m)) == 12                                 # a model without anchors writes what it always wrote
    m.set_anchors(torch.arange(12) % 3)
    args = capture(m)
    assert len(args) == 13
    m2 = restore(GaussianModel(3), args, optimizer="torch")
    assert torch.equal(m2._anchor, m._anchor)
    m3 = restore(GaussianModel(3), args[:12], optimizer="torch")
    assert m3._anchor is None
