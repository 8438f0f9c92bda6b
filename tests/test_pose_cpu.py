"""CPU tests of the camera-gradient feature's host side: scene_utils.pose (se3_exp, PoseCamera) and the C-ABI additions
(gsr_camera_grad_scratch_bytes, gsr_backward_camera); no GPU needed."""
import ctypes as C

import numpy as np
import pytest
import torch

from scene_utils import se3_exp, PoseCamera, camera_from_RT, fibonacci_cameras


def _twist(tau):
    M = torch.zeros(4, 4, dtype=tau.dtype)
    th = tau[3:]
    M[0, 1], M[0, 2], M[1, 2] = -th[2], th[1], -th[0]
    M[1, 0], M[2, 0], M[2, 1] = th[2], -th[1], th[0]
    M[:3, 3] = tau[:3]
    return M


@pytest.mark.parametrize("scale", [0.0, 1e-12, 1e-7, 1e-4, 3e-3, 0.05, 0.7, 2.5])
def test_se3_exp_matches_matrix_exp(scale):
    gen = torch.Generator().manual_seed(int(scale * 1e6) % 1000 + 1)
    tau = torch.randn(6, generator=gen, dtype=torch.float64)
    tau[3:] *= scale
    ref = torch.linalg.matrix_exp(_twist(tau))
    assert float((se3_exp(tau) - ref).abs().max()) < 1e-14
    assert float((se3_exp(tau.float()).double() - ref).abs().max()) < 5e-7
    assert torch.equal(se3_exp(tau)[3], torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64))


def test_se3_exp_gradient_finite_at_zero():
    tau = torch.zeros(6, dtype=torch.float64, requires_grad=True)
    se3_exp(tau).sum().backward()
    assert torch.isfinite(tau.grad).all()
    assert torch.autograd.gradcheck(se3_exp, (tau,))


def test_pose_camera_at_zero_reproduces_camera_from_RT():
    R = np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]])
    cam = camera_from_RT(R, np.array([0.3, -0.2, 4.1]), 0.69, 0.52, 160, 120)
    pc = PoseCamera(cam)
    assert torch.equal(pc.world_view_transform, cam.world_view_transform)
    assert torch.allclose(pc.full_proj_transform, cam.full_proj_transform, rtol=1e-6, atol=1e-6)
    assert torch.allclose(pc.camera_center, cam.camera_center, rtol=1e-6, atol=1e-6)
    for attr in ("image_width", "image_height", "FoVx", "FoVy", "znear", "zfar"):
        assert getattr(pc, attr) == getattr(cam, attr)


def test_pose_camera_gradcheck_and_commit():
    cam = fibonacci_cameras(3, 150, 100, seed=5)[1]
    pc = PoseCamera(cam, dtype=torch.float64)

    def f(tau):
        pc.tau = tau
        return pc.world_view_transform, pc.full_proj_transform, pc.camera_center
    for t0 in (torch.zeros(6, dtype=torch.float64), 1e-2 * torch.arange(1.0, 7.0, dtype=torch.float64)):
        assert torch.autograd.gradcheck(f, (t0.clone().requires_grad_(True),))
    pc.tau = torch.tensor([0.05, -0.1, 0.02, 0.01, 0.03, -0.02], dtype=torch.float64, requires_grad=True)
    before = [t.detach().clone() for t in (pc.world_view_transform, pc.full_proj_transform, pc.camera_center)]
    pc.commit()
    assert torch.equal(pc.tau, torch.zeros(6, dtype=torch.float64)) and pc.tau.requires_grad
    after = (pc.world_view_transform, pc.full_proj_transform, pc.camera_center)
    for a, b in zip(before, after):
        assert torch.allclose(a, b.detach(), rtol=0, atol=1e-14)
    # camera_center is -R^T t of the corrected W2C: the point it maps to the origin
    w2c = pc.w2c().detach()
    c = pc.camera_center.detach()
    assert torch.allclose(w2c[:3, :3] @ c + w2c[:3, 3], torch.zeros(3, dtype=torch.float64), atol=1e-6)   # (base from float32)


def test_camera_symbols_bound_with_argument_counts():
    from diff_gaussian_rasterization import _C
    lib = _C.lib()
    assert len(_C.EXPORTS["gsr_backward_camera"][1]) == len(_C.EXPORTS["gsr_backward"][1]) + 3
    assert len(_C.EXPORTS["gsr_camera_grad_scratch_bytes"][1]) == 1
    assert [f for f, _ in _C.gsr_camera_grads._fields_] == ["dL_dviewmatrix", "dL_dprojmatrix", "dL_dcampos"]
    assert C.sizeof(_C.gsr_camera_grads) == 3 * C.sizeof(C.c_void_p)
    assert lib.gsr_backward_camera.argtypes is not None


def test_camera_scratch_grows_with_P():
    from diff_gaussian_rasterization import _C
    lib = _C.lib()
    sizes = [lib.gsr_camera_grad_scratch_bytes(P) for P in (0, 1, 64, 65, 100_000, 1_000_000, 5_000_000)]
    assert all(s > 0 and s % 256 == 0 for s in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[4] > sizes[0]
    # one 32-float partial row per 64 Gaussians at least
    assert lib.gsr_camera_grad_scratch_bytes(1_000_000) >= (1_000_000 // 64) * 32 * 4


def test_camera_leaf_on_cpu_raises_no_cpu_path():
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from diff_gaussian_rasterization._C import GsrError
    vm = torch.eye(4, requires_grad=True)
    s = GaussianRasterizationSettings(16, 16, 0.5, 0.5, torch.zeros(3), 1.0, vm, torch.eye(4), 0, torch.zeros(3),
                                      False, False, False)
    P = 4
    with pytest.raises(GsrError, match="no CPU path"):
        GaussianRasterizer(s)(torch.rand(P, 3), torch.zeros(P, 3), torch.rand(P, 1), shs=torch.rand(P, 1, 3),
                              scales=torch.rand(P, 3), rotations=torch.rand(P, 4))
