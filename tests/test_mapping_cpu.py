"""CPU tests of the mapping surface: the `simple_knn` import of the reference resolves, the library exports the new entry points
and validates their arguments before anything is launched, the CPU restatements agree with hand-computed cases and with the
project's projection convention, and nothing falls back to the CPU."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import mapping_reference as MR
from scene_utils import GaussianModel, fibonacci_cameras, make_gaussians

INVALID, TOO_SMALL = -1, -5


def test_reference_import_resolves():
    from simple_knn._C import distCUDA2              # reference scene/gaussian_model.py:20
    import simple_knn
    assert callable(distCUDA2) and callable(simple_knn.knn_dist2)


def test_library_exports_and_size_queries():
    from diff_gaussian_rasterization import _C
    lib = _C.lib()
    for n in ("gsr_knn_workspace_bytes", "gsr_knn_dist2", "gsr_unproject_workspace_bytes", "gsr_unproject_rgbd"):
        assert n in _C.EXPORTS and hasattr(lib, n)
    a, b, c = (lib.gsr_knn_workspace_bytes(n) for n in (1000, 100000, 5000000))
    assert 0 < a < b < c
    assert c >= 5000000 * (16 + 16)                   # sorted points + two key / value pairs at least
    u0, u1 = lib.gsr_unproject_workspace_bytes(64, 48), lib.gsr_unproject_workspace_bytes(1920, 1080)
    assert 0 < u0 < u1 and u1 >= 1920 * 1080 * 8


def test_knn_argument_errors_without_a_gpu():
    from diff_gaussian_rasterization import _C
    lib = _C.lib()
    fake = C.c_void_p(4096)                           # never dereferenced: every case fails before a launch
    big = lib.gsr_knn_workspace_bytes(100)
    call = lib.gsr_knn_dist2
    assert call(0, fake, 0, fake, fake, big, None) == INVALID
    assert call(-3, fake, 0, fake, fake, big, None) == INVALID
    assert call(100, None, 0, fake, fake, big, None) == INVALID
    assert call(100, fake, 0, None, fake, big, None) == INVALID
    assert call(100, fake, 0, fake, None, big, None) == INVALID
    assert call(100, fake, -1, fake, fake, big, None) == INVALID
    assert call(100, fake, 100, fake, fake, big, None) == INVALID
    assert call(100, fake, 0, fake, fake, big - 1, None) == TOO_SMALL
    assert "workspace" in _C.last_error()


def test_unproject_argument_errors_without_a_gpu():
    from diff_gaussian_rasterization import _C
    lib = _C.lib()
    fake = C.c_void_p(4096)
    W, H = 40, 30
    ws = lib.gsr_unproject_workspace_bytes(W, H)

    def params(**kw):
        d = dict(image_height=H, image_width=W, tanfovx=0.5, tanfovy=0.4, viewmatrix=4096, stride=1, min_depth=0.2,
                 max_depth=10.0, alpha_below=0.5, front_margin=0.05)
        d.update(kw)
        return _C.gsr_unproject_params(**d)

    def call(p, depth=fake, color=fake, xyz=fake, rgb=fake, cap=W * H, count=fake, work=fake, nbytes=ws):
        return lib.gsr_unproject_rgbd(C.byref(p) if p is not None else None, depth, color, None, None, xyz, rgb, cap, count,
                                      work, nbytes, None)
    assert call(None) == INVALID
    assert call(params(), depth=None) == INVALID
    assert call(params(), color=None) == INVALID
    assert call(params(), count=None) == INVALID
    assert call(params(), work=None) == INVALID
    assert call(params(), xyz=None) == INVALID
    assert call(params(), cap=-1) == INVALID
    assert call(params(stride=0)) == INVALID
    assert call(params(image_width=0)) == INVALID
    assert call(params(viewmatrix=None)) == INVALID
    assert call(params(tanfovx=0.0)) == INVALID
    assert call(params(), nbytes=ws - 1) == TOO_SMALL


def test_bruteforce_on_a_hand_computed_case():
    # on a line: 0, 1, 3, 7, 7 (a duplicate)
    pts = np.array([[0, 0, 0], [1, 0, 0], [3, 0, 0], [7, 0, 0], [7, 0, 0]], dtype=np.float32)
    want = [(1 + 9 + 49) / 3, (1 + 4 + 36) / 3, (4 + 9 + 16) / 3, (0 + 16 + 36) / 3, (0 + 16 + 36) / 3]
    got = MR.knn_dist2_bruteforce(pts)
    assert np.allclose(got.numpy(), want, rtol=0, atol=1e-12)
    assert np.allclose(MR.knn_dist2_bruteforce(pts, first_query=3).numpy(), want[3:], rtol=0, atol=1e-12)
    assert np.allclose(MR.knn_dist2_bruteforce(pts, chunk=2).numpy(), want, rtol=0, atol=1e-12)
    # fewer than four points: the neighbours that exist
    assert MR.knn_dist2_bruteforce(pts[:1]).tolist() == [0.0]
    assert MR.knn_dist2_bruteforce(pts[:2]).tolist() == [1.0, 1.0]
    assert MR.knn_dist2_bruteforce(pts[:3]).tolist() == [5.0, 2.5, 6.5]


@pytest.mark.parametrize("stride", [1, 3])
def test_unprojection_inverts_the_projection_convention(stride):
    W, H = 52, 37
    cam = fibonacci_cameras(3, W, H, seed=4)[1]
    depth = MR.depth_sheet(H, W, seed=2, invalid_frac=0.03)
    image = np.random.default_rng(0).uniform(size=(3, H, W)).astype(np.float32)
    xyz, rgb, mask = MR.unproject_reference(cam, image, depth, stride=stride, max_depth=50.0)
    ys, xs = np.nonzero(mask)
    assert len(ys) > 0 and (ys % stride == 0).all() and (xs % stride == 0).all()
    bad = ~np.isfinite(depth) | (depth <= 0.2) | (depth > 50.0)
    assert bad.sum() > 0 and not mask[bad].any()
    px, py, z = MR.project_to_pixels(cam, xyz)
    # float64 chain against the float32 matrices of the camera: 1e-4 pixel is orders above rounding, far below a convention slip
    assert np.abs(px - xs).max() < 1e-4 and np.abs(py - ys).max() < 1e-4
    assert np.abs(z - depth[ys, xs]).max() < 1e-5
    assert (rgb == image[:, ys, xs].T).all()


def test_selection_rule_of_the_restatement():
    d = np.full((2, 3), 2.0, dtype=np.float32)
    A = np.array([[0.1, 0.9, 0.9], [0.9, 0.0, 0.9]], dtype=np.float32)
    z = np.array([[0.0, 1.8, 2.7], [1.8 * 1.06, 0.0, 1.8 * 1.04]], dtype=np.float32)     # surface = z / A: 2.0, 3.0, 2.12, -, 2.08
    m = MR.selection_mask(d, alpha=A, rendered_z=z)
    assert m.tolist() == [[True, False, True], [True, True, False]]
    assert MR.selection_mask(d, alpha=A).tolist() == [[True, False, False], [False, True, False]]
    assert MR.selection_mask(d).all()
    d[0, 0] = 0.0
    assert not MR.selection_mask(d)[0, 0]


def test_no_cpu_fallback():
    from diff_gaussian_rasterization import _C
    from simple_knn._C import distCUDA2, knn_dist2
    from scene_utils import unproject_rgbd
    pts = torch.rand(10, 3)
    with pytest.raises(_C.GsrError, match="no CPU path"):
        distCUDA2(pts)
    with pytest.raises(_C.GsrError, match="no CPU path"):
        knn_dist2(pts, first_query=4)
    with pytest.raises(_C.GsrError, match="no CPU path"):
        GaussianModel(3).create_from_pcd(pts, torch.rand(10, 3))
    cam = fibonacci_cameras(2, 16, 16)[0]
    with pytest.raises(_C.GsrError, match="no CPU path"):
        unproject_rgbd(cam, torch.rand(3, 16, 16), torch.rand(16, 16) + 1)
    m = GaussianModel.from_raw(make_gaussians(20, 1, seed=0))
    with pytest.raises(_C.GsrError, match="no CPU path"):
        m.add_from_rgbd(cam, torch.rand(3, 16, 16), torch.rand(16, 16) + 1)
    assert m.get_xyz.shape[0] == 20
