"""`simple_knn` module the reference imports for its point-cloud initialisation (scene/gaussian_model.py:20
`from simple_knn._C import distCUDA2`, used at :140; submodule absent from the reference tree).  The search runs in the HIP
kernels of csrc/knn.hip, csrc/registration.hip, csrc/normals.hip, csrc/features.hip and csrc/gicp.hip through the C ABI
(gsr_knn_dist2, gsr_knn_k, gsr_nn_search, gsr_estimate_normals, gsr_compute_fpfh, gsr_color_gradient, gsr_estimate_covariances,
gsr_regularize_covariances); there is no CPU path."""
from ._C import distCUDA2, knn_dist2, knn_k, nn_search, estimate_normals, compute_fpfh, estimate_color_gradients



def estimate_covariances(points, radius, max_nn=20, epsilon=1e-3, return_count=False):
    """-> covariances float32 [P,6] (with return_count also count int32 [P]): I - (1 - epsilon) n n^T about the covariance normal n
    of `estimate_normals`' neighbourhood - `scene_utils.estimate_covariances`."""
    from scene_utils.gicp import estimate_covariances as _estimate_covariances
    return _estimate_covariances(points, radius, max_nn, epsilon, return_count)


def regularize_covariances(covariances, epsilon=1e-3):
    """-> covariances float32 [P,6]: every given covariance with its extents replaced by (epsilon, 1, 1) -
    `scene_utils.regularize_covariances`."""
    from scene_utils.gicp import regularize_covariances as _regularize_covariances
    return _regularize_covariances(covariances, epsilon)


__all__ = ["distCUDA2", "knn_dist2", "knn_k", "nn_search", "estimate_normals", "compute_fpfh", "estimate_color_gradients",
           "estimate_covariances", "regularize_covariances"]
