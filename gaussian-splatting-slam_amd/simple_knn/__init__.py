"""`simple_knn` module the reference imports for its point-cloud initialisation (scene/gaussian_model.py:20
`from simple_knn._C import distCUDA2`, used at :140; submodule absent from the reference tree).  The search runs in the HIP
kernels of csrc/knn.hip, csrc/registration.hip, csrc/normals.hip and csrc/features.hip through the C ABI (gsr_knn_dist2, gsr_knn_k,
gsr_nn_search, gsr_estimate_normals, gsr_compute_fpfh, gsr_color_gradient); there is no CPU path."""
from ._C import distCUDA2, knn_dist2, knn_k, nn_search, estimate_normals, compute_fpfh, estimate_color_gradients

__all__ = ["distCUDA2", "knn_dist2", "knn_k", "nn_search", "estimate_normals", "compute_fpfh", "estimate_color_gradients"]
