"""ctypes binding of libgsr_hip.so (C ABI in include/gsr.h).

This is the stub a maintainer of the reference would add in place of the pybind11 `_C` extension of the
absent `diff_gaussian_rasterization` submodule (reference gaussian_renderer/__init__.py:14).  There is no
CPU fallback: if the HIP library is missing every call raises.
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (must be imported first: the library shares torch's HIP runtime - same SONAME)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GSR_LIB") or os.path.join(_HERE, "libgsr_hip.so")   # GSR_LIB: A/B a variant build

c_float_p = C.POINTER(C.c_float)


class gsr_settings(C.Structure):
    _fields_ = [
        ("image_height", C.c_int32), ("image_width", C.c_int32),
        ("tanfovx", C.c_float), ("tanfovy", C.c_float),
        ("bg", C.c_void_p), ("scale_modifier", C.c_float),
        ("viewmatrix", C.c_void_p), ("projmatrix", C.c_void_p),
        ("sh_degree", C.c_int32), ("campos", C.c_void_p),
        ("prefiltered", C.c_int32), ("debug", C.c_int32), ("antialiasing", C.c_int32),
    ]


class gsr_gaussians(C.Structure):
    _fields_ = [
        ("P", C.c_int32), ("sh_coeffs", C.c_int32),
        ("means3D", C.c_void_p), ("dc", C.c_void_p), ("shs", C.c_void_p), ("colors_precomp", C.c_void_p),
        ("opacities", C.c_void_p), ("scales", C.c_void_p), ("rotations", C.c_void_p), ("cov3D_precomp", C.c_void_p),
        ("raw_activations", C.c_int32),
    ]


class gsr_grads(C.Structure):
    _fields_ = [
        ("dL_dmeans3D", C.c_void_p), ("dL_dmeans2D", C.c_void_p), ("dL_ddc", C.c_void_p), ("dL_dshs", C.c_void_p),
        ("dL_dcolors", C.c_void_p), ("dL_dopacities", C.c_void_p), ("dL_dscales", C.c_void_p),
        ("dL_drotations", C.c_void_p), ("dL_dcov3D", C.c_void_p),
        ("xyz_gradient_accum", C.c_void_p), ("denom", C.c_void_p), ("max_radii2D", C.c_void_p),
    ]


class gsr_camera_grads(C.Structure):
    _fields_ = [("dL_dviewmatrix", C.c_void_p), ("dL_dprojmatrix", C.c_void_p), ("dL_dcampos", C.c_void_p)]


class gsr_pose_adam(C.Structure):
    # lives in DEVICE memory: eighteen 8-byte words (POSE_ADAM_WORDS; scene_utils.pose keeps it as a float64 tensor whose last word,
    # `step`, is read through an int64 view)
    _fields_ = [("exp_avg", C.c_double * 6), ("exp_avg_sq", C.c_double * 6), ("lr", C.c_double), ("beta1", C.c_double),
                ("beta2", C.c_double), ("eps", C.c_double), ("lr_decay", C.c_double), ("step", C.c_int64)]


POSE_ADAM_WORDS = 18
POSE_ADAM_LR, POSE_ADAM_BETA1, POSE_ADAM_BETA2, POSE_ADAM_EPS, POSE_ADAM_LR_DECAY, POSE_ADAM_STEP = 12, 13, 14, 15, 16, 17


class gsr_exposure_adam(C.Structure):
    # header of the exposure optimizer's DEVICE state: float exp_avg[12 V] and float exp_avg_sq[12 V] follow it
    # (scene_utils.exposure keeps the whole state as one float32 tensor of EXPOSURE_ADAM_HEADER_FLOATS + 24 V words)
    _fields_ = [("step", C.c_int64), ("reserved", C.c_int64)]


EXPOSURE_ADAM_HEADER_FLOATS = 4


class gsr_render_extras(C.Structure):
    # (ctypes zero-fills fields that are not given: three positional values leave n_touched NULL and touched_T_min 0)
    _fields_ = [("depth_kind", C.c_int32), ("out_alpha", C.c_void_p), ("dL_dalpha", C.c_void_p),
                ("n_touched", C.c_void_p), ("touched_T_min", C.c_float)]


DEPTH_KINDS = {"inverse": 0, "z": 1}     # gsr_render_extras.depth_kind: GSR_DEPTH_INVERSE, GSR_DEPTH_Z


class gsr_unproject_params(C.Structure):
    _fields_ = [
        ("image_height", C.c_int32), ("image_width", C.c_int32), ("tanfovx", C.c_float), ("tanfovy", C.c_float),
        ("viewmatrix", C.c_void_p), ("stride", C.c_int32), ("min_depth", C.c_float), ("max_depth", C.c_float),
        ("alpha_below", C.c_float), ("front_margin", C.c_float),
    ]


class gsr_unproject_params_k(C.Structure):
    _fields_ = [("base", gsr_unproject_params), ("ox", C.c_float), ("oy", C.c_float)]


class gsr_fused_adam(C.Structure):
    _fields_ = [
        ("exp_avg", C.c_void_p * 6), ("exp_avg_sq", C.c_void_p * 6), ("lr", C.c_float * 6), ("step", C.c_int64 * 6),
        ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("sparse", C.c_int32),
        ("dynamic", C.c_void_p),
    ]


class gsr_ransac_debug(C.Structure):
    _fields_ = [("samples", C.c_void_p), ("status", C.c_void_p), ("T", C.c_void_p)]


class gsr_pc2_layout(C.Structure):
    # HOST struct: the layout of a sensor_msgs/PointCloud2 byte buffer (datatype = ROS's PointField code, 1 .. 8)
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("point_step", C.c_uint32), ("row_step", C.c_uint32),
                ("is_bigendian", C.c_int32), ("offset", C.c_int32 * 3), ("datatype", C.c_int32 * 3),
                ("color_offset", C.c_int32), ("color_datatype", C.c_int32)]


PC2_CHUNK = 256              # points per workgroup of gsr_pc2_decode (csrc/pointcloud2.hip)
PC2_LDS_BYTES = 256 * 64 + 64      # its staging buffer: a chunk whose byte span exceeds it is read straight from global memory


class gsr_image_layout(C.Structure):
    # HOST struct: the layout of a sensor_msgs/Image byte buffer (encoding = a GSR_IMG_* code)
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("step", C.c_uint32), ("encoding", C.c_int32),
                ("is_bigendian", C.c_int32)]


# GSR_IMG_*: the names of sensor_msgs/image_encodings.h (16UC1 is also the code of a mono16 image read as depth)
IMAGE_ENCODINGS = {"rgb8": 1, "bgr8": 2, "rgba8": 3, "bgra8": 4, "mono8": 5, "rgb16": 6, "bgr16": 7, "rgba16": 8, "bgra16": 9,
                   "mono16": 10, "bayer_rggb8": 11, "bayer_bggr8": 12, "bayer_gbrg8": 13, "bayer_grbg8": 14, "bayer_rggb16": 15,
                   "bayer_bggr16": 16, "bayer_gbrg16": 17, "bayer_grbg16": 18, "16UC1": 19, "32FC1": 20}
IMG_TILE_W = 256             # GSR_IMG_TILE_W: pixels of one row per workgroup of gsr_image_decode (csrc/image.hip)
IMG_TILE_H = 1               # rows per workgroup: rows are not tiled (Bayer stages the rows above and below as halo)
DEPTH_REGISTER_CAP = 8       # columns / rows of a footprint of gsr_depth_register before it is cut


class gsr_cloud_camera(C.Structure):
    # HOST struct: the camera a cloud is projected into (csrc/cloud_image.hip); w2c = rows 0 .. 2 of cloud frame -> camera
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("K", C.c_float * 4), ("w2c", C.c_double * 12),
                ("z_near", C.c_float), ("z_far", C.c_float), ("footprint", C.c_int32), ("occlusion_scale", C.c_float)]


CLOUD_MAX_FOOTPRINT = 4      # GSR_CLOUD_MAX_FOOTPRINT
DENSIFY_MAX_RADIUS = 8       # GSR_DENSIFY_MAX_RADIUS
DENSIFY_TILE_W = 32          # pixels per workgroup of gsr_depth_densify: 32 x 8
DENSIFY_TILE_H = 8
SCAN_CONTEXT_MAX_RINGS = 40       # GSR_SCAN_CONTEXT_MAX_RINGS
SCAN_CONTEXT_MAX_SECTORS = 120    # GSR_SCAN_CONTEXT_MAX_SECTORS
SCAN_CONTEXT_MAX_ORIGINS = 16     # GSR_SCAN_CONTEXT_MAX_ORIGINS

class gsr_tsdf_volume(C.Structure):
    # HOST struct: the lattice of a TSDF volume (csrc/tsdf.hip)
    _fields_ = [("origin", C.c_double * 3), ("voxel_size", C.c_double), ("sdf_trunc", C.c_float), ("depth_trunc", C.c_float),
                ("max_weight", C.c_float), ("reserved", C.c_float)]


class gsr_tsdf_frame(C.Structure):
    # HOST struct: one depth frame; w2c = the first three rows of the world-to-camera matrix, row-major float64
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("K", C.c_float * 4), ("w2c", C.c_double * 12),
                ("depth", C.c_void_p), ("mask", C.c_void_p), ("color", C.c_void_p)]


TSDF_BLOCK = 8               # GSR_TSDF_BLOCK: voxels per block edge
TSDF_TOUCH_SLOTS = 27        # GSR_TSDF_TOUCH_SLOTS
TSDF_MAX_BLOCKS = 1 << 19    # GSR_TSDF_MAX_BLOCKS
TSDF_NO_KEY = (1 << 63) - 1  # GSR_TSDF_NO_KEY

ODOMETRY_TILE_W = 32         # GSR_ODO_TILE_W x GSR_ODO_TILE_H: pixels per workgroup of gsr_odometry_prepare (csrc/odometry.hip)
ODOMETRY_TILE_H = 8

FPFH_WIDTH = 33              # GSR_FPFH_WIDTH
FEATURE_NN_TILE = 128        # GSR_FEATURE_NN_TILE
RANSAC_N_MAX = 8             # GSR_RANSAC_N_MAX
RANSAC_MAX_TRIALS = 1 << 20  # GSR_RANSAC_MAX_TRIALS
RANSAC_BEST_WORDS = 20       # sizeof(gsr_ransac_best) / 8: count, sum_d2, trial, T[16], trials_checked

_EXTRAS = C.POINTER(gsr_render_extras)
_SCENE = [C.POINTER(gsr_settings), C.POINTER(gsr_gaussians)]
# shared argument prefixes of the rasterizer's entry points (include/gsr.h), each named by what follows (settings, Gaussians):
# geometry state + bytes, radii
_PREPARE = _SCENE + [C.c_void_p, C.c_size_t, C.c_void_p]
# geometry state, binning state + bytes, num_rendered, image state + bytes, color, invdepth, for_backward
_RENDER = _SCENE + [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int32]
# geometry state + bytes, radii, binning state + bytes, capacity, image state + bytes, color, invdepth, for_backward, split,
# event, status, tile_local, stream, count
_ASYNC = _PREPARE + [C.c_void_p, C.c_size_t, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                     C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_int64)]
# radii, geometry / binning / image state, num_rendered, dL_dcolor, dL_dinvdepth, scratch + bytes
_BACKWARD = _SCENE + [C.c_void_p] * 4 + [C.c_int64] + [C.c_void_p] * 3 + [C.c_size_t]
_CAMERA = [C.POINTER(gsr_camera_grads), C.c_void_p, C.c_size_t]      # camera gradients, reduction scratch + bytes

EXPORTS = {
    # name: (restype, argtypes)
    "gsr_abi_version": (C.c_int, []),
    "gsr_last_error": (C.c_char_p, []),
    "gsr_geometry_state_bytes": (C.c_size_t, [C.c_int32]),
    "gsr_image_state_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "gsr_binning_state_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int64]),
    "gsr_backward_scratch_bytes": (C.c_size_t, [C.c_int32, C.c_int64]),
    "gsr_forward_prepare": (C.c_int64, _PREPARE + [C.c_void_p]),
    "gsr_forward_prepare_geometry": (C.c_int64, _PREPARE + [C.c_void_p]),
    "gsr_forward_shade": (C.c_int, _SCENE + [C.c_void_p, C.c_void_p]),
    "gsr_forward_render": (C.c_int, _RENDER + [C.c_void_p]),
    "gsr_forward_render_shade": (C.c_int, _RENDER + [C.c_void_p, C.c_void_p]),                  # event, stream
    "gsr_forward_async": (C.c_int, _ASYNC),
    "gsr_forward_async_culled": (C.c_int, _ASYNC + [C.c_void_p, C.c_int32]),                    # tile_cull, apply
    "gsr_forward_rerender": (C.c_int, _RENDER + [C.c_int32, C.c_void_p, C.c_void_p]),           # tile_local, status, stream
    "gsr_backward": (C.c_int, _BACKWARD + [C.POINTER(gsr_grads), C.c_void_p]),
    "gsr_camera_grad_scratch_bytes": (C.c_size_t, [C.c_int32]),
    "gsr_backward_camera": (C.c_int, _BACKWARD + [C.POINTER(gsr_grads)] + _CAMERA + [C.c_void_p]),
    "gsr_backward_camera_only": (C.c_int, _BACKWARD + _CAMERA + [C.c_void_p]),
    "gsr_backward_adam": (C.c_int, _BACKWARD + [C.POINTER(gsr_grads), C.POINTER(gsr_fused_adam), C.c_void_p]),
    "gsr_adam_step_culled_rows": (C.c_int, [C.POINTER(gsr_gaussians), C.c_void_p, C.c_int64, C.POINTER(gsr_fused_adam),
                                            C.c_void_p]),
    "gsr_mark_visible": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsr_debug_geometry_views": (C.c_int, [C.c_void_p, C.c_int32] + [C.POINTER(C.c_void_p)] * 7),
    "gsr_debug_wave_reduce": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsr_debug_wave_reduce_pk": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsr_debug_mx_reduce": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsr_debug_binning_views": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_void_p),
                                          C.POINTER(C.c_void_p)]),
    "gsr_debug_slot_views": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_void_p)]),
    "gsr_debug_count_pairs": (C.c_int, [C.POINTER(gsr_settings), C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                        C.c_void_p]),
    "gsr_debug_radix_tmp_bytes": (C.c_size_t, [C.c_int64]),
    "gsr_debug_radix_sort": (C.c_int, [C.c_void_p] * 6 + [C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsr_debug_scan_tmp_bytes": (C.c_size_t, [C.c_int64]),
    "gsr_debug_scan_u32": (C.c_int, [C.c_void_p] * 3 + [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "gsr_debug_tile_sort": (C.c_int, [C.c_void_p] * 6 + [C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 4),
    "gsr_debug_tile_depth_sort": (C.c_int, [C.c_int32, C.c_int32] + [C.c_void_p] * 10),
    "gsr_debug_image_views": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p),
                                        C.POINTER(C.c_void_p)]),
    "gsr_debug_set_flags_min_r": (C.c_int64, [C.c_int64]),
    "gsr_debug_walk_views": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                       C.POINTER(C.c_void_p)]),
    "gsr_fused_ssim_forward": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float] + [C.c_void_p] * 7),
    "gsr_fused_ssim_backward": (C.c_int, [C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 8),
    "gsr_fused_loss_blocks": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "gsr_adam_set_dynamic": (C.c_int, [C.POINTER(gsr_fused_adam), C.c_void_p, C.c_void_p]),
    "gsr_l1_mean_blocks": (C.c_int32, []),
    "gsr_l1_mean_forward": (C.c_int, [C.c_int64, C.c_float] + [C.c_void_p] * 6),
    "gsr_l1_mean_backward": (C.c_int, [C.c_int64, C.c_float] + [C.c_void_p] * 6),
    "gsr_fused_l1_ssim_forward": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float] +
                                  [C.c_void_p] * 8),
    "gsr_fused_l1_ssim_backward": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_float] + [C.c_void_p] * 8),
    "gsr_adam_step": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_void_p]),
    "gsr_sparse_adam_step": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_int64, C.c_void_p, C.c_double, C.c_double, C.c_double,
                                       C.c_void_p]),
    "gsr_densification_stats": (C.c_int, [C.c_int64] + [C.c_void_p] * 6),
    "gsr_gaussian_activations_forward": (C.c_int, [C.c_int32] + [C.c_void_p] * 7),
    "gsr_gaussian_activations_backward": (C.c_int, [C.c_int32] + [C.c_void_p] * 10),
    "gsr_densify_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "gsr_densify_plan": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float,
                                   C.c_float, C.c_float, C.c_int32, C.c_void_p, C.c_size_t, C.POINTER(C.c_int64),
                                   C.c_void_p]),
    "gsr_densify_apply": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int64,
                                    C.c_int64, C.c_int64, C.c_uint32, C.c_void_p, C.c_void_p]),
    "gsr_sh_rank1_expand": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    "gsr_sh_rank1_adam": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p,
                                    C.c_void_p, C.POINTER(gsr_fused_adam), C.c_void_p]),
    "gsr_knn_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "gsr_knn_dist2": (C.c_int, [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    # P, points, k, dist2_out, mean_dist_out, workspace + bytes, stream
    "gsr_knn_k_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "gsr_knn_k": (C.c_int, [C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    # P, points, colors, voxel_size, origin (host), out_points, out_colors, out_npts, capacity, count_dev, workspace + bytes, stream
    "gsr_voxel_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "gsr_voxel_down_sample": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_float, c_float_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    # P, points, nb_neighbors, std_ratio, keep, mean_dist, stats_dev, workspace + bytes, stream
    "gsr_outlier_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "gsr_statistical_outliers": (C.c_int, [C.c_int64, C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_size_t, C.c_void_p]),
    # Pt, target, index + bytes, stream
    "gsr_nn_index_bytes": (C.c_size_t, [C.c_int64]),
    "gsr_nn_index_build": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    # Pt, index, Ps, source, T_dev, max_dist2, order, idx_out, dist2_out, stream
    "gsr_nn_search": (C.c_int, [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p]),
    # Pt, index, Ps, source, T_dev, order_out, workspace + bytes, stream
    "gsr_nn_order_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "gsr_nn_query_order": (C.c_int, [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_size_t, C.c_void_p]),
    # P, points, T_dev, out, stream
    "gsr_transform_points": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # Ps, source, Pt, target, idx, T_dev, stats_dev, workspace + bytes, stream
    "gsr_icp_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "gsr_icp_update": (C.c_int, [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_size_t, C.c_void_p]),
    # Ps, source, Pt, target, target_normals, idx, T_dev, stats_dev, workspace + bytes, stream
    "gsr_icp_update_plane": (C.c_int, [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_size_t, C.c_void_p]),
    # P, points, radius, max_nn, viewpoint (host), normals, count_out, eigenvalues_out, workspace + bytes, stream
    "gsr_normals_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "gsr_estimate_normals": (C.c_int, [C.c_int64, C.c_void_p, C.c_float, C.c_int32, c_float_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_size_t, C.c_void_p]),
    # P, points, colors, normals, radius, max_nn, gradient, count_out, status_out, workspace + bytes, stream
    "gsr_color_gradient_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "gsr_color_gradient": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    # Ps, source, source_colors, Pt, target, target_normals, target_colors, target_gradient, idx, lambda_geometric, T_dev,
    # stats_dev, workspace + bytes, stream
    "gsr_icp_colored_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "gsr_icp_update_colored": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                         C.c_void_p]),
    # P, points, radius, max_nn, epsilon, cov_out, count_out, workspace + bytes, stream
    "gsr_covariance_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "gsr_estimate_covariances": (C.c_int, [C.c_int64, C.c_void_p, C.c_float, C.c_int32, C.c_double, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_size_t, C.c_void_p]),
    # P, cov_in, epsilon, cov_out, stream
    "gsr_regularize_covariances": (C.c_int, [C.c_int64, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]),
    # Ps, source, source_cov, Pt, target, target_cov, idx, T_dev, stats_dev, workspace + bytes, stream
    "gsr_icp_generalized_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "gsr_icp_update_generalized": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    # w, h, color, depth, mask, depth_min, depth_max, intensity_out, depth_out, grad_out, stream
    "gsr_odometry_prepare": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    # w, h, K (host float64[4]), src_intensity, src_depth, tgt_intensity, tgt_depth, tgt_grad, lambda_geometric, depth_diff_max,
    # apply, T_dev, stats_dev, workspace + bytes, stream
    "gsr_odometry_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "gsr_odometry_update": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_double)] + [C.c_void_p] * 5 +
                            [C.c_double, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    # Pt, target, Ps, idx, info_out, stats_dev, workspace + bytes, stream
    "gsr_information_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "gsr_registration_information": (C.c_int, [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_size_t, C.c_void_p]),
    # N, E, edges (host int32 [E,2]), fixed (host uint8 [N]), host scratch (topology bytes), topology + bytes, stream
    "gsr_posegraph_topology_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "gsr_posegraph_topology": (C.c_int, [C.c_int64, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.c_void_p, C.c_void_p,
                                         C.c_size_t, C.c_void_p]),
    "gsr_posegraph_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    # N, E, topology, poses, edge_T, edge_info, edge_uncertain, mu, edge_out, node_out, scalars_out, stream
    "gsr_posegraph_linearize": (C.c_int, [C.c_int64, C.c_int64] + [C.c_void_p] * 5 + [C.c_double] + [C.c_void_p] * 4),
    # N, E, topology, edge_rec, node_rec, lambda, cg_rtol, cg_max_iteration, delta_out, stats_dev, workspace + bytes, stream
    "gsr_posegraph_solve": (C.c_int, [C.c_int64, C.c_int64] + [C.c_void_p] * 3 + [C.c_double, C.c_double, C.c_int32, C.c_void_p,
                                                                                 C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    # N, E, topology, poses, edge_T, edge_info, edge_uncertain, mu, max_iteration, min_relative_increment,
    # min_relative_residual_increment, cg_rtol, cg_max_iteration, edge_w_out, edge_r_out, stats_dev, workspace + bytes, stream
    "gsr_posegraph_optimize": (C.c_int, [C.c_int64, C.c_int64] + [C.c_void_p] * 5 + [C.c_double, C.c_int32, C.c_double, C.c_double,
                                                                                    C.c_double, C.c_int32] + [C.c_void_p] * 4 +
                               [C.c_size_t, C.c_void_p]),
    # P, points, normals, radius, max_nn, fpfh, spfh_counts, count, workspace + bytes, stream
    "gsr_fpfh_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "gsr_compute_fpfh": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_float, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_size_t, C.c_void_p]),
    # Nq, query, Nt, target, width, idx_out, dist2_out, workspace + bytes, stream
    "gsr_feature_nn_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "gsr_feature_nn_tiles_per_split": (C.c_int32, [C.c_int64, C.c_int64]),
    "gsr_feature_nn": (C.c_int, [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_size_t, C.c_void_p]),
    # Ps, source, Pt, target, M, pairs, max_distance, ransac_n, edge_length_threshold, seed, t0, n, best, workspace + bytes,
    # debug (host struct), stream
    "gsr_ransac_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "gsr_ransac_feature_matching": (C.c_int, [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_float,
                                              C.c_int32, C.c_float, C.c_uint64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                              C.c_size_t, C.POINTER(gsr_ransac_debug), C.c_void_p]),
    # w, h, image, channels, u8_out, box_out, stream
    "gsr_orb_prepare": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsr_orb_cells": (C.c_int64, [C.c_int32, C.c_int32]),
    # w, h, u8, mask, threshold, per_cell, slots, stream
    "gsr_orb_detect": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    # w, h, u8, box, M, keypoints, angle_bin, moments, descriptors, stream
    "gsr_orb_describe": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 5),
    "gsr_orb_pattern": (C.c_int, [C.c_void_p]),      # out: HOST int8 [30720]
    # Q, query, N, db, idx_out, best_out, second_out, stream
    "gsr_hamming_match": (C.c_int, [C.c_int64, C.c_void_p, C.c_int64] + [C.c_void_p] * 5),
    # Q, query, N, db, K, segments, max_distance, ratio, votes, stream
    "gsr_hamming_vote": (C.c_int, [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_float,
                                   C.c_void_p, C.c_void_p]),
    # N, points, frame (host [12] or NULL), B, origins (host [B,3] or NULL), rings, sectors, max_range, height_offset,
    # descriptors, norms, stream
    "gsr_scan_context": (C.c_int, [C.c_int64, C.c_void_p, c_float_p, C.c_int32, c_float_p, C.c_int32, C.c_int32, C.c_float,
                                   C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    # rings, sectors, B, query, query_norms, K, db, db_norms, dist, shift, variant, stream
    "gsr_scan_context_distance": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64] +
                                  [C.c_void_p] * 6),
    # layout (host), data + bytes, T_dev, min_y, max_range2, skip_nans, out_points, out_colors, out_index, cap, count_dev,
    # workspace + bytes, stream
    "gsr_pc2_decode_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "gsr_pc2_decode": (C.c_int, [C.POINTER(gsr_pc2_layout), C.c_void_p, C.c_size_t, C.c_void_p, C.c_double, C.c_double, C.c_int32,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    # P, points, colors, out, stream
    "gsr_pc2_encode": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsr_debug_pc2_force_direct": (C.c_int32, [C.c_int32]),
    # layout (host), data + bytes, depth_scale, depth_lo, depth_hi, out, stream
    "gsr_image_decode": (C.c_int, [C.POINTER(gsr_image_layout), C.c_void_p, C.c_size_t, C.c_float, C.c_float, C.c_float, C.c_void_p,
                                   C.c_void_p]),
    # W, H, image, out_bytes, stream
    "gsr_image_encode_rgb8": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    # Wd, Hd, depth, Kd[4] (host), Kc[4] (host), T_cd[12] (host float64), Wc, Hc, out, status_dev, workspace + bytes, stream
    "gsr_depth_register_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "gsr_depth_register": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                     C.POINTER(C.c_double), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                     C.c_void_p]),
    "gsr_cloud_project_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    # camera (host), N, points, image, mask, depth, index, pixel, z, visible, colors, count_dev, workspace + bytes, stream
    "gsr_cloud_project": (C.c_int, [C.POINTER(gsr_cloud_camera), C.c_int64] + [C.c_void_p] * 11 + [C.c_size_t, C.c_void_p]),
    # W, H, depth, radius, band_scale, min_neighbors, dense, valid, stream
    "gsr_depth_densify": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_float, C.c_int32, C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    "gsr_unproject_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "gsr_unproject_rgbd":(C.c_int, [C.POINTER(gsr_unproject_params)] + [C.c_void_p] * 6 + [C.c_int64, C.c_void_p, C.c_void_p,
                                                                                           C.c_size_t, C.c_void_p]),
    "gsr_unproject_rgbd_k": (C.c_int, [C.POINTER(gsr_unproject_params_k)] + [C.c_void_p] * 6 + [C.c_int64, C.c_void_p, C.c_void_p,
                                                                                               C.c_size_t, C.c_void_p]),
    # src_w, src_h, src_color, src_depth, src_K (host), dist (host), w, h, K (host), color, depth, mask, stream
    "gsr_frame_undistort": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, c_float_p, c_float_p, C.c_int32, C.c_int32,
                                      c_float_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # w, h, levels, color, depth, mask, depth_band, color_out / depth_out / mask_out (host arrays of device pointers), stream
    "gsr_frame_pyramid": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float] +
                          [C.POINTER(C.c_void_p)] * 3 + [C.c_void_p]),
    "gsr_pose_forward": (C.c_int, [C.c_void_p] * 7),
    "gsr_pose_backward": (C.c_int, [C.c_void_p] * 9),
    "gsr_exposure_blocks": (C.c_int32, []),
    "gsr_exposure_forward": (C.c_int, [C.c_int64] + [C.c_void_p] * 5),
    # n, image, exposure, mask, dL_dout, dL_dimage, partials, dL_dexposure, exposures, views, row, adam, lr, beta1, beta2, eps, stream
    "gsr_exposure_backward": (C.c_int, [C.c_int64] + [C.c_void_p] * 8 + [C.c_int32, C.c_int32, C.c_void_p] + [C.c_double] * 4 +
                              [C.c_void_p]),
    "gsr_transform_workspace_bytes": (C.c_size_t, [C.c_int32]),
    # P, anchor, K, transforms, workspace + bytes, xyz, rotation, scaling, features_rest, sh_coeffs_rest, moments8 (host), stream
    "gsr_transform_gaussians": (C.c_int, [C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_void_p] * 4 +
                                [C.c_int32, C.POINTER(C.c_void_p), C.c_void_p]),
    # volume (host), frame (host), keys_out, stream
    "gsr_tsdf_touch": (C.c_int, [C.POINTER(gsr_tsdf_volume), C.POINTER(gsr_tsdf_frame), C.c_void_p, C.c_void_p]),
    # volume, frame, n_blocks, keys, rows, n_rows, tsdf, weight, color, stream
    "gsr_tsdf_integrate": (C.c_int, [C.POINTER(gsr_tsdf_volume), C.POINTER(gsr_tsdf_frame), C.c_int64, C.c_void_p, C.c_void_p,
                                     C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsr_tsdf_extract_workspace_bytes": (C.c_size_t, [C.c_int64]),
    # volume, B, keys_sorted, row_of_sorted, tsdf, weight, color, min_weight, capacity, points, normals, colors, count_dev,
    # workspace + bytes, stream
    "gsr_tsdf_extract_points": (C.c_int, [C.POINTER(gsr_tsdf_volume), C.c_int64] + [C.c_void_p] * 5 + [C.c_float, C.c_int64] +
                                [C.c_void_p] * 5 + [C.c_size_t, C.c_void_p]),
    # volume, B, keys_sorted, row_of_sorted, tsdf, weight, color, min_weight, capacity, positions, colors, count_dev,
    # workspace + bytes, stream
    "gsr_tsdf_extract_triangles": (C.c_int, [C.POINTER(gsr_tsdf_volume), C.c_int64] + [C.c_void_p] * 5 + [C.c_float, C.c_int64] +
                                   [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p]),
    "gsr_profile_enable": (None, [C.c_int32]),
    "gsr_profile_reset": (None, []),
    "gsr_profile_read": (C.c_int32, [C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int32]),
}

# the *_ex forms: the same arguments plus a gsr_render_extras* (NULL = the form without _ex)
for _name in ("gsr_forward_prepare", "gsr_forward_prepare_geometry", "gsr_forward_render", "gsr_forward_render_shade",
              "gsr_forward_async", "gsr_forward_async_culled", "gsr_forward_rerender", "gsr_backward", "gsr_backward_camera",
              "gsr_backward_camera_only", "gsr_backward_adam"):
    EXPORTS[_name + "_ex"] = (EXPORTS[_name][0], EXPORTS[_name][1] + [_EXTRAS])

ADAM_DYNAMIC_FLOATS = 18     # GSR_ADAM_DYNAMIC_FLOATS
ABI_VERSION = 7      # GSR_ABI_VERSION of include/gsr.h
_lib = None


class GsrError(RuntimeError):
    pass


def lib():
    """Loads libgsr_hip.so once.  Raises (never falls back) when the library is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise GsrError(
                f"{LIB_PATH} not found: the HIP rasterizer is not built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C gaussian-splatting-slam_amd/csrc`). "
                "There is no CPU fallback.")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in EXPORTS.items():
            f = getattr(l, name)         # AttributeError if a declared symbol is not exported
            f.restype = res
            f.argtypes = args
        if l.gsr_abi_version() != ABI_VERSION:
            raise GsrError(f"libgsr_hip.so ABI {l.gsr_abi_version()} != {ABI_VERSION}: rebuild (make -C csrc)")
        _lib = l
    return _lib


def last_error() -> str:
    return lib().gsr_last_error().decode("utf-8", "replace")


def check(rc: int):
    if rc < 0:
        raise GsrError(f"libgsr_hip error {rc}: {last_error()}")
    return rc


def ptr(t):
    """device pointer of a tensor, or None"""
    return None if t is None else C.c_void_p(t.data_ptr())


def profile_read():
    l = lib()
    n = l.gsr_profile_read(None, None, None, 0)
    names = (C.c_char_p * n)()
    ms = (C.c_double * n)()
    calls = (C.c_int64 * n)()
    n = l.gsr_profile_read(names, ms, calls, n)
    return {names[i].decode(): (ms[i], calls[i]) for i in range(n)}


def raw_stream(device_index=None):
    """hipStream_t of torch's current stream as an int (no Stream object is built: this sits on every call's path)."""
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device() if device_index is None else device_index)


def _stream():
    return C.c_void_p(raw_stream())


class on_device:
    """`with torch.cuda.device(dev)` that does nothing at all when `dev` already is the current device (the usual case: one
    process per GPU) - the stock context manager costs ~10 us per use, several uses per training step."""
    __slots__ = ("idx", "prev")

    def __init__(self, dev):
        self.idx = dev.index if isinstance(dev, torch.device) else dev
        self.prev = None

    def __enter__(self):
        if self.idx is not None:
            cur = torch.cuda.current_device()
            if cur != self.idx:
                self.prev = cur
                torch.cuda.set_device(self.idx)
        return self

    def __exit__(self, *exc):
        if self.prev is not None:
            torch.cuda.set_device(self.prev)
        return False


# ---- the two functions reference utils/loss_utils.py:16-19 imports from `diff_gaussian_rasterization._C` ----
def _ssim_forward(C1, C2, img1, img2, want_partials):
    if not img1.is_cuda:
        raise GsrError("fusedssim needs tensors on the HIP device (no CPU path)")
    img1 = img1.detach().float().contiguous()
    img2 = img2.detach().float().contiguous()
    H, W = int(img1.shape[-2]), int(img1.shape[-1])
    planes = img1.numel() // (H * W) if H * W else 0
    out = torch.empty_like(img1)
    parts = [torch.empty_like(img1) for _ in range(3)] if want_partials else [None, None, None]
    with torch.cuda.device(img1.device):
        check(lib().gsr_fused_ssim_forward(planes, H, W, float(C1), float(C2), ptr(img1), ptr(img2), ptr(out),
                                           ptr(parts[0]), ptr(parts[1]), ptr(parts[2]), _stream()))
    return out, parts, img1, img2


def fusedssim(C1, C2, img1, img2):
    """-> ssim_map, same shape as img1 (reference utils/loss_utils.py:27)."""
    return _ssim_forward(C1, C2, img1, img2, False)[0]


def fusedssim_backward(C1, C2, img1, img2, dL_dmap, partials=None):
    """-> dL/dimg1 (reference utils/loss_utils.py:37).  `partials` (from a forward that kept them) avoids recomputation."""
    if partials is None:
        _, partials, img1, img2 = _ssim_forward(C1, C2, img1, img2, True)
    else:
        img1 = img1.detach().float().contiguous()
        img2 = img2.detach().float().contiguous()
    H, W = int(img1.shape[-2]), int(img1.shape[-1])
    planes = img1.numel() // (H * W) if H * W else 0
    g = dL_dmap.detach().float().expand_as(img1).contiguous()
    out = torch.empty_like(img1)
    with torch.cuda.device(img1.device):
        check(lib().gsr_fused_ssim_backward(planes, H, W, ptr(img1), ptr(img2), ptr(g), ptr(partials[0]),
                                            ptr(partials[1]), ptr(partials[2]), ptr(out), _stream()))
    return out


# ---- the low-level call forms of the absent module's `_C` (SURVEY.md 8b "Native surface"; nothing in the reference calls them
# directly, they are kept so code written against the published extension keeps working) ----
def _forward_on_own_buffers(s, g, P, W, H, dev):
    """The blocking forward on buffers allocated here: gsr_forward_prepare (reads num_rendered back), a binning state of exactly
    that size, gsr_forward_render.  -> (num_rendered, color, radii, geom, binning, img, invdepth)"""
    l = lib()
    color = torch.empty(3, H, W, dtype=torch.float32, device=dev)
    invdepth = torch.empty(1, H, W, dtype=torch.float32, device=dev)
    radii = torch.zeros(P, dtype=torch.int32, device=dev)
    geom = torch.empty(l.gsr_geometry_state_bytes(P), dtype=torch.uint8, device=dev)
    img = torch.empty(l.gsr_image_state_bytes(W, H), dtype=torch.uint8, device=dev)
    R = check(l.gsr_forward_prepare(C.byref(s), C.byref(g), ptr(geom), geom.numel(), ptr(radii), _stream()))
    binning = torch.empty(l.gsr_binning_state_bytes(P, W, H, R), dtype=torch.uint8, device=dev)
    check(l.gsr_forward_render(C.byref(s), C.byref(g), ptr(geom), ptr(binning), binning.numel(), R, ptr(img),
                               img.numel(), ptr(color), ptr(invdepth), 1, _stream()))
    return R, color, radii, geom, binning, img, invdepth


def rasterize_gaussians(bg, means3D, colors_precomp, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
                        projmatrix, tanfovx, tanfovy, image_height, image_width, sh, degree, campos, prefiltered,
                        antialiasing, debug):
    """-> (num_rendered, color[3,H,W], radii[P], geomBuffer, binningBuffer, imgBuffer, invdepth[1,H,W]); empty tensors stand
    for absent inputs, as in the published extension."""
    import diff_gaussian_rasterization as dgr

    def opt(t):
        return None if (t is None or t.numel() == 0) else t.detach().float().contiguous()
    rs = dgr.GaussianRasterizationSettings(int(image_height), int(image_width), float(tanfovx), float(tanfovy), bg,
                                           float(scale_modifier), viewmatrix, projmatrix, int(degree), campos,
                                           bool(prefiltered), bool(debug), bool(antialiasing))
    dev = means3D.device
    P, H, W = int(means3D.shape[0]), int(image_height), int(image_width)
    m3, col, op, sc, ro, cov, shs = opt(means3D), opt(colors_precomp), opt(opacity), opt(scales), opt(rotations), \
        opt(cov3D_precomp), opt(sh)
    with torch.cuda.device(dev):
        s, keep = dgr._settings_struct(rs, dev)
        g = dgr._gauss_struct(P, m3, None, shs, col, op, sc, ro, cov)
        return _forward_on_own_buffers(s, g, P, W, H, dev)


def rasterize_gaussians_backward(bg, means3D, radii, colors_precomp, opacities, scales, rotations, scale_modifier,
                                 cov3D_precomp, viewmatrix, projmatrix, tanfovx, tanfovy, dL_dcolor, dL_dinvdepth, sh, degree,
                                 campos, geomBuffer, num_rendered, binningBuffer, imgBuffer, antialiasing, debug):
    """-> (dL_dmeans2D[P,3], dL_dcolors[P,3], dL_dopacity[P,1], dL_dmeans3D[P,3], dL_dcov3D[P,6], dL_dsh[P,M,3],
    dL_dscales[P,3], dL_drotations[P,4]) - the published order; absent inputs give empty gradient tensors."""
    import diff_gaussian_rasterization as dgr

    def opt(t):
        return None if (t is None or t.numel() == 0) else t.detach().float().contiguous()
    dev = means3D.device
    P = int(means3D.shape[0])
    H, W = int(dL_dcolor.shape[-2]), int(dL_dcolor.shape[-1])
    rs = dgr.GaussianRasterizationSettings(H, W, float(tanfovx), float(tanfovy), bg, float(scale_modifier), viewmatrix,
                                           projmatrix, int(degree), campos, False, bool(debug), bool(antialiasing))
    m3, col, op, sc, ro, cov, shs = opt(means3D), opt(colors_precomp), opt(opacities), opt(scales), opt(rotations), \
        opt(cov3D_precomp), opt(sh)
    l = lib()

    def like(t, *shape):
        return torch.empty(*shape, dtype=torch.float32, device=dev) if t is not None else None
    with torch.cuda.device(dev):
        s, keep = dgr._settings_struct(rs, dev)
        g = dgr._gauss_struct(P, m3, None, shs, col, op, sc, ro, cov)
        d_m3 = torch.empty(P, 3, dtype=torch.float32, device=dev)
        d_m2 = torch.empty(P, 3, dtype=torch.float32, device=dev)
        d_op = torch.empty(P, 1, dtype=torch.float32, device=dev)
        d_sh, d_col = like(shs, *(shs.shape if shs is not None else ())), like(col, P, 3)
        d_sc, d_ro, d_cov = like(sc, P, 3), like(ro, P, 4), like(cov, P, 6)
        scratch = torch.empty(l.gsr_backward_scratch_bytes(P, int(num_rendered)), dtype=torch.uint8, device=dev)
        gr = gsr_grads(*[None if t is None else t.data_ptr() for t in (d_m3, d_m2, None, d_sh, d_col, d_op, d_sc, d_ro, d_cov)])
        check(l.gsr_backward(C.byref(s), C.byref(g), ptr(radii), ptr(geomBuffer), ptr(binningBuffer), ptr(imgBuffer),
                             int(num_rendered), ptr(opt(dL_dcolor)), ptr(opt(dL_dinvdepth)), ptr(scratch), scratch.numel(),
                             C.byref(gr), _stream()))
    e = torch.empty(0, device=dev)
    return (d_m2, d_col if d_col is not None else e, d_op, d_m3, d_cov if d_cov is not None else e,
            d_sh if d_sh is not None else e, d_sc if d_sc is not None else e, d_ro if d_ro is not None else e)


def mark_visible(positions, viewmatrix, projmatrix=None):
    """bool[P] (published `_C.mark_visible(positions, viewmatrix, projmatrix)`; the projection matrix is not needed for the
    near-plane test)."""
    positions = positions.detach().float().contiguous()
    P = int(positions.shape[0])
    present = torch.zeros(P, dtype=torch.uint8, device=positions.device)
    if P:
        vm = viewmatrix.detach().float().contiguous().to(positions.device)
        with torch.cuda.device(positions.device):
            check(lib().gsr_mark_visible(P, ptr(positions), ptr(vm), ptr(present), _stream()))
    return present.bool()
