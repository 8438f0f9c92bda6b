/*
 * gsr.h - C ABI of the MI355X-native differentiable Gaussian rasterizer (libgsr_hip.so).
 *
 * This is the drop-in boundary for the hot path named by BASELINE.json:north_star.  It replaces the
 * native half of the third-party module the reference imports at
 *     /root/reference/gaussian_renderer/__init__.py:14
 *         from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
 * i.e. what `_C.rasterize_gaussians`, `_C.rasterize_gaussians_backward` and `_C.mark_visible` of
 * graphdeco-inria/diff-gaussian-rasterization@9c5c2028 (pin: reference results.md:2, .gitmodules:4-6) do for
 * the call at gaussian_renderer/__init__.py:90-109.  The source of that module is NOT in the reference tree
 * (SURVEY.md 0.1), so entry points cite the reference call site / contract they serve.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless marked "host";
 *   - all tensors are contiguous; fp32 unless stated; matrices are the reference's row-major 4x4 tensors
 *     (world_view_transform = W2C^T, full_proj_transform = (P.W2C)^T; reference scene/cameras.py:69-71);
 *   - `stream` is a hipStream_t passed as void*; every call enqueues on it and is re-entrant per stream;
 *   - the library never allocates device memory on the hot path: the caller owns three opaque state
 *     buffers (geometry / binning / image) that carry forward -> backward, sized by the gsr_*_bytes()
 *     queries (the reference's rasterizer keeps the same three buffers as torch uint8 tensors in its
 *     autograd ctx - SURVEY.md 8b "Ownership");
 *   - return value < 0 is an error code; gsr_last_error() gives the message (thread-local).
 */
#ifndef GSR_H_
#define GSR_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 7: gsr_debug_mx_reduce (the compositing backward's sums on the matrix pipe: opt-in form GSR_BWD_REDUCE=mfma, measured slower);
 *    the image state carries the frame's walk classes (gsr_image_state_bytes grew; gsr_debug_walk_views); the backward's scratch
 *    carries validity flags of the gradient records (gsr_backward_scratch_bytes grew; gsr_debug_set_flags_min_r);
 *    later, additive: gsr_camera_grads, gsr_camera_grad_scratch_bytes, gsr_backward_camera (gradients of the camera);
 *    gsr_render_extras and the *_ex entry points (z-depth channel, accumulated-opacity plane and their gradients);
 *    gsr_knn_dist2 / gsr_knn_workspace_bytes (exact 3-nearest-neighbour distances) and gsr_unproject_rgbd /
 *    gsr_unproject_workspace_bytes (RGB-D keyframe -> points): the mapping half;
 *    gsr_render_extras.n_touched / touched_T_min (trailing fields; zero = as before): per-Gaussian visibility counts;
 *    gsr_backward_camera_only (+ _ex), gsr_pose_adam, gsr_pose_forward, gsr_pose_backward: pose tracking on the device;
 *    gsr_exposure_adam, gsr_exposure_blocks, gsr_exposure_forward, gsr_exposure_backward: per-view exposure and alpha mask;
 *    gsr_transform_workspace_bytes, gsr_transform_gaussians: the map follows keyframe pose corrections (SH bands rotated);
 *    gsr_unproject_params_k, gsr_unproject_rgbd_k (back-projection with a principal point), gsr_frame_undistort,
 *    gsr_frame_pyramid: frames of a real sensor - K-matrix cameras, undistortion, validity mask, image / depth pyramid;
 *    gsr_knn_k (k = 1 .. 32 neighbours), gsr_voxel_down_sample, gsr_statistical_outliers and their *_workspace_bytes queries:
 *    point-cloud conditioning before a cloud seeds Gaussians;
 *    gsr_debug_scan_tmp_bytes, gsr_debug_scan_u32, gsr_debug_tile_sort, gsr_debug_tile_depth_sort: test hooks of the binning stage's
 *    integer building blocks;
 *    gsr_nn_index_bytes, gsr_nn_index_build, gsr_nn_search, gsr_nn_order_workspace_bytes, gsr_nn_query_order, gsr_transform_points,
 *    gsr_icp_workspace_bytes, gsr_icp_update: nearest neighbours of one cloud in another, with the row, and point-to-point ICP;
 *    gsr_normals_workspace_bytes, gsr_estimate_normals (surface normals from a hybrid radius / max-count neighbourhood) and
 *    gsr_icp_update_plane (the point-to-plane update; gsr_icp_workspace_bytes grew);
 *    gsr_fpfh_workspace_bytes, gsr_compute_fpfh, gsr_feature_nn_workspace_bytes, gsr_feature_nn_tiles_per_split, gsr_feature_nn,
 *    gsr_ransac_workspace_bytes, gsr_ransac_feature_matching: global registration from feature matches (additions only);
 *    gsr_pc2_layout, gsr_pc2_decode_workspace_bytes, gsr_pc2_decode, gsr_pc2_encode, gsr_debug_pc2_force_direct: a
 *    sensor_msgs/PointCloud2 byte buffer decoded, cropped, posed and compacted on the device, and its inverse (additions only);
 *    gsr_image_layout, gsr_image_decode, gsr_image_encode_rgb8, gsr_depth_register_workspace_bytes, gsr_depth_register: a
 *    sensor_msgs/Image byte buffer (colour, Bayer, depth) decoded on the device, its rgb8 inverse, and a depth image moved into
 *    the colour camera (additions only);
 *    gsr_color_gradient_workspace_bytes, gsr_color_gradient, gsr_icp_colored_workspace_bytes, gsr_icp_update_colored: coloured
 *    ICP - the colour gradient of a cloud and the joint geometric / photometric update (additions only);
 *    gsr_odometry_prepare, gsr_odometry_workspace_bytes, gsr_odometry_update: dense frame-to-frame RGB-D odometry on the pixel
 *    grid - intensity / depth / Sobel planes and the hybrid photometric + depth Gauss-Newton update (additions only);
 *    gsr_information_workspace_bytes, gsr_registration_information, gsr_posegraph_topology_bytes, gsr_posegraph_topology,
 *    gsr_posegraph_workspace_bytes, gsr_posegraph_linearize, gsr_posegraph_solve, gsr_posegraph_optimize: an information matrix
 *    per edge and robust pose-graph optimisation in one launch (additions only);
 *    gsr_debug_slot_views: the emission slot of every list position, for tests that read the backward's gradient records;
 *    gsr_tsdf_volume, gsr_tsdf_frame, gsr_tsdf_touch, gsr_tsdf_integrate, gsr_tsdf_extract_workspace_bytes, gsr_tsdf_extract_points,
 *    gsr_tsdf_extract_triangles: depth frames fused into a block-sparse TSDF volume, out as a cloud and a mesh (additions only);
 *    gsr_orb_cells, gsr_orb_prepare, gsr_orb_detect, gsr_orb_describe, gsr_orb_pattern, gsr_hamming_match, gsr_hamming_vote: FAST
 *    corners, steered BRIEF descriptors and Hamming matching for place recognition (additions only);
 *    gsr_cloud_camera, gsr_cloud_project_workspace_bytes, gsr_cloud_project, gsr_depth_densify: a LiDAR cloud projected into the
 *    colour camera - sparse depth, winner rows, visibility, image colours - and the sparse depth filled (additions only);
 *    gsr_covariance_workspace_bytes, gsr_estimate_covariances, gsr_regularize_covariances, gsr_icp_generalized_workspace_bytes,
 *    gsr_icp_update_generalized: generalized ICP - a covariance per point and the plane-to-plane update (additions only);
 *    gsr_scan_context, gsr_scan_context_distance: the polar descriptor of a LiDAR scan and the search over all column shifts -
 *    place recognition with a yaw estimate (additions only);
 * 6: host_status word 0 bit 0 = radix-sort look-back time-out (was reserved; debug = 1 fails the call), gsr_debug_wave_reduce_pk,
 *    gsr_forward_async_culled (host_status word 0 bit 1 / word 6 = a truncated tile list was too short);
 * 5: gsr_fused_adam.dynamic + gsr_adam_set_dynamic (optimizer factors in device memory, for HIP-graph replay), gsr_l1_mean_*;
 * 4: gsr_forward_async(num_rendered_out) / gsr_forward_rerender (verified speculation), gsr_sh_rank1_*; 3: gsr_backward_adam */
#define GSR_ABI_VERSION 7

enum {
  GSR_OK = 0,
  GSR_ERR_INVALID_ARGUMENT = -1, /* bad combination of inputs (both/neither of shs|colors_precomp ...) */
  GSR_ERR_HIP = -2,              /* a HIP runtime call failed */
  GSR_ERR_PREFILTERED_CULLED = -3, /* prefiltered=1 but a point failed the near-plane test */
  GSR_ERR_TOO_MANY_INSTANCES = -4, /* num_rendered (or the capacity) exceeds 2^30 - 1 */
  GSR_ERR_STATE_TOO_SMALL = -5   /* a caller-provided state buffer is smaller than required */
};

/* GaussianRasterizationSettings, reference gaussian_renderer/__init__.py:36-50 (13 fields). */
typedef struct gsr_settings {
  int32_t image_height;
  int32_t image_width;
  float tanfovx;
  float tanfovy;
  const float* bg;          /* [3]  */
  float scale_modifier;
  const float* viewmatrix;  /* [16] */
  const float* projmatrix;  /* [16] */
  int32_t sh_degree;        /* active degree, 0..3 */
  const float* campos;      /* [3]  */
  int32_t prefiltered;
  int32_t debug;            /* 1: synchronise and check after every kernel */
  int32_t antialiasing;
} gsr_settings;

/* Arguments of GaussianRasterizer.forward, reference gaussian_renderer/__init__.py:90-109.
 * Exactly one of {shs (+ optional dc), colors_precomp} and exactly one of {scales+rotations, cov3D_precomp}
 * must be non-NULL (same rule, same error, as the reference's rasterizer). */
typedef struct gsr_gaussians {
  int32_t P;                   /* number of Gaussians */
  int32_t sh_coeffs;           /* coefficients per channel stored in `shs` (row stride), e.g. 16 (or 15 with dc) */
  const float* means3D;        /* [P,3] */
  const float* dc;             /* [P,1,3] or NULL: SH band 0 kept separately (the `separate_sh` call form, :90-99) */
  const float* shs;            /* [P,sh_coeffs,3] or NULL */
  const float* colors_precomp; /* [P,3] or NULL */
  const float* opacities;      /* [P] */
  const float* scales;         /* [P,3] or NULL */
  const float* rotations;      /* [P,4] (w,x,y,z), used as given, or NULL */
  const float* cov3D_precomp;  /* [P,6] (xx,xy,xz,yy,yz,zz) or NULL */
  int32_t raw_activations;     /* 0: opacities / scales / rotations are activated values (the reference's call form).
                                * 1: they are the model's RAW parameters (scene/gaussian_model.py:55-57 _scaling, _rotation,
                                *    _opacity): exp / normalize / sigmoid (:38-46) are applied on load, and gsr_backward returns
                                *    the gradients w.r.t. the raw parameters - the model then needs no activation kernels in
                                *    the training step.  Ignored for cov3D_precomp. */
} gsr_gaussians;

/* Gradients returned by the backward, in the order the reference's autograd Function returns them
 * (SURVEY.md 8(a) a3).  Every non-NULL pointer is fully written (zeros for culled Gaussians). */
typedef struct gsr_grads {
  float* dL_dmeans3D;   /* [P,3] */
  float* dL_dmeans2D;   /* [P,3] screen-space gradient in NDC units, z = 0 (consumed by
                           scene/gaussian_model.py:431-433 add_densification_stats) */
  float* dL_ddc;        /* [P,1,3] or NULL */
  float* dL_dshs;       /* [P,sh_coeffs,3] or NULL (NULL although `shs` was given: allowed with `dc` - only dL_ddc is formed,
                           the view-sharded "sh_rank1" exchange rebuilds the rest from it) */
  float* dL_dcolors;    /* [P,3] or NULL (colors_precomp) */
  float* dL_dopacities; /* [P] */
  float* dL_dscales;    /* [P,3] or NULL */
  float* dL_drotations; /* [P,4] or NULL */
  float* dL_dcov3D;     /* [P,6] or NULL (cov3D_precomp) */
  /* Optional (all three or none): the backward also performs this view's add_densification_stats (reference
   * scene/gaussian_model.py:431-433) and max_radii2D update (train.py:159) - where radii > 0: xyz_gradient_accum +=
   * |dL_dmeans2D.xy|, denom += 1, max_radii2D = max(max_radii2D, radii) - the same arithmetic as gsr_densification_stats,
   * without the extra pass over P. */
  float* xyz_gradient_accum; /* [P,1] */
  float* denom;              /* [P,1] */
  float* max_radii2D;        /* [P]   */
} gsr_grads;

int gsr_abi_version(void);
const char* gsr_last_error(void);

/* State-buffer sizes (bytes).  Binning state depends on num_rendered, known after gsr_forward_prepare. */
size_t gsr_geometry_state_bytes(int32_t P);
size_t gsr_image_state_bytes(int32_t image_width, int32_t image_height);
size_t gsr_binning_state_bytes(int32_t P, int32_t image_width, int32_t image_height, int64_t num_rendered);
size_t gsr_backward_scratch_bytes(int32_t P, int64_t num_rendered);

/* Forward, phase 1: preprocess (projection, EWA covariance, SH->RGB), depth ordering and the tile-count
 * prefix sum.  Writes radii[P] (int32; 0 = culled; reference :118-121 `radii`, `visibility_filter`).
 * Waits once for num_rendered to arrive on the host (the reference rasterizer has the same single read-back); the
 * count is taken right after the projection kernel, so on return the depth sort / prefix sum may still be running on
 * `stream` - everything later is stream-ordered behind them.  Returns num_rendered >= 0 or an error code. */
int64_t gsr_forward_prepare(const gsr_settings* s, const gsr_gaussians* g, void* geometry_state,
                            size_t geometry_bytes, int32_t* radii, void* stream);

/* Split form of phase 1 for the view-sharded data-parallel trainer: gsr_forward_prepare_geometry does everything
 * gsr_forward_prepare does EXCEPT the SH -> RGB evaluation (it does not read `dc` / `shs`); gsr_forward_shade fills the colours
 * and must run before gsr_forward_render.  Between the two calls the caller may wait for the SH coefficients of this step
 * (81 % of the gradient bytes) to finish their all-reduce + Adam update on another stream.  Results are bitwise identical
 * to the fused gsr_forward_prepare. */
int64_t gsr_forward_prepare_geometry(const gsr_settings* s, const gsr_gaussians* g, void* geometry_state,
                                     size_t geometry_bytes, int32_t* radii, void* stream);
int gsr_forward_shade(const gsr_settings* s, const gsr_gaussians* g, void* geometry_state, void* stream);

/* Forward, phase 2: instance emission, tile sort, tile ranges and 16x16-tile alpha compositing.
 * Writes out_color[3,H,W] and out_invdepth[1,H,W] (reference :90,:101 `rendered_image`, `depth_image`).
 * `for_backward` != 0 additionally records what gsr_backward needs in the state buffers (the emission slot of every list
 * position rides through the tile sort); 0 = forward-only render, a gsr_backward on these buffers is then undefined. */
int gsr_forward_render(const gsr_settings* s, const gsr_gaussians* g, void* geometry_state,
                       void* binning_state, size_t binning_bytes, int64_t num_rendered, void* image_state,
                       size_t image_bytes, float* out_color, float* out_invdepth, int32_t for_backward,
                       void* stream);

/* gsr_forward_prepare_geometry's companion that evaluates the colours as LATE as possible: instance emission, tile sort and
 * tile ranges run first (none of them reads `dc` / `shs`), then `stream` waits for `sh_ready_event` (a hipEvent_t recorded by
 * the caller after the SH coefficients' update; NULL = no wait), then the SH -> RGB pass (what gsr_forward_shade does), then
 * the compositing: the whole binning stage overlaps an SH exchange / update running on another stream.  Same results. */
int gsr_forward_render_shade(const gsr_settings* s, const gsr_gaussians* g, void* geometry_state,
                             void* binning_state, size_t binning_bytes, int64_t num_rendered, void* image_state,
                             size_t image_bytes, float* out_color, float* out_invdepth, int32_t for_backward,
                             void* sh_ready_event, void* stream);

/* Speculative forward (phase 1 + phase 2 in ONE call, sized by the caller's estimate): for callers that keep grow-only state
 * buffers (a SLAM / training loop).  The reference's rasterizer reads num_rendered back in the middle of every forward to size
 * its binning buffer (SURVEY.md 2.3 "D2H num_rendered"; call site gaussian_renderer/__init__.py:90-109), which leaves the device
 * idle while the host allocates and enqueues the rest.  Here the binning state is sized by the caller for `capacity` instances
 * (gsr_binning_state_bytes(.., capacity)), the WHOLE frame is enqueued, num_rendered stays on the device and every later stage
 * reads min(num_rendered, capacity) from there.  Two ways to use it:
 *
 *   verified (num_rendered_out != NULL; what diff_gaussian_rasterization does by default): after everything is enqueued the
 *     call waits until the count has reached the host - the kernel that knows it stores it straight into pinned memory, with
 *     the binning and compositing stages still queued behind it, so the device does not idle - and returns it in
 *     *num_rendered_out.  If it exceeds `capacity` the frame just enqueued was composited from a TRUNCATED instance list: the
 *     caller grows its binning state and calls gsr_forward_rerender, which repeats phase 2 exactly; outputs and state are then
 *     those of the blocking pair, bit for bit.  Every frame is exact.
 *   unverified (num_rendered_out == NULL): no wait at all.  A frame beyond `capacity` loses the surplus - emitted last: its
 *     farthest splats with tile_local_sort = 0, the Gaussians with the highest indices with tile_local_sort = 1 - never an
 *     out-of-bounds access; the caller learns it later from `host_status`.  gsr_backward / gsr_backward_adam on such a frame
 *     are NO-OPS by construction (every backward kernel reads the count): zero gradients, no optimizer update, no statistics.
 *
 *   host_status: NULL or 8 words of host memory, filled asynchronously on `stream` at the END of the call's work:
 *                [0] bit 0 = a radix-sort look-back wait timed out on the device (broken inter-workgroup hand-off: the frame is
 *                mis-sorted; with debug = 1 the call itself fails with GSR_ERR_HIP), [1] bit 0 = a prefiltered point failed the near-plane test, [2],[3] = num_rendered (lo, hi),
 *                [4] = longest tile list of the frame if it exceeds 2048 entries, else 0 (tile_local_sort only).
 *                Pinned memory (hipHostMalloc / torch pin_memory) is written by the compositing kernel itself through its
 *                device mapping; any other host memory gets a hipMemcpyAsync.  Read it after an event recorded behind this
 *                call has completed.
 *   tile_local_sort: 0 = the binning of the blocking path (global depth sort of the Gaussians, emission in depth order, stable
 *                tile sort).  1 = no global depth order: emission in index order, the same stable tile sort, then every
 *                tile orders ITS list by (depth bits, id) in LDS (binning.hip, k_tile_depth_sort) - identical lists, about
 *                0.07 ms less per frame at 1 M Gaussians / 1080p (the tile counts are then also scanned inside the projection
 *                and emission kernels: four launches fewer); lists longer than 4096 entries take a slow in-memory path, so a
 *                caller should fall back to 0 when host_status[4] approaches that (diff_gaussian_rasterization/_workspace.py).
 *   defer_color / sh_ready_event: as gsr_forward_prepare_geometry + gsr_forward_render_shade (0 / NULL: fused colour pass).
 * The matching gsr_backward takes `capacity` as its num_rendered.  Same kernels, same results as the blocking pair whenever
 * num_rendered <= capacity. */
int gsr_forward_async(const gsr_settings* s, const gsr_gaussians* g, void* geometry_state, size_t geometry_bytes,
                      int32_t* radii, void* binning_state, size_t binning_bytes, int64_t capacity, void* image_state,
                      size_t image_bytes, float* out_color, float* out_invdepth, int32_t for_backward,
                      int32_t defer_color, void* sh_ready_event, uint32_t* host_status, int32_t tile_local_sort,
                      void* stream, int64_t* num_rendered_out /* host, or NULL */);

/* gsr_forward_async with TILE LISTS TRUNCATED BY DEPTH (round 4).  tile_depth_cutoff: `tiles` uint32 words owned by the caller, one
 * array per VIEW it renders repeatedly (a training set's cameras), initialised to 0xFFFFFFFF.  Every call UPDATES it: the
 * compositing kernel leaves, per tile, the depth bits of the list entry at 1.75 x (+ 48) the position of the deepest one any pixel
 * of the tile needed before it saturated (T < 1e-4) - 0xFFFFFFFF if a pixel never saturated or the list is shorter than that.  Both
 * binning forms (tile_local_sort 0 and 1) learn the same words; a call with P == 0 or capacity == 0 leaves the array as it was
 * (tests/test_tile_cull_cutoffs_gpu.py holds every word to a float64 reconstruction).  With apply != 0 (honoured only for an
 * unverified frame, num_rendered_out == NULL, in the tile-local binning form, debug off) the array is also USED: a (tile, Gaussian)
 * instance whose depth lies behind its tile's cut-off is neither counted nor emitted - the tile's depth-ordered list loses its
 * tail.  If every pixel of a truncated tile still saturates inside its list, image, depth, final_T, n_contrib and all gradients
 * are those of the untruncated frame bit for bit (the loop never reached the missing tail).  If one does not, the frame flags
 * itself: status word 0 bit 1 on the device - gsr_backward / gsr_backward_adam are then NO-OPS, as for a frame beyond the capacity -
 * and word 6 of host_status (clear it before the call; final once an event recorded behind the call has completed); the caller
 * renders that view again with apply = 0.  Where a scene saturates early (dense captures) this removes most of the R-proportional
 * work of the step: emission, both tile-sort passes, per-tile ordering, the gradient-record gather. */
int gsr_forward_async_culled(const gsr_settings* s, const gsr_gaussians* g, void* geometry_state, size_t geometry_bytes,
                             int32_t* radii, void* binning_state, size_t binning_bytes, int64_t capacity, void* image_state,
                             size_t image_bytes, float* out_color, float* out_invdepth, int32_t for_backward,
                             int32_t defer_color, void* sh_ready_event, uint32_t* host_status, int32_t tile_local_sort,
                             void* stream, int64_t* num_rendered_out, uint32_t* tile_depth_cutoff, int32_t apply);
/* Phase 2 once more on the state a gsr_forward_async call with the same `s`, `g`, geometry / image state and tile_local_sort
 * left behind, for a (larger) binning state of `capacity` >= the count that call reported: instance emission, tile sort,
 * ranges, per-tile ordering, compositing.  Stream-ordered behind the first attempt; overwrites its outputs. */
int gsr_forward_rerender(const gsr_settings* s, const gsr_gaussians* g, void* geometry_state, void* binning_state,
                         size_t binning_bytes, int64_t capacity, void* image_state, size_t image_bytes, float* out_color,
                         float* out_invdepth, int32_t for_backward, int32_t tile_local_sort, uint32_t* host_status,
                         void* stream);

/* Backward of the calls above.  dL_dinvdepth may be NULL (treated as zero).  `num_rendered`: the value gsr_forward_prepare
 * returned (and gsr_forward_render was given), or the `capacity` given to gsr_forward_async. */
int gsr_backward(const gsr_settings* s, const gsr_gaussians* g, const int32_t* radii,
                 const void* geometry_state, const void* binning_state, const void* image_state,
                 int64_t num_rendered, const float* dL_dcolor, const float* dL_dinvdepth,
                 void* scratch, size_t scratch_bytes, const gsr_grads* grads, void* stream);

/* gsr_backward that also returns the gradients of the CAMERA: dL/d(viewmatrix), dL/d(projmatrix) (the settings' row-major
 * transposed 4x4 matrices, [16] each) and dL/d(campos) [3] - what a photometric pose refinement (tracking) differentiates through.
 * Everything gsr_backward writes is written too, bit for bit the same.  Each non-NULL pointer of `cam` is a DEVICE array written in
 * full: column 3 of dL/dviewmatrix and column 2 of dL/dprojmatrix are always zero, dL/dcampos is zero for colors_precomp and SH
 * degree 0, and all are zero for P = 0, a frame without visible Gaussians and an overflowed unverified frame.  The per-Gaussian
 * terms are summed per workgroup by cross-lane trees, then in a fixed order over the workgroups: no float atomics, the result is
 * bitwise reproducible.  cam_scratch: gsr_camera_grad_scratch_bytes(P) bytes of device memory.  `grads` as for gsr_backward. */
typedef struct gsr_camera_grads {
  float* dL_dviewmatrix; /* [16] or NULL */
  float* dL_dprojmatrix; /* [16] or NULL */
  float* dL_dcampos;     /* [3]  or NULL */
} gsr_camera_grads;
size_t gsr_camera_grad_scratch_bytes(int32_t P);
int gsr_backward_camera(const gsr_settings* s, const gsr_gaussians* g, const int32_t* radii,
                        const void* geometry_state, const void* binning_state, const void* image_state,
                        int64_t num_rendered, const float* dL_dcolor, const float* dL_dinvdepth,
                        void* scratch, size_t scratch_bytes, const gsr_grads* grads, const gsr_camera_grads* cam,
                        void* cam_scratch, size_t cam_scratch_bytes, void* stream);

/* gsr_backward_camera WITHOUT the per-Gaussian outputs: the backward of a tracking iteration, where the map is frozen and only
 * the pose is refined.  No gsr_grads: the projection backward stores nothing per Gaussian - at SH
 * degree 3 about 62 floats per Gaussian that nobody would read - and only forms what the 27 camera sums need.  The sums and
 * their order are gsr_backward_camera's: the three gradients equal, bit for bit, those of gsr_backward_camera on the same frame
 * (called with a 16-byte aligned dL_dshs, as every caller in this repository does: the alignment decides between the 64- and the
 * 256-Gaussian workgroup there, the alignment of `shs` alone here).  At least one pointer of `cam` must be set
 * (GSR_ERR_INVALID_ARGUMENT otherwise); cam_scratch as for gsr_backward_camera, checked before anything is launched. */
int gsr_backward_camera_only(const gsr_settings* s, const gsr_gaussians* g, const int32_t* radii,
                             const void* geometry_state, const void* binning_state, const void* image_state,
                             int64_t num_rendered, const float* dL_dcolor, const float* dL_dinvdepth,
                             void* scratch, size_t scratch_bytes, const gsr_camera_grads* cam,
                             void* cam_scratch, size_t cam_scratch_bytes, void* stream);

/* gsr_backward with the optimizer step folded in (single-GPU training step: reference train.py:139 loss.backward() followed
 * by :170-179 optimizer.step(), when nothing sits between the two - no gradient exchange, no accumulation over views, no
 * densification at this iteration).  The six parameter groups of reference scene/gaussian_model.py:160-168 are updated IN PLACE
 * by the backward's last kernel from the gradients it holds in registers / LDS; those gradients (59 floats per Gaussian at SH
 * degree 3) are never written to memory, and no separate optimizer kernel re-reads them.
 *   Requirements: raw_activations = 1 (opacities / scales / rotations are the model's raw parameters), `dc` and `shs` passed
 *   separately (the separate_sh call form), no colors_precomp / cov3D_precomp.  The arrays of `g` are the parameters themselves
 *   and are written to (the `const` of gsr_gaussians does not hold for this call).
 *   Group order of the arrays below: 0 xyz (g->means3D), 1 f_dc (g->dc), 2 f_rest (g->shs), 3 opacity, 4 scaling, 5 rotation.
 *   sparse = 0: torch.optim.Adam semantics (bias correction; `step` = 1-based step number AFTER this update), every row.
 *   sparse = 1: SparseGaussianAdam.step(radii > 0, P) semantics (reference train.py:173-176): rows with radii == 0 untouched,
 *               no bias correction.
 *   sparse = 2: as 0, but only the rows that have tile instances in this forward are updated here; the others (their gradient
 *               is exactly zero) must get their update from gsr_adam_step_culled_rows with the same `opt` values - a call
 *               that needs nothing from the backward and can therefore run on another stream while the compositing kernels
 *               (bound by VALU issue, not by HBM) are busy.  The pair equals sparse = 0 bit for bit.
 * grads->dL_dmeans2D is still written (densification statistics, scene/gaussian_model.py:431-433); the other members of `grads`
 * are ignored.  Same arithmetic as gsr_backward followed by gsr_adam_step / gsr_sparse_adam_step, bit for bit. */
typedef struct gsr_fused_adam {
  float* exp_avg[6];
  float* exp_avg_sq[6];
  float lr[6];
  int64_t step[6];
  double beta1, beta2, eps;
  int32_t sparse;
  /* Optional DEVICE pointer to GSR_ADAM_DYNAMIC_FLOATS floats (lr[6], lr / bias_correction1 [6], 1 / sqrt(bias_correction2) [6]),
   * or NULL.  When set, the kernels read the per-step factors from there instead of deriving them from `lr` / `step`: the call
   * then carries no per-step constant in its launch arguments and can be captured once into a HIP graph and replayed, with
   * gsr_adam_set_dynamic enqueued in front of every replay. */
  const float* dynamic;
} gsr_fused_adam;
#define GSR_ADAM_DYNAMIC_FLOATS 18
/* Computes the factors of `opt` (its lr / step / betas / sparse, exactly as gsr_backward_adam would) and enqueues a one-workgroup
 * kernel that stores them to `dynamic_dev`: the values travel as launch arguments, so the host may call it again at once. */
int gsr_adam_set_dynamic(const gsr_fused_adam* opt, float* dynamic_dev, void* stream);
int gsr_backward_adam(const gsr_settings* s, const gsr_gaussians* g, const int32_t* radii, const void* geometry_state,
                      const void* binning_state, const void* image_state, int64_t num_rendered, const float* dL_dcolor,
                      const float* dL_dinvdepth, void* scratch, size_t scratch_bytes, const gsr_grads* grads,
                      const gsr_fused_adam* opt, void* stream);

/* Depth and opacity images for RGB-D tracking.  Every `_ex` entry point below takes the
 * arguments of the entry point of the same name without `_ex`, plus `extras` LAST; extras == NULL is exactly that entry point.
 *   depth_kind: what the depth plane (`out_invdepth` of the forward, `dL_dinvdepth` of the backward) holds -
 *               GSR_DEPTH_INVERSE: sum_i w_i / z_i (the reference's inverse depth, the default);
 *               GSR_DEPTH_Z:       sum_i w_i z_i (view-space z-depth), w_i = alpha_i T_i the compositing weight.
 *               It takes effect in the projection (gsr_forward_prepare*_ex / gsr_forward_async*_ex: the state buffers then hold it)
 *               and must be given again, with the same value, to the backward of that frame.  Colour, radii, final_T and
 *               n_contrib do not depend on it.
 *   out_alpha:  forward: NULL, or a DEVICE [H,W] plane that receives the accumulated opacity A = 1 - T_final of every pixel
 *               (bit for bit 1 - the final_T of gsr_debug_image_views).
 *   dL_dalpha:  backward: NULL (zero), or the DEVICE [H,W] gradient of that plane.  It reaches opacities, means, covariances
 *               and the camera through the compositing backward's per-pixel background term (dA/dalpha_i = T_final / (1 -
 *               alpha_i)): no extra work per composited entry, no float atomics; a zero plane gives the gradients of NULL bit
 *               for bit.  An overflowed unverified frame gives zero gradients through it, as through everything else.
 * Per-Gaussian visibility counts for keyframe selection and pruning, two TRAILING fields: a
 * zero-initialised tail is the struct as it was.
 *   n_touched:  forward: NULL (off), or a DEVICE [P] array; n_touched[i] receives the number of pixels in which Gaussian i is
 *               BLENDED (power <= 0, alpha >= 1/255, pixel not finished, not the entry that stops the pixel) while the pixel's
 *               transmittance BEFORE blending it is > touched_T_min.  The memory may be uninitialised: every forward call that
 *               composites (phase 2, gsr_forward_async*_ex, gsr_forward_rerender_ex) zeroes it first, so the counts always belong
 *               to the frame that call returns and a repeated phase 2 counts nothing twice.  Rows that reach no tile get 0; an
 *               unverified frame truncated by its capacity gets all zeros, like its gradients.  Integer adds only: bit-identical
 *               from run to run and across forward modes, binning forms and walk orders.  gsr_forward_prepare*_ex and the
 *               backward ignore it.
 *   touched_T_min: in [0, 1); 0 counts every blended (Gaussian, pixel) pair, 0.5 "seen through less than half occlusion".
 *               Outside [0, 1), or NaN, with n_touched != NULL: GSR_ERR_INVALID_ARGUMENT before any device work. */
enum { GSR_DEPTH_INVERSE = 0, GSR_DEPTH_Z = 1 };
typedef struct gsr_render_extras {
  int32_t depth_kind;      /* GSR_DEPTH_INVERSE | GSR_DEPTH_Z; anything else: GSR_ERR_INVALID_ARGUMENT */
  float* out_alpha;        /* [H,W] or NULL (forward) */
  const float* dL_dalpha;  /* [H,W] or NULL (backward) */
  uint32_t* n_touched;     /* [P] or NULL (forward) */
  float touched_T_min;     /* [0, 1); read only when n_touched != NULL */
} gsr_render_extras;
int64_t gsr_forward_prepare_ex(const gsr_settings* s, const gsr_gaussians* g, void* geometry_state, size_t geometry_bytes,
                               int32_t* radii, void* stream, const gsr_render_extras* extras);
int64_t gsr_forward_prepare_geometry_ex(const gsr_settings* s, const gsr_gaussians* g, void* geometry_state,
                                        size_t geometry_bytes, int32_t* radii, void* stream, const gsr_render_extras* extras);
int gsr_forward_render_ex(const gsr_settings* s, const gsr_gaussians* g, void* geometry_state, void* binning_state,
                          size_t binning_bytes, int64_t num_rendered, void* image_state, size_t image_bytes, float* out_color,
                          float* out_invdepth, int32_t for_backward, void* stream, const gsr_render_extras* extras);
int gsr_forward_render_shade_ex(const gsr_settings* s, const gsr_gaussians* g, void* geometry_state, void* binning_state,
                                size_t binning_bytes, int64_t num_rendered, void* image_state, size_t image_bytes,
                                float* out_color, float* out_invdepth, int32_t for_backward, void* sh_ready_event,
                                void* stream, const gsr_render_extras* extras);
int gsr_forward_async_ex(const gsr_settings* s, const gsr_gaussians* g, void* geometry_state, size_t geometry_bytes,
                         int32_t* radii, void* binning_state, size_t binning_bytes, int64_t capacity, void* image_state,
                         size_t image_bytes, float* out_color, float* out_invdepth, int32_t for_backward,
                         int32_t defer_color, void* sh_ready_event, uint32_t* host_status, int32_t tile_local_sort,
                         void* stream, int64_t* num_rendered_out, const gsr_render_extras* extras);
int gsr_forward_async_culled_ex(const gsr_settings* s, const gsr_gaussians* g, void* geometry_state, size_t geometry_bytes,
                                int32_t* radii, void* binning_state, size_t binning_bytes, int64_t capacity, void* image_state,
                                size_t image_bytes, float* out_color, float* out_invdepth, int32_t for_backward,
                                int32_t defer_color, void* sh_ready_event, uint32_t* host_status, int32_t tile_local_sort,
                                void* stream, int64_t* num_rendered_out, uint32_t* tile_depth_cutoff, int32_t apply,
                                const gsr_render_extras* extras);
int gsr_forward_rerender_ex(const gsr_settings* s, const gsr_gaussians* g, void* geometry_state, void* binning_state,
                            size_t binning_bytes, int64_t capacity, void* image_state, size_t image_bytes, float* out_color,
                            float* out_invdepth, int32_t for_backward, int32_t tile_local_sort, uint32_t* host_status,
                            void* stream, const gsr_render_extras* extras);
int gsr_backward_ex(const gsr_settings* s, const gsr_gaussians* g, const int32_t* radii, const void* geometry_state,
                    const void* binning_state, const void* image_state, int64_t num_rendered, const float* dL_dcolor,
                    const float* dL_dinvdepth, void* scratch, size_t scratch_bytes, const gsr_grads* grads, void* stream,
                    const gsr_render_extras* extras);
int gsr_backward_camera_ex(const gsr_settings* s, const gsr_gaussians* g, const int32_t* radii, const void* geometry_state,
                           const void* binning_state, const void* image_state, int64_t num_rendered, const float* dL_dcolor,
                           const float* dL_dinvdepth, void* scratch, size_t scratch_bytes, const gsr_grads* grads,
                           const gsr_camera_grads* cam, void* cam_scratch, size_t cam_scratch_bytes, void* stream,
                           const gsr_render_extras* extras);
int gsr_backward_camera_only_ex(const gsr_settings* s, const gsr_gaussians* g, const int32_t* radii,
                                const void* geometry_state, const void* binning_state, const void* image_state,
                                int64_t num_rendered, const float* dL_dcolor, const float* dL_dinvdepth, void* scratch,
                                size_t scratch_bytes, const gsr_camera_grads* cam, void* cam_scratch,
                                size_t cam_scratch_bytes, void* stream, const gsr_render_extras* extras);
int gsr_backward_adam_ex(const gsr_settings* s, const gsr_gaussians* g, const int32_t* radii, const void* geometry_state,
                         const void* binning_state, const void* image_state, int64_t num_rendered, const float* dL_dcolor,
                         const float* dL_dinvdepth, void* scratch, size_t scratch_bytes, const gsr_grads* grads,
                         const gsr_fused_adam* opt, void* stream, const gsr_render_extras* extras);

/* Dense Adam update (zero gradient: moments decay, the parameter follows its momentum) of the rows that reached no tile in the
 * forward whose geometry state is given; companion of gsr_backward_adam(opt->sparse = 2).  May be enqueued on any stream once
 * the forward call that filled `geometry_state` has been enqueued and that stream waits for it; the caller orders it before the
 * next forward.  `g`, `num_rendered` and `opt` as for gsr_backward_adam (same `step` values). */
int gsr_adam_step_culled_rows(const gsr_gaussians* g, const void* geometry_state, int64_t num_rendered,
                              const gsr_fused_adam* opt, void* stream);

/* GaussianRasterizer.markVisible (near-plane test).  present[P] uint8. */
int gsr_mark_visible(int32_t P, const float* means3D, const float* viewmatrix, uint8_t* present, void* stream);

/* Introspection for tests / bench: DEVICE pointers into the opaque state buffers (valid while the buffer lives). */
/* rec48: the packed 48-B splat records, 12 floats per Gaussian = (mean2D.xy, conic A' B') (conic C', opacity, cut-off, r)
 * (g, b, 1/depth - or depth with GSR_DEPTH_Z -, depth); clamped: one byte per Gaussian, bit c set = colour channel c was clamped at 0 (any out pointer may
 * be NULL)
 *
 * Projection rules (what fills these views; SURVEY.md Appendix A plus the guards and margins stated only here; float32 throughout,
 * no fused multiply-add; tests/projection_reference.py restates them in numpy and tests/test_projection_replay_gpu.py holds the
 * kernels to that):
 *   t = V^T (p, 1); visible needs t.z > 0.2f, det != 0 and a non-empty 3-sigma rectangle.  hom = PV^T (p, 1),
 *   pw = 1 / (hom.w + 1e-7f), ndc = hom.xy pw, mean2D = ((ndc + 1) (W, H) - 1) / 2.
 *   Sigma = R diag(scale_modifier s)^2 R^T (q used as given; raw_activations: s = exp, q = q / max(|q|, 1e-12f), opacity = sigmoid).
 *   t.x / t.z and t.y / t.z are clamped to +-1.3f tanfov (then multiplied by t.z again); J = (fx / t.z, 0, -fx t.x / t.z^2;
 *   0, fy / t.z, -fy t.y / t.z^2), fx = W / (2 tanfovx); cov2D = (J W) Sigma (J W)^T; (a, b, c) = (cov.xx + 0.3f, cov.xy, cov.yy + 0.3f);
 *   det = a c - b^2; conic (A, B, C) = (c, -b, a) / det; antialiasing: opacity x sqrt(max(0.000025f, det0 / det)), det0 before the 0.3f.
 *   radius = ceil(3 sqrt(max(mid + r, mid - r))), mid = (a + c) / 2, r = sqrt(max(0.1f, mid^2 - det)); 3-sigma rectangle =
 *   clamp(trunc((mean2D -+ radius (+ 15)) / 16), 0, grid), the quotient clamped to +-1e9f before the conversion.
 *   cut-off pmin = -ln(255 op) - 0.01f (op > 0; else 1): a pixel with power < pmin has alpha < 1 / 255.
 *   first-stage box (what `rect` holds): q = -2 pmin; q <= 0 (255 op <= e^-0.01): empty; else half-widths
 *   h = sqrt(q (a | c)) 1.0001f + 0.01f and tiles ceil((mean - h - 15) / 16) .. floor((mean + h) / 16) inside the 3-sigma rectangle;
 *   the second stage keeps, per tile row ty of the box, the columns the ellipse d^T conic d <= q reaches: with (A, B, C, q) taken
 *   back from the record words, half-height hy = sqrt(q A / det) 1.0001f + 0.01f; the row's band y in [16 ty - mean.y, + 15] cut to
 *   [-hy, hy] (empty: no tile); at the band's y nearest to the extreme points -+B sqrt(q / (C det)) the column ends
 *   x = (-B y +- sqrt(A qa - det y^2)) / A +- 0.01f with qa = 1.0002f q + 0.002f; tiles ceil((mean.x + xlo - 15) / 16) ..
 *   floor((mean.x + xhi) / 16) inside the box (reciprocals and square roots to 1 ulp).  tiles_touched is their number and `rect`
 *   is all zeros where it is 0.
 *   record words 2, 3, 4, 6 are in base 2: A' = -(log2e / 2) A, B' = -log2e B, C' = -(log2e / 2) C, cut-off' = log2e pmin
 *   (log2e = 1.4426950408889634f), so that log2(alpha / op) = (A' dx + B' dy) dx + C' dy dy.
 *   colour = max(0, 0.5 + sum_k basis_k(dir) sh_k), dir = (p - campos) / |p - campos|; evaluated only where tiles_touched > 0
 *   (zeros elsewhere); word 10 = 1 / t.z or t.z (GSR_DEPTH_Z); word 11 = t.z, whose bits are the depth key (0xFFFFFFFF: invisible).
 *   backward only: d conic / d(a, b, c) carries 1 / (det^2 + 1e-7f); the clamped t.x (t.y) is a constant (zero dL/dt.x, and not
 *   differentiated in J's dependence on t.z); dL/dscale keeps the scale_modifier factor. */
int gsr_debug_geometry_views(const void* geometry_state, int32_t P, const float** rec48, const uint32_t** depth_keys_sorted,
                             const uint32_t** order, const uint32_t** tiles_touched, const uint16_t** rect,
                             const uint32_t** offsets, const uint8_t** clamped);
/* test hook: 64-lane sums through the render backward's cross-lane reductions; in[10][64] -> out[20]:
 * out[0..9] = the ten-value tree, out[10..18] = the nine-value tree on rows 0..8, out[19] unused */
int gsr_debug_wave_reduce(const float* in640, float* out20, void* stream);
/* the same sums through the packed-pair trees (v_pk_add_f32 behind the swap stages) of k_render_bwd_tile; same layout */
int gsr_debug_wave_reduce_pk(const float* in640, float* out20, void* stream);
/* test hook: the matrix-pipe form of the same reduction (k_render_bwd_tile_mx: each lane's terms about the mean, summed over the wave by
 * v_mfma_f32_16x16x4_f32).
 * in[514] = h[4][64] (sub-block s = 0..3, lane: the pixel's dL/dopacity_eff), c[4][64] (the lane's channel sums), mu[2] (the 2-D mean
 * relative to the tile centre); out[10] = the gradient record's ten values (sum h dx, sum h dy, sum h dx^2, sum h dx dy, sum h dy^2,
 * sum h, c0..c3) with d = mu - pixel, pixel (x, y) of (s, lane) = ((lane & 7) + 8 (s & 1) - 7.5, (lane >> 3) + 8 (s >> 1) - 7.5) */
int gsr_debug_mx_reduce(const float* in514, float* out10, void* stream);
int gsr_debug_binning_views(const void* binning_state, int32_t image_width, int32_t image_height,
                            int64_t num_rendered, const uint32_t** point_list, const uint32_t** ranges);
/* slot_of_pos[num_rendered]: the emission slot of every position of point_list, as a forward with a backward to follow leaves it
 * (for_backward != 0; either binning form).  gsr_backward writes the per-instance gradient record of list position p, three
 * float4 = (sum h dx, sum h dy, sum h dx^2, sum h dx dy) (sum h dy^2, sum h, d_r, d_g) (d_b, d_depth, -, -), at record index
 * slot_of_pos[p] of the caller's scratch buffer. */
int gsr_debug_slot_views(const void* binning_state, int32_t image_width, int32_t image_height, int64_t num_rendered,
                         const uint32_t** slot_of_pos);
/* Pair evaluations of the compositing forward (SURVEY.md 8(d) "FLOP model"): pairs[2*H*W] (uint32) = per pixel, the number of
 * list entries evaluated while the pixel was still compositing [0, H*W) and the number of entries it blended [H*W, 2*H*W),
 * counted by an instrumented build of the forward kernel on the state buffers of a finished forward.  (The backward's count is
 * the sum of n_contrib: it replays entries 1..n_contrib.) */
int gsr_debug_count_pairs(const gsr_settings* s, int32_t P, const void* geometry_state, const void* binning_state,
                          int64_t num_rendered, uint32_t* pairs, void* stream);
/* test / measurement hook: the library's stable LSD radix sort (sort_scan.hip) on caller-provided ping-pong buffers: keys k0
 * (input) / k1, values v0 / v1 (vals_iota != 0: value = index, v0 is not read), optional second payload w0 / w1 (both or
 * neither), key bits [0, bits); n_dev: optional device pointer to a 64-bit count (the kernels then sort min(*n_dev, n) keys).
 * tmp: gsr_debug_radix_tmp_bytes(n) bytes.  Returns 0 / 1 = the buffer set holding the result, or an error code. */
size_t gsr_debug_radix_tmp_bytes(int64_t n);
int gsr_debug_radix_sort(uint32_t* k0, uint32_t* v0, uint32_t* k1, uint32_t* v1, uint32_t* w0, uint32_t* w1, int64_t n,
                         int32_t bits, int32_t vals_iota, const uint32_t* n_dev, void* tmp, void* stream);
/* test hook: the library's prefix sum (sort_scan.hip): out[i] = sum of src[idx ? idx[j] : j] over j < i (inclusive != 0: j <= i),
 * modulo 2^32.  idx may be NULL; out may be src when idx is NULL.  tmp: gsr_debug_scan_tmp_bytes(n) bytes. */
size_t gsr_debug_scan_tmp_bytes(int64_t n);
int gsr_debug_scan_u32(const uint32_t* src, const uint32_t* idx, uint32_t* out, int64_t n, int32_t inclusive, void* tmp,
                       void* stream);
/* test hook: the same sort in the form the tile-local binning runs it (the digit histograms counted ahead of the passes, every
 * pass clearing the next one's look-back table, the last pass leaving tile ranges instead of sorted keys).  Arguments as for
 * gsr_debug_radix_sort, bits <= 24.  EVERY KEY MUST BE BELOW 2^bits (a tile id): the last pass indexes ranges_enc by the whole
 * key, so a larger key writes out of bounds; the hook cannot check this.  tmp may hold anything (only the first pass's look-back
 * table is cleared ahead of the passes, as in a frame).  ranges_enc: 2^bits pairs of uint32, zeroed by the caller; on return pair t holds
 * (~first sorted position, last sorted position + 1) of key value t, (0, 0) where t does not occur.  The key buffer holding the
 * result is NOT written by the last pass. */
int gsr_debug_tile_sort(uint32_t* k0, uint32_t* v0, uint32_t* k1, uint32_t* v1, uint32_t* w0, uint32_t* w1, int64_t n,
                        int32_t bits, int32_t vals_iota, const uint32_t* n_dev, uint32_t* ranges_enc, void* tmp, void* stream);
/* test hook: the tile-local binning's per-tile ordering (binning.hip k_tile_depth_sort) on caller-made lists.  ranges: `tiles`
 * pairs [start, end) into point_list; with ranges_enc (pairs as gsr_debug_tile_sort leaves them) `ranges` is output only.  Every
 * list is ordered by (depth_key[id], position in the list), id 0xFFFFFFFF counting as key 0xFFFFFFFF; dual != 0: slot_of_pos is
 * permuted along.  free_a / free_b / free_c: scratch as long as point_list; meta: 8 words, meta[4] receives (by maximum) the
 * longest list beyond 2048 entries. */
int gsr_debug_tile_depth_sort(int32_t tiles, int32_t dual, uint32_t* ranges, const uint32_t* ranges_enc, uint32_t* point_list,
                              uint32_t* slot_of_pos, const uint32_t* depth_key, uint32_t* free_a, uint32_t* free_b,
                              uint32_t* free_c, uint32_t* meta, void* stream);
int gsr_debug_image_views(const void* image_state, int32_t image_width, int32_t image_height,
                          const float** final_T, const uint32_t** n_contrib);
/* The walk classes a forward with a backward to follow leaves in the image state (ABI 7): walk_cnt[classes] = tiles per class,
 * walk_list[classes][tiles] = the tiles of each class in the order their compositing workgroups finished, walk_of_tile[tiles] = the
 * deepest contributor of any pixel of the tile = the number of list entries its backward walks; class = exponent and two leading
 * mantissa bits of that number (walks below 4: the number itself; clamped at 65535).  k_render_bwd_tile takes the classes
 * longest first (GSR_BWD_LPT=0: index order).  Returns the number of classes (64). */
/* From how many tile instances on a frame's per-instance gradient records carry validity flags (one byte per emission slot behind
 * the records of the backward's scratch buffer: an instance behind its tile's walk gets no all-zero record, and the projection
 * backward reads none).  Default 2 500 000 (smaller frames keep the zero records: there the flags are one more link in a
 * latency-bound kernel).  Tests force either form: 0 = always, 2^32 - 1 = never; negative: only report.  Returns the previous value. */
int64_t gsr_debug_set_flags_min_r(int64_t min_instances);
int gsr_debug_walk_views(const void* image_state, int32_t image_width, int32_t image_height, const uint32_t** walk_cnt,
                         const uint32_t** walk_list, const uint32_t** walk_of_tile);

/* ---- callers of the hot path that the reference also takes from native modules ---- */

/* Fused SSIM map, 11x11 Gaussian window sigma 1.5, zero "same" padding (what reference utils/loss_utils.py:100-159
 * computes; serves `_C.fusedssim` of utils/loss_utils.py:16-38 and `fused_ssim.fused_ssim` of train.py:31-35,116-117).
 * img*, maps: [planes,H,W].  The three dm_* maps (all NULL or all non-NULL) are what the backward needs. */
int gsr_fused_ssim_forward(int32_t planes, int32_t H, int32_t W, float C1, float C2, const float* img1,
                           const float* img2, float* ssim_map, float* dm_dmu1, float* dm_dsigma1_sq,
                           float* dm_dsigma12, void* stream);
int gsr_fused_ssim_backward(int32_t planes, int32_t H, int32_t W, const float* img1, const float* img2,
                            const float* dL_dmap, const float* dm_dmu1, const float* dm_dsigma1_sq,
                            const float* dm_dsigma12, float* dL_dimg1, void* stream);

/* Fused training loss of reference train.py:114-121, (1-l)*mean|a-b| + l*(1-mean(ssim)) (SURVEY.md 8(f) f3 "Fused L1 + SSIM
 * loss"): forward writes the dm_* maps and per-block partial sums partials[2*gsr_fused_loss_blocks()] = (sum ssim, sum |a-b|);
 * a one-workgroup finalize adds them in a fixed order into the device scalar `loss`; backward reads dL/dloss from the device. */
int64_t gsr_fused_loss_blocks(int32_t planes, int32_t H, int32_t W);
int gsr_fused_l1_ssim_forward(int32_t planes, int32_t H, int32_t W, float C1, float C2, float lambda_dssim,
                              const float* img1, const float* img2, float* dm_dmu1, float* dm_dsigma1_sq,
                              float* dm_dsigma12, float* partials, float* loss /*device scalar*/, void* stream);
int gsr_fused_l1_ssim_backward(int32_t planes, int32_t H, int32_t W, float lambda_dssim, const float* img1,
                               const float* img2, const float* upstream /*device scalar dL/dloss or NULL*/,
                               const float* dm_dmu1, const float* dm_dsigma1_sq, const float* dm_dsigma12,
                               float* dL_dimg1, void* stream);

/* weight * mean|(a - b) mask| over n floats and its gradient w.r.t. a: the inverse-depth regularisation term of a training
 * step (reference train.py:124-132, `Ll1depth`; `mask` = depth_mask, may be NULL), three launches instead of torch's dozen.
 * a, b, mask 16-byte aligned; partials: gsr_l1_mean_blocks() floats of scratch; out / upstream: DEVICE scalars (upstream NULL
 * = 1).  Deterministic. */
int32_t gsr_l1_mean_blocks(void);
int gsr_l1_mean_forward(int64_t n, float weight, const float* a, const float* b, const float* mask, float* partials, float* out,
                        void* stream);
int gsr_l1_mean_backward(int64_t n, float weight, const float* a, const float* b, const float* mask, const float* upstream,
                         float* grad, void* stream);

/* One-launch Adam over up to 8 tensors.  Dense = torch.optim.Adam semantics (reference scene/gaussian_model.py:169-170
 * default optimizer); sparse = `SparseGaussianAdam.step(visibility, N)` (reference train.py:37-41,173-176): rows of
 * invisible Gaussians untouched, no bias correction.  Array arguments are HOST arrays of `count` entries; betas / eps are
 * doubles so that 1-beta is formed in double like torch does (1.f-0.999f is off by 1.3e-5 relative). */
int gsr_adam_step(int32_t count, float* const* params, const float* const* grads, float* const* exp_avg,
                  float* const* exp_avg_sq, const int64_t* numel, const float* lr, const int64_t* step, double beta1,
                  double beta2, double eps, void* stream);
int gsr_sparse_adam_step(int32_t count, float* const* params, const float* const* grads, float* const* exp_avg,
                         float* const* exp_avg_sq, const int64_t* numel, const float* lr, int64_t N,
                         const uint8_t* visible, double beta1, double beta2, double eps, void* stream);

/* GaussianModel.densify_and_prune (reference scene/gaussian_model.py:367-429 + optimizer surgery :274-344) as two passes.
 * plan: decides keep / clone / split per Gaussian with the reference's predicates (NaN grads -> 0; clone: small & grad >= thr;
 * split: large & grad >= thr; prune: sigmoid(opacity) < min_opacity, or world size > 0.1*extent when use_world_size_prune),
 * runs the prefix sums, and returns counts_host[3] = {kept originals, clones, split sources} (one stream sync).
 * apply: writes the new arrays in the reference's order [kept originals][clones][children copy 0][children copy 1];
 * in_ptrs / out_ptrs are HOST arrays of 18 device pointers: (xyz, f_dc, f_rest, opacity, scaling, rotation) x
 * (value, exp_avg, exp_avg_sq); moments may be NULL.  New size = keep + clone + 2*child. */
/* add_densification_stats (reference scene/gaussian_model.py:431-433) + max_radii2D update (train.py:159), one pass:
 * where radii > 0: accum += ||grad_means2D.xy||, denom += 1, max_radii2D = max(max_radii2D, radii). */
int gsr_densification_stats(int64_t P, const float* grad_means2D, const int32_t* radii, float* xyz_gradient_accum,
                            float* denom, float* max_radii2D, void* stream);
size_t gsr_densify_workspace_bytes(int64_t P);
int gsr_densify_plan(int64_t P, const float* xyz_gradient_accum, const float* denom, const float* scaling_raw,
                     const float* opacity_raw, float max_grad, float min_opacity, float extent, float percent_dense,
                     int32_t use_world_size_prune, void* workspace, size_t workspace_bytes, int64_t* counts_host,
                     void* stream);
int gsr_densify_apply(int64_t P, const void* workspace, const float* const* in_ptrs, float* const* out_ptrs,
                      const int32_t* row_floats, int64_t n_keep, int64_t n_clone, int64_t n_child, uint32_t seed,
                      int32_t* source_of_row, void* stream);

/* The model's parameter activations, fused (reference scene/gaussian_model.py:38-46 setup_functions, :101-121 getters):
 * scaling = exp(_scaling) [P,3], rotation = normalize(_rotation) = x / max(|x|, 1e-12) [P,4], opacity = sigmoid(_opacity)
 * [P,1]; what render() reads through pc.get_scaling / get_rotation / get_opacity (gaussian_renderer/__init__.py:55-62).
 * One launch each way instead of ~25 elementwise / reduce launches per training step.
 * backward: dL_d* of the three outputs (any may be NULL = zero) -> gradients of the raw parameters (always written). */
int gsr_gaussian_activations_forward(int32_t P, const float* raw_scaling, const float* raw_rotation,
                                     const float* raw_opacity, float* scaling, float* rotation, float* opacity,
                                     void* stream);
int gsr_gaussian_activations_backward(int32_t P, const float* raw_rotation, const float* scaling, const float* opacity,
                                      const float* dL_dscaling, const float* dL_drotation, const float* dL_dopacity,
                                      float* dL_draw_scaling, float* dL_draw_rotation, float* dL_draw_opacity,
                                      void* stream);

/* View-sharded data parallelism (the reference itself is single-GPU): with ONE view per rank per step the SH
 * gradient of a rank is rank one per Gaussian, dL/dsh[k][c] = basis_k(dir) * dL/drgb_c, and dL/df_dc = C0 * dL/drgb carries it
 * whole.  The ranks all-gather `gathered`[n_ranks][P + 1][3]: rows 0..P-1 = that rank's dL/df_dc, row P = its camera centre
 * (12 B per Gaussian and rank instead of 192 B all-reduced), and this call rebuilds the MEAN gradients of f_dc [P, 1, 3] and
 * f_rest [P, sh_coeffs_rest, 3] (scale = 1 / n_ranks), summing the ranks in order: identical bits on every rank.  `means3D` are
 * the positions the forwards saw.  Coefficients beyond the active degree get zeros. */
int gsr_sh_rank1_expand(int32_t P, int32_t n_ranks, int32_t sh_degree, int32_t sh_coeffs_rest, const float* means3D,
                        const float* gathered, float scale, float* dL_ddc_mean, float* dL_dsh_rest_mean, void* stream);
/* gsr_sh_rank1_expand followed by the dense Adam update (torch.optim.Adam semantics) of f_dc and f_rest, in ONE kernel: the
 * rebuilt gradients are never written to memory.  `opt`: groups 1 (f_dc) and 2 (f_rest) of a gsr_fused_adam are used (moments,
 * lr, 1-based step AFTER this update; sparse must be 0).  Bit-identical to gsr_sh_rank1_expand + gsr_adam_step on those tensors. */
int gsr_sh_rank1_adam(int32_t P, int32_t n_ranks, int32_t sh_degree, int32_t sh_coeffs_rest, const float* means3D,
                      const float* gathered, float scale, float* f_dc, float* f_rest, const gsr_fused_adam* opt, void* stream);

/* ---- mapping: seeding Gaussians from point clouds and RGB-D keyframes ---- */

/* What the reference takes from `simple_knn._C.distCUDA2` (scene/gaussian_model.py:20,:140; the fourth native module it imports):
 * mean_dist2[i - first_query] = mean of the three smallest squared Euclidean distances from point i to the OTHER points of the
 * whole set (other = a different index: a duplicate at distance 0 counts), for first_query <= i < P.  first_query = 0 is distCUDA2;
 * first_query > 0 is the keyframe case - neighbours are searched in map + new points, answers only for the new ones - and gives
 * the tail of the first_query = 0 result bit for bit.  EXACT nearest neighbours (Morton order + two levels of boxes that only
 * prune, csrc/knn.hip); distances are formed from differences, never as |a|^2 + |b|^2 - 2 a.b.  No float atomics, nothing depends on
 * scheduling: two runs give identical bits.  No device allocation: everything lives in `workspace` (gsr_knn_workspace_bytes(P)).
 * Fewer than four points: the mean runs over the min(3, P - 1) neighbours that exist, P == 1 gives 0.  (The upstream module is
 * recalled to leave FLT_MAX-derived values there; nothing in the reference pins either behaviour.)  Non-finite coordinates: no hang
 * and no out-of-bounds access; the values of those rows (and of rows whose neighbours they would be) are unspecified.
 * Errors, all before anything is launched: P <= 0 or > 2^30 - 1, NULL pointers, first_query outside [0, P):
 * GSR_ERR_INVALID_ARGUMENT; workspace_bytes too small: GSR_ERR_STATE_TOO_SMALL. */
size_t gsr_knn_workspace_bytes(int64_t P);
int gsr_knn_dist2(int64_t P, const float* points /*[P,3]*/, int64_t first_query, float* mean_dist2 /*[P - first_query]*/,
                  void* workspace, size_t workspace_bytes, void* stream);

/* The same exact search for k = 1 .. GSR_KNN_K_MAX neighbours, every row a query, answers in ORIGINAL row order.  With
 * k_eff = min(k, P - 1):
 *   dist2_out[i, 0 .. k_eff)  the k_eff smallest squared distances from row i to the OTHER rows, ascending (the same float32
 *                             rounding sequence as gsr_knn_dist2: k = 3 gives the three values whose mean gsr_knn_dist2 returns);
 *   dist2_out[i, k_eff .. k)  +inf;
 *   mean_dist_out[i]          (sum of the square roots of those k_eff values) / (k_eff + 1): root and sum in float64 inside the
 *                             kernel, rounded to float32 once.  The divisor counts the point itself at distance 0 - the average
 *                             a statistical outlier filter takes over a neighbour search that returns the query too.  P == 1: 0.
 * Either output may be NULL, not both.  A row with a non-finite coordinate gets +inf distances and a NaN mean and is nobody's
 * neighbour.  Deterministic, no float atomics, no allocation (gsr_knn_k_workspace_bytes(P)).
 * Errors before any launch: k outside [1, GSR_KNN_K_MAX], P <= 0 or > 2^30 - 1, NULL points / workspace, both outputs NULL:
 * GSR_ERR_INVALID_ARGUMENT; workspace too small: GSR_ERR_STATE_TOO_SMALL. */
#define GSR_KNN_K_MAX 32
size_t gsr_knn_k_workspace_bytes(int64_t P);
int gsr_knn_k(int64_t P, const float* points /*[P,3]*/, int32_t k, float* dist2_out /*[P,k] or NULL*/,
              float* mean_dist_out /*[P] or NULL*/, void* workspace, size_t workspace_bytes, void* stream);

/* ---- point-cloud conditioning: voxel-grid down-sampling, statistical outlier filter (csrc/pointcloud.hip; DESIGN.md section 4
 * item 29) - what the reference's process_point_cloud does with Open3D before a cloud reaches create_from_pcd ---- */

/* One averaged point per occupied voxel.  Lattice: per axis o_a = origin[a] (`origin`: HOST float[3]) or, with origin == NULL,
 * o_a = min_a - 0.5 voxel_size (min_a: the smallest finite coordinate); cell index i_a = floor((p_a - o_a) / voxel_size) - one
 * correctly rounded float32 operation each (subtract, divide, floor; 0.5 voxel_size is a float32 product), so a float32
 * restatement assigns every point to the same voxel bit for bit.  Rows with a non-finite coordinate are dropped.  An index outside
 * [-2^20, 2^20) on any axis sets count_dev[1] (status) non-zero and the other outputs are then meaningless.
 * Output rows in ascending (i_z, i_y, i_x): mean position, mean colour (`colors` and `out_colors` both given, else neither is
 * touched), `out_npts` (NULL: not wanted) the number of points of the voxel.  Sums in float64 in an order that depends on the
 * sorted position only (the stable sort keeps a voxel's points in row order), mean formed in float64, rounded to float32 once.
 * count_dev[0] = number of voxels (device int64; it may exceed `capacity`: rows beyond `capacity` are never written).
 * Deterministic, no float atomics, no allocation (gsr_voxel_workspace_bytes(P)).
 * Errors before any launch: voxel_size <= 0 or not finite, a non-finite origin, P <= 0 or > 2^30 - 1, capacity < 0, NULL points /
 * count_dev / workspace, out_points NULL with capacity > 0, colors without out_colors (capacity > 0): GSR_ERR_INVALID_ARGUMENT;
 * workspace too small: GSR_ERR_STATE_TOO_SMALL. */
size_t gsr_voxel_workspace_bytes(int64_t P);
int gsr_voxel_down_sample(int64_t P, const float* points /*[P,3]*/, const float* colors /*[P,3] or NULL*/, float voxel_size,
                          const float* origin /*HOST [3] or NULL*/, float* out_points /*[capacity,3]*/,
                          float* out_colors /*[capacity,3] or NULL*/, int32_t* out_npts /*[capacity] or NULL*/, int64_t capacity,
                          int64_t* count_dev /*[2]: voxels, status*/, void* workspace, size_t workspace_bytes, void* stream);

/* Statistical outlier filter.  dbar_i = mean_dist_out of gsr_knn_k with k = nb_neighbors - 1 (nb_neighbors in [2, 33] counts the
 * point itself); mu = mean of dbar over the n_valid rows whose dbar is finite (rows with a non-finite coordinate are not);
 * sigma = sqrt(sum (dbar_i - mu)^2 / (n_valid - 1)), 0 with n_valid < 2; threshold = mu + std_ratio sigma - float64, from
 * fixed-order per-workgroup partial sums and one final workgroup, never on the host.  keep[i] = dbar_i > 0 && dbar_i < threshold
 * (0 for the non-finite rows).  stats_dev (device double[4], or NULL) = n_valid, mu, sigma, threshold; mean_dist (device
 * float[P], or NULL) = dbar.  Errors before any launch: nb_neighbors outside [2, 33], std_ratio not finite, P <= 0 or > 2^30 - 1,
 * NULL points / keep / workspace: GSR_ERR_INVALID_ARGUMENT; workspace too small: GSR_ERR_STATE_TOO_SMALL. */
size_t gsr_outlier_workspace_bytes(int64_t P);
int gsr_statistical_outliers(int64_t P, const float* points /*[P,3]*/, int32_t nb_neighbors, double std_ratio,
                             uint8_t* keep /*[P]*/, float* mean_dist /*[P] or NULL*/, double* stats_dev /*[4] or NULL*/,
                             void* workspace, size_t workspace_bytes, void* stream);

/* ---- registration of one cloud to another: nearest-neighbour index, point-to-point ICP (csrc/registration.hip; DESIGN.md
 * section 4 item 30) - what the reference's pointcloud_registeration does with Open3D before it merges two clouds ---- */

/* The transformed point every entry below means by "q = T s": with T a row-major 4 x 4 in DEVICE float64 (NULL: the identity),
 *   q_i = (float)(((T[i,0] s_x + T[i,1] s_y) + T[i,2] s_z) + T[i,3]),   i = 0, 1, 2
 * - every product and every sum one correctly rounded float64 operation (no fused multiply-add), in exactly this order, then ONE
 * rounding to float32.  A float64 restatement that keeps the order gives the same bits.  Row 3 of T is never read. */

/* Index over a target cloud, built once and searched many times (the target of a registration does not move).  `index`: caller's
 * device memory of gsr_nn_index_bytes(Pt) bytes, 256-byte aligned; opaque - the points in Morton order as float4 (xyz, original
 * row), the AABBs of 64-point boxes and of 64-box super-boxes, the bounding box of the finite coordinates and its centre, then
 * the build's scratch.  A row with a non-finite coordinate is never anybody's neighbour.  Deterministic, no allocation.
 * Errors before any launch: Pt outside [1, 2^30 - 1], NULL target / index: GSR_ERR_INVALID_ARGUMENT; index_bytes too small:
 * GSR_ERR_STATE_TOO_SMALL. */
size_t gsr_nn_index_bytes(int64_t Pt);
int gsr_nn_index_build(int64_t Pt, const float* target /*[Pt,3]*/, void* index, size_t index_bytes, void* stream);

/* Exact nearest neighbour in the indexed target of every q = T s, s a row of `source`, answers in ORIGINAL row order.  Distances
 * are the float32 values of gsr_knn_k (differences, then fma(dz,dz, fma(dy,dy, dx*dx))).  The answer of a row is the
 * lexicographic minimum of (d2, target row) over the finite target rows: among equal float32 distances the smallest row wins,
 * so the row as well as the distance is independent of the traversal - two runs, any permutation of the source rows and any
 * `order` give the same bits.  A correspondence is valid iff d2 <= max_dist2 (+inf allowed; it also is the initial pruning
 * bound); otherwise, and for a source row whose q is not finite, idx_out = -1 and dist2_out = +inf.
 * order (device int32[Ps], or NULL): a permutation of the source rows; thread t answers row order[t], so that the lanes of a
 * wave can be given neighbouring queries (gsr_nn_query_order).  It changes no output bit.  Entries outside [0, Ps) are skipped.
 * Errors before the launch: Pt / Ps outside [1, 2^30 - 1], NULL index / source / idx_out, max_dist2 negative or NaN:
 * GSR_ERR_INVALID_ARGUMENT.  (The index is not sized here: it must be the one gsr_nn_index_build filled for this Pt.) */
int gsr_nn_search(int64_t Pt, const void* index, int64_t Ps, const float* source /*[Ps,3]*/,
                  const double* T_dev /*[16] row-major, or NULL*/, float max_dist2, const int32_t* order /*[Ps] or NULL*/,
                  int32_t* idx_out /*[Ps]*/, float* dist2_out /*[Ps] or NULL*/, void* stream);

/* order_out[Ps]: the source rows sorted (stably) by the 30-bit Morton code of q = T s in the index's bounding box - queries outside
 * the box fall into the cells of its faces.  Errors before any launch: sizes outside [1, 2^30 - 1], NULL index / source /
 * order_out / workspace: GSR_ERR_INVALID_ARGUMENT; workspace below gsr_nn_order_workspace_bytes(Ps): GSR_ERR_STATE_TOO_SMALL. */
size_t gsr_nn_order_workspace_bytes(int64_t Ps);
int gsr_nn_query_order(int64_t Pt, const void* index, int64_t Ps, const float* source /*[Ps,3]*/,
                       const double* T_dev /*[16] or NULL*/, int32_t* order_out /*[Ps]*/, void* workspace, size_t workspace_bytes,
                       void* stream);

/* out[i] = q = T points[i] as defined above (what a registration applies to the full-resolution cloud once it has T).  `out` may
 * be `points`.  Errors before the launch: P outside [1, 2^30 - 1], NULL points / out: GSR_ERR_INVALID_ARGUMENT. */
int gsr_transform_points(int64_t P, const float* points /*[P,3]*/, const double* T_dev /*[16] or NULL*/, float* out /*[P,3]*/,
                         void* stream);

/* One point-to-point ICP update on the device.  Row i takes part iff 0 <= idx[i] < Pt and both q_i = T s_i and
 * p_i = target[idx[i]] are finite.  Over those n rows, in float64, about a shift taken from the target (a cloud far from the
 * origin loses nothing): sum |q - p|^2, sum q, sum p, sum q p^T - at most 256 workgroups over fixed slices, a fixed butterfly
 * inside the wave, wave and workgroup sums added in order, no float atomics: deterministic.  One thread then finds the rigid dT
 * (no scale) that minimises sum |dT q - p|^2 by Horn's closed form - the rotation is the unit eigenvector of the largest
 * eigenvalue of the symmetric 4 x 4 matrix of the centred cross-covariance, found by cyclic Jacobi with a fixed number of sweeps
 * and normalised again before the matrix is formed, so dT is a proper rotation whatever the data (a planar cloud too) - and
 * stores T <- dT T (row 3 = 0 0 0 1).
 * stats_dev[8] = n, fitness = n / Ps, inlier_rmse = sqrt(sum |q - p|^2 / n) (0 with n = 0), status, sum |q - p|^2, the largest
 * eigenvalue, 0, 0.  n, fitness and inlier_rmse describe the INCOMING T (Open3D's convention: the correspondence set of the
 * search that produced idx).  status: 0 = T updated; 1 = n < 3, T unchanged; 2 = no usable eigenvector (sums not finite), T
 * unchanged.  Errors before any launch: sizes outside [1, 2^30 - 1], NULL source / target / idx / T_dev / stats_dev / workspace:
 * GSR_ERR_INVALID_ARGUMENT; workspace below gsr_icp_workspace_bytes(Ps): GSR_ERR_STATE_TOO_SMALL.  No allocation.
 * gsr_icp_workspace_bytes serves gsr_icp_update_plane too and grew with it (30 partial sums per workgroup instead of 17: 61 696
 * bytes, was 35 072); BOTH entries check against it, so a caller must ask the query and not keep the earlier figure. */
size_t gsr_icp_workspace_bytes(int64_t Ps);
int gsr_icp_update(int64_t Ps, const float* source /*[Ps,3]*/, int64_t Pt, const float* target /*[Pt,3]*/,
                   const int32_t* idx /*[Ps]*/, double* T_dev /*[16] in/out*/, double* stats_dev /*[8] out*/, void* workspace,
                   size_t workspace_bytes, void* stream);

/* One point-to-plane ICP update on the device: gsr_icp_update with the residual r_i = (q_i - p_i).n_i, n_i =
 * target_normals[idx[i]].  Row i takes part iff 0 <= idx[i] < Pt and q_i = T s_i, p_i = target[idx[i]] and n_i are all finite.
 * Everything is formed about the shift c of gsr_icp_update (the target point of the first row whose q and p are finite): with
 * q' = q - c and p' = p - c, r_i = (q'_i - p'_i).n_i and J_i = [q'_i x n_i, n_i].  Over the n rows, in float64 and with the
 * summation structure of gsr_icp_update (deterministic, no float atomics): the 21 entries of the upper triangle of J^T J, the 6
 * of J^T r, n, sum |q - p|^2 and sum r^2.  One thread solves J^T J x = -J^T r by LDL^T; x = (alpha, beta, gamma, t),
 * dR = Rz(gamma) Ry(beta) Rx(alpha) (what Open3D's TransformVector6dToMatrix4d forms: a product of exact rotations),
 * dT = Tr(c) [dR, t] Tr(-c), and T <- dT T (row 3 = 0 0 0 1).
 * stats_dev[8] = n, fitness = n / Ps, inlier_rmse = sqrt(sum |q - p|^2 / n) (the Euclidean one, Open3D's convention for every
 * estimator; 0 with n = 0), status, sum |q - p|^2, sum r^2, 0, 0 - all of the INCOMING T.  status: 0 = T updated; 1 = n < 6, T
 * unchanged; 2 = a pivot of the factorisation is not finite or is <= 1e-12 x its own diagonal entry of J^T J (the planes met do
 * not fix that unknown - a single plane, say - or sums overflowed), T unchanged.
 * Errors before any launch: sizes outside [1, 2^30 - 1], NULL source / target / target_normals / idx / T_dev / stats_dev /
 * workspace: GSR_ERR_INVALID_ARGUMENT; workspace below gsr_icp_workspace_bytes(Ps): GSR_ERR_STATE_TOO_SMALL.  No allocation. */
int gsr_icp_update_plane(int64_t Ps, const float* source /*[Ps,3]*/, int64_t Pt, const float* target /*[Pt,3]*/,
                         const float* target_normals /*[Pt,3]*/, const int32_t* idx /*[Ps]*/, double* T_dev /*[16] in/out*/,
                         double* stats_dev /*[8] out*/, void* workspace, size_t workspace_bytes, void* stream);

/* ---- surface normals (csrc/normals.hip) - what the reference takes from Open3D's
 * estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)) ---- */

/* Normal of every row from the covariance of a hybrid neighbourhood, defined so that nothing depends on traversal or scheduling.
 * d2(i,j): the float32 squared distance of gsr_knn_k.  k = max_nn - 1 (max_nn in [3, GSR_KNN_K_MAX + 1] counts the point itself);
 * d_k = the k-th smallest d2 from row i to the OTHER finite rows, +inf if fewer than k exist; bound = min(r2, d_k), r2 the float32
 * square of `radius` (> 0; +inf: count-limited only).  N_i = {i} + {j != i : d2(i,j) <= bound}: rows tied at the bound are ALL
 * members, so count_i = |N_i| may exceed max_nn at exact ties - the one departure from Open3D's hybrid search; duplicates at
 * distance 0 are members.
 * delta_j = p_j - p_i per component in float32, promoted; S1 = sum delta, S2 = sum delta delta^T in float64 in the order of the
 * sorted structure (fixed for a given input: two runs give identical bits); C = S2 / n - (S1 / n)(S1 / n)^T, n = count_i.
 * Eigen-solve: cyclic Jacobi on the symmetric 3 x 3 in float64, a fixed number of sweeps.  eigenvalues_out: ascending.  The normal
 * is the unit eigenvector of the smallest eigenvalue, normalised again in float64, rounded to float32 once.
 * Sign: with `viewpoint` v (HOST float[3]) n.(v - p_i) >= 0 (Open3D's orient_normals_towards_camera_location); with NULL the
 * component of largest magnitude (the first on ties) is positive.
 * count_i < 3: n = (0, 0, 1) - whatever the viewpoint - and eigenvalues 0 (Open3D's fallback).  A row with a non-finite
 * coordinate gets a NaN normal, NaN eigenvalues and count 0, and is nobody's neighbour.
 * No float atomics, no allocation (gsr_normals_workspace_bytes(P)).  Errors before any launch: max_nn outside [3, 33], radius
 * <= 0 or NaN, a non-finite viewpoint, P outside [1, 2^30 - 1], NULL points / normals / workspace: GSR_ERR_INVALID_ARGUMENT;
 * workspace too small: GSR_ERR_STATE_TOO_SMALL. */
size_t gsr_normals_workspace_bytes(int64_t P);
int gsr_estimate_normals(int64_t P, const float* points /*[P,3]*/, float radius, int32_t max_nn,
                         const float* viewpoint /*HOST [3] or NULL*/, float* normals /*[P,3]*/, int32_t* count_out /*[P] or NULL*/,
                         float* eigenvalues_out /*[P,3] ascending, or NULL*/, void* workspace, size_t workspace_bytes,
                         void* stream);

/* ---- generalized ICP (csrc/gicp.hip) - Segal, Haehnel, Thrun 2009 as Open3D's
 * registration_generalized_icp states it: a covariance per point on BOTH clouds, and updates that weigh every pair by the inverse of
 * the combined covariance.  A covariance is six float32 per row: xx, xy, xz, yy, yz, zz (the layout of cov3D_precomp).  Every
 * result is a function of the input only, never of traversal, scheduling or launch shape; no float atomics, no allocation. ---- */

/* The regularised covariance of a symmetric 3 x 3 matrix A (float64) with epsilon in (0, 1] - R(A, epsilon) below:
 * cyclic Jacobi on A in float64, the rotations and the fixed number of sweeps of gsr_estimate_normals, in its order (0,1), (0,2),
 * (1,2).  With a00, a11, a22 the diagonal after the sweeps: if a00 == a11 && a11 == a22 (float64 equality; a multiple of the
 * identity meets it exactly, since a zero off-diagonal entry is never rotated) the result is I.  Otherwise w = the column of the
 * eigenvector matrix that belongs to the smallest of the three (the first on ties), divided by sqrt((wx wx + wy wy) + wz wz), k = 1
 * - epsilon, and
 *   xx = 1 - (k wx) wx,  xy = 0 - (k wx) wy,  xz = 0 - (k wx) wz,  yy = 1 - (k wy) wy,  yz = 0 - (k wy) wz,  zz = 1 - (k wz) wz
 * - every product and difference one float64 operation, in this order, no fused multiply-add, each entry rounded to float32 once.
 * That is I - (1 - epsilon) w w^T = V diag(epsilon, 1, 1) V^T, Open3D's regularisation (the surface is flat along its normal and
 * of unit extent across it); w enters as a square, so no sign rule is needed. */

/* Covariance of every row from its hybrid neighbourhood.  Neighbourhood: N_i of gsr_estimate_normals exactly (float32 d2, k =
 * max_nn - 1, bound = min(r2, d_k), rows tied at the bound all belong - the departure from Open3D's hybrid search inherited from
 * there - duplicates are members; a row with a non-finite coordinate is masked and is nobody's neighbour), max_nn in [3,
 * GSR_KNN_K_MAX + 1].  S1, S2 and C = S2 / n - (S1 / n)(S1 / n)^T as gsr_estimate_normals forms them (float64, the order of the
 * sorted structure: two runs give identical bits).  cov_out[i] = R(C, epsilon); count_i < 3: I (that row then pulls as a
 * point-to-point pair does); a non-finite row: six NaN and count 0.  count_out = |N_i|.  One launch after the index build.
 * Errors before any launch: P outside [1, 2^30 - 1], NULL points / cov_out / workspace, radius <= 0 or NaN, max_nn outside [3, 33],
 * epsilon outside (0, 1] or NaN: GSR_ERR_INVALID_ARGUMENT; workspace below gsr_covariance_workspace_bytes(P):
 * GSR_ERR_STATE_TOO_SMALL. */
size_t gsr_covariance_workspace_bytes(int64_t P);
int gsr_estimate_covariances(int64_t P, const float* points /*[P,3]*/, float radius, int32_t max_nn, double epsilon,
                             float* cov_out /*[P,6]*/, int32_t* count_out /*[P] or NULL*/, void* workspace, size_t workspace_bytes,
                             void* stream);

/* cov_out[i] = R(A_i, epsilon) of covariances that are GIVEN (a Gaussian map's own), A_i the float32 entries of cov_in[i] promoted:
 * their shape is kept - the direction of least extent - and their size replaced by (epsilon, 1, 1).  A row with a non-finite entry:
 * six NaN.  One thread per row, no workspace; cov_out may be cov_in.  Errors before the launch: P outside [1, 2^30 - 1], NULL
 * cov_in / cov_out, epsilon outside (0, 1] or NaN: GSR_ERR_INVALID_ARGUMENT. */
int gsr_regularize_covariances(int64_t P, const float* cov_in /*[P,6]*/, double epsilon, float* cov_out /*[P,6]*/, void* stream);

/* One generalized ICP update on the device: gsr_icp_update_plane with the residual d_i = q_i - p_i (three components) weighted by
 * W_i = M_i^-1.  With k = idx[i] and R the rotation block of the INCOMING T: row i takes part iff 0 <= k < Pt, q = T s_i and p =
 * target[k] are finite, the six entries of source_cov[i] and of target_cov[k] are finite, and det M (below) is finite and > 0.
 * Everything is formed about the shift c of gsr_icp_update (the target point of the first row whose q and p are finite - the
 * covariances play no part in it), q' = q - c, all in float64, every operation rounded on its own (no fused multiply-add), sums
 * of three terms as (a + b) + c:
 *   A = R Sigma_s:   A[a][b] = (R[a][0] S[0][b] + R[a][1] S[1][b]) + R[a][2] S[2][b]
 *   M = Sigma_t + A R^T, the upper triangle (the lower one is its mirror image):
 *                    M[a][b] = Sigma_t[a][b] + ((A[a][0] R[b][0] + A[a][1] R[b][1]) + A[a][2] R[b][2]),  a <= b
 *   adjugate, M = [m0 m1 m2; m1 m3 m4; m2 m4 m5]:
 *                    k00 = m3 m5 - m4 m4,  k01 = m2 m4 - m1 m5,  k02 = m1 m4 - m2 m3,
 *                    k11 = m0 m5 - m2 m2,  k12 = m1 m2 - m0 m4,  k22 = m0 m3 - m1 m1,   det = (m0 k00 + m1 k01) + m2 k02
 *   W[a][b] = k_ab / det (symmetric);  d = q - p (float32 values promoted, so d = q' - p');
 *   J = [-[q']x, I] (3 x 6: the derivative of dR q' + t - p' at 0):  rows (0, q'z, -q'y, 1, 0, 0), (-q'z, 0, q'x, 0, 1, 0),
 *   (q'y, -q'x, 0, 0, 0, 1).
 * Over the n rows, with the summation structure of gsr_icp_update (at most 256 workgroups over fixed slices, a fixed butterfly, no
 * float atomics: deterministic), 30 sums per workgroup: the 21 entries of the upper triangle of J^T W J, the 6 of J^T W d, n,
 * sum |d|^2 and sum d^T W d.  Solve and composition are the plane update's: J^T W J x = -J^T W d by LDL^T with its pivot rule, x =
 * (alpha, beta, gamma, t), dR = Rz(gamma) Ry(beta) Rx(alpha), dT = Tr(c) [dR, t] Tr(-c), T <- dT T (row 3 = 0 0 0 1).
 * stats_dev[8] = n, fitness = n / Ps, inlier_rmse = sqrt(sum |d|^2 / n) (Euclidean; 0 with n = 0), status, sum |d|^2, sum d^T W d,
 * 0, 0 - all of the INCOMING T.  status: 0 = T updated; 1 = n < 6, T unchanged; 2 = a rejected pivot (gsr_icp_update_plane's rule),
 * T unchanged - with isotropic covariances on one side M is positive definite in every direction and a single plane is solved,
 * where the plane update returns 2.  Covariances are used as given: nothing here regularises them.
 * Errors before any launch: sizes outside [1, 2^30 - 1], a NULL pointer: GSR_ERR_INVALID_ARGUMENT; workspace below
 * gsr_icp_generalized_workspace_bytes(Ps): GSR_ERR_STATE_TOO_SMALL.  No allocation. */
size_t gsr_icp_generalized_workspace_bytes(int64_t Ps);
int gsr_icp_update_generalized(int64_t Ps, const float* source /*[Ps,3]*/, const float* source_cov /*[Ps,6]*/, int64_t Pt,
                               const float* target /*[Pt,3]*/, const float* target_cov /*[Pt,6]*/, const int32_t* idx /*[Ps]*/,
                               double* T_dev /*[16] in/out*/, double* stats_dev /*[8] out*/, void* workspace, size_t workspace_bytes,
                               void* stream);

/* ---- coloured ICP (csrc/colored.hip, csrc/registration.hip) - Park, Zhou, Koltun 2017 as Open3D's
 * registration_colored_icp states it: a colour gradient per target point, then updates that join the point-to-plane residual
 * with a photometric one measured in the target's tangent plane.  Every result is a function of the input only, never of
 * traversal, scheduling or launch shape; no float atomics, no allocation. ---- */

/* Gradient of the intensity I = (((double)r + (double)g) + (double)b) / 3 over the tangent plane of every row.
 * Neighbourhood: N_i of gsr_estimate_normals exactly (float32 d2, k = max_nn - 1, bound = min(r2, d_k), rows tied at the bound
 * all belong - the departure from Open3D's hybrid search inherited from there - duplicates are members), max_nn in
 * [4, GSR_KNN_K_MAX + 1].  A row whose point, normal or colour has a non-finite component is masked before the structure is built
 * (it takes no part in the bounding box, the sort or the boxes, so no other row's bits depend on where it lies): gradient NaN,
 * count 0, status 3, nobody's neighbour.
 * Row i with normal n (taken as given: a unit vector is the caller's to provide) and n_i = |N_i|, all in float64: for every member
 * j != i, in the order of the sorted structure (fixed for a given input: two runs give identical bits), delta = p_j - p_i per
 * component in float32, promoted; u = delta - (delta.n) n with delta.n = (dx nx + dy ny) + dz nz; b = I_j - I_i.  M = sum u u^T
 * (six sums), v = sum u b (three).  Then the constraint row (n_i - 1) n with right-hand side 0 (Open3D's
 * InitializePointCloudForColoredICP): M += (n_i - 1)^2 n n^T.  M g = v is solved by LDL^T, g rounded to float32 once.
 * status_out: 0 = solved; 1 = n_i < 4, gradient 0 (Open3D's rule); 2 = a pivot of the factorisation is not finite or is <= 1e-12 x
 * its own diagonal entry of M (a collinear neighbourhood, say), gradient 0; 3 = masked.  count_out = n_i (0 for a masked row).
 * Errors before any launch: P outside [1, 2^30 - 1], NULL points / colors / normals / gradient / workspace, radius <= 0 or NaN,
 * max_nn outside [4, 33]: GSR_ERR_INVALID_ARGUMENT; workspace below gsr_color_gradient_workspace_bytes(P):
 * GSR_ERR_STATE_TOO_SMALL. */
size_t gsr_color_gradient_workspace_bytes(int64_t P);
int gsr_color_gradient(int64_t P, const float* points /*[P,3]*/, const float* colors /*[P,3]*/, const float* normals /*[P,3]*/,
                       float radius, int32_t max_nn, float* gradient /*[P,3]*/, int32_t* count_out /*[P] or NULL*/,
                       uint8_t* status_out /*[P] or NULL*/, void* workspace, size_t workspace_bytes, void* stream);

/* One coloured ICP update on the device: gsr_icp_update_plane with a second residual per row.  With k = idx[i]: p =
 * target[k], n = target_normals[k], d = target_gradient[k] (gsr_color_gradient of the target), I_s and I_t the intensities (as
 * above) of source_colors[i] and target_colors[k].  Row i takes part iff 0 <= k < Pt and q = T s_i, p, n, d, I_s and I_t are all
 * finite.  Everything is formed about the shift c of gsr_icp_update (the target point of the first row whose q and p are finite),
 * q' = q - c, e = q - p, lambda = lambda_geometric, in float64:
 *   geometric    r_G = sqrt(lambda) (e.n),                       J_G = sqrt(lambda) [q' x n, n];
 *   photometric  q_proj - p = e - (e.n) n,  I_proj = I_t + d.(q_proj - p),  r_I = sqrt(1 - lambda) (I_s - I_proj),
 *                m = -(I - n n^T) d = (d.n) n - d,              J_I = sqrt(1 - lambda) [q' x m, m]
 * (Open3D's TransformationEstimationForColoredICP::ComputeTransformation; its default lambda is 0.968).  Over the n rows, with the
 * summation structure of gsr_icp_update (deterministic, no float atomics), 31 sums per workgroup: the 21 entries of the upper
 * triangle of J^T J and the 6 of J^T r over both residuals, n, sum |q - p|^2, sum (e.n)^2 and sum (I_s - I_proj)^2 - each of the
 * last two 0 where its weight (lambda, 1 - lambda) is 0.  Solve and composition are the plane update's: LDL^T, x = (alpha, beta,
 * gamma, t), dR = Rz(gamma) Ry(beta) Rx(alpha), dT = Tr(c) [dR, t] Tr(-c), T <- dT T (row 3 = 0 0 0 1).
 * stats_dev[8] = n, fitness = n / Ps, inlier_rmse = sqrt(sum |q - p|^2 / n) (Euclidean; 0 with n = 0), status, sum |q - p|^2,
 * sum r_G^2 / lambda, sum r_I^2 / (1 - lambda) (the unweighted residuals), 0 - all of the INCOMING T.  status: 0 = T updated; 1 = n
 * < 6, T unchanged; 2 = a rejected pivot (gsr_icp_update_plane's rule: an untextured single plane, say), T unchanged.
 * The workspace holds one sum more per workgroup than gsr_icp_workspace_bytes provides: it has its own query.
 * Errors before any launch: sizes outside [1, 2^30 - 1], a NULL pointer, lambda_geometric outside [0, 1] or NaN:
 * GSR_ERR_INVALID_ARGUMENT; workspace below gsr_icp_colored_workspace_bytes(Ps): GSR_ERR_STATE_TOO_SMALL.  No allocation. */
size_t gsr_icp_colored_workspace_bytes(int64_t Ps);
int gsr_icp_update_colored(int64_t Ps, const float* source /*[Ps,3]*/, const float* source_colors /*[Ps,3]*/, int64_t Pt,
                           const float* target /*[Pt,3]*/, const float* target_normals /*[Pt,3]*/,
                           const float* target_colors /*[Pt,3]*/, const float* target_gradient /*[Pt,3]*/,
                           const int32_t* idx /*[Ps]*/, double lambda_geometric, double* T_dev /*[16] in/out*/,
                           double* stats_dev /*[8] out*/, void* workspace, size_t workspace_bytes, void* stream);

/* ---- dense RGB-D odometry (csrc/odometry.hip) - the hybrid photometric + depth term of
 * Steinbruecker et al. 2011 / Park et al. 2017, Open3D's compute_rgbd_odometry with the hybrid Jacobian: the coloured ICP above on
 * the pixel grid, where the association is a projection instead of a search.  Every result is a function of the input only, never
 * of scheduling or launch shape; no float atomics, no allocation, nothing read back. ---- */

/* The planes one frame contributes, ONE launch, all float32, every operation rounded on its own (no contraction).
 * seen(x,y) = mask is NULL or mask(x,y) == 1 exactly; ok(x,y) = seen and depth finite and depth_min < depth <= depth_max.
 *   depth_out     = depth where ok, NaN elsewhere;
 *   intensity_out = ((r + g) + b) / 3.0f where seen, NaN elsewhere (gsr_frame_undistort writes colour 0 outside the mask: that must
 *                   not become an edge); a non-finite colour component gives what IEEE arithmetic gives;
 *   grad_out      = four planes dI/dx, dI/dy, dD/dx, dD/dy: the 3 x 3 Sobel operator on intensity_out resp. depth_out times 0.125.
 *                   With P = the plane:  d/dx = (((P(x+1,y-1) - P(x-1,y-1)) + 2.0f (P(x+1,y) - P(x-1,y))) + (P(x+1,y+1) - P(x-1,y+1)))
 *                   * 0.125f, and d/dy its transpose: (((P(x-1,y+1) - P(x-1,y-1)) + 2.0f (P(x,y+1) - P(x,y-1))) + (P(x+1,y+1) -
 *                   P(x+1,y-1))) * 0.125f.  Pixels on the image border (x = 0, y = 0, x = w - 1, y = h - 1) get NaN in all four;
 *                   inside, an invalid tap spreads by IEEE NaN arithmetic alone.  NULL: not wanted (the source frame of
 *                   gsr_odometry_update needs only the first two outputs).
 * Errors before the launch: NULL color / depth / intensity_out / depth_out, a side < 1 or more than 2^30 - 1 pixels, depth_min or
 * depth_max NaN, depth_max <= depth_min: GSR_ERR_INVALID_ARGUMENT. */
int gsr_odometry_prepare(int32_t w, int32_t h, const float* color /*[3,h,w]*/, const float* depth /*[h,w]*/,
                         const float* mask /*[h,w] or NULL*/, float depth_min, float depth_max, float* intensity_out /*[h,w]*/,
                         float* depth_out /*[h,w]*/, float* grad_out /*[4,h,w] or NULL*/, void* stream);

/* One Gauss-Newton step for T (float64 row-major 4 x 4, source-camera to target-camera coordinates), both images w x h with
 * K = (fx, fy, cx, cy) (HOST float64[4], pixel centres at integer coordinates), planes from gsr_odometry_prepare.  For the source
 * pixel (x, y), everything in float64 from the float32 planes, every operation rounded on its own, in this order:
 *   1. d = src_depth, I_s = src_intensity: both finite;
 *   2. P = (d ((x - cx) / fx), d ((y - cy) / fy), d);
 *   3. Q = R P + t, component k = ((T[k,0] Px + T[k,1] Py) + T[k,2] Pz) + T[k,3];
 *   4. Qz finite and > 0;
 *   5. u = fx (Qx / Qz) + cx, v = fy (Qy / Qz) + cy;
 *   6. ui = floor(u + 0.5), vi = floor(v + 0.5), 0 <= ui <= w - 1 and 0 <= vi <= h - 1 compared as doubles (a NaN, an infinity or
 *      a value beyond an int drops out here, before any conversion);
 *   7. at (vi, ui): d_t = tgt_depth, I_t = tgt_intensity and the four components gIx, gIy, gDx, gDy of tgt_grad all finite;
 *   8. |d_t - Qz| <= depth_diff_max.
 * The pixels that pass are the n participants.  With a = fx / Qz, b = fy / Qz, lambda = lambda_geometric:
 *   depth        r_D = d_t - Qz,   c_D = (gDx a, gDy b, -(((gDx a) Qx + (gDy b) Qy) / Qz) - 1),   J_D = sqrt(lambda) [Q x c_D, c_D];
 *   photometric  r_I = I_t - I_s,  c_I = (gIx a, gIy b, -(((gIx a) Qx + (gIy b) Qy) / Qz)),       J_I = sqrt(1 - lambda) [Q x c_I, c_I]
 * (Q x c = (Qy c2 - Qz c1, Qz c0 - Qx c2, Qx c1 - Qy c0), each entry then times the weight), the residuals weighted by the same
 * factors.  Over the participants, with the summation structure of gsr_icp_update (at most 256 workgroups over fixed slices of
 * the row-major pixel index, a fixed in-wave butterfly, wave and workgroup sums added in order), 30 sums: the 21 entries of the
 * upper triangle of J^T J (J_D[p] J_D[q] + J_I[p] J_I[q]) and the 6 of J^T r (J_D[p] r_D' + J_I[p] r_I', the weighted residuals), n,
 * sum r_D^2 and sum r_I^2 - the last two unweighted, each 0 where its weight (lambda, 1 - lambda) is 0.  One thread solves J^T J x =
 * -J^T r by LDL^T with the pivot rule of gsr_icp_update_plane; x = (alpha, beta, gamma, t), dR = Rz(gamma) Ry(beta) Rx(alpha),
 * T <- [dR, t] T (row 3 = 0 0 0 1; no shift: camera coordinates lie near the origin).
 * stats_dev[8] = n, fitness = n / (w h), inlier_rmse = sqrt(sum r_D^2 / n) (0 with n = 0), status, sum r_D^2, sum r_I^2, 0, 0 - all
 * of the INCOMING T.  status: 0 = T updated; 1 = n < 6; 2 = a rejected pivot (a fronto-parallel untextured wall, say).  With
 * status != 0, or with apply == 0 (stats and status only), T_dev is left bit for bit as it was.
 * Errors before any launch: a NULL pointer, a side < 1 or more than 2^30 - 1 pixels, K not finite or fx, fy not > 0,
 * lambda_geometric outside [0, 1] or NaN, depth_diff_max not > 0: GSR_ERR_INVALID_ARGUMENT; workspace below
 * gsr_odometry_workspace_bytes(w, h): GSR_ERR_STATE_TOO_SMALL. */
size_t gsr_odometry_workspace_bytes(int32_t w, int32_t h);
int gsr_odometry_update(int32_t w, int32_t h, const double* K /*HOST [4]*/, const float* src_intensity /*[h,w]*/,
                        const float* src_depth /*[h,w]*/, const float* tgt_intensity /*[h,w]*/, const float* tgt_depth /*[h,w]*/,
                        const float* tgt_grad /*[4,h,w]*/, double lambda_geometric, double depth_diff_max, int32_t apply,
                        double* T_dev /*[16] in/out*/, double* stats_dev /*[8] out*/, void* workspace, size_t workspace_bytes,
                        void* stream);

/* ---- pose graph (csrc/posegraph.hip): the edges that gsr_icp_update*, gsr_ransac_feature_matching
 * and gsr_odometry_update produce become the per-keyframe corrections that gsr_transform_gaussians consumes.  Float64 throughout,
 * no float atomics, no allocation on the device, deterministic: two runs give identical bits. ---- */

/* Information matrix of a registration (Open3D's GetInformationMatrixFromPointClouds).  Row i takes part iff 0 <= idx[i] < Pt and
 * p = target[idx[i]] is finite.  Per row, G^T G is added for the three rows G_1 = [0, z, -y, 1, 0, 0], G_2 = [-z, 0, x, 0, 1, 0],
 * G_3 = [y, -x, 0, 0, 0, 1] of p = (x, y, z): 21 float64 sums plus n, with the summation structure of gsr_icp_update (at most 256
 * workgroups over fixed slices, a fixed in-wave butterfly, wave and workgroup sums added in order).  info_out[36]: the symmetric
 * 6 x 6 row-major, unknowns (alpha, beta, gamma, tx, ty, tz); entry [3][3] = n.  stats_dev[4] = n, 0, 0, 0.  n = 0 gives a zero
 * matrix.  Errors before any launch: sizes outside [1, 2^30 - 1], a NULL pointer: GSR_ERR_INVALID_ARGUMENT; workspace below
 * gsr_information_workspace_bytes(Ps): GSR_ERR_STATE_TOO_SMALL. */
size_t gsr_information_workspace_bytes(int64_t Ps);
int gsr_registration_information(int64_t Pt, const float* target /*[Pt,3]*/, int64_t Ps, const int32_t* idx /*[Ps]*/,
                                 double* info_out /*[36]*/, double* stats_dev /*[4]*/, void* workspace, size_t workspace_bytes,
                                 void* stream);

/* The pose graph.  Nodes i = 0 .. N-1 with poses X_i (float64 row-major 4 x 4, node frame to world) and fixed[i] (the node does not
 * move).  Edges k = 0 .. E-1 with s_k != t_k, T_k (takes coordinates of node s_k to coordinates of node t_k: what gsr_icp_update
 * leaves in T_dev for source s_k and target t_k), Lambda_k (symmetric float64 6 x 6) and uncertain_k (a loop closure).  Unknowns in
 * the order (alpha, beta, gamma, tx, ty, tz); M(delta) = [Rz(gamma) Ry(beta) Rx(alpha), t], the composition of gsr_icp_update_plane
 * (one body, csrc/solve6_common.h).
 *   residual   D_k = T_k^-1 X_t^-1 X_s, e_k = vec6(D_k), the inverse of M: with sy = sqrt(R00^2 + R10^2), sy > 1e-6: alpha =
 *              atan2(R21, R22), beta = atan2(-R20, sy), gamma = atan2(R10, R00); otherwise alpha = atan2(-R12, R11), beta =
 *              atan2(-R20, sy), gamma = 0; t = the last column.  Rigid inverses are [R^T, -R^T t]; X_t^-1 X_s is formed as
 *              [Rt^T Rs, Rt^T (ts - tt)], the difference first, so a graph far from the origin loses nothing.
 *   Jacobian   (Open3D's linearisation) column j of J_k = lin6(T_k^-1 X_t^-1 G_j X_s), G_0..2 the generators of rotation about x, y,
 *              z, G_3..5 the translations, lin6(M) = ((M21 - M12) / 2, (M02 - M20) / 2, (M10 - M01) / 2, M03, M13, M23); delta_s
 *              enters with +J_k, delta_t with -J_k.
 *   objective  r_k = e_k^T Lambda_k e_k; F = sum over certain edges of r_k + sum over uncertain edges of mu r_k / (mu + r_k) (the line
 *              process at its optimum: Geman-McClure); w_k = 1 for a certain edge, (mu / (mu + r_k))^2 for an uncertain one;
 *              W_k = w_k J_k^T Lambda_k J_k (upper triangle, 21 values, rows from the diagonal on), g_k = w_k J_k^T Lambda_k e_k.
 *              Over free nodes: H_ii = the sum of W_k over the edges incident to i, the off-diagonal block of an edge is -W_k,
 *              b_s += g_k, b_t -= g_k; an edge to a fixed node contributes only to the free node's H_ii and b.  A node sums its
 *              edges in ascending k.  The records of a fixed node are zero.
 *   solve      (H + lambda I) delta = -b by preconditioned conjugate gradients from delta = 0.  Every free node's H_ii is first
 *              held to the LDL^T pivot rule of gsr_icp_update_plane, once per linearisation (lambda I would hide a node that its
 *              edges do not fix, Lambda = 0 say), then H_ii + lambda I is factored by the same body: the block-Jacobi preconditioner.  Stops at |r|_2 <=
 *              cg_rtol |b|_2 (status 0) or after cg_max_iteration products (status 1).  Status 2: a rejected pivot, or a direction
 *              with p.Ap not > 0 (sums that are not finite); delta is then all zeros.  Rows of fixed nodes are exactly 0.
 *   step       X_i <- M(delta_i) X_i (left product, row 3 written as 0 0 0 1).  rho = (F - F_new) / (delta^T (lambda delta - b)).
 *              Accepted iff F_new < F: lambda <- lambda max(1/3, 1 - (2 rho - 1)^3), nu <- 2; otherwise lambda <- lambda nu, nu <-
 *              2 nu.  Start: lambda = 1e-5 max diag(H), nu = 2.
 *   stop       GSR_PG_MAX_ITERATION: max_iteration solves; GSR_PG_CONVERGED_STEP: |delta|_inf <= min_relative_increment (|x|_inf +
 *              min_relative_increment), x the stacked vec6(X_i) of all nodes (the step is not applied; note that the rule is
 *              relative to the LARGEST coordinate: 10 km from the origin 1e-6 stops at a centimetre - keep a graph near its own
 *              origin, or tighten the figure); GSR_PG_CONVERGED_RESIDUAL: an accepted step with F - F_new <=
 *              min_relative_residual_increment F; GSR_PG_ZERO_RESIDUAL: F == 0 (E = 0 too: nothing moves);
 *              GSR_PG_LAMBDA: lambda not finite or above 1e32; GSR_PG_SOLVER_FAILED: solve status 2 - the poses are those of
 *              the last accepted step, bit for bit the input when the first solve fails.
 * Every launch is ONE workgroup of 256 lanes: work strided over nodes and edges, iterates in the workspace, LDS for the reductions
 * only (N and E are bounded by 2^30 - 1, not by LDS), no grid-wide synchronisation, no cooperative launch, and every loop bounded by
 * max_iteration, cg_max_iteration or a count.  Dot products: each thread's nodes in order, the fixed butterfly, the four wave sums
 * in order. */
enum {
  GSR_PG_CONVERGED_STEP = 0,
  GSR_PG_MAX_ITERATION = 1,
  GSR_PG_SOLVER_FAILED = 2,
  GSR_PG_CONVERGED_RESIDUAL = 3,
  GSR_PG_ZERO_RESIDUAL = 4,
  GSR_PG_LAMBDA = 5
};
#define GSR_PG_EDGE_STRIDE 35 /* e[6], r, w, W[21], g[6] */
#define GSR_PG_NODE_STRIDE 27 /* H_ii[21], b[6] */

/* The graph's topology on the device, built once on the host: the edge ends, fixed[], and the CSR node_ptr[N + 1] / node_edge[2E]
 * (2 k + 1 where the node is edge k's target, 2 k where it is its source; ascending k per node).  edges_host: HOST int32 [E,2] =
 * (s_k, t_k); fixed_host: HOST uint8 [N]; host_scratch: gsr_posegraph_topology_bytes(N, E) bytes of HOST memory, 4-byte
 * aligned, that the blob is laid out in - the caller's, so nothing is allocated here.  The blob is then copied with ONE
 * hipMemcpyAsync on `stream` and the call does not wait for it: host_scratch must stay valid and unchanged until the stream has
 * passed the copy (scene_utils.PoseGraph keeps it beside the device blob).
 * Errors before any device work: N outside [1, 2^30 - 1], E outside [0, 2^30 - 1], a NULL pointer (edges_host may be NULL with E =
 * 0), an end outside [0, N), s_k == t_k: GSR_ERR_INVALID_ARGUMENT; topology_bytes below gsr_posegraph_topology_bytes(N, E):
 * GSR_ERR_STATE_TOO_SMALL.  The three entries below trust the blob: it must be the one filled here for this N and E. */
size_t gsr_posegraph_topology_bytes(int64_t N, int64_t E);
int gsr_posegraph_topology(int64_t N, int64_t E, const int32_t* edges_host /*HOST [E,2]*/, const uint8_t* fixed_host /*HOST [N]*/,
                           void* host_scratch /*HOST, topology_bytes*/, void* topology, size_t topology_bytes, void* stream);

/* One workspace size for gsr_posegraph_solve and gsr_posegraph_optimize (0 for sizes out of range). */
size_t gsr_posegraph_workspace_bytes(int64_t N, int64_t E);

/* Linearisation at `poses`: edge_out[E,35] = e[6], r, w, W[21], g[6] per edge; node_out[N,27] = H_ii[21], b[6] per node;
 * scalars_out[2] = F, max diag(H).  edge_uncertain: uint8 [E] on the device.  E = 0 is legal (the edge pointers may be NULL).
 * Errors before the launch: sizes out of range, a NULL pointer, mu not > 0: GSR_ERR_INVALID_ARGUMENT. */
int gsr_posegraph_linearize(int64_t N, int64_t E, const void* topology, const double* poses /*[N,16]*/,
                            const double* edge_T /*[E,16]*/, const double* edge_info /*[E,36]*/, const uint8_t* edge_uncertain /*[E]*/,
                            double mu, double* edge_out /*[E,35]*/, double* node_out /*[N,27]*/, double* scalars_out /*[2]*/,
                            void* stream);

/* The solve above on records in the layout of gsr_posegraph_linearize (W and g of edge_rec, H_ii and b of node_rec are read):
 * delta_out[N,6]; stats_dev[4] = products taken, the achieved |r| / |b|, status 0 / 1 / 2, 0.
 * Errors before the launch: sizes out of range, a NULL pointer, lambda not finite or < 0, cg_rtol < 0 or NaN, cg_max_iteration <
 * 1: GSR_ERR_INVALID_ARGUMENT; workspace below gsr_posegraph_workspace_bytes(N, E): GSR_ERR_STATE_TOO_SMALL. */
int gsr_posegraph_solve(int64_t N, int64_t E, const void* topology, const double* edge_rec /*[E,35]*/,
                        const double* node_rec /*[N,27]*/, double lambda, double cg_rtol, int32_t cg_max_iteration,
                        double* delta_out /*[N,6]*/, double* stats_dev /*[4]*/, void* workspace, size_t workspace_bytes, void* stream);

/* The whole Levenberg-Marquardt loop above in ONE launch: poses[N,16] in place; edge_w_out[E] and edge_r_out[E] = w_k and r_k at the
 * returned poses; stats_dev[16] = status (GSR_PG_*), solves, accepted steps, F at the start, F at the end, lambda at the end, the
 * total of PCG products, the worst achieved |r| / |b| of a solve, then zeros.  Poses of fixed nodes are never written.
 * Errors before the launch: sizes out of range, a NULL pointer (the edge pointers may be NULL with E = 0), mu not > 0,
 * max_iteration < 0, an increment or cg_rtol < 0 or NaN, cg_max_iteration < 1: GSR_ERR_INVALID_ARGUMENT; workspace below
 * gsr_posegraph_workspace_bytes(N, E): GSR_ERR_STATE_TOO_SMALL.  No allocation. */
int gsr_posegraph_optimize(int64_t N, int64_t E, const void* topology, double* poses /*[N,16] in/out*/,
                           const double* edge_T /*[E,16]*/, const double* edge_info /*[E,36]*/, const uint8_t* edge_uncertain /*[E]*/,
                           double mu, int32_t max_iteration, double min_relative_increment, double min_relative_residual_increment,
                           double cg_rtol, int32_t cg_max_iteration, double* edge_w_out /*[E]*/, double* edge_r_out /*[E]*/,
                           double* stats_dev /*[16]*/, void* workspace, size_t workspace_bytes, void* stream);

/* ---- global registration (csrc/features.hip) - what the reference's commented pipeline would take
 * from Open3D's compute_fpfh_feature and registration_ransac_based_on_feature_matching.  Every result is a function of the input
 * only, never of traversal, scheduling or launch shape; no float atomics, no allocation. ---- */

#define GSR_FPFH_WIDTH 33              /* three blocks of 11 bins */

/* Fast point feature histogram of every row.
 * Neighbourhood: N_i of gsr_estimate_normals exactly (float32 d2, bound = min(r2, d_k), rows tied at the bound all belong,
 * duplicates are members), max_nn in [3, GSR_KNN_K_MAX + 1]; or max_nn = 0: radius only, bound = r2, `radius` finite - the
 * departure that serves Open3D's (5 voxel, 100) call: on a voxel-sampled surface a ball of five voxel sizes holds fewer than
 * 100 rows almost everywhere, so the cut at 100 never acts.  Others_i = N_i \ {i}, m_i = |Others_i|.  A row whose point or normal
 * has a non-finite component is masked before the structure is built (it takes no part in the bounding box, the sort or the
 * boxes, so no other row's bits depend on where it lies): fpfh NaN, counts 0, count 0, nobody's neighbour.
 * Pair feature of (i, j), all in float64: delta = p_j - p_i per component in float32, promoted; normals promoted;
 * d2 = (dx dx + dy dy) + dz dz, d = sqrt(d2).  d2 = 0: (0, 0, 0).  Otherwise a1 = n_i.delta / d, a2 = n_j.delta / d; if
 * |a1| < |a2| (strictly) (n1, n2, delta) <- (n_j, n_i, -delta) and f2 = -a2, else n1 = n_i, n2 = n_j, f2 = a1.  v = delta x n1;
 * |v| = 0: (0, 0, 0); else v <- v / |v|, w = n1 x v, f1 = v.n2, f0 = atan2(w.n2, n1.n2).  Bins, each clamped to [0, 10]:
 * floor(11 (f0 + pi) / (2 pi)) in block 0, floor(11 (f1 + 1) / 2) in block 1, floor(11 (f2 + 1) / 2) in block 2.
 * spfh_counts[i][b]: the number of j in Others_i whose feature falls into bin b - integers, exact, independent of any order.
 * SPFH_i(b) = 100 c / m_i.  FPFH_i: A_b = sum over j in Others_i with d2 > 0 of SPFH_j(b) / d2 - evaluated as
 * c_j(b) (100 / (m_j d2)) - in float64 in the order of the sorted structure (fixed for a given input); each block of 11 scaled
 * by 100 / (sum of its A_b) where that sum is not 0; SPFH_i(b) added; ONE rounding to float32.  m_i = 0: a zero row.
 * count[i] = |N_i| = m_i + 1 (0 for a masked row).
 * Errors before any launch: P outside [1, 2^30 - 1], NULL points / normals / fpfh / workspace, radius <= 0 or NaN, max_nn outside
 * {0} + [3, 33], max_nn = 0 with an infinite radius: GSR_ERR_INVALID_ARGUMENT; workspace below gsr_fpfh_workspace_bytes(P):
 * GSR_ERR_STATE_TOO_SMALL. */
size_t gsr_fpfh_workspace_bytes(int64_t P);
int gsr_compute_fpfh(int64_t P, const float* points /*[P,3]*/, const float* normals /*[P,3]*/, float radius, int32_t max_nn,
                     float* fpfh /*[P,33]*/, int32_t* spfh_counts /*[P,33] or NULL*/, int32_t* count /*[P] or NULL*/,
                     void* workspace, size_t workspace_bytes, void* stream);

/* Nearest target feature of every query feature, brute force.  d2(q, t) = sum over b ascending of (q_b - t_b)^2 in float32:
 * e = q_b - t_b rounded, d2 = fma(e, e, d2) from d2 = 0.  idx_out[i] = the row of the lexicographic minimum of (d2, row) over the
 * target rows whose d2 is not NaN, dist2_out[i] its d2: a target row with a NaN never wins, identical rows give the smallest.
 * A query with a NaN: -1 and NaN; no target row without a NaN: -1 and +inf.
 * Target rows pass through LDS GSR_FEATURE_NN_TILE at a time; with few queries the target's tiles are split over a second grid
 * dimension in runs of gsr_feature_nn_tiles_per_split(Nq, Nt) tiles (aiming at GSR_FEATURE_NN_WORKGROUPS workgroups), and the
 * partial minima meet in one 64-bit integer atomicMin per query on (bits of d2, row): no output bit depends on the split.
 * `width` must be GSR_FPFH_WIDTH.  Errors before any launch: sizes outside [1, 2^30 - 1], NULL query / target / idx_out /
 * workspace, another width: GSR_ERR_INVALID_ARGUMENT; workspace below gsr_feature_nn_workspace_bytes(Nq): GSR_ERR_STATE_TOO_SMALL. */
#define GSR_FEATURE_NN_TILE 128
#define GSR_FEATURE_NN_WORKGROUPS 512
size_t gsr_feature_nn_workspace_bytes(int64_t Nq);
int32_t gsr_feature_nn_tiles_per_split(int64_t Nq, int64_t Nt);
int gsr_feature_nn(int64_t Nq, const float* query /*[Nq,33]*/, int64_t Nt, const float* target /*[Nt,33]*/, int32_t width,
                   int32_t* idx_out /*[Nq]*/, float* dist2_out /*[Nq] or NULL*/, void* workspace, size_t workspace_bytes,
                   void* stream);

/* RANSAC over given correspondences (Open3D's registration_ransac_based_on_feature_matching after the matching): trials
 * [t0, t0 + n) against the DEVICE record `best`, which the call improves on - consecutive calls over consecutive ranges give
 * exactly what one call over the union gives.  A fresh record: count = -1, sum_d2 = +inf, trial = -1, T = identity,
 * trials_checked = 0.  All geometry in float64 from the float32 coordinates.
 * A pair (source row, target row) that names a row outside its cloud or a non-finite point is unusable: a trial that samples it
 * is rejected, and it is never an inlier; nothing is read out of bounds.
 * Trial t: sample s = 0 .. ransac_n - 1 picks pair ((mix(seed + (8 t + s + 1) 0x9E3779B97F4A7C15) >> 32) M) >> 32, mix the
 * splitmix64 finaliser (z ^= z >> 30, z *= 0xBF58476D1CE4E5B9, z ^= z >> 27, z *= 0x94D049BB133111EB, z ^= z >> 31), all
 * mod 2^64.  Status, the first that applies: 1 two samples coincide; 2 a sampled pair is unusable; 3 (edge_length_threshold
 * theta > 0) some sample pair (a, b) fails |s_a - s_b| >= theta |t_a - t_b| or |t_a - t_b| >= theta |s_a - s_b|; 4 no rotation
 * (sums not finite); 5 some sample has |T s - t|^2 > max_distance^2; 0 survives.  T: Horn's quaternion form on the samples'
 * centred cross-covariance (the routine of gsr_icp_update), t = tbar - R sbar.
 * Score of a survivor, over ALL M pairs in their order: a usable pair is an inlier iff |T s - t|^2 <= max_distance^2
 * ((double)max_distance squared in float64); count, and sum_d2 over the inliers in float64.  The winner is the lexicographic
 * best of (count max, sum_d2 min, trial min) over the survivors and the incoming record; trials_checked grows by the number of
 * survivors.  Without a survivor the record is not written.
 * debug (NULL in production): per trial of this call the samples (-1 beyond ransac_n), the status and T (rows 0 .. 2 zero unless
 * status is 0 or 5) - any of the three pointers may be NULL.
 * Errors before any launch: sizes outside [1, 2^30 - 1], NULL source / target / pairs / best / workspace, max_distance negative,
 * NaN or infinite, ransac_n outside [3, GSR_RANSAC_N_MAX], theta outside [0, 1], t0 outside [0, 2^56] (8 t + 8 must not wrap a
 * signed 64-bit trial number), n outside [1, GSR_RANSAC_MAX_TRIALS]:
 * GSR_ERR_INVALID_ARGUMENT; workspace below gsr_ransac_workspace_bytes(M, n): GSR_ERR_STATE_TOO_SMALL. */
#define GSR_RANSAC_N_MAX 8
#define GSR_RANSAC_MAX_TRIALS (1 << 20)
typedef struct gsr_ransac_best {
  int64_t count;
  double sum_d2;
  int64_t trial;
  double T[16];            /* row-major 4 x 4 */
  int64_t trials_checked;  /* survivors scored so far */
} gsr_ransac_best;
typedef struct gsr_ransac_debug {
  int32_t* samples;        /* device [n,8] or NULL */
  int32_t* status;         /* device [n] or NULL */
  double* T;               /* device [n,16] or NULL */
} gsr_ransac_debug;
size_t gsr_ransac_workspace_bytes(int64_t M, int64_t n);
int gsr_ransac_feature_matching(int64_t Ps, const float* source /*[Ps,3]*/, int64_t Pt, const float* target /*[Pt,3]*/, int64_t M,
                                const int32_t* pairs /*[M,2]*/, float max_distance, int32_t ransac_n, float edge_length_threshold,
                                uint64_t seed, int64_t t0, int64_t n, gsr_ransac_best* best /*device, in/out*/, void* workspace,
                                size_t workspace_bytes, const gsr_ransac_debug* debug /*HOST struct or NULL*/, void* stream);

/* ---- sparse image features for place recognition (csrc/orb.hip): FAST-9 corners, a 256-bit BRIEF
 * descriptor steered by the intensity centroid, brute-force Hamming matching.  After the quantisation every step is integer
 * arithmetic (one float64 atan2 of two integers aside): every output is a function of the input alone - no global atomics in the
 * image kernels, no float atomics anywhere, the same bits on every run.  This is not OpenCV's ORB: the sampling pattern is the
 * library's own (tools/make_orb_pattern.py), so the descriptors are not interchangeable with OpenCV's. ---- */
#define GSR_ORB_CELL 32          /* a workgroup of the detector owns one 32 x 32 cell of pixels */
#define GSR_ORB_BORDER 17        /* a keypoint has 17 <= x < w - 17, 17 <= y < h - 17: disc 15 + box 2 */
#define GSR_ORB_BINS 30          /* orientation bins of 12 degrees */
#define GSR_ORB_PER_CELL_MAX 16
#define GSR_HAMMING_NONE 257     /* "no such row": larger than any distance of 256-bit words */

/* Quantised planes of an image.  image: [3,h,w] planar with channels = 3 - the intensity is the odometry's I = ((r + g) + b) / 3,
 * each step rounded to float32 - or [h,w] with channels = 1 (I as given).
 *   u8[y][x]  = clamp(floor(fmaf(255, I, 0.5)), 0, 255): ONE fused multiply-add in float32 (a float64 evaluation of 255 I + 0.5
 *               rounded once to float32 gives the same value), a NaN counts as 0, +inf as 255, -inf as 0;
 *   box[y][x] = the sum of u8 over the 5 x 5 window centred on (x, y), coordinates clamped to the image (replicated border);
 *               uint16, at most 6375.
 * Errors before any launch: a side < 1 or w h > 2^30 - 1, a NULL pointer, channels not 1 or 3: GSR_ERR_INVALID_ARGUMENT. */
int gsr_orb_prepare(int32_t w, int32_t h, const float* image, int32_t channels, uint8_t* u8_out /*[h,w]*/,
                    uint16_t* box_out /*[h,w]*/, void* stream);

/* ceil(w / 32) ceil(h / 32): the cells of gsr_orb_detect, row-major (cell = cy * ceil(w / 32) + cx); 0 for a bad size. */
int64_t gsr_orb_cells(int32_t w, int32_t h);

/* FAST-9 corners of the u8 plane.  Circle of pixel p = (x, y), clockwise from the top with y down: c[0 .. 15] at the offsets
 * (0,-3) (1,-3) (2,-2) (3,-1) (3,0) (3,1) (2,2) (1,3) (0,3) (-1,3) (-2,2) (-3,1) (-3,0) (-3,-1) (-2,-2) (-1,-3).
 *   score(p) = max over s = 0 .. 15 of max( min_{k<9} (c[(s+k) % 16] - p), min_{k<9} (p - c[(s+k) % 16]) )   (integers);
 *   p qualifies iff 17 <= x < w - 17 and 17 <= y < h - 17 and (mask == NULL or mask[y][x] > 0);
 *   p is a corner iff it qualifies and score(p) > threshold; S(p) = score(p) for a corner, 0 for every other pixel;
 *   3 x 3 non-maximum suppression: a corner p survives iff for each of its 8 neighbours q: S(p) > S(q), or S(p) == S(q) and p
 *   comes before q in raster order (y, then x).
 * Every cell keeps its per_cell best survivors, ordered by score descending, then raster order ascending, in its own slots:
 * slots[cell][r] = (x, y, score) int32, r = 0 .. per_cell - 1; an empty slot is (0, 0, 0).  Every slot is written.  An image with
 * a side < 35 has no pixel that qualifies: all slots empty.
 * Errors before the launch: a bad size, NULL u8 / slots, threshold outside 0 .. 254, per_cell outside 1 .. 16, more than 65535
 * rows of cells: GSR_ERR_INVALID_ARGUMENT. */
int gsr_orb_detect(int32_t w, int32_t h, const uint8_t* u8 /*[h,w]*/, const float* mask /*[h,w] or NULL*/, int32_t threshold,
                   int32_t per_cell, int32_t* slots /*[cells,per_cell,3]*/, void* stream);

/* Orientation and descriptor of M keypoints (x, y, score), e.g. the slots of gsr_orb_detect as they are.  A row with score <= 0 or
 * outside the border of 17 is skipped: angle_bin -1, moments 0, descriptor 0 - nothing is read out of bounds.  Otherwise
 *   m10 = sum dx u8[y+dy][x+dx],  m01 = sum dy u8[y+dy][x+dx]  over the disc dx^2 + dy^2 <= 15^2   (int32, exact);
 *   angle_bin = floor(atan2(m01, m10) / (2 pi / 30) + 0.5) mod 30 in float64 (m10 = m01 = 0: bin 0);
 *   bit b of the descriptor = box[y + y1][x + x1] < box[y + y2][x + x2] with (x1, y1, x2, y2) = pattern[angle_bin][b];
 *   descriptors[k][b / 32] holds bit b at position b % 32.
 * moments: [M,2] = (m10, m01), or NULL.  M = 0 is legal.
 * Errors before the launch: a bad size, NULL u8 / box, M outside [0, 2^30 - 1], with M > 0 a NULL keypoints / angle_bin /
 * descriptors: GSR_ERR_INVALID_ARGUMENT. */
int gsr_orb_describe(int32_t w, int32_t h, const uint8_t* u8, const uint16_t* box, int64_t M, const int32_t* keypoints /*[M,3]*/,
                     int32_t* angle_bin /*[M]*/, int32_t* moments /*[M,2] or NULL*/, int32_t* descriptors /*[M,8]*/, void* stream);

/* The sampling pattern the library was built with, int8 [30][256][4] = (x1, y1, x2, y2) per bin and bit, into HOST memory `out`
 * (30720 bytes).  256 pairs drawn iid from a Gaussian (sigma = 31 / 5) by a counter-based generator with a fixed seed, a draw
 * rejected outside the disc of radius 15; each pair rotated by the bin angles 2 pi k / 30 as (x cos - y sin, x sin + y cos) and
 * rounded to nearest; a pair is accepted only if all its rounded points stay within radius 15, otherwise it is drawn again
 * (tools/make_orb_pattern.py writes csrc/orb_pattern.inc).  Needs no device. */
int gsr_orb_pattern(int8_t* out /*HOST [30720]*/);

/* Brute-force Hamming matching of 256-bit rows (8 x int32, 16-byte aligned).  For every query row i over the database rows j in
 * ascending order: d = popcount(q_i xor t_j); idx_out[i] = the row of the smallest d, among equal distances the lowest row;
 * best_out[i] = that d; second_out[i] = the second smallest d of the multiset (a duplicate of the best row: second == best).
 * Where there is no such row (N = 0, or N = 1 for the second): idx -1, distance GSR_HAMMING_NONE.  Q = 0 or N = 0 is legal.
 * The database passes through LDS in tiles; distances use the hardware popcount.
 * Errors before the launch: Q or N outside [0, 2^30 - 1], a NULL or misaligned query (Q > 0) / db (N > 0), with Q > 0 a NULL
 * output: GSR_ERR_INVALID_ARGUMENT. */
int gsr_hamming_match(int64_t Q, const int32_t* query /*[Q,8]*/, int64_t N, const int32_t* db /*[N,8]*/, int32_t* idx_out /*[Q]*/,
                      int32_t* best_out /*[Q]*/, int32_t* second_out /*[Q]*/, void* stream);

/* The keyframe-database query: db holds the descriptors of K frames one behind the other, frame k = rows [segments[k],
 * segments[k+1]) (device int32 [K+1], ascending; a value outside 0 .. N is clamped, so nothing is read past the database).
 * votes[k] = the number of query rows whose match INSIDE frame k (best, second as gsr_hamming_match defines them over the
 * segment alone) has best <= max_distance and (float)best < ratio * (float)second, the product rounded to float32 - with a
 * segment of one row second is GSR_HAMMING_NONE, an empty segment gets no vote.  One grid row per frame; the counts are int32
 * sums (cleared by the call), the same on every run.  Q = 0, N = 0 or K = 0 is legal.
 * Errors before any launch: sizes as gsr_hamming_match, K outside [0, 65535], with K > 0 a NULL segments / votes, max_distance
 * < 0, ratio negative or NaN: GSR_ERR_INVALID_ARGUMENT. */
int gsr_hamming_vote(int64_t Q, const int32_t* query /*[Q,8]*/, int64_t N, const int32_t* db /*[N,8]*/, int64_t K,
                     const int32_t* segments /*[K+1]*/, int32_t max_distance, float ratio, int32_t* votes /*[K]*/, void* stream);

/* ---- LiDAR scans for place recognition (csrc/scancontext.hip): the polar "scan context" descriptor
 * of Kim & Kim (IROS 2018) - rings x sectors around the sensor, the largest height per cell - and the exhaustive search over all
 * column shifts.  A rotation of the sensor about its vertical axis is a cyclic shift of the descriptor's columns, so the search
 * gives a distance and a yaw together.  Integer atomic max only (a height >= +0 orders by its float bits), every sum in one
 * fixed order: the same bits on every run, whatever the order of the points.  No workspace. ---- */
#define GSR_SCAN_CONTEXT_MAX_RINGS 40
#define GSR_SCAN_CONTEXT_MAX_SECTORS 120
#define GSR_SCAN_CONTEXT_MAX_ORIGINS 16

/* B descriptors of one cloud, one per origin.  frame: HOST, row-major 3 x 4, cloud -> levelled sensor frame with z up (NULL: the
 * identity, no arithmetic at all); origins: HOST [B,3] in the levelled frame (NULL: B = 1, the origin 0 0 0).  Per point and
 * origin, every operation rounded to float32 on its own (no fused multiply-add):
 *   q_i = ((F[i][0] x + F[i][1] y) + F[i][2] z) + F[i][3]  (q = the point itself without a frame);  p = q - origin;
 *   the point is skipped if a component of p is not finite;
 *   rho2 = p.x p.x + p.y p.y; skipped unless 0 < rho2 < max_range max_range;
 *   ring = min(R - 1, floor(sqrt(rho2) R / max_range));
 *   theta = atan2f(p.y, p.x), + float32(2 pi) where negative;  sector = min(S - 1, floor(theta S / float32(2 pi)));
 *   h = p.z + height_offset where that is > 0, else +0;   descriptors[b][ring][sector] = max over the points; an empty cell is 0.
 * (atan2f is the device library's: a point within a few ulp of a sector boundary may fall on either side.)
 * norms[b][c] = sqrt(s_R) with s_0 = 0, s_{r+1} = s_r + d d, d = descriptors[b][r][c]: rings in ascending order.
 * N = 0 is legal: all zeros.
 * Errors before any launch: rings outside 1 .. 40, sectors outside 1 .. 120, B outside 1 .. 16, NULL origins with B > 1, N
 * outside [0, 2^30 - 1], NULL descriptors / norms, NULL points with N > 0, max_range not finite or <= 0, height_offset, a frame
 * or an origin entry not finite: GSR_ERR_INVALID_ARGUMENT. */
int gsr_scan_context(int64_t N, const float* points /*[N,3]*/, const float* frame /*HOST [12] or NULL*/, int32_t B,
                     const float* origins /*HOST [B,3] or NULL*/, int32_t rings, int32_t sectors, float max_range,
                     float height_offset, float* descriptors /*[B,rings,sectors]*/, float* norms /*[B,sectors]*/, void* stream);

/* B query descriptors (the variants: one scan seen from B origins) against K database descriptors, with their norms.  For variant b
 * and shift s, in float32, every operation rounded on its own:
 *   d(b, s) = 1 - (sum over c of dot(c) / (nq[b][(c + s) mod S] nd[k][c])) / n,
 *   dot(c) = sum over r ascending of q[b][r][(c + s) mod S] d[k][r][c], starting from 0;
 * the outer sum runs, c ascending from 0, over the n columns where both norms are non-zero; n = 0: d = 1.
 * dist[k] = the minimum over b and s, variant[k] and shift[k] where it is reached: among equal distances the smallest b, then the
 * smallest s.  A shift s says: the query's points are about Rz(s 2 pi / S) times the database scan's points.
 * Descriptors and norms are expected finite, as gsr_scan_context writes them: a d(b, s) that comes out NaN (an inf or NaN in a
 * grid supplied by the caller) never wins, and a row where no d(b, s) is comparable gets dist +inf, shift = variant = INT32_MAX.
 * One workgroup per database row, both grids in LDS, one lane per shift.  K = 0 is legal.
 * Errors before the launch: sizes as gsr_scan_context, K outside [0, 2^30 - 1], NULL query / query_norms, with K > 0 a NULL db /
 * db_norms / output: GSR_ERR_INVALID_ARGUMENT. */
int gsr_scan_context_distance(int32_t rings, int32_t sectors, int32_t B, const float* query /*[B,rings,sectors]*/,
                              const float* query_norms /*[B,sectors]*/, int64_t K, const float* db /*[K,rings,sectors]*/,
                              const float* db_norms /*[K,sectors]*/, float* dist /*[K]*/, int32_t* shift /*[K]*/,
                              int32_t* variant /*[K]*/, void* stream);

/* ---- sensor_msgs/PointCloud2 on the device (csrc/pointcloud2.hip): what the reference's
 * process_pointcloud / read_pointcloud do point by point with `struct` in Python before a cloud reaches Open3D ---- */

/* The layout of a message's byte buffer (HOST struct).  Point n = v * width + u starts at byte v * row_step + u * point_step.
 * datatype: ROS's PointField code - 1 INT8, 2 UINT8, 3 INT16, 4 UINT16, 5 INT32, 6 UINT32, 7 FLOAT32, 8 FLOAT64.  Field offsets
 * need not be aligned to the field's size, point_step need not be a multiple of 4, row_step may exceed width * point_step. */
#define GSR_PC2_INT8 1
#define GSR_PC2_UINT8 2
#define GSR_PC2_INT16 3
#define GSR_PC2_UINT16 4
#define GSR_PC2_INT32 5
#define GSR_PC2_UINT32 6
#define GSR_PC2_FLOAT32 7
#define GSR_PC2_FLOAT64 8
typedef struct gsr_pc2_layout {
  uint32_t width, height, point_step, row_step;
  int32_t is_bigendian;
  int32_t offset[3];       /* of x, y, z inside a point */
  int32_t datatype[3];
  int32_t color_offset;    /* -1: the message has no colour */
  int32_t color_datatype;  /* FLOAT32, UINT32 or INT32: the packed 0x00RRGGBB word ROS calls rgb / rgba */
} gsr_pc2_layout;

/* Decode, crop, pose and compact a PointCloud2 byte buffer (`data`: DEVICE bytes, any alignment).  Per point n, in this order:
 *  1. x, y, z are read in the message's byte order and converted to float32: FLOAT32 bit for bit (NaN payloads survive), FLOAT64
 *     and the 32-bit integers by ONE round-to-nearest-even conversion, the small integers exactly - numpy.astype(float32).
 *  2. skip_nans != 0: the row is dropped if x, y or z is NaN, or if the message has a FLOAT32 colour field whose bit pattern is a
 *     NaN (what sensor_msgs.point_cloud2.read_points(field_names = x, y, z, rgb, skip_nans = True) drops; it applies whether or
 *     not out_colors is given).  +-inf is no NaN.  With skip_nans == 0 NaN rows pass: every comparison of step 3 is false for them.
 *  3. crop on the sensor-frame values, BEFORE the pose.  Height: dropped iff (double)y < min_y (-inf: off).  Range: dropped iff
 *     d2 > max_range2 (+inf: off), d2 = ((double)x * x + (double)y * y) + (double)z * z - the squares are exact in float64, the two
 *     sums round once each, no fused multiply-add.  A caller with a range r passes max_range2 = (double)r * (double)r.  This is
 *     the library's OWN definition of the crop: it is not a claim of bit parity with numpy.linalg.norm(...) > r at the boundary.
 *  4. pose: q = T s as defined above for registration (T_dev: DEVICE float64[16] row-major; NULL: the coordinates pass with their
 *     bits) - the same bits as gsr_transform_points on the kept rows.
 *  5. colour (out_colors given): the colour word w in the message's byte order, r = (w >> 16) & 255, g = (w >> 8) & 255,
 *     b = w & 255, every channel (float)byte / 255.0f - one correctly rounded float32 division.
 * The kept rows come out in message order (a stable compaction: ballot and prefix inside a workgroup, gsr_scan_u32 over the
 * workgroup counts): out_points, out_colors (or NULL), out_index (int32, or NULL) = the kept row's n.  count_dev[0] = rows kept,
 * count_dev[1] = 1 iff more than `cap` were kept: nothing is written at or beyond row `cap`, the count stays the true one.
 * Deterministic, no float atomics, no allocation; no byte at or beyond data_bytes (or in front of data) is ever read.
 * Errors before any launch: NULL layout / data / count_dev / workspace, out_points NULL with cap > 0, cap < 0, a datatype outside
 * 1 .. 8, a colour datatype that is not FLOAT32 / UINT32 / INT32, out_colors without a colour field, a field that does not fit
 * inside point_step, row_step < width * point_step, width * height outside [1, 2^30 - 1], (height - 1) * row_step + width *
 * point_step > data_bytes, NaN min_y / max_range2: GSR_ERR_INVALID_ARGUMENT; workspace below
 * gsr_pc2_decode_workspace_bytes(width * height): GSR_ERR_STATE_TOO_SMALL. */
size_t gsr_pc2_decode_workspace_bytes(int64_t N);
int gsr_pc2_decode(const gsr_pc2_layout* layout /*HOST*/, const void* data, size_t data_bytes, const double* T_dev /*[16] or NULL*/,
                   double min_y, double max_range2, int32_t skip_nans, float* out_points /*[cap,3]*/,
                   float* out_colors /*[cap,3] or NULL*/, int32_t* out_index /*[cap] or NULL*/, int64_t cap,
                   int64_t* count_dev /*[2]: kept, status*/, void* workspace, size_t workspace_bytes, void* stream);

/* The inverse for the canonical layout - little-endian, x / y / z FLOAT32 at 0 / 4 / 8, packed rgb FLOAT32 at 12, point_step 16,
 * height 1: out[16 P] device bytes (4-byte aligned).  Coordinates keep their bits.  Colour byte = (int)(min(max(c, 0), 1) * 255.0f
 * + 0.5f), product and sum rounded separately, a NaN colour gives 0; word = r << 16 | g << 8 | b; colors == NULL: word 0.
 * Errors before the launch: P outside [1, 2^30 - 1], NULL points / out, a misaligned out: GSR_ERR_INVALID_ARGUMENT. */
int gsr_pc2_encode(int64_t P, const float* points /*[P,3]*/, const float* colors /*[P,3] or NULL*/, void* out /*[16 P]*/,
                   void* stream);

/* test / measurement hook: on != 0 makes gsr_pc2_decode read every field straight from global memory (the path that otherwise
 * serves only the runs of points whose byte span exceeds the LDS staging buffer); 0 restores the default.  Returns the previous
 * setting.  Both paths give identical bits.  The switch is ONE process-wide variable, read when gsr_pc2_decode is called: it is
 * not meant for concurrent callers, and a caller that sets it restores it. */
int32_t gsr_debug_pc2_force_direct(int32_t on);

/* ---- sensor_msgs/Image on the device (csrc/image.hip): what the reference's imgmsg_to_pli
 * (scene/dataset_readers.py:278-309) does on the host for rgb8 / bgr8 / mono8, with `step` and `is_bigendian` honoured ---- */

/* The encodings, named as in sensor_msgs/image_encodings.h.  GSR_IMG_16UC1 is also what a caller passes for a mono16 image that
 * holds depth. */
#define GSR_IMG_RGB8 1
#define GSR_IMG_BGR8 2
#define GSR_IMG_RGBA8 3
#define GSR_IMG_BGRA8 4
#define GSR_IMG_MONO8 5
#define GSR_IMG_RGB16 6
#define GSR_IMG_BGR16 7
#define GSR_IMG_RGBA16 8
#define GSR_IMG_BGRA16 9
#define GSR_IMG_MONO16 10
#define GSR_IMG_BAYER_RGGB8 11
#define GSR_IMG_BAYER_BGGR8 12
#define GSR_IMG_BAYER_GBRG8 13
#define GSR_IMG_BAYER_GRBG8 14
#define GSR_IMG_BAYER_RGGB16 15
#define GSR_IMG_BAYER_BGGR16 16
#define GSR_IMG_BAYER_GBRG16 17
#define GSR_IMG_BAYER_GRBG16 18
#define GSR_IMG_16UC1 19
#define GSR_IMG_32FC1 20
/* The layout of a message's byte buffer (HOST struct).  Pixel (x, y) starts at byte y * step + x * bpp, bpp = channels * bytes per
 * channel (3, 4, 1 / 6, 8, 2 for the colour forms, 1 / 2 for Bayer, 2 and 4 for depth).  step may exceed width * bpp. */
typedef struct gsr_image_layout {
  uint32_t width, height, step;
  int32_t encoding;        /* GSR_IMG_* */
  int32_t is_bigendian;    /* byte order of the 16-bit words and of the 32FC1 float */
} gsr_image_layout;
#define GSR_IMG_TILE_W 256 /* pixels of one row that a workgroup stages and decodes */

/* Decode a sensor_msgs/Image byte buffer (`data`: DEVICE bytes, any alignment).  Every value is a fixed sequence of correctly
 * rounded float32 operations, none fused:
 *  colour (rgb8 .. mono16): out = planar [3,H,W]; channel = (float)sample / 255.0f, or / 65535.0f for the 16-bit forms whose word
 *     is assembled in the message's byte order.  Alpha is dropped, mono goes to all three planes.
 *  Bayer: out = planar [3,H,W].  The name spells the colours of pixels (0,0), (1,0) of row 0, then (0,1), (1,1) of row 1 (ROS's
 *     convention, not OpenCV's).  Bilinear over the 3 x 3 window: the site's own colour is its sample (n = 1); a colour found on
 *     the two horizontal or the two vertical neighbours is their mean (n = 2); a colour found on the four edge or the four
 *     diagonal neighbours is their mean (n = 4).  A tap outside the image is reflected without repeating the edge (-1 -> 1,
 *     W -> W - 2), which keeps the Bayer phase.  The taps are summed as integers and divided once:
 *     (float)sum / (float)(n * 255), or n * 65535.  Needs width >= 2 and height >= 2.
 *  depth, 16UC1: out = [H,W]; d = (float)u16 * depth_scale, byte order honoured.
 *  depth, 32FC1: the float f by its bits, byte order honoured; d = f * depth_scale; d = 0 where f is NaN, +-inf or <= 0.
 *  both depth forms, after the scaling and in float32: d = 0 where d is not a finite value > 0 (raw 0 stays 0, the library's "no
 *     reading"); then d = 0 where d < depth_lo or d > depth_hi (-inf / +inf turn a bound off).
 * No byte at or beyond data_bytes (or in front of data) is ever read.  No allocation, no atomics.  Zero pixels: no launch.
 * Errors before any launch: NULL layout / data / out, an unknown encoding, width * height above 2^30 - 1, a Bayer image below
 * 2 x 2, (depth) a depth_scale that is not finite and > 0 or a NaN bound, step < width * bpp,
 * (height - 1) * step + width * bpp > data_bytes: GSR_ERR_INVALID_ARGUMENT. */
int gsr_image_decode(const gsr_image_layout* layout /*HOST*/, const void* data, size_t data_bytes, float depth_scale, float depth_lo,
                     float depth_hi, float* out /*[3,H,W] or [H,W]*/, void* stream);

/* The inverse for publishing a render: planar [3,H,W] float32 -> interleaved rgb8, step = 3 W (out_bytes: 3 W H device bytes,
 * 4-byte aligned).  byte = (uint8)(min(max(c, 0), 1) * 255.0f): one rounded product, then truncation - what .byte() does in the
 * reference's train.py:80; a NaN gives 0.
 * Errors before the launch: sides < 1, W * H above 2^30 - 1, NULL image / out_bytes, a misaligned out_bytes:
 * GSR_ERR_INVALID_ARGUMENT. */
int gsr_image_encode_rgb8(int32_t W, int32_t H, const float* image /*[3,H,W]*/, void* out_bytes /*[3 W H]*/, void* stream);

/* Move a depth image [Hd,Wd] of the depth camera (intrinsics Kd = fx, fy, cx, cy; HOST) into the colour camera (Kc, Wc x Hc):
 * "aligned depth to colour".  T_cd: HOST float64[12], the row-major 3 x 4 matrix from the depth-camera frame to the colour-camera
 * frame.  Per depth pixel (u, v) with a reading d > 0, for the centre (u, v) and the two pixel corners (u - 0.5, v - 0.5),
 * (u + 0.5, v + 0.5), every step one correctly rounded float32 operation:
 *   x = ((uc - cx_d) / fx_d) * d, y = ((vc - cy_d) / fy_d) * d, z = d;  (x', y', z') = T_cd (x, y, z) as "q = T s" above (products
 *   and sums in float64 in that order, one rounding to float32);  px = fx_c * (x' / z') + cx_c, py = fy_c * (y' / z') + cy_c.
 * The reading is skipped if the centre's z' is not a finite value > 0, or if px or py of either corner is not finite.  Each
 * corner is rounded, floorf(p + 0.5f), and clamped IN FLOAT to [-1, Wc] / [-1, Hc] before the conversion to int.  Every colour
 * pixel of the inclusive rectangle spanned by the two rounded corners (either may be the low one) that lies inside the image
 * takes the MINIMUM of its value and the centre's z' - librealsense's footprint rule; with equal cameras a 2 x 2 splat.  The
 * minimum is an integer atomicMin on the bits of z' (positive floats order as their bits): independent of the order of arrival,
 * bit-exact from run to run.  The part of a rectangle inside the image is cut to its first 8 columns and 8 rows; a cut sets bit 0
 * of status_dev[0] (device int32, cleared by the call).  A pixel no reading reached is 0.  The workspace (one uint32 per colour
 * pixel) is initialised by the call.  No float atomics, no allocation.
 * Errors before any launch: a NULL pointer, a side < 1, Wd * Hd or Wc * Hc above 2^30 - 1, an intrinsic or an entry of T_cd that
 * is not finite, fx or fy <= 0: GSR_ERR_INVALID_ARGUMENT; workspace below gsr_depth_register_workspace_bytes(Wc, Hc):
 * GSR_ERR_STATE_TOO_SMALL. */
size_t gsr_depth_register_workspace_bytes(int32_t Wc, int32_t Hc);
int gsr_depth_register(int32_t Wd, int32_t Hd, const float* depth /*[Hd,Wd]*/, const float* Kd /*HOST [4]*/,
                       const float* Kc /*HOST [4]*/, const double* T_cd /*HOST [12]*/, int32_t Wc, int32_t Hc, float* out /*[Hc,Wc]*/,
                       int32_t* status_dev /*[1]*/, void* workspace, size_t workspace_bytes, void* stream);

/* ---- a LiDAR cloud in the colour camera (csrc/cloud_image.hip): the fourth member of a
 * /Visual_Merged message, Local_Map, joined with the first.  The reference carries the field and has no code for this step: the
 * rules below are this library's own.  Occlusion by a square footprint is the crude, standard form; hidden-point removal by
 * convex hull and per-beam ray tests are not attempted.  Every step is one correctly rounded float32 operation unless stated.
 *
 * PROJECT, per row i of points [N,3] (cloud frame):
 *   q = w2c p as "q = T s" above: per component (float)(((T[k,0] x + T[k,1] y) + T[k,2] z) + T[k,3]), the three products and
 *   three sums each rounded to float64, then one rounding to float32.
 *   The row TAKES PART iff q.x, q.y, q.z are finite and z_near <= q.z <= z_far.
 *   px = fx * (q.x / q.z) + cx, py = fy * (q.y / q.z) + cy;  (u, v) = (floorf(px + 0.5f), floorf(py + 0.5f)), clamped IN FLOAT to
 *   [-(r + 1), W + r] / [-(r + 1), H + r] before the conversion to int (r = footprint).
 *   Every row that takes part OCCLUDES: each pixel of [u - r, u + r] x [v - r, v + r] inside the image takes the minimum of its
 *   word of zocc and the bits of q.z (32-bit integer atomicMin: positive floats order as their bits).
 *   A CANDIDATE is a row that takes part whose (u, v) is inside the image and, with a mask, has mask[v W + u] != 0.  It competes
 *   for its pixel with the 64-bit key (bits(q.z) << 32) | i by integer atomicMin: the nearest wins, on equal z the lowest row.
 *   z[i] = q.z, or 0 for a row that does not take part;  pixel[i] = v W + u for a candidate, else -1.
 * RESOLVE:
 *   a candidate is VISIBLE iff z[i] <= zocc[pixel[i]] * occlusion_scale (one product).  visible[i] = 1 / 0 (0 for every other row).
 *   Per pixel p with winner (z_w, i_w): visible -> depth[p] = z_w, index[p] = i_w;  not visible, or no candidate -> depth[p] = 0,
 *   index[p] = -1.  The winner has the smallest z of its pixel's candidates and the test is monotone in z, so where the winner
 *   is not visible no candidate of that pixel is: index[p] >= 0 exactly where some visible row has pixel == p.
 *   count_dev[0] = visible rows, count_dev[1] = candidates (device int64, cleared by the call; integer atomics).
 *   With image and colors: a visible row gets, per channel plane I, the bilinear sample at (px, py): x0 = floorf(px), tx = px - x0,
 *   likewise y0, ty; the taps x0, x0 + 1, y0, y0 + 1 clamped to the image; top = a + tx * (b - a) on row y0, bot likewise on row
 *   y0 + 1, colour = top + ty * (bot - top).  Rows that are not visible are NOT WRITTEN: one colour array can be painted over
 *   many frames.  image without colors is ignored.
 * The result does not depend on the order of arrival; depth is unchanged under a permutation of the rows.  The workspace (a
 * uint32 and a uint64 per pixel) is initialised by the call.  No float atomics, no allocation.  N == 0: depth = 0, index = -1,
 * counts 0, no per-row launch (points, pixel, z, visible may then be NULL).
 * Errors before any launch: NULL cam / depth / index / count_dev / workspace, NULL points / pixel / z / visible with N > 0, N < 0 or
 * above 2^30 - 1, colors without image, a side < 1 or W H above 2^30 - 1, K or w2c not finite, fx or fy <= 0, not 0 < z_near <
 * z_far < inf, footprint outside 0 .. GSR_CLOUD_MAX_FOOTPRINT, occlusion_scale not a finite value >= 1: GSR_ERR_INVALID_ARGUMENT;
 * workspace below gsr_cloud_project_workspace_bytes(W, H): GSR_ERR_STATE_TOO_SMALL.
 *
 * DENSIFY, per pixel of depth [H,W] (0 = no reading):
 *   depth > 0: dense = depth, valid = 1.  Otherwise, over the (2 radius + 1)^2 window around it (outside the image: no reading):
 *   zn = the smallest reading > 0; none: dense = 0, valid = 0.  The IN-BAND readings are those with 0 < z <= zn * band_scale.
 *   Fewer than min_neighbors of them: dense = 0, valid = 0.  Else dense = (sum w z) / (sum w), valid = 1, with w = 1.0f /
 *   (float)(dx^2 + dy^2) and both sums accumulated in float32 from 0 in row-major window order (s = s + w; t = t + w * z).
 *   The rule prefers the foreground, as gsr_frame_pyramid's depth_band does: a hole beside a depth edge takes the near
 *   surface's depth, never a mix of the two.  valid is float32 1 / 0, what a Frame's mask is.  No atomics, no workspace.
 * Errors before the launch: NULL depth / dense / valid, a side < 1, W H above 2^30 - 1, radius outside 1 ..
 * GSR_DENSIFY_MAX_RADIUS, band_scale not a finite value >= 1, min_neighbors < 1: GSR_ERR_INVALID_ARGUMENT. */
#define GSR_CLOUD_MAX_FOOTPRINT 4
#define GSR_DENSIFY_MAX_RADIUS 8

typedef struct gsr_cloud_camera {   /* HOST struct */
  int32_t width, height;
  float K[4];                       /* fx, fy, cx, cy; centre of pixel (0,0) at (0,0) */
  double w2c[12];                   /* rows 0..2 of the rigid cloud-frame -> camera matrix */
  float z_near, z_far;              /* 0 < z_near < z_far, finite */
  int32_t footprint;                /* r, 0 .. GSR_CLOUD_MAX_FOOTPRINT: a point occludes (2r+1)^2 pixels */
  float occlusion_scale;            /* >= 1, finite: float32(1 + relative margin), formed by the host */
} gsr_cloud_camera;
size_t gsr_cloud_project_workspace_bytes(int32_t W, int32_t H);
int gsr_cloud_project(const gsr_cloud_camera* cam, int64_t N, const float* points /*[N,3]*/,
                      const float* image /*[3,H,W] or NULL*/, const float* mask /*[H,W] or NULL*/, float* depth /*[H,W]*/,
                      int32_t* index /*[H,W]*/, int32_t* pixel /*[N]*/, float* z /*[N]*/, uint8_t* visible /*[N]*/,
                      float* colors /*[N,3] or NULL*/, int64_t* count_dev /*[2]*/, void* workspace, size_t workspace_bytes,
                      void* stream);
int gsr_depth_densify(int32_t W, int32_t H, const float* depth /*[H,W]*/, int32_t radius, float band_scale,
                      int32_t min_neighbors, float* dense /*[H,W]*/, float* valid /*[H,W]*/, void* stream);

/* Back-projection and selection of an RGB-D keyframe.  Pixel centres sit at integer coordinates, as everywhere in this library:
 * ndc = (2 px + 1) / S - 1, p_view = (ndc_x tanfovx d, ndc_y tanfovy d, d), p_world = C2W p_view with C2W the rigid inverse of
 * the view matrix (R^T, -R^T t).  A strided pixel is selected iff its reading is valid and
 *   alpha == NULL: always (first keyframe; `rendered_z` is then ignored);
 *   else: A < alpha_below (the map does not cover it), or - with `rendered_z`, what a render with GSR_DEPTH_Z returns, sum w_i z_i,
 *         not normalised, hence the division by A - d < rendered_z / A - front_margin * d (the reading lies in front of the map).
 * The selected pixels are compacted in ROW-MAJOR pixel order (prefix sum): deterministic.  *count_dev (device int64) receives the
 * number selected; rows beyond `capacity` are dropped, never written.  capacity = ceil(W / stride) ceil(H / stride) cannot overflow.
 * Errors before any launch: NULL p / depth / color / count_dev / workspace / viewmatrix, xyz or rgb NULL with capacity > 0,
 * capacity < 0, sides < 1, stride < 1, tanfov <= 0: GSR_ERR_INVALID_ARGUMENT; workspace too small: GSR_ERR_STATE_TOO_SMALL. */
typedef struct gsr_unproject_params {
  int32_t image_height, image_width;
  float tanfovx, tanfovy;
  const float* viewmatrix;      /* [16] device, the settings' row-major W2C^T */
  int32_t stride;               /* >= 1: pixels with x % stride == 0 && y % stride == 0 */
  float min_depth, max_depth;   /* a reading d is valid iff finite and min_depth < d <= max_depth */
  float alpha_below;
  float front_margin;
} gsr_unproject_params;
size_t gsr_unproject_workspace_bytes(int32_t image_width, int32_t image_height);
int gsr_unproject_rgbd(const gsr_unproject_params* p, const float* depth /*[H,W] view-space z*/, const float* color /*[3,H,W]*/,
                       const float* alpha /*[H,W] or NULL*/, const float* rendered_z /*[H,W] or NULL*/, float* xyz /*[capacity,3]*/,
                       float* rgb /*[capacity,3]*/, int64_t capacity, int64_t* count_dev, void* workspace, size_t workspace_bytes,
                       void* stream);

/* The same call for a camera whose principal point is not the image centre: ox, oy are the offsets the projection matrix carries
 * in P[0,2], P[1,2] - ox = (2 cx - (W - 1)) / W for a principal point cx in pixel-index coordinates (centre of pixel (0,0) at (0,0)),
 * the same for y - and p_view = ((ndc_x - ox) tanfovx d, (ndc_y - oy) tanfovy d, d), each step rounded to float32 on its own.
 * ox = oy = 0 gives the points of gsr_unproject_rgbd bit for bit.  |ox| or |oy| > 1 (or not finite): GSR_ERR_INVALID_ARGUMENT. */
typedef struct gsr_unproject_params_k {
  gsr_unproject_params base;
  float ox, oy;
} gsr_unproject_params_k;
int gsr_unproject_rgbd_k(const gsr_unproject_params_k* p, const float* depth, const float* color, const float* alpha,
                         const float* rendered_z, float* xyz, float* rgb, int64_t capacity, int64_t* count_dev, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ---- sensor frames: undistortion, validity mask, image / depth pyramid (csrc/frames.hip) ---- */

/* Resamples a distorted sensor frame onto an ideal pinhole image, ONE launch.  Intrinsics are HOST arrays K = (fx, fy, cx, cy) in
 * pixels with the centre of pixel (0,0) at (0,0); `dist` HOST (k1, k2, p1, p2, k3), the Brown-Conrady ("plumb_bob") model; `K` ==
 * NULL: the target has the source's K.  Source: `src_color` [3,src_h,src_w], `src_depth` [src_h,src_w] view-space z (0 = no reading)
 * or NULL (then `depth` is not written and may be NULL).  Target: `color` [3,h,w], `depth` [h,w], `mask` [h,w].
 * For the target pixel (u, v), every operation rounded to float32 on its own, in this order (no contraction):
 *   x = (u - cx') / fx',  y = (v - cy') / fy';   x2 = x x,  y2 = y y,  xy = x y,  r2 = x2 + y2;
 *   rho = 1 + r2 (k1 + r2 (k2 + r2 k3))                                   (Horner form of 1 + k1 r^2 + k2 r^4 + k3 r^6);
 *   xd = (x rho + (2 p1) xy) + p2 (r2 + 2 x2),   yd = (y rho + p1 (r2 + 2 y2)) + (2 p2) xy;
 *   us = fx xd + cx,  vs = fy yd + cy.
 * All-zero `dist` with a target K equal to the source K: the map is the identity, us = u, vs = v exactly.
 * mask = 1 iff 0 <= us <= src_w - 1 and 0 <= vs <= src_h - 1, i.e. the bilinear taps x0 = floor(us), x1 = ceil(us), y0 = floor(vs),
 * y1 = ceil(vs) all lie inside the source (on an integer coordinate the taps coincide); elsewhere - a coordinate that overflowed
 * to inf or NaN included - mask, colour and depth are 0.
 * colour: ax = us - x0, ay = vs - y0;  top = c(y0,x0) + ax (c(y0,x1) - c(y0,x0)),  bot = the same on row y1,  out = top + ay (bot - top)
 *   - at integer coordinates the source pixel, bit for bit.
 * depth: the source value at (floor(us + 0.5), floor(vs + 0.5)) - the nearest pixel, halves rounded up; never blended; z-depth is
 *   what undistortion leaves unchanged, so the value is copied (0 stays 0).
 * No atomics, nothing read back.  Errors before the launch, GSR_ERR_INVALID_ARGUMENT: a NULL src_color / src_K / dist / color / mask,
 * src_depth without depth, a side < 1 or more than 2^30 pixels, a focal length that is not > 0, a coefficient that is not finite. */
int gsr_frame_undistort(int32_t src_w, int32_t src_h, const float* src_color, const float* src_depth, const float* src_K,
                        const float* dist, int32_t w, int32_t h, const float* K, float* color, float* depth, float* mask,
                        void* stream);

/* Levels 1 .. `levels` (<= 3) of the pyramid of an image [3,h,w], its depth [h,w] (or NULL) and its mask [h,w] (or NULL), ONE launch:
 * level l is w_l x h_l = (w_(l-1) / 2) x (h_(l-1) / 2), integer division - a trailing odd row or column is dropped - and its pixel
 * (X, Y) comes from the quad a = (2X, 2Y), b = (2X+1, 2Y), c = (2X, 2Y+1), d = (2X+1, 2Y+1) of the level below:
 *   colour  ((a + b) + (c + d)) 0.25, float32, in that order;
 *   depth   the valid readings are those > 0 and < +inf (so NaN, -0.0, negative readings and +inf are not; a denormal is); m = the
 *           smallest; the result is the mean of the valid readings <= m (1 + depth_band) (1 + depth_band rounded once, the
 *           product rounded once; m itself always is one; a reading equal to the product is inside), summed in the order a, b,
 *           c, d and divided by their count, every step in float32; 0 if none is valid: the near surface survives at a depth
 *           edge, a hole does not pull a reading towards 0.  A quad whose only readings > 0 are +inf gives 0, as a quad without a
 *           valid reading does, and +inf never enters a mean - not beside finite readings, and not when depth_band is so large
 *           that the product overflows (then every finite valid reading is taken);
 *   mask    1 iff all four are exactly 1, else 0 (0.5, 2 and NaN give 0).
 * A workgroup reads one 32 x 32 block of level 0 once and writes its part of every level (coarser levels reduced through LDS).
 * color_out / depth_out / mask_out: HOST arrays of `levels` device pointers (level 1 first); depth_out / mask_out may be NULL where
 * the input is.  Errors before the launch, GSR_ERR_INVALID_ARGUMENT: levels outside 1 .. 3, a level whose side would reach 0
 * (w >> levels or h >> levels == 0), NULL color / color_out or a NULL entry, depth without depth_out (mask alike),
 * depth_band not >= 0. */
int gsr_frame_pyramid(int32_t w, int32_t h, int32_t levels, const float* color, const float* depth, const float* mask,
                      float depth_band, float* const* color_out, float* const* depth_out, float* const* mask_out, void* stream);

/* ---- tracking: the camera pose as an SE(3) correction, on the device ---- */

/* The pose of a tracking iteration is W2C' = exp(tau) W2C: `base_w2c` [16] the row-major 4x4 world-to-camera matrix (column-
 * vector convention), `tau` [6] = (rho, theta) the twist [[hat(theta), rho], [0, 0]] applied on the left, `proj_T` [16] the
 * TRANSPOSED projection matrix.  All three are float64 in DEVICE memory and the arithmetic is float64; one single-wave launch each
 * way, no atomics, bitwise reproducible.
 * gsr_pose_forward writes the three float32 tensors of gsr_settings: viewmatrix = T^T, projmatrix = T^T proj_T, campos = -R^T t of
 * T = exp(tau) base_w2c.  exp: R = I + A K + B K^2, V = I + B K + C K^2 (K = hat(theta), A = sin t / t, B = (1 - cos t) / t^2,
 * C = (t - sin t) / t^3); where |theta|^2 < 1e-6 the Taylor polynomials in |theta|^2 up to the second order, else the closed
 * forms with 1 - cos t = 2 sin^2(t / 2).
 * gsr_pose_backward takes the gradients of those three tensors (float32, each may be NULL = zero: what gsr_backward_camera*
 * returns) and writes dL/dtau [6] (float64; may be NULL when `adam` is given), exact at any tau.
 * adam: NULL, or a gsr_pose_adam in DEVICE memory: the same launch then applies one torch.optim.Adam step (bias correction, no
 * weight decay, no amsgrad) to `tau` IN PLACE with the stored learning rate, then multiplies the stored learning rate by lr_decay
 * and increments the stored step - nothing per step comes from the host.  Every member is 8 bytes wide: a caller may keep the
 * struct as 18 consecutive 64-bit words. */
typedef struct gsr_pose_adam {
  double exp_avg[6];
  double exp_avg_sq[6];
  double lr;        /* learning rate of the NEXT step; multiplied by lr_decay after each */
  double beta1, beta2, eps;
  double lr_decay;
  int64_t step;     /* steps taken so far */
} gsr_pose_adam;
int gsr_pose_forward(const double* base_w2c, const double* tau, const double* proj_T, float* viewmatrix, float* projmatrix,
                     float* campos, void* stream);
int gsr_pose_backward(const double* base_w2c, double* tau, const double* proj_T, const float* dL_dviewmatrix,
                      const float* dL_dprojmatrix, const float* dL_dcampos, double* dL_dtau, gsr_pose_adam* adam, void* stream);

/* ---- per-view exposure: the affine colour correction of a training view and its alpha mask ---- */

/* out[j,p] = m[p] ( sum_k E[k][j] I[k,p] + E[j][3] ): `image` / `out` [3,n] planar (n = H W), `exposure` E [3,4] row-major in
 * DEVICE memory, `mask` [n] or NULL (= 1).  The index convention is the reference's (gaussian_renderer/__init__.py:141-144: the
 * 3x3 part multiplies the pixel from the right, the bias of channel j is E[j][3]) times the alpha mask of train.py:109-111.  One
 * elementwise launch; 16-byte accesses when n % 4 == 0 and every tensor is 16-byte aligned, 4-byte accesses otherwise.
 * gsr_exposure_backward: dL_dimage[k,p] = m[p] sum_j E[k][j] dL_dout[j,p] (NULL: not formed) and, when `dL_dexposure` or `adam`
 * is given, the twelve sums dE[k][j] = sum_p m I[k] g[j], dE[j][3] = sum_p m g[j] ([3,4] row-major): per-workgroup partial sums
 * in `partials` (12 gsr_exposure_blocks() floats of scratch), added by one workgroup in index order - no float atomics, bitwise
 * reproducible.  `dL_dexposure` [12] may be NULL when `adam` is given.
 * adam: NULL, or a gsr_exposure_adam in DEVICE memory: this header followed by float exp_avg[12 views] and float
 * exp_avg_sq[12 views].  The finalize launch then applies one torch.optim.Adam step (bias correction from the stored step count,
 * no weight decay, no amsgrad) IN PLACE to all of `exposures` [views,3,4] - of which `exposure` is row `row` - with the twelve
 * sums as the gradient of row `row` and zero for every other row (their moments decay and keep moving them, as under a dense
 * optimizer), and increments the stored step; lr, beta1, beta2 and eps are this step's hyper-parameters (ignored without `adam`).
 * Nothing is read back by the host in either direction. */
typedef struct gsr_exposure_adam {
  int64_t step;     /* steps taken so far */
  int64_t reserved; /* zero; keeps the moments that follow 16-byte aligned */
} gsr_exposure_adam;
int32_t gsr_exposure_blocks(void);
int gsr_exposure_forward(int64_t n, const float* image, const float* exposure, const float* mask, float* out, void* stream);
int gsr_exposure_backward(int64_t n, const float* image, const float* exposure, const float* mask, const float* dL_dout,
                          float* dL_dimage, float* partials, float* dL_dexposure, float* exposures, int32_t views, int32_t row,
                          gsr_exposure_adam* adam, double lr, double beta1, double beta2, double eps, void* stream);

/* ---- map maintenance: Gaussians follow the pose corrections of their keyframes ---- */

/* Moves rows of the model into a corrected world frame, in place.  `transforms` [K,4,4] row-major float64 in DEVICE memory, each
 * x' = s R x + t: upper-left block s R with R a proper rotation and s > 0, last column t, bottom row (0, 0, 0, 1) - trusted, not
 * checked.  `anchor` int32 [P]: row i moves by transform anchor[i]; a value < 0 or >= K leaves the row untouched - nothing is
 * written to it.  anchor == NULL: every row moves by transform 0.  A row that moves:
 *   xyz            s R x + t, formed in float64 from the float32 input and rounded once;
 *   rotation       (raw quaternion, w x y z) q' = q_R (x) q, the Hamilton product with the unit quaternion of R (norm preserved);
 *   scaling_raw    (log-scale) + ln s; NULL: skipped;
 *   features_rest  [P, sh_coeffs_rest, 3], sh_coeffs_rest in {0, 3, 8, 15}: SH bands 1..3 are expressed in the world frame, so per
 *                  channel and band c'_l = D_l(R) c_l with the band's (2 l + 1)^2 real-SH rotation matrix (basis and signs of the
 *                  reference's utils/sh_utils.py); may be NULL when sh_coeffs_rest == 0;
 *   moments8       NULL, or a HOST array of eight device pointers, each of which may be NULL: exp_avg, exp_avg_sq of xyz, of rotation,
 *                  of scaling, of features_rest (shapes of their parameters).  The moved rows get zeros - their moments describe
 *                  gradients in the old frame -, the other rows are not written.
 * features_dc and opacity are invariant and not arguments.  `workspace`: gsr_transform_workspace_bytes(K) bytes, holds the
 * per-transform table (s, R, t, quaternion, ln s, D_1..D_3; float64 arithmetic, one lane per transform); its layout is private.
 * Two launches, no atomics, bitwise reproducible, nothing read back.  P == 0 or K == 0 launches nothing.
 * Errors, all before any device work, all GSR_ERR_INVALID_ARGUMENT: sh_coeffs_rest outside {0, 3, 8, 15}; P < 0 or > 2^31 - 1,
 * K < 0; workspace NULL or too small (K > 0); xyz NULL (P > 0); transforms, rotation or a needed features_rest NULL; rotation,
 * features_rest, their moments or the workspace not 16-byte aligned. */
size_t gsr_transform_workspace_bytes(int32_t K);
int gsr_transform_gaussians(int64_t P, const int32_t* anchor, int32_t K, const double* transforms, void* workspace,
                            size_t workspace_bytes, float* xyz, float* rotation, float* scaling_raw, float* features_rest,
                            int32_t sh_coeffs_rest, float* const* moments8, void* stream);

/* ---- TSDF fusion: depth frames into a block-sparse signed distance volume, out as a cloud and a mesh (csrc/tsdf.hip; DESIGN.md
 * section 4 item 38) ----
 *
 * THE VOLUME.  Voxels have edge voxel_size; a block is 8 x 8 x 8 voxels and is named by its signed integer coordinate (bx, by, bz),
 * each in -2^20 .. 2^20 - 1.  key = ((bx + 2^20) << 42) | ((by + 2^20) << 21) | (bz + 2^20), an int64 >= 0: key order is block order,
 * x highest.  Voxel (lx, ly, lz) of a block has the linear index lx + 8 ly + 64 lz and the global integer coordinate g = 8 b + l; its
 * centre is origin + (g + 0.5) voxel_size.  The float32 world position of a centre is a function of g alone: per axis
 * float32(origin_a + (g_a + 0.5) * voxel_size) with the product and the sum each rounded to float64 (no fused multiply-add) and ONE
 * rounding to float32 - two blocks that name the same centre produce the same bits.
 * Storage, owned by the caller: rows in allocation order, append-only - tsdf [B,512], weight [B,512], color [B,512,3] float32, zero
 * when allocated; beside them keys_sorted int64 [B] (strictly ascending) and row_of_sorted int32 [B] (the row of each sorted key).  A
 * block is found by binary search in keys_sorted.  B <= GSR_TSDF_MAX_BLOCKS.
 * A FRAME is depth [H,W] (view-space z, 0 = no reading), mask [H,W] (NULL: every pixel; else pixels with mask != 0), color [3,H,W]
 * (NULL: colours are not touched), K = (fx, fy, cx, cy) in float32 pixels (centre of pixel (0, 0) at (0, 0)) and `w2c`, HOST
 * float64[12]: the first three rows of the rigid world-to-camera matrix, row-major (x_cam = R x_world + t; rigidity is trusted).
 *
 * TOUCH.  Every pixel with mask != 0 and 0 < depth <= depth_trunc is unprojected, p = R^T (((u - cx) / fx d, (v - cy) / fy d, d) - t),
 * in float64; every block that intersects the axis-aligned box p +- sdf_trunc is touched: per axis the blocks
 * floor((p_a - sdf_trunc - origin_a) / (8 voxel_size)) .. floor((p_a + sdf_trunc - origin_a) / (8 voxel_size)).  voxel_size <=
 * sdf_trunc <= 8 voxel_size, so these are at most 3 per axis.  gsr_tsdf_touch writes 27 candidate keys per pixel, slot-major
 * (keys_out int64 [27, H W]); unused slots, and blocks outside the coordinate range, hold GSR_TSDF_NO_KEY.  The caller uniques them,
 * merges them into keys_sorted and appends zeroed rows.
 *
 * INTEGRATE.  One workgroup per touched block (`keys`, `rows` [n]: its key and its row), 256 lanes, voxels lane and lane + 256.  The
 * camera-space position of the centre of voxel (0, 0, 0) of the block, c = R (origin + (8 b + 0.5) voxel_size) + t, is formed in
 * float64 and rounded to float32; the steps a_k = float32(R[:,k] voxel_size) likewise; the voxel's camera-space position is
 * (x, y, z) = c + lx a_0 + ly a_1 + lz a_2 in float32 - its error does not grow with the distance from the world origin.  With z > 0:
 * u = fx x / z + cx, v = fy y / z + cy; the pixel is (floor(u + 0.5), floor(v + 0.5)), inside the image, with mask != 0; d = its
 * depth, 0 < d <= depth_trunc; sdf = (d - z) sqrt(1 + (x/z)^2 + (y/z)^2), the distance along the ray; sdf <= -sdf_trunc: skipped;
 * f = min(1, sdf / sdf_trunc); tsdf <- (tsdf w + f) / (w + 1), each colour channel likewise from the pixel's colour;
 * w <- min(w + 1, max_weight) (max_weight >= 1).  A voxel is read and written by exactly one lane; no LDS, no atomics.
 *
 * SURFACE POINTS.  Voxel i is observed when weight > min_weight.  An edge runs from an observed voxel i to its +x, +y or +z
 * neighbour j (possibly in the next block), also observed, where exactly one of the two has tsdf < 0.  With lo = i, hi = j (lo is
 * the endpoint with the smaller global coordinate) and t = f_lo / (f_lo - f_hi), float32: point = p_lo + t (p_hi - p_lo) on the
 * float32 centres; colour interpolated the same way; normal = normalise(g_lo + t (g_hi - g_lo)), g the gradient of tsdf in voxel
 * units: per axis (f+ - f-) / 2 when both neighbours are observed, f+ - f0 or f0 - f- when one is, 0 when none is.  The normal
 * points toward positive tsdf (where the cameras were); a zero vector stays (0, 0, 0).  Output order: blocks in key order, voxels in
 * linear order, axes x, y, z.
 *
 * TRIANGLES.  Marching tetrahedra.  The cube of voxel g has the corners g + (c & 1, (c >> 1) & 1, c >> 2), c = 0 .. 7, and is used
 * when all eight are observed.  It is split into the six Kuhn tetrahedra around the diagonal corner 0 -> corner 7: for each order
 * (a, b, c) of the axes - xyz, xzy, yxz, yzx, zxy, zyx, in this order - the tetrahedron (v0, v0 + e_a, v0 + e_a + e_b, v7).  Every
 * cube face is cut along the diagonal from its lowest to its highest corner.  "Inside" is tsdf < 0: 1 or 3 inside corners give one
 * triangle, 2 give two (the quad AC, AD, BD, BC of inside A < B and outside C < D in path order, cut along AC - BD: both triangles start with AC; the triangle of a single corner k starts with the edge to the lowest
 * other corner).  The vertex on
 * the edge of two corners is p_lo + t (p_hi - p_lo) as above, lo the corner earlier on the path (smaller in every coordinate), so
 * every cube and tetrahedron that shares an edge produces the same bits.  Triangles are wound so that the right-hand normal points
 * toward positive tsdf.  Output: triangle soup, positions [T,3,3] and colours [T,3,3]; order: block key, voxel, tetrahedron, triangle.
 *
 * The extract calls take an output capacity and report the count they needed in count_dev[0] (device int64); rows beyond the
 * capacity are never written; capacity == 0 with NULL outputs counts only.  Two launches and one scan each; deterministic.
 * Every call checks its arguments before any device work (GSR_ERR_INVALID_ARGUMENT; a short workspace GSR_ERR_STATE_TOO_SMALL):
 * NULL or non-finite volume fields, voxel_size <= 0, sdf_trunc outside [voxel_size, 8 voxel_size], depth_trunc <= 0, max_weight < 1,
 * an image side < 1 or W H > 2^26, fx or fy <= 0, non-finite K / w2c, NULL depth, a block count < 0 or > GSR_TSDF_MAX_BLOCKS, NULL
 * arrays where the count is > 0, a negative capacity, outputs NULL with capacity > 0, min_weight negative or NaN.  A block count
 * of 0 launches nothing (the extract calls then write count 0). */
#define GSR_TSDF_BLOCK 8
#define GSR_TSDF_BLOCK_VOXELS 512
#define GSR_TSDF_TOUCH_SLOTS 27
#define GSR_TSDF_MAX_BLOCKS (1 << 19)
#define GSR_TSDF_NO_KEY INT64_MAX

typedef struct gsr_tsdf_volume {   /* HOST struct */
  double origin[3];
  double voxel_size;
  float sdf_trunc, depth_trunc, max_weight, reserved;
} gsr_tsdf_volume;

typedef struct gsr_tsdf_frame {    /* HOST struct; depth / mask / color are device pointers */
  int32_t width, height;
  float K[4];
  double w2c[12];
  const float* depth;
  const float* mask;
  const float* color;
} gsr_tsdf_frame;

int gsr_tsdf_touch(const gsr_tsdf_volume* vol, const gsr_tsdf_frame* frame, int64_t* keys_out /*[H W 27]*/, void* stream);
int gsr_tsdf_integrate(const gsr_tsdf_volume* vol, const gsr_tsdf_frame* frame, int64_t n_blocks, const int64_t* keys /*[n]*/,
                       const int32_t* rows /*[n]*/, int64_t n_rows, float* tsdf, float* weight, float* color, void* stream);
size_t gsr_tsdf_extract_workspace_bytes(int64_t B);
int gsr_tsdf_extract_points(const gsr_tsdf_volume* vol, int64_t B, const int64_t* keys_sorted, const int32_t* row_of_sorted,
                            const float* tsdf, const float* weight, const float* color, float min_weight, int64_t capacity,
                            float* points /*[cap,3]*/, float* normals /*[cap,3]*/, float* colors /*[cap,3]*/,
                            int64_t* count_dev /*[1]*/, void* workspace, size_t workspace_bytes, void* stream);
int gsr_tsdf_extract_triangles(const gsr_tsdf_volume* vol, int64_t B, const int64_t* keys_sorted, const int32_t* row_of_sorted,
                               const float* tsdf, const float* weight, const float* color, float min_weight, int64_t capacity,
                               float* positions /*[cap,3,3]*/, float* colors /*[cap,3,3]*/, int64_t* count_dev /*[1]*/,
                               void* workspace, size_t workspace_bytes, void* stream);

/* Per-kernel timing with HIP events on the launch stream (used by bench.py's roofline block).  A measurement aid, process-
 * global and meant for ONE host thread driving the library at a time: enabling it while several host threads launch
 * concurrently attributes times correctly per thread (the open event pair is thread-local) but adds a lock to every launch. */
void gsr_profile_enable(int32_t on);
void gsr_profile_reset(void);
/* Fills up to `max` entries; returns the number of distinct kernels.  `names` receives pointers to
 * static strings. */
int32_t gsr_profile_read(const char** names, double* total_ms, int64_t* calls, int32_t max);

#ifdef __cplusplus
}
#endif
#endif /* GSR_H_ */
