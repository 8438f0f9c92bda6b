"""Host-side helpers around the rasterizer path: camera conventions and synthetic scenes."""
from .cameras import MiniCam, camera_from_RT, look_at_camera, fibonacci_cameras, fov2focal, focal2fov, \
    world_to_view, projection_matrix, camera_projection, camera_from_intrinsics, camera_intrinsics, scaled_camera
from .synthetic import RawGaussians, make_gaussians, make_config, CONFIGS
from .model import GaussianModel
from .sh import eval_sh, RGB2SH, SH2RGB
from .losses import l1_loss, psnr, training_loss_fused
from .parallel import init_from_env, shard_views, GradBucket, ShardedStep, reduce_densification_stats, \
    rank1_sh_exchange, exchange_bytes_per_gaussian
from .trainer import Trainer
from .io import save_ply, load_ply, read_ply_vertices, capture, restore, save_mesh_ply, read_mesh_ply
from .pose import se3_exp, PoseCamera, refine_pose, pose_error, DevicePoseCamera, track_pose
from .mapping import unproject_rgbd, create_from_pcd, add_from_rgbd
from .keyframes import covisibility, KeyframeWindow, prune_unobserved
from .exposure import apply_exposure
from .transform import transform_camera, correct_keyframes, validate_transforms
from .frames import Frame, FramePyramid, undistort, build_pyramid
from .pointcloud import voxel_down_sample, statistical_outlier_mask, remove_statistical_outliers, condition_point_cloud, \
    estimate_normals, estimate_color_gradients
from .registration import NeighborIndex, RegistrationResult, nn_search, transform_points, icp_update, evaluate_registration, \
    registration_icp, register_and_merge, align_map, compute_fpfh_feature, feature_nn, match_features, \
    registration_ransac_based_on_feature_matching, global_registration, ransac_trials, registration_colored_icp, \
    registration_multiscale
from .gicp import estimate_covariances, regularize_covariances, gicp_update, registration_generalized_icp, register_scan_to_map
from .messages import PointField, PointCloud2, decode_pointcloud2, pose_matrix, process_pointcloud, accumulate_pointclouds, \
    encode_pointcloud2, Image, CameraInfo, decode_image, encode_image, camera_info_intrinsics, pose_from_transform, register_depth, \
    frame_from_messages, frame_from_visual_merged
from .odometry import OdometryLevel, OdometryResult, prepare_odometry_level, odometry_update, rgbd_odometry, \
    camera_after_odometry
from .posegraph import PoseGraph, PoseGraphResult, information_from_point_clouds
from .tsdf import TSDFVolume, fuse_views, weld_triangles
from .features2d import OrbFeatures, PlaceEntry, PlaceDatabase, detect_orb, match_descriptors, hamming_match, keypoint_points, \
    relative_pose_from_features, loop_closure_edge, orb_prepare, orb_detect, orb_describe
from .lidar import CloudProjection, project_cloud, densify_depth, colorize_cloud, lidar_frame, frame_from_visual_merged_map
from .scancontext import ScanContext, ScanEntry, ScanDatabase, scan_context, scan_context_distance, scan_loop_closure_edge
