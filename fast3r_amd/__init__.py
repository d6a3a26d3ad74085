"""fast3r_amd: the Fast3R single-forward-pass inference hot path, MI355X-native (hand-written HIP for gfx950 behind
the reference's Python API).  See DESIGN.md."""
from .fast3r import Fast3R  # noqa: F401
from .inference_multiview import inference  # noqa: F401
from .multiview_dust3r_module import MultiViewDUSt3RLitModule  # noqa: F401
from .align import align_local_pts3d_to_global  # noqa: F401
from .focal import estimate_focal, estimate_focals  # noqa: F401
from .pose import estimate_camera_poses, estimate_poses  # noqa: F401
from .image import load_images  # noqa: F401
from .recon_metric import accuracy, completion, completion_ratio, estimate_normals, nearest_neighbors  # noqa: F401
from .cam_pose_metric import calculate_auc, camera_pose_metrics, camera_to_rel_deg  # noqa: F401
from .depth_metric import depth_metrics, evaluate_multiview_depth  # noqa: F401
from .matching import ViewMatches, find_reciprocal_matches, match_views, scene_graph_pairs  # noqa: F401
from .clean import CleanedCloud, clean_confidences, clean_pointcloud  # noqa: F401
from .global_align import (GlobalAlignerMode, Observations, PointCloudOptimizer, alignment_loss, global_aligner,  # noqa: F401
                           pairs_from_passes)
from .losses import ConfLossMultiviewV2, L21, L21Loss, Regr3DMultiviewV3, Regr3DMultiviewV4  # noqa: F401
from .scene import Scene, assemble_scene, generate_ply_bytes, save_ply  # noqa: F401
from .mesh import Mesh, build_mesh, cat_meshes, generate_mesh_ply_bytes, pts3d_to_trimesh, save_mesh_ply  # noqa: F401
from .cloud import combine_points, downsample_cloud, export_combined_ply, farthest_point_down_sample, voxel_down_sample  # noqa: F401
from .sky import detect_sky_mask, detect_sky_masks, label_components  # noqa: F401
from .render import Camera, birdseye_camera, pinhole_camera, render_cumulative_pts3d_viz, render_points  # noqa: F401
from .viz import (CAM_COLORS, SceneViz, auto_cam_size, camera_meshes, plot_3d_points_with_estimated_camera_poses,  # noqa: F401
                  render_mesh)
from .maps import (colorize_maps, maybe_plot_local_depth_and_conf, plot_confidence_maps, plot_rgb_images,  # noqa: F401
                   save_pointmaps_and_camera_parameters_to_folder)
from .gt_views import (build_gt_views, crop_resize_if_necessary, depthmap_to_absolute_camera_coordinates,  # noqa: F401
                       depthmap_to_camera_coordinates)
