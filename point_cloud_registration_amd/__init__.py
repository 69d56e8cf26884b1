"""MI355X-native drop-in for the registration hot path of scomup/point-cloud-registration.

Same public names as the reference's ``point_cloud_registration/__init__.py:1-10``: the O(N) work
of ``set_target`` / ``calc_H_g_e2`` / ``align`` and of the Gauss-Newton coresets
(``create_gn_set`` / ``fast_caratheodory``) runs in hand-written HIP kernels for gfx950 behind
a C ABI (include/pcr.h); there is no CPU fallback.
"""

from .registration import Registration
from .math_tools import (makeRt, expSO3, makeT, skews, huber_weight, plus, transform_points,
                         skew_time_vector, skew, skew2, robust_weight, trim_threshold)
from .voxelized_plane_icp import VPlaneICP
from .plane_icp import PlaneICP
from .icp import ICP
from .ndt import NDT
from .gicp import GICP
from .vgicp import VGICP
from .symmetric_icp import SymmetricICP
from .colored_icp import ColoredICP
from .kdtree import KDTree
from .voxel import VoxelGrid, voxel_filter, color_by_voxel, get_keys
from .estimate_normals import estimate_normals, get_norm_lines, estimate_norm_with_tree, ball_moments
from .caratheodory import fast_caratheodory, create_gn_set
from .outliers import remove_radius_outliers, remove_statistical_outliers
from .features import compute_fpfh, compute_fpfh_rows, match_features, select_matches
from .keypoints import iss_keypoints
from .global_registration import (score_poses, fit_rigid, ransac_pose, fgr_pose, register_global, match_compatibility,
                                  sc2_pose)

__all__ = [
    "Registration", "ICP", "PlaneICP", "VPlaneICP", "NDT", "GICP", "VGICP", "SymmetricICP", "ColoredICP", "KDTree", "VoxelGrid", "voxel_filter",
    "color_by_voxel", "get_keys", "estimate_normals", "get_norm_lines", "estimate_norm_with_tree",
    "makeRt", "expSO3", "makeT", "skews", "huber_weight", "plus", "transform_points",
    "skew_time_vector", "skew", "skew2", "fast_caratheodory", "create_gn_set",
    "remove_radius_outliers", "remove_statistical_outliers", "compute_fpfh", "match_features", "select_matches",
    "score_poses", "fit_rigid", "ransac_pose", "fgr_pose", "register_global", "iss_keypoints", "compute_fpfh_rows",
    "robust_weight", "trim_threshold", "match_compatibility", "sc2_pose", "ball_moments",
]
