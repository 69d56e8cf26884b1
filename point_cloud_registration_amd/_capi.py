"""ctypes binding of libpcr_hip.so (include/pcr.h) -- the only way the Python host reaches the GPU.

There is NO CPU fallback: if the HIP library is missing or no MI355X is visible, the calls
raise.  (The CPU restatement under oracle/ is test infrastructure and is never imported here.)
"""

import atexit
import ctypes as C
import os
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# PCR_LIB: developer switch, another build of the same library: libpcr_hip_dev.so (`make dev`: + the developer / A-B
# kernels of csrc/kernels_dev.hip), or an experimental variant (tools/build_variant.sh)
LIB_PATH = os.environ.get("PCR_LIB") or os.path.join(_HERE, "libpcr_hip.so")
DEV_LIB_PATH = os.path.join(_HERE, "libpcr_hip_dev.so")

PCR_OK = 0
PCR_ERR_INVALID, PCR_ERR_HIP, PCR_ERR_NO_TARGET, PCR_ERR_COMM, PCR_ERR_SINGULAR, PCR_ERR_NOMEM = -1, -2, -3, -4, -5, -6
PCR_ERR_UNSUPPORTED = -7
ICP, PLANE, VPLANE, NDT = 0, 1, 2, 3
FLAG_ICP_RR_QUIRK = 1
FLAG_NO_SCAN_SORT = 2
FLAG_LOCAL_ONLY = 4          # no all-reduce even when the context has a communicator
FLAG_HOST_LOOP = 8           # pcr_align: host-driven loop instead of the device-resident one
FLAG_DEVICE_LOOP = 16        # pcr_align: device-resident loop even for small scans (where the host-driven one is picked)
FLAG_KEEP_ORDER = 32         # pcr_scan_create: a sorted scan remembers the caller's point order (rows, weighted sums, coresets)
K_LINEARIZE, K_FINALIZE, K_NN, K_REDUCE, K_ALLREDUCE, K_CERTIFY, K_COUNT = 0, 1, 2, 3, 4, 5, 6
KERNEL_NAMES = ("linearize", "finalize", "nn", "reduce", "allreduce", "certify")
NN_FULL, NN_TRACK, NN_LIST = 0, 1, 2      # what the search of a pass did (certified reuse, include/pcr.h)
COV_PLANE, COV_RAW = 0, 1                 # GICP covariance modes (include/pcr.h)

_lib = None
_torch_lib_dir = None           # set when torch's bundled HIP runtime was pre-loaded (see below)
_live = weakref.WeakSet()      # targets / scans still holding device memory
_live_groups = weakref.WeakSet()   # pcr_groups (worker threads + member contexts)
_groups = {}
_shutdown = False

_f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
_f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
_i64p = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
_u32p = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
_i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
_u8p = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")
_vp = C.c_void_p

# name -> (restype, argtypes); also the list of symbols the library must export
PROTOTYPES = {
    "pcr_last_error": (C.c_char_p, []),
    "pcr_version": (C.c_char_p, []),
    "pcr_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "pcr_context_create": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "pcr_context_destroy": (C.c_int, [_vp]),
    "pcr_context_stream": (C.c_int, [_vp, C.POINTER(_vp)]),
    "pcr_context_synchronize": (C.c_int, [_vp]),
    "pcr_comm_unique_id": (C.c_int, [C.c_char_p]),
    "pcr_comm_init": (C.c_int, [_vp, C.c_char_p, C.c_int, C.c_int]),
    "pcr_comm_destroy": (C.c_int, [_vp]),
    "pcr_comm_p2p_export": (C.c_int, [_vp, C.c_char_p]),
    "pcr_comm_p2p_attach": (C.c_int, [_vp, C.c_char_p, C.c_int, C.c_int]),
    "pcr_comm_p2p_failed": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "pcr_target_points_create": (C.c_int, [_vp, _vp, C.c_int64, _vp, C.c_float, C.POINTER(_vp)]),
    "pcr_target_points_create_device": (C.c_int, [_vp, _vp, C.c_int64, _vp, C.c_float, C.POINTER(_vp)]),
    "pcr_target_set_normals": (C.c_int, [_vp, _f32p]),
    "pcr_target_points_set_f64": (C.c_int, [_vp, _f64p]),
    "pcr_target_estimate_normals": (C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    "pcr_target_get_normals": (C.c_int, [_vp, _f32p]),
    "pcr_target_voxels_create": (C.c_int, [_vp, _vp, C.c_int, C.c_int64, C.c_double, C.c_int, C.POINTER(_vp)]),
    "pcr_target_voxels_create_from_stats": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int64, C.c_double, C.POINTER(_vp)]),
    "pcr_target_voxels_get": (C.c_int, [_vp, C.POINTER(C.c_int64), _vp, _vp, _vp, _vp, _vp, _vp]),
    "pcr_target_size": (C.c_int, [_vp, C.POINTER(C.c_int64)]),
    "pcr_target_destroy": (C.c_int, [_vp]),
    "pcr_scan_create": (C.c_int, [_vp, _vp, C.c_int64, C.c_uint, C.POINTER(_vp)]),
    "pcr_scan_create_device": (C.c_int, [_vp, _vp, C.c_int64, C.c_uint, C.POINTER(_vp)]),
    "pcr_scan_size": (C.c_int, [_vp, C.POINTER(C.c_int64)]),
    "pcr_scan_destroy": (C.c_int, [_vp]),
    "pcr_linearize": (C.c_int, [_vp, _vp, C.c_int, _f64p, C.c_double, C.c_uint, _f64p]),
    "pcr_align": (C.c_int, [_vp, _vp, C.c_int, _f64p, C.c_int, C.c_double, C.c_double, C.c_uint, _f64p,
                            C.POINTER(C.c_int), _vp]),
    "pcr_nn_query": (C.c_int, [_vp, _f32p, C.c_int64, C.c_float, _f32p, _i64p]),
    "pcr_nn_query_f64": (C.c_int, [_vp, _f32p, C.c_int64, C.c_double, _f64p, _i64p]),
    "pcr_knn_query": (C.c_int, [_vp, _f32p, C.c_int64, C.c_int, _f32p, _i64p]),
    "pcr_nn_query_dd": (C.c_int, [_vp, _f64p, C.c_int64, C.c_double, _f64p, _i64p]),
    "pcr_knn_query_f64": (C.c_int, [_vp, _f64p, C.c_int64, C.c_int, _f64p, _i64p]),
    # fixed-radius search and the mean k-NN distance (include/pcr.h, outliers.py)
    "pcr_radius_count": (C.c_int, [_vp, _f32p, C.c_int64, C.c_float, _i64p]),
    "pcr_radius_query": (C.c_int, [_vp, _f32p, C.c_int64, C.c_float, _i64p, _f32p, _i64p]),
    "pcr_radius_count_dd": (C.c_int, [_vp, _f64p, C.c_int64, C.c_double, _i64p]),
    "pcr_radius_query_dd": (C.c_int, [_vp, _f64p, C.c_int64, C.c_double, _i64p, _f64p, _i64p]),
    "pcr_knn_mean_distance": (C.c_int, [_vp, C.c_int, _f64p]),
    # FPFH descriptors and exact feature matching (include/pcr.h, features.py)
    "pcr_target_spfh": (C.c_int, [_vp, C.c_float, _u32p, _i64p]),
    "pcr_target_fpfh": (C.c_int, [_vp, C.c_float, _f32p, _vp]),
    "pcr_feature_match": (C.c_int, [_vp, _f32p, C.c_int64, _f32p, C.c_int64, C.c_int, _i64p, _f32p, _f32p]),
    "pcr_target_fpfh_rows": (C.c_int, [_vp, C.c_float, _i64p, C.c_int64, _f32p, _vp]),
    # ISS keypoints (include/pcr.h, keypoints.py)
    "pcr_target_iss_saliency": (C.c_int, [_vp, C.c_float, C.c_double, C.c_double, C.c_int, _f64p, _f64p, _i64p]),
    "pcr_target_iss_keypoints": (C.c_int, [_vp, C.c_float, C.c_float, C.c_double, C.c_double, C.c_int, _u8p, _vp]),
    # radius and hybrid neighbourhoods for normals and covariances (include/pcr.h, ball.py)
    "pcr_target_ball_moments": (C.c_int, [_vp, C.c_float, C.c_int, _i64p, _f64p, _f64p]),
    "pcr_target_estimate_normals_radius": (C.c_int, [_vp, C.c_float, C.c_int, _vp, _vp]),
    "pcr_scan_estimate_normals_radius": (C.c_int, [_vp, C.c_float, C.c_int, _vp, _vp]),
    "pcr_target_estimate_covariances_radius": (C.c_int, [_vp, C.c_float, C.c_int, C.c_int, C.c_double, _vp, _vp]),
    "pcr_scan_estimate_covariances_radius": (C.c_int, [_vp, C.c_float, C.c_int, C.c_int, C.c_double, _vp, _vp]),
    # pose hypotheses from correspondences and pose scoring (include/pcr.h, global_registration.py)
    "pcr_pose_score": (C.c_int, [_vp, _f32p, _f32p, C.c_int64, _f32p, C.c_int64, C.c_float, _i32p, _vp]),
    "pcr_ransac_poses": (C.c_int, [_vp, _f32p, _f32p, C.c_int64, C.c_int64, C.c_uint64, C.c_float, C.c_float, C.c_float,
                                   C.POINTER(C.c_int64), _f32p, C.POINTER(C.c_int32), C.POINTER(C.c_int64), _vp, _vp, _vp]),
    "pcr_pose_score_splits": (C.c_int, [C.c_int64, C.c_int64]),
    # fast global registration: the robust pass over a match list, its loop and the tuple test (include/pcr.h)
    "pcr_fgr_linearize": (C.c_int, [_vp, _f32p, _f32p, C.c_int64, _vp, _f64p, C.c_double, _f64p, _vp]),
    "pcr_fgr_pose": (C.c_int, [_vp, _f32p, _f32p, C.c_int64, _vp, _f64p, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int,
                               C.c_double, C.c_uint, _f64p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), _vp, _vp]),
    "pcr_fgr_tuples": (C.c_int, [_vp, _f32p, _f32p, C.c_int64, C.c_int64, C.c_uint64, C.c_float, C.c_float, _vp,
                                 C.POINTER(C.c_int64)]),
    "pcr_fgr_blocks": (C.c_int, [C.c_int64]),
    "pcr_fgr_solo_max": (C.c_int, [_vp, C.POINTER(C.c_int64)]),
    # the compatibility graph of a match list, its degrees and the consensus sets around its seeds (include/pcr.h)
    "pcr_compat_bits": (C.c_int, [_vp, _f32p, _f32p, C.c_int64, C.c_double, _vp]),
    "pcr_compat_degrees": (C.c_int, [_vp, _f32p, _f32p, C.c_int64, C.c_double, _vp, _vp]),
    "pcr_compat_consensus": (C.c_int, [_vp, _f32p, _f32p, C.c_int64, C.c_double, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp,
                                       C.POINTER(C.c_int)]),
    "pcr_profile_enable": (C.c_int, [_vp, C.c_int]),
    "pcr_profile_reset": (C.c_int, [_vp]),
    "pcr_profile_read": (C.c_int, [_vp, _i64p, _f64p]),
    "pcr_target_index_info": (C.c_int, [_vp, C.POINTER(C.c_double), _i64p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "pcr_target_index_halo": (C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "pcr_target_index_population": (C.c_int, [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "pcr_target_index_x_order": (C.c_int, [_vp, C.POINTER(C.c_double)]),
    "pcr_x_order_rule": (C.c_int, [C.c_int, C.c_int, C.c_int64, C.c_int]),
    "pcr_set_variant": (C.c_int, [_vp, C.c_int]),
    "pcr_get_variant": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "pcr_set_nn_mode": (C.c_int, [_vp, C.c_int]),
    "pcr_set_fuse_finalize": (C.c_int, [_vp, C.c_int]),
    "pcr_get_pipeline": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "pcr_nn_counters": (C.c_int, [_vp, _vp, _f64p, C.c_double, _f64p]),
    "pcr_nn_counters_x": (C.c_int, [_vp, _vp, _f64p, C.c_double, _f64p]),
    "pcr_nn_counters_edge": (C.c_int, [_vp, _vp, _f64p, C.c_double, _f64p]),
    "pcr_set_reuse": (C.c_int, [_vp, C.c_int, C.c_double, C.c_double]),
    "pcr_get_reuse": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pcr_scan_reuse_stats": (C.c_int, [_vp, _f64p]),
    "pcr_context_host_fold_passes": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "pcr_hash64": (C.c_int, [_vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "pcr_target_filter_band": (C.c_int, [_vp, C.POINTER(C.c_double)]),
    "pcr_target_index_halo2": (C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "pcr_target_index_list_set": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "pcr_usable_cpus": (C.c_int, []),
    "pcr_has_dev_kernels": (C.c_int, []),
    "pcr_abi_version": (C.c_int, []),
    "pcr_context_trim": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "pcr_profile_read_n": (C.c_int, [_vp, C.c_int, _i64p, _f64p, C.POINTER(C.c_int)]),
    "pcr_scan_read_matches": (C.c_int, [_vp, _vp]),
    "pcr_comm_p2p_finegrained": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "pcr_lzf_decompress": (C.c_int, [_vp, C.c_uint64, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "pcr_lzf_compress": (C.c_int, [_vp, C.c_uint64, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    # Gauss-Newton coresets (include/pcr.h, caratheodory.py)
    "pcr_gn_set": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, C.c_int64, C.c_int, _f64p]),
    "pcr_coreset": (C.c_int, [_vp, _f64p, C.c_int, C.c_int64, _f64p, C.c_int, C.c_int64, C.POINTER(C.c_int64), _f64p, _i64p,
                              _f64p]),
    # per-correspondence rows, weighted sums, scan coresets (include/pcr.h)
    "pcr_linearize_rows": (C.c_int, [_vp, _vp, C.c_int, _f64p, C.c_double, C.c_uint, _vp, _vp, _vp, _vp, _vp]),
    "pcr_linearize_weighted": (C.c_int, [_vp, _vp, C.c_int, _f64p, C.c_double, C.c_uint, _f64p, _f64p]),
    "pcr_scan_coreset": (C.c_int, [_vp, _vp, C.c_int, _f64p, C.c_double, C.c_uint, C.c_int, C.c_int64, _i64p, _f64p,
                                   C.POINTER(C.c_int64)]),
    # Generalized ICP: per-point covariances and the distribution-to-distribution pass (include/pcr.h)
    "pcr_target_estimate_covariances": (C.c_int, [_vp, C.c_int, C.c_int, C.c_double, _vp]),
    "pcr_target_set_covariances": (C.c_int, [_vp, _f32p]),
    "pcr_target_get_covariances": (C.c_int, [_vp, _f32p]),
    "pcr_scan_estimate_covariances": (C.c_int, [_vp, C.c_int, C.c_int, C.c_double, _vp]),
    "pcr_scan_set_covariances": (C.c_int, [_vp, _f32p]),
    "pcr_scan_get_covariances": (C.c_int, [_vp, _f32p]),
    "pcr_gicp_linearize": (C.c_int, [_vp, _vp, _f64p, C.c_double, C.c_uint, _f64p]),
    "pcr_gicp_align": (C.c_int, [_vp, _vp, _f64p, C.c_int, C.c_double, C.c_double, C.c_uint, _f64p, C.POINTER(C.c_int), _vp]),
    # Symmetric point-to-plane ICP: normals on a scan and the pass that uses both clouds' normals (include/pcr.h)
    "pcr_scan_estimate_normals": (C.c_int, [_vp, C.c_int, _vp]),
    "pcr_scan_set_normals": (C.c_int, [_vp, _f32p]),
    "pcr_scan_get_normals": (C.c_int, [_vp, _f32p]),
    "pcr_symm_linearize": (C.c_int, [_vp, _vp, _f64p, C.c_double, C.c_double, C.c_uint, _f64p]),
    "pcr_symm_align": (C.c_int, [_vp, _vp, _f64p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_uint, _f64p, C.POINTER(C.c_int), _vp]),
    # Colored ICP: intensities and tangent-plane gradients on a target, intensities on a scan, the two-row pass (include/pcr.h)
    "pcr_target_set_intensity": (C.c_int, [_vp, _f32p, _vp]),
    "pcr_target_estimate_color_gradients": (C.c_int, [_vp, C.c_int, _vp]),
    "pcr_target_get_color": (C.c_int, [_vp, _vp, _vp]),
    "pcr_scan_set_intensity": (C.c_int, [_vp, _f32p]),
    "pcr_scan_get_intensity": (C.c_int, [_vp, _f32p]),
    "pcr_color_linearize": (C.c_int, [_vp, _vp, _f64p, C.c_double, C.c_double, C.c_uint, _f64p]),
    "pcr_color_align": (C.c_int, [_vp, _vp, _f64p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_uint, _f64p, C.POINTER(C.c_int), _vp]),
    # Voxelized GICP: per-voxel covariances and the distribution-to-voxel pass (include/pcr.h)
    "pcr_target_voxels_set_covariances": (C.c_int, [_vp, C.c_int, C.c_double, _vp]),
    "pcr_target_voxels_get_covariances": (C.c_int, [_vp, _f64p]),
    "pcr_vgicp_linearize": (C.c_int, [_vp, _vp, _f64p, C.c_double, C.c_uint, _f64p]),
    "pcr_vgicp_align": (C.c_int, [_vp, _vp, _f64p, C.c_int, C.c_double, C.c_double, C.c_uint, _f64p, C.POINTER(C.c_int), _vp]),
    # robust kernels inside the pass of the four match-list aligners, and the squared residuals a scale is chosen from
    # (include/pcr.h); rb: a pcr_robust by pointer, or NULL
    "pcr_gicp_linearize_robust": (C.c_int, [_vp, _vp, _f64p, C.c_double, _vp, C.c_uint, _f64p]),
    "pcr_gicp_align_robust": (C.c_int, [_vp, _vp, _f64p, C.c_int, C.c_double, C.c_double, _vp, C.c_uint, _f64p, C.POINTER(C.c_int), _vp]),
    "pcr_gicp_residuals": (C.c_int, [_vp, _vp, _f64p, C.c_double, C.c_uint, _vp]),
    "pcr_vgicp_linearize_robust": (C.c_int, [_vp, _vp, _f64p, C.c_double, _vp, C.c_uint, _f64p]),
    "pcr_vgicp_align_robust": (C.c_int, [_vp, _vp, _f64p, C.c_int, C.c_double, C.c_double, _vp, C.c_uint, _f64p, C.POINTER(C.c_int), _vp]),
    "pcr_vgicp_residuals": (C.c_int, [_vp, _vp, _f64p, C.c_double, C.c_uint, _vp]),
    "pcr_symm_linearize_robust": (C.c_int, [_vp, _vp, _f64p, C.c_double, C.c_double, _vp, C.c_uint, _f64p]),
    "pcr_symm_align_robust": (C.c_int, [_vp, _vp, _f64p, C.c_int, C.c_double, C.c_double, C.c_double, _vp, C.c_uint, _f64p,
                                        C.POINTER(C.c_int), _vp]),
    "pcr_symm_residuals": (C.c_int, [_vp, _vp, _f64p, C.c_double, C.c_double, C.c_uint, _vp]),
    "pcr_color_linearize_robust": (C.c_int, [_vp, _vp, _f64p, C.c_double, C.c_double, _vp, C.c_uint, _f64p]),
    "pcr_color_align_robust": (C.c_int, [_vp, _vp, _f64p, C.c_int, C.c_double, C.c_double, C.c_double, _vp, C.c_uint, _f64p,
                                         C.POINTER(C.c_int), _vp]),
    "pcr_color_residuals": (C.c_int, [_vp, _vp, _f64p, C.c_double, C.c_double, C.c_uint, _vp]),
    # VGICP with direct voxel neighbourhoods: the containing-voxel lookup and the pass over 1, 7 or 27 voxels per point
    # (include/pcr.h); rb: a pcr_robust by pointer, or NULL
    "pcr_target_voxels_lookup": (C.c_int, [_vp, _vp, C.c_int64, C.c_int, _vp]),
    "pcr_target_voxels_set_keys": (C.c_int, [_vp, _vp]),
    "pcr_vgicp_direct_linearize": (C.c_int, [_vp, _vp, _f64p, C.c_double, C.c_int, _vp, C.c_uint, _f64p]),
    "pcr_vgicp_direct_align": (C.c_int, [_vp, _vp, _f64p, C.c_int, C.c_double, C.c_double, C.c_int, _vp, C.c_uint, _f64p,
                                         C.POINTER(C.c_int), _vp]),
    "pcr_vgicp_direct_residuals": (C.c_int, [_vp, _vp, _f64p, C.c_double, C.c_int, C.c_uint, _vp]),
    # the adaptive pass of the same four: a trim or a robust scale from each pass's own residuals, and the exact order statistic
    # behind it (include/pcr.h); ad: a pcr_adaptive by pointer; stats: 4 doubles (per iteration)
    "pcr_order_statistic": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64, _vp, _vp]),
    "pcr_gicp_linearize_adaptive": (C.c_int, [_vp, _vp, _f64p, C.c_double, _vp, C.c_uint, _f64p, _f64p]),
    "pcr_gicp_align_adaptive": (C.c_int, [_vp, _vp, _f64p, C.c_int, C.c_double, C.c_double, _vp, C.c_uint, _f64p, C.POINTER(C.c_int), _vp, _vp]),
    "pcr_vgicp_linearize_adaptive": (C.c_int, [_vp, _vp, _f64p, C.c_double, _vp, C.c_uint, _f64p, _f64p]),
    "pcr_vgicp_align_adaptive": (C.c_int, [_vp, _vp, _f64p, C.c_int, C.c_double, C.c_double, _vp, C.c_uint, _f64p, C.POINTER(C.c_int), _vp, _vp]),
    "pcr_symm_linearize_adaptive": (C.c_int, [_vp, _vp, _f64p, C.c_double, C.c_double, _vp, C.c_uint, _f64p, _f64p]),
    "pcr_symm_align_adaptive": (C.c_int, [_vp, _vp, _f64p, C.c_int, C.c_double, C.c_double, C.c_double, _vp, C.c_uint, _f64p,
                                          C.POINTER(C.c_int), _vp, _vp]),
    "pcr_color_linearize_adaptive": (C.c_int, [_vp, _vp, _f64p, C.c_double, C.c_double, _vp, C.c_uint, _f64p, _f64p]),
    "pcr_color_align_adaptive": (C.c_int, [_vp, _vp, _f64p, C.c_int, C.c_double, C.c_double, C.c_double, _vp, C.c_uint, _f64p,
                                           C.POINTER(C.c_int), _vp, _vp]),
    # batches: many scans / start poses against one target in one launch (include/pcr.h)
    "pcr_scan_batch_create": (C.c_int, [_vp, _vp, _i64p, C.c_int, C.c_uint, C.POINTER(_vp)]),
    "pcr_scan_batch_size": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
    "pcr_scan_batch_destroy": (C.c_int, [_vp]),
    "pcr_linearize_batch": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, _f64p, C.c_double, C.c_uint, _f64p]),
    "pcr_align_batch": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, _f64p, C.c_int, C.c_double, C.c_double, C.c_uint, _f64p,
                                  _vp, _vp, _vp]),
    # single-process multi-device groups (include/pcr.h)
    "pcr_group_create": (C.c_int, [C.POINTER(C.c_int), C.c_int, C.POINTER(_vp)]),
    "pcr_group_destroy": (C.c_int, [_vp]),
    "pcr_group_size": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "pcr_group_context": (C.c_int, [_vp, C.c_int, C.POINTER(_vp)]),
    "pcr_group_target_points_create": (C.c_int, [_vp, _vp, C.c_int64, _vp, C.c_float, C.POINTER(_vp)]),
    "pcr_group_target_voxels_create": (C.c_int, [_vp, _vp, C.c_int, C.c_int64, C.c_double, C.c_int, C.POINTER(_vp)]),
    "pcr_group_target_estimate_normals": (C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    "pcr_group_target_set_normals": (C.c_int, [_vp, _f32p]),
    "pcr_group_target_points_set_f64": (C.c_int, [_vp, _f64p]),
    "pcr_group_target_member": (C.c_int, [_vp, C.c_int, C.POINTER(_vp)]),
    "pcr_group_target_destroy": (C.c_int, [_vp]),
    "pcr_group_scan_create": (C.c_int, [_vp, _vp, C.c_int64, C.c_uint, C.POINTER(_vp)]),
    "pcr_group_scan_size": (C.c_int, [_vp, C.POINTER(C.c_int64)]),
    "pcr_group_scan_member": (C.c_int, [_vp, C.c_int, C.POINTER(_vp)]),
    "pcr_group_scan_destroy": (C.c_int, [_vp]),
    "pcr_group_linearize": (C.c_int, [_vp, _vp, C.c_int, _f64p, C.c_double, C.c_uint, _f64p]),
    "pcr_group_align": (C.c_int, [_vp, _vp, C.c_int, _f64p, C.c_int, C.c_double, C.c_double, C.c_uint, _f64p,
                                  C.POINTER(C.c_int), _vp]),
}
ABI_VERSION = 5                 # PCR_ABI_VERSION of the include/pcr.h this binding was written against


class PcrError(RuntimeError):
    """HIP / RCCL / argument failure reported by libpcr_hip.so."""


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  A PyTorch-ROCm wheel bundles its own libamdhip64.so and loads it
    by path; if libpcr_hip.so has already pulled in /opt/rocm's copy, a later ``import torch`` leaves
    TWO runtimes in the process (observed: "double free or corruption" at exit).  When torch is
    installed but not imported yet, load its runtime first so both sides resolve to the same one
    (same SONAME, libamdhip64.so.7).  PCR_KEEP_SYSTEM_HIP=1 skips this.

    Everything is loaded with RTLD_LOCAL: the loader reuses an already-loaded object by SONAME / inode
    whatever its scope, and putting RCCL's dependency librocm_smi64.so into the GLOBAL scope makes a
    later libamd_smi.so (loaded by ``import torch`` through the amdsmi module) bind its static
    ``amd::smi`` maps to librocm_smi64's copies -- constructed twice, destroyed twice, glibc aborts
    at exit (reproducible with six lines of ctypes, no libpcr involved)."""
    import importlib.util
    import sys
    if "torch" in sys.modules or os.environ.get("PCR_KEEP_SYSTEM_HIP"):
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.submodule_search_locations:
        return
    global _torch_lib_dir
    libdir = os.path.join(list(spec.submodule_search_locations)[0], "lib")
    path = os.path.join(libdir, "libamdhip64.so")
    if os.path.exists(path):
        try:
            C.CDLL(path, mode=C.RTLD_LOCAL)
            _torch_lib_dir = libdir
        except OSError:
            pass


def _share_rccl_with_torch():
    """Same idea for RCCL (bound lazily with dlopen("librccl.so.1") inside libpcr_hip.so): when the
    process runs on torch's HIP runtime, use the RCCL built against it."""
    if _torch_lib_dir is None:
        return
    path = os.path.join(_torch_lib_dir, "librccl.so")
    if os.path.exists(path):
        try:
            C.CDLL(path, mode=C.RTLD_LOCAL)
        except OSError:
            pass


def lib():
    """Load libpcr_hip.so (built in-tree by __graft_entry__.build() / csrc/Makefile)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PcrError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the registration hot path.")
    _share_hip_runtime_with_torch()
    L = C.CDLL(LIB_PATH, mode=C.RTLD_LOCAL)
    for name, (res, args) in PROTOTYPES.items():
        try:
            fn = getattr(L, name)      # AttributeError if the symbol is not exported
        except AttributeError:
            if not os.environ.get("PCR_LIB"):
                raise
            if name == "pcr_abi_version":
                raise PcrError(f"{LIB_PATH} predates pcr_abi_version (ABI < 4): too old for this binding, rebuild it")
            # an A/B library built from an older revision (tools/build_rev_lib.sh): instrumentation entry points it
            # does not have yet read as "nothing" (status 0, outputs untouched)
            setattr(L, name, lambda *a, **k: 0)
            continue
        fn.restype = res
        fn.argtypes = args
    if L.pcr_abi_version() != ABI_VERSION:
        raise PcrError(f"{LIB_PATH} has ABI version {L.pcr_abi_version()}, this binding expects {ABI_VERSION}: rebuild it")
    _lib = L
    return L


def check(status):
    if status == PCR_OK:
        return
    msg = lib().pcr_last_error().decode("utf-8", "replace")
    if status == PCR_ERR_SINGULAR:
        raise np.linalg.LinAlgError("Singular matrix")          # what numpy.linalg.solve raises (quirk Q7)
    if status == PCR_ERR_INVALID:
        raise ValueError(msg)
    if status == PCR_ERR_NO_TARGET:
        raise ValueError(msg)
    raise PcrError(f"libpcr_hip status {status}: {msg}")


def cloud_f32(a, name, finite=True):
    """``a`` as a C-contiguous float32 (N, 3) array, what every kernel reads, else ValueError (checked before the GPU is
    touched): the shape and, with ``finite``, every value finite -- as given and still as float32."""
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError(f"{name} must have shape (N, 3)")
    if finite and not np.all(np.isfinite(a)):
        raise ValueError(f"{name} must be finite")
    with np.errstate(over="ignore"):
        a = np.ascontiguousarray(a, dtype=np.float32)
    if finite and not np.all(np.isfinite(a)):
        raise ValueError(f"{name} must be finite as float32")
    return a


def check_radius(r):
    """A search radius as a float: finite and >= 0, else ValueError (checked before the GPU is touched)."""
    r = float(r)
    if not (np.isfinite(r) and r >= 0):
        raise ValueError(f"radius must be finite and >= 0, got {r}")
    return r


def check_ball(radius, max_nn):
    """A ball neighbourhood as (float radius, int max_nn): the radius finite and >= 0, ``max_nn`` None or 0 (the whole ball) or
    an integer in [1, 64] (its nearest ``max_nn``), the library's own rule (csrc/ball_moments.hip: ball_check), else ValueError
    before the GPU is touched.  ``max_nn`` without a radius is an error as well."""
    if radius is None:
        if max_nn is not None:
            raise ValueError("max_nn needs a radius")
        raise ValueError("radius must be finite and >= 0, got None")
    r = check_radius(radius)
    if max_nn is None:
        return r, 0
    if int(max_nn) != max_nn or not 0 <= int(max_nn) <= 64:
        raise ValueError("max_nn must be an integer in [0, 64] (0 or None: the whole ball)")
    return r, int(max_nn)


def check_iss(gamma_21, gamma_32, min_neighbors):
    """The ISS parameters as (float, float, int): gammas finite and > 0, min_neighbors an integer >= 1 (the library's own
    rule, csrc/keypoints.hip: iss_check), else ValueError before the GPU is touched."""
    g21, g32 = float(gamma_21), float(gamma_32)
    if not (np.isfinite(g21) and g21 > 0 and np.isfinite(g32) and g32 > 0):
        raise ValueError("gamma_21 and gamma_32 must be finite and > 0")
    if int(min_neighbors) != min_neighbors or not 1 <= int(min_neighbors) < 2 ** 31:
        raise ValueError("min_neighbors must be an integer >= 1")
    return g21, g32, int(min_neighbors)


def check_k(k):
    """1 <= k <= 64, the library's own bound and message (csrc/knn_normals.hip: check_k)."""
    if not 1 <= int(k) <= 64:
        raise ValueError("k must be in [1, 64]")
    return int(k)


def has_dev_kernels():
    """True when the loaded library is a developer build (unfused folds, wave-cooperative search, work counters)."""
    return bool(lib().pcr_has_dev_kernels())


def device_count():
    n = C.c_int(0)
    check(lib().pcr_device_count(C.byref(n)))
    return n.value


class Context:
    """One GPU + one HIP stream (pcr_context)."""

    def __init__(self, device=0):
        self.device = int(device)
        h = _vp()
        check(lib().pcr_context_create(self.device, C.byref(h)))
        self.handle = h
        self.nranks, self.rank = 1, 0

    def synchronize(self):
        check(lib().pcr_context_synchronize(self.handle))

    def stream(self):
        s = _vp()
        check(lib().pcr_context_stream(self.handle, C.byref(s)))
        return s.value

    def set_variant(self, v):
        check(lib().pcr_set_variant(self.handle, int(v)))

    def get_variant(self):
        v = C.c_int(0)
        check(lib().pcr_get_variant(self.handle, C.byref(v)))
        return v.value

    def set_nn_mode(self, m):
        check(lib().pcr_set_nn_mode(self.handle, int(m)))

    def set_fuse_finalize(self, on):
        check(lib().pcr_set_fuse_finalize(self.handle, int(bool(on))))

    def set_reuse(self, mode=None, tau=0.0, mu=0.0):
        """Certified reuse of the previous pass' matches: 0 off (default), 1 automatic, 2 always; ``tau`` / ``mu``
        in units of the target index' cell size (<= 0 keeps the current value)."""
        if mode is None:
            mode = self.get_reuse()["mode"]
        check(lib().pcr_set_reuse(self.handle, int(mode), float(tau), float(mu)))

    def get_reuse(self):
        m, t, u = C.c_int(0), C.c_double(0), C.c_double(0)
        check(lib().pcr_get_reuse(self.handle, C.byref(m), C.byref(t), C.byref(u)))
        return {"mode": m.value, "tau": t.value, "mu": u.value}

    def host_fold_passes(self):
        """Passes of this context whose last fold level the host took (0 with PCR_HOST_FOLD=0)."""
        n = C.c_uint64(0)
        check(lib().pcr_context_host_fold_passes(self.handle, C.byref(n)))
        return int(n.value)

    def get_pipeline(self):
        v, f, m = C.c_int(0), C.c_int(0), C.c_int(0)
        check(lib().pcr_get_pipeline(self.handle, C.byref(v), C.byref(f), C.byref(m)))
        return {"variant": v.value, "fuse_finalize": f.value, "nn_mode": m.value, "reuse": self.get_reuse()["mode"]}

    def pipeline(self, variant=None, fuse_finalize=None, nn_mode=None, reuse=None):
        """Context manager: select a kernel pipeline for the enclosed calls and RESTORE the previous
        selection afterwards (the context is process-wide)."""
        import contextlib

        @contextlib.contextmanager
        def _cm():
            prev = self.get_pipeline()
            try:
                if variant is not None:
                    self.set_variant(variant)
                if fuse_finalize is not None:
                    self.set_fuse_finalize(fuse_finalize)
                if nn_mode is not None:
                    self.set_nn_mode(nn_mode)
                if reuse is not None:
                    self.set_reuse(reuse)
                yield self
            finally:
                # restore everything that can be restored; a failing setter must not mask the body's own exception
                # or leave the rest of the selection behind
                errs = []
                for fn, val in ((self.set_variant, prev["variant"]), (self.set_fuse_finalize, prev["fuse_finalize"]),
                                (self.set_nn_mode, prev["nn_mode"]), (self.set_reuse, prev["reuse"])):
                    try:
                        fn(val)
                    except Exception as exc:          # noqa: BLE001
                        errs.append(exc)
                import sys as _sys
                if errs and _sys.exc_info()[0] is None:
                    raise errs[0]
        return _cm()

    # -- RCCL
    def comm_init(self, uid, nranks, rank):
        _share_rccl_with_torch()
        check(lib().pcr_comm_init(self.handle, uid, int(nranks), int(rank)))
        self.nranks, self.rank = int(nranks), int(rank)

    def comm_p2p_export(self):
        """Peer-to-peer transport (include/pcr.h): this rank's 64-byte IPC handle, to be all-gathered out of band."""
        buf = C.create_string_buffer(64)
        check(lib().pcr_comm_p2p_export(self.handle, buf))
        return buf.raw

    def comm_p2p_attach(self, handles, rank):
        blob = b"".join(handles)
        assert len(blob) == 64 * len(handles)
        check(lib().pcr_comm_p2p_attach(self.handle, blob, len(handles), int(rank)))
        self.nranks, self.rank = len(handles), int(rank)

    def comm_p2p_finegrained(self):
        """True: this rank's slots are fine-grained device memory (coherent across devices while a kernel runs)."""
        f = C.c_int(0)
        check(lib().pcr_comm_p2p_finegrained(self.handle, C.byref(f)))
        return bool(f.value)

    def comm_p2p_failed(self):
        f = C.c_int(0)
        check(lib().pcr_comm_p2p_failed(self.handle, C.byref(f)))
        return bool(f.value)

    def comm_destroy(self):
        check(lib().pcr_comm_destroy(self.handle))
        self.nranks, self.rank = 1, 0

    # -- profiling
    def profile_enable(self, on=True, period=1):
        """HIP events around the hot-path launches; ``period`` = n brackets every n-th pass only."""
        check(lib().pcr_profile_enable(self.handle, (max(int(period), 1) if on else 0)))

    def profile_reset(self):
        check(lib().pcr_profile_reset(self.handle))

    def profile_read(self):
        n = np.zeros(K_COUNT, np.int64)
        ms = np.zeros(K_COUNT, np.float64)
        cnt = C.c_int(0)
        check(lib().pcr_profile_read_n(self.handle, K_COUNT, n, ms, C.byref(cnt)))
        return {KERNEL_NAMES[i]: (int(n[i]), float(ms[i])) for i in range(min(K_COUNT, cnt.value))}

    def trim(self):
        """hipFree every idle block of the context's block cache (destroyed targets / scans leave up to 1 GiB there,
        invisible to torch's allocator); returns the bytes released."""
        b = C.c_uint64(0)
        check(lib().pcr_context_trim(self.handle, C.byref(b)))
        return int(b.value)

    def close(self):
        if getattr(self, "handle", None) and not _shutdown and not getattr(self, "_borrowed", False):
            lib().pcr_context_destroy(self.handle)
        self.handle = None


@atexit.register
def _release_all():
    """Free every device object and context while the HIP runtime is still alive.  Leaving this to
    ``__del__`` during interpreter teardown runs hipFree after the runtime's own static destructors
    (observed: "double free or corruption" at exit of a long pytest run)."""
    global _shutdown
    for obj in list(_live):
        try:
            obj.close()
        except Exception:
            pass
    for ctx in list(_contexts.values()):
        try:
            ctx.close()
        except Exception:
            pass
    _contexts.clear()
    for grp in list(_groups.values()) + list(_live_groups):
        try:
            grp.close()
        except Exception:
            pass
    _groups.clear()
    _shutdown = True


def comm_unique_id():
    buf = C.create_string_buffer(128)
    _share_rccl_with_torch()
    check(lib().pcr_comm_unique_id(buf))
    return buf.raw


_contexts = {}


def get_context(device=None):
    """Process-wide context per device; default device = LOCAL_RANK (one process per GPU)."""
    if device is None:
        device = int(os.environ.get("PCR_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        n = device_count()
        if n > 0:
            device %= n
    if device not in _contexts:
        _contexts[device] = Context(device)
    return _contexts[device]


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_vp)


class Target:
    """pcr_target handle (point target or voxel target)."""

    def __init__(self, ctx, handle, is_voxel):
        self.ctx, self.handle, self.is_voxel = ctx, handle, is_voxel
        _live.add(self)

    @classmethod
    def points(cls, ctx, xyz, normals=None, cell_hint=0.0):
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        if normals is not None:
            normals = np.ascontiguousarray(normals, dtype=np.float32)
            if normals.shape != xyz.shape:
                raise ValueError("normals must have the shape of the target")
        h = _vp()
        if isinstance(ctx, Group):
            check(lib().pcr_group_target_points_create(ctx.handle, _ptr(xyz), xyz.shape[0], _ptr(normals),
                                                       float(cell_hint), C.byref(h)))
            return GroupTarget(ctx, h, False)
        check(lib().pcr_target_points_create(ctx.handle, _ptr(xyz), xyz.shape[0], _ptr(normals),
                                             float(cell_hint), C.byref(h)))
        return cls(ctx, h, False)

    @classmethod
    def points_device(cls, ctx, d_xyz, n, d_normals=None, cell_hint=0.0):
        h = _vp()
        check(lib().pcr_target_points_create_device(ctx.handle, _vp(d_xyz), int(n),
                                                    _vp(d_normals) if d_normals else None,
                                                    float(cell_hint), C.byref(h)))
        return cls(ctx, h, False)

    @classmethod
    def voxels(cls, ctx, xyz, voxel_size, min_points=10):
        a = np.asarray(xyz)
        is64 = a.dtype == np.float64
        a = np.ascontiguousarray(a, dtype=np.float64 if is64 else np.float32)
        h = _vp()
        if isinstance(ctx, Group):
            check(lib().pcr_group_target_voxels_create(ctx.handle, _ptr(a), int(is64), a.shape[0], float(voxel_size),
                                                       int(min_points), C.byref(h)))
            return GroupTarget(ctx, h, True)
        check(lib().pcr_target_voxels_create(ctx.handle, _ptr(a), int(is64), a.shape[0], float(voxel_size),
                                             int(min_points), C.byref(h)))
        return cls(ctx, h, True)

    @classmethod
    def voxels_from_stats(cls, ctx, mean, norm, icov, voxel_size):
        mean = np.ascontiguousarray(mean, dtype=np.float64)
        norm = None if norm is None else np.ascontiguousarray(norm, dtype=np.float64)
        icov = None if icov is None else np.ascontiguousarray(icov, dtype=np.float64)
        h = _vp()
        check(lib().pcr_target_voxels_create_from_stats(ctx.handle, _ptr(mean), _ptr(norm), _ptr(icov),
                                                        mean.shape[0], float(voxel_size), C.byref(h)))
        return cls(ctx, h, True)

    def size(self):
        n = C.c_int64(0)
        check(lib().pcr_target_size(self.handle, C.byref(n)))
        return n.value

    def set_points_f64(self, xyz64):
        """Quirk Q6 (plane_icp.py:20-22, kdtree.py:18-21): the float64 coordinates of the points this target was created
        from -- PlaneICP passes and ``nn_query`` then search in float64, as the reference's tree over a float64 array does."""
        xyz64 = np.ascontiguousarray(xyz64, dtype=np.float64)
        if xyz64.shape != (self.size(), 3):
            raise ValueError("xyz64 must have the shape of the target")
        fn = lib().pcr_group_target_points_set_f64 if getattr(self, "ghandle", None) else lib().pcr_target_points_set_f64
        if not hasattr(fn, "argtypes"):          # (an older PCR_LIB without the entry point: its stub would "succeed")
            return False
        st = fn(getattr(self, "ghandle", None) or self.handle, xyz64)
        if st == PCR_ERR_UNSUPPORTED:
            # coordinates float32 cannot resolve (UTM-scale clouds): the float32 index stays, as before Q6 was reproduced
            import warnings
            warnings.warn("float64 target searched through its float32 copy: "
                          + lib().pcr_last_error().decode("utf-8", "replace"), RuntimeWarning, stacklevel=3)
            return False
        check(st)
        self.has_f64 = True
        return True

    def set_normals(self, normals):
        check(lib().pcr_target_set_normals(self.handle, np.ascontiguousarray(normals, dtype=np.float32)))

    def estimate_normals(self, k=15, compat=True, want=True):
        out = np.empty((self.size(), 3), np.float32) if want else None
        check(lib().pcr_target_estimate_normals(self.handle, int(k), int(bool(compat)), _ptr(out)))
        return out

    def get_normals(self):
        out = np.empty((self.size(), 3), np.float32)
        check(lib().pcr_target_get_normals(self.handle, out))
        return out

    # -- radius / hybrid neighbourhoods (include/pcr.h): ``max_nn`` None or 0 = the whole ball; everything in the caller's order
    def ball_moments(self, r, max_nn=None):
        """-> (count (N,) int64, mean (N, 3) float64, cov (N, 6) float64: the raw covariance xx xy xz yy yz zz)."""
        r, max_nn = check_ball(r, max_nn)
        n = self.size()
        count, mean, cov = np.zeros(n, np.int64), np.zeros((n, 3), np.float64), np.zeros((n, 6), np.float64)
        check(lib().pcr_target_ball_moments(self.handle, r, max_nn, count, mean, cov))
        return count, mean, cov

    def estimate_normals_radius(self, r, max_nn=None, want=True, want_counts=False):
        """Fills the target's normals from the ball; -> normals (N, 3) float32 (``want``), or (normals, counts (N,) int64)."""
        r, max_nn = check_ball(r, max_nn)
        out = np.empty((self.size(), 3), np.float32) if want else None
        cnt = np.zeros(self.size(), np.int64) if want_counts else None
        check(lib().pcr_target_estimate_normals_radius(self.handle, r, max_nn, _ptr(out), _ptr(cnt)))
        return (out, cnt) if want_counts else out

    def estimate_covariances_radius(self, r, max_nn=None, mode=COV_PLANE, eps=1e-3, want=True, want_counts=False):
        r, max_nn = check_ball(r, max_nn)
        out = np.empty((self.size(), 6), np.float32) if want else None
        cnt = np.zeros(self.size(), np.int64) if want_counts else None
        check(lib().pcr_target_estimate_covariances_radius(self.handle, r, max_nn, int(mode), float(eps), _ptr(out), _ptr(cnt)))
        return (out, cnt) if want_counts else out

    # -- ColoredICP: float32 intensities (N,) and tangent-plane gradients (N, 3), in the caller's order (include/pcr.h)
    def set_intensity(self, intensity, gradient=None):
        intensity = np.ascontiguousarray(intensity, dtype=np.float32)
        if intensity.shape != (self.size(),):
            raise ValueError("intensity must have shape (N,)")
        if gradient is not None:
            gradient = np.ascontiguousarray(gradient, dtype=np.float32)
            if gradient.shape != (self.size(), 3):
                raise ValueError("gradient must have shape (N, 3)")
        check(lib().pcr_target_set_intensity(self.handle, intensity, _ptr(gradient)))

    def estimate_color_gradients(self, k=10, want=True):
        out = np.empty((self.size(), 3), np.float32) if want else None
        check(lib().pcr_target_estimate_color_gradients(self.handle, int(k), _ptr(out)))
        return out

    def get_color(self):
        """-> (intensity (N,), gradient (N, 3))"""
        inten, grad = np.empty(self.size(), np.float32), np.empty((self.size(), 3), np.float32)
        check(lib().pcr_target_get_color(self.handle, _ptr(inten), _ptr(grad)))
        return inten, grad

    # -- GICP covariances: float32 (N, 6) = xx xy xz yy yz zz, in the caller's order (include/pcr.h)
    def estimate_covariances(self, k=10, mode=COV_PLANE, eps=1e-3, want=True):
        out = np.empty((self.size(), 6), np.float32) if want else None
        check(lib().pcr_target_estimate_covariances(self.handle, int(k), int(mode), float(eps), _ptr(out)))
        return out

    def set_covariances(self, cov):
        cov = cov6(cov)
        if cov.shape != (self.size(), 6):
            raise ValueError("covariances must have shape (N, 6) or (N, 3, 3)")
        check(lib().pcr_target_set_covariances(self.handle, cov))

    def get_covariances(self):
        out = np.empty((self.size(), 6), np.float32)
        check(lib().pcr_target_get_covariances(self.handle, out))
        return out

    # -- VGICP covariances of a voxel target: float64 (Nv, 6) = xx xy xz yy yz zz, in the order of voxel_stats (ascending key)
    def set_voxel_covariances(self, mode=COV_PLANE, eps=1e-3, cov=None):
        """``cov`` (Nv, 6) or (Nv, 3, 3) float64 overrides ``mode`` (COV_PLANE: from the voxel normals, COV_RAW: the voxels' own)."""
        if cov is not None:
            cov = cov6_f64(cov)
            if cov.shape != (self.size(), 6):
                raise ValueError("voxel covariances must have shape (Nv, 6) or (Nv, 3, 3)")
        check(lib().pcr_target_voxels_set_covariances(self.handle, int(mode), float(eps), _ptr(cov)))

    def get_voxel_covariances(self):
        out = np.empty((self.size(), 6), np.float64)
        check(lib().pcr_target_voxels_get_covariances(self.handle, out))
        return out

    # -- direct voxel lookup (include/pcr.h): the kept voxel that contains a point, and its neighbours
    def lookup(self, q, neighbors=1):
        """-> (M, neighbors) int64 rows of voxel_stats for the float32 points ``q``, -1 where there is no kept voxel."""
        q = np.ascontiguousarray(q, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != 3:
            raise ValueError("points must have shape (M, 3)")
        idx = np.empty((q.shape[0], max(int(neighbors), 0)), np.int64)
        check(lib().pcr_target_voxels_lookup(self.handle, _ptr(q), q.shape[0], int(neighbors), _ptr(idx)))
        return idx

    def set_voxel_keys(self, keys):
        """The hash keys of a target made by ``voxels_from_stats``, in the order of its means."""
        keys = np.ascontiguousarray(keys, dtype=np.int64)
        if keys.shape != (self.size(),):
            raise ValueError("keys must have shape (Nv,)")
        check(lib().pcr_target_voxels_set_keys(self.handle, _ptr(keys)))

    def voxel_stats(self, names=("mean", "cov", "norm", "icov", "counts", "keys")):
        n = self.size()
        bufs = {"mean": np.empty((n, 3)), "cov": np.empty((n, 3, 3)), "norm": np.empty((n, 3)),
                "icov": np.empty((n, 3, 3)), "counts": np.empty(n, np.int64), "keys": np.empty(n, np.int64)}
        nv = C.c_int64(0)
        args = [_ptr(bufs[k]) if k in names else None for k in ("mean", "cov", "norm", "icov", "counts", "keys")]
        check(lib().pcr_target_voxels_get(self.handle, C.byref(nv), *args))
        return {k: bufs[k] for k in names}

    def index_info(self):
        cell, occ, n = C.c_double(0), C.c_int64(0), C.c_int64(0)
        dims = np.zeros(3, np.int64)
        check(lib().pcr_target_index_info(self.handle, C.byref(cell), dims, C.byref(occ), C.byref(n)))
        halo, nh = C.c_double(0), C.c_int64(0)
        check(lib().pcr_target_index_halo(self.handle, C.byref(halo), C.byref(nh)))
        band = C.c_double(0)
        check(lib().pcr_target_filter_band(self.handle, C.byref(band)))
        halo2, nh2 = C.c_double(0), C.c_int64(0)
        check(lib().pcr_target_index_halo2(self.handle, C.byref(halo2), C.byref(nh2)))
        sets = []                       # near, mid, far: (margin in metres, records); zeros while a set does not exist
        for k in range(3):
            hk, nk = C.c_double(0), C.c_int64(0)
            check(lib().pcr_target_index_list_set(self.handle, k, C.byref(hk), C.byref(nk)))
            sets.append((hk.value, nk.value))
        pmax, p99, heavy = C.c_int64(0), C.c_int64(0), C.c_int(0)
        check(lib().pcr_target_index_population(self.handle, C.byref(pmax), C.byref(p99), C.byref(heavy)))
        xq = C.c_double(0)
        check(lib().pcr_target_index_x_order(self.handle, C.byref(xq)))
        return {"cell": cell.value, "dims": tuple(int(d) for d in dims), "occupied": occ.value, "n": n.value,
                "halo": halo.value, "halo_records": nh.value, "filter_band": band.value,
                "halo2": halo2.value, "halo2_records": nh2.value, "list_sets": sets,
                "pop_max": pmax.value, "pop_p99": p99.value, "heavy": bool(heavy.value),
                "x_ordered": xq.value > 0.0, "xq": xq.value}

    def searches_f64(self):
        """True when the target answers in float64: a voxel target, or a point target that holds the float64 coordinates
        of its points (``set_points_f64`` succeeded)."""
        return bool(self.is_voxel or getattr(self, "has_f64", False))

    def nn_query(self, q, r_max=np.inf):
        """Nearest neighbour of every query.  A float64 array on a target that answers in float64 is searched as it is
        (pcr_nn_query_dd); every other array as float32, by the calls it has always taken."""
        q = np.asarray(q)
        if q.dtype == np.float64 and self.searches_f64():
            q = np.ascontiguousarray(q)
            m = q.shape[0]
            dist, idx = np.empty(m, np.float64), np.empty(m, np.int64)
            check(lib().pcr_nn_query_dd(self.handle, q, m, float(r_max), dist, idx))
            return dist, idx
        q = np.ascontiguousarray(q, dtype=np.float32)
        m = q.shape[0]
        idx = np.empty(m, np.int64)
        if self.searches_f64():
            dist = np.empty(m, np.float64)
            check(lib().pcr_nn_query_f64(self.handle, q, m, float(r_max), dist, idx))
        else:
            dist = np.empty(m, np.float32)
            check(lib().pcr_nn_query(self.handle, q, m, float(r_max), dist, idx))
        return dist, idx

    def knn_query(self, q, k):
        """k nearest neighbours, rows nearest first.  On a target that answers in float64 every query array is taken to
        float64 (exact for float32) and the float64 coordinates are searched (pcr_knn_query_f64): float64 distances."""
        if self.searches_f64():
            q = np.ascontiguousarray(q, dtype=np.float64)
            m = q.shape[0]
            dist, idx = np.empty((m, k), np.float64), np.empty((m, k), np.int64)
            check(lib().pcr_knn_query_f64(self.handle, q, m, int(k), dist, idx))
            return dist, idx
        q = np.ascontiguousarray(q, dtype=np.float32)
        m = q.shape[0]
        dist = np.empty((m, k), np.float32)
        idx = np.empty((m, k), np.int64)
        check(lib().pcr_knn_query(self.handle, q, m, int(k), dist, idx))
        return dist, idx

    # -- fixed-radius search (include/pcr.h): CSR results, float64 on a point target that holds float64 coordinates
    def _radius_args(self, q, r):
        r = check_radius(r)
        f64 = self.searches_f64()
        q = np.ascontiguousarray(q, dtype=np.float64 if f64 else np.float32)
        if q.ndim != 2 or q.shape[1] != 3:
            raise ValueError("points must have shape (M, 3)")
        return q, r, f64

    def radius_count(self, q, r):
        """Neighbours within ``r`` of every query: (M,) int64.  A target that answers in float64 takes every query array to
        float64 (exact for float32) and searches the float64 coordinates; any other rounds the queries to float32."""
        q, r, f64 = self._radius_args(q, r)
        count = np.empty(q.shape[0], np.int64)
        check((lib().pcr_radius_count_dd if f64 else lib().pcr_radius_count)(self.handle, q, q.shape[0], r, count))
        return count

    def radius_query(self, q, r, offsets=None, out=None):
        """-> (dist, idx, offsets): the neighbours of query i at [offsets[i], offsets[i + 1]), ordered by (squared distance,
        index).  ``offsets`` (M + 1 int64, the running sums of ``radius_count``) is computed when not given; ``out`` =
        (dist, idx) arrays to fill.  Offsets that do not match what the search finds raise ValueError and leave ``out`` as
        it was."""
        q, r, f64 = self._radius_args(q, r)
        if offsets is None:
            offsets = np.zeros(q.shape[0] + 1, np.int64)
            np.cumsum(self.radius_count(q, r), out=offsets[1:])
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if offsets.shape != (q.shape[0] + 1,):
            raise ValueError("offsets must have M + 1 entries")
        total = max(int(offsets[-1]), 0)
        dist, idx = out if out is not None else (np.empty(total, np.float64 if f64 else np.float32), np.empty(total, np.int64))
        if dist.dtype != (np.float64 if f64 else np.float32) or idx.dtype != np.int64 or len(dist) < total or len(idx) < total:
            raise ValueError("out arrays do not fit the offsets")
        check((lib().pcr_radius_query_dd if f64 else lib().pcr_radius_query)(self.handle, q, q.shape[0], r, offsets, dist, idx))
        return dist, idx, offsets

    def knn_mean_distance(self, k):
        """Mean distance of every point to its k nearest neighbours within the target (itself included): (N,) float64 in
        the caller's order, over the float32 copy of the points."""
        out = np.empty(self.size(), np.float64)
        check(lib().pcr_knn_mean_distance(self.handle, int(k), out))
        return out

    # -- FPFH descriptors (include/pcr.h): a point target that has normals
    def spfh(self, r):
        """-> (counts (N, 33) uint32, k (N,) int64): the simplified point feature histograms as integer counts and the
        number of neighbours, in the caller's order."""
        r = check_radius(r)
        n = self.size()
        counts, k = np.zeros((n, 33), np.uint32), np.zeros(n, np.int64)
        check(lib().pcr_target_spfh(self.handle, r, counts, k))
        return counts, k

    def fpfh(self, r, want_k=False, rows=None):
        """-> (N, 33) float32 FPFH descriptors in the caller's order (and k (N,) int64 with ``want_k``).  ``rows``: strictly
        ascending int64 indices -> the (len(rows), 33) descriptors of those points only, equal to ``fpfh(r)[rows]``."""
        r = check_radius(r)
        if rows is not None:
            rows = np.ascontiguousarray(rows, dtype=np.int64)
            if rows.ndim != 1:
                raise ValueError("rows must be a vector")
            out = np.zeros((len(rows), 33), np.float32)
            k = np.zeros(len(rows), np.int64) if want_k else None
            check(lib().pcr_target_fpfh_rows(self.handle, r, rows, len(rows), out, _ptr(k)))
            return (out, k) if want_k else out
        n = self.size()
        out = np.zeros((n, 33), np.float32)
        k = np.zeros(n, np.int64) if want_k else None
        check(lib().pcr_target_fpfh(self.handle, r, out, _ptr(k)))
        return (out, k) if want_k else out

    # -- ISS keypoints (include/pcr.h): a point target, no normals needed
    def iss_saliency(self, r, gamma_21=0.975, gamma_32=0.975, min_neighbors=5):
        """-> (eig (N, 3) float64, l1 >= l2 >= l3; saliency (N,) float64; k (N,) int64) at the salient radius ``r``, in the
        caller's order."""
        r = check_radius(r)
        g21, g32, mn = check_iss(gamma_21, gamma_32, min_neighbors)
        n = self.size()
        eig, sal, k = np.zeros((n, 3), np.float64), np.zeros(n, np.float64), np.zeros(n, np.int64)
        check(lib().pcr_target_iss_saliency(self.handle, r, g21, g32, mn, eig, sal, k))
        return eig, sal, k

    def iss_keypoints(self, r_salient, r_nonmax, gamma_21=0.975, gamma_32=0.975, min_neighbors=5, want_saliency=False):
        """-> (N,) bool keypoint mask in the caller's order (and the saliency (N,) float64 with ``want_saliency``)."""
        r_salient, r_nonmax = check_radius(r_salient), check_radius(r_nonmax)
        g21, g32, mn = check_iss(gamma_21, gamma_32, min_neighbors)
        n = self.size()
        mask = np.zeros(n, np.uint8)
        sal = np.zeros(n, np.float64) if want_saliency else None
        check(lib().pcr_target_iss_keypoints(self.handle, r_salient, r_nonmax, g21, g32, mn, mask, _ptr(sal)))
        mask = mask.astype(bool)
        return (mask, sal) if want_saliency else mask

    def close(self):
        if getattr(self, "handle", None) and not _shutdown and not getattr(self, "_borrowed", False):
            lib().pcr_target_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Scan:
    """pcr_scan handle: the float32 scan, uploaded and Morton-sorted once per align()."""

    def __init__(self, ctx, xyz=None, flags=0, device_ptr=None, n=None):
        self.ctx = ctx
        self.ghandle = None
        self.flags = int(flags)
        h = _vp()
        if isinstance(ctx, Group):
            # a group scan: cut into one contiguous shard per member inside pcr_group_scan_create
            xyz = np.ascontiguousarray(xyz, dtype=np.float32)
            if xyz.ndim != 2 or xyz.shape[1] != 3:
                raise ValueError("scan must have shape (N, 3)")
            check(lib().pcr_group_scan_create(ctx.handle, _ptr(xyz), xyz.shape[0], int(flags), C.byref(h)))
            self.n = xyz.shape[0]
            self.ghandle, self.handle = h, None
            _live.add(self)
            return
        if device_ptr is not None:
            check(lib().pcr_scan_create_device(ctx.handle, _vp(device_ptr), int(n), int(flags), C.byref(h)))
            self.n = int(n)
        else:
            xyz = np.ascontiguousarray(xyz, dtype=np.float32)
            if xyz.ndim != 2 or xyz.shape[1] != 3:
                raise ValueError("scan must have shape (N, 3)")
            check(lib().pcr_scan_create(ctx.handle, _ptr(xyz), xyz.shape[0], int(flags), C.byref(h)))
            self.n = xyz.shape[0]
        self.handle = h
        _live.add(self)

    def reuse_stats(self):
        """Certified reuse on this scan: passes by search mode, points the list passes searched, last pass."""
        o = np.zeros(8)
        check(lib().pcr_scan_reuse_stats(self.handle, o))
        return {"passes_full": int(o[0]), "passes_track": int(o[1]), "passes_list": int(o[2]),
                "list_searched": int(o[3]), "list_points": int(o[4]),
                "last_mode": int(o[5]), "last_searched": int(o[6]), "last_motion": float(o[7])}

    def matches(self):
        """The correspondences of the last search + reduce pass over this scan (test / diagnostic seam): per scan
        point in the scan's DEVICE order, the cell-sorted index of the matched target record, -1 = none."""
        out = np.empty(self.n, np.uint32)
        check(lib().pcr_scan_read_matches(self.handle, _ptr(out)))
        m = out.astype(np.int64)
        m[out == 0xFFFFFFFF] = -1
        return m

    # -- GICP covariances: float32 (N, 6) = xx xy xz yy yz zz, in the caller's order (include/pcr.h)
    def estimate_covariances(self, k=10, mode=COV_PLANE, eps=1e-3, want=True):
        out = np.empty((self.n, 6), np.float32) if want else None
        check(lib().pcr_scan_estimate_covariances(self.handle, int(k), int(mode), float(eps), _ptr(out)))
        return out

    def set_covariances(self, cov):
        cov = cov6(cov)
        if cov.shape != (self.n, 6):
            raise ValueError("covariances must have shape (N, 6) or (N, 3, 3)")
        check(lib().pcr_scan_set_covariances(self.handle, cov))

    def get_covariances(self):
        out = np.empty((self.n, 6), np.float32)
        check(lib().pcr_scan_get_covariances(self.handle, out))
        return out

    # -- SymmetricICP normals: float32 (N, 3), in the caller's order (include/pcr.h)
    def estimate_normals(self, k=10, want=True):
        out = np.empty((self.n, 3), np.float32) if want else None
        check(lib().pcr_scan_estimate_normals(self.handle, int(k), _ptr(out)))
        return out

    # -- the same from a ball (include/pcr.h: radius and hybrid neighbourhoods), as the methods of ``Target``
    def estimate_normals_radius(self, r, max_nn=None, want=True, want_counts=False):
        r, max_nn = check_ball(r, max_nn)
        out = np.empty((self.n, 3), np.float32) if want else None
        cnt = np.zeros(self.n, np.int64) if want_counts else None
        check(lib().pcr_scan_estimate_normals_radius(self.handle, r, max_nn, _ptr(out), _ptr(cnt)))
        return (out, cnt) if want_counts else out

    def estimate_covariances_radius(self, r, max_nn=None, mode=COV_PLANE, eps=1e-3, want=True, want_counts=False):
        r, max_nn = check_ball(r, max_nn)
        out = np.empty((self.n, 6), np.float32) if want else None
        cnt = np.zeros(self.n, np.int64) if want_counts else None
        check(lib().pcr_scan_estimate_covariances_radius(self.handle, r, max_nn, int(mode), float(eps), _ptr(out), _ptr(cnt)))
        return (out, cnt) if want_counts else out

    def set_normals(self, normals):
        normals = np.ascontiguousarray(normals, dtype=np.float32)
        if normals.shape != (self.n, 3):
            raise ValueError("normals must have shape (N, 3)")
        check(lib().pcr_scan_set_normals(self.handle, normals))

    def get_normals(self):
        out = np.empty((self.n, 3), np.float32)
        check(lib().pcr_scan_get_normals(self.handle, out))
        return out

    # -- ColoredICP intensities: float32 (N,), in the caller's order (include/pcr.h)
    def set_intensity(self, intensity):
        intensity = np.ascontiguousarray(intensity, dtype=np.float32)
        if intensity.shape != (self.n,):
            raise ValueError("intensity must have shape (N,)")
        check(lib().pcr_scan_set_intensity(self.handle, intensity))

    def get_intensity(self):
        out = np.empty(self.n, np.float32)
        check(lib().pcr_scan_get_intensity(self.handle, out))
        return out

    def member(self, i):
        """Member i's shard of a group scan (borrowed: destroyed with the group scan; ``ctx`` is the member's context).  A plain
        ``linearize`` over it needs FLAG_LOCAL_ONLY: the member's context takes part in the group's exchange."""
        if self.ghandle is None:
            raise ValueError("member() of a scan that is not a group scan")
        h, n = _vp(), C.c_int64(0)
        check(lib().pcr_group_scan_member(self.ghandle, int(i), C.byref(h)))
        check(lib().pcr_scan_size(h, C.byref(n)))
        s = Scan.__new__(Scan)
        s.ctx, s.ghandle, s.handle, s.n, s._borrowed, s._owner = self.ctx.member(i), None, h, n.value, True, self
        return s

    def close(self):
        if getattr(self, "ghandle", None) and not _shutdown:
            lib().pcr_group_scan_destroy(self.ghandle)
        elif getattr(self, "handle", None) and not _shutdown and not getattr(self, "_borrowed", False):
            lib().pcr_scan_destroy(self.handle)
        self.handle = None
        self.ghandle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Group:
    """pcr_group: single-process multi-device (include/pcr.h).  One context + host thread per entry of ``devices`` (an id
    may repeat: ``[0, 0]`` = two contexts on one GPU).  Pass it wherever a Context is expected by ``Target.points`` /
    ``Target.voxels`` / ``Scan``: targets are then built on every member, scans sharded contiguously, and ``linearize`` /
    ``align`` return the sums / the pose over the WHOLE scan."""

    def __init__(self, devices):
        self.devices = tuple(int(d) for d in devices)
        if not 1 <= len(self.devices) <= 8:
            raise ValueError("a group has 1 to 8 member devices")
        ids = (C.c_int * len(self.devices))(*self.devices)
        h = _vp()
        check(lib().pcr_group_create(ids, len(self.devices), C.byref(h)))
        self.handle = h
        self.nranks, self.rank = len(self.devices), 0
        _live_groups.add(self)

    def member(self, i):
        """Member i's context (borrowed, not owned): profiling, pipeline switches, synchronize."""
        h = _vp()
        check(lib().pcr_group_context(self.handle, int(i), C.byref(h)))
        c = Context.__new__(Context)
        c.device, c.handle, c.nranks, c.rank, c._borrowed = self.devices[i], h, len(self.devices), int(i), True
        return c

    def synchronize(self):
        for i in range(len(self.devices)):
            self.member(i).synchronize()

    def close(self):
        if getattr(self, "handle", None) and not _shutdown:
            lib().pcr_group_destroy(self.handle)
        self.handle = None


def get_group(devices):
    """Process-wide group per device tuple (like get_context per device)."""
    key = tuple(int(d) for d in devices)
    if key not in _groups:
        _groups[key] = Group(key)
    return _groups[key]


class GroupTarget(Target):
    """pcr_group_target: the same target on every member.  ``handle`` is member 0's pcr_target (borrowed), so every
    read-only method of Target (statistics, queries, index_info) answers from member 0; what changes the target runs on all."""

    def __init__(self, group, ghandle, is_voxel):
        self.ghandle = ghandle
        h = _vp()
        check(lib().pcr_group_target_member(ghandle, 0, C.byref(h)))
        super().__init__(group, h, is_voxel)

    def member(self, i):
        """Member i's target (borrowed: destroyed with the group target; ``ctx`` is the member's context): index_info,
        queries and read-backs of that member."""
        h = _vp()
        check(lib().pcr_group_target_member(self.ghandle, int(i), C.byref(h)))
        t = Target.__new__(Target)
        t.ctx, t.handle, t.is_voxel, t._borrowed, t._owner = self.ctx.member(i), h, self.is_voxel, True, self
        return t

    def set_normals(self, normals):
        check(lib().pcr_group_target_set_normals(self.ghandle, np.ascontiguousarray(normals, dtype=np.float32)))

    def estimate_normals(self, k=15, compat=True, want=True):
        out = np.empty((self.size(), 3), np.float32) if want else None
        check(lib().pcr_group_target_estimate_normals(self.ghandle, int(k), int(bool(compat)), _ptr(out)))
        return out

    def close(self):
        if getattr(self, "ghandle", None) and not _shutdown:
            lib().pcr_group_target_destroy(self.ghandle)
        self.ghandle = None
        self.handle = None


def lzf_decompress(data, out_len):
    """LZF stream -> bytes of length out_len (pcr_lzf_decompress: host C, no GPU needed)."""
    src = np.frombuffer(data, dtype=np.uint8)
    out = np.empty(int(out_len), np.uint8)
    w = C.c_uint64(0)
    st = lib().pcr_lzf_decompress(src.ctypes.data_as(_vp), src.size, out.ctypes.data_as(_vp), out.size, C.byref(w))
    if st != PCR_OK or w.value != out_len:
        raise ValueError("corrupt LZF stream in PCD file")
    return out.tobytes()


def lzf_compress(data):
    src = np.frombuffer(data, dtype=np.uint8)
    out = np.empty(src.size + src.size // 32 + 16, np.uint8)
    w = C.c_uint64(0)
    check(lib().pcr_lzf_compress(src.ctypes.data_as(_vp), src.size, out.ctypes.data_as(_vp), out.size, C.byref(w)))
    return out[:w.value].tobytes()


def feature_match(ctx, A, B):
    """pcr_feature_match: A (na, D), B (nb, D) float32 -> (idx (na,) int64, d2_first (na,) float32, d2_second (na,) float32)."""
    A, B = np.ascontiguousarray(A, dtype=np.float32), np.ascontiguousarray(B, dtype=np.float32)
    if A.ndim != 2 or B.ndim != 2 or A.shape[1] != B.shape[1]:
        raise ValueError("features must have shapes (NA, D) and (NB, D)")
    if not 1 <= A.shape[1] <= 64:
        raise ValueError("features must have 1 to 64 columns")
    na = A.shape[0]
    idx, d1, d2 = np.empty(na, np.int64), np.empty(na, np.float32), np.empty(na, np.float32)
    check(lib().pcr_feature_match(ctx.handle, A, na, B, B.shape[0], A.shape[1], idx, d1, d2))
    return idx, d1, d2


RANSAC_TILE = 256               # PCR_RANSAC_TILE of include/pcr.h: rows per tile of k_pose_score
RANSAC_M_MAX = 1 << 24
RANSAC_H_MAX = 1 << 26


def check_pairs(src, dst):
    """Paired correspondences as C-contiguous float32 (M, 3) arrays: finite, M <= 2^24, else ValueError (checked before the
    GPU is touched)."""
    src, dst = np.asarray(src), np.asarray(dst)
    if src.ndim != 2 or src.shape[1] != 3 or src.shape != dst.shape:
        raise ValueError("src and dst must have one shape (M, 3)")
    if len(src) > RANSAC_M_MAX:
        raise ValueError("more than 2^24 correspondences")
    return cloud_f32(src, "src and dst"), cloud_f32(dst, "src and dst")


def check_distance(d, name):
    """A float32 distance: finite and >= 0, else ValueError."""
    with np.errstate(over="ignore"):
        d = float(np.float32(d))
    if not (np.isfinite(d) and d >= 0):
        raise ValueError(f"{name} must be finite and >= 0")
    return d


def pose_score(ctx, src, dst, poses, max_dist, want_mask=False):
    """pcr_pose_score: src, dst (M, 3), poses (B, 12) float32 -> counts (B,) int32 (and masks (B, M) bool with ``want_mask``).
    ``ctx`` may be a callable that returns the context: it is called after the arguments have passed."""
    src, dst = check_pairs(src, dst)
    poses = np.asarray(poses)
    if poses.ndim != 2 or poses.shape[1] != 12:
        raise ValueError("poses must have shape (B, 12)")
    if len(poses) > RANSAC_H_MAX:
        raise ValueError("more than 2^26 poses")
    poses = np.ascontiguousarray(poses, dtype=np.float32)
    max_dist = check_distance(max_dist, "max_dist")
    b, m = len(poses), len(src)
    count = np.zeros(b, np.int32)
    mask = np.zeros((b, m), np.uint8) if want_mask else None
    if b and m:
        if callable(ctx):
            ctx = ctx()
        check(lib().pcr_pose_score(ctx.handle, src, dst, m, poses, b, max_dist, count, _ptr(mask)))
    return (count, mask.view(np.bool_)) if want_mask else count


def ransac_poses(ctx, src, dst, n_hyp, seed, max_dist, edge_similarity, min_edge, want_all=False):
    """pcr_ransac_poses -> dict(best, pose (12,) float32, count, n_valid) and, with ``want_all``, samples (H, 3) int32, poses
    (H, 12) float32 and counts (H,) int32 of every hypothesis.  ``ctx`` may be a callable, as for ``pose_score``."""
    src, dst = check_pairs(src, dst)
    n_hyp, seed = int(n_hyp), int(seed)
    if not 0 <= n_hyp <= RANSAC_H_MAX:
        raise ValueError("n_hypotheses must be in [0, 2^26]")
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed must be in [0, 2^64)")
    max_dist, min_edge = check_distance(max_dist, "max_dist"), check_distance(min_edge, "min_edge")
    edge_similarity = float(np.float32(edge_similarity))
    if not 0 <= edge_similarity <= 1:
        raise ValueError("edge_similarity must be in [0, 1]")
    m = len(src)
    pose = np.zeros(12, np.float32)
    pose[[0, 4, 8]] = 1
    out = {"best": -1, "pose": pose, "count": 0, "n_valid": 0}
    if want_all:
        out["samples"] = np.full((n_hyp, 3), -1, np.int32)
        out["poses"] = np.full((n_hyp, 12), np.nan, np.float32)
        out["counts"] = np.full(n_hyp, -1, np.int32)
    if n_hyp == 0 or m < 3:
        return out
    if callable(ctx):
        ctx = ctx()
    best, count, n_valid = C.c_int64(-1), C.c_int32(0), C.c_int64(0)
    check(lib().pcr_ransac_poses(ctx.handle, src, dst, m, n_hyp, seed, max_dist, edge_similarity, min_edge, C.byref(best), pose,
                                 C.byref(count), C.byref(n_valid), _ptr(out.get("samples")), _ptr(out.get("poses")),
                                 _ptr(out.get("counts"))))
    out.update(best=best.value, count=count.value, n_valid=n_valid.value)
    return out


def pose_score_splits(m, b):
    """pcr_pose_score_splits: how many row splits a pcr_pose_score call of b poses over m rows uses (a host-side rule)."""
    return int(lib().pcr_pose_score_splits(int(m), int(b)))


FGR_TILE, FGR_WIDTH, FGR_TRACE = 256, 4, 46     # PCR_FGR_TILE, PCR_FGR_WIDTH, PCR_FGR_TRACE of include/pcr.h


def check_mult(mult, m):
    """Multiplicities as C-contiguous int32 (M,), every one >= 0, or None; else ValueError."""
    if mult is None:
        return None
    mult = np.asarray(mult)
    if mult.shape != (m,) or not np.issubdtype(mult.dtype, np.integer):
        raise ValueError("mult must be M integers")
    if m and (mult.min() < 0 or mult.max() >= 1 << 31):
        raise ValueError("mult must be >= 0 and fit int32")
    return np.ascontiguousarray(mult, dtype=np.int32)


def _pose16(T, name):
    T = np.ascontiguousarray(T, dtype=np.float64)
    if T.shape != (4, 4):
        raise ValueError(f"{name} must have shape (4, 4)")
    return T


def check_fgr(mu0, mu_min, division, period, max_iter):
    """The schedule of pcr_fgr_pose as (float, float, float, int, int), the library's own rule, else ValueError."""
    mu0, mu_min, division = float(mu0), float(mu_min), float(division)
    if not (np.isfinite(mu0) and mu0 > 0 and np.isfinite(mu_min) and mu_min > 0):
        raise ValueError("mu0 and mu_min must be finite and > 0")
    if not (np.isfinite(division) and division > 1):
        raise ValueError("division_factor must be finite and > 1")
    if int(period) != period or not 1 <= int(period) < 1 << 31:
        raise ValueError("period must be an integer >= 1")
    if int(max_iter) != max_iter or not 0 <= int(max_iter) < 1 << 31:
        raise ValueError("iterations must be an integer >= 0")
    return mu0, mu_min, division, int(period), int(max_iter)


def fgr_linearize(ctx, src, dst, T, mu, mult=None, want_weight=False):
    """pcr_fgr_linearize: one robust pass over the matches at (T, mu) -> the 29 sums (and the weights l*l (M,) with
    ``want_weight``).  ``ctx`` may be a callable, as for ``pose_score``."""
    src, dst = check_pairs(src, dst)
    m = len(src)
    mult, T, mu = check_mult(mult, m), _pose16(T, "T"), float(mu)
    if not (np.isfinite(mu) and mu > 0):
        raise ValueError("mu must be finite and > 0")
    out = np.zeros(29)
    weight = np.ones(m) if want_weight else None
    if m:
        if callable(ctx):
            ctx = ctx()
        check(lib().pcr_fgr_linearize(ctx.handle, src, dst, m, _ptr(mult), T, mu, out, _ptr(weight)))
    return (out, weight) if want_weight else out


def fgr_pose(ctx, src, dst, T_init, mu0, mu_min, division, period, max_iter, tol=0.0, flags=0, mult=None, want_trace=False):
    """pcr_fgr_pose -> dict(T (4, 4), iterations, status (0 ran out, 1 converged, 2 singular), mu, weights (M,)) and, with
    ``want_trace``, trace (max_iter, 46): T before the step, the 29 sums, mu -- rows beyond ``iterations`` are 0."""
    src, dst = check_pairs(src, dst)
    m = len(src)
    mult, T_init = check_mult(mult, m), _pose16(T_init, "T_init")
    mu0, mu_min, division, period, max_iter = check_fgr(mu0, mu_min, division, period, max_iter)
    T = T_init.copy()
    weight = np.ones(m)
    trace = np.zeros((max_iter, FGR_TRACE)) if want_trace else None
    it, status, mu = C.c_int(0), C.c_int(0), C.c_double(mu0)
    if m and max_iter:
        if callable(ctx):
            ctx = ctx()
        check(lib().pcr_fgr_pose(ctx.handle, src, dst, m, _ptr(mult), T_init, mu0, mu_min, division, period, max_iter, float(tol),
                                 int(flags), T, C.byref(it), C.byref(status), C.byref(mu), _ptr(weight), _ptr(trace)))
    out = {"T": T, "iterations": it.value, "status": status.value, "mu": mu.value, "weights": weight}
    if want_trace:
        out["trace"] = trace
    return out


def fgr_tuples(ctx, src, dst, n_tuples, seed, tuple_scale, min_edge):
    """pcr_fgr_tuples -> (mult (M,) int32, n_valid)."""
    src, dst = check_pairs(src, dst)
    n_tuples, seed = int(n_tuples), int(seed)
    if not 0 <= n_tuples <= RANSAC_H_MAX:
        raise ValueError("n_tuples must be in [0, 2^26]")
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed must be in [0, 2^64)")
    min_edge = check_distance(min_edge, "min_edge")
    tuple_scale = float(np.float32(tuple_scale))
    if not 0 <= tuple_scale <= 1:
        raise ValueError("tuple_scale must be in [0, 1]")
    m = len(src)
    mult, n_valid = np.zeros(m, np.int32), C.c_int64(0)
    if m >= 3 and n_tuples:
        if callable(ctx):
            ctx = ctx()
        check(lib().pcr_fgr_tuples(ctx.handle, src, dst, m, n_tuples, seed, tuple_scale, min_edge, _ptr(mult), C.byref(n_valid)))
    return mult, n_valid.value


def fgr_blocks(m):
    """pcr_fgr_blocks: the grid of the robust pass over m matches (a host-side rule; PCR_FGR_BLOCKS caps it)."""
    return int(lib().pcr_fgr_blocks(int(m)))


def fgr_solo_max(ctx):
    """pcr_fgr_solo_max: the largest match list the single-block form of the loop serves; 0 in a library without it."""
    n = C.c_int64(0)
    check(lib().pcr_fgr_solo_max(ctx.handle, C.byref(n)))
    return n.value


COMPAT_M_MAX, COMPAT_K_MAX = 32768, 64          # PCR_COMPAT_M_MAX, PCR_COMPAT_K_MAX of include/pcr.h


def check_compat(src, dst, d):
    """The matches of the pcr_compat_* calls as C-contiguous float32 (M, 3) arrays -- non-finite values are allowed: such a
    match is compatible with nothing -- and the threshold as a float: M <= PCR_COMPAT_M_MAX, d finite and > 0, else ValueError
    (checked before the GPU is touched)."""
    src, dst = np.asarray(src), np.asarray(dst)
    if src.ndim != 2 or src.shape[1] != 3 or src.shape != dst.shape:
        raise ValueError("src and dst must have one shape (M, 3)")
    if len(src) > COMPAT_M_MAX:
        raise ValueError(f"more than {COMPAT_M_MAX} matches (PCR_COMPAT_M_MAX)")
    d = float(d)
    if not (np.isfinite(d) and d > 0):
        raise ValueError("the compatibility threshold must be finite and > 0")
    return cloud_f32(src, "src and dst", finite=False), cloud_f32(dst, "src and dst", finite=False), d


def compat_bits(ctx, src, dst, d):
    """pcr_compat_bits -> the compatibility matrix (M, ceil(M / 64)) uint64.  ``ctx`` may be a callable, as for ``pose_score``."""
    src, dst, d = check_compat(src, dst, d)
    m = len(src)
    bits = np.zeros((m, (m + 63) // 64), np.uint64)
    if m:
        if callable(ctx):
            ctx = ctx()
        check(lib().pcr_compat_bits(ctx.handle, src, dst, m, d, _ptr(bits)))
    return bits


def compat_degrees(ctx, src, dst, d):
    """pcr_compat_degrees -> (deg1 (M,) int64, deg2 (M,) int64)."""
    src, dst, d = check_compat(src, dst, d)
    m = len(src)
    deg1, deg2 = np.zeros(m, np.int64), np.zeros(m, np.int64)
    if m:
        if callable(ctx):
            ctx = ctx()
        check(lib().pcr_compat_degrees(ctx.handle, src, dst, m, d, _ptr(deg1), _ptr(deg2)))
    return deg1, deg2


def compat_consensus(ctx, src, dst, d, n_seeds, k):
    """pcr_compat_consensus -> dict(deg1 (M,) int64, deg2 (M,) int64, seeds (S,) int32, members (S, k) int32, scores (S, k)
    int32), S = min(n_seeds, M)."""
    src, dst, d = check_compat(src, dst, d)
    if int(n_seeds) != n_seeds or not 1 <= int(n_seeds) < 1 << 31:
        raise ValueError("n_seeds must be an integer >= 1")
    if int(k) != k or not 2 <= int(k) <= COMPAT_K_MAX:
        raise ValueError(f"k must be an integer in [2, {COMPAT_K_MAX}]")
    n_seeds, k, m = int(n_seeds), int(k), len(src)
    s = min(n_seeds, m)
    out = {"deg1": np.zeros(m, np.int64), "deg2": np.zeros(m, np.int64), "seeds": np.full(s, -1, np.int32),
           "members": np.full((s, k), -1, np.int32), "scores": np.full((s, k), -1, np.int32)}
    if m:
        if callable(ctx):
            ctx = ctx()
        n_out = C.c_int(0)
        check(lib().pcr_compat_consensus(ctx.handle, src, dst, m, d, s, k, _ptr(out["deg1"]), _ptr(out["deg2"]), _ptr(out["seeds"]),
                                         _ptr(out["members"]), _ptr(out["scores"]), C.byref(n_out)))
        if n_out.value != s:
            raise PcrError(f"pcr_compat_consensus wrote {n_out.value} seeds, {s} expected")
    return out


def gn_set(ctx, J, r):
    """pcr_gn_set: J (n, d) and r (n), each C-contiguous float32 or float64 -> P (m, n) float64."""
    n, d = J.shape
    P = np.empty((d * (d + 1) // 2 + d + 1, n))
    check(lib().pcr_gn_set(ctx.handle, _ptr(J), int(J.dtype == np.float64), _ptr(r), int(r.dtype == np.float64), n, d, P))
    return P


def coreset(ctx, P, u, k, n_target):
    """pcr_coreset: P (m, n) and u (n) C-contiguous float64 -> (P_sel (m, n_out), w (n_out), idx (n_out))."""
    m, n = P.shape
    cap = max(min(int(n_target), n), 1)
    w, idx, sel = np.empty(cap), np.empty(cap, np.int64), np.empty(m * cap)
    n_out = C.c_int64(0)
    check(lib().pcr_coreset(ctx.handle, P, m, n, u, int(k), int(n_target), C.byref(n_out), w, idx, sel))
    c = n_out.value
    return sel[:m * c].reshape(m, c), w[:c], idx[:c]


def hash64(arr):
    """Content hash of a C-contiguous NumPy array's buffer (pcr_hash64: multi-threaded, 64 bits)."""
    h = C.c_uint64(0)
    check(lib().pcr_hash64(arr.ctypes.data_as(_vp), arr.nbytes, C.byref(h)))
    return h.value


def linearize_rows(target, scan, kind, T, max_dist, flags=FLAG_ICP_RR_QUIRK, want_index=False):
    """pcr_linearize_rows -> (J (n, m, 6), r (n, m), w (n), W (n, 3, 3) or None, idx (n) or None), caller order."""
    n, m = scan.n, (1 if kind in (PLANE, VPLANE) else 3)
    T = np.ascontiguousarray(T, dtype=np.float64).reshape(16)
    J, r, w = np.zeros((n, m, 6)), np.zeros((n, m)), np.zeros(n)
    W = np.zeros((n, 3, 3)) if kind == NDT else None
    idx = np.full(n, -1, np.int64) if want_index else None
    check(lib().pcr_linearize_rows(target.handle, scan.handle, int(kind), T, float(max_dist), int(flags), _ptr(J), _ptr(r), _ptr(w),
                                   _ptr(W) if W is not None else None, _ptr(idx) if idx is not None else None))
    return J, r, w, W, idx


def linearize_weighted(target, scan, kind, T, max_dist, weights, flags=FLAG_ICP_RR_QUIRK):
    """pcr_linearize_weighted -> the 28 weighted sums and the sum of the gated-in weights (see include/pcr.h)."""
    T = np.ascontiguousarray(T, dtype=np.float64).reshape(16)
    out = np.empty(29)
    check(lib().pcr_linearize_weighted(target.handle, scan.handle, int(kind), T, float(max_dist), int(flags),
                                       np.ascontiguousarray(weights, dtype=np.float64), out))
    return out


def scan_coreset(target, scan, kind, T, max_dist, k, n_target, flags=FLAG_ICP_RR_QUIRK):
    """pcr_scan_coreset -> (idx (n_out) ascending caller indices, w (n_out))."""
    T = np.ascontiguousarray(T, dtype=np.float64).reshape(16)
    cap = max(min(int(n_target), scan.n), 1)
    idx, w, n_out = np.empty(cap, np.int64), np.empty(cap), C.c_int64(0)
    check(lib().pcr_scan_coreset(target.handle, scan.handle, int(kind), T, float(max_dist), int(flags), int(k), int(n_target), idx, w,
                                 C.byref(n_out)))
    return idx[:n_out.value].copy(), w[:n_out.value].copy()


def cov6(cov, dtype=np.float32):
    """Covariances as C-contiguous ``dtype`` (N, 6) = xx xy xz yy yz zz; (N, 3, 3) input contributes its upper triangle."""
    cov = np.asarray(cov)
    if cov.ndim == 3 and cov.shape[1:] == (3, 3):
        cov = cov[:, (0, 0, 0, 1, 1, 2), (0, 1, 2, 1, 2, 2)]
    return np.ascontiguousarray(cov, dtype=dtype)


def cov6_f64(cov):
    """Voxel covariances: ``cov6`` in float64."""
    return cov6(cov, np.float64)


def _align(entry, head, T_init, max_iter, tol, max_dist, flags, want_trace, mid=()):
    """entry(*head, T_init, max_iter, tol, max_dist, *mid, flags, T_out, &iterations, trace) -> (T, iterations[, trace rows])."""
    T0 = np.ascontiguousarray(T_init, dtype=np.float64).reshape(16)
    T = np.zeros(16)
    iters = C.c_int(0)
    trace = np.zeros((max(int(max_iter), 1), 45)) if want_trace else None
    check(entry(*head, T0, int(max_iter), float(tol), float(max_dist), *mid, int(flags), T, C.byref(iters), _ptr(trace)))
    T = T.reshape(4, 4)
    if want_trace:
        return T, iters.value, trace[:iters.value]
    return T, iters.value


# ---- robust kernels inside the pass of the four match-list aligners (include/pcr.h) ----------------------------------
ROBUST_NONE, ROBUST_HUBER, ROBUST_CAUCHY, ROBUST_TUKEY, ROBUST_GM = 0, 1, 2, 3, 4
ROBUST_KINDS = {None: ROBUST_NONE, "huber": ROBUST_HUBER, "cauchy": ROBUST_CAUCHY, "tukey": ROBUST_TUKEY, "gm": ROBUST_GM}


class Robust(C.Structure):
    """pcr_robust: a kind (ROBUST_*) and its scale c."""
    _fields_ = [("kind", C.c_int), ("scale", C.c_double)]


def check_robust(robust, scale):
    """``robust`` (None, "huber", "cauchy", "tukey", "gm") and ``scale`` as (kind, float), the library's own rule, else
    ValueError: the scale finite and > 0, and so its square (not read when ``robust`` is None)."""
    if robust not in ROBUST_KINDS:
        raise ValueError('robust must be None, "huber", "cauchy", "tukey" or "gm"')
    scale = float(scale)
    if robust is not None and not (0.0 < scale < np.inf and 0.0 < scale * scale < np.inf):      # (false for NaN)
        raise ValueError("robust_scale must be finite and > 0, and so must its square")
    return ROBUST_KINDS[robust], scale


def _rb(robust):
    """None or (kind, scale) -> the pointer argument of a *_robust entry point (and the object that keeps it alive)."""
    if robust is None:
        return None, None
    rb = Robust(int(robust[0]), float(robust[1]))
    return C.cast(C.pointer(rb), _vp), rb


# ---- the adaptive pass of the same four, and the exact order statistic behind it (include/pcr.h) ----------------------
ROBUST_TRIM = 5
ADAPTIVE_KINDS = {"huber": ROBUST_HUBER, "cauchy": ROBUST_CAUCHY, "tukey": ROBUST_TUKEY, "gm": ROBUST_GM, "trim": ROBUST_TRIM}


class Adaptive(C.Structure):
    """pcr_adaptive: a kind (ROBUST_HUBER .. ROBUST_TRIM), the quantile and the factor of c = factor * sqrt(tau)."""
    _fields_ = [("kind", C.c_int), ("quantile", C.c_double), ("factor", C.c_double)]


def check_adaptive(kind, quantile, factor=1.0):
    """``kind`` ("huber", "cauchy", "tukey", "gm", "trim"), ``quantile`` and ``factor`` as (kind, quantile, factor), the library's
    own rule, else ValueError: the quantile in (0, 1], the factor finite and > 0 (not read under "trim")."""
    if kind not in ADAPTIVE_KINDS:
        raise ValueError('adaptive kind must be "huber", "cauchy", "tukey", "gm" or "trim"')
    quantile, factor = float(quantile), float(factor)
    if not 0.0 < quantile <= 1.0:                                                                 # (false for NaN)
        raise ValueError("the quantile (the trim ratio) must be in (0, 1]")
    if kind != "trim" and not 0.0 < factor < np.inf:
        raise ValueError("the factor of an adaptive robust scale must be finite and > 0")
    return ADAPTIVE_KINDS[kind], quantile, factor


def _ad(adaptive):
    """(kind, quantile, factor) -> the pointer argument of a *_adaptive entry point (and the object that keeps it alive)."""
    ad = Adaptive(int(adaptive[0]), float(adaptive[1]), float(adaptive[2]))
    return C.cast(C.pointer(ad), _vp), ad


def order_statistic(ctx, keys, k):
    """pcr_order_statistic: the k-th smallest (1-based) of the float64 ``keys`` that are < +inf, found on the device, and the
    number of keys <= it -> (value, n_le).  Exact: ``value == np.sort(keys)[k - 1]``."""
    keys = np.ascontiguousarray(keys, dtype=np.float64).ravel()
    value, n_le = C.c_double(0.0), C.c_int64(0)
    check(lib().pcr_order_statistic(ctx.handle, _ptr(keys), keys.size, int(k), C.byref(value), C.byref(n_le)))
    return value.value, n_le.value


# ---- the entry points of the four match-list aligners (include/pcr.h): one table, seven wrappers per unit ----------------
# unit -> (its pass parameter between max_dist and rb / the flags: () or ((name, default),); squared residuals per point)
MATCH_UNITS = {
    "gicp": ((), 1),
    "vgicp": ((), 1),
    "symm": ((("min_cos", 0.0),), 1),
    "color": ((("lambda_geometric", 0.968),), 2),
}


def _trailing(*params):
    """(name, default) pairs -> bind(args, kw): the values of these trailing parameters of a wrapper, given by position or
    by keyword, in order, else TypeError.  (By hand, 0.5 us a call: these wrappers sit inside passes of well under a millisecond.)"""
    def bind(args, kw):
        if len(args) > len(params):
            raise TypeError(f"at most {len(params)} trailing argument(s) ({', '.join(n for n, _ in params)}), got {len(args)}")
        vals = list(args) + [kw.pop(n, d) for n, d in params[len(args):]]
        if kw:
            raise TypeError(f"unexpected keyword argument(s): {', '.join(sorted(kw))}")
        return vals
    return bind


def _match_unit(unit):
    """The seven wrappers of ``unit``, with P its pass parameter (``min_cos=0.0`` / ``lambda_geometric=0.968``; none for gicp, vgicp):
      linearize(target, scan, T, max_dist[, P], flags=0) -> the 29 sums of one pass (pcr_<unit>_linearize)
      align(target, scan, T_init, max_iter, tol, max_dist[, P], flags=0, want_trace=False) -> (T, iterations[, trace rows]):
          the host-driven Gauss-Newton loop over the pass, behind the boundary (pcr_<unit>_align)
      linearize_robust(target, scan, T, max_dist[, P], robust=None, flags=0), align_robust(..., max_dist[, P], robust=None, flags=0,
          want_trace=False): the same through pcr_<unit>_*_robust; ``robust``: (kind, scale), or None -> NULL.  P has no default
      residuals(target, scan, T, max_dist[, P], flags=0) -> the squared residuals in the caller's order, (N,) float64 -- color:
          (N, 2), both rows -- inf where a point has no correspondence (pcr_<unit>_residuals)
      linearize_adaptive(target, scan, T, max_dist[, P], adaptive=(kind, quantile, factor), flags=0) -> (the 29 sums, stats (4,)
          = tau, c, n_le, k) (pcr_<unit>_linearize_adaptive)
      align_adaptive(..., max_dist[, P], adaptive=..., flags=0, want_trace=False) -> (T, iterations, stats rows (iterations, 4)
          [, trace rows]) (pcr_<unit>_align_adaptive)"""
    extra, m = MATCH_UNITS[unit]
    pass_tail, align_tail = _trailing(*extra, ("flags", 0)), _trailing(*extra, ("flags", 0), ("want_trace", False))

    def entry(what):
        return getattr(lib(), f"pcr_{unit}_{what}")

    def floats(args):
        if len(args) != len(extra):
            raise TypeError(f"expected {len(extra)} pass parameter(s) after max_dist, got {len(args)}")
        return tuple(float(v) for v in args)

    def call(what, target, scan, T, max_dist, mid, flags, *out):
        T = np.ascontiguousarray(T, dtype=np.float64).reshape(16)
        check(entry(what)(target.handle, scan.handle, T, float(max_dist), *mid, int(flags), *out))

    def sums(what, *args):
        out = np.empty(29)
        call(what, *args, out)
        return out

    def loop(what, target, scan, head, mid, flags, want_trace):
        return _align(entry(what), (target.handle, scan.handle), *head, flags, want_trace, mid=mid)

    def linearize(target, scan, T, max_dist, *args, **kw):
        *p, flags = pass_tail(args, kw)
        return sums("linearize", target, scan, T, max_dist, floats(p), flags)

    def align(target, scan, T_init, max_iter, tol, max_dist, *args, **kw):
        *p, flags, want_trace = align_tail(args, kw)
        return loop("align", target, scan, (T_init, max_iter, tol, max_dist), floats(p), flags, want_trace)

    def linearize_robust(target, scan, T, max_dist, *args, robust=None, flags=0):
        rb, keep = _rb(robust)
        return sums("linearize_robust", target, scan, T, max_dist, floats(args) + (rb,), flags)

    def align_robust(target, scan, T_init, max_iter, tol, max_dist, *args, robust=None, flags=0, want_trace=False):
        rb, keep = _rb(robust)
        return loop("align_robust", target, scan, (T_init, max_iter, tol, max_dist), floats(args) + (rb,), flags, want_trace)

    def residuals(target, scan, T, max_dist, *args, **kw):
        *p, flags = pass_tail(args, kw)
        out = np.empty((scan.n, m) if m > 1 else (scan.n,))
        call("residuals", target, scan, T, max_dist, floats(p), flags, _ptr(out))
        return out

    def linearize_adaptive(target, scan, T, max_dist, *args, adaptive, flags=0):
        ad, keep = _ad(adaptive)
        out, stats = np.empty(29), np.empty(4)
        call("linearize_adaptive", target, scan, T, max_dist, floats(args) + (ad,), flags, out, stats)
        return out, stats

    def align_adaptive(target, scan, T_init, max_iter, tol, max_dist, *args, adaptive, flags=0, want_trace=False):
        ad, keep = _ad(adaptive)
        T0 = np.ascontiguousarray(T_init, dtype=np.float64).reshape(16)
        T, iters = np.zeros(16), C.c_int(0)
        rows = max(int(max_iter), 1)
        stats, trace = np.zeros((rows, 4)), np.zeros((rows, 45)) if want_trace else None
        check(entry("align_adaptive")(target.handle, scan.handle, T0, int(max_iter), float(tol), float(max_dist), *floats(args), ad, int(flags), T,
                                      C.byref(iters), _ptr(trace), _ptr(stats)))
        res = (T.reshape(4, 4), iters.value, stats[:iters.value])
        return res + (trace[:iters.value],) if want_trace else res

    return {f"{unit}_{f.__name__}": f for f in (linearize, align, linearize_robust, align_robust, residuals, linearize_adaptive, align_adaptive)}


for _unit in MATCH_UNITS:
    globals().update(_match_unit(_unit))


# ---- VGICP with direct voxel neighbourhoods (include/pcr.h): entry points of its own, not a row of MATCH_UNITS -------------
NEIGHBORS = (1, 7, 27)


def vgicp_direct_linearize(target, scan, T, max_dist, neighbors, robust=None, flags=0):
    """pcr_vgicp_direct_linearize -> the 29 sums over the kept (point, voxel) pairs; ``robust``: (kind, scale), or None -> NULL."""
    rb, keep = _rb(robust)
    T = np.ascontiguousarray(T, dtype=np.float64).reshape(16)
    out = np.empty(29)
    check(lib().pcr_vgicp_direct_linearize(target.handle, scan.handle, T, float(max_dist), int(neighbors), rb, int(flags), out))
    return out


def vgicp_direct_align(target, scan, T_init, max_iter, tol, max_dist, neighbors, robust=None, flags=0, want_trace=False):
    """pcr_vgicp_direct_align -> (T, iterations[, trace rows])."""
    rb, keep = _rb(robust)
    return _align(lib().pcr_vgicp_direct_align, (target.handle, scan.handle), T_init, max_iter, tol, max_dist, flags, want_trace,
                  mid=(int(neighbors), rb))


def vgicp_direct_residuals(target, scan, T, max_dist, neighbors, flags=0):
    """pcr_vgicp_direct_residuals -> (N, neighbors) float64 in the caller's order, inf where there is no kept pair."""
    T = np.ascontiguousarray(T, dtype=np.float64).reshape(16)
    out = np.empty((scan.n, max(int(neighbors), 0)))
    check(lib().pcr_vgicp_direct_residuals(target.handle, scan.handle, T, float(max_dist), int(neighbors), int(flags), _ptr(out)))
    return out


_linearize_fast = None


def linearize(target, scan, kind, T, max_dist, flags=FLAG_ICP_RR_QUIRK):
    """One pass of the hot path -> the 29 sums (see include/pcr.h).

    Called once per Gauss-Newton iteration: the binding goes through a second ctypes prototype with plain pointer
    arguments (``numpy.ctypeslib.ndpointer`` re-validates dtype / flags / shape of every array on every call, a few
    microseconds against a 50-150 us pass); the arrays are made float64 C-contiguous right here."""
    global _linearize_fast
    if _linearize_fast is None:
        proto = C.CFUNCTYPE(C.c_int, _vp, _vp, C.c_int, _vp, C.c_double, C.c_uint, _vp)
        _linearize_fast = C.cast(lib().pcr_linearize, proto)
    out = np.empty(29)
    if not (isinstance(T, np.ndarray) and T.dtype == np.float64 and T.flags.c_contiguous and T.size == 16):
        T = np.ascontiguousarray(T, dtype=np.float64).reshape(16)
    if getattr(target, "ghandle", None) is not None:              # a group: the sums over every member's shard
        if getattr(scan, "ghandle", None) is None:
            raise ValueError("a group target needs a scan created on the same group")
        check(lib().pcr_group_linearize(target.ghandle, scan.ghandle, int(kind), T.reshape(16), float(max_dist), int(flags), out))
        return out
    st = _linearize_fast(target.handle, scan.handle, kind, T.ctypes.data, max_dist, flags, out.ctypes.data)
    if st != PCR_OK:
        check(st)
    return out


def align(target, scan, kind, T_init, max_iter, tol, max_dist, flags=FLAG_ICP_RR_QUIRK, want_trace=False):
    """pcr_align: the whole Gauss-Newton loop behind the boundary."""
    if getattr(target, "ghandle", None) is not None:
        if getattr(scan, "ghandle", None) is None:
            raise ValueError("a group target needs a scan created on the same group")
        entry, head = lib().pcr_group_align, (target.ghandle, scan.ghandle, int(kind))
    else:
        entry, head = lib().pcr_align, (target.handle, scan.handle, int(kind))
    return _align(entry, head, T_init, max_iter, tol, max_dist, flags, want_trace)


class ScanBatch:
    """pcr_scan_batch handle: S float32 scans uploaded together, each Morton-sorted as a ``Scan`` of those points is."""

    def __init__(self, ctx, arrays, flags=0):
        if isinstance(ctx, Group):
            raise ValueError("a scan batch lives on one context, not on a group")
        arrays = [np.ascontiguousarray(a, dtype=np.float32) for a in arrays]
        for a in arrays:
            if a.ndim != 2 or a.shape[1] != 3:
                raise ValueError("every scan of a batch must have shape (N, 3)")
        offsets = np.zeros(len(arrays) + 1, np.int64)
        np.cumsum([a.shape[0] for a in arrays], out=offsets[1:])
        xyz = np.concatenate(arrays) if arrays else np.zeros((0, 3), np.float32)
        self.ctx = ctx
        self.offsets = offsets
        h = _vp()
        check(lib().pcr_scan_batch_create(ctx.handle, _ptr(xyz), offsets, len(arrays), int(flags), C.byref(h)))
        self.handle = h
        _live.add(self)

    def size(self):
        """(number of scans, points held on the device)."""
        s, n = C.c_int(0), C.c_int64(0)
        check(lib().pcr_scan_batch_size(self.handle, C.byref(s), C.byref(n)))
        return s.value, n.value

    def close(self):
        if getattr(self, "handle", None) and not _shutdown:
            lib().pcr_scan_batch_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _batch_items(target, batch, Ts, item_scan):
    if getattr(target, "ghandle", None) is not None:
        raise ValueError("batched passes run on one context, not on a group target")
    Ts = np.ascontiguousarray(Ts, dtype=np.float64)
    if Ts.ndim != 3 or Ts.shape[1:] != (4, 4):
        raise ValueError("poses of a batch must have shape (B, 4, 4)")
    if item_scan is not None:
        item_scan = np.ascontiguousarray(item_scan, dtype=np.intc)
        if item_scan.shape != (Ts.shape[0],):
            raise ValueError("item_scan must name one scan per pose")
    return Ts, item_scan


def linearize_batch(target, batch, kind, Ts, max_dist, flags=FLAG_ICP_RR_QUIRK, item_scan=None):
    """pcr_linearize_batch: item i = scan ``item_scan[i]`` of ``batch`` (None: scan i) at ``Ts[i]`` -> (B, 29) sums."""
    Ts, item_scan = _batch_items(target, batch, Ts, item_scan)
    out = np.zeros((Ts.shape[0], 29))
    check(lib().pcr_linearize_batch(target.handle, batch.handle, int(kind), Ts.shape[0], _ptr(item_scan), Ts.reshape(-1),
                                    float(max_dist), int(flags), out.reshape(-1)))
    return out


def align_batch(target, batch, kind, T_init, max_iter, tol, max_dist, flags=FLAG_ICP_RR_QUIRK, item_scan=None,
                want_trace=False):
    """pcr_align_batch: the Gauss-Newton loops of all items, one launch per iteration for the whole batch ->
    (T (B, 4, 4), iterations (B,), status (B,) of PCR_OK / PCR_ERR_SINGULAR[, trace (B, max_iter, 45)])."""
    T0, item_scan = _batch_items(target, batch, T_init, item_scan)
    B = T0.shape[0]
    T = np.zeros((B, 16))
    iters = np.zeros(B, np.intc)
    status = np.zeros(B, np.intc)
    trace = np.zeros((B, max(int(max_iter), 1), 45)) if want_trace else None
    check(lib().pcr_align_batch(target.handle, batch.handle, int(kind), B, _ptr(item_scan), T0.reshape(-1), int(max_iter),
                                float(tol), float(max_dist), int(flags), T.reshape(-1), _ptr(iters), _ptr(status), _ptr(trace)))
    T = T.reshape(B, 4, 4)
    if want_trace:
        return T, iters, status, trace
    return T, iters, status


def nn_counters(target, scan, T, max_dist):
    """Search work counters for one pose (see include/pcr.h: pcr_nn_counters)."""
    out = np.zeros(11)
    check(lib().pcr_nn_counters(target.handle, scan.handle, np.ascontiguousarray(T, np.float64).reshape(16),
                                float(max_dist), out))
    names = ("rings", "rows_loaded", "rows_pruned", "candidates")
    n = max(scan.n, 1)
    waves = max((scan.n + 63) // 64, 1)
    return {**{k: out[i] / n for i, k in enumerate(names)},
            **{"wave_" + k: out[4 + i] / n for i, k in enumerate(names)},
            "cyc_prologue": out[8] / waves, "cyc_ring0": out[9] / waves, "cyc_rings": out[10] / waves}


def nn_counters_x(target, scan, T, max_dist):
    """Per query, on a target in the old order inside a cell: candidates tested and how many of them an x-ordered scan could
    not have skipped, against the best at the time / the final best (see include/pcr.h: pcr_nn_counters_x)."""
    out = np.zeros(3)
    check(lib().pcr_nn_counters_x(target.handle, scan.handle, np.ascontiguousarray(T, np.float64).reshape(16),
                                  float(max_dist), out))
    n = max(scan.n, 1)
    return {"candidates": out[0] / n, "x_now": out[1] / n, "x_final": out[2] / n}


def nn_counters_edge(target, scan, T, max_dist):
    """The queries outside the target's grid box against those inside it (see include/pcr.h: pcr_nn_counters_edge): their
    share of the queries and of the 64-query tiles, candidates and row segments per query of either class, the share of
    all candidates (per lane, and charged at each wave's maximum) that falls on the outside ones, and the candidates per
    query of the in-grid queries that start from a cell seed."""
    e = np.zeros(9)
    a = np.zeros(11)
    Tf = np.ascontiguousarray(T, np.float64).reshape(16)
    check(lib().pcr_nn_counters_edge(target.handle, scan.handle, Tf, float(max_dist), e))
    check(lib().pcr_nn_counters(target.handle, scan.handle, Tf, float(max_dist), a))
    n = max(scan.n, 1)
    n_out, n_in = max(e[0], 1), max(n - e[0], 1)
    return {"out_share": e[0] / n, "out_tile_share": e[5] / max(e[6], 1),
            "cand_out": e[1] / n_out, "cand_in": (a[3] - e[1]) / n_in, "rows_out": e[2] / n_out, "rows_in": (a[1] - e[2]) / n_in,
            "wave_cand_out": e[3] / n_out, "wave_cand_in": (a[7] - e[3]) / n_in,
            "cand_share_out": e[1] / max(a[3], 1), "wave_cand_share_out": e[3] / max(a[7], 1), "wave_rows_share_out": e[4] / max(a[5], 1),
            "empty_in_share": e[7] / n, "cand_empty_in": e[8] / max(e[7], 1)}


def unpack29(out):
    """29 sums -> (H 6x6 symmetric, g 6, e2, count)."""
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = out[:21]
    H = H + np.triu(H, 1).T
    return H, np.array(out[21:27]), float(out[27]), int(round(out[28]))
