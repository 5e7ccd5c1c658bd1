"""ctypes mirror of the C ABI in include/osg.h and include/osg_ba.h.

Only plain pointers and sizes cross the boundary; every pointer field is a ``c_void_p`` filled
from a numpy array's address by the helpers in this package.  The structures are shared by the
product bindings (liborbslam3_amd.so); the oracle's (test infrastructure) are in tests/oracle_calls.py.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# OSG_LIB_PATH points the package at another build of the same library (a profiling build)
LIB_PATH = os.environ.get("OSG_LIB_PATH") or os.path.join(_HERE, "liborbslam3_amd.so")

OSG_OK = 0
OSG_E_INVALID = -1
OSG_E_HIP = -2
OSG_E_NOMEM = -3
OSG_E_UNSUPPORTED = -4
OSG_E_NODEVICE = -5

TH_HIGH = 100
TH_LOW = 50
HISTO_LENGTH = 30
GRID_COLS = 64
GRID_ROWS = 48
GRID_CELLS = GRID_COLS * GRID_ROWS

CAM_PINHOLE = 0
CAM_KB8 = 1
EDGE_MONO = 0
EDGE_STEREO = 1
EDGE_BODY = 2

P = C.c_void_p
i32 = C.c_int32
f32 = C.c_float
f64 = C.c_double


class OsgFrame(C.Structure):
    _fields_ = [
        ("n", i32), ("nleft", i32), ("desc", P), ("kp_x", P), ("kp_y", P), ("kp_angle", P),
        ("kp_octave", P), ("u_right", P), ("grid_start", P), ("grid_idx", P),
        ("grid_start_r", P), ("grid_idx_r", P), ("left_to_right", P), ("right_to_left", P),
        ("min_x", f32), ("max_x", f32), ("min_y", f32), ("max_y", f32),
        ("grid_inv_w", f32), ("grid_inv_h", f32), ("scale_factors", P), ("n_levels", i32),
        ("mb", f32), ("mbf", f32),
    ]


class OsgMpQueries(C.Structure):
    _fields_ = [
        ("n", i32), ("mp_id", P), ("desc", P), ("usable", P), ("has_obs", P), ("in_view", P),
        ("proj_x", P), ("proj_y", P), ("proj_xr", P), ("view_cos", P), ("pred_level", P),
        ("track_depth", P), ("in_view_r", P), ("proj_yr", P), ("view_cos_r", P),
        ("pred_level_r", P),
    ]


class OsgLastQueries(C.Structure):
    _fields_ = [
        ("n", i32), ("mp_id", P), ("desc", P), ("valid", P), ("has_obs", P), ("u", P),
        ("v", P), ("invz", P), ("u_r", P), ("v_r", P), ("octave", P), ("angle", P),
        ("tlc_z", f32),
    ]


class OsgKfQueries(C.Structure):
    _fields_ = [
        ("n", i32), ("mp_id", P), ("desc", P), ("valid", P), ("u", P), ("v", P),
        ("pred_level", P), ("angle", P),
    ]


class OsgFuseQueries(C.Structure):
    _fields_ = [
        ("n", i32), ("desc", P), ("valid", P), ("u", P), ("v", P), ("ur", P), ("pred_level", P),
        ("inv_level_sigma2", P),
    ]


class OsgFeatVec(C.Structure):
    _fields_ = [("n_nodes", i32), ("node_id", P), ("node_start", P), ("feat", P)]


class OsgBowSide(C.Structure):
    _fields_ = [
        ("n", i32), ("nleft", i32), ("desc", P), ("angle", P), ("mp_id", P), ("mp_good", P),
        ("fv", OsgFeatVec),
    ]


class OsgKfSide(C.Structure):
    _fields_ = [
        ("n", i32), ("nleft", i32), ("two_cam", i32), ("desc", P), ("kp_x", P), ("kp_y", P), ("kp_angle", P),
        ("kp_octave", P), ("u_right", P), ("has_mp", P), ("level_sigma2", P), ("scale_factors", P),
        ("n_levels", i32), ("fv", OsgFeatVec),
    ]


class OsgTriangGeom(C.Structure):
    _fields_ = [("ep_x", f32), ("ep_y", f32), ("F12", f32 * 36), ("pinhole", i32), ("R12", f32 * 36),
                ("t12", f32 * 12), ("kb", f32 * 32)]


class OsgNpKf(C.Structure):
    _fields_ = [("Tcw", f32 * 24), ("Ow", f32 * 6), ("Rwc", f32 * 9), ("twc", f32 * 3), ("cam_type", i32),
                ("cam", f32 * 16), ("fx", f32), ("fy", f32), ("cx", f32), ("cy", f32), ("invfx", f32), ("invfy", f32),
                ("mb", f32), ("mbf", f32), ("depth", P), ("keys_x", P), ("keys_y", P), ("median_depth", f32)]


class OsgNewPointsProblem(C.Structure):
    _fields_ = [("kf1", OsgKfSide), ("g1", OsgNpKf), ("n_neigh", i32), ("kf2", P), ("g2", P), ("geom", P),
                ("monocular", i32), ("inertial", i32), ("coarse", i32), ("far_points", i32),
                ("th_far_points", f32), ("ratio_factor", f32)]


class OsgNewPointsResult(C.Structure):
    _fields_ = [("match", P), ("status", P), ("x3d", P), ("skipped", P), ("n_created", P)]


NEWPOINTS_MAX_NEIGHBOURS = 64
NP_NONE, NP_CREATED, NP_LOW_PARALLAX, NP_NO_POINT, NP_Z1, NP_Z2 = 0, 1, 2, 3, 4, 5
NP_REPROJ1, NP_REPROJ2, NP_ZERO_DIST, NP_FAR, NP_SCALE = 6, 7, 8, 9, 10
NP_STEREO_BIT = 0x80


FRUSTUM_NOT_CANDIDATE, FRUSTUM_NEG_DEPTH, FRUSTUM_OUTSIDE, FRUSTUM_DISTANCE, FRUSTUM_VIEW_COS, FRUSTUM_IN_VIEW = range(6)


class OsgFrustumCamera(C.Structure):
    _fields_ = [("R", f32 * 9), ("t", f32 * 3), ("c", f32 * 3), ("cam_type", i32), ("cam", f32 * 8)]


class OsgFrustumFrame(C.Structure):
    _fields_ = [("two_cam", i32), ("cam", OsgFrustumCamera * 2), ("min_x", f32), ("max_x", f32), ("min_y", f32),
                ("max_y", f32), ("mbf", f32), ("log_scale_factor", f32), ("n_levels", i32)]


class OsgFrustumPoints(C.Structure):
    _fields_ = [("n", i32), ("pos", P), ("normal", P), ("max_dist", P), ("min_dist", P), ("candidate", P),
                ("prev_depth", P)]


class OsgFrustumResult(C.Structure):
    _fields_ = [("status", P * 2), ("proj_x", P * 2), ("proj_y", P * 2), ("proj_xr", P), ("view_cos", P * 2),
                ("depth", P * 2), ("level", P * 2), ("n_to_match", i32)]


class OsgLocalPoints(C.Structure):
    _fields_ = [("pts", OsgFrustumPoints), ("mp_id", P), ("desc", P), ("has_obs", P)]


class OsgImagePyramid(C.Structure):
    _fields_ = [("n_levels", i32), ("on_device", i32), ("data", P), ("rows", P), ("cols", P), ("step", P)]


class OsgStereoFrame(C.Structure):
    _fields_ = [
        ("n", i32), ("x", P), ("y", P), ("octave", P), ("desc", P), ("n_right", i32), ("xr", P), ("yr", P),
        ("octave_r", P), ("desc_r", P), ("scale_factors", P), ("inv_scale_factors", P), ("n_levels", i32),
        ("mb", f32), ("mbf", f32), ("left", OsgImagePyramid), ("right", OsgImagePyramid),
    ]


class OsgOrbExtractParams(C.Structure):
    _fields_ = [
        ("n_levels", i32), ("scale_factors", P), ("inv_scale_factors", P), ("n_features_per_level", P),
        ("ini_th_fast", i32), ("min_th_fast", i32), ("pattern", P), ("umax", P),
    ]


class OsgOrbKeypoints(C.Structure):
    _fields_ = [("n", i32), ("x", P), ("y", P), ("level", P)]


class OsgCamera(C.Structure):
    _fields_ = [
        ("type", i32), ("p", f32 * 8), ("fx", f32), ("fy", f32), ("cx", f32), ("cy", f32),
        ("bf", f32), ("trl", f64 * 7),
    ]


class OsgPoseProblem(C.Structure):
    _fields_ = [
        ("pose", f64 * 7), ("n_edges", i32), ("kind", P), ("xw", P), ("obs", P),
        ("inv_sigma2", P), ("cam", OsgCamera), ("cam2", OsgCamera),
    ]


class OsgPoseResult(C.Structure):
    _fields_ = [
        ("pose", f64 * 7), ("outlier", P), ("n_inliers", i32), ("lm_iterations", i32),
        ("lm_trials", i32),
    ]


class OsgPioState(C.Structure):
    _fields_ = [("Rwb", f64 * 9), ("twb", f64 * 3), ("v", f64 * 3), ("bg", f64 * 3), ("ba", f64 * 3)]


class OsgPioCamera(C.Structure):
    _fields_ = [("cam", OsgCamera), ("Rcw", f64 * 9), ("tcw", f64 * 3), ("Rcb", f64 * 9), ("tcb", f64 * 3),
                ("tbc", f64 * 3)]


class OsgPioPreintegrated(C.Structure):
    _fields_ = [
        ("dR", f32 * 9), ("dV", f32 * 3), ("dP", f32 * 3), ("JRg", f32 * 9), ("JVg", f32 * 9), ("JVa", f32 * 9),
        ("JPg", f32 * 9), ("JPa", f32 * 9), ("b", f32 * 6), ("dT", f32), ("C", f32 * 225),
    ]


class OsgImuPreintegrated(C.Structure):
    _fields_ = [("pre", OsgPioPreintegrated), ("avgA", f32 * 3), ("avgW", f32 * 3)]


class OsgImuProblem(C.Structure):
    _fields_ = [("meas", P), ("n", i32), ("bias", f32 * 6), ("nga", f32 * 6), ("nga_walk", f32 * 6), ("init", P)]


OSG_IMU_MAX_STEPS = 65536
OSG_IMU_MAX_BATCH_STEPS = 1 << 24


class OsgPioPrior(C.Structure):
    _fields_ = [("Rwb", f64 * 9), ("twb", f64 * 3), ("vwb", f64 * 3), ("bg", f64 * 3), ("ba", f64 * 3),
                ("H", f64 * 225)]


class OsgPoseInertialProblem(C.Structure):
    _fields_ = [
        ("mode", i32), ("rec_init", i32), ("cur", OsgPioState), ("prev", OsgPioState), ("n_cams", i32),
        ("cams", OsgPioCamera * 2), ("bf", f64), ("n_edges", i32), ("kind", P), ("xw", P), ("obs", P),
        ("inv_sigma2", P), ("track_depth", P), ("preint", P), ("C_rw", P), ("prior", P),
    ]


class OsgPoseInertialResult(C.Structure):
    _fields_ = [
        ("state", OsgPioState), ("outlier", P), ("n_inliers", i32), ("rounds_run", i32), ("iterations", i32),
        ("solve_failed", i32), ("recovered", i32), ("H", f64 * 225), ("edge_chi2", P),
    ]


OSG_PIO_LAST_KEYFRAME = 0
OSG_PIO_LAST_FRAME = 1


class OsgInertialProblem(C.Structure):
    _fields_ = [
        ("n_kf", i32), ("Rwb", P), ("twb", P), ("v", P), ("n_edges", i32), ("prev", P), ("cur", P), ("preint", P),
        ("bg", f64 * 3), ("ba", f64 * 3), ("Rwg", f64 * 9), ("scale", f64), ("prior_g", f64), ("prior_a", f64),
        ("has_priors", i32), ("free_vel_bias", i32), ("free_gdir", i32), ("free_scale", i32), ("algorithm", i32),
        ("iterations", i32), ("lambda_init", f64), ("huber_delta", f64),
    ]


class OsgInertialResult(C.Structure):
    _fields_ = [
        ("v", P), ("bg", f64 * 3), ("ba", f64 * 3), ("Rwg", f64 * 9), ("scale", f64), ("chi2_initial", f64),
        ("chi2_final", f64), ("iterations", i32), ("trials_rejected", i32), ("solve_failed", i32), ("trace", P),
    ]


OSG_INERTIAL_LM = 0
OSG_INERTIAL_GN = 1
OSG_INERTIAL_MAX_KF = 4096
OSG_INERTIAL_MAX_ITERATIONS = 1000


class OsgLibaKeyframe(C.Structure):
    _fields_ = [("state", OsgPioState), ("fixed", i32), ("n_cams", i32), ("cams", OsgPioCamera * 2), ("bf", f64)]


class OsgLibaLink(C.Structure):
    _fields_ = [("prev", i32), ("cur", i32), ("huber", i32), ("downweight", i32), ("preint", OsgPioPreintegrated)]


class OsgLocalInertialBaProblem(C.Structure):
    _fields_ = [
        ("n_kf", i32), ("kf", P), ("n_points", i32), ("xw", P), ("track_depth", P), ("n_edges", i32), ("e_point", P),
        ("e_kf", P), ("e_kind", P), ("e_obs", P), ("e_inv_sigma2", P), ("n_links", i32), ("links", P),
        ("iterations", i32), ("large", i32), ("lambda_init", f64),
    ]


class OsgLocalInertialBaResult(C.Structure):
    _fields_ = [
        ("state", P), ("Rcw", P), ("tcw", P), ("xw", P), ("edge_bad", P), ("edge_chi2", P), ("chi2_initial", f64),
        ("chi2_last", f64), ("chi2_accepted", f64), ("iterations", i32), ("trials_rejected", i32),
        ("solve_failed", i32), ("failed", i32), ("trace", P),
    ]


OSG_LIBA_MAX_FREE_KF = 32
OSG_LIBA_MAX_FIXED_KF = 512
OSG_LIBA_MAX_POINTS = 65536
OSG_LIBA_MAX_EDGES = 524288
OSG_LIBA_MAX_PAIRS = 16777216
OSG_LIBA_MAX_ITERATIONS = 100


class OsgSim3Problem(C.Structure):
    _fields_ = [
        ("q", f64 * 4), ("t", f64 * 3), ("s", f64), ("fix_scale", i32), ("th2", f32),
        ("cam1", OsgCamera), ("cam2", OsgCamera), ("n_pairs", i32), ("p1c", P), ("p2c", P),
        ("obs1", P), ("obs2", P), ("inv_sigma2_1", P), ("inv_sigma2_2", P), ("max_iterations", i32),
    ]


class OsgSim3Result(C.Structure):
    _fields_ = [
        ("q", f64 * 4), ("t", f64 * 3), ("s", f64), ("n_inliers", i32), ("pair_state", P),
        ("n_bad_first", i32), ("lm_iterations", i32 * 2), ("lm_trials", i32 * 2), ("chi2_final", f64),
        ("pair_chi2", P), ("early_return", i32),
    ]


class OsgSim3RansacProblem(C.Structure):
    _fields_ = [
        ("n", i32), ("p1c", P), ("p2c", P), ("max_err1", P), ("max_err2", P), ("cam1", OsgCamera),
        ("cam2", OsgCamera), ("fix_scale", i32), ("min_inliers", i32), ("n_hyp", i32), ("samples", P),
    ]


class OsgSim3RansacResult(C.Structure):
    _fields_ = [
        ("converged", i32), ("hyp", i32), ("n_iterations", i32), ("n_inliers", i32), ("n_best", i32),
        ("R", f32 * 9), ("t", f32 * 3), ("s", f32), ("T12", f32 * 16), ("inlier", P), ("hyp_inliers", P),
        ("hyp_sim3", P),
    ]


class OsgMlpnpProblem(C.Structure):
    _fields_ = [
        ("n", i32), ("bearing", P), ("p3dw", P), ("p2d", P), ("max_err", P), ("cam", OsgCamera),
        ("min_inliers", i32), ("n_hyp", i32), ("samples", P),
    ]


class OsgMlpnpResult(C.Structure):
    _fields_ = [
        ("converged", i32), ("hyp", i32), ("n_iterations", i32), ("n_inliers", i32), ("n_best", i32),
        ("Tcw", f32 * 16), ("R", f64 * 9), ("t", f64 * 3), ("inlier", P), ("hyp_inliers", P), ("hyp_pose", P),
        ("hyp_info", P),
    ]


class OsgTwoViewProblem(C.Structure):
    _fields_ = [
        ("K", f32 * 4), ("sigma", f32), ("n_hyp", i32), ("n", i32), ("kp1", P), ("kp2", P), ("n_keys1", i32),
        ("n_keys2", i32), ("keys1", P), ("keys2", P), ("idx1", P), ("idx2", P), ("sets", P), ("min_parallax", f32),
        ("min_triangulated", i32),
    ]


class OsgTwoViewResult(C.Structure):
    _fields_ = [
        ("ok", i32), ("model", i32), ("score_h", f32), ("score_f", f32), ("hyp_h", i32), ("hyp_f", i32),
        ("H21", f32 * 9), ("F21", f32 * 9), ("R", f32 * 9), ("t", f32 * 3), ("cand", i32), ("n_inliers", i32),
        ("n_good", i32 * 8), ("parallax", f32 * 8), ("cand_Rt", f32 * 96), ("p3d", P), ("triangulated", P),
        ("inlier_h", P), ("inlier_f", P), ("hyp_score_h", P), ("hyp_score_f", P), ("hyp_models", P),
    ]


class OsgEssGraphProblem(C.Structure):
    _fields_ = [
        ("n_vertices", i32), ("sim3", P), ("fixed", P), ("fix_scale", i32), ("n_edges", i32), ("e_v0", P),
        ("e_v1", P), ("e_meas", P), ("max_iterations", i32), ("lambda_init", f64),
    ]


class OsgEssGraphResult(C.Structure):
    _fields_ = [
        ("sim3", P), ("chi2_initial", f64), ("chi2_final", f64), ("lm_iterations", i32), ("lm_trials", i32),
        ("edge_chi2", P),
    ]


class OsgEssGraph4Problem(C.Structure):
    _fields_ = [
        ("n_vertices", i32), ("pose", P), ("fixed", P), ("n_edges", i32), ("e_v0", P), ("e_v1", P), ("e_meas", P),
        ("info_diag", f64 * 6), ("max_iterations", i32), ("lambda_init", f64),
    ]


class OsgEssGraph4Result(C.Structure):
    _fields_ = [
        ("pose", P), ("chi2_initial", f64), ("chi2_final", f64), ("lm_iterations", i32), ("lm_trials", i32),
        ("edge_chi2", P),
    ]


class OsgBaGraph(C.Structure):
    _fields_ = [
        ("n_poses", i32), ("pose", P), ("pose_fixed", P), ("n_points", i32), ("point", P),
        ("n_edges", i32), ("e_point", P), ("e_pose", P), ("e_kind", P), ("e_cam", P),
        ("e_obs", P), ("e_inv_sigma2", P), ("n_cams", i32), ("cams", P), ("iterations", i32),
        ("user_lambda_init", f64), ("e_robust", P), ("huber_mono", f32), ("huber_stereo", f32),
    ]


class OsgBaResult(C.Structure):
    _fields_ = [
        ("pose", P), ("point", P), ("edge_bad", P), ("iterations", i32), ("trials", i32),
        ("chi2_initial", f64), ("chi2_final", f64), ("aborted", i32), ("edge_chi2", P),
    ]


class OsgVocabularyDesc(C.Structure):
    _fields_ = [
        ("k", i32), ("L", i32), ("scoring", i32), ("weighting", i32), ("n_nodes", i32),
        ("parent", P), ("is_leaf", P), ("desc", P), ("weight", P),
    ]


class OsgBowOut(C.Structure):
    _fields_ = [
        ("n_words", i32), ("word", P), ("value", P), ("n_nodes", i32), ("node_id", P),
        ("node_start", P), ("feat", P),
    ]


class OsgKfdbState(C.Structure):
    _fields_ = [
        ("place_query", C.c_int64), ("reloc_query", C.c_int64), ("place_words", i32), ("reloc_words", i32),
        ("place_score", f32), ("reloc_score", f32),
    ]


class OsgKfdbQueryOut(C.Structure):
    _fields_ = [
        ("n_sharing", i32), ("max_common_words", i32), ("min_common_words", i32), ("n_scored", i32),
        ("capacity", i32), ("entry", P), ("words", P), ("score", P), ("score_f64", P),
    ]


class OsgKfdbKf(C.Structure):
    _fields_ = [
        ("query", C.c_int64), ("score", f32), ("handle", i32), ("map_id", i32), ("bad", C.c_uint8),
        ("map_bad", C.c_uint8), ("pad", C.c_uint8 * 2),
    ]


OSG_KFDB_PLACE = 0
OSG_KFDB_RELOC = 1
OSG_KFDB_MAX_NEIGH = 10


# Every symbol include/osg.h, include/osg_ba.h and include/osg_dbow.h declare (checked by tests/test_abi.py).
EXPORTS = [
    "osg_ctx_create", "osg_ctx_destroy", "osg_ctx_set_stream", "osg_ctx_stream",
    "osg_ctx_synchronize", "osg_strerror", "osg_ctx_last_error", "osg_version",
    "osg_descriptor_distance", "osg_descriptor_distance_pairs", "osg_hamming_top2",
    "osg_hamming_top2_dev", "osg_hamming_top2_batch_dev", "osg_hamming_top2_plan", "osg_hamming_top2_batch_plan", "osg_search_by_projection_mps", "osg_search_by_projection_last",
    "osg_search_by_projection_kf", "osg_search_by_bow_kf_f", "osg_search_by_bow_kf_kf",
    "osg_search_by_projection_mps_batch", "osg_search_by_projection_last_batch",
    "osg_search_by_projection_kf_batch", "osg_search_by_bow_kf_f_batch", "osg_search_by_bow_kf_kf_batch",
    "osg_match_last_stats", "osg_match_last_path", "osg_debug_match_plan", "osg_ctx_last_kernel_ms", "osg_ctx_device_bytes", "osg_pose_optimization", "osg_pose_optimization_batch",
    "osg_local_bundle_adjustment", "osg_local_bundle_adjustment_batch", "osg_bundle_adjustment",
    "osg_lba_kernel_times", "osg_optimize_sim3", "osg_optimize_sim3_batch",
    "osg_pose_inertial_optimization", "osg_pose_inertial_optimization_batch", "osg_pose_inertial_check",
    "osg_pose_inertial_informations",
    "osg_inertial_optimization", "osg_inertial_optimization_batch", "osg_inertial_check",
    "osg_local_inertial_ba", "osg_local_inertial_ba_batch", "osg_local_inertial_ba_check",
    "osg_sim3_ransac", "osg_sim3_ransac_batch", "osg_sim3_ransac_iterations",
    "osg_mlpnp_ransac", "osg_mlpnp_ransac_batch", "osg_mlpnp_ransac_parameters", "osg_mlpnp_check_samples",
    "osg_optimize_essential_graph", "osg_essgraph_correct_points", "osg_essgraph_kernel_times",
    "osg_optimize_essential_graph_4dof", "osg_essgraph4_check",
    "osg_vocabulary_create", "osg_vocabulary_load_text", "osg_vocabulary_destroy", "osg_vocabulary_info",
    "osg_vocabulary_transform", "osg_vocabulary_transform_batch",
    "osg_kfdb_create", "osg_kfdb_destroy", "osg_kfdb_size", "osg_kfdb_add", "osg_kfdb_erase",
    "osg_kfdb_clear", "osg_kfdb_clear_map", "osg_kfdb_state_get", "osg_kfdb_state_set", "osg_kfdb_query",
    "osg_kfdb_select_nbest", "osg_kfdb_select_reloc",
    "osg_fuse_search", "osg_fuse_search_batch", "osg_search_for_triangulation", "osg_search_for_triangulation_batch",
    "osg_create_new_map_points", "osg_create_new_map_points_batch", "osg_create_new_map_points_check",
    "osg_frustum", "osg_frustum_batch", "osg_frustum_check", "osg_search_local_points",
    "osg_search_local_points_batch",
    "osg_compute_distinctive_descriptors", "osg_compute_distinctive_descriptors_dev",
    "osg_search_by_projection_sim3", "osg_search_by_projection_sim3_batch", "osg_search_by_sim3",
    "osg_search_for_initialization", "osg_search_for_initialization_batch",
    "osg_two_view_reconstruct", "osg_two_view_reconstruct_batch", "osg_two_view_kernel_times",
    "osg_compute_stereo_matches", "osg_compute_stereo_matches_batch", "osg_compute_stereo_fisheye_matches",
    "osg_orb_describe", "osg_orb_detect", "osg_orb_extract_batch",
    "osg_debug_distribute_oct_tree", "osg_orb_pyramid_layout", "osg_orb_pyramid", "osg_debug_gaussian_kernel7",
]

# Every symbol include/osg_imu.h declares (checked by tests/test_preintegration_abi.py).
IMU_EXPORTS = [
    "osg_imu_preintegrate", "osg_imu_preintegrate_batch", "osg_imu_preintegrate_check",
    "osg_imu_select", "osg_imu_integrables", "osg_imu_delta", "osg_imu_predict_state",
]


def declare(lib: C.CDLL) -> C.CDLL:
    """Attach argtypes/restypes for the product library."""
    vp = C.c_void_p
    lib.osg_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    lib.osg_ctx_destroy.argtypes = [vp]
    lib.osg_ctx_set_stream.argtypes = [vp, vp]
    lib.osg_ctx_stream.argtypes = [vp]
    lib.osg_ctx_stream.restype = vp
    lib.osg_ctx_synchronize.argtypes = [vp]
    lib.osg_strerror.argtypes = [C.c_int]
    lib.osg_strerror.restype = C.c_char_p
    lib.osg_ctx_last_error.argtypes = [vp]
    lib.osg_ctx_last_error.restype = C.c_char_p
    lib.osg_version.argtypes = []
    lib.osg_version.restype = C.c_char_p
    lib.osg_descriptor_distance.argtypes = [vp, vp]
    lib.osg_descriptor_distance_pairs.argtypes = [vp, vp, vp, i32, vp]
    lib.osg_hamming_top2.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp]
    lib.osg_hamming_top2_dev.argtypes = [vp, vp, i32, vp, i32, vp]
    lib.osg_hamming_top2_batch_dev.argtypes = [vp, vp, i32, vp, i32, i32, vp]
    lib.osg_hamming_top2_plan.argtypes = [vp, i32, i32, C.c_char_p, i32]
    lib.osg_hamming_top2_batch_plan.argtypes = [vp, i32, i32, i32, C.c_char_p, i32]
    lib.osg_search_by_projection_mps.argtypes = [vp, C.POINTER(OsgFrame), C.POINTER(OsgMpQueries),
                                                 f32, f32, C.c_int, f32, vp, vp]
    lib.osg_search_by_projection_last.argtypes = [vp, C.POINTER(OsgFrame),
                                                  C.POINTER(OsgLastQueries), f32, C.c_int, C.c_int,
                                                  vp, vp]
    lib.osg_search_by_projection_kf.argtypes = [vp, C.POINTER(OsgFrame), C.POINTER(OsgKfQueries),
                                                f32, C.c_int, C.c_int, vp]
    lib.osg_search_by_bow_kf_f.argtypes = [vp, C.POINTER(OsgBowSide), C.POINTER(OsgBowSide), f32,
                                           C.c_int, vp]
    lib.osg_search_by_bow_kf_kf.argtypes = [vp, C.POINTER(OsgBowSide), C.POINTER(OsgBowSide), f32,
                                            C.c_int, vp]
    lib.osg_search_by_projection_mps_batch.argtypes = [vp, vp, vp, i32, f32, f32, C.c_int, f32, vp, vp, vp]
    lib.osg_search_by_projection_last_batch.argtypes = [vp, vp, vp, i32, f32, C.c_int, C.c_int, vp, vp, vp]
    lib.osg_search_by_projection_kf_batch.argtypes = [vp, vp, vp, i32, f32, C.c_int, C.c_int, vp, vp]
    lib.osg_search_by_bow_kf_f_batch.argtypes = [vp, vp, vp, i32, f32, C.c_int, vp, vp]
    lib.osg_search_by_bow_kf_kf_batch.argtypes = [vp, vp, vp, i32, f32, C.c_int, vp, vp]
    lib.osg_match_last_stats.argtypes = [vp, vp]
    lib.osg_match_last_path.argtypes = [vp, vp]
    lib.osg_debug_match_plan.argtypes = [i32, i32, i32, i32, C.POINTER(i32), C.POINTER(C.c_int64)]
    lib.osg_ctx_last_kernel_ms.argtypes = [vp, vp]
    lib.osg_ctx_device_bytes.argtypes = [vp, vp]
    lib.osg_pose_optimization.argtypes = [vp, C.POINTER(OsgPoseProblem), C.POINTER(OsgPoseResult)]
    lib.osg_pose_optimization_batch.argtypes = [vp, C.POINTER(OsgPoseProblem), i32,
                                                C.POINTER(OsgPoseResult)]
    lib.osg_pose_inertial_optimization.argtypes = [vp, C.POINTER(OsgPoseInertialProblem),
                                                   C.POINTER(OsgPoseInertialResult)]
    lib.osg_pose_inertial_optimization_batch.argtypes = [vp, C.POINTER(OsgPoseInertialProblem), i32,
                                                         C.POINTER(OsgPoseInertialResult)]
    lib.osg_pose_inertial_check.argtypes = [C.POINTER(OsgPoseInertialProblem)]
    lib.osg_pose_inertial_informations.argtypes = [vp, vp, vp, vp, vp]
    lib.osg_pose_inertial_informations.restype = None
    lib.osg_inertial_optimization.argtypes = [vp, C.POINTER(OsgInertialProblem), C.POINTER(OsgInertialResult)]
    lib.osg_inertial_optimization_batch.argtypes = [vp, C.POINTER(OsgInertialProblem), i32,
                                                    C.POINTER(OsgInertialResult)]
    lib.osg_inertial_check.argtypes = [C.POINTER(OsgInertialProblem)]
    lib.osg_local_inertial_ba.argtypes = [vp, C.POINTER(OsgLocalInertialBaProblem),
                                          C.POINTER(OsgLocalInertialBaResult)]
    lib.osg_local_inertial_ba_batch.argtypes = [vp, C.POINTER(OsgLocalInertialBaProblem), i32,
                                                C.POINTER(OsgLocalInertialBaResult)]
    lib.osg_local_inertial_ba_check.argtypes = [C.POINTER(OsgLocalInertialBaProblem)]
    lib.osg_imu_preintegrate.argtypes = [vp, C.POINTER(OsgImuProblem), C.POINTER(OsgImuPreintegrated)]
    lib.osg_imu_preintegrate_batch.argtypes = [vp, C.POINTER(OsgImuProblem), i32, C.POINTER(OsgImuPreintegrated)]
    lib.osg_imu_preintegrate_check.argtypes = [C.POINTER(OsgImuProblem)]
    lib.osg_imu_select.argtypes = [vp, i32, C.c_double, C.c_double, C.c_double, vp, vp]
    lib.osg_imu_integrables.argtypes = [vp, vp, vp, i32, C.c_double, C.c_double, vp]
    lib.osg_imu_delta.argtypes = [C.POINTER(OsgImuPreintegrated), vp, vp, vp, vp]
    lib.osg_imu_delta.restype = None
    lib.osg_imu_predict_state.argtypes = [C.POINTER(OsgImuPreintegrated), vp, vp, vp, vp, vp, vp, vp]
    lib.osg_imu_predict_state.restype = None
    lib.osg_optimize_sim3.argtypes = [vp, C.POINTER(OsgSim3Problem), C.POINTER(OsgSim3Result)]
    lib.osg_optimize_sim3_batch.argtypes = [vp, C.POINTER(OsgSim3Problem), i32, C.POINTER(OsgSim3Result)]
    lib.osg_sim3_ransac.argtypes = [vp, C.POINTER(OsgSim3RansacProblem), C.POINTER(OsgSim3RansacResult)]
    lib.osg_sim3_ransac_batch.argtypes = [vp, C.POINTER(OsgSim3RansacProblem), i32, C.POINTER(OsgSim3RansacResult)]
    lib.osg_sim3_ransac_iterations.argtypes = [C.c_double, i32, i32, i32]
    lib.osg_mlpnp_ransac.argtypes = [vp, C.POINTER(OsgMlpnpProblem), C.POINTER(OsgMlpnpResult)]
    lib.osg_mlpnp_ransac_batch.argtypes = [vp, C.POINTER(OsgMlpnpProblem), i32, C.POINTER(OsgMlpnpResult)]
    lib.osg_mlpnp_ransac_parameters.argtypes = [C.c_double, i32, i32, i32, C.c_float, i32, C.POINTER(i32), C.POINTER(i32)]
    lib.osg_mlpnp_ransac_parameters.restype = None
    lib.osg_mlpnp_check_samples.argtypes = [C.POINTER(OsgMlpnpProblem)]
    lib.osg_two_view_reconstruct.argtypes = [vp, C.POINTER(OsgTwoViewProblem), C.POINTER(OsgTwoViewResult)]
    lib.osg_two_view_reconstruct_batch.argtypes = [vp, C.POINTER(OsgTwoViewProblem), i32, C.POINTER(OsgTwoViewResult)]
    lib.osg_two_view_kernel_times.argtypes = [vp, i32, vp]
    lib.osg_sim3_ransac_iterations.restype = i32
    lib.osg_optimize_essential_graph.argtypes = [vp, C.POINTER(OsgEssGraphProblem), C.POINTER(OsgEssGraphResult)]
    lib.osg_essgraph_correct_points.argtypes = [vp, i32, vp, vp, i32, vp, vp, vp]
    lib.osg_essgraph_kernel_times.argtypes = [vp, i32, vp]
    lib.osg_optimize_essential_graph_4dof.argtypes = [vp, C.POINTER(OsgEssGraph4Problem), C.POINTER(OsgEssGraph4Result)]
    lib.osg_essgraph4_check.argtypes = [C.POINTER(OsgEssGraph4Problem), C.POINTER(OsgEssGraph4Result)]
    lib.osg_local_bundle_adjustment.argtypes = [vp, C.POINTER(OsgBaGraph), C.POINTER(OsgBaResult),
                                                vp]
    lib.osg_bundle_adjustment.argtypes = [vp, C.POINTER(OsgBaGraph), C.POINTER(OsgBaResult),
                                                vp]
    lib.osg_local_bundle_adjustment_batch.argtypes = [vp, vp, i32, vp, vp]
    lib.osg_lba_kernel_times.argtypes = [vp, i32, vp, vp]
    lib.osg_vocabulary_create.argtypes = [vp, C.POINTER(OsgVocabularyDesc), C.POINTER(vp)]
    lib.osg_vocabulary_load_text.argtypes = [vp, C.c_char_p, C.POINTER(vp)]
    lib.osg_vocabulary_destroy.argtypes = [vp]
    lib.osg_vocabulary_info.argtypes = [vp, vp]
    lib.osg_vocabulary_transform.argtypes = [vp, vp, vp, i32, i32, C.POINTER(OsgBowOut)]
    lib.osg_vocabulary_transform_batch.argtypes = [vp, vp, vp, vp, i32, i32, vp]
    lib.osg_kfdb_create.argtypes = [vp, vp, C.POINTER(vp)]
    lib.osg_kfdb_destroy.argtypes = [vp]
    lib.osg_kfdb_size.argtypes = [vp, vp]
    lib.osg_kfdb_add.argtypes = [vp, vp, i32, vp, vp, i32, C.POINTER(OsgKfdbState), C.POINTER(i32)]
    lib.osg_kfdb_erase.argtypes = [vp, vp, i32]
    lib.osg_kfdb_clear.argtypes = [vp, vp]
    lib.osg_kfdb_clear_map.argtypes = [vp, vp, i32]
    lib.osg_kfdb_state_get.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp]
    lib.osg_kfdb_state_set.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp]
    lib.osg_kfdb_query.argtypes = [vp, vp, i32, C.c_int64, i32, vp, vp, i32, vp, C.POINTER(OsgKfdbQueryOut)]
    lib.osg_kfdb_select_nbest.argtypes = [i32, vp, vp, vp, C.c_int64, i32, i32, vp, vp, vp, vp]
    lib.osg_kfdb_select_reloc.argtypes = [i32, vp, vp, vp, C.c_int64, i32, vp, vp]
    lib.osg_fuse_search.argtypes = [vp, C.POINTER(OsgFrame), C.POINTER(OsgFuseQueries), f32, C.c_int, C.c_int,
                                    vp, vp]
    lib.osg_fuse_search_batch.argtypes = [vp, vp, vp, i32, f32, C.c_int, C.c_int, vp, vp, vp]
    lib.osg_search_for_triangulation.argtypes = [vp, C.POINTER(OsgKfSide), C.POINTER(OsgKfSide),
                                                 C.POINTER(OsgTriangGeom), C.c_int, C.c_int, C.c_int, vp]
    lib.osg_search_by_sim3.argtypes = [vp, C.POINTER(OsgFrame), C.POINTER(OsgFrame), C.POINTER(OsgFuseQueries),
                                       C.POINTER(OsgFuseQueries), f32, vp]
    lib.osg_search_by_projection_sim3.argtypes = [vp, C.POINTER(OsgFrame), C.POINTER(OsgFuseQueries), f32, f32, vp]
    lib.osg_search_by_projection_sim3_batch.argtypes = [vp, vp, vp, i32, f32, f32, vp, vp]
    lib.osg_search_for_initialization.argtypes = [vp, C.POINTER(OsgFrame), C.POINTER(OsgFrame), vp, C.c_int, f32,
                                                  C.c_int, vp]
    lib.osg_search_for_initialization_batch.argtypes = [vp, vp, vp, i32, vp, C.c_int, f32, C.c_int, vp, vp]
    lib.osg_compute_stereo_matches.argtypes = [vp, C.POINTER(OsgStereoFrame), vp, vp]
    lib.osg_compute_stereo_matches_batch.argtypes = [vp, vp, i32, vp, vp, vp]
    lib.osg_compute_stereo_fisheye_matches.argtypes = [vp, i32, i32, vp, vp, vp, i32, i32, vp, vp, vp, vp, i32,
                                                       vp, vp, vp, vp, vp, vp, vp, vp]
    lib.osg_debug_distribute_oct_tree.argtypes = [vp, i32, i32, i32, i32, i32, i32, vp, i32]
    lib.osg_orb_detect.argtypes = [vp, C.POINTER(OsgImagePyramid), i32, i32, vp, vp, i32, vp, vp, vp, vp, vp]
    lib.osg_orb_pyramid_layout.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp]
    lib.osg_orb_pyramid_layout.restype = C.c_int64
    lib.osg_orb_pyramid.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp, C.c_int64, i32]
    lib.osg_debug_gaussian_kernel7.argtypes = [vp]
    lib.osg_debug_gaussian_kernel7.restype = None
    lib.osg_orb_describe.argtypes = [vp, C.POINTER(OsgImagePyramid), C.POINTER(OsgImagePyramid),
                                     C.POINTER(OsgOrbKeypoints), vp, vp, i32, vp, vp]
    lib.osg_orb_extract_batch.argtypes = [vp, vp, C.c_int64, i32, i32, i32, i32, C.POINTER(OsgOrbExtractParams), i32,
                                          vp, vp, vp, vp, vp, vp, vp, vp]
    lib.osg_compute_distinctive_descriptors.argtypes = [vp, vp, vp, i32, vp]
    lib.osg_compute_distinctive_descriptors_dev.argtypes = [vp, vp, vp, i32, vp]
    lib.osg_search_for_triangulation_batch.argtypes = [vp, vp, vp, vp, i32, C.c_int, C.c_int, C.c_int, vp, vp]
    lib.osg_create_new_map_points.argtypes = [vp, C.POINTER(OsgNewPointsProblem), C.POINTER(OsgNewPointsResult)]
    lib.osg_create_new_map_points_batch.argtypes = [vp, vp, vp, i32]
    lib.osg_create_new_map_points_check.argtypes = [C.POINTER(OsgNewPointsProblem)]
    lib.osg_frustum.argtypes = [vp, C.POINTER(OsgFrustumFrame), C.POINTER(OsgFrustumPoints), f32,
                                C.POINTER(OsgFrustumResult)]
    lib.osg_frustum_batch.argtypes = [vp, vp, vp, i32, f32, vp]
    lib.osg_frustum_check.argtypes = [C.POINTER(OsgFrustumFrame), C.POINTER(OsgFrustumPoints)]
    lib.osg_search_local_points.argtypes = [vp, C.POINTER(OsgFrame), C.POINTER(OsgFrustumFrame),
                                            C.POINTER(OsgLocalPoints), f32, f32, f32, C.c_int, f32, vp, vp,
                                            C.POINTER(OsgFrustumResult)]
    lib.osg_search_local_points_batch.argtypes = [vp, vp, vp, vp, i32, f32, f32, f32, C.c_int, f32, vp, vp, vp, vp]
    return lib
