"""ctypes mirror of include/vilfusion.h (POD structs only; no torch types).

The same structs are fed to the HIP library (libvilfusion_hip.so) and — in tests only — to the CPU oracle
(liboracle_vilf.so), so both see byte-identical inputs.
"""
import ctypes as C
import numpy as np

VILF_MAX_FRAMES = 11
VILF_MAX_FEATURES = 1000
VILF_PRIOR_MAX_DIM = 160
VILF_PRIOR_MAX_BLOCKS = 24

VILF_OK = 0
VILF_ERR_INVALID_ARGUMENT = -1
VILF_ERR_DEVICE = -2
VILF_ERR_UNSUPPORTED = -3
VILF_ERR_NO_GPU = -4

MARGIN_OLD = 0
MARGIN_SECOND_NEW = 1

TERM_NAMES = {0: "NO_CONVERGENCE", 1: "CONVERGENCE_FUNCTION", 2: "CONVERGENCE_PARAMETER", 3: "CONVERGENCE_GRADIENT", 4: "FAILURE"}

c_double_p = C.POINTER(C.c_double)
c_long_p = C.POINTER(C.c_long)      # vilf_icp_global_map*: point counts of a map are long


class Options(C.Structure):
    _fields_ = [
        ("window_size", C.c_int), ("max_num_iterations", C.c_int), ("max_solver_time", C.c_double),
        ("focal_length", C.c_double), ("cauchy_a", C.c_double), ("G", C.c_double * 3),
        ("estimate_extrinsic", C.c_int), ("estimate_td", C.c_int), ("use_lidar_const", C.c_int),
        ("RIC", C.c_double * 9), ("TIC", C.c_double * 3), ("RCL", C.c_double * 9), ("TCL", C.c_double * 3),
        ("TR", C.c_double), ("ROW", C.c_double), ("init_depth", C.c_double),
        ("edge_leaf_size", C.c_double), ("surf_leaf_size", C.c_double), ("huber_a", C.c_double),
        ("s2m_outer_iterations", C.c_int), ("s2m_max_iterations", C.c_int), ("s2m_crop_half", C.c_double),
    ]


class ImuPreint(C.Structure):
    _fields_ = [
        ("sum_dt", C.c_double), ("delta_p", C.c_double * 3), ("delta_q", C.c_double * 4), ("delta_v", C.c_double * 3),
        ("linearized_ba", C.c_double * 3), ("linearized_bg", C.c_double * 3),
        ("jacobian", C.c_double * 225), ("covariance", C.c_double * 225),
    ]


IMU_DOUBLES = 1 + 3 + 4 + 3 + 3 + 3 + 225 + 225  # 467
assert C.sizeof(ImuPreint) == 8 * IMU_DOUBLES
# numpy view of ImuPreint: a row of 467 doubles
IMU_OFF = {"sum_dt": (0, 1), "delta_p": (1, 4), "delta_q": (4, 8), "delta_v": (8, 11), "linearized_ba": (11, 14),
           "linearized_bg": (14, 17), "jacobian": (17, 242), "covariance": (242, 467)}


class LidarConstraint(C.Structure):
    _fields_ = [("q", C.c_double * 4), ("t", C.c_double * 3)]


class WindowIn(C.Structure):
    _fields_ = [
        ("n_frames", C.c_int), ("para_pose", c_double_p), ("para_speed_bias", c_double_p),
        ("para_ex_pose", C.c_double * 7), ("para_td", C.c_double),
        ("n_features", C.c_int), ("para_feature", c_double_p), ("feature_const", C.POINTER(C.c_uint8)),
        ("feature_start_frame", C.POINTER(C.c_int32)), ("feature_obs_offset", C.POINTER(C.c_int32)),
        ("n_obs", C.c_int), ("obs_point", c_double_p), ("obs_velocity", c_double_p), ("obs_cur_td", c_double_p),
        ("obs_row", c_double_p), ("imu", C.POINTER(ImuPreint)), ("lidar", C.POINTER(LidarConstraint)),
        ("marginalization_flag", C.c_int), ("gauge_R0", c_double_p), ("gauge_P0", c_double_p),
    ]


class Summary(C.Structure):
    _fields_ = [
        ("num_iterations", C.c_int), ("num_successful_steps", C.c_int), ("num_linear_solves", C.c_int),
        ("termination", C.c_int), ("initial_cost", C.c_double), ("final_cost", C.c_double),
        ("final_radius", C.c_double), ("usec_solve", C.c_double),
    ]


class WindowOut(C.Structure):
    _fields_ = [
        ("para_pose", c_double_p), ("para_speed_bias", c_double_p), ("para_feature", c_double_p),
        ("Ps", c_double_p), ("Rs", c_double_p), ("Vs", c_double_p), ("Bas", c_double_p), ("Bgs", c_double_p),
        ("tic", C.c_double * 3), ("ric", C.c_double * 9), ("td", C.c_double), ("summary", Summary),
    ]


class Prior(C.Structure):
    _fields_ = [
        ("valid", C.c_int), ("n", C.c_int), ("m", C.c_int), ("n_blocks", C.c_int),
        ("block_id", C.c_int * VILF_PRIOR_MAX_BLOCKS), ("block_size", C.c_int * VILF_PRIOR_MAX_BLOCKS),
        ("block_idx", C.c_int * VILF_PRIOR_MAX_BLOCKS), ("block_x0", (C.c_double * 9) * VILF_PRIOR_MAX_BLOCKS),
        ("linearized_residuals", C.c_double * VILF_PRIOR_MAX_DIM),
        ("linearized_jacobians", C.c_double * (VILF_PRIOR_MAX_DIM * VILF_PRIOR_MAX_DIM)),
    ]


class PgEdge(C.Structure):
    _fields_ = [("i", C.c_int), ("j", C.c_int), ("q", C.c_double * 4), ("t", C.c_double * 3), ("sigma", C.c_double * 6), ("robust", C.c_int), ("pad_", C.c_int)]


class ImuNoise(C.Structure):
    _fields_ = [("acc_n", C.c_double), ("gyr_n", C.c_double), ("acc_w", C.c_double), ("gyr_w", C.c_double)]


class Scan2MapResult(C.Structure):
    _fields_ = [
        ("pose_qt", C.c_double * 7), ("rel_q", C.c_double * 4), ("rel_t", C.c_double * 3),
        ("n_edge_ds", C.c_int), ("n_surf_ds", C.c_int), ("n_edge_factors", C.c_int * 2), ("n_surf_factors", C.c_int * 2),
        ("iterations", C.c_int * 2), ("final_cost", C.c_double * 2), ("map_edge_size", C.c_int), ("map_surf_size", C.c_int),
    ]


class ScParams(C.Structure):
    """vilf_sc_params: SCManager's constants (Scancontext.h:304-327)"""
    _fields_ = [
        ("num_rings", C.c_int), ("num_sectors", C.c_int), ("max_radius", C.c_double), ("lidar_height", C.c_double),
        ("num_exclude_recent", C.c_int), ("num_candidates", C.c_int), ("search_ratio", C.c_double), ("dist_thres", C.c_double),
        ("tree_making_period", C.c_int), ("pad_", C.c_int),
    ]


class ScResult(C.Structure):
    """vilf_sc_result: what detectLoopClosureID returns and what it only prints"""
    _fields_ = [
        ("loop_id", C.c_int), ("nearest", C.c_int), ("shift", C.c_int), ("n_candidates", C.c_int), ("min_dist", C.c_double),
        ("yaw_diff_rad", C.c_float), ("candidates", C.c_int * 16),
    ]


class IcpParams(C.Structure):
    """vilf_icp_params: the constants of icpCalculation (poseGraphOptimization.cpp:394-414, :646-647) and of DefaultConvergenceCriteria"""
    _fields_ = [
        ("max_correspondence_distance", C.c_double), ("max_iterations", C.c_int), ("history_keyframes", C.c_int), ("transformation_epsilon", C.c_double),
        ("euclidean_fitness_epsilon", C.c_double), ("rotation_threshold", C.c_double), ("mse_relative", C.c_double), ("fitness_threshold", C.c_double),
        ("leaf_size", C.c_double), ("own_pose", C.c_int), ("pad_", C.c_int),
    ]


class IcpResult(C.Structure):
    """vilf_icp_result"""
    _fields_ = [
        ("converged", C.c_int), ("accepted", C.c_int), ("criterion", C.c_int), ("iterations", C.c_int),
        ("n_source", C.c_int), ("n_target", C.c_int), ("n_correspondences", C.c_int), ("pad_", C.c_int),
        ("fitness", C.c_double), ("final_mse", C.c_double), ("transform", C.c_float * 16), ("pose6", C.c_double * 6), ("pose_qt", C.c_double * 7),
    ]


class IcpIter(C.Structure):
    """vilf_icp_iter: one round"""
    _fields_ = [("n_correspondences", C.c_int), ("criterion", C.c_int), ("mse", C.c_double), ("cos_angle", C.c_double), ("translation_sqr", C.c_double)]


class TrackParams(C.Structure):
    """vilf_track_params: COL, ROW, MAX_CNT, MIN_DIST and the pinhole camera of the feature tracker"""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("max_cnt", C.c_int), ("min_dist", C.c_int),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("k1", C.c_double), ("k2", C.c_double), ("p1", C.c_double), ("p2", C.c_double)]


class TrackFrontend(C.Structure):
    """vilf_track_frontend: the two optional steps of readImage, CLAHE (EQUALIZE) and rejectWithF (F_THRESHOLD, FOCAL_LENGTH)"""
    _fields_ = [("equalize", C.c_int), ("clahe_clip", C.c_double), ("clahe_tiles_x", C.c_int), ("clahe_tiles_y", C.c_int),
                ("reject_f", C.c_int), ("f_threshold", C.c_double), ("focal_length", C.c_double), ("n_hypotheses", C.c_int), ("seed", C.c_uint)]


VILF_TRACK_MAX_TILES = 1024
VILF_TRACK_MAX_HYPOTHESES = 2048


class TrackMaskParams(C.Structure):
    """vilf_track_mask_params: readImage_mask's erosion radius, probe distance and rejectWithF_mask (on / off, the search's and the final test's thresholds)"""
    _fields_ = [("erode_radius", C.c_int), ("probe", C.c_int), ("reject", C.c_int), ("f_threshold", C.c_double), ("epi_threshold", C.c_double)]


VILF_TRACK_MAX_ERODE = 16


class StartupParams(C.Structure):
    """vilf_startup_params: K and seed of the search, the gates of relativePose / solveRelativeRT, the RANSAC threshold, FOCAL_LENGTH, recoverPose's distance"""
    _fields_ = [("n_hypotheses", C.c_int), ("seed", C.c_uint), ("min_count", C.c_int), ("min_solve_count", C.c_int), ("min_inliers", C.c_int), ("pad_", C.c_int),
                ("ransac_threshold", C.c_double), ("focal_length", C.c_double), ("min_parallax", C.c_double), ("distance_threshold", C.c_double)]


class StartupWindow(C.Structure):
    """vilf_startup_window: the feature table relativePose reads"""
    _fields_ = [("n_frames", C.c_int), ("n_features", C.c_int), ("start_frame", C.POINTER(C.c_int32)), ("first_obs", C.POINTER(C.c_int32)), ("pts", c_double_p)]


class StartupResult(C.Structure):
    """vilf_startup_result: l, relative_R, relative_T"""
    _fields_ = [("l", C.c_int), ("inlier_cnt", C.c_int), ("R", C.c_double * 9), ("T", C.c_double * 3)]


class StartupPair(C.Structure):
    """vilf_startup_pair: one row of the table of pairs (i, newest)"""
    _fields_ = [("count", C.c_int), ("flags", C.c_int), ("best_k", C.c_int), ("score", C.c_int), ("cheirality", C.c_int * 4), ("chosen", C.c_int),
                ("inlier_cnt", C.c_int), ("parallax", C.c_double), ("F", C.c_double * 9), ("R", C.c_double * 9), ("T", C.c_double * 3)]


VILF_SU_COUNT, VILF_SU_PARALLAX, VILF_SU_SOLVE_COUNT, VILF_SU_HYPOTHESIS, VILF_SU_FINITE, VILF_SU_INLIERS, VILF_SU_PASS = 1, 2, 4, 8, 16, 32, 63
VILF_STARTUP_MAX_WINDOWS = 256
# the C name of every mirror of the start-up, for the layout check (tests/test_startup_relative_pose.py compiles the header as tests/test_abi.py does)
STARTUP_LAYOUTS = {"vilf_startup_params": StartupParams, "vilf_startup_window": StartupWindow, "vilf_startup_result": StartupResult,
                   "vilf_startup_pair": StartupPair}


class StartupSfmParams(C.Structure):
    """vilf_startup_sfm_params: the count gates of solveFrameByPnP, the iterations and the first damping of its Levenberg-Marquardt"""
    _fields_ = [("min_pnp_count", C.c_int), ("warn_pnp_count", C.c_int), ("pnp_iterations", C.c_int), ("pad_", C.c_int), ("lambda0", C.c_double)]


class StartupFrame(C.Structure):
    """vilf_startup_frame: a frame of GlobalSFM's chain, or a problem of vilf_startup_pnp"""
    _fields_ = [("count", C.c_int), ("flags", C.c_int), ("accepted", C.c_int), ("pad_", C.c_int), ("cost0", C.c_double), ("cost1", C.c_double),
                ("R", C.c_double * 9), ("t", C.c_double * 3), ("Q", C.c_double * 9), ("T", C.c_double * 3)]


class StartupStructure(C.Structure):
    """vilf_startup_structure: a window's result of vilf_startup_sfm"""
    _fields_ = [("ok", C.c_int), ("fail_frame", C.c_int), ("n_triangulated", C.c_int), ("l", C.c_int)]


class StartupPnpProblem(C.Structure):
    """vilf_startup_pnp_problem: the points in member order, the per-problem minimum count and the guess"""
    _fields_ = [("n", C.c_int), ("min_count", C.c_int), ("pts3", c_double_p), ("pts2", c_double_p), ("R", C.c_double * 9), ("t", C.c_double * 3)]


VILF_SFM_FIXED, VILF_SFM_PNP, VILF_SFM_FEW, VILF_SFM_FAIL_COUNT, VILF_SFM_FAIL_FINITE, VILF_SFM_POSE = 1, 2, 4, 8, 16, 32
VILF_STARTUP_MAX_PROBLEMS = 4096
# the mirrors of the second stage, for the layout check of tests/test_startup_sfm.py
STARTUP_SFM_LAYOUTS = {"vilf_startup_sfm_params": StartupSfmParams, "vilf_startup_frame": StartupFrame, "vilf_startup_structure": StartupStructure,
                       "vilf_startup_pnp_problem": StartupPnpProblem}


class StartupBaParams(C.Structure):
    """vilf_startup_ba_params: the iterations and the first damping of the BA's Levenberg-Marquardt, the function tolerance that ends it, the verdict's cost"""
    _fields_ = [("ba_iterations", C.c_int), ("pad_", C.c_int), ("lambda0", C.c_double), ("function_tolerance", C.c_double), ("cost_threshold", C.c_double)]


class StartupBaStart(C.Structure):
    """vilf_startup_ba_start: l, whether the chain succeeded, the poses and the structure the BA starts from"""
    _fields_ = [("l", C.c_int), ("chain_ok", C.c_int), ("R", c_double_p), ("t", c_double_p), ("state", C.POINTER(C.c_uint8)), ("positions", c_double_p)]


class StartupBaResult(C.Structure):
    """vilf_startup_ba_result: a window's result of vilf_startup_ba / vilf_startup_construct"""
    _fields_ = [("ok", C.c_int), ("flags", C.c_int), ("iterations", C.c_int), ("accepted", C.c_int), ("n_camera", C.c_int), ("n_members", C.c_int),
                ("n_residuals", C.c_int), ("l", C.c_int), ("cost0", C.c_double), ("cost1", C.c_double), ("lambda_", C.c_double)]


class StartupBaFrame(C.Structure):
    """vilf_startup_ba_frame: a frame's pose after the BA, in both conventions"""
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("Q", C.c_double * 9), ("T", C.c_double * 3)]


VILF_BA_CONVERGED, VILF_BA_COST, VILF_BA_FINITE = 1, 2, 4
# the mirrors of the third stage and the C names of their fields where they differ (lambda is a Python keyword), for the layout check of tests/test_startup_ba.py
STARTUP_BA_LAYOUTS = {"vilf_startup_ba_params": StartupBaParams, "vilf_startup_ba_start": StartupBaStart, "vilf_startup_ba_result": StartupBaResult,
                      "vilf_startup_ba_frame": StartupBaFrame}
STARTUP_BA_C_NAMES = {"lambda_": "lambda"}


class TriWindow(C.Structure):
    """vilf_tri_window: the poses, the extrinsics and the whole feature list FeatureManager::triangulate reads, and where its outputs go"""
    _fields_ = [("n_frames", C.c_int), ("n_features", C.c_int), ("Ps", c_double_p), ("Rs", c_double_p), ("tic", C.c_double * 3), ("ric", C.c_double * 9),
                ("start_frame", C.POINTER(C.c_int32)), ("first_obs", C.POINTER(C.c_int32)), ("points", c_double_p), ("depth_in", c_double_p),
                ("depth_out", c_double_p), ("inv_depth_out", c_double_p), ("flags_out", C.POINTER(C.c_uint8)), ("sweeps_out", C.POINTER(C.c_uint8))]


class TriResult(C.Structure):
    """vilf_tri_result: a window's counts"""
    _fields_ = [("n_used", C.c_int), ("n_candidates", C.c_int), ("n_reset", C.c_int), ("n_nonfinite", C.c_int)]


VILF_TRI_USED, VILF_TRI_DONE, VILF_TRI_RESET, VILF_TRI_NONFINITE = 1, 2, 4, 8
VILF_TRI_MAX_WINDOWS = 4096
# the mirrors of the feature triangulation, for the layout check of tests/test_feature_triangulate.py
TRI_LAYOUTS = {"vilf_tri_window": TriWindow, "vilf_tri_result": TriResult}


class ExrotParams(C.Structure):
    """vilf_exrot_params: K and seed of the search, the gates of solveRelativeR and CalibrationExRotation, the RANSAC threshold, the Huber angle, the sigma gate"""
    _fields_ = [("n_hypotheses", C.c_int), ("seed", C.c_uint), ("min_corres", C.c_int), ("min_frames", C.c_int),
                ("ransac_threshold", C.c_double), ("huber_deg", C.c_double), ("min_sigma", C.c_double)]


class ExrotPair(C.Structure):
    """vilf_exrot_pair: a slot's correspondences of the last two frames and the pre-integrated rotation between them; n = -1 skips the slot"""
    _fields_ = [("n", C.c_int), ("pad_", C.c_int), ("a", c_double_p), ("b", c_double_p), ("delta_q", C.c_double * 4)]


class ExrotResult(C.Structure):
    """vilf_exrot_result: a slot's row of one push"""
    _fields_ = [("frame_count", C.c_int), ("flags", C.c_int), ("count", C.c_int), ("best_k", C.c_int), ("score", C.c_int), ("front", C.c_int * 4),
                ("chosen", C.c_int), ("ok", C.c_int), ("pad_", C.c_int), ("Rc", C.c_double * 9), ("angle", C.c_double), ("weight", C.c_double),
                ("sigma", C.c_double * 4), ("x", C.c_double * 4), ("ric", C.c_double * 9)]


VILF_EXROT_COUNT, VILF_EXROT_HYPOTHESIS, VILF_EXROT_FINITE, VILF_EXROT_SOLVED, VILF_EXROT_SKIPPED = 1, 2, 4, 7, 8
VILF_EXROT_MAX_SLOTS, VILF_EXROT_MAX_HISTORY = 256, 256
# the mirrors of the camera-IMU rotation calibration, for the layout check of tests/test_exrot_reference.py
EXROT_LAYOUTS = {"vilf_exrot_params": ExrotParams, "vilf_exrot_pair": ExrotPair, "vilf_exrot_result": ExrotResult}

VILF_KF_BITS, VILF_KF_WORDS, VILF_KF_MAX_OFFSET, VILF_KF_MATCH_CHUNK, VILF_KF_MAX_CANDIDATES = 256, 4, 64, 256, 256


class KfParams(C.Structure):
    """vilf_kf_params: the image size, FAST and match thresholds, the pinhole camera and the BRIEF pattern of the key-frame store"""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("fast_threshold", C.c_int), ("match_max_dist", C.c_int), ("match_accept_dist", C.c_int), ("pad_", C.c_int),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("k1", C.c_double), ("k2", C.c_double), ("p1", C.c_double), ("p2", C.c_double),
                ("x1", C.c_int * VILF_KF_BITS), ("y1", C.c_int * VILF_KF_BITS), ("x2", C.c_int * VILF_KF_BITS), ("y2", C.c_int * VILF_KF_BITS)]


# the mirror of the key-frame store, for the layout check of tests/test_keyframe_reference.py
KF_LAYOUTS = {"vilf_kf_params": KfParams}

VILF_KFL_GATE, VILF_KFL_NO_HYPOTHESIS, VILF_KFL_REFIT, VILF_KFL_REFIT_DROPPED, VILF_KFL_LOOP = 1, 2, 4, 8, 16


class KfLoopParams(C.Structure):
    """vilf_kf_loop_params: the PnP-RANSAC search, the loop gates and the camera-IMU extrinsic of a vilf_kf_find_connection"""
    _fields_ = [("n_hypotheses", C.c_int), ("seed", C.c_uint), ("hyp_iterations", C.c_int), ("refine_iterations", C.c_int), ("min_loop_num", C.c_int), ("pad_", C.c_int),
                ("lambda0", C.c_double), ("reproj_threshold", C.c_double), ("max_yaw", C.c_double), ("max_dist", C.c_double),
                ("qic", C.c_double * 9), ("tic", C.c_double * 3)]


class KfLoopResult(C.Structure):
    """vilf_kf_loop_result: one old key frame's row of a vilf_kf_find_connection"""
    _fields_ = [("n_matched", C.c_int), ("n_inliers", C.c_int), ("best_k", C.c_int), ("flags", C.c_int), ("has_loop", C.c_int), ("accepted", C.c_int),
                ("R", C.c_double * 9), ("t", C.c_double * 3), ("PnP_R_old", C.c_double * 9), ("PnP_T_old", C.c_double * 3),
                ("relative_t", C.c_double * 3), ("relative_q", C.c_double * 4), ("relative_yaw", C.c_double), ("cost0", C.c_double), ("cost1", C.c_double)]


# the mirrors of the second stage, for the layout check of tests/test_keyframe_loop_reference.py
KFL_LAYOUTS = {"vilf_kf_loop_params": KfLoopParams, "vilf_kf_loop_result": KfLoopResult}

VILF_BOW_MAX_DEPTH, VILF_BOW_MAX_RESULTS, VILF_BOW_LDS_WORDS = 16, 16, 2048
VILF_BOW_L1_NORM = 0
VILF_BOW_TF_IDF, VILF_BOW_TF, VILF_BOW_IDF, VILF_BOW_BINARY = 0, 1, 2, 3


class BowNode(C.Structure):
    """vilf_bow_node: VINSLoop::Node, a record of the vocabulary file"""
    _fields_ = [("nodeId", C.c_int), ("parentId", C.c_int), ("weight", C.c_double), ("descriptor", C.c_uint64 * 4)]


class BowWord(C.Structure):
    """vilf_bow_word: VINSLoop::Word"""
    _fields_ = [("nodeId", C.c_int), ("wordId", C.c_int)]


class BowVocabulary(C.Structure):
    """vilf_bow_vocabulary: the header of the vocabulary file and pointers to its two record arrays"""
    _fields_ = [("k", C.c_int), ("L", C.c_int), ("scoringType", C.c_int), ("weightingType", C.c_int), ("nNodes", C.c_int), ("nWords", C.c_int),
                ("nodes", C.POINTER(BowNode)), ("words", C.POINTER(BowWord))]


class BowParams(C.Structure):
    """vilf_bow_params: the constants of detectLoop (pose_graph.cpp:322, :351, :355, :376)"""
    _fields_ = [("max_results", C.c_int), ("min_gap", C.c_int), ("neighbour_score", C.c_double), ("loop_score", C.c_double)]


class BowResult(C.Structure):
    """vilf_bow_result: detectLoop's return value and the query results it was taken from"""
    _fields_ = [("loop_index", C.c_int), ("find_loop", C.c_int), ("n_results", C.c_int), ("n_words", C.c_int),
                ("id", C.c_int * VILF_BOW_MAX_RESULTS), ("score", C.c_double * VILF_BOW_MAX_RESULTS)]


# the mirrors of candidate retrieval, for the layout check of tests/test_bow_reference.py
BOW_LAYOUTS = {"vilf_bow_node": BowNode, "vilf_bow_word": BowWord, "vilf_bow_vocabulary": BowVocabulary, "vilf_bow_params": BowParams, "vilf_bow_result": BowResult}
# the records of the VINS binary vocabulary file (ThirdParty/VocabularyBinary.hpp) as numpy sees them; BowNode and BowWord have the same layouts
BOW_NODE_DTYPE = np.dtype([("nodeId", "<i4"), ("parentId", "<i4"), ("weight", "<f8"), ("descriptor", "<u8", (4,))])
BOW_WORD_DTYPE = np.dtype([("nodeId", "<i4"), ("wordId", "<i4")])

VILF_PG4_BAND = 4
VILF_PG4_MAX_ITERATIONS, VILF_PG4_FUNCTION, VILF_PG4_GRADIENT, VILF_PG4_PARAMETER, VILF_PG4_RADIUS, VILF_PG4_FINITE = 1, 2, 4, 8, 16, 32


class Pg4Params(C.Structure):
    """vilf_pg4_params: the Levenberg-Marquardt rule, the Huber width and the loops' yaw scale of a vilf_pg4_optimize"""
    _fields_ = [("max_iterations", C.c_int), ("pad_", C.c_int), ("initial_radius", C.c_double), ("max_radius", C.c_double), ("min_radius", C.c_double),
                ("min_relative_decrease", C.c_double), ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double), ("parameter_tolerance", C.c_double),
                ("huber", C.c_double), ("loop_yaw_scale", C.c_double)]


class Pg4Loop(C.Structure):
    """vilf_pg4_loop: one verified loop, from the old key frame to the one that found it"""
    _fields_ = [("from_", C.c_int), ("to", C.c_int), ("rel_t", C.c_double * 3), ("rel_yaw", C.c_double)]


class Pg4Result(C.Structure):
    """vilf_pg4_result: how a vilf_pg4_optimize ended, and the drift of its last node"""
    _fields_ = [("iterations", C.c_int), ("accepted", C.c_int), ("pivot_rejections", C.c_int), ("flags", C.c_int), ("cost0", C.c_double), ("cost1", C.c_double),
                ("radius", C.c_double), ("yaw_drift", C.c_double), ("r_drift", C.c_double * 9), ("t_drift", C.c_double * 3)]


def dptr(a):
    """pointer to a C-contiguous float64 numpy array (None -> NULL)."""
    if a is None:
        return c_double_p()
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"], (a.dtype, a.flags)
    return a.ctypes.data_as(c_double_p)


class Window:
    """One sliding-window snapshot ≙ the Estimator members optimization() reads (estimator.h:70-146).

    All arrays are numpy, C-contiguous, in the reference's layouts (see include/vilfusion.h).
    """

    def __init__(self, para_pose, para_speed_bias, para_ex_pose, para_feature, feature_const, feature_start_frame,
                 feature_obs_offset, obs_point, imu, lidar=None, para_td=0.0, marginalization_flag=MARGIN_OLD,
                 obs_velocity=None, obs_cur_td=None, obs_row=None, gauge_R0=None, gauge_P0=None):
        f64 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        self.para_pose = f64(para_pose)
        self.para_speed_bias = f64(para_speed_bias)
        self.para_ex_pose = f64(para_ex_pose)
        self.para_td = float(para_td)
        self.para_feature = f64(para_feature)
        self.feature_const = np.ascontiguousarray(feature_const, dtype=np.uint8)
        self.feature_start_frame = np.ascontiguousarray(feature_start_frame, dtype=np.int32)
        self.feature_obs_offset = np.ascontiguousarray(feature_obs_offset, dtype=np.int32)
        self.obs_point = f64(obs_point)
        self.obs_velocity = f64(obs_velocity)
        self.obs_cur_td = f64(obs_cur_td)
        self.obs_row = f64(obs_row)
        self.imu = f64(imu)          # (n_frames, 467) rows ≙ vilf_imu_preint; row 0 unused
        self.lidar = f64(lidar)      # (n_frames, 7) [qx qy qz qw tx ty tz]; row 0 unused
        self.marginalization_flag = int(marginalization_flag)
        self.gauge_R0 = f64(gauge_R0)
        self.gauge_P0 = f64(gauge_P0)
        self.n_frames = self.para_pose.shape[0]
        assert self.para_pose.shape == (self.n_frames, 7)
        assert self.para_speed_bias.shape == (self.n_frames, 9)
        assert self.imu.shape == (self.n_frames, IMU_DOUBLES)
        assert self.feature_obs_offset.shape[0] == self.n_features + 1
        assert self.obs_point.shape == (self.n_obs, 3)

    @property
    def n_features(self):
        return int(self.para_feature.shape[0])

    @property
    def n_obs(self):
        return int(self.obs_point.shape[0])

    @property
    def n_factors(self):
        return self.n_obs - self.n_features

    def as_struct(self):
        """vilf_window_in pointing into this object's arrays (keep `self` alive while the struct is used)."""
        w = WindowIn()
        w.n_frames = self.n_frames
        w.para_pose = dptr(self.para_pose)
        w.para_speed_bias = dptr(self.para_speed_bias)
        for i in range(7):
            w.para_ex_pose[i] = self.para_ex_pose[i]
        w.para_td = self.para_td
        w.n_features = self.n_features
        w.para_feature = dptr(self.para_feature)
        w.feature_const = self.feature_const.ctypes.data_as(C.POINTER(C.c_uint8))
        w.feature_start_frame = self.feature_start_frame.ctypes.data_as(C.POINTER(C.c_int32))
        w.feature_obs_offset = self.feature_obs_offset.ctypes.data_as(C.POINTER(C.c_int32))
        w.n_obs = self.n_obs
        w.obs_point = dptr(self.obs_point)
        w.obs_velocity = dptr(self.obs_velocity)
        w.obs_cur_td = dptr(self.obs_cur_td)
        w.obs_row = dptr(self.obs_row)
        w.imu = C.cast(self.imu.ctypes.data, C.POINTER(ImuPreint))
        w.lidar = C.cast(self.lidar.ctypes.data, C.POINTER(LidarConstraint)) if self.lidar is not None else C.POINTER(LidarConstraint)()
        w.marginalization_flag = self.marginalization_flag
        w.gauge_R0 = dptr(self.gauge_R0)
        w.gauge_P0 = dptr(self.gauge_P0)
        return w


class WindowResult:
    """Caller-owned output buffers for vilf_window_out."""

    def __init__(self, n_frames, n_features):
        self.para_pose = np.zeros((n_frames, 7))
        self.para_speed_bias = np.zeros((n_frames, 9))
        self.para_feature = np.zeros(max(n_features, 1))[:n_features]
        self.Ps = np.zeros((n_frames, 3))
        self.Rs = np.zeros((n_frames, 3, 3))
        self.Vs = np.zeros((n_frames, 3))
        self.Bas = np.zeros((n_frames, 3))
        self.Bgs = np.zeros((n_frames, 3))
        self._feat_buf = np.zeros(max(n_features, 1))
        self.struct = WindowOut()
        s = self.struct
        s.para_pose = dptr(self.para_pose)
        s.para_speed_bias = dptr(self.para_speed_bias)
        s.para_feature = dptr(self._feat_buf)
        s.Ps, s.Rs, s.Vs, s.Bas, s.Bgs = dptr(self.Ps), dptr(self.Rs), dptr(self.Vs), dptr(self.Bas), dptr(self.Bgs)
        self._nfeat = n_features

    def finish(self):
        self.para_feature = self._feat_buf[:self._nfeat].copy()
        self.tic = np.array(self.struct.tic[:])
        self.ric = np.array(self.struct.ric[:]).reshape(3, 3)
        self.td = self.struct.td
        s = self.struct.summary
        self.summary = dict(num_iterations=s.num_iterations, num_successful_steps=s.num_successful_steps,
                            num_linear_solves=s.num_linear_solves, termination=s.termination,
                            initial_cost=s.initial_cost, final_cost=s.final_cost, final_radius=s.final_radius,
                            usec_solve=s.usec_solve)
        return self


def prior_to_numpy(p):
    """(J0 [n,n], r0 [n], blocks list) from a Prior struct."""
    n = p.n
    J = np.frombuffer(p.linearized_jacobians, dtype=np.float64, count=n * n).reshape(n, n).copy()
    r = np.frombuffer(p.linearized_residuals, dtype=np.float64, count=n).copy()
    blocks = [dict(id=p.block_id[i], size=p.block_size[i], idx=p.block_idx[i], x0=np.array(p.block_x0[i][:p.block_size[i]]))
              for i in range(p.n_blocks)]
    return J, r, blocks


def make_prior(J0, r0, blocks, m=0):
    """Prior struct from numpy parts; blocks = list of dict(id,size,idx,x0)."""
    p = Prior()
    n = J0.shape[0]
    assert J0.shape == (n, n) and n <= VILF_PRIOR_MAX_DIM and len(blocks) <= VILF_PRIOR_MAX_BLOCKS
    p.valid, p.n, p.m, p.n_blocks = 1, n, m, len(blocks)
    flat = np.ascontiguousarray(J0, dtype=np.float64).ravel()
    C.memmove(p.linearized_jacobians, flat.ctypes.data, 8 * n * n)
    rr = np.ascontiguousarray(r0, dtype=np.float64)
    C.memmove(p.linearized_residuals, rr.ctypes.data, 8 * n)
    for i, b in enumerate(blocks):
        p.block_id[i], p.block_size[i], p.block_idx[i] = int(b["id"]), int(b["size"]), int(b["idx"])
        for k in range(b["size"]):
            p.block_x0[i][k] = float(b["x0"][k])
    return p
