"""ctypes loader for libvilfusion_hip.so (the product). Fails loudly: there is no CPU fallback."""
import ctypes as C
import os
import subprocess
from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
SO_PATH = os.environ.get("VILF_SO") or os.path.join(CSRC, "libvilfusion_hip.so")      # VILF_SO: another build of the library (same-box A/B of a kernel change: tools/)
_lib = None

EXPORTED = [
    "vilf_default_options", "vilf_create", "vilf_destroy", "vilf_reset", "vilf_last_error", "vilf_version",
    "vilf_window_solve", "vilf_window_solve_group", "vilf_window_marginalize", "vilf_batch_upload", "vilf_batch_solve", "vilf_batch_rewind",
    "vilf_batch_marginalize", "vilf_batch_download", "vilf_batch_download_states", "vilf_batch_summaries", "vilf_synchronize", "vilf_wait_for", "vilf_set_async_upload", "vilf_set_profiling", "vilf_get_profile",
    "vilf_batch_newest_poses_device", "vilf_prior_export", "vilf_prior_import", "vilf_eval_projection", "vilf_eval_imu", "vilf_eval_imu_raw",
    "vilf_eval_lidar_between", "vilf_eval_projection_td", "vilf_eval_prior", "vilf_eval_edge", "vilf_eval_surf", "vilf_pose_plus", "vilf_se3_plus",
    "vilf_imu_preintegrate", "vilf_imu_preintegrate_batch", "vilf_visual_imu_alignment", "vilf_posegraph_optimize", "vilf_scan2map_init", "vilf_scan2map_step", "vilf_scan2map_get_map", "vilf_scan2map_set_pose",
    "vilf_scan2map_batch_create", "vilf_scan2map_batch_init", "vilf_scan2map_batch_set_scan", "vilf_scan2map_batch_step", "vilf_scan2map_batch_snapshot",
    "vilf_scan2map_batch_rewind", "vilf_scan2map_batch_copy_stream", "vilf_scan2map_batch_results", "vilf_scan2map_batch_get_map", "vilf_get_profile_scan2map", "vilf_get_profile_marginalize", "vilf_batch_marginalize_stats", "vilf_get_profile_large_window", "vilf_lidar_extract_features", "vilf_feature_depth",
    "vilf_comm_unique_id", "vilf_comm_create", "vilf_comm_destroy", "vilf_gather_poses", "vilf_gather_poses_handle", "vilf_comm_ranks", "vilf_get_stream", "vilf_comm_last_error",
    "vilf_sc_default_params", "vilf_sc_create", "vilf_sc_add_keyframe", "vilf_sc_add_keyframes", "vilf_sc_detect", "vilf_sc_detect_range", "vilf_sc_get", "vilf_sc_size", "vilf_get_profile_sc",
    "vilf_icp_default_params", "vilf_icp_create", "vilf_icp_add_cloud", "vilf_icp_add_clouds", "vilf_icp_size", "vilf_icp_submap", "vilf_icp_align", "vilf_icp_align_pairs",
    "vilf_icp_get_history", "vilf_icp_get_search", "vilf_get_profile_icp",
    "vilf_icp_global_map", "vilf_icp_global_map_size", "vilf_icp_global_map_get", "vilf_get_profile_icp_map",
    "vilf_track_init", "vilf_track_reset", "vilf_track_read_image", "vilf_track_get", "vilf_track_pyramid", "vilf_track_lk", "vilf_track_detect", "vilf_track_profile",
    "vilf_track_configure", "vilf_track_clahe", "vilf_track_reject_f", "vilf_track_profile_frontend",
    "vilf_track_configure_mask", "vilf_track_set_fisheye_mask", "vilf_track_read_image_mask", "vilf_track_erode", "vilf_track_probe", "vilf_track_reject_f_mask",
    "vilf_track_detect_masked", "vilf_track_profile_mask",
    "vilf_startup_default_params", "vilf_startup_relative_pose", "vilf_startup_get_correspondences", "vilf_startup_profile",
    "vilf_startup_default_sfm_params", "vilf_startup_sfm", "vilf_startup_get_structure", "vilf_startup_pnp", "vilf_startup_sfm_profile",
    "vilf_startup_default_ba_params", "vilf_startup_ba", "vilf_startup_construct", "vilf_startup_get_ba_structure", "vilf_startup_ba_profile",
    "vilf_features_triangulate", "vilf_features_profile",
    "vilf_exrot_default_params", "vilf_exrot_reset", "vilf_exrot_push", "vilf_exrot_get_history", "vilf_exrot_profile",
    "vilf_kf_default_params", "vilf_kf_create", "vilf_kf_add_keyframe", "vilf_kf_add_loaded", "vilf_kf_get", "vilf_kf_size", "vilf_kf_match",
    "vilf_kf_blur", "vilf_kf_fast", "vilf_kf_brief", "vilf_kf_profile",
    "vilf_kf_default_loop_params", "vilf_kf_set_geometry", "vilf_kf_find_connection", "vilf_kf_loop_profile",
    "vilf_pg4_default_params", "vilf_pg4_optimize", "vilf_pg4_profile",
    "vilf_kf_bow_default_params", "vilf_kf_bow_set_vocabulary", "vilf_kf_bow_add", "vilf_kf_bow_add_range", "vilf_kf_bow_detect", "vilf_kf_bow_detect_range", "vilf_kf_bow_get",
    "vilf_kf_bow_transform", "vilf_kf_bow_size", "vilf_kf_bow_profile",
]


class VilfError(RuntimeError):
    pass


def build(verbose=False):
    """hipcc --offload-arch=gfx950 build of the HIP library (cross-compiles without a GPU)."""
    subprocess.check_call(["make", "-C", CSRC, "-j4"] + ([] if verbose else ["-s"]))
    res = os.path.join(CSRC, "kernel_resources.json")          # registers / spills / LDS per kernel from the code objects (bench.py quotes the window kernels)
    tool = os.path.join(os.path.dirname(_HERE), "tools", "kernel_resources.py")
    if os.path.exists(tool) and (not os.path.exists(res) or os.path.getmtime(res) < os.path.getmtime(SO_PATH)):
        # generated next to the .so and git-ignored like it (it travels to the GPU box with the snapshot); a failure of the tool is reported, never fatal
        r = subprocess.run(["python3", tool, "__none__"], check=False, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0 or verbose:
            print(f"[vil_fusion_amd.build] tools/kernel_resources.py rc={r.returncode}" + (": " + r.stdout.strip()[-400:] if r.returncode != 0 else ""))
    return SO_PATH


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise VilfError(f"{SO_PATH} is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950). "
                        "There is no CPU fallback for the solve path.")
    L = C.CDLL(SO_PATH)
    vp = C.c_void_p
    dpp = C.POINTER(abi.c_double_p)
    L.vilf_version.restype = C.c_char_p
    L.vilf_last_error.restype = C.c_char_p
    L.vilf_last_error.argtypes = [vp]
    L.vilf_default_options.argtypes = [C.POINTER(abi.Options)]
    L.vilf_default_options.restype = None
    L.vilf_create.argtypes = [C.POINTER(abi.Options), C.c_int, vp, C.POINTER(vp)]
    L.vilf_destroy.argtypes = [vp]
    L.vilf_destroy.restype = None
    L.vilf_reset.argtypes = [vp]
    L.vilf_window_solve.argtypes = [vp, C.POINTER(abi.WindowIn), C.POINTER(abi.WindowOut)]
    L.vilf_window_solve_group.argtypes = [vp, C.c_int, C.POINTER(abi.WindowIn), C.POINTER(abi.WindowOut)]
    L.vilf_window_marginalize.argtypes = [vp]
    L.vilf_batch_upload.argtypes = [vp, C.c_int, C.POINTER(abi.WindowIn)]
    L.vilf_batch_solve.argtypes = [vp, C.c_int]
    L.vilf_batch_rewind.argtypes = [vp]
    L.vilf_batch_marginalize.argtypes = [vp, C.c_int]
    L.vilf_batch_download.argtypes = [vp, C.c_int, C.c_int, C.POINTER(abi.WindowOut)]
    L.vilf_batch_summaries.argtypes = [vp, C.c_int, C.c_int, C.POINTER(abi.Summary)]
    L.vilf_synchronize.argtypes = [vp]
    L.vilf_wait_for.argtypes = [vp, vp]
    L.vilf_set_async_upload.argtypes = [vp, C.c_int]
    L.vilf_set_profiling.argtypes = [vp, C.c_int]
    L.vilf_get_profile.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_long)]
    L.vilf_batch_newest_poses_device.argtypes = [vp, abi.c_double_p, vp]
    L.vilf_prior_export.argtypes = [vp, C.c_int, C.POINTER(abi.Prior)]
    L.vilf_prior_import.argtypes = [vp, C.c_int, C.POINTER(abi.Prior)]
    L.vilf_eval_projection.argtypes = [vp, dpp, abi.c_double_p, abi.c_double_p, abi.c_double_p, dpp]
    L.vilf_eval_imu.argtypes = [vp, dpp, C.POINTER(abi.ImuPreint), abi.c_double_p, dpp]
    L.vilf_eval_imu_raw.argtypes = [vp, dpp, C.POINTER(abi.ImuPreint), abi.c_double_p, dpp, abi.c_double_p]
    L.vilf_eval_lidar_between.argtypes = [vp, dpp, C.POINTER(abi.LidarConstraint), abi.c_double_p, dpp]
    L.vilf_eval_edge.argtypes = [vp, abi.c_double_p, abi.c_double_p, abi.c_double_p, abi.c_double_p, abi.c_double_p, abi.c_double_p]
    L.vilf_eval_surf.argtypes = [vp, abi.c_double_p, abi.c_double_p, abi.c_double_p, C.c_double, abi.c_double_p, abi.c_double_p]
    L.vilf_pose_plus.argtypes = [vp, abi.c_double_p, abi.c_double_p, abi.c_double_p]
    L.vilf_se3_plus.argtypes = [vp, abi.c_double_p, abi.c_double_p, abi.c_double_p]
    L.vilf_imu_preintegrate.argtypes = [C.POINTER(abi.ImuNoise), abi.c_double_p, abi.c_double_p, abi.c_double_p, abi.c_double_p, C.c_int,
                                        abi.c_double_p, abi.c_double_p, abi.c_double_p, C.POINTER(abi.ImuPreint)]
    L.vilf_scan2map_init.argtypes = [vp, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_float), C.c_int]
    L.vilf_scan2map_step.argtypes = [vp, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_float), C.c_int, C.POINTER(abi.Scan2MapResult)]
    L.vilf_scan2map_get_map.argtypes = [vp, C.c_int, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int)]
    L.vilf_scan2map_set_pose.argtypes = [vp, abi.c_double_p, abi.c_double_p]
    fpp = C.POINTER(C.c_float)
    L.vilf_scan2map_batch_create.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.vilf_scan2map_batch_init.argtypes = [vp, C.c_int, fpp, C.c_int, fpp, C.c_int, abi.c_double_p, abi.c_double_p]
    L.vilf_scan2map_batch_set_scan.argtypes = [vp, C.c_int, fpp, C.c_int, fpp, C.c_int]
    L.vilf_scan2map_batch_step.argtypes = [vp, C.c_int]
    L.vilf_scan2map_batch_snapshot.argtypes = [vp]
    L.vilf_get_profile_scan2map.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_long)]
    L.vilf_get_profile_marginalize.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_long)]
    L.vilf_batch_marginalize_stats.argtypes = [vp, C.POINTER(C.c_int)]
    L.vilf_get_profile_large_window.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_long)]
    L.vilf_scan2map_batch_rewind.argtypes = [vp]
    L.vilf_scan2map_batch_copy_stream.argtypes = [vp, C.c_int, C.c_int]
    L.vilf_scan2map_batch_results.argtypes = [vp, C.c_int, C.c_int, C.POINTER(abi.Scan2MapResult)]
    L.vilf_scan2map_batch_get_map.argtypes = [vp, C.c_int, C.c_int, fpp, C.c_int, C.POINTER(C.c_int)]
    ip = C.POINTER(C.c_int)
    L.vilf_sc_default_params.argtypes = [C.POINTER(abi.ScParams)]
    L.vilf_sc_default_params.restype = None
    L.vilf_sc_create.argtypes = [vp, C.POINTER(abi.ScParams), C.c_int]
    L.vilf_sc_add_keyframe.argtypes = [vp, fpp, C.c_int, ip]
    L.vilf_sc_add_keyframes.argtypes = [vp, C.c_int, fpp, ip, ip]
    L.vilf_sc_detect.argtypes = [vp, C.POINTER(abi.ScResult)]
    L.vilf_sc_detect_range.argtypes = [vp, C.c_int, C.c_int, C.POINTER(abi.ScResult)]
    L.vilf_sc_get.argtypes = [vp, C.c_int, abi.c_double_p, fpp, abi.c_double_p]
    L.vilf_sc_size.argtypes = [vp, ip]
    L.vilf_get_profile_sc.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_long)]
    L.vilf_icp_default_params.argtypes = [C.POINTER(abi.IcpParams)]
    L.vilf_icp_default_params.restype = None
    L.vilf_icp_create.argtypes = [vp, C.POINTER(abi.IcpParams), C.c_int, C.c_long]
    L.vilf_icp_add_cloud.argtypes = [vp, fpp, C.c_int, ip]
    L.vilf_icp_add_clouds.argtypes = [vp, C.c_int, fpp, ip, ip]
    L.vilf_icp_size.argtypes = [vp, ip]
    L.vilf_icp_submap.argtypes = [vp, C.c_int, C.c_int, C.c_int, abi.c_double_p, fpp, C.c_int, ip]
    L.vilf_icp_align.argtypes = [vp, C.c_int, C.c_int, abi.c_double_p, abi.c_double_p, C.POINTER(abi.IcpResult)]
    L.vilf_icp_align_pairs.argtypes = [vp, C.c_int, ip, ip, abi.c_double_p, abi.c_double_p, C.POINTER(abi.IcpResult)]
    L.vilf_icp_get_history.argtypes = [vp, C.c_int, C.POINTER(abi.IcpIter), C.c_int, ip]
    L.vilf_icp_get_search.argtypes = [vp, C.c_int, C.c_int, ip, fpp, C.c_int, ip]
    L.vilf_get_profile_icp.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_long)]
    L.vilf_icp_global_map.argtypes = [vp, C.c_int, C.c_int, C.c_int, abi.c_double_p, abi.c_long_p]
    L.vilf_icp_global_map_size.argtypes = [vp, abi.c_long_p]
    L.vilf_icp_global_map_get.argtypes = [vp, C.c_long, C.c_long, fpp]
    L.vilf_get_profile_icp_map.argtypes = [vp, C.POINTER(C.c_double), abi.c_long_p]
    u8p = C.POINTER(C.c_uint8)
    L.vilf_track_init.argtypes = [vp, C.POINTER(abi.TrackParams)]
    L.vilf_track_reset.argtypes = [vp]
    L.vilf_track_read_image.argtypes = [vp, u8p, C.c_int, C.c_double, ip]
    L.vilf_track_get.argtypes = [vp, C.c_int, ip, ip, fpp, fpp, fpp, ip]
    L.vilf_track_pyramid.argtypes = [vp, u8p, C.c_int, C.c_int, u8p]
    L.vilf_track_lk.argtypes = [vp, u8p, u8p, fpp, C.c_int, fpp, u8p]
    L.vilf_track_detect.argtypes = [vp, u8p, fpp, C.c_int, C.c_int, fpp, ip]
    L.vilf_track_profile.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_long)]
    L.vilf_track_configure.argtypes = [vp, C.POINTER(abi.TrackFrontend)]
    L.vilf_track_clahe.argtypes = [vp, u8p, C.c_int, u8p]
    L.vilf_track_reject_f.argtypes = [vp, fpp, fpp, C.c_int, u8p, abi.c_double_p, ip, ip]
    L.vilf_track_profile_frontend.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_long)]
    L.vilf_track_configure_mask.argtypes = [vp, C.POINTER(abi.TrackMaskParams)]
    L.vilf_track_set_fisheye_mask.argtypes = [vp, u8p, C.c_int]
    L.vilf_track_read_image_mask.argtypes = [vp, u8p, C.c_int, u8p, C.c_int, C.c_double, ip]
    L.vilf_track_erode.argtypes = [vp, u8p, C.c_int, u8p]
    L.vilf_track_probe.argtypes = [vp, u8p, fpp, C.c_int, u8p]
    L.vilf_track_reject_f_mask.argtypes = [vp, fpp, fpp, u8p, C.c_int, u8p, abi.c_double_p, ip, ip]
    L.vilf_track_detect_masked.argtypes = [vp, u8p, u8p, fpp, C.c_int, C.c_int, fpp, ip]
    L.vilf_track_profile_mask.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_long)]
    L.vilf_startup_default_params.argtypes = [C.POINTER(abi.StartupParams)]
    L.vilf_startup_default_params.restype = None
    L.vilf_startup_relative_pose.argtypes = [vp, C.POINTER(abi.StartupParams), C.c_int, C.POINTER(abi.StartupWindow), C.POINTER(abi.StartupResult), C.POINTER(abi.StartupPair)]
    L.vilf_startup_get_correspondences.argtypes = [vp, C.c_int, ip, u8p, abi.c_double_p]
    L.vilf_startup_profile.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_long)]
    L.vilf_startup_default_sfm_params.argtypes = [C.POINTER(abi.StartupSfmParams)]
    L.vilf_startup_default_sfm_params.restype = None
    L.vilf_startup_sfm.argtypes = [vp, C.POINTER(abi.StartupSfmParams), C.c_int, C.POINTER(abi.StartupWindow), C.POINTER(abi.StartupResult), C.POINTER(abi.StartupStructure),
                                   C.POINTER(abi.StartupFrame)]
    L.vilf_startup_get_structure.argtypes = [vp, C.c_int, u8p, abi.c_double_p]
    L.vilf_startup_pnp.argtypes = [vp, C.POINTER(abi.StartupSfmParams), C.c_int, C.POINTER(abi.StartupPnpProblem), C.POINTER(abi.StartupFrame)]
    L.vilf_startup_sfm_profile.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_long)]
    L.vilf_startup_default_ba_params.argtypes = [C.POINTER(abi.StartupBaParams)]
    L.vilf_startup_default_ba_params.restype = None
    L.vilf_startup_ba.argtypes = [vp, C.POINTER(abi.StartupBaParams), C.c_int, C.POINTER(abi.StartupWindow), C.POINTER(abi.StartupBaStart), C.POINTER(abi.StartupBaResult),
                                  C.POINTER(abi.StartupBaFrame)]
    L.vilf_startup_construct.argtypes = [vp, C.POINTER(abi.StartupSfmParams), C.POINTER(abi.StartupBaParams), C.c_int, C.POINTER(abi.StartupWindow), C.POINTER(abi.StartupResult),
                                         C.POINTER(abi.StartupBaResult), C.POINTER(abi.StartupBaFrame), C.POINTER(abi.StartupStructure), C.POINTER(abi.StartupFrame)]
    L.vilf_startup_get_ba_structure.argtypes = [vp, C.c_int, u8p, abi.c_double_p]
    L.vilf_startup_ba_profile.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_long)]
    L.vilf_features_triangulate.argtypes = [vp, C.c_int, C.POINTER(abi.TriWindow), C.POINTER(abi.TriResult)]
    L.vilf_features_profile.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_long)]
    L.vilf_exrot_default_params.argtypes = [C.POINTER(abi.ExrotParams)]
    L.vilf_exrot_default_params.restype = None
    L.vilf_exrot_reset.argtypes = [vp, C.c_int]
    L.vilf_exrot_push.argtypes = [vp, C.POINTER(abi.ExrotParams), C.c_int, C.POINTER(abi.ExrotPair), C.POINTER(abi.ExrotResult)]
    L.vilf_exrot_get_history.argtypes = [vp, C.c_int, ip, abi.c_double_p, abi.c_double_p, abi.c_double_p, abi.c_double_p, abi.c_double_p]
    L.vilf_exrot_profile.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_long)]
    u64p = C.POINTER(C.c_uint64)
    L.vilf_kf_default_params.argtypes = [C.POINTER(abi.KfParams)]
    L.vilf_kf_default_params.restype = None
    L.vilf_kf_create.argtypes = [vp, C.POINTER(abi.KfParams), C.c_int, C.c_long]
    L.vilf_kf_add_keyframe.argtypes = [vp, u8p, C.c_int, fpp, C.c_int, ip, ip]
    L.vilf_kf_add_loaded.argtypes = [vp, C.c_int, fpp, fpp, u64p, C.c_int, fpp, u64p, ip]
    L.vilf_kf_get.argtypes = [vp, C.c_int, C.c_int, fpp, fpp, u64p, ip, C.c_int, fpp, u64p, ip]
    L.vilf_kf_size.argtypes = [vp, ip]
    L.vilf_kf_match.argtypes = [vp, C.c_int, C.c_int, ip, u8p, fpp, fpp, ip, ip, ip]
    L.vilf_kf_blur.argtypes = [vp, u8p, C.c_int, u8p]
    L.vilf_kf_fast.argtypes = [vp, u8p, C.c_int, C.c_int, fpp, u8p, ip]
    L.vilf_kf_brief.argtypes = [vp, u8p, C.c_int, fpp, C.c_int, u64p]
    L.vilf_kf_profile.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_long)]
    L.vilf_kf_default_loop_params.argtypes = [C.POINTER(abi.KfLoopParams)]
    L.vilf_kf_default_loop_params.restype = None
    L.vilf_kf_set_geometry.argtypes = [vp, C.c_int, fpp, abi.c_double_p, abi.c_double_p]
    L.vilf_kf_find_connection.argtypes = [vp, C.POINTER(abi.KfLoopParams), C.c_int, C.c_int, ip, C.POINTER(abi.KfLoopResult), u8p, fpp]
    L.vilf_kf_loop_profile.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_long)]
    L.vilf_pg4_default_params.argtypes = [C.POINTER(abi.Pg4Params)]
    L.vilf_pg4_default_params.restype = None
    L.vilf_pg4_optimize.argtypes = [vp, C.POINTER(abi.Pg4Params), C.c_int, abi.c_double_p, abi.c_double_p, ip, ip, C.c_int, C.POINTER(abi.Pg4Loop),
                                    abi.c_double_p, abi.c_double_p, abi.c_double_p, C.POINTER(abi.Pg4Result), abi.c_double_p]
    L.vilf_pg4_profile.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_long)]
    L.vilf_kf_bow_default_params.argtypes = [C.POINTER(abi.BowParams)]
    L.vilf_kf_bow_default_params.restype = None
    L.vilf_kf_bow_set_vocabulary.argtypes = [vp, C.POINTER(abi.BowVocabulary)]
    L.vilf_kf_bow_add.argtypes = [vp, C.c_int]
    L.vilf_kf_bow_add_range.argtypes = [vp, C.c_int, C.c_int]
    L.vilf_kf_bow_detect.argtypes = [vp, C.POINTER(abi.BowParams), C.c_int, C.POINTER(abi.BowResult)]
    L.vilf_kf_bow_detect_range.argtypes = [vp, C.POINTER(abi.BowParams), C.c_int, C.c_int, C.POINTER(abi.BowResult)]
    L.vilf_kf_bow_get.argtypes = [vp, C.c_int, C.c_int, ip, abi.c_double_p, ip]
    L.vilf_kf_bow_transform.argtypes = [vp, u64p, C.c_int, ip, abi.c_double_p]
    L.vilf_kf_bow_size.argtypes = [vp, ip]
    L.vilf_kf_bow_profile.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_long)]
    _lib = L
    return L


def default_options():
    o = abi.Options()
    lib().vilf_default_options(C.byref(o))
    return o
