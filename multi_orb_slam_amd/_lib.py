"""ctypes loader of lib/libmorb.so.  Fails loudly when the HIP library is missing: there is no fallback path."""
import ctypes as C
import os
import subprocess
import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_PKG, "csrc")
# MORB_LIB_PATH: load an instrumented build of the same library (csrc/Makefile PHASES=1) instead; experiments only
LIB_PATH = os.environ.get("MORB_LIB_PATH") or os.path.join(_PKG, "lib", "libmorb.so")

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                     ("octave", "<i4"), ("class_id", "<i4")])
QUERY_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("radius", "<f4"), ("ur", "<f4"), ("min_level", "<i4"),
                        ("max_level", "<i4"), ("cam", "<i4"), ("blocks", "<i4"), ("angle", "<f4"),
                        ("desc", "u1", (32,))])
WINDOW_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("radius", "<f4"), ("cam", "<i4"), ("min_level", "<i4"), ("max_level", "<i4")])
assert KP_DTYPE.itemsize == 28 and QUERY_DTYPE.itemsize == 68 and WINDOW_DTYPE.itemsize == 24
POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_dist", "<f4"), ("max_dist", "<f4"),
                        ("blocks", "<i4"), ("desc", "u1", (32,))])
TRACK_DTYPE = np.dtype([("proj_x", "<f4"), ("proj_y", "<f4"), ("proj_xr", "<f4"), ("view_cos", "<f4"), ("level", "<i4"),
                        ("in_view", "<i4")])
assert POINT_DTYPE.itemsize == 68 and TRACK_DTYPE.itemsize == 24
REFRESH_DTYPE = np.dtype([("desc", "u1", (32,)), ("normal", "<f4", (3,)), ("min_dist", "<f4"), ("max_dist", "<f4"),
                          ("best_obs", "<i4"), ("best_median", "<i4")])   # orbm_refresh_out
assert REFRESH_DTYPE.itemsize == 60
REFRESH_DESCRIPTOR, REFRESH_NORMAL_DEPTH, REFRESH_CAP = 1, 2, 256
OBS_DTYPE = np.dtype([("point", "<i4"), ("keyframe", "<i4")])   # orbm_obs
assert OBS_DTYPE.itemsize == 8
MAX_POINTS, MAP_MAX_KEYFRAMES, MAP_MAX_FEATURES, MAP_MAX_LOCAL, POINT_BAD = 65535, 16384, 8192, 4096, 1
COVIS_DTYPE = np.dtype([("keyframe", "<i4"), ("all", "<i4"), ("cam1", "<i4")])   # orbm_covis_entry
assert COVIS_DTYPE.itemsize == 12
CORRECT_DTYPE = np.dtype([("point", "<i4"), ("position", "<i4")])   # orbm_correct_entry
FEATURE_LEVEL_MASK, FEATURE_FAR = 0x1f, 0x80
POSE_PROBLEM_DTYPE = np.dtype([("Tcw", "<f4", (16,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("bf", "<f4"),
                               ("Rcam12", "<f4", (9,)), ("tcam12", "<f4", (3,)), ("inv_level_sigma2", "<f4", (32,)),
                               ("n_levels", "<i4"), ("mode", "<i4"), ("n_cam0", "<i4")])   # orbm_pose_problem
POSE_ROUND_DTYPE = np.dtype([("iterations", "<i4"), ("trials", "<i4"), ("chi2", "<f8"), ("lambda", "<f8")])
POSE_RESULT_DTYPE = np.dtype([("Tcw", "<f4", (16,)), ("q", "<f8", (4,)), ("t", "<f8", (3,)), ("n_initial", "<i4"), ("n_bad", "<i4"),
                              ("n_inliers", "<i4"), ("rounds", "<i4"), ("round", POSE_ROUND_DTYPE, (4,))])   # orbm_pose_result
assert POSE_PROBLEM_DTYPE.itemsize == 272 and POSE_RESULT_DTYPE.itemsize == 232
POSE_CAM0, POSE_ALL_CAMS, POSE_ORDER_INDEX, POSE_ORDER_DEVICE, POSE_CAP, POSE_MAX_BATCH = 0, 1, 0, 1, 8192, 64
SIM3_PROBLEM_DTYPE = np.dtype([("fx1", "<f4"), ("fy1", "<f4"), ("cx1", "<f4"), ("cy1", "<f4"), ("fx2", "<f4"), ("fy2", "<f4"), ("cx2", "<f4"),
                               ("cy2", "<f4"), ("Rcam21", "<f4", (9,)), ("tcam21", "<f4", (3,)), ("fix_scale", "<i4")])   # orbm_sim3_problem
SIM3_HYP_DTYPE = np.dtype([("R12", "<f4", (9,)), ("t12", "<f4", (3,)), ("s12", "<f4"), ("T12", "<f4", (16,)), ("T21", "<f4", (16,)),
                           ("n_inliers", "<i4")])   # orbm_sim3_hyp
SIM3_WALK_DTYPE = np.dtype([("iterations", "<i4"), ("best_inliers", "<i4"), ("best_index", "<i4"), ("no_more", "<i4")])   # orbm_sim3_walk_state
assert SIM3_PROBLEM_DTYPE.itemsize == 84 and SIM3_HYP_DTYPE.itemsize == 184 and SIM3_WALK_DTYPE.itemsize == 16
SIM3_MATH_LIBM, SIM3_MATH_DEVICE, SIM3_CAP, SIM3_MAX_ITS, SIM3_MAX_BATCH = 0, 1, 8192, 1024, 64
SIM3OPT_PROBLEM_DTYPE = np.dtype([("K1", "<f4", (4,)), ("K2", "<f4", (4,)), ("inv_level_sigma2_1", "<f4", (32,)),
                                  ("inv_level_sigma2_2", "<f4", (32,)), ("n_levels1", "<i4"), ("n_levels2", "<i4"), ("R", "<f4", (9,)),
                                  ("t", "<f4", (3,)), ("s", "<f4"), ("th2", "<f4"), ("fix_scale", "<i4")])   # orbm_sim3opt_problem
SIM3OPT_RESULT_DTYPE = np.dtype([("q", "<f8", (4,)), ("t", "<f8", (3,)), ("s", "<f8"), ("n_inliers", "<i4"), ("n_correspondences", "<i4"),
                                 ("n_bad", "<i4"), ("n_more_iterations", "<i4"), ("written", "<i4"), ("optimisations", "<i4"),
                                 ("round", POSE_ROUND_DTYPE, (2,))])   # orbm_sim3opt_result
assert SIM3OPT_PROBLEM_DTYPE.itemsize == 356 and SIM3OPT_RESULT_DTYPE.itemsize == 136
SIM3OPT_CAP, SIM3OPT_MAX_BATCH = 8192, 64
LBA_MAX_FREE, LBA_MAX_POSES, LBA_MAX_POINTS, LBA_MAX_EDGES = 64, 4096, 65536, 262144
LBA_ENDED_COMPLETE, LBA_ENDED_STOPPED_AT_START, LBA_ENDED_NO_SECOND = 0, 1, 2
LBA_FLAG_LEVEL1, LBA_FLAG_ERASE = 1, 2
BA_MAX_FREE, BA_MAX_POSES, BA_MAX_POINTS, BA_MAX_EDGES, BA_PANEL = 1024, 4096, 1 << 19, 1 << 22, 64
EG_MAX_FREE, EG_MAX_VERTICES, EG_MAX_EDGES, EG_MAX_POINTS = 877, 4096, 65536, 1 << 19
PNP_PROBLEM_DTYPE = np.dtype([("fu", "<f8"), ("fv", "<f8"), ("uc", "<f8"), ("vc", "<f8"), ("min_inliers", "<i4"), ("best_start", "<i4")])   # orbm_pnp_problem
PNP_HYP_DTYPE = np.dtype([("R", "<f8", (9,)), ("t", "<f8", (3,)), ("rep_error", "<f8"), ("choice", "<i4"), ("n_inliers", "<i4"), ("flags", "<i4"),
                          ("reserved", "<i4")])   # orbm_pnp_hyp
PNP_REFINED_DTYPE = np.dtype([("hyp", "<i4"), ("n_set", "<i4"), ("n_inliers", "<i4"), ("flags", "<i4"), ("R", "<f8", (9,)), ("t", "<f8", (3,))])   # orbm_pnp_refined
PNP_WALK_DTYPE = np.dtype([("iterations", "<i4"), ("best_inliers", "<i4"), ("best_hyp", "<i4"), ("best_record", "<i4"), ("best_refined_inliers", "<i4"),
                           ("no_more", "<i4"), ("current", "<i4"), ("exhausted", "<i4")])   # orbm_pnp_walk_state
assert PNP_PROBLEM_DTYPE.itemsize == 40 and PNP_HYP_DTYPE.itemsize == 120 and PNP_REFINED_DTYPE.itemsize == 112 and PNP_WALK_DTYPE.itemsize == 32
PNP_CAP, PNP_MAX_ITS, PNP_MAX_BATCH, PNP_MAX_RECORDS = 8192, 1024, 64, 16
PNP_FLAG_SINGULAR_QR, PNP_FLAG_RANDOM_SVD = 1, 2
PNP_WALK_NOTHING, PNP_WALK_REFINED, PNP_WALK_BEST = 0, 1, 2

ORB_OK, ORB_E_ARG, ORB_E_HIP, ORB_E_CAPACITY, ORB_E_NO_DEVICE, ORB_E_TIMEOUT = 0, -1, -2, -3, -4, -5


class OrbError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libmorb error %d: %s" % (code, msg))
        self.code = code


class LbaProblem(C.Structure):  # orbm_lba_problem
    _fields_ = [("n_free", C.c_int32), ("n_poses", C.c_int32), ("n_points", C.c_int32), ("reserved", C.c_int32), ("Tcw", C.c_void_p),
                ("K", C.c_void_p), ("points", C.c_void_p), ("bad", C.c_void_p), ("first", C.c_void_p), ("edge_pose", C.c_void_p),
                ("edge_cam", C.c_void_p), ("obs", C.c_void_p), ("inv_sigma2", C.c_void_p), ("Tcim", C.c_float * 32)]


class PoseRound(C.Structure):  # orbm_pose_round
    _fields_ = [("iterations", C.c_int32), ("trials", C.c_int32), ("chi2", C.c_double), ("lambda_", C.c_double)]


class LbaResult(C.Structure):  # orbm_lba_result
    _fields_ = [("pose", C.c_void_p), ("Tcw", C.c_void_p), ("point", C.c_void_p), ("point_f", C.c_void_p), ("flags", C.c_void_p),
                ("round", PoseRound * 2), ("ended", C.c_int32), ("optimisations", C.c_int32), ("polls", C.c_int32), ("n_level1", C.c_int32),
                ("n_erase", C.c_int32), ("active_poses", C.c_int32 * 2), ("active_points", C.c_int32 * 2), ("active_edges", C.c_int32 * 2),
                ("reserved", C.c_int32)]


class BaResult(C.Structure):  # orbm_ba_result
    _fields_ = [("pose", C.c_void_p), ("Tcw", C.c_void_p), ("point", C.c_void_p), ("point_f", C.c_void_p), ("round", PoseRound),
                ("optimised", C.c_int32), ("polls", C.c_int32), ("active_poses", C.c_int32), ("active_points", C.c_int32),
                ("active_edges", C.c_int32), ("reserved", C.c_int32 * 3)]


class EgProblem(C.Structure):  # orbm_eg_problem
    _fields_ = [("n_free", C.c_int32), ("n_vertices", C.c_int32), ("n_edges", C.c_int32), ("n_points", C.c_int32), ("fix_scale", C.c_int32),
                ("reserved", C.c_int32 * 3), ("vertex", C.c_void_p), ("measurement", C.c_void_p), ("edge_v0", C.c_void_p),
                ("edge_v1", C.c_void_p), ("points", C.c_void_p), ("point_ref", C.c_void_p)]


class EgResult(C.Structure):  # orbm_eg_result
    _fields_ = [("estimate", C.c_void_p), ("Tiw", C.c_void_p), ("point_f", C.c_void_p), ("round", PoseRound), ("optimised", C.c_int32),
                ("active_vertices", C.c_int32), ("active_edges", C.c_int32), ("reserved", C.c_int32)]


LBA_STOP_FN = C.CFUNCTYPE(C.c_int, C.c_void_p)   # orbm_lba_stop_fn


class Params(C.Structure):  # orbx_params
    _fields_ = [("nfeatures", C.c_int32), ("scale_factor", C.c_float), ("nlevels", C.c_int32),
                ("ini_th_fast", C.c_int32), ("min_th_fast", C.c_int32)]


class Calibration(C.Structure):  # orb_calibration
    _fields_ = [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")]


class CamFeatures(C.Structure):  # orbm_cam_features
    _fields_ = [("d_kps", C.c_void_p), ("d_desc", C.c_void_p), ("n", C.c_int32), ("d_depth", C.c_void_p),
                ("depth_stride", C.c_int32)]


class FImage(C.Structure):  # orbf_image
    _fields_ = [("data", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("stride", C.c_int32),
                ("on_device", C.c_int32), ("generation", C.c_uint64)]


class FResult(C.Structure):  # orbf_result
    _fields_ = [("n_cams", C.c_int32), ("n_total", C.c_int32), ("counts", C.c_void_p), ("kps", C.c_void_p),
                ("desc", C.c_void_p), ("uright", C.c_void_p), ("depth", C.c_void_p), ("nmatches", C.c_int32),
                ("match_of_feature", C.c_void_p), ("cross_best_idx", C.c_void_p), ("cross_best_dist", C.c_void_p),
                ("cross_second_dist", C.c_void_p), ("gpu_wait_us", C.c_float), ("n_queries", C.c_int32),
                ("queries", C.c_void_p), ("un_x", C.c_void_p), ("un_y", C.c_void_p), ("host_us", C.c_float * 4),
                ("rig_cams", C.c_int32), ("rig_counts", C.c_void_p)]


class FMotion(C.Structure):  # orbf_motion
    _fields_ = [("du", C.c_float), ("dv", C.c_float), ("th", C.c_float)]


class FStreamStats(C.Structure):  # orbf_stream_stats
    _fields_ = [("features", C.c_int64), ("temporal_matches", C.c_int64), ("cross_accepted", C.c_int64), ("digest", C.c_uint64),
                ("seconds", C.c_double)]


class FrameDesc(C.Structure):  # orbm_frame_desc
    _fields_ = [("n_total", C.c_int32), ("n_cams", C.c_int32), ("un_x", C.c_void_p), ("un_y", C.c_void_p),
                ("octave", C.c_void_p), ("angle", C.c_void_p), ("uright", C.c_void_p), ("cam_of", C.c_void_p),
                ("local_of", C.c_void_p), ("desc", C.c_void_p), ("min_x", C.c_float), ("min_y", C.c_float),
                ("max_x", C.c_float), ("max_y", C.c_float)]


class View(C.Structure):  # orbm_view
    _fields_ = [("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("Ow", C.c_float * 3)] + \
               [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "mbf", "min_x", "max_x", "min_y", "max_y",
                                         "viewing_cos_limit", "th", "log_scale_factor")] + \
               [("n_levels", C.c_int32), ("scale_factors", C.c_void_p)]


class RefreshIn(C.Structure):  # orbm_refresh_in
    _fields_ = [("n_points", C.c_int32), ("n_obs", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("first", "obs_desc", "obs_centre", "obs_alive", "pos", "ref_centre", "ref_level", "what",
                                          "scale_factors")] + [("n_levels", C.c_int32)]


class DeviceFeatures(C.Structure):  # orbf_device_features
    _fields_ = [("n_total", C.c_int32), ("n_cams", C.c_int32), ("counts", C.c_int32 * 8), ("d_desc", C.c_void_p), ("d_angle", C.c_void_p),
                ("d_un_x", C.c_void_p), ("d_un_y", C.c_void_p), ("d_octave", C.c_void_p), ("d_uright", C.c_void_p), ("stream", C.c_void_p)]


class DeviceSide(C.Structure):  # orbv_device_side
    _fields_ = [("n", C.c_int32), ("d_desc", C.c_void_p), ("d_angle", C.c_void_p), ("d_x", C.c_void_p), ("d_y", C.c_void_p),
                ("d_octave", C.c_void_p), ("d_uright", C.c_void_p), ("n_cams", C.c_int32), ("cam_start", C.c_int32 * 9)]


class BowSide(C.Structure):  # orbv_side
    _fields_ = [("n", C.c_int32), ("desc", C.c_void_p), ("angle", C.c_void_p), ("flags", C.c_void_p), ("n_nodes", C.c_int32),
                ("node_id", C.c_void_p), ("node_start", C.c_void_p), ("items", C.c_void_p), ("x", C.c_void_p), ("y", C.c_void_p),
                ("octave", C.c_void_p), ("cam_of", C.c_void_p)]


class Triangulation(C.Structure):  # orbv_triangulation
    _fields_ = [("n_cams", C.c_int32), ("n_levels", C.c_int32), ("F12", (C.c_float * 9) * 8), ("ex", C.c_float * 8),
                ("ey", C.c_float * 8), ("scale_factors", C.c_void_p), ("level_sigma2", C.c_void_p)]


class TriKeyframe(C.Structure):  # orbv_tri_keyframe
    _fields_ = [("Tcw", (C.c_float * 12) * 2), ("centre", (C.c_float * 3) * 2), ("Twc", C.c_float * 12), ("Rcam12", C.c_float * 9),
                ("tcam12", C.c_float * 3)] + [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "invfx", "invfy", "mbf")] + \
               [("n_levels", C.c_int32), ("scale_factors", C.c_void_p), ("level_sigma2", C.c_void_p), ("n", C.c_int32), ("n_cam1", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("x", "y", "xd", "yd", "octave", "uright", "depth", "cos_stereo", "cam_of")]


class TriGeometry(C.Structure):  # orbv_tri_geometry
    _fields_ = [("kf1", TriKeyframe), ("kf2", TriKeyframe), ("cam_enabled", C.c_uint8 * 2), ("ratio_factor", C.c_float)]


class NewPointsRound(C.Structure):  # orbv_new_points_round
    _fields_ = [("b", C.c_void_p), ("flags_b", C.c_void_p), ("t", Triangulation), ("geometry", TriGeometry)]


def build(verbose=False):
    """Compile every HIP source for gfx950 into lib/libmorb.so (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC] + ([] if verbose else ["-s"])
    subprocess.check_call(cmd)
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OrbError(ORB_E_NO_DEVICE, "HIP library %s is not built (run `python -c 'import __graft_entry__ as g; "
                       "g.build()'` or `make -C multi_orb_slam_amd/csrc`); there is no CPU fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
    L.orb_last_error.restype = C.c_char_p
    L.orbx_tables.argtypes = [vp] * 7
    L.orbx_create.argtypes = [vp, i32, i32, i32, i32, vp]
    L.orbx_destroy.argtypes = [vp]; L.orbx_destroy.restype = None
    L.orbx_extract.argtypes = [vp, i32] + [vp] * 8
    L.orbx_upload.argtypes = [vp, i32, vp, i32, i32, i32]
    L.orbx_upload_device.argtypes = [vp, i32, vp, i32, i32, i32]
    L.orbx_run.argtypes = [vp]
    L.orbx_count.argtypes = [vp, i32]
    L.orbx_download.argtypes = [vp, i32, vp, vp, i32]
    L.orbx_device_keypoints.argtypes = [vp, i32]; L.orbx_device_keypoints.restype = vp
    L.orbx_device_descriptors.argtypes = [vp, i32]; L.orbx_device_descriptors.restype = vp
    L.orbx_stream.argtypes = [vp]; L.orbx_stream.restype = vp
    L.orbx_wait_for_stream.argtypes = [vp, vp]
    L.orbx_bind_output.argtypes = [vp, i32, vp, vp, i32]
    L.orbx_debug_level.argtypes = [vp, i32, i32, vp, i32, vp, vp]
    L.orbx_debug_candidates.argtypes = [vp, i32, i32, vp, i32, vp]
    L.orbx_debug_distribute_octree.argtypes = [vp, i32, i32, i32, i32, i32, i32, vp, i32, vp]
    L.orbx_set_profiling.argtypes = [vp, i32]
    L.orbx_stage_times_us.argtypes = [vp, vp]
    L.orbm_create.argtypes = [i32, vp]
    L.orbm_destroy.argtypes = [vp]; L.orbm_destroy.restype = None
    L.orbm_stream.argtypes = [vp]; L.orbm_stream.restype = vp
    L.orbm_descriptor_distance.argtypes = [vp, vp]
    L.orbm_three_maxima.argtypes = [vp, i32, vp]; L.orbm_three_maxima.restype = None
    L.orbm_hamming_top2.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp]
    L.orbm_use_matrix_cores.argtypes = [i32]
    L.orbm_use_fp4_top2.argtypes = [i32]
    L.orbm_top2_scratch_bytes.argtypes = [i32, i32]; L.orbm_top2_scratch_bytes.restype = C.c_size_t
    L.orbm_hamming_top2_device.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp, vp]
    L.orbm_hamming_matrix.argtypes = [vp, vp, i32, vp, i32, vp]
    L.orbm_hamming_matrix_device.argtypes = [vp, i32, vp, i32, vp, vp]
    L.orbm_frame_create.argtypes = [vp, vp, vp]
    L.orbm_frame_create_resident.argtypes = [vp, vp, vp, vp]
    L.orbm_frame_destroy.argtypes = [vp]; L.orbm_frame_destroy.restype = None
    L.orbm_set_stream.argtypes = [vp, vp]
    L.orbm_wait_for_stream.argtypes = [vp, vp]
    L.orbm_frame_from_device.argtypes = [vp, vp, i32, f32, f32, f32, f32, f32, vp]
    L.orbm_debug_frame_from_device_counts.argtypes = [vp, vp, i32, vp, f32, f32, f32, f32, f32, vp]
    L.orbm_frame_download.argtypes = [vp, vp, vp, vp, vp, vp]
    L.orbm_frame_count.argtypes = [vp]
    L.orbx_debug_last_path.argtypes = [vp]
    L.orbx_debug_level0_in_place.argtypes = [vp]
    L.orbx_debug_pyramid_form.argtypes = [vp]
    L.orbx_debug_pyramid_plan.argtypes = [i32, i32, i32]
    L.orbf_create.argtypes = [vp, i32, i32, i32, i32, vp]
    L.orbf_create_depth.argtypes = [vp, i32, i32, i32, i32, i32, vp]
    L.orbf_destroy.argtypes = [vp]; L.orbf_destroy.restype = None
    L.orbf_set_depth.argtypes = [vp, i32, vp, i32]
    L.orbf_configure.argtypes = [vp, f32, i32, i32]
    L.orbf_step.argtypes = [vp, vp, vp, i32, i32, vp]
    L.orbf_step_motion.argtypes = [vp, vp, vp, i32, vp]
    L.orbf_reset.argtypes = [vp]
    L.orbf_run_stream.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, i32, C.c_float, vp]
    L.orbf_prefetch.argtypes = [vp, vp]
    L.orbf_step_begin.argtypes = [vp, vp, vp, i32, i32, vp]
    L.orbf_step_motion_begin.argtypes = [vp, vp, vp, i32, vp]
    L.orbf_step_end.argtypes = [vp, vp]
    L.orbm_cross_top2_gathered_enqueue.argtypes = [vp, vp, i32, C.c_size_t, i32, i32, i32, vp, i32]
    L.orbm_cross_top2_gathered_collect.argtypes = [vp, vp, vp, vp, vp, vp]
    L.orbf_export_block.argtypes = [vp, vp, vp, vp]
    L.orbf_exchange_unique_id.argtypes = [vp]
    L.orbf_exchange_init.argtypes = [vp, vp, i32, i32]
    L.orbf_exchange_active.argtypes = [vp]
    L.orbf_step_motion_ahead.argtypes = [vp, vp, vp, vp, i32, i32, f32, vp, vp]
    L.orbf_ahead_depth.argtypes = [vp]
    L.orbf_exchange_placement.argtypes = [vp]
    L.orbf_debug_exchange_timing.argtypes = [vp, C.c_int]
    L.orbf_debug_exchange_us.argtypes = [vp, C.POINTER(C.c_float)]
    L.orbf_debug_exchange_redos.argtypes = [vp]; L.orbf_debug_exchange_redos.restype = C.c_long
    L.orbf_debug_last_frame.argtypes = [vp, vp]; L.orbf_debug_last_frame.restype = vp
    L.orbf_exchange_init_loopback.argtypes = [vp, i32, i32, i32]
    L.orbf_exchange_shutdown.argtypes = [vp]
    L.orbf_exchange_peer_handle_bytes.argtypes = []; L.orbf_exchange_peer_handle_bytes.restype = C.c_size_t
    L.orbf_exchange_peer_export.argtypes = [vp, i32, i32, vp]
    L.orbf_exchange_peer_open.argtypes = [vp, vp]
    L.orbf_peek_block.argtypes = [vp, vp, vp, vp, vp]
    L.orbm_cross_top2_gathered_views.argtypes = [vp, vp, vp, vp]
    L.orbm_cross_top2_gathered.argtypes = [vp, vp, i32, C.c_size_t, i32, i32, i32, vp, vp, vp, vp, vp]
    L.orbf_extractor.argtypes = [vp]; L.orbf_extractor.restype = vp
    L.orbf_matcher.argtypes = [vp]; L.orbf_matcher.restype = vp
    L.orbm_debug_last_resolve.argtypes = [vp, vp]
    L.orbm_debug_last_resolve_form.argtypes = [vp, vp]
    L.orbm_queries_from_motion.argtypes = [vp, vp, vp, vp, i32, f32, f32, f32, vp, f32, vp, vp, vp]
    L.orbm_count_ratio_accepted.argtypes = [vp, vp, i32, i32, f32]
    L.orbm_set_calibration.argtypes = [vp, vp]
    L.orbm_undistort_points.argtypes = [vp, vp, vp, i32, vp, vp]
    L.orbm_image_bounds.argtypes = [vp, i32, i32, vp]
    L.orbf_set_calibration.argtypes = [vp, vp]
    L.orbm_cross_top2.argtypes = [vp, vp, vp, vp, vp]
    L.orbm_cross_top2_blocks.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, vp]
    L.orbm_frame_grid.argtypes = [vp, vp, vp]
    L.orbm_features_in_area.argtypes = [vp, vp, i32, f32, f32, f32, i32, i32, vp, i32, vp]
    L.orbm_project_candidates.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp]
    L.orbm_project_best.argtypes = [vp, vp, vp, i32, vp, i32, vp, i32, vp, vp]
    L.orbm_search_by_projection.argtypes = [vp, vp, vp, i32, vp, i32, i32, vp, vp]
    L.orbm_search_by_projection_windows.argtypes = [vp, vp, vp, vp, i32, vp, i32, i32, vp, vp]
    L.orbm_debug_time_project.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp]
    L.orbm_search_by_projection_points.argtypes = [vp, vp, vp, i32, vp, f32, i32, vp, vp]
    L.orbm_points_create.argtypes = [vp, i32, vp]
    L.orbm_points_destroy.argtypes = [vp]; L.orbm_points_destroy.restype = None
    L.orbm_points_write.argtypes = [vp, vp, i32, i32, vp]
    L.orbm_points_count.argtypes = [vp]
    L.orbm_search_local_points.argtypes = [vp, vp, vp, i32, vp, vp, vp, f32, i32, vp, vp, vp, vp]
    L.orbm_level_thresholds.argtypes = [f32, i32, vp]
    L.orbm_frustum_host.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    L.orbm_map_create.argtypes = [vp, i32, i32, i32, i32, vp]
    L.orbm_map_destroy.argtypes = [vp]; L.orbm_map_destroy.restype = None
    L.orbm_map_write_points.argtypes = [vp, vp, vp, i32, vp, vp]
    L.orbm_map_write_observations.argtypes = [vp, vp, vp, i32, vp]
    L.orbm_map_write_keyframe.argtypes = [vp, vp, i32, vp, i32, i32]
    L.orbm_map_set_keyframe_bad.argtypes = [vp, vp, i32, i32]
    L.orbm_map_keyframes.argtypes = [vp]
    L.orbm_map_keyframe_bad.argtypes = [vp, i32]
    L.orbm_map_vote.argtypes = [vp, vp, vp, i32, vp]
    L.orbm_map_local_points.argtypes = [vp, vp, vp, i32, vp, vp]
    L.orbm_map_search_local_points.argtypes = [vp, vp, vp, vp, vp, i32, vp, i32, vp, f32, i32, vp, vp, vp, vp]
    L.orbm_local_map_vote_host.argtypes = [vp, i32, vp, i32, vp, i32, i32, vp]
    L.orbm_local_map_points_host.argtypes = [vp, vp, i32, i32, vp, i32, vp, i32, vp, i32, vp]
    L.orbm_debug_last_local_map.argtypes = [vp, vp]
    L.orbm_map_write_observation_features.argtypes = [vp, vp, vp, i32, vp]
    L.orbm_map_write_keyframe_features.argtypes = [vp, vp, i32, vp, i32, i32]
    L.orbm_map_write_point_nobs.argtypes = [vp, vp, vp, i32, vp]
    L.orbm_map_covisibility.argtypes = [vp, vp, vp, i32, vp, vp, i32]
    L.orbm_map_culling_counts.argtypes = [vp, vp, vp, i32, i32, vp]
    L.orbm_local_map_covisibility_host.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp, i32, i32, vp, i32, vp, vp, i32]
    L.orbm_local_map_culling_host.argtypes = [vp, vp, i32, vp, vp, i32, vp, vp, vp, i32, i32, vp, i32, i32, vp]
    L.orbm_debug_last_covisibility.argtypes = [vp, vp]
    L.orbm_map_points.argtypes = [vp]
    L.orbm_map_write_positions.argtypes = [vp, vp, vp, i32, vp]
    L.orbm_map_write_point_ref.argtypes = [vp, vp, vp, i32, vp]
    L.orbm_map_correct_sim3.argtypes = [vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, i32, vp, vp]
    L.orbm_map_correct_rigid.argtypes = [vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, i32, vp, vp]
    L.orbm_local_map_correct_sim3_host.argtypes = [vp, vp, i32, i32, vp, vp, i32, i32, vp, i32, vp, vp, vp, i32, vp, vp, i32, vp, vp]
    L.orbm_local_map_correct_rigid_host.argtypes = [vp, i32, vp, vp, i32, vp, i32, vp, vp, vp, i32, vp, vp, i32, vp, vp]
    L.orbm_debug_last_correction.argtypes = [vp, vp]
    L.orbm_debug_map_read_points.argtypes = [vp, vp, vp, i32, vp]
    L.orbm_refresh_points.argtypes = [vp, vp, vp]
    L.orbm_refresh_points_host.argtypes = [vp, vp]
    L.orbm_debug_last_refresh.argtypes = [vp, vp]
    L.orbm_pose_optimize.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.orbm_pose_optimize_host.argtypes = [vp, i32, vp, vp, vp, vp, vp, i32, vp, vp]
    L.orbm_pose_optimize_resident.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.orbm_debug_last_pose.argtypes = [vp, vp]
    L.orbm_pose_sincos.argtypes = [C.c_double, vp, vp]; L.orbm_pose_sincos.restype = None
    L.orbm_sim3_ransac.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbm_sim3_ransac_host.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp]
    L.orbm_sim3_walk.argtypes = [vp, i32, i32, i32, i32, i32, vp]
    L.orbm_sim3_iterations.argtypes = [C.c_double, i32, i32, i32]
    L.orbm_sim3_atan2.argtypes = [C.c_double, C.c_double]; L.orbm_sim3_atan2.restype = C.c_double
    L.orbm_debug_last_sim3.argtypes = [vp, vp]
    L.orbm_sim3_optimize.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbm_sim3_optimize_host.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp]
    L.orbm_sim3opt_exp.argtypes = [C.c_double]; L.orbm_sim3opt_exp.restype = C.c_double
    L.orbm_sim3opt_expmap.argtypes = [vp, i32, vp]
    L.orbm_sim3opt_ldlt7.argtypes = [vp, vp, vp]
    L.orbm_debug_last_sim3opt.argtypes = [vp, vp]
    L.orbm_local_ba.argtypes = [vp, vp, LBA_STOP_FN, vp, vp]
    L.orbm_local_ba_host.argtypes = [vp, LBA_STOP_FN, vp, i32, vp]
    L.orbm_lba_edge_eval.argtypes = [vp, vp, vp, vp, i32, vp, f32, vp]
    L.orbm_lba_ldlt.argtypes = [i32, vp, vp, vp]
    L.orbm_lba_controller_trace.argtypes = [vp, i32, vp, vp, i32, i32, i32, vp, vp]
    L.orbm_debug_last_local_ba.argtypes = [vp, vp]
    L.orbm_bundle_adjust.argtypes = [vp, vp, i32, i32, LBA_STOP_FN, vp, vp]
    L.orbm_bundle_adjust_host.argtypes = [vp, i32, i32, LBA_STOP_FN, vp, i32, vp]
    L.orbm_ba_ldlt.argtypes = [i32, vp, vp, vp]
    L.orbm_ba_ldlt_device.argtypes = [vp, i32, vp, vp, vp]
    L.orbm_debug_last_bundle_adjust.argtypes = [vp, vp]
    L.orbm_essential_graph.argtypes = [vp, vp, i32, vp]
    L.orbm_essential_graph_host.argtypes = [vp, i32, i32, vp]
    L.orbm_eg_edge_eval.argtypes = [vp, vp, vp, i32, i32, vp]
    L.orbm_sim3_log_eval.argtypes = [vp, i32, vp]
    L.orbm_pose_acos.argtypes = [C.c_double]; L.orbm_pose_acos.restype = C.c_double
    L.orbm_pose_log.argtypes = [C.c_double]; L.orbm_pose_log.restype = C.c_double
    L.orbm_debug_last_essential_graph.argtypes = [vp, vp]
    L.orbm_pnp_ransac.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32]
    L.orbm_pnp_ransac_host.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32]
    L.orbm_pnp_walk.argtypes = [vp, i32, i32, vp, vp, i32, i32, i32, i32, i32, vp]
    L.orbm_pnp_parameters.argtypes = [C.c_double, i32, i32, i32, C.c_float, i32, vp, vp]
    L.orbm_pnp_svd.argtypes = [vp, i32, i32, vp, vp, vp]
    L.orbm_pnp_qr_solve.argtypes = [vp, i32, i32, vp, vp]
    L.orbm_pnp_compute_pose.argtypes = [vp, vp, i32, vp, vp, vp, vp]; L.orbm_pnp_compute_pose.restype = C.c_double
    L.orbm_debug_last_pnp.argtypes = [vp, vp]
    L.orbm_debug_pnp_buffers.argtypes = [vp, vp]
    f64 = C.c_double
    L.orbv_create.argtypes = [i32, i32, vp, vp, vp, vp, i32, vp]
    L.orbv_load_text.argtypes = [C.c_char_p, i32, vp]
    L.orbv_destroy.argtypes = [vp]; L.orbv_destroy.restype = None
    L.orbv_info.argtypes = [vp, vp, vp, vp, vp]
    L.orbv_stream.argtypes = [vp]; L.orbv_stream.restype = vp
    L.orbv_transform.argtypes = [vp, vp, i32, i32, vp, vp, vp]
    L.orbv_transform_device.argtypes = [vp, vp, i32, i32, vp, vp, vp]
    L.orbv_bow_vectors.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.orbv_score_l1.argtypes = [vp, vp, i32, vp, vp, i32]; L.orbv_score_l1.restype = f64
    L.orbv_workspace_create.argtypes = [i32, vp]
    L.orbv_workspace_destroy.argtypes = [vp]; L.orbv_workspace_destroy.restype = None
    L.orbv_search_by_bow.argtypes = [vp, vp, vp, i32, i32, f32, i32, vp, vp]
    L.orbv_search_for_triangulation.argtypes = [vp, vp, vp, vp, i32, i32, vp, vp]
    L.orbv_debug_last_join.argtypes = [vp, vp]
    L.orbv_keyframe_create.argtypes = [vp, vp, vp]
    L.orbv_keyframe_destroy.argtypes = [vp]; L.orbv_keyframe_destroy.restype = None
    L.orbv_keyframe_count.argtypes = [vp]
    L.orbv_keyframe_from_device.argtypes = [vp, vp, vp, i32, vp, vp]
    L.orbv_keyframe_download.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbf_export_features.argtypes = [vp, vp]
    L.orbv_search_by_bow_resident.argtypes = [vp, vp, vp, vp, vp, i32, i32, f32, i32, vp, vp]
    L.orbv_search_for_triangulation_resident.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, vp, vp]
    L.orbv_cos_stereo.argtypes = [f32, vp, i32, vp]
    L.orbv_triangulate_pairs_host.argtypes = [vp, vp, vp, vp, i32, f32, vp]
    L.orbv_triangulate_pairs.argtypes = [vp, vp, vp, vp, vp, i32, f32, vp]
    L.orbv_keyframe_set_geometry.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.orbv_create_new_points_resident.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp]
    L.orbv_create_new_points_keyframe.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp]
    L.orbv_debug_last_keyframe_call.argtypes = [vp, vp]
    L.orbv_debug_last_keyframe_build.argtypes = [vp, vp]
    L.orbv_debug_last_db_query.argtypes = [vp, vp]
    L.orbv_db_create.argtypes = [i32, i32, vp]
    L.orbv_db_destroy.argtypes = [vp]; L.orbv_db_destroy.restype = None
    L.orbv_db_add.argtypes = [vp, C.c_uint64, vp, vp, i32]
    L.orbv_db_erase.argtypes = [vp, C.c_uint64]
    L.orbv_db_clear.argtypes = [vp]
    L.orbv_db_count.argtypes = [vp]
    L.orbv_db_query.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp, vp, vp]
    L.orbv_db_score.argtypes = [vp, vp, vp, i32, vp, i32, vp]
    _lib = L
    return L


def check(rc):
    if rc != ORB_OK:
        raise OrbError(rc, lib().orb_last_error().decode("utf-8", "replace"))


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)
