"""ctypes loader for cv_amd/lib/libakz.so (the C ABI of include/akz.h).

There is no CPU fallback: if the library is missing or no HIP device is usable, every entry point
raises.  (The CPU oracle under oracle/ is test infrastructure and is never imported from here.)
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libakz.so")


class AkzError(RuntimeError):
    def __init__(self, status, what=""):
        self.status = status
        msg = lib().akz_strerror(status).decode()
        hip = lib().akz_last_hip_error()
        if status == -5 and hip:
            msg += f" (hip {hip}: {lib().akz_last_hip_error_string().decode()})"
        super().__init__(f"{what}: {msg}" if what else msg)


class Config(C.Structure):
    """akz_config == akaze::Akaze (akaze/src/lib.rs:109-142)."""
    _fields_ = [
        ("maximum_features", C.c_uint64),
        ("num_sublevels", C.c_uint32),
        ("max_octave_evolution", C.c_uint32),
        ("base_scale_offset", C.c_double),
        ("initial_contrast", C.c_double),
        ("contrast_percentile", C.c_double),
        ("contrast_factor_num_bins", C.c_uint64),
        ("derivative_factor", C.c_double),
        ("detector_threshold", C.c_double),
        ("descriptor_channels", C.c_uint64),
        ("descriptor_pattern_size", C.c_uint64),
    ]


class Options(C.Structure):
    """akz_options (include/akz.h): behaviour switches of one context; all-zero = the defaults."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("flags", C.c_uint32), ("fed_block", C.c_uint32),
        ("sup_capacity", C.c_uint32), ("max_candidates", C.c_uint32), ("desc_tile_shift", C.c_uint32),
        ("stream_waves", C.c_uint32), ("stream_min_waves", C.c_uint32), ("arith", C.c_uint32), ("cu_ss", C.c_uint32),
        ("cu_kp", C.c_uint32), ("resident_min_frames", C.c_uint32), ("reserved", C.c_uint32 * 4),
    ]


OPT_KEEP_ALL, OPT_NO_FRAME_PAIRS, OPT_SERIAL_SUPPRESSION, OPT_NO_PIPELINE = 1, 2, 4, 8
OPT_STREAM_PRIORITY, OPT_CONTRAST_EXACT, OPT_CONTRAST_FORCE_ODD, OPT_TILE_KERNELS, OPT_SERIAL_DET, OPT_SPLIT_FRONT_FED, OPT_EQUAL_PRIORITY, OPT_NO_RESIDENT_LEVELS = 16, 32, 64, 128, 256, 512, 1024, 2048
HM_OPT_NO_FP4, HM_OPT_NO_MFMA, HM_OPT_STREAM_PRIORITY, HM_OPT_NO_LDS_DMA = 1, 2, 4, 8
HM_OPT_REVERSE_SEARCH, HM_OPT_REVERSE_LISTS, HM_OPT_REVERSE_SHARE_SHIFT = 16, 32, 8
FMT_U8, FMT_F32, FMT_U16 = 0, 1, 2
ARITH_REDUCE_PAIRWISE, ARITH_FMA, ARITH_HALF_SEQUENTIAL = 1, 2, 4


BOOL_OPTIONS = ("keep_all", "frame_pairs", "parallel_suppression", "pipeline", "stream_priority", "stream_kernels",
                "det_side_stream", "fuse_front_fed", "resident_levels")


def make_options(keep_all=False, frame_pairs=True, parallel_suppression=True, pipeline=True, stream_priority=True,
                 contrast="fine", fed_block=0, sup_capacity=0, max_candidates=0, desc_tile_shift=0, stream_kernels=True,
                 stream_waves=0, stream_min_waves=0, det_side_stream=True, fuse_front_fed=True, arith=0, cu_ss=0, cu_kp=0,
                 resident_levels=True, resident_min_frames=0):
    """Options with readable names.  contrast: "fine" (default), "exact", "force_odd".  arith: AKZ_ARITH_* bits (1: pairwise
    reduce_add, 2: fused mul_add, 4: sequential 2 x 2 sum) — the one option that changes results (include/akz.h)."""
    o = Options()
    o.struct_size = C.sizeof(Options)
    o.flags = ((OPT_KEEP_ALL if keep_all else 0) | (0 if frame_pairs else OPT_NO_FRAME_PAIRS)
               | (0 if parallel_suppression else OPT_SERIAL_SUPPRESSION) | (0 if pipeline else OPT_NO_PIPELINE)
               | (0 if stream_priority else OPT_EQUAL_PRIORITY) | (0 if stream_kernels else OPT_TILE_KERNELS)
               | (0 if det_side_stream else OPT_SERIAL_DET) | (0 if fuse_front_fed else OPT_SPLIT_FRONT_FED)
               | (0 if resident_levels else OPT_NO_RESIDENT_LEVELS)
               | {"fine": 0, "exact": OPT_CONTRAST_EXACT, "force_odd": OPT_CONTRAST_FORCE_ODD}[contrast])
    o.fed_block, o.sup_capacity, o.max_candidates, o.desc_tile_shift = fed_block, sup_capacity, max_candidates, desc_tile_shift
    o.stream_waves, o.stream_min_waves = stream_waves, stream_min_waves
    o.arith = arith
    o.cu_ss, o.cu_kp = cu_ss, cu_kp
    o.resident_min_frames = resident_min_frames
    return o


class ArrsacParams(C.Structure):
    """rs_arrsac_params (include/akz.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_hypotheses", C.c_uint32), ("block_size", C.c_uint32),
                ("init_blocks", C.c_uint32), ("max_candidates", C.c_uint32), ("flags", C.c_uint32),
                ("threshold", C.c_double), ("sprt_delta", C.c_double), ("sprt_ratio", C.c_double), ("seed", C.c_uint64),
                ("estimations_per_block", C.c_uint32), ("reserved", C.c_uint32)]


class ArrsacStats(C.Structure):
    _fields_ = [("poses", C.c_uint32), ("survivors", C.c_uint32), ("blocks", C.c_uint32), ("reserved", C.c_uint32),
                ("residuals_evaluated", C.c_uint64), ("residuals_exhaustive", C.c_uint64)]


RS_PRUNE_BOUND, RS_PRUNE_SPRT, RS_PRUNE_HALVE = 1, 2, 4
RS_ESTIMATOR_FIVE_POINT = 8
RS_BATCH_SHUFFLE = 1


class Camera(C.Structure):
    """rs_camera (include/akz.h)."""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("skew", C.c_double),
                ("k1", C.c_double), ("use_k1", C.c_int32), ("reserved", C.c_int32)]


class TriangulateParams(C.Structure):
    """rs_triangulate_params (include/akz.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("max_sweeps", C.c_uint32), ("eps", C.c_double),
                ("robust_minimum_observations", C.c_uint32), ("n_views", C.c_uint32),
                ("incidence_minimum_cosine_distance", C.c_double)]


class ThreeViewParams(C.Structure):
    """rs_three_view_params (include/akz.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("robust_view_num_robust_bearing_pair", C.c_uint32),
                ("maximum_cosine_distance", C.c_double), ("maximum_sine_distance", C.c_double),
                ("robust_observation_incidence_minimum_cosine_distance", C.c_double),
                ("robust_view_bearing_pair_minimum_cosine_distance", C.c_double), ("optimization_rate", C.c_double),
                ("three_view_minimum_relative_scales", C.c_uint32), ("three_view_filter_loop_iterations", C.c_uint32),
                ("three_view_optimization_landmarks", C.c_uint32), ("three_view_patience", C.c_uint32),
                ("three_view_minimum_robust_matches", C.c_uint32), ("hard_minimum_matches", C.c_uint32),
                ("triangulate", TriangulateParams)]


RS_TV_OK, RS_TV_FEW_SCALES, RS_TV_FEW_BEARING_PAIRS, RS_TV_FEW_MATCHES, RS_TV_LOST_HALF, RS_TV_FEW_ROBUST, RS_TV_BAD_INDEX = range(7)
RS_TV_MAX_LANDMARKS, RS_TV_MAX_RUNS, RS_TV_MAX_ITERATIONS, RS_TV_MAX_COMMON, RS_TV_STATS = 1024, 9, 1 << 20, 9216, 24
RS_TV_S_SCALES, RS_TV_S_MEDIAN, RS_TV_S_PAIRS, RS_TV_S_RUN_MATCHES, RS_TV_S_RUN_STOP, RS_TV_S_ROBUST, RS_TV_S_STAGE = 0, 1, 3, 4, 13, 22, 23


class ThreeViewConstraintParams(C.Structure):
    """rs_three_view_constraint_params (include/akz.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("optimization_minimum_landmarks", C.c_uint32),
                ("optimization_maximum_landmarks", C.c_uint32), ("constraint_patience", C.c_uint32),
                ("robust_view_num_robust_bearing_pair", C.c_uint32),
                ("robust_view_bearing_pair_minimum_cosine_distance", C.c_double)]


RS_TVC_OK, RS_TVC_FEW_LANDMARKS, RS_TVC_FEW_BEARING_PAIRS, RS_TVC_BAD_INDEX = range(4)
RS_TVC_MAX_LANDMARKS, RS_TVC_MAX_ITERATIONS, RS_TVC_STATS = 256, 1 << 20, 8
RS_TVC_S_LANDMARKS, RS_TVC_S_USED, RS_TVC_S_PAIRS, RS_TVC_S_ORIGINAL_SCALE, RS_TVC_S_FINAL_SCALE, RS_TVC_S_STAGE = 0, 1, 2, 3, 5, 7


class PoseGraphParams(C.Structure):
    """rs_pose_graph_params (include/akz.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("optimization_iterations", C.c_uint32), ("graph_optimization_rate", C.c_double)]


RS_PG_OK, RS_PG_FEW_VIEWS, RS_PG_NONFINITE, RS_PG_BAD_INDEX = range(4)
RS_PG_VIEW_UPDATED, RS_PG_VIEW_NO_CONSTRAINT, RS_PG_VIEW_NONFINITE = range(3)
RS_PG_RESIDENT_VIEWS, RS_PG_DEFAULT_RESIDENT_VIEWS, RS_PG_MAX_ITERATIONS, RS_PG_STATS = 256, 8, 1 << 20, 8
RS_PG_S_VIEWS, RS_PG_S_UPDATED, RS_PG_S_EDGES, RS_PG_S_ROUNDS, RS_PG_S_STAGE, RS_PG_S_FIRST_BAD_VIEW = range(6)

class ObservationFilterParams(C.Structure):
    """rs_observation_filter_params (include/akz.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("minimum_robust_landmarks", C.c_uint32), ("maximum_cosine_distance", C.c_double),
                ("maximum_sine_distance", C.c_double), ("reconstruction_optimization_iterations", C.c_uint32),
                ("reserved", C.c_uint32), ("triangulate", TriangulateParams)]


RS_OF_KEPT, RS_OF_SINGLE, RS_OF_PAIR_SPLIT, RS_OF_NO_POINT, RS_OF_KICKED, RS_OF_BAD_INDEX, RS_OF_SKIPPED = range(7)
RS_OF_OK, RS_OF_FEW_LANDMARKS, RS_OF_BAD_RANGE, RS_OF_RECON_SKIPPED = range(4)
RS_OF_NO_SOLVE, RS_OF_ROBUST_BEFORE, RS_OF_ROBUST_AFTER, RS_OF_STATS, RS_OF_MAX_ITERATIONS = 255, 1, 2, 8, 64
RS_OF_S_LANDMARKS, RS_OF_S_ROBUST_BEFORE, RS_OF_S_ROBUST_AFTER, RS_OF_S_OBS_SPLIT, RS_OF_S_PAIR_SPLIT, RS_OF_S_NO_POINT, RS_OF_S_KICKED = range(7)
RS_OR_OK, RS_OR_STAGE_RELAX, RS_OR_STAGE_FILTER, RS_OR_STOPPED = 0, 1, 2, 1 << 30

class CovisibilityParams(C.Structure):
    """rs_covisibility_params (include/akz.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("optimization_robust_covisibility_minimum_landmarks", C.c_uint32),
                ("optimization_maximum_three_view_constraints", C.c_uint32), ("optimization_minimum_new_constraints", C.c_uint32),
                ("optimization_minimum_landmarks", C.c_uint32), ("optimization_maximum_landmarks", C.c_uint32),
                ("candidate_limit", C.c_uint32), ("shuffle_seed", C.c_uint32)]


RS_CV_OK, RS_CV_FEW_CONSTRAINTS, RS_CV_BAD_INDEX, RS_CV_NO_GRAPH = range(4)
RS_CV_NOT_RECORDED, RS_CV_MAX_CANDIDATE_VIEWS, RS_CV_MAX_SLOTS, RS_CV_MAX_FEATURES, RS_CV_STATS = 16, 128, 256, 8192, 8
RS_CV_S_ROBUST, RS_CV_S_CANDIDATES, RS_CV_S_PAIRS, RS_CV_S_UNIQUE, RS_CV_S_EMITTED, RS_CV_S_FLAGS, RS_CV_S_RECORDED = range(7)
RS_CV_F_CANDIDATES_CAPPED, RS_CV_F_LIMIT_REACHED = 1, 2

class SingleViewParams(C.Structure):
    """rs_single_view_params (include/akz.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("single_view_optimization_num_matches", C.c_uint32),
                ("single_view_filter_loop_iterations", C.c_uint32), ("single_view_patience", C.c_uint32),
                ("single_view_optimization_rate", C.c_double), ("single_view_minimum_landmarks", C.c_uint32),
                ("single_view_minimum_robust_landmarks", C.c_uint32), ("maximum_cosine_distance", C.c_double),
                ("maximum_sine_distance", C.c_double), ("triangulate", TriangulateParams)]


RS_SV_OK, RS_SV_NO_MODEL, RS_SV_FEW_LANDMARKS, RS_SV_LOST_HALF, RS_SV_FEW_ROBUST, RS_SV_BAD_INDEX = range(6)
RS_SV_MAX_MATCHES, RS_SV_MAX_RUNS, RS_SV_MAX_ITERATIONS, RS_SV_STATS = 2048, 9, 1 << 20, 24
RS_SV_S_INLIERS, RS_SV_S_RUN_MATCHES, RS_SV_S_RUN_STOP, RS_SV_S_ROBUST, RS_SV_S_NO_OTHER, RS_SV_S_STAGE = 0, 1, 10, 19, 20, 21

RS_AV_OK, RS_AV_NOT_ACCEPTED, RS_AV_BAD_INDEX, RS_AV_BAD_TABLE = range(4)
RS_AV_S_OBSERVATIONS, RS_AV_S_MERGED, RS_AV_S_DEMOTED, RS_AV_S_NEW_LANDMARKS = range(4)
RS_AV_STATS, RS_AV_COUNTS, RS_LT_TILE = 4, 4, 1024
RS_IR_OK, RS_IR_BAD_TABLE, RS_IR_BAD_INDEX, RS_IR_SHARED_BLOCK = range(4)
RS_IR_C_ROWS, RS_IR_C_OBSERVATIONS, RS_IR_C_APPLIED, RS_IR_C_DEMOTED, RS_IR_C_NEW_ROWS, RS_IR_C_DROPPED, RS_IR_COUNTS = range(7)
RS_NR_OK, RS_NR_NOT_NORMAL, RS_NR_BAD_INDEX = range(3)
RS_EX_OK, RS_EX_OVERFLOW, RS_EX_BAD_TABLE = range(3)
RS_EX_C_POINTS, RS_EX_C_NO_POINT, RS_EX_C_INFINITE, RS_EX_C_BAD_ROWS, RS_EX_COUNTS = range(5)
RS_EX_CAMERA_WORDS, RS_EX_CAMERA_VERTICES = 10, 5
RS_JP_OK, RS_JP_NO_MODEL, RS_JP_FEW_INLIERS, RS_JP_BAD_INDEX = range(4)
RS_JP_DEFAULT_MINIMUM_ROBUST_MATCHES, RS_JP_MAX_FEATURES = 256, 9216
RS_AR_OK, RS_AR_NOT_ACCEPTED, RS_AR_BAD_INDEX, RS_AR_TAKEN, RS_AR_BAD_TABLE = range(5)
RS_AR_S_TRIPLES, RS_AR_S_FIRST, RS_AR_S_SECOND, RS_AR_S_LANDMARKS = range(4)
RS_AR_STATS, RS_AR_COUNTS = 4, 4
RS_RP_OK, RS_RP_BAD_TABLE, RS_RP_BAD_INDEX, RS_RP_BAD_MAP, RS_RP_NO_ROOM = range(5)
RS_RP_C_ROWS, RS_RP_C_OBSERVATIONS, RS_RP_C_EMPTY_DROPPED, RS_RP_C_ROWS_DROPPED, RS_RP_C_OBS_DROPPED, RS_RP_COUNTS = range(6)


class PlaceParams(C.Structure):
    """hm_place_params (include/akz.h)."""
    _fields_ = [("num_similar", C.c_uint32), ("num_recent", C.c_uint32), ("recent_threshold", C.c_uint32), ("search_num", C.c_uint32)]


HM_PL_OK, HM_PL_BAD_INDEX, HM_PL_BAD_TABLE = range(3)
HM_PL_C_RECENT, HM_PL_C_SIMILAR, HM_PL_C_SEARCHED, HM_PL_C_GROUPS, HM_PL_C_FREE, HM_PL_COUNTS = range(6)
HM_PL_MAX_HASH_BYTES, HM_PL_MAX_SEARCH, HM_PL_MAX_RECENT, HM_PL_NONE = 4096, 2048, 256, 0xFFFFFFFF
HM_VP_OK, HM_VP_CUT, HM_VP_NO_GROUP, HM_VP_FIND_REFUSED, HM_VP_BAD_VIEW, HM_VP_NO_ROOM = range(6)
HM_VP_C_BLOCKS, HM_VP_C_LIVE, HM_VP_C_VERDICT, HM_VP_C_FRAMES, HM_VP_COUNTS = range(5)
HM_VP_PICK_RECON, HM_VP_MAX_VIEWS = 1, 64

TRI_OK, TRI_TOO_FEW, TRI_NOT_ROBUST, TRI_EIGEN, TRI_NOT_FINITE, TRI_CHEIRALITY, TRI_BAD_INDEX = range(7)


class OverflowInfo(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("needed_candidates", C.c_uint32), ("candidate_capacity", C.c_uint32),
                ("keypoint_capacity", C.c_uint32)]


class LevelInfo(C.Structure):
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32),
        ("octave", C.c_uint32), ("sublevel", C.c_uint32),
        ("esigma", C.c_double), ("etime", C.c_double),
        ("n_fed_steps", C.c_uint32), ("deriv_sigma", C.c_uint32),
    ]


KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("response", "<f4"), ("size", "<f4"),
                     ("angle", "<f4"), ("octave", "<u4"), ("class_id", "<u4")])
NB_DTYPE = np.dtype([("index", "<u4"), ("distance", "<u4")])
assert KP_DTYPE.itemsize == 28 and NB_DTYPE.itemsize == 8

ABI_VERSION = 11         # include/akz.h AKZ_ABI_VERSION this file's argtypes were written against

# every symbol include/akz.h declares (tests check that the library exports all of them)
ABI_SYMBOLS = [
    "akz_config_default", "akz_create", "akz_create_ex", "akz_destroy", "akz_extract_gray_u8", "akz_extract_gray_u16",
    "akz_extract_gray_f32", "akz_extract_color",
    "akz_extract_batch", "akz_extract_batch_device", "akz_sync", "akz_stream", "akz_scale_space_device",
    "akz_last_overflow", "akz_num_levels", "akz_level", "akz_fed_tau", "akz_debug_get_level", "akz_debug_get_contrast",
    "akz_debug_get_keypoints", "akz_debug_portable_math", "akz_debug_orientation_masks", "akz_debug_rcp_error", "akz_gaussian_kernel", "akz_horizontal_filter", "akz_vertical_filter",
    "akz_half_size", "akz_sample_colors_rgb8", "hm_create", "hm_create_ex", "hm_destroy", "hm_knn2", "hm_knn", "hm_knn_views_device", "hm_knn_batch_device", "hm_best_of_views_device", "hm_best_of_views_batch_device", "hm_match",
    "hm_match_batch_device", "hm_sync", "hm_hash_bag", "hm_hash_bag_device", "hm_hash_knn", "hm_timing_enable",
    "hm_timing_get",
    "hm_stream", "rs_create", "rs_destroy", "rs_calibrate", "rs_essential_batch", "rs_five_point_batch", "rs_debug_essentials", "rs_essential_arrsac", "rs_p3p_arrsac", "rs_arrsac_samples",
    "rs_p3p_batch", "rs_debug_counts", "rs_debug_poses", "rs_batch_reserve", "rs_essential_arrsac_batch_device", "rs_sync",
    "rs_stream", "rs_debug_scene", "rs_debug_residuals", "rs_p3p_arrsac_batch_device", "hm_landmark_pairs_batch_device", "hm_landmark_matches_batch_device", "hm_landmark_matches_ordered_batch_device", "hm_landmark_original_matches_batch_device", "hm_set_targets", "hm_targets_generation", "hm_knn_targets", "rs_debug_scene_world", "rs_debug_far",
    "rs_triangulate_params_default", "rs_triangulate_observations", "rs_triangulate_landmarks_device", "rs_triangulate_merged_device",
    "rs_triangulate_pairs_batch_device", "rs_three_view_params_default", "rs_three_view_init_batch_device",
    "rs_three_view_constraint_params_default", "rs_three_view_constraint_batch_device",
    "rs_pose_graph_params_default", "rs_pose_graph_edges_device", "rs_pose_graph_relax_batch_device", "rs_pose_graph_debug_resident_views",
    "rs_observation_filter_params_default", "rs_filter_observations_device", "rs_optimize_reconstruction_batch_device",
    "rs_single_view_params_default", "rs_refine_poses_batch_device",
    "rs_covisibility_params_default", "rs_covisibility_candidates_device", "rs_covisibility_record_device", "rs_pose_graph_rows_device",
    "rs_landmarks_sharing_view_device", "rs_add_views_device",
    "rs_merge_map_device", "rs_incorporate_reconstruction_device", "rs_normalize_reconstruction_device",
    "rs_export_reconstruction_device", "rs_write_ply", "akz_sample_colors_batch_device",
    "rs_join_pairs_batch_device", "rs_add_reconstruction_batch_device",
    "hm_place_params_default", "hm_place_room", "hm_find_frames_batch_device",
    "hm_view_plan_device", "hm_knn_planned_batch_device", "hm_best_of_views_planned_batch_device",
    "rs_repack_table_device", "rs_gather_blocks_device", "rs_repack_constraints_device", "hm_place_remap_views_device",
    "akz_strerror", "akz_last_hip_error", "akz_last_hip_error_string", "akz_version", "akz_abi_version",
    "akz_timing_enable", "akz_timing_reset", "akz_timing_get",
    "akz_comm_unique_id", "akz_comm_create", "akz_comm_destroy", "akz_comm_shift_blocks", "akz_comm_allgather_blocks", "akz_comm_sync",
    "akz_comm_stream", "akz_comm_rank", "akz_comm_world", "akz_comm_timing", "akz_comm_last_error_string",
]

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -m cv_amd.build` (hipcc, gfx950). "
            "cv_amd has no CPU fallback.")
    # PyTorch-ROCm bundles its own HIP/HSA runtime.  A process must initialise only one: if libakz pulls in the
    # system runtime first and torch is imported afterwards (or the other way round with the roles swapped), the
    # second copy finds "no ROCm-capable device".  Importing torch first makes libakz resolve against the
    # runtime that is already loaded, whatever order the caller uses.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, i32, u32 = C.c_void_p, C.c_int32, C.c_uint32
    L.akz_strerror.restype = C.c_char_p
    L.akz_strerror.argtypes = [i32]
    L.akz_last_hip_error_string.restype = C.c_char_p
    L.akz_version.restype = C.c_char_p
    if not hasattr(L, "akz_abi_version"):   # a library from before the ABI carried a version: the same remedy
        raise RuntimeError(f"{LIB_PATH} exports no akz_abi_version (a build older than ABI 6), this binding was written "
                           f"against {ABI_VERSION} (include/akz.h AKZ_ABI_VERSION): rebuild with `python -m cv_amd.build`")
    L.akz_abi_version.restype = C.c_uint32
    L.akz_debug_rcp_error.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_double)]
    L.hm_targets_generation.restype = C.c_uint64
    L.hm_targets_generation.argtypes = [C.c_void_p]
    if L.akz_abi_version() != ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH} exports ABI {L.akz_abi_version()}, this binding was written against {ABI_VERSION} "
                           "(include/akz.h AKZ_ABI_VERSION): rebuild with `python -m cv_amd.build`")
    L.akz_config_default.argtypes = [C.POINTER(Config)]
    L.akz_create.argtypes = [C.POINTER(Config), i32, i32, i32, i32, u32, C.POINTER(vp)]
    L.akz_create_ex.argtypes = [C.POINTER(Config), i32, i32, i32, i32, u32, C.POINTER(Options), C.POINTER(vp)]
    L.akz_destroy.argtypes = [vp]
    L.akz_extract_gray_u16.argtypes = [vp, vp, i32, i32, i32, vp, vp, u32, C.POINTER(u32)]
    L.akz_extract_gray_u8.argtypes = [vp, vp, i32, i32, i32, vp, vp, u32, C.POINTER(u32)]
    L.akz_extract_gray_f32.argtypes = [vp, vp, i32, i32, i32, vp, vp, u32, C.POINTER(u32)]
    L.akz_extract_color.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp, u32, C.POINTER(u32)]
    L.akz_extract_batch.argtypes = [vp, C.POINTER(vp), i32, i32, i32, i32, i32, vp, vp, u32, vp]
    L.akz_extract_batch_device.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, u32, vp, vp]
    L.akz_scale_space_device.argtypes = [vp, vp, i32, i32, i32, i32, vp]
    L.akz_sync.argtypes = [vp]
    L.akz_stream.restype = vp
    L.akz_stream.argtypes = [vp]
    L.akz_last_overflow.argtypes = [vp, C.POINTER(OverflowInfo), u32, C.POINTER(u32)]
    L.akz_num_levels.argtypes = [vp, i32, i32, C.POINTER(i32)]
    L.akz_level.argtypes = [vp, i32, i32, i32, C.POINTER(LevelInfo)]
    L.akz_fed_tau.argtypes = [vp, i32, i32, i32, vp, u32, C.POINTER(u32)]
    L.akz_debug_get_level.argtypes = [vp, i32, i32, i32, vp]
    L.akz_debug_get_contrast.argtypes = [vp, i32, C.POINTER(C.c_double)]
    L.akz_debug_get_keypoints.argtypes = [vp, i32, i32, vp, u32, C.POINTER(u32)]
    L.akz_debug_portable_math.argtypes = [vp, i32, vp, vp, u32, vp]
    L.akz_debug_orientation_masks.argtypes = [vp, vp, vp, u32, vp, vp, vp]
    L.akz_gaussian_kernel.argtypes = [C.c_float, u32, vp]
    L.akz_horizontal_filter.argtypes = [vp, vp, i32, i32, vp, u32, vp]
    L.akz_vertical_filter.argtypes = [vp, vp, i32, i32, vp, u32, vp]
    L.akz_half_size.argtypes = [vp, vp, i32, i32, vp]
    L.akz_sample_colors_rgb8.argtypes = [vp, vp, i32, i32, i32, vp, u32, vp]
    L.akz_sample_colors_batch_device.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, u32, vp, vp]
    L.hm_create.argtypes = [i32, u32, u32, C.POINTER(vp)]
    L.hm_create_ex.argtypes = [i32, u32, u32, u32, C.POINTER(vp)]
    L.hm_destroy.argtypes = [vp]
    L.hm_knn2.argtypes = [vp, vp, u32, vp, u32, vp]
    L.hm_knn.argtypes = [vp, vp, u32, vp, u32, u32, vp]
    L.hm_knn_views_device.argtypes = [vp, vp, vp, vp, vp, u32, vp, u32, u32, vp, vp]
    L.hm_knn_batch_device.argtypes = [vp, vp, vp, vp, vp, u32, vp, vp, u32, u32, vp, vp]
    L.hm_best_of_views_batch_device.argtypes = [vp, vp, vp, vp, u32, vp, u32, u32, u32, vp, vp, u32, vp, vp, vp]
    L.hm_best_of_views_device.argtypes = [vp, vp, vp, u32, vp, u32, u32, vp, vp, u32, vp, vp, vp]
    L.hm_set_targets.argtypes = [vp, vp, u32]
    L.hm_knn_targets.argtypes = [vp, vp, u32, u32, vp]
    L.hm_landmark_pairs_batch_device.argtypes = [vp, vp, vp, vp, vp, u32, u32, vp, u32, vp, vp, vp]
    L.hm_landmark_matches_batch_device.argtypes = [vp, vp, vp, vp, vp, vp, u32, u32, vp, u32, vp, vp, vp]
    L.hm_landmark_matches_ordered_batch_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, u32, u32, vp, u32, vp, vp, vp]
    L.hm_landmark_original_matches_batch_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, u32, u32, u32, vp, vp, vp]
    L.hm_match.argtypes = [vp, vp, u32, vp, u32, i32, u32, C.c_float, i32, vp, u32, C.POINTER(u32)]
    L.hm_match_batch_device.argtypes = [vp, vp, vp, vp, vp, u32, vp, vp, u32, i32, u32, C.c_float, i32, vp, vp, vp]
    L.hm_sync.argtypes = [vp]
    L.hm_hash_bag.argtypes = [vp, vp, u32, vp, u32, vp, vp]
    L.hm_hash_bag_device.argtypes = [vp, vp, vp, u32, u32, vp, u32, vp, vp, vp]
    L.hm_hash_knn.argtypes = [vp, vp, vp, u32, u32, u32, vp, C.POINTER(u32)]
    L.hm_timing_enable.argtypes = [vp, i32]
    L.hm_timing_get.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64), i32]
    L.hm_stream.restype = vp
    L.hm_stream.argtypes = [vp]
    L.rs_create.argtypes = [i32, u32, u32, C.POINTER(vp)]
    L.rs_destroy.argtypes = [vp]
    L.rs_calibrate.argtypes = [vp, i32, C.c_double, vp, u32, vp]
    L.rs_essential_batch.argtypes = [vp, vp, vp, u32, vp, u32, C.c_double, vp, C.POINTER(u32), vp, u32, C.POINTER(u32)]
    L.rs_five_point_batch.argtypes = L.rs_essential_batch.argtypes
    L.rs_debug_essentials.argtypes = [vp, vp, vp, u32]
    L.rs_essential_arrsac.argtypes = [vp, vp, vp, u32, vp, C.POINTER(ArrsacParams), vp, C.POINTER(u32), vp, u32, C.POINTER(u32),
                                      C.POINTER(ArrsacStats)]
    L.rs_p3p_arrsac.argtypes = L.rs_essential_arrsac.argtypes
    L.rs_arrsac_samples.argtypes = [C.c_uint64, u32, u32, u32, vp]
    L.rs_p3p_batch.argtypes = [vp, vp, vp, u32, vp, u32, C.c_double, vp, C.POINTER(u32), vp, u32, C.POINTER(u32)]
    L.rs_debug_counts.argtypes = [vp, vp, u32]
    L.rs_debug_poses.argtypes = [vp, vp, vp, u32]
    L.rs_batch_reserve.argtypes = [vp, u32]
    L.rs_essential_arrsac_batch_device.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, u32, C.POINTER(Camera), C.POINTER(Camera),
                                                   C.POINTER(ArrsacParams), u32, vp, vp, vp, vp, vp, vp]
    L.rs_p3p_arrsac_batch_device.argtypes = [vp, vp, u32, vp, vp, vp, u32, vp, u32, C.POINTER(Camera), C.POINTER(ArrsacParams), u32,
                                             vp, vp, vp, vp, vp, vp]
    L.rs_debug_scene_world.argtypes = [vp, u32, C.POINTER(u32), vp, vp, vp, u32]
    L.rs_sync.argtypes = [vp]
    L.rs_stream.restype = vp
    L.rs_stream.argtypes = [vp]
    L.rs_debug_scene.argtypes = [vp, u32, C.POINTER(u32), vp, vp, vp, u32]
    L.rs_debug_residuals.argtypes = [vp, vp, u32, vp, vp, u32, i32, vp]
    L.rs_debug_far.argtypes = [vp, vp, u32, vp, vp, u32, C.c_double, vp]
    tp = C.POINTER(TriangulateParams)
    L.rs_triangulate_params_default.argtypes = [tp]
    L.rs_triangulate_observations.argtypes = [vp, vp, vp, u32, tp, vp, vp]
    L.rs_triangulate_landmarks_device.argtypes = [vp, vp, u32, u32, vp, C.POINTER(Camera), vp, vp, u32, u32, tp, vp, vp, vp]
    L.rs_triangulate_merged_device.argtypes = [vp, vp, u32, u32, vp, C.POINTER(Camera), vp, vp, u32, u32, tp, vp, vp, vp, u32, u32,
                                               vp, vp, vp]
    L.rs_triangulate_pairs_batch_device.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, u32, C.POINTER(Camera), C.POINTER(Camera),
                                                    vp, vp, vp, vp, tp, vp, vp, vp]
    L.rs_three_view_params_default.argtypes = [C.POINTER(ThreeViewParams)]
    L.rs_three_view_init_batch_device.argtypes = [vp, vp, u32, u32, vp, vp, vp, C.POINTER(Camera), vp, vp, vp, vp, vp, vp, vp, vp, u32,
                                                  C.POINTER(ThreeViewParams), vp, vp, vp, vp, vp, vp, vp]
    L.rs_three_view_constraint_params_default.argtypes = [C.POINTER(ThreeViewConstraintParams)]
    L.rs_three_view_constraint_batch_device.argtypes = [vp, vp, u32, u32, vp, C.POINTER(Camera), vp, vp, vp, u32, u32,
                                                        C.POINTER(ThreeViewConstraintParams), vp, vp, vp, vp]
    L.rs_pose_graph_params_default.argtypes = [C.POINTER(PoseGraphParams)]
    L.rs_pose_graph_edges_device.argtypes = [vp, vp, vp, vp, u32, vp, vp]
    L.rs_pose_graph_relax_batch_device.argtypes = [vp, vp, u32, vp, u32, vp, vp, u32, vp, vp, vp, u32, C.POINTER(PoseGraphParams),
                                                   vp, vp, vp, vp]
    L.rs_pose_graph_debug_resident_views.argtypes = [vp, u32]
    ofp = C.POINTER(ObservationFilterParams)
    L.rs_observation_filter_params_default.argtypes = [ofp]
    L.rs_filter_observations_device.argtypes = [vp, vp, u32, u32, vp, C.POINTER(Camera), vp, vp, u32, u32, vp, vp, u32, vp, ofp] + [vp] * 11
    L.rs_optimize_reconstruction_batch_device.argtypes = ([vp, vp, u32, vp, u32, vp, vp, u32, vp, vp, vp, u32, C.POINTER(PoseGraphParams),
                                                           vp, u32, C.POINTER(Camera), vp, vp, u32, u32, vp, ofp] + [vp] * 17)
    svp = C.POINTER(SingleViewParams)
    L.rs_single_view_params_default.argtypes = [svp]
    L.rs_refine_poses_batch_device.argtypes = ([vp, vp, u32, u32, vp, C.POINTER(Camera), vp, vp, u32, u32, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp,
                                                u32, svp] + [vp] * 6)
    cvp = C.POINTER(CovisibilityParams)
    L.rs_covisibility_params_default.argtypes = [cvp]
    L.rs_covisibility_candidates_device.argtypes = [vp, vp, vp, u32, u32, u32, u32, vp, vp, u32, cvp] + [vp] * 7
    L.rs_covisibility_record_device.argtypes = [vp, vp, vp, u32, vp, u32, cvp, vp, vp, vp, vp]
    L.rs_pose_graph_rows_device.argtypes = [vp, vp, u32, u32, vp, vp, vp, vp]
    L.rs_landmarks_sharing_view_device.argtypes = [vp, vp, vp, u32, u32, vp, vp, u32, u32, vp, vp]
    L.rs_add_views_device.argtypes = [vp, vp, vp, u32, u32, u32, vp, vp, u32, u32, u32, vp, u32] + [vp] * 8 + [u32, u32] + [vp] * 10
    L.rs_merge_map_device.argtypes = [vp, vp, vp, vp, vp, u32, u32, u32, u32, vp, vp, u32, u32, vp, vp, vp]
    L.rs_incorporate_reconstruction_device.argtypes = ([vp, vp, vp, u32, u32, vp, vp, u32, u32, vp, vp, u32, u32, u32, vp, u32, u32, vp, vp, u32, u32] +
                                                       [vp] * 9)
    L.rs_normalize_reconstruction_device.argtypes = [vp, vp, u32, vp, vp, u32, u32, vp, u32, vp, vp, u32, vp, vp, vp]
    L.rs_export_reconstruction_device.argtypes = [vp, vp, u32, vp, vp, u32, u32, vp, vp, u32, vp, vp, u32, u32, vp, u32, vp, vp, vp, vp, vp, vp, vp]
    L.rs_write_ply.argtypes = [C.c_char_p, vp, vp, u32, u32, i32]
    L.rs_join_pairs_batch_device.argtypes = [vp] * 7 + [u32, u32, vp, vp, u32, u32, u32, C.c_uint64] + [vp] * 10
    L.rs_add_reconstruction_batch_device.argtypes = ([vp] * 15 + [u32, vp, vp, u32, u32, vp, vp, vp, u32, u32, vp, vp, u32, vp, vp, vp, u32, u32, u32, u32] +
                                                     [vp] * 14)
    L.hm_place_params_default.argtypes = [C.POINTER(PlaceParams)]
    L.hm_place_room.restype = u32
    L.hm_place_room.argtypes = [C.POINTER(PlaceParams)]
    L.hm_find_frames_batch_device.argtypes = [vp] * 6 + [u32, u32, vp, vp, u32, C.POINTER(PlaceParams), u32] + [vp] * 9
    L.hm_view_plan_device.argtypes = [vp] * 6 + [u32, vp] + [u32] * 5 + [vp] * 5
    L.hm_knn_planned_batch_device.argtypes = [vp] * 5 + [u32, vp, vp, vp] + [u32] * 5 + [vp, vp]
    L.hm_best_of_views_planned_batch_device.argtypes = [vp] * 4 + [u32, vp, vp] + [u32] * 4 + [vp, vp, u32, vp, vp, vp]
    L.rs_repack_table_device.argtypes = [vp, vp, vp, u32, u32, u32, u32, vp, u32, vp, u32, u32, u32] + [vp] * 9
    L.rs_gather_blocks_device.argtypes = [vp, vp, vp, u32, u32, vp, u32, vp, vp]
    L.rs_repack_constraints_device.argtypes = [vp, vp, vp, vp, u32, vp, u32, u32, vp, u32] + [vp] * 6
    L.hm_place_remap_views_device.argtypes = [vp, vp, vp, u32, u32, vp, u32, vp, vp]
    L.akz_comm_unique_id.argtypes = [vp]
    L.akz_comm_create.argtypes = [vp, i32, i32, i32, C.POINTER(vp)]
    L.akz_comm_destroy.argtypes = [vp]
    L.akz_comm_shift_blocks.argtypes = [vp, vp, vp, u32, u32, vp, vp, vp]
    L.akz_comm_allgather_blocks.argtypes = [vp, vp, vp, u32, u32, vp, vp, vp]
    L.akz_comm_sync.argtypes = [vp]
    L.akz_comm_stream.restype = vp
    L.akz_comm_stream.argtypes = [vp]
    L.akz_comm_rank.argtypes = [vp]
    L.akz_comm_world.argtypes = [vp]
    L.akz_comm_timing.argtypes = [vp, i32, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), i32]
    L.akz_comm_last_error_string.restype = C.c_char_p
    L.akz_timing_enable.argtypes = [vp, i32]
    L.akz_timing_reset.argtypes = [vp]
    L.akz_timing_get.argtypes = [vp, i32, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    _lib = L
    return L


def check(status, what=""):
    if status != 0:
        raise AkzError(status, what)


STREAM_LEGACY = 1   # include/akz.h AKZ_STREAM_LEGACY (= hipStreamLegacy)


def wait_handle(stream):
    """The `stream_to_wait` argument for a torch stream: its handle, or AKZ_STREAM_LEGACY for the legacy default stream —
    whose handle is 0, which the ABI reads as "nothing to wait for" (the library's streams are non-blocking: they do not
    synchronise with the default stream by themselves)."""
    h = stream.cuda_stream
    return h if h else STREAM_LEGACY


def params(struct_type, default_symbol, **kw):
    """A parameter struct of the ABI with the defaults its `*_params_default` symbol gives and `kw` on top; struct_size or
    an unknown name raises TypeError."""
    p = struct_type()
    check(getattr(lib(), default_symbol)(C.byref(p)), default_symbol)
    c_name = default_symbol[:-len("_default")]
    for k, v in kw.items():
        if k == "struct_size" or not hasattr(p, k):
            raise TypeError(f"{c_name} has no setting {k!r}")
        setattr(p, k, v)
    return p


def stat_f64(stats, at):
    """the float64 that the two u32 stats words at `at` (low, high) hold"""
    return float(stats[at:at + 2].copy().view(np.float64)[0])


def device_bytes(torch, a, dev):
    """A host array as a flat uint8 tensor on `dev`; an empty one as 8 zero bytes, so that it still has an address."""
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return torch.zeros(8, dtype=torch.uint8, device=dev)
    return torch.from_numpy(a.view(np.uint8).reshape(-1)).to(dev)
