"""ctypes binding of include/ndt2d_hip.h (libndt2d_hip.so).

This is the only place the package touches native code.  Importing it fails
loudly if the HIP extension has not been built -- there is no Python or CPU
fallback for any compute entry point.
"""
import ctypes as C
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
# NDT2D_HIP_LIB selects another build of the same library (A/B timing of kernels)
LIB_PATH = os.environ.get("NDT2D_HIP_LIB") or os.path.join(_PKG, "libndt2d_hip.so")

OK = 0
ERR_INVALID = 1
ERR_NO_GRID = 2
ERR_HIP = 3
ERR_NO_DEVICE = 4
ERR_STATE = 5
ERR_ALLOC = 6
ERR_INTERNAL = 7
NO_INDEX = (1 << 64) - 1
# NDT2D_REFINE_*: how a Newton registration job stopped
REFINE_CONVERGED, REFINE_MAX_EVALS, REFINE_STALLED, REFINE_NO_OVERLAP, REFINE_NOT_FINITE = range(5)
REFINE_STATUS_NAMES = ("converged", "max_evals", "stalled", "no_overlap", "not_finite")
# NDT2D_BEAM_*: the class of a beam (the two low bits of its byte) and the pierced bit; the record of a job
BEAM_OFF, BEAM_UNSEEN, BEAM_OUTLIER, BEAM_INLIER = range(4)
BEAM_PIERCED = 4
VERIFY_RECORD_U32 = 8
VERIFY_NO_CELL = 0xFFFFFFFF
# NDT2D_POSEGRAPH_*: how a pose-graph job stopped; the doubles of its record
POSEGRAPH_CONVERGED_GRADIENT, POSEGRAPH_CONVERGED_COST, POSEGRAPH_CONVERGED_STEP, POSEGRAPH_MAX_ITERATIONS, POSEGRAPH_FAILED = range(5)
POSEGRAPH_STATUS_NAMES = ("converged_gradient", "converged_cost", "converged_step", "max_iterations", "failed")
POSEGRAPH_RECORD_DOUBLES = 6
# NDT2D_MARGINALS_*: how a query of the marginal covariances ended; the doubles of its record
MARGINALS_CONVERGED, MARGINALS_CG_CAP, MARGINALS_BREAKDOWN, MARGINALS_NOT_FREE = range(4)
MARGINALS_STATUS_NAMES = ("converged", "cg_cap", "breakdown", "not_free")
MARGINALS_RECORD_DOUBLES = 5
# NDT2D_COVARIANCE_*: how a job of the dense covariance ended; the doubles of its record
COVARIANCE_OK, COVARIANCE_NOT_POSITIVE_DEFINITE = range(2)
COVARIANCE_STATUS_NAMES = ("ok", "not_positive_definite")
COVARIANCE_RECORD_DOUBLES = 3
# the doubles of a direct solve's record (its status values are POSEGRAPH_*)
DIRECT_RECORD_DOUBLES = 8
MATCH_RECORD_DOUBLES = 12
POSE_STATS_DOUBLES = 8
PF_RESULT_DOUBLES = 8

_ERR_NAMES = {1: "NDT2D_ERR_INVALID", 2: "NDT2D_ERR_NO_GRID", 3: "NDT2D_ERR_HIP",
              4: "NDT2D_ERR_NO_DEVICE", 5: "NDT2D_ERR_STATE", 6: "NDT2D_ERR_ALLOC", 7: "NDT2D_ERR_INTERNAL"}


class Ndt2dError(RuntimeError):
    def __init__(self, code, where, detail=""):
        self.code = code
        super().__init__("%s failed: %s%s" % (where, _ERR_NAMES.get(code, str(code)),
                                               (" (" + detail + ")") if detail else ""))


class MatchResult(C.Structure):
    _fields_ = [("best_score", C.c_double), ("best_index", C.c_uint64),
                ("acc", C.c_double * 10), ("n_candidates", C.c_uint64), ("near_tie", C.c_uint64)]


class LaserScan(C.Structure):
    """ndt2d_laser_scan"""
    _fields_ = [("angle_min", C.c_float), ("angle_increment", C.c_float),
                ("range_max", C.c_double), ("inverted", C.c_int),
                ("laser_x", C.c_double), ("laser_y", C.c_double), ("laser_theta", C.c_double),
                ("motion_x", C.c_double), ("motion_y", C.c_double), ("motion_theta", C.c_double)]


class OccupancyInfo(C.Structure):
    """ndt2d_occupancy_info"""
    _fields_ = [("resolution", C.c_double), ("width", C.c_uint32), ("height", C.c_uint32),
                ("origin_x", C.c_double), ("origin_y", C.c_double)]


class OccmapResult(C.Structure):
    """ndt2d_occmap_result"""
    _fields_ = [("info", OccupancyInfo), ("mode", C.c_int), ("beams_traced", C.c_uint64),
                ("rect_x0", C.c_uint32), ("rect_y0", C.c_uint32), ("rect_w", C.c_uint32),
                ("rect_h", C.c_uint32)]


OCCMAP_FULL = 0
OCCMAP_INCREMENTAL = 1
OCCMAP_UNCHANGED = 2


class ClusterHeader(C.Structure):
    """ndt2d_cluster_header"""
    _fields_ = [("n", C.c_uint64), ("n_left_out", C.c_uint64), ("n_bins", C.c_uint64),
                ("n_clusters", C.c_uint64), ("rounds", C.c_uint64), ("w_total", C.c_double)]


class ClusterRecord(C.Structure):
    """ndt2d_cluster_record"""
    _fields_ = [("label", C.c_uint32), ("count", C.c_uint32), ("mass", C.c_double), ("weight", C.c_double),
                ("mean_x", C.c_double), ("mean_y", C.c_double), ("mean_theta", C.c_double),
                ("cxx", C.c_double), ("cxy", C.c_double), ("cyy", C.c_double), ("var_theta", C.c_double)]


CLUSTER_MAX_RECORDS = 16
CLEARANCE_FAR = 0xFFFFFFFF      # NDT2D_CLEARANCE_FAR


class World(C.Structure):
    _fields_ = [("room_half", C.c_double), ("pillar_pitch", C.c_double),
                ("pillar_half", C.c_double)]


_dp = C.POINTER(C.c_double)
_vp = C.c_void_p
_d = C.c_double
_sz = C.c_size_t
_u64 = C.c_uint64
_u32 = C.c_uint32
_szp = C.POINTER(C.c_size_t)

# name -> (restype, argtypes); one entry per function declared in ndt2d_hip.h
SIGNATURES = {
    "ndt2d_abi_version": (C.c_int, []),
    "ndt2d_build_info": (C.c_char_p, []),
    "ndt2d_create": (C.c_int, [C.POINTER(_vp), C.c_int]),
    "ndt2d_destroy": (C.c_int, [_vp]),
    "ndt2d_last_error": (C.c_char_p, [_vp]),
    "ndt2d_set_stream": (C.c_int, [_vp, _vp]),
    "ndt2d_get_stream": (_vp, [_vp]),
    "ndt2d_device_id": (C.c_int, [_vp]),
    "ndt2d_set_grid": (C.c_int, [_vp, _dp, _u32, _u32, _d, _d, _d]),
    "ndt2d_set_grid_sparse": (C.c_int, [_vp, C.POINTER(C.c_uint32), _dp, _sz, _u32, _u32, _d, _d, _d]),
    "ndt2d_build_grid": (C.c_int, [_vp, _d, _d, _dp, _dp, _szp, _sz]),
    "ndt2d_build_grid_small": (C.c_int, [_vp, _d, _d, _dp, _dp, _szp, _sz]),
    "ndt2d_build_grid_small_fits": (C.c_int, [_d, _d, _dp, _sz, _sz]),
    "ndt2d_build_small_max_points": (_sz, []),
    "ndt2d_build_small_set_eigenvalue_form": (C.c_int, [_vp, C.c_char_p]),
    "ndt2d_build_small_last_error": (C.c_char_p, [_vp]),
    "ndt2d_build_small_release": (C.c_int, [_vp]),
    "ndt2d_scanstore_set_eigenvalue_form": (C.c_int, [_vp, C.c_char_p]),
    "ndt2d_scanstore_create": (C.c_int, [_vp, _sz, _sz, C.POINTER(_vp)]),
    "ndt2d_scanstore_destroy": (C.c_int, [_vp]),
    "ndt2d_scanstore_last_error": (C.c_char_p, [_vp]),
    "ndt2d_scanstore_append": (C.c_int, [_vp, _dp, _sz, _szp]),
    "ndt2d_scanstore_count": (C.c_int, [_vp, _szp]),
    "ndt2d_scanstore_reset": (C.c_int, [_vp]),
    "ndt2d_scanstore_build": (C.c_int, [_vp, _szp, _dp, _sz, _d, _d]),
    "ndt2d_closure_create": (C.c_int, [_vp, _vp, _sz, C.POINTER(_vp)]),
    "ndt2d_closure_destroy": (C.c_int, [_vp]),
    "ndt2d_closure_last_error": (C.c_char_p, [_vp]),
    "ndt2d_closure_match": (C.c_int, [_vp, _sz, _szp, _szp, _dp, _d, _d, _dp, _sz, _d, _d, _dp, _dp, _dp, _sz,
                                     _dp, _sz, _dp, _dp]),
    "ndt2d_closure_refine": (C.c_int, [_vp, _sz, _szp, _szp, _dp, _d, _d, _dp, C.POINTER(_u32), C.POINTER(_u32), _sz, _dp, _szp, _sz,
                                       _u32, _d, _d, _dp]),
    "ndt2d_closure_set_neighbourhood": (C.c_int, [_vp, _u32]),
    "ndt2d_closure_neighbourhood": (C.c_int, [_vp, C.POINTER(_u32)]),
    "ndt2d_closure_verify": (C.c_int, [_vp, _sz, _szp, _szp, _dp, _d, _d, _dp, C.POINTER(_u32), C.POINTER(_u32), _sz, _dp, _szp, _sz,
                                       C.POINTER(_u32), C.POINTER(C.c_uint8), _dp, C.POINTER(_u32)]),
    "ndt2d_closure_set_verify_neighbourhood": (C.c_int, [_vp, _u32]),
    "ndt2d_closure_verify_neighbourhood": (C.c_int, [_vp, C.POINTER(_u32)]),
    "ndt2d_closure_set_verify_gates": (C.c_int, [_vp, _d, _d]),
    "ndt2d_closure_verify_gates": (C.c_int, [_vp, _dp, _dp]),
    "ndt2d_closure_set_verify_rays": (C.c_int, [_vp, C.c_int]),
    "ndt2d_closure_verify_rays": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "ndt2d_closure_set_timing": (C.c_int, [_vp, C.c_int]),
    "ndt2d_closure_last_ms": (C.c_int, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "ndt2d_grid_view_get": (C.c_int, [_vp, _vp]),
    "ndt2d_starts_create": (C.c_int, [_vp, _sz, C.POINTER(_vp)]),
    "ndt2d_starts_destroy": (C.c_int, [_vp]),
    "ndt2d_starts_last_error": (C.c_char_p, [_vp]),
    "ndt2d_starts_match": (C.c_int, [_vp, _dp, _sz, _dp, _sz, _dp, _sz, _dp, _sz, _dp, _dp]),
    "ndt2d_starts_set_timing": (C.c_int, [_vp, C.c_int]),
    "ndt2d_starts_last_ms": (C.c_int, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "ndt2d_wide_create": (C.c_int, [_vp, _sz, C.POINTER(_vp)]),
    "ndt2d_wide_destroy": (C.c_int, [_vp]),
    "ndt2d_wide_last_error": (C.c_char_p, [_vp]),
    "ndt2d_wide_set_tile": (C.c_int, [_vp, _u32, _u32]),
    "ndt2d_wide_tile": (C.c_int, [_vp, C.POINTER(_u32), C.POINTER(_u32)]),
    "ndt2d_wide_match": (C.c_int, [_vp, _dp, _dp, _sz, _dp, _sz, _dp, _sz, C.c_int, _dp, C.POINTER(_u64), _dp,
                                   C.POINTER(C.c_uint8)]),
    "ndt2d_wide_read_image": (C.c_int, [_vp, _dp, _dp, _sz]),
    "ndt2d_wide_set_timing": (C.c_int, [_vp, C.c_int]),
    "ndt2d_wide_last_ms": (C.c_int, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                     C.POINTER(C.c_float)]),
    "ndt2d_scans_create": (C.c_int, [_vp, _sz, C.POINTER(_vp)]),
    "ndt2d_scans_destroy": (C.c_int, [_vp]),
    "ndt2d_scans_last_error": (C.c_char_p, [_vp]),
    "ndt2d_scans_match": (C.c_int, [_vp, _dp, C.POINTER(_u32), _sz, _dp, _szp, _sz, _dp, _sz, _dp, _sz, _dp, _dp]),
    "ndt2d_scans_set_timing": (C.c_int, [_vp, C.c_int]),
    "ndt2d_scans_last_ms": (C.c_int, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "ndt2d_refine_create": (C.c_int, [_vp, _sz, C.POINTER(_vp)]),
    "ndt2d_refine_destroy": (C.c_int, [_vp]),
    "ndt2d_refine_last_error": (C.c_char_p, [_vp]),
    "ndt2d_refine_run": (C.c_int, [_vp, _dp, C.POINTER(_u32), _sz, _dp, _szp, _sz, _u32, _d, _d, _dp]),
    "ndt2d_refine_set_timing": (C.c_int, [_vp, C.c_int]),
    "ndt2d_refine_last_ms": (C.c_int, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "ndt2d_refine_set_neighbourhood": (C.c_int, [_vp, _u32]),
    "ndt2d_refine_neighbourhood": (C.c_int, [_vp, C.POINTER(_u32)]),
    "ndt2d_refine_covariance": (C.c_int, [_dp, _dp]),
    "ndt2d_verify_create": (C.c_int, [_vp, _sz, C.POINTER(_vp)]),
    "ndt2d_verify_destroy": (C.c_int, [_vp]),
    "ndt2d_verify_last_error": (C.c_char_p, [_vp]),
    "ndt2d_verify_run": (C.c_int, [_vp, _dp, C.POINTER(_u32), _sz, _dp, _szp, _sz, C.POINTER(_u32), C.POINTER(C.c_uint8), _dp,
                                   C.POINTER(_u32)]),
    "ndt2d_verify_set_neighbourhood": (C.c_int, [_vp, _u32]),
    "ndt2d_verify_neighbourhood": (C.c_int, [_vp, C.POINTER(_u32)]),
    "ndt2d_verify_set_gates": (C.c_int, [_vp, _d, _d]),
    "ndt2d_verify_gates": (C.c_int, [_vp, _dp, _dp]),
    "ndt2d_verify_set_rays": (C.c_int, [_vp, C.c_int]),
    "ndt2d_verify_rays": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "ndt2d_verify_set_timing": (C.c_int, [_vp, C.c_int]),
    "ndt2d_verify_last_ms": (C.c_int, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "ndt2d_posegraph_create": (C.c_int, [_vp, _sz, _sz, _sz, C.POINTER(_vp)]),
    "ndt2d_posegraph_destroy": (C.c_int, [_vp]),
    "ndt2d_posegraph_last_error": (C.c_char_p, [_vp]),
    "ndt2d_posegraph_set_graph": (C.c_int, [_vp, _dp, _sz, C.POINTER(_u32), C.POINTER(_u32), _dp, _dp, _sz, _sz]),
    "ndt2d_posegraph_set_weighting": (C.c_int, [_vp, C.c_char_p]),
    "ndt2d_posegraph_weighting": (C.c_char_p, [_vp]),
    "ndt2d_pose_graph_set_preconditioner": (C.c_int, [_vp, C.c_char_p]),
    "ndt2d_pose_graph_preconditioner": (C.c_char_p, [_vp]),
    "ndt2d_posegraph_evaluate": (C.c_int, [_vp, C.POINTER(C.c_uint8), _sz, _dp, _dp, _dp]),
    "ndt2d_posegraph_solve": (C.c_int, [_vp, C.POINTER(C.c_uint8), _sz, _u32, _d, _d, _d, _dp, _dp, _dp]),
    "ndt2d_posegraph_set_timing": (C.c_int, [_vp, C.c_int]),
    "ndt2d_posegraph_last_ms": (C.c_int, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "ndt2d_robust_rho": (C.c_int, [C.c_char_p, _d, _d, _dp]),
    "ndt2d_robust_set_loss": (C.c_int, [_vp, C.c_char_p, _d]),
    "ndt2d_robust_loss": (C.c_char_p, [_vp, _dp]),
    "ndt2d_robust_select": (C.c_int, [_vp, C.POINTER(C.c_uint8), _sz]),
    "ndt2d_marginals_columns": (C.c_int, [_vp, C.POINTER(C.c_uint8), _sz, _dp, C.POINTER(_u32), _sz, _d, _d, _u32, _dp, _dp, _dp]),
    "ndt2d_marginals_relative": (C.c_int, [_dp, _dp, _dp, _dp, _dp]),
    "ndt2d_marginals_distance": (C.c_int, [_dp, _dp, _dp, _dp, _dp]),
    "ndt2d_covariance_create": (C.c_int, [_vp, _sz, C.POINTER(_vp)]),
    "ndt2d_covariance_destroy": (C.c_int, [_vp]),
    "ndt2d_covariance_last_error": (C.c_char_p, [_vp]),
    "ndt2d_covariance_compute": (C.c_int, [_vp, C.POINTER(C.c_uint8), _sz, _dp, _d, C.POINTER(_u32), _sz, _dp, _dp, _dp]),
    "ndt2d_covariance_set_timing": (C.c_int, [_vp, C.c_int]),
    "ndt2d_covariance_last_ms": (C.c_int, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "ndt2d_direct_create": (C.c_int, [_vp, _sz, C.POINTER(_vp)]),
    "ndt2d_direct_destroy": (C.c_int, [_vp]),
    "ndt2d_direct_last_error": (C.c_char_p, [_vp]),
    "ndt2d_direct_solve": (C.c_int, [_vp, C.POINTER(C.c_uint8), _sz, _u32, _d, _d, _d, _dp, _dp, _dp]),
    "ndt2d_direct_set_timing": (C.c_int, [_vp, C.c_int]),
    "ndt2d_direct_last_ms": (C.c_int, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "ndt2d_sparse_create": (C.c_int, [_vp, _sz, C.POINTER(_vp)]),
    "ndt2d_sparse_destroy": (C.c_int, [_vp]),
    "ndt2d_sparse_last_error": (C.c_char_p, [_vp]),
    "ndt2d_sparse_solve": (C.c_int, [_vp, C.POINTER(C.c_uint8), _sz, _u32, _d, _d, _d, _dp, _dp, _dp]),
    "ndt2d_sparse_layout": (C.c_int, [_vp, C.POINTER(_sz), C.POINTER(_sz)]),
    "ndt2d_sparse_set_timing": (C.c_int, [_vp, C.c_int]),
    "ndt2d_sparse_last_ms": (C.c_int, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "ndt2d_sparsecov_create": (C.c_int, [_vp, _sz, C.POINTER(_vp)]),
    "ndt2d_sparsecov_destroy": (C.c_int, [_vp]),
    "ndt2d_sparsecov_last_error": (C.c_char_p, [_vp]),
    "ndt2d_sparsecov_compute": (C.c_int, [_vp, C.POINTER(C.c_uint8), _sz, _dp, _d, C.POINTER(_u32), _sz, _dp, _dp, _dp]),
    "ndt2d_sparsecov_set_timing": (C.c_int, [_vp, C.c_int]),
    "ndt2d_sparsecov_last_ms": (C.c_int, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "ndt2d_set_eigenvalue_form": (C.c_int, [_vp, C.c_char_p]),
    "ndt2d_get_grid": (C.c_int, [_vp, _dp, _sz, C.POINTER(_u32), C.POINTER(_u32), _dp, _dp, _dp]),
    "ndt2d_clear_grid": (C.c_int, [_vp]),
    "ndt2d_has_grid": (C.c_int, [_vp]),
    "ndt2d_set_beams": (C.c_int, [_vp, _dp, _sz]),
    "ndt2d_set_search": (C.c_int, [_vp, _d, _d, _dp, _dp, _dp, _sz, _dp, _sz]),
    "ndt2d_set_search_beams": (C.c_int, [_vp, _dp, _sz, _d, _d, _dp, _dp, _dp, _sz, _dp, _sz]),
    "ndt2d_match_launch": (C.c_int, [_vp, _sz, _sz, _vp, _vp]),
    "ndt2d_match_launch_strided": (C.c_int, [_vp, _sz, _sz, _sz, _vp, _vp]),
    "ndt2d_match_fetch": (C.c_int, [_vp, C.POINTER(MatchResult)]),
    "ndt2d_match": (C.c_int, [_vp, _sz, _sz, _dp, C.POINTER(MatchResult)]),
    "ndt2d_score_poses_launch": (C.c_int, [_vp, _vp, _sz, _vp, _vp]),
    "ndt2d_score_poses": (C.c_int, [_vp, _dp, _sz, _dp, _dp]),
    "ndt2d_score_poses_beams": (C.c_int, [_vp, _dp, _sz, _dp, _sz, _dp]),
    "ndt2d_grid_stage_begin": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _sz, C.POINTER(C.POINTER(C.c_uint32)),
                                         C.POINTER(C.POINTER(C.c_double))]),
    "ndt2d_grid_stage_commit": (C.c_int, [_vp, _sz, _d, _d, _d]),
    "ndt2d_score_poses_beams_launch": (C.c_int, [_vp, _dp, _sz, _dp, _sz]),
    "ndt2d_score_fetch": (C.c_int, [_vp, _dp]),
    "ndt2d_pf_finalize_launch": (C.c_int, [_vp, _vp, _sz, _vp, _vp, _vp]),
    "ndt2d_pose_sums_launch": (C.c_int, [_vp, _vp, _sz, _vp]),
    "ndt2d_pose_sums_fetch": (C.c_int, [_vp, _dp]),
    "ndt2d_pf_finalize_totals_launch": (C.c_int, [_vp, _vp, _sz, _vp, _dp]),
    "ndt2d_pf_result_read": (C.c_int, [_vp, _dp]),
    "ndt2d_pf_measure": (C.c_int, [_vp, _dp, _sz, _dp, _dp]),
    "ndt2d_pf_noise_launch": (C.c_int, [_vp, _u64, _u64, _u64, _sz, _vp]),
    "ndt2d_pf_motion_launch": (C.c_int, [_vp, _vp, _sz, _d, _d, _d, _dp, _vp, _u64, _u64, _u64]),
    "ndt2d_pf_init_launch": (C.c_int, [_vp, _vp, _sz, _d, _d, _d, _d, _d, _d, _vp, _u64, _u64,
                                       _u64]),
    "ndt2d_pose_moments_launch": (C.c_int, [_vp, _vp, _sz, _vp, _vp]),
    "ndt2d_pf_update": (C.c_int, [_vp, _dp, _sz, _d, _d, _d, _dp, C.POINTER(C.c_float), _u64,
                                  _u64, _dp, _dp]),
    "ndt2d_resampler_create": (C.c_int, [_vp, _sz, _sz, C.POINTER(_vp)]),
    "ndt2d_resampler_destroy": (C.c_int, [_vp]),
    "ndt2d_resampler_last_error": (C.c_char_p, [_vp]),
    "ndt2d_resample_uniforms_launch": (C.c_int, [_vp, _u64, _u64, _u64, _sz, _vp]),
    "ndt2d_resample_launch": (C.c_int, [_vp, _vp, _vp, _sz, _sz, _sz, _d, _d, _dp, _vp, _u64, _u64,
                                        _vp, _vp, _vp]),
    "ndt2d_resample_fetch": (C.c_int, [_vp, _szp]),
    "ndt2d_resampler_set_timing": (C.c_int, [_vp, C.c_int]),
    "ndt2d_resampler_cdf_ms": (C.c_int, [_vp, C.POINTER(C.c_float)]),
    "ndt2d_pf_resample": (C.c_int, [_vp, _dp, _dp, _sz, _sz, _sz, _d, _d, _dp, _dp, _sz,
                                    C.POINTER(_u32), _szp]),
    "ndt2d_convert_scan_launch": (C.c_int, [_vp, _vp, _sz, C.POINTER(LaserScan), _vp, _vp]),
    "ndt2d_convert_scan": (C.c_int, [_vp, C.POINTER(C.c_float), _sz, C.POINTER(LaserScan), _dp,
                                     _szp]),
    "ndt2d_set_beams_from_ranges": (C.c_int, [_vp, C.POINTER(C.c_float), _sz,
                                              C.POINTER(LaserScan), _sz, _szp, _szp]),
    "ndt2d_scan_points": (_vp, [_vp, _szp]),
    "ndt2d_occupancy_grid": (C.c_int, [_vp, _d, _d, _dp, _dp, _szp, _sz, _sz, _dp,
                                       C.POINTER(OccupancyInfo), _vp, _sz]),
    "ndt2d_occmap_create": (C.c_int, [_vp, _d, _d, C.POINTER(_vp)]),
    "ndt2d_occmap_destroy": (C.c_int, [_vp]),
    "ndt2d_occmap_last_error": (C.c_char_p, [_vp]),
    "ndt2d_occmap_append_scan": (C.c_int, [_vp, _dp, _sz, _szp]),
    "ndt2d_occmap_scan_count": (C.c_int, [_vp, _szp]),
    "ndt2d_occmap_reset": (C.c_int, [_vp]),
    "ndt2d_occmap_update": (C.c_int, [_vp, _dp, _sz, C.POINTER(OccmapResult)]),
    "ndt2d_occmap_read": (C.c_int, [_vp, _u32, _u32, _u32, _u32, _vp, _sz]),
    "ndt2d_occmap_bounds": (C.c_int, [_vp, _dp, _szp]),
    "ndt2d_occmap_device_map": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(OccupancyInfo)]),
    "ndt2d_seed_create": (C.c_int, [_vp, C.POINTER(_vp)]),
    "ndt2d_seed_destroy": (C.c_int, [_vp]),
    "ndt2d_seed_last_error": (C.c_char_p, [_vp]),
    "ndt2d_seed_set_map": (C.c_int, [_vp, _vp, _u32, _u32, _d, _d, _d, C.POINTER(_u32)]),
    "ndt2d_seed_set_map_device": (C.c_int, [_vp, _vp, _u32, _u32, _d, _d, _d, C.POINTER(_u32)]),
    "ndt2d_seed_free_count": (C.c_int, [_vp, _szp]),
    "ndt2d_seed_read_table": (C.c_int, [_vp, C.POINTER(_u32), _sz, _szp]),
    "ndt2d_seed_launch": (C.c_int, [_vp, _vp, _sz, _u64, _u64, _u64]),
    "ndt2d_seed_inject_launch": (C.c_int, [_vp, _vp, _sz, _d, _u64, _u64, _u64, _vp]),
    "ndt2d_seed_set_timing": (C.c_int, [_vp, C.c_int]),
    "ndt2d_seed_last_ms": (C.c_int, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "ndt2d_clearance_create": (C.c_int, [_vp, C.POINTER(_vp)]),
    "ndt2d_clearance_destroy": (C.c_int, [_vp]),
    "ndt2d_clearance_last_error": (C.c_char_p, [_vp]),
    "ndt2d_clearance_compute": (C.c_int, [_vp, _vp, _u32, _u32, C.c_int, C.c_int64]),
    "ndt2d_clearance_compute_device": (C.c_int, [_vp, _vp, _u32, _u32, C.c_int, C.c_int64]),
    "ndt2d_clearance_min_d2": (C.c_int, [_d, _d, C.c_int64, C.POINTER(_u32)]),
    "ndt2d_clearance_read": (C.c_int, [_vp, _u32, _u32, _u32, _u32, _vp, _sz]),
    "ndt2d_clearance_device": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_u32), C.POINTER(_u32)]),
    "ndt2d_clearance_mask": (C.c_int, [_vp, _u32, C.POINTER(_vp)]),
    "ndt2d_clearance_read_mask": (C.c_int, [_vp, _u32, _u32, _u32, _u32, _vp, _sz]),
    "ndt2d_clearance_set_timing": (C.c_int, [_vp, C.c_int]),
    "ndt2d_clearance_last_ms": (C.c_int, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "ndt2d_cluster_create": (C.c_int, [_vp, _sz, C.POINTER(_vp)]),
    "ndt2d_cluster_destroy": (C.c_int, [_vp]),
    "ndt2d_cluster_last_error": (C.c_char_p, [_vp]),
    "ndt2d_cluster_set_bins": (C.c_int, [_vp, _d, _d, C.c_int]),
    "ndt2d_cluster_set_max_clusters": (C.c_int, [_vp, C.c_int]),
    "ndt2d_cluster_launch": (C.c_int, [_vp, _vp, _vp, _sz]),
    "ndt2d_cluster_fetch": (C.c_int, [_vp, C.POINTER(ClusterHeader), C.POINTER(ClusterRecord), _sz, _szp]),
    "ndt2d_cluster_read_labels": (C.c_int, [_vp, C.POINTER(_u32), _sz]),
    "ndt2d_cluster_set_timing": (C.c_int, [_vp, C.c_int]),
    "ndt2d_cluster_last_ms": (C.c_int, [_vp, C.POINTER(C.c_float)]),
    "ndt2d_device_alloc": (C.c_int, [_vp, _sz, C.POINTER(_vp)]),
    "ndt2d_device_free": (C.c_int, [_vp, _vp]),
    "ndt2d_copy_to_device": (C.c_int, [_vp, _vp, _vp, _sz]),
    "ndt2d_copy_to_host": (C.c_int, [_vp, _vp, _vp, _sz]),
    "ndt2d_copy_to_device_async": (C.c_int, [_vp, _vp, _vp, _sz]),
    "ndt2d_copy_to_host_async": (C.c_int, [_vp, _vp, _vp, _sz]),
    "ndt2d_match_near_best": (C.c_int, [_vp, _sz, _sz, _d, C.POINTER(C.c_uint64), _sz, _szp,
                                        C.POINTER(MatchResult)]),
    "ndt2d_match_status": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "ndt2d_launch_history_ms": (C.c_int, [_vp, C.POINTER(C.c_float), _sz, _szp]),
    "ndt2d_host_alloc": (C.c_int, [_vp, _sz, C.POINTER(_vp)]),
    "ndt2d_host_free": (C.c_int, [_vp, _vp]),
    "ndt2d_set_timing": (C.c_int, [_vp, C.c_int]),
    "ndt2d_synchronize": (C.c_int, [_vp]),
    "ndt2d_last_launch_ms": (C.c_int, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "ndt2d_last_variant": (C.c_char_p, [_vp]),
    "ndt2d_set_variant": (C.c_int, [_vp, C.c_char_p]),
    "ndt2d_set_pipeline_pieces": (C.c_int, [_vp, C.c_int]),
    "ndt2d_last_pipeline_pieces": (C.c_int, [_vp]),
    "ndt2d_matcher_create": (C.c_int, [C.POINTER(_vp), C.c_int]),
    "ndt2d_matcher_create_multi": (C.c_int, [C.POINTER(_vp), C.POINTER(C.c_int), C.c_int]),
    "ndt2d_matcher_device_count": (C.c_int, [_vp]),
    "ndt2d_matcher_device_at": (_vp, [_vp, C.c_int]),
    "ndt2d_matcher_set_exchange": (C.c_int, [_vp, C.c_char_p]),
    "ndt2d_matcher_set_multi_min_units": (C.c_int, [_vp, _d]),
    "ndt2d_matcher_set_multi_thresholds": (C.c_int, [_vp, _d, _d]),
    "ndt2d_matcher_get_multi_thresholds": (C.c_int, [_vp, _dp, _dp]),
    "ndt2d_matcher_last_fanout_us": (C.c_int, [_vp, _dp, _sz, _szp]),
    "ndt2d_matcher_last_variant": (C.c_char_p, [_vp]),
    "ndt2d_matcher_set_timing": (C.c_int, [_vp, C.c_int]),
    "ndt2d_matcher_destroy": (C.c_int, [_vp]),
    "ndt2d_matcher_last_error": (C.c_char_p, [_vp]),
    "ndt2d_matcher_device": (_vp, [_vp]),
    "ndt2d_matcher_initialize": (C.c_int, [_vp, _d, _d, _d, _d, _d, _sz, _d]),
    "ndt2d_matcher_add_scans": (C.c_int, [_vp, _dp, _dp, _szp, _sz]),
    "ndt2d_matcher_set_eigenvalue_form": (C.c_int, [_vp, C.c_char_p]),
    "ndt2d_matcher_set_build_mode": (C.c_int, [_vp, C.c_char_p]),
    "ndt2d_matcher_store_scan": (C.c_int, [_vp, _dp, _sz, _szp]),
    "ndt2d_matcher_add_scans_by_id": (C.c_int, [_vp, _dp, _szp, _sz]),
    "ndt2d_matcher_drop_scans": (C.c_int, [_vp]),
    "ndt2d_matcher_last_build": (C.c_char_p, [_vp]),
    "ndt2d_matcher_match_scan": (C.c_int, [_vp, _dp, _dp, _sz, _dp, _dp, _dp]),
    "ndt2d_matcher_match_scan_ex": (C.c_int, [_vp, _dp, _dp, _sz, _dp, _dp, _dp, _dp, _sz,
                                             _szp, C.POINTER(C.c_uint64)]),
    "ndt2d_matcher_match_candidates": (C.c_int, [_vp, _dp, _dp, _sz, _szp, _szp, _dp, _sz, _dp, _dp, _dp,
                                                C.POINTER(C.c_uint64), _dp, _sz, _szp]),
    "ndt2d_matcher_closure": (_vp, [_vp]),
    "ndt2d_matcher_match_starts": (C.c_int, [_vp, _dp, _sz, _dp, _sz, _dp, _dp, _dp, C.POINTER(C.c_uint64), _dp, _sz,
                                             _szp]),
    "ndt2d_matcher_starts": (_vp, [_vp]),
    "ndt2d_matcher_match_wide": (C.c_int, [_vp, _dp, _dp, _sz, _d, _d, _d, _d, _u32, _dp, _dp, C.POINTER(_u64),
                                           C.POINTER(C.c_int), C.POINTER(_u64)]),
    "ndt2d_matcher_wide": (_vp, [_vp]),
    "ndt2d_matcher_match_scans": (C.c_int, [_vp, _dp, C.POINTER(_u32), _sz, _dp, _szp, _sz, _dp, _dp, _dp,
                                            C.POINTER(C.c_uint64), _dp, _sz, _szp]),
    "ndt2d_matcher_scans": (_vp, [_vp]),
    "ndt2d_matcher_refine_scans": (C.c_int, [_vp, _dp, C.POINTER(_u32), _sz, _dp, _szp, _sz, _u32, _d, _d, _dp, _dp, _dp, _dp,
                                             _dp, C.POINTER(C.c_int32), C.POINTER(_u32)]),
    "ndt2d_matcher_refine_candidates": (C.c_int, [_vp, _szp, _szp, _dp, _sz, _dp, C.POINTER(_u32), C.POINTER(_u32), _sz, _dp, _szp,
                                                  _sz, _u32, _d, _d, _dp, _dp, _dp, _dp, _dp, C.POINTER(C.c_int32),
                                                  C.POINTER(_u32)]),
    "ndt2d_matcher_refine": (_vp, [_vp]),
    "ndt2d_matcher_set_refine_neighbourhood": (C.c_int, [_vp, _u32]),
    "ndt2d_matcher_refine_neighbourhood": (C.c_int, [_vp, C.POINTER(_u32)]),
    "ndt2d_matcher_verify_scans": (C.c_int, [_vp, _dp, C.POINTER(_u32), _sz, _dp, _szp, _sz, _sz, C.POINTER(_u32), _szp,
                                             C.POINTER(C.c_uint8), _dp, C.POINTER(_u32), _sz]),
    "ndt2d_matcher_verify_candidates": (C.c_int, [_vp, _szp, _szp, _dp, _sz, _dp, C.POINTER(_u32), C.POINTER(_u32), _sz, _dp, _szp,
                                                  _sz, _sz, C.POINTER(_u32), _szp, C.POINTER(C.c_uint8), _dp, C.POINTER(_u32), _sz]),
    "ndt2d_matcher_verify": (_vp, [_vp]),
    "ndt2d_matcher_set_verify_neighbourhood": (C.c_int, [_vp, _u32]),
    "ndt2d_matcher_verify_neighbourhood": (C.c_int, [_vp, C.POINTER(_u32)]),
    "ndt2d_matcher_set_verify_gates": (C.c_int, [_vp, _d, _d]),
    "ndt2d_matcher_verify_gates": (C.c_int, [_vp, _dp, _dp]),
    "ndt2d_matcher_set_verify_rays": (C.c_int, [_vp, C.c_int]),
    "ndt2d_matcher_verify_rays": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "ndt2d_matcher_match_laser_scan": (C.c_int, [_vp, _dp, C.POINTER(C.c_float), _sz,
                                                 C.POINTER(LaserScan), _dp, _dp, _dp, _szp]),
    "ndt2d_matcher_prepare_search": (C.c_int, [_vp, _dp, _dp, _sz, _szp, _szp, _szp]),
    "ndt2d_matcher_finish_match": (C.c_int, [_vp, _dp, _dp, _dp, _dp]),
    "ndt2d_matcher_prepare_beams": (C.c_int, [_vp, _dp, _sz, _szp]),
    "ndt2d_matcher_score_scan": (C.c_int, [_vp, _dp, _dp, _sz, _dp]),
    "ndt2d_matcher_set_search_ahead": (C.c_int, [_vp, C.c_int]),
    "ndt2d_matcher_set_adjudication": (C.c_int, [_vp, C.c_int]),
    "ndt2d_matcher_settle_near_tie": (C.c_int, [_vp, _dp, _dp]),
    "ndt2d_matcher_adjudication_stats": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                                   C.POINTER(C.c_uint64)]),
    "ndt2d_matcher_set_single_pose_path": (C.c_int, [_vp, C.c_char_p, _sz]),
    "ndt2d_matcher_search_ahead_stats": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "ndt2d_matcher_score_points": (C.c_int, [_vp, _dp, _sz, _dp, _dp]),
    "ndt2d_matcher_reset": (C.c_int, [_vp]),
    "ndt2d_matcher_has_ndt": (C.c_int, [_vp]),
    "ndt2d_matcher_score_poses": (C.c_int, [_vp, _dp, _sz, _dp, _sz, _dp]),
    "ndt2d_matcher_pf_measure": (C.c_int, [_vp, _dp, _sz, _dp, _sz, _dp, _dp, _dp]),
    "ndt2d_matcher_grid_info": (C.c_int, [_vp, C.POINTER(_u32), C.POINTER(_u32), _dp, _dp, _dp]),
    "ndt2d_matcher_grid_cells6": (C.c_int, [_vp, _dp, _sz]),
    "ndt2d_search_offsets": (C.c_int, [_d, _d, _dp, _sz, _szp]),
    "ndt2d_kld_resample": (C.c_int, [_dp, _dp, _sz, _sz, _sz, _d, _d, _dp, _dp, _sz,
                                     C.POINTER(_u32), _szp]),
    "ndt2d_host_build_grid": (C.c_int, [_d, _d, _dp, _dp, _szp, _sz, _dp, _sz,
                                       C.POINTER(_u32), C.POINTER(_u32), _dp, _dp]),
    "ndt2d_host_build_grid_ex": (C.c_int, [_d, _d, _dp, _dp, _szp, _sz, C.c_uint, _dp, _sz,
                                          C.POINTER(_u32), C.POINTER(_u32), _dp, _dp]),
    "ndt2d_synth_scan": (C.c_int, [C.POINTER(World), _dp, _sz, _d, C.c_uint64, _dp]),
    "ndt2d_synth_pose_blocked": (C.c_int, [C.POINTER(World), _d, _d, _d]),
    "ndt2d_synth_uniform": (C.c_int, [C.c_uint64, _sz, _dp]),
}

_lib = None


def lib():
    """The loaded library.  Raises ImportError if the extension is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "ndt_2d_amd: %s is missing -- build it with `python -m ndt_2d_amd.build` "
            "(or __graft_entry__.build()); there is no CPU fallback" % LIB_PATH)
    # PyTorch-ROCm wheels bundle their own HIP runtime.  If this library pulled in
    # the system libamdhip64 first, a later `import torch` would bring a second
    # runtime into the process and find no GPUs; loading torch's first makes both
    # share one.  (Pure C/C++ hosts, e.g. the ROS plugin, never see torch.)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


def build_info():
    """ndt2d_build_info() of the loaded library."""
    return lib().ndt2d_build_info().decode()


def lib_source_sha256():
    """The source hash the loaded library carries (build.source_sha256() at its build time)."""
    info = build_info()
    key = "NDT2D_SOURCE_SHA256="
    at = info.find(key)
    return info[at + len(key):at + len(key) + 64] if at >= 0 else None


def dptr(a):
    return a.ctypes.data_as(_dp)
