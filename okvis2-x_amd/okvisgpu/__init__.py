"""ctypes binding of the okvisgpu C ABI (include/okvisgpu.h).

The product is the C-ABI shared library ``okvis2-x_amd/libokvisgpu.so`` (HIP kernels for gfx950 +
C++ host runtime). This module only marshals structs for tests, the benchmark and Python callers;
it contains no solver logic and no CPU fallback: if the library (or its GPU code object) is
missing, every call fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(_HERE)
REPO_ROOT = os.path.dirname(PKG_ROOT)
LIB_PATH = os.environ.get("OKVISGPU_LIB") or os.path.join(PKG_ROOT, "libokvisgpu.so")  # env: A/B builds

IMU_STATE_DOUBLES = 526
GPS_STATE_DOUBLES = 292

DIST_NONE, DIST_RADTAN, DIST_EQUIDISTANT, DIST_RADTAN8 = 0, 1, 2, 3
DENSE_SCHUR, SPARSE_NORMAL_CHOLESKY = 0, 1
TERMINATION = {0: "CONVERGENCE", 1: "NO_CONVERGENCE", 2: "FAILURE", 3: "USER_SUCCESS"}

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_lp = C.POINTER(C.c_int64)
_up = C.POINTER(C.c_uint8)
_fp = C.POINTER(C.c_float)


class Camera(C.Structure):
    _fields_ = [("distortion", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("fu", C.c_double), ("fv", C.c_double), ("cu", C.c_double), ("cv", C.c_double),
                ("dist", C.c_double * 8)]


class ImuParams(C.Structure):
    _fields_ = [("a_max", C.c_double), ("g_max", C.c_double), ("sigma_g_c", C.c_double),
                ("sigma_a_c", C.c_double), ("sigma_gw_c", C.c_double), ("sigma_aw_c", C.c_double),
                ("g", C.c_double)]


# robust losses (ABI 6; okvisgpu_loss_kind): ::ceres::LossFunction family
LOSS_NONE, LOSS_CAUCHY, LOSS_TUKEY, LOSS_HUBER, LOSS_SOFTLONE, LOSS_ARCTAN, LOSS_TOLERANT = range(7)
LOSS_KINDS = {"none": LOSS_NONE, "cauchy": LOSS_CAUCHY, "tukey": LOSS_TUKEY, "huber": LOSS_HUBER,
              "softlone": LOSS_SOFTLONE, "arctan": LOSS_ARCTAN, "tolerant": LOSS_TOLERANT}


class Loss(C.Structure):
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("a", C.c_double), ("b", C.c_double)]


# numpy record layout of okvisgpu_loss (arrays of per-factor losses: host_loss)
LOSS_DTYPE = np.dtype([("kind", "<i4"), ("reserved", "<i4"), ("a", "<f8"), ("b", "<f8")])


def loss_array(specs):
    """[(kind name or id, a[, b]), ...] -> LOSS_DTYPE array for okvisgpu_problem.host_loss."""
    out = np.zeros(len(specs), dtype=LOSS_DTYPE)
    for i, sp in enumerate(specs):
        k = LOSS_KINDS[sp[0]] if isinstance(sp[0], str) else int(sp[0])
        out[i] = (k, 0, float(sp[1]) if len(sp) > 1 else 1.0, float(sp[2]) if len(sp) > 2 else 0.0)
    return out


def loss_evaluate(kind, a=1.0, b=0.0, s=0.0):
    """okvisgpu_loss_evaluate: (rho, rho', rho'') of a loss at the squared norm s (host only)."""
    L = Loss(LOSS_KINDS[kind] if isinstance(kind, str) else int(kind), 0, a, b)
    rho = (C.c_double * 3)()
    rc = lib().okvisgpu_loss_evaluate(C.byref(L), float(s), rho)
    if rc != 0:
        raise OkvisGpuError(f"okvisgpu_loss_evaluate failed ({rc})")
    return tuple(rho)


# okvisgpu_host_evaluate_fn (ABI 5): (user, factor, parameters, residuals, jacobians) -> nonzero = ok
HOST_EVALUATE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.POINTER(_dp), _dp, C.POINTER(_dp))
HOST_MAX_RESIDUALS = 15


class Problem(C.Structure):
    _fields_ = [
        ("n_poses", C.c_int32), ("poses", _dp), ("pose_constant", _up),
        ("n_speed_biases", C.c_int32), ("speed_biases", _dp), ("speed_bias_constant", _up),
        ("n_landmarks", C.c_int32), ("landmarks", _dp), ("landmark_constant", _up),
        ("n_cameras", C.c_int32), ("cameras", C.POINTER(Camera)), ("extrinsics", _dp),
        ("n_observations", C.c_int32), ("obs_pose", _ip), ("obs_landmark", _ip), ("obs_camera", _ip),
        ("obs_keypoint", _dp), ("obs_sqrt_info", _dp), ("obs_cauchy", _up),
        ("n_imu", C.c_int32), ("imu_blocks", _ip), ("imu_t0_ns", _lp), ("imu_t1_ns", _lp),
        ("imu_sample_begin", _ip), ("imu_sample_t_ns", _lp), ("imu_sample_gyr_acc", _dp),
        ("imu_params", ImuParams), ("imu_state", _dp),
        ("n_pose_priors", C.c_int32), ("pose_prior_block", _ip), ("pose_prior_meas", _dp),
        ("pose_prior_sqrt_info", _dp),
        ("n_sb_priors", C.c_int32), ("sb_prior_block", _ip), ("sb_prior_meas", _dp),
        ("sb_prior_sqrt_info", _dp),
        ("n_relpose", C.c_int32), ("relpose_blocks", _ip), ("relpose_delta_x", _dp),
        ("relpose_sqrt_info", _dp), ("relpose_lin_point", _dp), ("relpose_kind", _up),
        ("extrinsics_constant", _up), ("n_extrinsics_priors", C.c_int32), ("extrinsics_prior_camera", _ip),
        ("extrinsics_prior_meas", _dp), ("extrinsics_prior_sqrt_info", _dp),
        ("n_host", C.c_int32), ("host_dim", _ip), ("host_param_kind", _ip), ("host_param_index", _ip),
        ("host_cauchy", _up), ("host_evaluate", HOST_EVALUATE_FN), ("host_user", C.c_void_p),
        ("host_loss", C.c_void_p),
    ]


def host_evaluate(fn, block_sizes):
    """Wrap a Python cost function as an okvisgpu_host_evaluate_fn (the §8b host fallback).

    fn(factor, params) -> (r, jacobians) or None (evaluation failure): params is the list of the
    factor's parameter blocks (numpy copies, ambient: 7 pose-kind / 9 speed-bias), r the residual
    vector, jacobians one ambient [dim, size] array per block (ceres::CostFunction::Evaluate
    semantics). block_sizes[factor] = the blocks' ambient sizes. Keep the returned object alive as
    long as a problem points at it."""
    def cb(_user, factor, params, residuals, jacobians):
        try:
            sizes = block_sizes[factor]
            out = fn(factor, [np.ctypeslib.as_array(params[k], shape=(n,)).copy() for k, n in enumerate(sizes)])
            if out is None:
                return 0
            r, J = out
            r = np.asarray(r, dtype=np.float64)
            np.ctypeslib.as_array(residuals, shape=(len(r),))[:] = r
            if jacobians:
                for k, n in enumerate(sizes):
                    if jacobians[k]:
                        np.ctypeslib.as_array(jacobians[k], shape=(len(r) * n,))[:] = np.asarray(J[k]).reshape(-1)
            return 1
        except Exception:  # a Python error is an evaluation failure, never an unwinding through C
            return 0
    return HOST_EVALUATE_FN(cb)


class Options(C.Structure):
    _fields_ = [
        ("max_num_iterations", C.c_int32), ("linear_solver", C.c_int32),
        ("trust_region_strategy", C.c_int32), ("jacobi_scaling", C.c_int32),
        ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double),
        ("parameter_tolerance", C.c_double), ("initial_trust_region_radius", C.c_double),
        ("max_trust_region_radius", C.c_double), ("min_trust_region_radius", C.c_double),
        ("min_relative_decrease", C.c_double), ("min_lm_diagonal", C.c_double),
        ("max_lm_diagonal", C.c_double), ("max_num_consecutive_invalid_steps", C.c_int32),
        ("time_limit_s", C.c_double), ("min_iterations", C.c_int32),
        ("redo_propagation_always", C.c_int32), ("num_threads", C.c_int32), ("verbose", C.c_int32),
        ("cholesky_schedule", C.c_int32),
    ]


class Summary(C.Structure):
    _fields_ = [("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("num_iterations", C.c_int32), ("num_successful_steps", C.c_int32),
                ("num_unsuccessful_steps", C.c_int32), ("termination_type", C.c_int32),
                ("total_time_s", C.c_double), ("final_radius", C.c_double), ("final_mu", C.c_double),
                ("preprocessor_time_s", C.c_double), ("minimizer_time_s", C.c_double),
                ("postprocessor_time_s", C.c_double), ("linear_solver_time_s", C.c_double),
                ("residual_evaluation_time_s", C.c_double), ("jacobian_evaluation_time_s", C.c_double),
                ("step_time_s", C.c_double)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["termination"] = TERMINATION.get(self.termination_type, "?")
        return d


class SynthConfig(C.Structure):
    _fields_ = [("n_keyframes", C.c_int32), ("n_landmarks", C.c_int32), ("n_observations", C.c_int32),
                ("max_obs_per_landmark", C.c_int32), ("kf_dt_s", C.c_double), ("imu_rate_hz", C.c_double),
                ("pixel_noise", C.c_double), ("init_sigma_pos", C.c_double), ("init_sigma_rot", C.c_double),
                ("init_sigma_lm", C.c_double), ("init_sigma_vel", C.c_double), ("seed", C.c_uint64),
                ("n_relpose", C.c_int32), ("relpose_stride", C.c_int32), ("relpose_kind", C.c_int32),
                ("do_extrinsics", C.c_int32), ("extrinsics_sigma_r", C.c_double), ("extrinsics_sigma_alpha", C.c_double)]


class ProblemStats(C.Structure):
    _fields_ = [("n_windows", C.c_int32), ("cholesky_launches", C.c_int32)] + [(k, C.c_int64) for k in (
        "n_poses", "n_speed_biases", "n_landmarks", "n_landmarks_free", "n_extrinsics_free", "n_observations",
        "n_visits", "n_imu", "n_imu_samples", "n_pose_priors", "n_sb_priors", "n_relpose", "reduced_dim",
        "s_tiles_nonzero", "s_tiles_dense", "n_block_pairs", "n_visit_segments", "n_partial_blocks",
        "arena_bytes", "cholesky_split_windows")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ImuAppendBatch(C.Structure):
    _fields_ = [("n", C.c_int32), ("imu_params", ImuParams), ("state", _dp), ("t1_old_ns", _lp), ("t1_new_ns", _lp),
                ("speed_biases", _dp), ("sample_begin", _ip), ("sample_t_ns", _lp), ("sample_gyr_acc", _dp)]


class ImuPropagateBatch(C.Structure):
    """okvisgpu_imu_propagate_batch: ImuError::propagation for a batch of items."""
    _fields_ = [("n", C.c_int32), ("imu_params", ImuParams), ("poses", _dp), ("speed_biases", _dp),
                ("t_start_ns", _lp), ("t_end_ns", _lp), ("sample_begin", _ip), ("sample_t_ns", _lp),
                ("sample_gyr_acc", _dp), ("covariance", _dp), ("jacobian", _dp)]


class GpsBatch(C.Structure):
    """okvisgpu_gps_batch: GpsErrorAsynchronous (kind 0) / GpsErrorSynchronous (kind 1) factors to evaluate."""
    _fields_ = [("n", C.c_int32), ("kind", C.c_int32), ("use_imu_covariance", C.c_int32),
                ("redo_propagation_always", C.c_int32), ("imu_params", ImuParams), ("r_SA", C.c_double * 3),
                ("poses", _dp), ("speed_biases", _dp), ("n_gw", C.c_int32), ("T_GW", _dp), ("gw_index", _ip),
                ("measurement", _dp), ("information", _dp), ("t_k_ns", _lp), ("t_g_ns", _lp), ("sample_begin", _ip),
                ("sample_t_ns", _lp), ("sample_gyr_acc", _dp), ("state", _dp)]


class GpsResult(C.Structure):
    """okvisgpu_gps_result: the caller-owned outputs of okvisgpu_gps_evaluate (any may be NULL)."""
    _fields_ = [("r", _dp), ("error", _dp), ("sqrt_info", _dp), ("J_pose", _dp), ("J_speed_bias", _dp), ("J_T_GW", _dp),
                ("J_pose_ambient", _dp), ("J_T_GW_ambient", _dp), ("steps", _ip)]


class LidarDeskewBatch(C.Structure):
    """okvisgpu_lidar_deskew_batch: scans (a state, IMU samples, stamped rays) to undistort."""
    _fields_ = [("n_scans", C.c_int32), ("g", C.c_double), ("pose0", _dp), ("speed_bias0", _dp), ("t_start_ns", _lp),
                ("sample_begin", _ip), ("sample_t_ns", _lp), ("sample_gyr_acc", _dp), ("query_begin", _ip),
                ("query_t_ns", _lp), ("ray", _dp), ("pose_live", _dp), ("T_SL", _dp)]


class LidarDeskewResult(C.Structure):
    """okvisgpu_lidar_deskew_result: the caller-owned outputs of okvisgpu_lidar_deskew (any may be NULL)."""
    _fields_ = [("valid", _up), ("point", _fp), ("point_f64", _dp), ("pose", _dp), ("speed", _dp), ("omega_S", _dp),
                ("n_before", _ip)]


class VoxelDownsampleBatch(C.Structure):
    """okvisgpu_voxel_downsample_batch: point clouds, each with its voxel size."""
    _fields_ = [("n_clouds", C.c_int32), ("cloud_begin", _ip), ("point", _fp), ("voxel_size", _dp), ("use", _up)]


class VoxelDownsampleResult(C.Structure):
    """okvisgpu_voxel_downsample_result: the caller-owned outputs of okvisgpu_voxel_downsample."""
    _fields_ = [("keep", _up), ("n_kept", _ip)]


class FrameOverlapBatch(C.Structure):
    """okvisgpu_frame_overlap_batch: frames (images with keypoints and landmark ids) and the overlap jobs over them."""
    _fields_ = [("n_frames", C.c_int32), ("image_begin", _ip), ("rows", _ip), ("cols", _ip), ("kp_begin", _ip),
                ("keypoint", _fp), ("landmark", C.POINTER(C.c_uint64)), ("flag", _up), ("n_jobs", C.c_int32),
                ("job_kind", _ip), ("job_frame_a", _ip), ("job_frame_b", _ip), ("job_radius_factor", _dp),
                ("n_groups", C.c_int32), ("group_begin", _ip)]


class FrameOverlapResult(C.Structure):
    """okvisgpu_frame_overlap_result: the caller-owned outputs of okvisgpu_frame_overlap (any may be NULL)."""
    _fields_ = [("overlap", _dp), ("count", _ip), ("n_matched", _ip), ("n_keypoints", _ip), ("group_best", _ip),
                ("group_max", _dp)]


class MatchBatch(C.Structure):
    """okvisgpu_match_batch: one map and the jobs (camera image x pass) matched against it."""
    _fields_ = [("n_poses", C.c_int32), ("poses", _dp), ("n_cameras", C.c_int32), ("cameras", C.POINTER(Camera)),
                ("extrinsics", _dp), ("n_landmarks", C.c_int32), ("landmarks", _dp), ("landmark_quality", _dp),
                ("landmark_use", _up), ("obs_begin", _ip), ("obs_pose", _ip), ("obs_camera", _ip),
                ("obs_descriptor", _up), ("obs_ray", _dp), ("imu_use", C.c_int32), ("loop_closure", C.c_int32),
                ("matching_threshold", C.c_double), ("n_jobs", C.c_int32), ("job_camera", _ip), ("job_pass", _ip),
                ("job_pose_prepare", _dp), ("job_pose_match", _dp), ("kp_begin", _ip), ("keypoint", _dp),
                ("descriptor", _up), ("ray", _dp), ("ray_valid", _up), ("landmark", _ip)]


class MatchResult(C.Structure):
    """okvisgpu_match_result: the caller-owned outputs of okvisgpu_match_to_map (any may be NULL)."""
    _fields_ = [("match_landmark", _ip), ("match_distance", _ip), ("n_records", _ip), ("record_repr_sum", _dp),
                ("point", _dp), ("cand_n", _ip), ("cand_is3d", _up), ("cand_obs", _ip), ("cand_projection", _dp)]


class FrameMatchBatch(C.Structure):
    """okvisgpu_frame_match_batch: jobs matching the keypoints of one image against those of another."""
    _fields_ = [("n_cameras", C.c_int32), ("cameras", C.POINTER(Camera)), ("matching_threshold", C.c_double),
                ("n_jobs", C.c_int32), ("job_mode", _ip), ("job_camera0", _ip), ("job_camera1", _ip),
                ("job_pose0", _dp), ("job_pose1", _dp), ("job_extrinsics0", _dp), ("job_extrinsics1", _dp),
                ("kp0_begin", _ip), ("kp1_begin", _ip),
                ("keypoint0", _dp), ("size0", _dp), ("descriptor0", _up), ("ray0", _dp), ("ray_valid0", _up), ("use0", _up),
                ("keypoint1", _dp), ("size1", _dp), ("descriptor1", _up), ("ray1", _dp), ("ray_valid1", _up), ("use1", _up)]


class FrameMatchResult(C.Structure):
    """okvisgpu_frame_match_result: the caller-owned outputs of okvisgpu_match_frames (any may be NULL)."""
    _fields_ = [("match", _ip), ("distance", _ip), ("point", _dp), ("initialisable", _up), ("quality", _dp)]


class PlaceMatchBatch(C.Structure):
    """okvisgpu_place_match_batch: candidates (old frames' landmarks) matched against new frames' images."""
    _fields_ = [("matching_threshold", C.c_double), ("n_cameras", C.c_int32), ("n_images", C.c_int32),
                ("kp_begin", _ip), ("descriptor", _up), ("n_jobs", C.c_int32), ("job_image", _ip), ("lm_begin", _ip),
                ("desc_begin", _ip), ("old_descriptor", _up)]


class PlaceMatchResult(C.Structure):
    """okvisgpu_place_match_result: the caller-owned outputs of okvisgpu_place_match (any may be NULL)."""
    _fields_ = [("match_keypoint", _ip), ("match_distance", _ip), ("job_matches", _ip)]


class PlaceRefineBatch(C.Structure):
    """okvisgpu_place_refine_batch: candidates whose relative pose is refined on their inlier observations."""
    _fields_ = [("n_cameras", C.c_int32), ("cameras", C.POINTER(Camera)), ("extrinsics", _dp), ("loss", Loss),
                ("max_num_iterations", C.c_int32), ("n_jobs", C.c_int32), ("pose", _dp), ("obs_begin", _ip),
                ("obs_camera", _ip), ("obs_keypoint", _dp), ("obs_sqrt_info", _dp), ("obs_point", _dp)]


class PlaceRefineResult(C.Structure):
    """okvisgpu_place_refine_result: the caller-owned outputs of okvisgpu_place_refine (any may be NULL)."""
    _fields_ = [("H", _dp), ("n_outliers", _ip), ("initial_cost", _dp), ("final_cost", _dp), ("num_iterations", _ip),
                ("num_successful_steps", _ip), ("num_unsuccessful_steps", _ip), ("termination_type", _ip)]


class TwoPoseEdges(C.Structure):
    _fields_ = [("n_edges", C.c_int32), ("ref_pose", _dp), ("other_pose", _dp),
                ("n_cameras", C.c_int32), ("cameras", C.POINTER(Camera)), ("extrinsics", _dp),
                ("landmark_begin", _ip), ("landmarks", _dp), ("obs_begin", _ip), ("obs_other", _up),
                ("obs_camera", _ip), ("obs_keypoint", _dp), ("obs_sqrt_info", _dp), ("obs_cauchy", _up)]


class TwoPoseExtrinsicsEval(C.Structure):
    """okvisgpu_twopose_extrinsics_eval: computed calibrating edges and the values to evaluate them at."""
    _fields_ = [("n_edges", C.c_int32), ("n_cameras", C.c_int32), ("ref_pose", _dp), ("other_pose", _dp),
                ("extrinsics", _dp), ("delta_x", _dp), ("sqrt_info", _dp), ("lin_point", _dp),
                ("lin_extrinsics", _dp), ("camera_seen", _up)]


class LandmarkUpdate(C.Structure):
    """okvisgpu_landmark_update: one window's outputs of okvisgpu_update_landmarks."""
    _fields_ = [("quality", _dp), ("initialised", _up), ("reset", _up), ("obs_error", _dp),
                ("n_initialised", C.c_int32), ("n_reset", C.c_int32), ("in_front", C.c_int32),
                ("reserved", C.c_int32)]


class Covisibility(C.Structure):
    """okvisgpu_covisibility: one window's exclusion mask and outputs of okvisgpu_covisibilities."""
    _fields_ = [("landmark_excluded", _up), ("counts", _ip), ("n_observed", _ip), ("visible", _up),
                ("n_pairs", C.c_int32), ("n_visible", C.c_int32), ("any", C.c_int32), ("path", C.c_int32)]


# Exported symbols of include/okvisgpu.h (checked by tests/test_abi.py).
EXPORTED_SYMBOLS = [
    "okvisgpu_abi_version", "okvisgpu_default_options", "okvisgpu_device_count", "okvisgpu_ctx_create",
    "okvisgpu_ctx_destroy", "okvisgpu_last_error", "okvisgpu_set_problems", "okvisgpu_update_params",
    "okvisgpu_set_block_constant", "okvisgpu_solve", "okvisgpu_get_params", "okvisgpu_evaluate",
    "okvisgpu_linearize_reduce", "okvisgpu_eval_reprojection", "okvisgpu_eval_imu",
    "okvisgpu_synth_default_config", "okvisgpu_synth_create", "okvisgpu_synth_problem",
    "okvisgpu_synth_ground_truth", "okvisgpu_synth_reset", "okvisgpu_synth_destroy",
    "okvisgpu_solve_begin", "okvisgpu_solve_iterate", "okvisgpu_solve_end", "okvisgpu_synchronize",
    "okvisgpu_profile_iteration", "okvisgpu_phase_name", "okvisgpu_kernel_count", "okvisgpu_kernel_name",
    "okvisgpu_time_kernel", "okvisgpu_eval_relpose", "okvisgpu_twopose_compute",
    "okvisgpu_graph_load", "okvisgpu_graph_problem", "okvisgpu_graph_ids", "okvisgpu_graph_destroy",
    "okvisgpu_graph_save", "okvisgpu_get_stats", "okvisgpu_synth_true_extrinsics", "okvisgpu_imu_append",
    "okvisgpu_eval_host", "okvisgpu_plan_window", "okvisgpu_loss_evaluate", "okvisgpu_plan_digest",
    "okvisgpu_launch_regime", "okvisgpu_update_landmarks", "okvisgpu_covisibilities", "okvisgpu_imu_propagate",
    "okvisgpu_twopose_extrinsics_compute", "okvisgpu_twopose_extrinsics_evaluate", "okvisgpu_gauss_newton_step",
    "okvisgpu_match_to_map", "okvisgpu_plan_assembly", "okvisgpu_match_frames", "okvisgpu_place_match",
    "okvisgpu_place_refine", "okvisgpu_lidar_deskew", "okvisgpu_voxel_downsample", "okvisgpu_gps_evaluate",
    "okvisgpu_frame_overlap",
]
N_PHASES = 15
TWOPOSE_MAX_CAMERAS = 6

_lib = None


def lib():
    """Load libokvisgpu.so (fails loudly if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"okvisgpu: {LIB_PATH} missing — build it with `make -C okvis2-x_amd`")
        L = C.CDLL(LIB_PATH)
        L.okvisgpu_abi_version.restype = C.c_int
        L.okvisgpu_default_options.argtypes = [C.POINTER(Options)]
        L.okvisgpu_device_count.argtypes = [_ip]
        L.okvisgpu_ctx_create.argtypes = [C.c_int32, C.POINTER(C.c_void_p)]
        L.okvisgpu_ctx_destroy.argtypes = [C.c_void_p]
        L.okvisgpu_last_error.argtypes = [C.c_void_p]
        L.okvisgpu_last_error.restype = C.c_char_p
        L.okvisgpu_set_problems.argtypes = [C.c_void_p, C.POINTER(Problem), C.c_int32]
        L.okvisgpu_update_params.argtypes = [C.c_void_p]
        L.okvisgpu_set_block_constant.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
        L.okvisgpu_solve.argtypes = [C.c_void_p, C.POINTER(Options), C.POINTER(Summary)]
        L.okvisgpu_get_params.argtypes = [C.c_void_p]
        L.okvisgpu_evaluate.argtypes = [C.c_void_p, C.c_int32, _dp]
        L.okvisgpu_linearize_reduce.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_double, _dp, _dp, _dp, _ip]
        L.okvisgpu_gauss_newton_step.argtypes = [C.c_void_p, C.c_int32, C.POINTER(Options), C.c_double, _dp, _dp, _ip]
        L.okvisgpu_eval_reprojection.argtypes = [C.c_void_p, C.c_int32, _dp, _dp, _dp]
        L.okvisgpu_eval_imu.argtypes = [C.c_void_p, C.c_int32, C.c_int32, _dp, _dp]
        L.okvisgpu_synth_default_config.argtypes = [C.POINTER(SynthConfig), C.c_int32, C.c_int32, C.c_int32, C.c_uint64]
        L.okvisgpu_synth_create.argtypes = [C.POINTER(SynthConfig), C.POINTER(C.c_void_p)]
        L.okvisgpu_synth_problem.argtypes = [C.c_void_p]
        L.okvisgpu_synth_problem.restype = C.POINTER(Problem)
        L.okvisgpu_synth_ground_truth.argtypes = [C.c_void_p, _dp, _dp, _dp]
        L.okvisgpu_synth_reset.argtypes = [C.c_void_p]
        L.okvisgpu_synth_true_extrinsics.argtypes = [C.c_void_p, _dp]
        L.okvisgpu_synth_destroy.argtypes = [C.c_void_p]
        L.okvisgpu_solve_begin.argtypes = [C.c_void_p, C.POINTER(Options)]
        L.okvisgpu_solve_iterate.argtypes = [C.c_void_p, C.c_int32]
        L.okvisgpu_solve_end.argtypes = [C.c_void_p, C.POINTER(Summary)]
        L.okvisgpu_synchronize.argtypes = [C.c_void_p]
        L.okvisgpu_profile_iteration.argtypes = [C.c_void_p, _dp]
        L.okvisgpu_phase_name.argtypes = [C.c_int32]
        L.okvisgpu_phase_name.restype = C.c_char_p
        L.okvisgpu_kernel_count.restype = C.c_int
        L.okvisgpu_kernel_name.argtypes = [C.c_int32]
        L.okvisgpu_kernel_name.restype = C.c_char_p
        L.okvisgpu_time_kernel.argtypes = [C.c_void_p, C.c_int32, C.c_int32, _dp, _dp, C.POINTER(C.c_int32)]
        L.okvisgpu_eval_relpose.argtypes = [C.c_void_p, C.c_int32, _dp, _dp]
        L.okvisgpu_eval_host.argtypes = [C.c_void_p, C.c_int32, _dp, _dp]
        L.okvisgpu_graph_load.argtypes = [C.c_char_p, C.POINTER(Camera), C.c_int32, C.POINTER(ImuParams),
                                          C.POINTER(C.c_void_p)]
        L.okvisgpu_graph_problem.argtypes = [C.c_void_p]
        L.okvisgpu_graph_problem.restype = C.POINTER(Problem)
        L.okvisgpu_graph_ids.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), _lp, C.POINTER(C.c_uint64)]
        L.okvisgpu_graph_destroy.argtypes = [C.c_void_p]
        L.okvisgpu_graph_save.argtypes = [C.POINTER(Problem), _lp, C.c_char_p]
        L.okvisgpu_get_stats.argtypes = [C.c_void_p, C.POINTER(ProblemStats)]
        L.okvisgpu_plan_window.argtypes = [C.POINTER(Problem), C.c_int32, _lp, C.POINTER(C.c_uint8), _ip, _ip]
        L.okvisgpu_plan_digest.argtypes = [C.POINTER(Problem), C.c_int32, C.c_int32, _lp, C.c_int32, _ip, C.c_char_p,
                                           _ip, _lp, C.POINTER(C.c_uint64)]
        L.okvisgpu_launch_regime.argtypes = [C.c_int32] * 9 + [_ip]
        L.okvisgpu_plan_assembly.argtypes = [C.POINTER(Problem), C.c_int32, C.c_int32, _ip, C.c_int32, _ip, _lp]
        L.okvisgpu_imu_append.argtypes = [C.c_void_p, C.POINTER(ImuAppendBatch), _ip]
        L.okvisgpu_imu_propagate.argtypes = [C.c_void_p, C.POINTER(ImuPropagateBatch), _ip]
        L.okvisgpu_gps_evaluate.argtypes = [C.c_void_p, C.POINTER(GpsBatch), C.POINTER(GpsResult)]
        L.okvisgpu_lidar_deskew.argtypes = [C.c_void_p, C.POINTER(LidarDeskewBatch), C.POINTER(LidarDeskewResult)]
        L.okvisgpu_voxel_downsample.argtypes = [C.c_void_p, C.POINTER(VoxelDownsampleBatch),
                                                C.POINTER(VoxelDownsampleResult)]
        L.okvisgpu_frame_overlap.argtypes = [C.c_void_p, C.POINTER(FrameOverlapBatch), C.POINTER(FrameOverlapResult)]
        L.okvisgpu_match_to_map.argtypes = [C.c_void_p, C.POINTER(MatchBatch), C.POINTER(MatchResult)]
        L.okvisgpu_match_frames.argtypes = [C.c_void_p, C.POINTER(FrameMatchBatch), C.POINTER(FrameMatchResult)]
        L.okvisgpu_place_match.argtypes = [C.c_void_p, C.POINTER(PlaceMatchBatch), C.POINTER(PlaceMatchResult)]
        L.okvisgpu_place_refine.argtypes = [C.c_void_p, C.POINTER(PlaceRefineBatch), C.POINTER(PlaceRefineResult)]
        L.okvisgpu_twopose_compute.argtypes = [C.c_void_p, C.POINTER(TwoPoseEdges), _dp, _dp, _dp, _dp, _dp]
        L.okvisgpu_twopose_extrinsics_compute.argtypes = [C.c_void_p, C.POINTER(TwoPoseEdges), _dp, _dp, _dp, _up, _dp,
                                                          _dp]
        L.okvisgpu_twopose_extrinsics_evaluate.argtypes = [C.c_void_p, C.POINTER(TwoPoseExtrinsicsEval), _dp, _dp, _dp,
                                                           _dp]
        L.okvisgpu_loss_evaluate.argtypes = [C.POINTER(Loss), C.c_double, _dp]
        L.okvisgpu_update_landmarks.argtypes = [C.c_void_p, C.POINTER(LandmarkUpdate)]
        L.okvisgpu_covisibilities.argtypes = [C.c_void_p, C.POINTER(Covisibility)]
        _lib = L
    return _lib


def plan_window(problem, nested_dissection):
    """okvisgpu_plan_window (host only): the window's state order, filled tile pattern and
    tile-parallel factorisation schedule."""
    L = lib()
    info = (C.c_int64 * 8)()
    pp = C.byref(problem) if isinstance(problem, Problem) else problem
    rc = L.okvisgpu_plan_window(pp, int(nested_dissection), info, None, None, None)
    if rc != 0:
        raise RuntimeError(f"okvisgpu_plan_window failed ({rc})")
    keys = ("reduced_dim", "s_dim", "tiles", "nonzero_tiles", "launches", "split_tL", "split_tS", "gap_rows")
    out = {k: int(v) for k, v in zip(keys, info)}
    T, D = out["tiles"], out["s_dim"]
    nz = np.zeros(T * T, dtype=np.uint8)
    launch = np.zeros(T, dtype=np.int32)
    nat = np.zeros(D, dtype=np.int32)
    rc = L.okvisgpu_plan_window(pp, int(nested_dissection), info, nz.ctypes.data_as(C.POINTER(C.c_uint8)),
                                launch.ctypes.data_as(_ip), nat.ctypes.data_as(_ip))
    if rc != 0:
        raise RuntimeError(f"okvisgpu_plan_window failed ({rc})")
    out["tile_nz"] = nz.reshape(T, T)
    out["step_launch"] = launch
    out["natural"] = nat
    return out


PLAN_DIGEST_TOTALS = ("f_total", "s_total", "linv_total", "fwd_total", "defer_total", "max_fpad", "max_panels",
                      "n_chol_launches", "n_panels", "n_band_updates", "n_band_updates_diag", "any_split", "obs_iso",
                      "upload_bytes", "scratch_bytes")


def plan_digest(problems, cu_count):
    """okvisgpu_plan_digest (host only): the plan of a batch on a device of cu_count CUs as its
    scalar totals and, in arena-table order, [name, region (0 uploaded, 1 scratch), bytes,
    FNV-1a-64 of the uploaded bytes as hex (None for scratch)] per device array."""
    L = lib()
    arr = (Problem * len(problems))(*problems)
    totals, n = (C.c_int64 * 16)(), C.c_int32(0)
    rc = L.okvisgpu_plan_digest(arr, len(problems), int(cu_count), totals, 0, C.byref(n), None, None, None, None)
    if rc != 0:
        raise RuntimeError(f"okvisgpu_plan_digest failed ({rc})")
    cap = n.value
    names = C.create_string_buffer(32 * cap)
    region, nbytes, hashes = (C.c_int32 * cap)(), (C.c_int64 * cap)(), (C.c_uint64 * cap)()
    rc = L.okvisgpu_plan_digest(arr, len(problems), int(cu_count), totals, cap, C.byref(n), names, region, nbytes, hashes)
    if rc != 0 or n.value != cap:
        raise RuntimeError(f"okvisgpu_plan_digest failed ({rc})")
    entries = [[names.raw[32 * i:32 * i + 32].split(b"\0")[0].decode(), int(region[i]), int(nbytes[i]),
                f"{hashes[i]:016x}" if region[i] == 0 else None] for i in range(cap)]
    return {"totals": {k: int(v) for k, v in zip(PLAN_DIGEST_TOTALS, totals)}, "entries": entries}


def plan_assembly(problems, cu_count):
    """okvisgpu_plan_assembly (host only): (counts of the heavy / light / speed-bias item lists,
    records [n][12] int32, arrays [n][16] int64) of a batch's plan on a device of cu_count CUs."""
    L = lib()
    arr = (Problem * len(problems))(*problems)
    counts = (C.c_int32 * 4)()
    rc = L.okvisgpu_plan_assembly(arr, len(problems), int(cu_count), counts, 0, None, None)
    if rc != 0:
        raise RuntimeError(f"okvisgpu_plan_assembly failed ({rc})")
    n = int(counts[3])
    rec, old = np.zeros((max(n, 1), 12), np.int32), np.zeros((max(n, 1), 16), np.int64)
    rc = L.okvisgpu_plan_assembly(arr, len(problems), int(cu_count), counts, n, rec.ctypes.data_as(_ip),
                                  old.ctypes.data_as(_lp))
    if rc != 0 or int(counts[3]) != n:
        raise RuntimeError(f"okvisgpu_plan_assembly failed ({rc})")
    return [int(c) for c in counts[:3]], rec[:n], old[:n]


LAUNCH_REGIME = ("few", "many", "serial_graph", "lin_prep", "fused_gradnorm", "graph_iters", "chol_schedule")


def launch_regime(n_windows, cu_count, any_split=False, persistent_fits=True, pipe_fits=True, schedule=0,
                  serial_graph=-1, lin_prep=-1, graph_iters=-1):
    """okvisgpu_launch_regime (host only): what the batch size decides about a solve's launches; the
    last three arguments are the parsed measurement overrides (-1: not set)."""
    out = (C.c_int32 * 7)()
    rc = lib().okvisgpu_launch_regime(int(n_windows), int(cu_count), int(any_split), int(persistent_fits),
                                      int(pipe_fits), int(schedule), int(serial_graph), int(lin_prep),
                                      int(graph_iters), out)
    if rc != 0:
        raise RuntimeError(f"okvisgpu_launch_regime failed ({rc})")
    return dict(zip(LAUNCH_REGIME, (int(v) for v in out)))


def default_options(**kw) -> Options:
    o = Options()
    lib().okvisgpu_default_options(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def dptr(a: np.ndarray):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_dp)


class OkvisGpuError(RuntimeError):
    pass


class _OwnedBuffer:
    """numpy base object of a view into library-owned memory: holds a reference to the Python
    object that owns the memory, so the view keeps it (and its C allocation) alive."""

    def __init__(self, ptr, shape, owner):
        addr = C.cast(ptr, C.c_void_p).value
        if not addr and int(np.prod(shape)) > 0:
            raise OkvisGpuError("null array in problem")
        self.__array_interface__ = {"data": (addr or 0, False), "shape": tuple(int(n) for n in shape),
                                    "typestr": "<f8", "version": 3}
        self._owner = owner


def _owned_view(ptr, shape, owner) -> np.ndarray:
    return np.asarray(_OwnedBuffer(ptr, shape, owner))


def _owned_problem(ptr, owner):
    """POINTER(Problem) / Problem from the library, each holding a reference to its owner (the
    SynthWindow / Graph whose allocation the arrays point into)."""
    ptr._owner = owner
    return ptr


class SynthWindow:
    """A synthetic sliding window (owned by the C library)."""

    def __init__(self, n_kf=10, n_lm=500, n_obs=4000, seed=20251015, **overrides):
        cfg = SynthConfig()
        lib().okvisgpu_synth_default_config(C.byref(cfg), n_kf, n_lm, n_obs, seed)
        for k, v in overrides.items():
            setattr(cfg, k, v)
        h = C.c_void_p()
        rc = lib().okvisgpu_synth_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise OkvisGpuError(f"okvisgpu_synth_create failed ({rc})")
        self.handle = h
        self.cfg = cfg

    @property
    def problem(self) -> Problem:
        pr = self.problem_ptr().contents
        pr._owner = self  # the struct's arrays live in this window's allocation
        return pr

    def problem_ptr(self):
        return _owned_problem(lib().okvisgpu_synth_problem(self.handle), self)

    def reset(self):
        lib().okvisgpu_synth_reset(self.handle)

    def ground_truth(self):
        p = self.problem
        poses = np.zeros((p.n_poses, 7))
        lms = np.zeros((p.n_landmarks, 4))
        sbs = np.zeros((p.n_speed_biases, 9))
        lib().okvisgpu_synth_ground_truth(self.handle, dptr(poses), dptr(lms), dptr(sbs))
        return poses, lms, sbs

    def true_extrinsics(self):
        e = np.zeros((self.problem.n_cameras, 7))
        lib().okvisgpu_synth_true_extrinsics(self.handle, dptr(e))
        return e

    def extrinsics(self):
        p = self.problem
        return _owned_view(p.extrinsics, (p.n_cameras, 7), self)

    # views into the (mutable) parameter arrays; each view keeps this window alive
    def poses(self):
        p = self.problem
        return _owned_view(p.poses, (p.n_poses, 7), self)

    def speed_biases(self):
        p = self.problem
        return _owned_view(p.speed_biases, (p.n_speed_biases, 9), self)

    def landmarks(self):
        p = self.problem
        return _owned_view(p.landmarks, (p.n_landmarks, 4), self)

    def imu_state(self):
        p = self.problem
        return _owned_view(p.imu_state, (p.n_imu, IMU_STATE_DOUBLES), self)

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                lib().okvisgpu_synth_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


def imu_append_batch(imu_params, state, t1_old, t1_new, speed_biases, sample_begin, sample_t, sample_ga):
    """An okvisgpu_imu_append_batch over numpy arrays: (struct, arrays it points into). `state`
    [n, IMU_STATE_DOUBLES] float64 C-contiguous is referenced, not copied (updated in place)."""
    n = len(t1_old)
    keep = [np.ascontiguousarray(t1_old, dtype=np.int64), np.ascontiguousarray(t1_new, dtype=np.int64),
            np.ascontiguousarray(speed_biases, dtype=np.float64).reshape(n, 9),
            np.ascontiguousarray(sample_begin, dtype=np.int32), np.ascontiguousarray(sample_t, dtype=np.int64),
            np.ascontiguousarray(sample_ga, dtype=np.float64).reshape(-1, 6)]
    assert state.dtype == np.float64 and state.flags["C_CONTIGUOUS"] and state.shape == (n, IMU_STATE_DOUBLES)
    b = ImuAppendBatch()
    b.n = n
    b.imu_params = imu_params
    b.state = dptr(state)
    b.t1_old_ns, b.t1_new_ns = keep[0].ctypes.data_as(_lp), keep[1].ctypes.data_as(_lp)
    b.speed_biases = dptr(keep[2])
    b.sample_begin = keep[3].ctypes.data_as(_ip)
    b.sample_t_ns = keep[4].ctypes.data_as(_lp)
    b.sample_gyr_acc = dptr(keep[5])
    return b, keep


def imu_propagate_batch(imu_params, poses, speed_biases, t_start, t_end, sample_begin, sample_t, sample_ga,
                        covariance=None, jacobian=None):
    """An okvisgpu_imu_propagate_batch over numpy arrays: (struct, arrays it points into). `poses`
    [n, 7] and `speed_biases` [n, 9] (float64, C-contiguous) are referenced, not copied (updated in
    place), and so are `covariance` / `jacobian` [n, 15, 15] when given (None = NULL)."""
    n = len(t_start)
    keep = [np.ascontiguousarray(t_start, dtype=np.int64), np.ascontiguousarray(t_end, dtype=np.int64),
            np.ascontiguousarray(sample_begin, dtype=np.int32), np.ascontiguousarray(sample_t, dtype=np.int64),
            np.ascontiguousarray(sample_ga, dtype=np.float64).reshape(-1, 6)]
    for a, shape in ((poses, (n, 7)), (speed_biases, (n, 9)), (covariance, (n, 15, 15)), (jacobian, (n, 15, 15))):
        assert a is None or (a.dtype == np.float64 and a.flags["C_CONTIGUOUS"] and a.shape == shape)
    b = ImuPropagateBatch()
    b.n = n
    b.imu_params = imu_params
    b.poses, b.speed_biases = dptr(poses), dptr(speed_biases)
    b.t_start_ns, b.t_end_ns = keep[0].ctypes.data_as(_lp), keep[1].ctypes.data_as(_lp)
    b.sample_begin = keep[2].ctypes.data_as(_ip)
    b.sample_t_ns = keep[3].ctypes.data_as(_lp)
    b.sample_gyr_acc = dptr(keep[4])
    if covariance is not None:
        b.covariance = dptr(covariance)
    if jacobian is not None:
        b.jacobian = dptr(jacobian)
    return b, keep + [poses, speed_biases, covariance, jacobian]


def gps_batch(imu_params, r_SA, poses, T_GW, measurement, information, speed_biases=None, t_k=None, t_g=None,
              sample_begin=None, sample_t=None, sample_ga=None, gw_index=None, state=None, kind=0,
              use_imu_covariance=True, redo_propagation_always=False):
    """An okvisgpu_gps_batch over numpy arrays (copied to the struct's types where they differ): (struct,
    arrays it points into). `state` [n, GPS_STATE_DOUBLES] float64 C-contiguous is referenced, not copied
    (updated in place); None = NULL (every factor fresh). `gw_index` None = NULL (block 0). kind 1 needs
    none of speed_biases, the stamps and the samples."""
    f8 = lambda a, *shape: np.ascontiguousarray(a, dtype=np.float64).reshape(*shape)
    k = {"poses": f8(poses, -1, 7), "T_GW": f8(T_GW, -1, 7), "measurement": f8(measurement, -1, 3),
         "information": f8(information, -1, 9)}
    n = len(k["poses"])
    for name, a, conv in (("speed_biases", speed_biases, lambda a: f8(a, -1, 9)),
                          ("t_k_ns", t_k, lambda a: np.ascontiguousarray(a, dtype=np.int64).reshape(-1)),
                          ("t_g_ns", t_g, lambda a: np.ascontiguousarray(a, dtype=np.int64).reshape(-1)),
                          ("sample_begin", sample_begin, lambda a: np.ascontiguousarray(a, dtype=np.int32).reshape(-1)),
                          ("sample_t_ns", sample_t, lambda a: np.ascontiguousarray(a, dtype=np.int64).reshape(-1)),
                          ("sample_gyr_acc", sample_ga, lambda a: f8(a, -1, 6)),
                          ("gw_index", gw_index, lambda a: np.ascontiguousarray(a, dtype=np.int32).reshape(-1))):
        if a is not None:
            k[name] = conv(a)
    if state is not None:
        assert state.dtype == np.float64 and state.flags["C_CONTIGUOUS"] and state.shape == (n, GPS_STATE_DOUBLES)
        k["state"] = state
    b = GpsBatch()
    b.n, b.kind, b.n_gw = n, int(kind), len(k["T_GW"])
    b.use_imu_covariance, b.redo_propagation_always = int(bool(use_imu_covariance)), int(bool(redo_propagation_always))
    b.imu_params = imu_params
    b.r_SA = (C.c_double * 3)(*[float(x) for x in r_SA])
    _set_arrays(b, k)
    return b, k


GPS_OUTPUTS = {"r": (3,), "error": (3,), "sqrt_info": (3, 3), "J_pose": (3, 6), "J_speed_bias": (3, 9), "J_T_GW": (3, 6),
               "J_pose_ambient": (3, 7), "J_T_GW_ambient": (3, 7), "steps": ()}


def lidar_deskew_batch(pose0, speed_bias0, t_start, sample_begin, sample_t, sample_ga, query_begin, query_t, ray=None,
                       pose_live=None, T_SL=None, g=9.81):
    """An okvisgpu_lidar_deskew_batch over numpy arrays (copied to the struct's types where they differ):
    (struct, arrays it points into). `ray` [n_queries, 3], `pose_live` and `T_SL` [n_scans, 7] may be None
    (NULL) when no point output is asked for; `g` is the reference's hard-coded 9.81 by default."""
    f8 = lambda a, *shape: np.ascontiguousarray(a, dtype=np.float64).reshape(*shape)
    i4 = lambda a: np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
    i8 = lambda a: np.ascontiguousarray(a, dtype=np.int64).reshape(-1)
    k = {"pose0": f8(pose0, -1, 7), "speed_bias0": f8(speed_bias0, -1, 9), "t_start_ns": i8(t_start),
         "sample_begin": i4(sample_begin), "sample_t_ns": i8(sample_t), "sample_gyr_acc": f8(sample_ga, -1, 6),
         "query_begin": i4(query_begin), "query_t_ns": i8(query_t)}
    for name, a, cols in (("ray", ray, 3), ("pose_live", pose_live, 7), ("T_SL", T_SL, 7)):
        if a is not None:
            k[name] = f8(a, -1, cols)
    b = LidarDeskewBatch()
    b.n_scans, b.g = len(k["t_start_ns"]), float(g)
    _set_arrays(b, k)
    return b, k


def voxel_downsample_batch(cloud_begin, point, voxel_size, use=None):
    """An okvisgpu_voxel_downsample_batch over numpy arrays (copied to the struct's types where they
    differ): (struct, arrays it points into). `point` [n_points, 3] float32, `voxel_size` [n_clouds],
    `use` [n_points] or None = NULL (every point)."""
    k = {"cloud_begin": np.ascontiguousarray(cloud_begin, dtype=np.int32).reshape(-1),
         "point": np.ascontiguousarray(point, dtype=np.float32).reshape(-1, 3),
         "voxel_size": np.ascontiguousarray(voxel_size, dtype=np.float64).reshape(-1)}
    if use is not None:
        k["use"] = np.ascontiguousarray(use, dtype=np.uint8).reshape(-1)
    b = VoxelDownsampleBatch()
    b.n_clouds = len(k["cloud_begin"]) - 1
    _set_arrays(b, k)
    return b, k


def frame_overlap_batch(image_begin, rows, cols, kp_begin, keypoint, landmark, job_kind, job_frame_a, job_frame_b,
                        job_radius_factor, flag=None, group_begin=None):
    """An okvisgpu_frame_overlap_batch over numpy arrays (copied to the struct's types where they differ):
    (struct, arrays it points into). `keypoint` [n_kp, 2] float32 (cv::KeyPoint::pt), `landmark` [n_kp]
    uint64 (0 = none), `flag` [n_kp] or None = NULL (kind 3 needs it), `job_frame_b` None = NULL (no job of
    kind 0 or 1), `group_begin` [n_groups + 1] or None = no groups."""
    i4 = lambda a: np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
    k = {"image_begin": i4(image_begin), "rows": i4(rows), "cols": i4(cols), "kp_begin": i4(kp_begin),
         "keypoint": np.ascontiguousarray(keypoint, dtype=np.float32).reshape(-1, 2), "job_kind": i4(job_kind),
         "job_frame_a": i4(job_frame_a),
         "job_radius_factor": np.ascontiguousarray(job_radius_factor, dtype=np.float64).reshape(-1)}
    if job_frame_b is not None:
        k["job_frame_b"] = i4(job_frame_b)
    if flag is not None:
        k["flag"] = np.ascontiguousarray(flag, dtype=np.uint8).reshape(-1)
    if group_begin is not None:
        k["group_begin"] = i4(group_begin)
    b = FrameOverlapBatch()
    b.n_frames, b.n_jobs = len(k["image_begin"]) - 1, len(k["job_kind"])
    b.n_groups = len(k["group_begin"]) - 1 if group_begin is not None else 0
    _set_arrays(b, k)
    k["landmark"] = np.ascontiguousarray(landmark, dtype=np.uint64).reshape(-1)
    b.landmark = k["landmark"].ctypes.data_as(C.POINTER(C.c_uint64))
    return b, k


def match_batch(poses, cameras, extrinsics, landmarks, landmark_quality, obs_begin, obs_pose, obs_camera,
                obs_descriptor, obs_ray, job_camera, job_pass, job_pose_prepare, job_pose_match, kp_begin, keypoint,
                descriptor, ray, ray_valid, landmark, landmark_use=None, imu_use=True, loop_closure=False,
                matching_threshold=60.0):
    """An okvisgpu_match_batch over numpy arrays (copied to the struct's types where they differ):
    (struct, arrays it points into). `cameras` is a sequence of Camera; the other arguments are the
    arrays of the header's struct, `landmark_use` None = NULL (all landmarks)."""
    f8 = lambda a, *shape: np.ascontiguousarray(a, dtype=np.float64).reshape(*shape)
    i4 = lambda a: np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
    u1 = lambda a, *shape: np.ascontiguousarray(a, dtype=np.uint8).reshape(*shape)
    cams = (Camera * max(1, len(cameras)))(*cameras)
    k = {"poses": f8(poses, -1, 7), "extrinsics": f8(extrinsics, -1, 7), "landmarks": f8(landmarks, -1, 4),
         "landmark_quality": f8(landmark_quality, -1), "obs_begin": i4(obs_begin), "obs_pose": i4(obs_pose),
         "obs_camera": i4(obs_camera), "obs_descriptor": u1(obs_descriptor, -1, 48), "obs_ray": f8(obs_ray, -1, 3),
         "job_camera": i4(job_camera), "job_pass": i4(job_pass), "job_pose_prepare": f8(job_pose_prepare, -1, 7),
         "job_pose_match": f8(job_pose_match, -1, 7), "kp_begin": i4(kp_begin), "keypoint": f8(keypoint, -1, 2),
         "descriptor": u1(descriptor, -1, 48), "ray": f8(ray, -1, 3), "ray_valid": u1(ray_valid, -1),
         "landmark": i4(landmark)}
    if landmark_use is not None:
        k["landmark_use"] = u1(landmark_use, -1)
    b = MatchBatch()
    b.n_poses, b.n_cameras, b.n_landmarks = len(k["poses"]), len(cameras), len(k["landmarks"])
    b.n_jobs = len(k["job_camera"])
    b.cameras = cams
    b.imu_use, b.loop_closure, b.matching_threshold = int(bool(imu_use)), int(bool(loop_closure)), matching_threshold
    for name, a in k.items():
        ptr = {np.dtype(np.float64): _dp, np.dtype(np.int32): _ip, np.dtype(np.uint8): _up}[a.dtype]
        setattr(b, name, a.ctypes.data_as(ptr))
    return b, (cams, k)


def frame_match_batch(cameras, job_mode, job_camera0, job_camera1, job_pose0, job_pose1, job_extrinsics0,
                      job_extrinsics1, kp0_begin, kp1_begin, keypoint0, size0, descriptor0, ray0, ray_valid0,
                      keypoint1, size1, descriptor1, ray1, ray_valid1, use0=None, use1=None, matching_threshold=60.0):
    """An okvisgpu_frame_match_batch over numpy arrays (copied to the struct's types where they differ):
    (struct, arrays it points into). `cameras` is a sequence of Camera; the other arguments are the
    arrays of the header's struct, `use0` / `use1` None = NULL (every keypoint)."""
    f8 = lambda a, *shape: np.ascontiguousarray(a, dtype=np.float64).reshape(*shape)
    i4 = lambda a: np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
    u1 = lambda a, *shape: np.ascontiguousarray(a, dtype=np.uint8).reshape(*shape)
    cams = (Camera * max(1, len(cameras)))(*cameras)
    k = {"job_mode": i4(job_mode), "job_camera0": i4(job_camera0), "job_camera1": i4(job_camera1),
         "job_pose0": f8(job_pose0, -1, 7), "job_pose1": f8(job_pose1, -1, 7),
         "job_extrinsics0": f8(job_extrinsics0, -1, 7), "job_extrinsics1": f8(job_extrinsics1, -1, 7),
         "kp0_begin": i4(kp0_begin), "kp1_begin": i4(kp1_begin)}
    for side, (kp, size, desc, ray, valid, use) in enumerate(((keypoint0, size0, descriptor0, ray0, ray_valid0, use0),
                                                              (keypoint1, size1, descriptor1, ray1, ray_valid1, use1))):
        k.update({f"keypoint{side}": f8(kp, -1, 2), f"size{side}": f8(size, -1), f"descriptor{side}": u1(desc, -1, 48),
                  f"ray{side}": f8(ray, -1, 3), f"ray_valid{side}": u1(valid, -1)})
        if use is not None:
            k[f"use{side}"] = u1(use, -1)
    b = FrameMatchBatch()
    b.n_cameras, b.n_jobs, b.cameras, b.matching_threshold = len(cameras), len(k["job_mode"]), cams, matching_threshold
    for name, a in k.items():
        ptr = {np.dtype(np.float64): _dp, np.dtype(np.int32): _ip, np.dtype(np.uint8): _up}[a.dtype]
        setattr(b, name, a.ctypes.data_as(ptr))
    return b, (cams, k)


def _set_arrays(b, arrays):
    for name, a in arrays.items():
        ptr = {np.dtype(np.float64): _dp, np.dtype(np.int32): _ip, np.dtype(np.uint8): _up, np.dtype(np.int64): _lp,
               np.dtype(np.float32): _fp}[a.dtype]
        setattr(b, name, a.ctypes.data_as(ptr))


def place_match_batch(n_cameras, kp_begin, descriptor, job_image, lm_begin, desc_begin, old_descriptor,
                      matching_threshold=60.0):
    """An okvisgpu_place_match_batch over numpy arrays (copied to the struct's types where they differ):
    (struct, arrays it points into). The arguments are the arrays of the header's struct; `job_image` is
    [n_jobs, n_cameras]."""
    i4 = lambda a: np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
    u1 = lambda a: np.ascontiguousarray(a, dtype=np.uint8).reshape(-1, 48)
    k = {"kp_begin": i4(kp_begin), "descriptor": u1(descriptor), "job_image": i4(job_image), "lm_begin": i4(lm_begin),
         "desc_begin": i4(desc_begin), "old_descriptor": u1(old_descriptor)}
    b = PlaceMatchBatch()
    b.matching_threshold, b.n_cameras = matching_threshold, int(n_cameras)
    b.n_images, b.n_jobs = len(k["kp_begin"]) - 1, len(k["lm_begin"]) - 1
    _set_arrays(b, k)
    return b, k


def place_refine_batch(cameras, extrinsics, pose, obs_begin, obs_camera, obs_keypoint, obs_sqrt_info, obs_point,
                       loss=("cauchy", 3.0), max_num_iterations=10):
    """An okvisgpu_place_refine_batch over numpy arrays (copied to the struct's types where they differ):
    (struct, arrays it points into). `cameras` is a sequence of Camera; `pose` [n_jobs, 7] (float64,
    C-contiguous) is referenced, not copied: the call refines it in place. `loss` is (kind name or id, a[, b])."""
    f8 = lambda a, *shape: np.ascontiguousarray(a, dtype=np.float64).reshape(*shape)
    i4 = lambda a: np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
    cams = (Camera * max(1, len(cameras)))(*cameras)
    k = {"extrinsics": f8(extrinsics, -1, 7), "obs_begin": i4(obs_begin), "obs_camera": i4(obs_camera),
         "obs_keypoint": f8(obs_keypoint, -1, 2), "obs_sqrt_info": f8(obs_sqrt_info, -1, 4),
         "obs_point": f8(obs_point, -1, 4)}
    n = len(k["obs_begin"]) - 1
    assert pose.dtype == np.float64 and pose.flags["C_CONTIGUOUS"] and pose.shape == (n, 7)
    b = PlaceRefineBatch()
    b.n_cameras, b.cameras, b.n_jobs, b.max_num_iterations = len(cameras), cams, n, int(max_num_iterations)
    b.loss = Loss(*loss_array([loss])[0].tolist())
    b.pose = dptr(pose)
    _set_arrays(b, k)
    return b, (cams, k, pose)


class TwoPoseBatch:
    """Owns the arrays of an okvisgpu_twopose_edges batch (TwoPoseStandardGraphError::compute inputs).

    edges: list of dicts with keys ref_pose [7], other_pose [7], landmarks [n_l,4] and
    observations: list (one per landmark) of lists of (other: bool, camera: int, keypoint [2],
    sqrt_info [4], cauchy: bool). cameras: list of Camera; extrinsics [n_cam,7]."""

    def __init__(self, edges, cameras, extrinsics):
        self.ref = np.ascontiguousarray([e["ref_pose"] for e in edges], dtype=np.float64).reshape(-1, 7)
        self.other = np.ascontiguousarray([e["other_pose"] for e in edges], dtype=np.float64).reshape(-1, 7)
        lb, lms, ob, oo, oc, kp, L, ca = [0], [], [0], [], [], [], [], []
        for e in edges:
            for l, obs in zip(e["landmarks"], e["observations"]):
                lms.append(l)
                for (other, cam, k, s, cauchy) in obs:
                    oo.append(1 if other else 0)
                    oc.append(cam)
                    kp.append(k)
                    L.append(s)
                    ca.append(1 if cauchy else 0)
                ob.append(len(oo))
            lb.append(len(lms))
        self.lb = np.asarray(lb, dtype=np.int32)
        self.lms = np.ascontiguousarray(np.asarray(lms, dtype=np.float64).reshape(-1, 4))
        self.ob = np.asarray(ob, dtype=np.int32)
        self.oo = np.asarray(oo, dtype=np.uint8)
        self.oc = np.asarray(oc, dtype=np.int32)
        self.kp = np.ascontiguousarray(np.asarray(kp, dtype=np.float64).reshape(-1, 2))
        self.L = np.ascontiguousarray(np.asarray(L, dtype=np.float64).reshape(-1, 4))
        self.ca = np.asarray(ca, dtype=np.uint8)
        self.cams = (Camera * len(cameras))(*cameras)
        self.ex = np.ascontiguousarray(extrinsics, dtype=np.float64).reshape(-1, 7)
        s = TwoPoseEdges()
        s.n_edges = len(edges)
        s.ref_pose, s.other_pose = dptr(self.ref), dptr(self.other)
        s.n_cameras = len(cameras)
        s.cameras = self.cams
        s.extrinsics = dptr(self.ex)
        s.landmark_begin = self.lb.ctypes.data_as(_ip)
        s.landmarks = dptr(self.lms)
        s.obs_begin = self.ob.ctypes.data_as(_ip)
        s.obs_other = self.oo.ctypes.data_as(_up)
        s.obs_camera = self.oc.ctypes.data_as(_ip)
        s.obs_keypoint = dptr(self.kp)
        s.obs_sqrt_info = dptr(self.L)
        s.obs_cauchy = self.ca.ctypes.data_as(_up)
        self.struct = s


class Graph:
    """An okvis Component text graph loaded into an okvisgpu problem (okvisgpu_graph_load)."""

    def __init__(self, path, cameras, imu_params):
        cams = (Camera * len(cameras))(*cameras)
        h = C.c_void_p()
        rc = lib().okvisgpu_graph_load(str(path).encode(), cams, len(cameras), C.byref(imu_params), C.byref(h))
        if rc != 0:
            raise OkvisGpuError(f"okvisgpu_graph_load({path}) failed ({rc})")
        self.handle = h

    @property
    def problem(self) -> Problem:
        pr = self.problem_ptr().contents
        pr._owner = self
        return pr

    def problem_ptr(self):
        return _owned_problem(lib().okvisgpu_graph_problem(self.handle), self)

    def ids(self):
        p = self.problem
        sid = (C.c_uint64 * p.n_poses)()
        lid = (C.c_uint64 * max(1, p.n_landmarks))()
        t = np.zeros(p.n_poses, dtype=np.int64)
        lib().okvisgpu_graph_ids(self.handle, sid, t.ctypes.data_as(_lp), lid)
        return np.array(sid[:], dtype=np.uint64), t, np.array(lid[:p.n_landmarks], dtype=np.uint64)

    def poses(self):
        p = self.problem
        return _owned_view(p.poses, (p.n_poses, 7), self)

    def landmarks(self):
        p = self.problem
        return _owned_view(p.landmarks, (p.n_landmarks, 4), self)

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                lib().okvisgpu_graph_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


def save_graph(problem_ptr, path, state_t_ns=None):
    """okvisgpu_graph_save: write a problem as an okvis Component text graph."""
    t = None if state_t_ns is None else np.ascontiguousarray(state_t_ns, dtype=np.int64).ctypes.data_as(_lp)
    rc = lib().okvisgpu_graph_save(problem_ptr, t, str(path).encode())
    if rc != 0:
        raise OkvisGpuError(f"okvisgpu_graph_save({path}) failed ({rc})")


class Context:
    """One okvisgpu_ctx (one HIP stream + device buffers) holding a batch of windows."""

    def __init__(self, device: int = 0):
        h = C.c_void_p()
        rc = lib().okvisgpu_ctx_create(device, C.byref(h))
        if rc != 0:
            raise OkvisGpuError(f"okvisgpu_ctx_create({device}) failed with status {rc}")
        self.h = h
        self._keep = None

    def _check(self, rc, what):
        if rc != 0:
            msg = lib().okvisgpu_last_error(self.h)
            raise OkvisGpuError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def set_problems(self, problems):
        arr = (Problem * len(problems))(*problems)
        self._keep = None
        self._check(lib().okvisgpu_set_problems(self.h, arr, len(problems)), "okvisgpu_set_problems")
        self._keep = (arr, list(problems))

    def update_params(self):
        self._check(lib().okvisgpu_update_params(self.h), "okvisgpu_update_params")

    def set_block_constant(self, window, kind, index, is_constant):
        self._check(lib().okvisgpu_set_block_constant(self.h, window, kind, index, int(is_constant)),
                    "okvisgpu_set_block_constant")

    def _n_windows(self, n_windows):
        """Summaries are written for every window of the context (okvisgpu_solve / _solve_end fill
        [n_windows] entries), so the buffer is sized from the problems held, never smaller."""
        if self._keep is None:
            raise OkvisGpuError("no problem set")
        n = len(self._keep[1])
        if n_windows is not None and n_windows != n:
            raise ValueError(f"n_windows={n_windows} but the context holds {n} windows")
        return n

    def solve(self, options: Optional[Options] = None, n_windows: Optional[int] = None):
        o = options or default_options()
        sums = (Summary * self._n_windows(n_windows))()
        self._check(lib().okvisgpu_solve(self.h, C.byref(o), sums), "okvisgpu_solve")
        return [s.as_dict() for s in sums]

    def solve_begin(self, options: Options):
        self._opts = options
        self._check(lib().okvisgpu_solve_begin(self.h, C.byref(options)), "okvisgpu_solve_begin")

    def solve_iterate(self, n: int):
        self._check(lib().okvisgpu_solve_iterate(self.h, n), "okvisgpu_solve_iterate")

    def synchronize(self):
        self._check(lib().okvisgpu_synchronize(self.h), "okvisgpu_synchronize")

    def solve_end(self, n_windows: Optional[int] = None):
        sums = (Summary * self._n_windows(n_windows))()
        self._check(lib().okvisgpu_solve_end(self.h, sums), "okvisgpu_solve_end")
        return [s.as_dict() for s in sums]

    def profile_iteration(self):
        ms = np.zeros(N_PHASES)
        self._check(lib().okvisgpu_profile_iteration(self.h, dptr(ms)), "okvisgpu_profile_iteration")
        return {lib().okvisgpu_phase_name(i).decode(): float(ms[i]) for i in range(N_PHASES)}

    def time_kernel(self, name, reps=5):
        """(avg_ms, work, bound) of one iteration's launches of kernel `name` (see include/okvisgpu.h)."""
        names = kernel_names()
        k = names.index(name)
        ms, work, bound = C.c_double(), C.c_double(), C.c_int32()
        self._check(lib().okvisgpu_time_kernel(self.h, k, reps, C.byref(ms), C.byref(work), C.byref(bound)),
                    "okvisgpu_time_kernel")
        return ms.value, work.value, ("hbm", "mfma")[bound.value]

    def stats(self):
        st = ProblemStats()
        self._check(lib().okvisgpu_get_stats(self.h, C.byref(st)), "okvisgpu_get_stats")
        return st.as_dict()

    def get_params(self):
        self._check(lib().okvisgpu_get_params(self.h), "okvisgpu_get_params")

    def evaluate(self, window=0):
        c = C.c_double()
        self._check(lib().okvisgpu_evaluate(self.h, window, C.byref(c)), "okvisgpu_evaluate")
        return c.value

    def linearize_reduce(self, window=0, jacobi_scaling=True, mu=0.0, dim_hint=None):
        dim = C.c_int32()
        cost = C.c_double()
        self._check(lib().okvisgpu_linearize_reduce(self.h, window, int(jacobi_scaling), mu, None, None,
                                                     C.byref(cost), C.byref(dim)), "linearize_reduce(dim)")
        n = dim.value
        S = np.zeros((n, n))
        rhs = np.zeros(n)
        self._check(lib().okvisgpu_linearize_reduce(self.h, window, int(jacobi_scaling), mu, dptr(S), dptr(rhs),
                                                     C.byref(cost), C.byref(dim)), "linearize_reduce")
        return S, rhs, cost.value

    def gauss_newton_step(self, window=0, options: Optional[Options] = None, mu=0.0):
        """okvisgpu_gauss_newton_step (development): (y_f [dim], y_l [n_landmarks, 3]) of one Gauss-Newton
        solve of `window` at the current parameters: y_f solves the system linearize_reduce(window,
        options.jacobi_scaling, mu) returns, y_l are the landmarks' back-substituted steps in the
        caller's order. Raises OkvisGpuError (status OKVISGPU_ERR_NUMERICAL) when the step failed."""
        if self._keep is None:
            raise OkvisGpuError("no problem set")
        o = C.byref(options) if options is not None else None
        dim = C.c_int32()
        self._check(lib().okvisgpu_gauss_newton_step(self.h, window, o, mu, None, None, C.byref(dim)),
                    "gauss_newton_step(dim)")
        y_f = np.zeros(dim.value)
        y_l = np.zeros((self._keep[1][window].n_landmarks, 3))
        self._check(lib().okvisgpu_gauss_newton_step(self.h, window, o, mu, dptr(y_f), dptr(y_l), C.byref(dim)),
                    "gauss_newton_step")
        return y_f, y_l

    def eval_reprojection(self, n_obs, window=0):
        r = np.zeros((n_obs, 2))
        Jp = np.zeros((n_obs, 2, 6))
        Jl = np.zeros((n_obs, 2, 3))
        self._check(lib().okvisgpu_eval_reprojection(self.h, window, dptr(r), dptr(Jp), dptr(Jl)),
                    "eval_reprojection")
        return r, Jp, Jl

    def eval_imu(self, n_imu, window=0, redo_always=False):
        r = np.zeros((n_imu, 15))
        J = np.zeros((n_imu, 15, 30))
        self._check(lib().okvisgpu_eval_imu(self.h, window, int(redo_always), dptr(r), dptr(J)), "eval_imu")
        return r, J

    def eval_relpose(self, n_relpose, window=0):
        r = np.zeros((n_relpose, 6))
        J = np.zeros((n_relpose, 6, 12))
        self._check(lib().okvisgpu_eval_relpose(self.h, window, dptr(r), dptr(J)), "eval_relpose")
        return r, J

    def eval_host(self, n_host, window=0):
        """Host-evaluated factors through the device path (gather, callback, upload), no loss:
        r [n, 15], minimal J [n, 15, 30] in the IMU column layout."""
        r = np.zeros((n_host, 15))
        J = np.zeros((n_host, 15, 30))
        self._check(lib().okvisgpu_eval_host(self.h, window, dptr(r), dptr(J)), "eval_host")
        return r, J

    def imu_append(self, imu_params, state, t1_old, t1_new, speed_biases, sample_begin, sample_t, sample_ga):
        """okvisgpu_imu_append (ImuError::append for a batch): `state` [n, IMU_STATE_DOUBLES] is updated
        in place; returns the integrated steps per factor (-1: samples do not reach t1_new)."""
        b, keep = imu_append_batch(imu_params, state, t1_old, t1_new, speed_biases, sample_begin, sample_t,
                                   sample_ga)
        steps = np.zeros(b.n, dtype=np.int32)
        self._check(lib().okvisgpu_imu_append(self.h, C.byref(b), steps.ctypes.data_as(_ip)), "okvisgpu_imu_append")
        return steps

    def imu_propagate(self, imu_params, poses, speed_biases, t_start, t_end, sample_begin, sample_t, sample_ga,
                      covariance=False, jacobian=False):
        """okvisgpu_imu_propagate (ImuError::propagation for a batch): `poses` [n, 7] and `speed_biases`
        [n, 9] are updated in place; returns the integrated steps per item (-1: samples do not reach
        t_end, item untouched), followed by the covariance and / or the Jacobian [n, 15, 15] when
        requested. `covariance` / `jacobian` may also be arrays to write into (rows of items with -1
        steps keep their contents)."""
        n = len(t_start)
        P = np.zeros((n, 15, 15)) if covariance is True else (None if covariance is False else covariance)
        J = np.zeros((n, 15, 15)) if jacobian is True else (None if jacobian is False else jacobian)
        b, keep = imu_propagate_batch(imu_params, poses, speed_biases, t_start, t_end, sample_begin, sample_t,
                                      sample_ga, P, J)
        steps = np.zeros(n, dtype=np.int32)
        self._check(lib().okvisgpu_imu_propagate(self.h, C.byref(b), steps.ctypes.data_as(_ip)),
                    "okvisgpu_imu_propagate")
        out = (steps,) + ((P,) if P is not None else ()) + ((J,) if J is not None else ())
        return out[0] if len(out) == 1 else out

    def gps_evaluate(self, batch: GpsBatch, fill=None, outputs=None):
        """okvisgpu_gps_evaluate (GpsErrorAsynchronous / GpsErrorSynchronous for a batch of factors) for a
        batch built by gps_batch(): dict of r, error [n, 3], sqrt_info [n, 3, 3], J_pose, J_T_GW [n, 3, 6],
        J_speed_bias [n, 3, 9], J_pose_ambient, J_T_GW_ambient [n, 3, 7] and steps [n] (int32); the batch's
        `state` is updated in place. `outputs` names the outputs to ask for (the others are passed as NULL
        and left out of the dict; default: all); `fill` (a float, e.g. NaN) pre-fills the float arrays the
        call writes into, and steps with -7."""
        n = batch.n
        names = list(GPS_OUTPUTS) if outputs is None else list(outputs)
        out = {k: (np.full(n, 0 if fill is None else -7, dtype=np.int32) if k == "steps" else
                   np.full((n,) + GPS_OUTPUTS[k], 0.0 if fill is None else float(fill))) for k in names}
        r = GpsResult()
        _set_arrays(r, out)
        self._check(lib().okvisgpu_gps_evaluate(self.h, C.byref(batch), C.byref(r)), "okvisgpu_gps_evaluate")
        return out

    def lidar_deskew(self, batch: LidarDeskewBatch, fill=None, outputs=None):
        """okvisgpu_lidar_deskew (LidarMotionUndistortion::deskew and the per-ray states of
        Trajectory::getStates) for a batch built by lidar_deskew_batch(): dict of valid [n_queries] (uint8),
        point [n_queries, 3] (float32), point_f64 [n_queries, 3], pose [n_queries, 7], speed, omega_S
        [n_queries, 3], n_before [n_scans]. `outputs` names the outputs to ask for (the others are passed as
        NULL and left out of the dict; default: all, without the points when the batch has no rays); `fill`
        (a dict of per-output values) pre-fills the arrays the call writes into."""
        n = batch.n_scans
        nq = int(batch.query_begin[n]) if batch.query_begin and n > 0 else 0
        spec = {"valid": ((nq,), np.uint8), "point": ((nq, 3), np.float32), "point_f64": ((nq, 3), np.float64),
                "pose": ((nq, 7), np.float64), "speed": ((nq, 3), np.float64), "omega_S": ((nq, 3), np.float64),
                "n_before": ((n,), np.int32)}
        if outputs is None:
            outputs = [k for k in spec if batch.ray or k not in ("point", "point_f64")]
        out = {k: np.full(spec[k][0], (fill or {}).get(k, 0), dtype=spec[k][1]) for k in spec if k in outputs}
        r = LidarDeskewResult()
        _set_arrays(r, out)
        self._check(lib().okvisgpu_lidar_deskew(self.h, C.byref(batch), C.byref(r)), "okvisgpu_lidar_deskew")
        return out

    def voxel_downsample(self, batch: VoxelDownsampleBatch, fill=None):
        """okvisgpu_voxel_downsample (VoxelDownSample<float>) for a batch built by voxel_downsample_batch():
        dict of keep [n_points] (uint8: the first point, in input order, of its voxel) and n_kept [n_clouds].
        `fill` (a dict of per-output values) pre-fills the arrays the call writes into."""
        n = batch.n_clouds
        npts = int(batch.cloud_begin[n]) if batch.cloud_begin and n > 0 else 0
        out = {"keep": np.full(npts, (fill or {}).get("keep", 0), dtype=np.uint8),
               "n_kept": np.full(n, (fill or {}).get("n_kept", 0), dtype=np.int32)}
        r = VoxelDownsampleResult()
        _set_arrays(r, out)
        self._check(lib().okvisgpu_voxel_downsample(self.h, C.byref(batch), C.byref(r)), "okvisgpu_voxel_downsample")
        return out

    def frame_overlap(self, batch: FrameOverlapBatch, fill=None):
        """okvisgpu_frame_overlap (ViSlamBackend::overlapFraction / trackingQuality and both parts of
        Frontend::doWeNeedANewKeyframe) for a batch built by frame_overlap_batch(): dict of overlap [n_jobs],
        count [n_jobs, 4] (I, U of side A, I, U of side B), n_matched [n_jobs, 2], n_keypoints [n_jobs],
        group_best [n_groups] (a job index or -1) and group_max [n_groups]. `fill` (a dict of per-output
        values) pre-fills the arrays the call writes into."""
        nj, ng = batch.n_jobs, batch.n_groups
        spec = {"overlap": ((nj,), np.float64), "count": ((nj, 4), np.int32), "n_matched": ((nj, 2), np.int32),
                "n_keypoints": ((nj,), np.int32), "group_best": ((ng,), np.int32), "group_max": ((ng,), np.float64)}
        out = {k: np.full(shape, (fill or {}).get(k, 0), dtype=dt) for k, (shape, dt) in spec.items()}
        r = FrameOverlapResult()
        _set_arrays(r, out)
        self._check(lib().okvisgpu_frame_overlap(self.h, C.byref(batch), C.byref(r)), "okvisgpu_frame_overlap")
        return out

    def match_to_map(self, batch: MatchBatch, fill=None):
        """okvisgpu_match_to_map (Frontend::matchToMap's candidate preparation and both matching passes)
        for a batch built by match_batch(): dict of match_landmark, match_distance, n_records
        [n_kp], record_repr_sum [n_kp], point [n_kp, 4], cand_n, cand_is3d [n_jobs, n_landmarks], cand_obs
        [.., 3], cand_projection [.., 2]. `fill` (a dict of per-output values) pre-fills the arrays
        the call writes into."""
        nj, nl = batch.n_jobs, batch.n_landmarks
        nk = int(batch.kp_begin[nj]) if batch.kp_begin else 0
        spec = {"match_landmark": ((nk,), np.int32), "match_distance": ((nk,), np.int32), "n_records": ((nk,), np.int32),
                "record_repr_sum": ((nk,), np.float64), "point": ((nk, 4), np.float64), "cand_n": ((nj, nl), np.int32),
                "cand_is3d": ((nj, nl), np.uint8), "cand_obs": ((nj, nl, 3), np.int32),
                "cand_projection": ((nj, nl, 2), np.float64)}
        out = {k: np.full(shape, (fill or {}).get(k, 0), dtype=dt) for k, (shape, dt) in spec.items()}
        r = MatchResult()
        for k, a in out.items():
            setattr(r, k, a.ctypes.data_as({np.dtype(np.float64): _dp, np.dtype(np.int32): _ip,
                                            np.dtype(np.uint8): _up}[a.dtype]))
        self._check(lib().okvisgpu_match_to_map(self.h, C.byref(batch), C.byref(r)), "okvisgpu_match_to_map")
        return out

    def match_frames(self, batch: FrameMatchBatch, fill=None):
        """okvisgpu_match_frames (the matching loops of Frontend::matchMotionStereo and ::matchStereo) for a
        batch built by frame_match_batch(): dict of match, distance [n_kp0], point [n_kp0, 4],
        initialisable [n_kp0] (uint8), quality [n_kp0]. `fill` (a dict of per-output values) pre-fills
        the arrays the call writes into."""
        nk = int(batch.kp0_begin[batch.n_jobs]) if batch.kp0_begin else 0
        spec = {"match": ((nk,), np.int32), "distance": ((nk,), np.int32), "point": ((nk, 4), np.float64),
                "initialisable": ((nk,), np.uint8), "quality": ((nk,), np.float64)}
        out = {k: np.full(shape, (fill or {}).get(k, 0), dtype=dt) for k, (shape, dt) in spec.items()}
        r = FrameMatchResult()
        for k, a in out.items():
            setattr(r, k, a.ctypes.data_as({np.dtype(np.float64): _dp, np.dtype(np.int32): _ip,
                                            np.dtype(np.uint8): _up}[a.dtype]))
        self._check(lib().okvisgpu_match_frames(self.h, C.byref(batch), C.byref(r)), "okvisgpu_match_frames")
        return out

    def place_match(self, batch: PlaceMatchBatch, fill=None):
        """okvisgpu_place_match (the descriptor matching of Frontend::verifyRecognisedPlace) for a batch built
        by place_match_batch(): dict of match_keypoint, match_distance [n_lm, n_cameras], job_matches
        [n_jobs]. `fill` (a dict of per-output values) pre-fills the arrays the call writes into."""
        nj, nc = batch.n_jobs, batch.n_cameras
        nl = int(batch.lm_begin[nj]) if batch.lm_begin else 0
        spec = {"match_keypoint": (nl, nc), "match_distance": (nl, nc), "job_matches": (nj,)}
        out = {k: np.full(shape, (fill or {}).get(k, 0), dtype=np.int32) for k, shape in spec.items()}
        r = PlaceMatchResult()
        _set_arrays(r, out)
        self._check(lib().okvisgpu_place_match(self.h, C.byref(batch), C.byref(r)), "okvisgpu_place_match")
        return out

    def place_refine(self, batch: PlaceRefineBatch, fill=None):
        """okvisgpu_place_refine (the pose refinement of Frontend::verifyRecognisedPlace and the evaluation
        after it) for a batch built by place_refine_batch(): the batch's `pose` array is refined in place;
        dict of H [n_jobs, 6, 6], n_outliers, initial_cost, final_cost, num_iterations,
        num_successful_steps, num_unsuccessful_steps, termination_type [n_jobs]. `fill` (a dict of
        per-output values) pre-fills the arrays the call writes into."""
        n = batch.n_jobs
        spec = {"H": ((n, 6, 6), np.float64), "n_outliers": ((n,), np.int32), "initial_cost": ((n,), np.float64),
                "final_cost": ((n,), np.float64), "num_iterations": ((n,), np.int32),
                "num_successful_steps": ((n,), np.int32), "num_unsuccessful_steps": ((n,), np.int32),
                "termination_type": ((n,), np.int32)}
        out = {k: np.full(shape, (fill or {}).get(k, 0), dtype=dt) for k, (shape, dt) in spec.items()}
        r = PlaceRefineResult()
        _set_arrays(r, out)
        self._check(lib().okvisgpu_place_refine(self.h, C.byref(batch), C.byref(r)), "okvisgpu_place_refine")
        return out

    def twopose_compute(self, edges: "TwoPoseBatch"):
        """TwoPoseStandardGraphError::compute for every edge of the batch: dict of DeltaX_ [n,6],
        J_ [n,6,6], linearisation point [n,7], H00_ [n,6,6], b0_ [n,6]."""
        n = edges.struct.n_edges
        out = {"delta_x": np.zeros((n, 6)), "sqrt_info": np.zeros((n, 6, 6)), "lin_point": np.zeros((n, 7)),
               "H00": np.zeros((n, 6, 6)), "b0": np.zeros((n, 6))}
        self._check(lib().okvisgpu_twopose_compute(self.h, C.byref(edges.struct), dptr(out["delta_x"]),
                                                   dptr(out["sqrt_info"]), dptr(out["lin_point"]), dptr(out["H00"]),
                                                   dptr(out["b0"])), "okvisgpu_twopose_compute")
        return out

    def twopose_extrinsics_compute(self, edges: "TwoPoseBatch", out=None):
        """TwoPoseExtrinsicsGraphError::compute (the edge of do_extrinsics: true) for every edge of the
        batch, D = 6 + 6 n_cameras: dict of DeltaX_ [n,D], J_ [n,D,D], linearisation point [n,7],
        camera_seen [n,C] (uint8), H00_ [n,D,D], b0_ [n,D]. `out` may be such a dict to write into."""
        n, nc = edges.struct.n_edges, edges.struct.n_cameras
        D = 6 + 6 * nc
        if out is None:
            out = {"delta_x": np.zeros((n, D)), "sqrt_info": np.zeros((n, D, D)), "lin_point": np.zeros((n, 7)),
                   "camera_seen": np.zeros((n, nc), dtype=np.uint8), "H00": np.zeros((n, D, D)), "b0": np.zeros((n, D))}
        self._check(lib().okvisgpu_twopose_extrinsics_compute(
            self.h, C.byref(edges.struct), dptr(out["delta_x"]), dptr(out["sqrt_info"]), dptr(out["lin_point"]),
            out["camera_seen"].ctypes.data_as(_up), dptr(out["H00"]), dptr(out["b0"])),
            "okvisgpu_twopose_extrinsics_compute")
        return out

    def twopose_extrinsics_evaluate(self, ref_pose, other_pose, extrinsics, edges, lin_extrinsics,
                                    want=("r", "J_ref", "J_other", "J_extrinsics")):
        """TwoPoseExtrinsicsGraphError::EvaluateWithMinimalJacobians for a batch of computed edges.
        ref_pose / other_pose [n,7] and extrinsics [C,7] are the values to evaluate at, `edges` the dict
        twopose_extrinsics_compute returned, lin_extrinsics [n,C,7] (or [C,7] for all edges) the
        extrinsics the edges were computed with. Returns a dict of the outputs named in `want`:
        r [n,D], J_ref / J_other [n,D,6], J_extrinsics [n,C,D,6] (minimal, row-major)."""
        ref = np.ascontiguousarray(ref_pose, dtype=np.float64).reshape(-1, 7)
        oth = np.ascontiguousarray(other_pose, dtype=np.float64).reshape(-1, 7)
        ex = np.ascontiguousarray(extrinsics, dtype=np.float64).reshape(-1, 7)
        n, nc = len(ref), len(ex)
        D = 6 + 6 * nc
        lex = np.asarray(lin_extrinsics, dtype=np.float64)
        lex = np.ascontiguousarray(np.broadcast_to(lex.reshape(-1, nc, 7) if nc else lex.reshape(-1, 0, 7), (n, nc, 7)))
        dx = np.ascontiguousarray(edges["delta_x"], dtype=np.float64).reshape(n, D)
        J = np.ascontiguousarray(edges["sqrt_info"], dtype=np.float64).reshape(n, D, D)
        lin = np.ascontiguousarray(edges["lin_point"], dtype=np.float64).reshape(n, 7)
        seen = np.ascontiguousarray(edges["camera_seen"], dtype=np.uint8).reshape(n, nc)
        s = TwoPoseExtrinsicsEval()
        s.n_edges, s.n_cameras = n, nc
        s.ref_pose, s.other_pose, s.extrinsics = dptr(ref), dptr(oth), dptr(ex)
        s.delta_x, s.sqrt_info, s.lin_point, s.lin_extrinsics = dptr(dx), dptr(J), dptr(lin), dptr(lex)
        s.camera_seen = seen.ctypes.data_as(_up)
        shapes = {"r": (n, D), "J_ref": (n, D, 6), "J_other": (n, D, 6), "J_extrinsics": (n, nc, D, 6)}
        out = {k: np.zeros(shapes[k]) for k in want}
        ptr = [dptr(out[k]) if k in out else None for k in ("r", "J_ref", "J_other", "J_extrinsics")]
        self._check(lib().okvisgpu_twopose_extrinsics_evaluate(self.h, C.byref(s), *ptr),
                    "okvisgpu_twopose_extrinsics_evaluate")
        return out

    def update_landmarks(self, n_windows: Optional[int] = None):
        """okvisgpu_update_landmarks (ViGraph::updateLandmarks on the current device values): one dict
        per window with quality [n_landmarks], initialised / reset [n_landmarks] (bool), obs_error
        [n_observations], n_initialised, n_reset and in_front (bool), in the caller's indices. A reset
        landmark is re-placed on the device and in the window's `landmarks` array."""
        n = self._n_windows(n_windows)
        ups = (LandmarkUpdate * n)()
        out = []
        for u, p in zip(ups, self._keep[1]):
            d = {"quality": np.zeros(p.n_landmarks), "initialised": np.zeros(p.n_landmarks, dtype=np.uint8),
                 "reset": np.zeros(p.n_landmarks, dtype=np.uint8), "obs_error": np.zeros(p.n_observations)}
            u.quality, u.obs_error = dptr(d["quality"]), dptr(d["obs_error"])
            u.initialised, u.reset = d["initialised"].ctypes.data_as(_up), d["reset"].ctypes.data_as(_up)
            out.append(d)
        self._check(lib().okvisgpu_update_landmarks(self.h, ups), "okvisgpu_update_landmarks")
        for u, d in zip(ups, out):
            d["initialised"], d["reset"] = d["initialised"].astype(bool), d["reset"].astype(bool)
            d["n_initialised"], d["n_reset"], d["in_front"] = int(u.n_initialised), int(u.n_reset), bool(u.in_front)
        return out

    def covisibilities(self, excluded=None, n_windows: Optional[int] = None):
        """okvisgpu_covisibilities (ViGraph::computeCovisibilities on the structure of the last
        set_problems): one dict per window with counts [S, S] (int32, symmetric, zero diagonal),
        n_observed [S], visible [S] (bool), n_pairs, n_visible, any (bool) and path (0 window in LDS,
        1 tiled), in the caller's pose indices. `excluded`: None, or per window None or a
        [n_landmarks] mask of the landmarks to leave out (a single array for a single window)."""
        n = self._n_windows(n_windows)
        if excluded is None:
            excluded = [None] * n
        elif n == 1 and not isinstance(excluded, (list, tuple)):
            excluded = [excluded]
        if len(excluded) != n:
            raise ValueError(f"{len(excluded)} exclusion masks for {n} windows")
        vs = (Covisibility * n)()
        out, keep = [], []
        for v, p, ex in zip(vs, self._keep[1], excluded):
            S = p.n_poses
            d = {"counts": np.zeros((S, S), dtype=np.int32), "n_observed": np.zeros(S, dtype=np.int32),
                 "visible": np.zeros(S, dtype=np.uint8)}
            if ex is not None:
                ex = np.ascontiguousarray(np.asarray(ex) != 0, dtype=np.uint8)
                if ex.shape != (p.n_landmarks,):
                    raise ValueError(f"exclusion mask of shape {ex.shape} for {p.n_landmarks} landmarks")
                keep.append(ex)
                v.landmark_excluded = ex.ctypes.data_as(_up)
            v.counts, v.n_observed = d["counts"].ctypes.data_as(_ip), d["n_observed"].ctypes.data_as(_ip)
            v.visible = d["visible"].ctypes.data_as(_up)
            out.append(d)
        self._check(lib().okvisgpu_covisibilities(self.h, vs), "okvisgpu_covisibilities")
        for v, d in zip(vs, out):
            d["visible"] = d["visible"].astype(bool)
            d["n_pairs"], d["n_visible"], d["any"], d["path"] = int(v.n_pairs), int(v.n_visible), bool(v.any), int(v.path)
        return out

    def close(self):
        if getattr(self, "h", None):
            lib().okvisgpu_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def kernel_names():
    return [lib().okvisgpu_kernel_name(i).decode() for i in range(lib().okvisgpu_kernel_count())]


def device_count() -> int:
    n = C.c_int32(0)
    rc = lib().okvisgpu_device_count(C.byref(n))
    return n.value if rc == 0 else 0
