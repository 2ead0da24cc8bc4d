"""ctypes binding of libdvo.so (include/dvo.h): the MI355X-native direct-VO hot path.

The names mirror the reference's interface for this path (include/system/system.hpp, include/track/*.hpp,
include/map/implement.hpp, include/core/{convert,transform}.hpp) so the parity tests read like the
reference's own demos.  There is NO CPU fallback: if lib/libdvo.so is missing, or no GPU is visible when a
compute entry point is called, this raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DVO_LIB_PATH") or os.path.join(os.path.dirname(_HERE), "lib", "libdvo.so")  # (override: A/B runs of two builds)
INVALID = np.float32(-2.0)
MAX_LEVELS = 8
MAX_ITERATIONS = 32
FP = C.POINTER(C.c_float)


class DvoError(RuntimeError):
    pass


# status codes of include/dvo.h
DVO_OK, DVO_ERR_BAD_ARGUMENT, DVO_ERR_HIP, DVO_ERR_NO_DEVICE, DVO_ERR_NO_VALID_PIXELS, DVO_ERR_NOT_READY, DVO_ERR_OUT_OF_MEMORY = range(7)


class Config(C.Structure):
    _fields_ = [("max_iterations", C.c_int), ("min_update", C.c_float), ("min_residual", C.c_float),
                ("fixed_iterations", C.c_int), ("crop_enable", C.c_int), ("step_default", C.c_float),
                ("step_level1", C.c_float), ("step_level2", C.c_float), ("sigma_min", C.c_float),
                ("sigma_max", C.c_float), ("min_depth", C.c_float), ("keyframe_min_translation", C.c_float),
                ("keyframe_max_frames", C.c_int), ("rng_seed", C.c_uint32), ("device", C.c_int),
                ("stream", C.c_void_p), ("profile", C.c_int), ("gn_pixels_per_thread", C.c_int),
                ("gn_use_lds_patch", C.c_int), ("gn_gather_group", C.c_int), ("track_streams", C.c_int), ("track_adaptive", C.c_int), ("track_fused_tiles", C.c_int),
                ("track_single_launch", C.c_int)]


class TrackLog(C.Structure):
    _fields_ = [("levels", C.c_int), ("n_iter", C.c_int * MAX_LEVELS),
                ("residual", (C.c_float * MAX_ITERATIONS) * MAX_LEVELS),
                ("update_norm", (C.c_float * MAX_ITERATIONS) * MAX_LEVELS),
                ("n_valid", (C.c_int * MAX_ITERATIONS) * MAX_LEVELS),
                ("xi_after", ((C.c_float * 6) * MAX_ITERATIONS) * MAX_LEVELS),
                ("xi_update", ((C.c_float * 6) * MAX_ITERATIONS) * MAX_LEVELS)]

    def to_dict(self):
        L = self.levels
        out = dict(n_iter=[self.n_iter[l] for l in range(L)], residual=[], upd_norm=[], n_valid=[], xi_after=[], xi_update=[])
        for l in range(L):
            n = self.n_iter[l]
            out["xi_update"].append(np.array([self.xi_update[l][i][:] for i in range(n)], np.float32).reshape(n, 6))
            out["residual"].append(np.array(self.residual[l][:n], np.float32))
            out["upd_norm"].append(np.array(self.update_norm[l][:n], np.float32))
            out["n_valid"].append(np.array(self.n_valid[l][:n], np.int32))
            out["xi_after"].append(np.array([self.xi_after[l][i][:] for i in range(n)], np.float32).reshape(n, 6))
        return out


class GnResult(C.Structure):
    _fields_ = [("H", C.c_double * 21), ("g", C.c_double * 6), ("sum_r2", C.c_double), ("n_valid", C.c_int),
                ("xi_update", C.c_float * 6), ("residual", C.c_float), ("xi_next", C.c_float * 6)]


class TrackQuality(C.Structure):
    """dvo_track_quality (include/dvo.h): one sequence's tracking-quality record of the last push / call."""
    _fields_ = [("struct_size", C.c_int), ("status", C.c_int), ("flags", C.c_int), ("n_valid", C.c_int),
                ("n_iter", C.c_int * MAX_LEVELS), ("residual", C.c_float), ("update_norm", C.c_float), ("sum_r2", C.c_double),
                ("H", C.c_double * 21), ("g", C.c_double * 6), ("eigenvalues", C.c_double * 6), ("covariance", C.c_double * 21)]


# the same layout as a numpy structured dtype (Batch / MonoBatch .last_track_quality)
TRACK_QUALITY_DTYPE = np.dtype({"names": [f[0] for f in TrackQuality._fields_],
                                "formats": ["<i4", "<i4", "<i4", "<i4", ("<i4", (MAX_LEVELS,)), "<f4", "<f4", "<f8",
                                            ("<f8", (21,)), ("<f8", (6,)), ("<f8", (6,)), ("<f8", (21,))],
                                "offsets": [getattr(TrackQuality, f[0]).offset for f in TrackQuality._fields_],
                                "itemsize": C.sizeof(TrackQuality)})


class RobustConfig(C.Structure):
    """dvo_robust_config (include/dvo.h): robust residual weights of a batch."""
    _fields_ = [("struct_size", C.c_int), ("kind", C.c_int), ("scale_mode", C.c_int), ("param", C.c_float), ("scale_floor", C.c_float)]


class AffineConfig(C.Structure):
    """dvo_affine_config (include/dvo.h): affine brightness compensation of a batch."""
    _fields_ = [("struct_size", C.c_int), ("mode", C.c_int), ("min_pixels", C.c_int), ("min_contrast", C.c_float),
                ("gain_min", C.c_float), ("gain_max", C.c_float)]


class AffineLog(C.Structure):
    """dvo_affine_log (include/dvo.h): the (a, b) every logged iteration used, indexed like TrackLog."""
    _fields_ = [("struct_size", C.c_int), ("levels", C.c_int), ("n_iter", C.c_int * MAX_LEVELS),
                ("a", (C.c_float * MAX_ITERATIONS) * MAX_LEVELS), ("b", (C.c_float * MAX_ITERATIONS) * MAX_LEVELS),
                ("prime_a", C.c_float), ("prime_b", C.c_float)]


AFFINE_LOG_DTYPE = np.dtype({"names": [f[0] for f in AffineLog._fields_],
                             "formats": [np.int32, np.int32, (np.int32, MAX_LEVELS), (np.float32, (MAX_LEVELS, MAX_ITERATIONS)),
                                         (np.float32, (MAX_LEVELS, MAX_ITERATIONS)), np.float32, np.float32],
                             "offsets": [getattr(AffineLog, f[0]).offset for f in AffineLog._fields_],
                             "itemsize": C.sizeof(AffineLog)})


class RobustLog(C.Structure):
    """dvo_robust_log (include/dvo.h): the median scale's s2, median bin and count of every logged iteration, indexed like TrackLog."""
    _fields_ = [("struct_size", C.c_int), ("levels", C.c_int), ("n_iter", C.c_int * MAX_LEVELS),
                ("s2", (C.c_float * MAX_ITERATIONS) * MAX_LEVELS), ("median_bin", (C.c_int * MAX_ITERATIONS) * MAX_LEVELS),
                ("count", (C.c_int * MAX_ITERATIONS) * MAX_LEVELS), ("prime_bin", C.c_int), ("prime_count", C.c_int)]


ROBUST_LOG_DTYPE = np.dtype({"names": [f[0] for f in RobustLog._fields_],
                             "formats": [np.int32, np.int32, (np.int32, MAX_LEVELS), (np.float32, (MAX_LEVELS, MAX_ITERATIONS)),
                                         (np.int32, (MAX_LEVELS, MAX_ITERATIONS)), (np.int32, (MAX_LEVELS, MAX_ITERATIONS)),
                                         np.int32, np.int32],
                             "offsets": [getattr(RobustLog, f[0]).offset for f in RobustLog._fields_],
                             "itemsize": C.sizeof(RobustLog)})


class GeometricConfig(C.Structure):
    """dvo_geometric_config (include/dvo.h): the geometric (depth) term of a sensor-depth batch."""
    _fields_ = [("struct_size", C.c_int), ("mode", C.c_int), ("weight", C.c_float), ("max_diff", C.c_float)]


class GeometricRecord(C.Structure):
    """dvo_geometric_record (include/dvo.h): n_geo and S29 / n_geo of the finest level's last iteration."""
    _fields_ = [("n_geo", C.c_int), ("mean_sq", C.c_float)]


class GeometricLog(C.Structure):
    """dvo_geometric_log (include/dvo.h): n_geo and (float)S29 of every logged iteration, indexed like TrackLog."""
    _fields_ = [("struct_size", C.c_int), ("levels", C.c_int), ("n_iter", C.c_int * MAX_LEVELS),
                ("n_geo", (C.c_int * MAX_ITERATIONS) * MAX_LEVELS), ("sum_sq", (C.c_float * MAX_ITERATIONS) * MAX_LEVELS)]


GEOMETRIC_RECORD_DTYPE = np.dtype([("n_geo", np.int32), ("mean_sq", np.float32)])
GEOMETRIC_LOG_DTYPE = np.dtype({"names": [f[0] for f in GeometricLog._fields_],
                                "formats": [np.int32, np.int32, (np.int32, MAX_LEVELS), (np.int32, (MAX_LEVELS, MAX_ITERATIONS)),
                                            (np.float32, (MAX_LEVELS, MAX_ITERATIONS))],
                                "offsets": [getattr(GeometricLog, f[0]).offset for f in GeometricLog._fields_],
                                "itemsize": C.sizeof(GeometricLog)})


class LmConfig(C.Structure):
    """dvo_lm_config (include/dvo.h): step control (damped Gauss-Newton with step acceptance) of a batch."""
    _fields_ = [("struct_size", C.c_int), ("mode", C.c_int), ("lambda0", C.c_float), ("lambda_up", C.c_float), ("lambda_down", C.c_float),
                ("lambda_floor", C.c_float), ("lambda_max", C.c_float), ("min_valid_fraction", C.c_float)]


class LmRecord(C.Structure):
    """dvo_lm_record (include/dvo.h): the decisions of the last push / call, the final lambda and the finest level's accepted residual."""
    _fields_ = [("n_first", C.c_int), ("n_accepted", C.c_int), ("n_rejected", C.c_int), ("lambda_", C.c_float), ("residual", C.c_float)]


class LmLog(C.Structure):
    """dvo_lm_log (include/dvo.h): the lambda every logged iteration's solve used and its decision, indexed like TrackLog."""
    _fields_ = [("struct_size", C.c_int), ("levels", C.c_int), ("n_iter", C.c_int * MAX_LEVELS),
                ("lambda_", (C.c_float * MAX_ITERATIONS) * MAX_LEVELS), ("decision", (C.c_int * MAX_ITERATIONS) * MAX_LEVELS)]


class LmEntry(C.Structure):
    """dvo_lm_entry (include/dvo.h): a sequence's accepted pose, the sums of its evaluation and lambda."""
    _fields_ = [("Tc", C.c_double * 12), ("H", C.c_double * 21), ("g", C.c_double * 6), ("sum_r2", C.c_double), ("xi", C.c_float * 6),
                ("pose", C.c_float * 12), ("n_valid", C.c_int), ("residual", C.c_float), ("lambda_", C.c_float), ("reserved", C.c_int)]


LM_RECORD_DTYPE = np.dtype([("n_first", np.int32), ("n_accepted", np.int32), ("n_rejected", np.int32), ("lambda", np.float32),
                            ("residual", np.float32)])
LM_LOG_DTYPE = np.dtype({"names": ["struct_size", "levels", "n_iter", "lambda", "decision"],
                         "formats": [np.int32, np.int32, (np.int32, MAX_LEVELS), (np.float32, (MAX_LEVELS, MAX_ITERATIONS)),
                                     (np.int32, (MAX_LEVELS, MAX_ITERATIONS))],
                         "offsets": [getattr(LmLog, f[0]).offset for f in LmLog._fields_],
                         "itemsize": C.sizeof(LmLog)})
LM_ENTRY_DTYPE = np.dtype({"names": ["Tc", "H", "g", "sum_r2", "xi", "pose", "n_valid", "residual", "lambda", "reserved"],
                           "formats": [("<f8", (12,)), ("<f8", (21,)), ("<f8", (6,)), "<f8", ("<f4", (6,)), ("<f4", (12,)), "<i4", "<f4",
                                       "<f4", "<i4"],
                           "offsets": [getattr(LmEntry, f[0]).offset for f in LmEntry._fields_],
                           "itemsize": C.sizeof(LmEntry)})


class GnProfile(C.Structure):
    _fields_ = [("gn_ms", C.c_double), ("gn_launches", C.c_uint64), ("gn_pixels", C.c_uint64),
                ("gn_iterations", C.c_uint64)]


class MonoStats(C.Structure):
    _fields_ = [("frames", C.c_int), ("keyframes_created", C.c_int), ("ring_keyframes", C.c_int),
                ("valid_updates_last_frame", C.c_int), ("clamped_pixels", C.c_int)]


class MapProfile(C.Structure):
    _fields_ = [("frames", C.c_uint64), ("depth_update_ms", C.c_double), ("regularize_ms", C.c_double), ("propagate_ms", C.c_double),
                ("update_window_pixels", C.c_uint64), ("map_pixels", C.c_uint64)]


EXPORTS = [
    "dvo_config_default", "dvo_version", "dvo_status_string", "dvo_last_error", "dvo_device_count",
    "dvo_vo_create", "dvo_vo_destroy", "dvo_vo_set_initial_depth", "dvo_vo_init_keyframe", "dvo_vo_odometrize",
    "dvo_vo_odometrize_depth", "dvo_vo_odometrize_raw", "dvo_vo_keyframe_count", "dvo_vo_keyframe_info", "dvo_vo_keyframe_get",
    "dvo_vo_last_frame_pose", "dvo_vo_last_valid_updates", "dvo_vo_last_track_log", "dvo_debug_persist_timeline",
    "dvo_batch_create", "dvo_batch_destroy", "dvo_batch_push_device", "dvo_batch_push_host", "dvo_batch_last_poses",
    "dvo_batch_prefetch_device", "dvo_batch_copy_poses_device", "dvo_batch_last_track_log", "dvo_batch_synchronize", "dvo_batch_profile", "dvo_batch_probe_gn", "dvo_shard_range", "dvo_batch_gather_poses_rccl",
    "dvo_batch_push_raw_device", "dvo_batch_prefetch_raw_device", "dvo_batch_push_raw_host", "dvo_batch_odometrize_raw_device",
    "dvo_batch_odometrize_host", "dvo_batch_odometrize_raw_host",
    "dvo_batch_create_mono", "dvo_batch_set_initial_depth", "dvo_batch_set_initial_depth_device", "dvo_batch_odometrize_device",
    "dvo_batch_world_poses", "dvo_batch_copy_world_poses_device", "dvo_batch_keyframe_get", "dvo_batch_mono_stats", "dvo_batch_profile_mapping",
    "dvo_op_cull_image", "dvo_op_gradient", "dvo_op_warp_image", "dvo_op_pyramid", "dvo_op_gn_step", "dvo_op_track",
    "dvo_op_propagate", "dvo_op_regularize", "dvo_op_depth_update", "dvo_op_se3_exp", "dvo_op_se3_log",
    "dvo_op_se3_concatenate", "dvo_op_pose_algebra",
    "dvo_png_info", "dvo_png_read", "dvo_dataset_open_tum", "dvo_dataset_open_list", "dvo_dataset_size", "dvo_dataset_entry",
    "dvo_dataset_close", "dvo_op_ingest", "dvo_vo_odometrize_depth_raw", "dvo_op_undistort",
    "dvo_eval_ate", "dvo_eval_rpe", "dvo_pose_inverse", "dvo_traj_write_tum",
    "dvo_vo_save", "dvo_vo_load", "dvo_vo_set_history_limit", "dvo_op_visualize", "dvo_ppm_write",
    "dvo_selftest_reciprocal", "dvo_selftest_sqrt", "dvo_selftest_division", "dvo_selftest_trig",
    "dvo_batch_set_actions", "dvo_batch_last_status", "dvo_batch_copy_status_device",
    "dvo_batch_set_intrinsics", "dvo_batch_get_intrinsics", "dvo_batch_create_mono_cameras",
    "dvo_batch_set_distortion", "dvo_batch_get_distortion", "dvo_vo_set_distortion",
    "dvo_batch_set_sensor_distortion", "dvo_batch_get_sensor_distortion",
    "dvo_batch_set_mono_actions", "dvo_batch_mono_last_status", "dvo_batch_copy_mono_status_device",
    "dvo_batch_set_mono_start_depth_device",
    "dvo_batch_set_pose_guess_mode", "dvo_batch_set_pose_guess", "dvo_batch_last_start_poses",
    "dvo_batch_set_keyframe_tracking",
    "dvo_batch_set_track_quality", "dvo_batch_last_track_quality", "dvo_batch_copy_track_quality_device",
    "dvo_batch_frame_get", "dvo_debug_batch_level_plan",
    "dvo_batch_set_robust_weights", "dvo_batch_set_robust_scales", "dvo_batch_last_robust_scales", "dvo_op_gn_step_robust",
    "dvo_batch_set_affine_brightness", "dvo_batch_set_affine_rows", "dvo_batch_last_affine", "dvo_batch_last_affine_log",
    "dvo_op_gn_step_affine",
    "dvo_geometric_config_default", "dvo_batch_set_geometric", "dvo_batch_last_geometric", "dvo_batch_last_geometric_log",
    "dvo_op_gn_step_geometric",
    "dvo_batch_set_geometric_affine", "dvo_op_gn_step_geometric_affine",
    "dvo_kf_fusion_config_default", "dvo_batch_set_keyframe_fusion", "dvo_batch_last_keyframe_fusion", "dvo_batch_keyframe_fusion_counts",
    "dvo_kf_carry_config_default", "dvo_batch_set_keyframe_carry", "dvo_batch_last_keyframe_carry",
    "dvo_op_pyramid_frames",
    "dvo_op_depth_update_batch",
    "dvo_batch_set_robust_median", "dvo_batch_last_robust_log", "dvo_batch_last_robust_histogram", "dvo_op_gn_step_robust_median",
    "dvo_batch_set_photometric", "dvo_batch_get_photometric", "dvo_vo_set_photometric", "dvo_debug_batch_photometric_gain",
    "dvo_debug_batch_last_pyramid_kernel",
    "dvo_lm_config_default", "dvo_batch_set_step_control", "dvo_batch_last_step_control", "dvo_batch_last_step_control_log",
    "dvo_op_lm_step",
    "dvo_points_config_default", "dvo_batch_export_points", "dvo_batch_last_points",
    "dvo_batch_set_pyramid_filter", "dvo_batch_pyramid_filter", "dvo_op_pyramid_frames_filtered",
]

# per-sequence action of the next Batch push (Batch.set_actions) and outcome of the last one (Batch.last_status): include/dvo.h
SEQ_SKIP, SEQ_TRACK, SEQ_RESTART = 0, 1, 2
SEQ_TRACKED, SEQ_SKIPPED, SEQ_STARTED, SEQ_BAD_ACTION = 0, 1, 2, 3
# start pose of a batch's tracking (Batch / MonoBatch .set_pose_guess_mode): include/dvo.h
GUESS_NONE, GUESS_GIVEN, GUESS_CONSTANT_VELOCITY = 0, 1, 2
# flags of a tracking-quality record (TrackQuality.flags): include/dvo.h
QUALITY_CONVERGED, QUALITY_CAPPED, QUALITY_NO_VALID, QUALITY_NOT_FINITE, QUALITY_RANK_DEFICIENT = 1, 2, 4, 8, 16

# robust residual weights (Batch / MonoBatch .set_robust_weights): include/dvo.h
ROBUST_NONE, ROBUST_HUBER, ROBUST_STUDENT_T = 0, 1, 2
ROBUST_SCALE_ADAPTIVE, ROBUST_SCALE_GIVEN = 0, 1
ROBUST_SCALE_MEDIAN = 2   # the median (MAD) scale: Batch / MonoBatch .set_robust_median
MEDIAN_BINS = 256
# affine brightness compensation (Batch / MonoBatch .set_affine_brightness): include/dvo.h
AFFINE_OFF, AFFINE_ESTIMATE, AFFINE_GIVEN = 0, 1, 2
# the geometric (depth) term (Batch.set_geometric): include/dvo.h
GEOMETRIC_OFF, GEOMETRIC_ON = 0, 1
# step control (Batch / MonoBatch .set_step_control) and its decisions: include/dvo.h
LM_OFF, LM_ON = 0, 1
LM_FIRST, LM_ACCEPT, LM_REJECT = 1, 2, 3
# keyframe depth fusion (Batch.set_keyframe_fusion): include/dvo.h
KF_FUSION_OFF, KF_FUSION_ON = 0, 1
# keyframe carry (Batch.set_keyframe_carry): include/dvo.h
KF_CARRY_OFF, KF_CARRY_ON = 0, 1
# launch form of a level (Batch / MonoBatch .level_plan): include/dvo.h
PLAN_PAIRS, PLAN_ITERATION, PLAN_LEVEL, PLAN_LDS_PATCH = 0, 1, 2, 3


def _level_plan(handle, level):
    """dvo_debug_batch_level_plan of a batch handle: dict(ppt, group, tiles_2d, tiles, schedule) of one pyramid level"""
    v = [C.c_int() for _ in range(5)]
    _check(lib().dvo_debug_batch_level_plan(handle, int(level), *[C.byref(x) for x in v]))
    return dict(ppt=v[0].value, group=v[1].value, tiles_2d=bool(v[2].value), tiles=v[3].value, schedule=v[4].value)


class KfFusionConfig(C.Structure):
    _fields_ = [("mode", C.c_int), ("max_diff", C.c_float), ("max_count", C.c_int)]


class KfFusionRecord(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("n_candidates", C.c_int), ("n_fused", C.c_int), ("n_gated", C.c_int)]


KF_FUSION_RECORD_DTYPE = np.dtype([("struct_size", np.int32), ("n_candidates", np.int32), ("n_fused", np.int32), ("n_gated", np.int32)])



class KfCarryConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("mode", C.c_int), ("max_diff", C.c_float)]

    def __init__(self, mode=KF_CARRY_ON, max_diff=0.05, struct_size=None):
        super().__init__(C.sizeof(KfCarryConfig) if struct_size is None else int(struct_size), int(mode), float(max_diff))


class KfCarryRecord(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("n_candidates", C.c_int), ("n_carried", C.c_int), ("n_gated", C.c_int)]


KF_CARRY_RECORD_DTYPE = np.dtype([("struct_size", np.int32), ("n_candidates", np.int32), ("n_carried", np.int32), ("n_gated", np.int32)])

# the kernel a pyramid build ran and the flags of op_pyramid_frames: include/dvo.h
PYRAMID_KERNEL_SCALAR, PYRAMID_KERNEL_RAW4, PYRAMID_KERNEL_SPLIT, PYRAMID_KERNEL_REMAP = 0, 1, 2, 3
# ... of a handle with a photometric calibration (MonoBatch.set_photometric)
PYRAMID_KERNEL_PHOTO_RAW4, PYRAMID_KERNEL_PHOTO_SCALAR, PYRAMID_KERNEL_PHOTO_REMAP = 4, 5, 6
PYRAMID_ROWS_DECIMATED, PYRAMID_FORCE_WEIGHT_MAPS, PYRAMID_SPLIT = 1, 2, 4
# the low-pass filter of a sensor-depth batch's gray pyramid (Batch.set_pyramid_filter, op_pyramid_frames_filtered) and its kernels
PYRAMID_FILTER_NONE, PYRAMID_FILTER_BINOMIAL3 = 0, 1
PYRAMID_KERNEL_FILTER = 7


def _photometric_arrays(who, n_cal, inv_response, vignette, height, width):
    """the float32 arrays of a photometric calibration, shape-checked: ([n_cal, 256] or None, [n_cal, H, W] or None)"""
    r = v = None
    if inv_response is not None:
        r = f32(inv_response).reshape(-1, 256) if np.ndim(inv_response) == 1 else f32(inv_response)
        if r.shape != (n_cal, 256):
            raise ValueError("%s: inv_response must be float[256] or float[%d, 256], got shape %s" % (who, n_cal, r.shape))
    if vignette is not None:
        v = f32(vignette)
        if v.ndim == 2:
            v = v.reshape((1,) + v.shape)
        if v.shape != (n_cal, height, width):
            raise ValueError("%s: vignette must be float[%d, %d] or float[%d, %d, %d], got shape %s"
                             % (who, height, width, n_cal, height, width, v.shape))
    return r, v


class PyramidKernel(C.Structure):
    """dvo_pyramid_kernel (include/dvo.h): kind, and the CULLS and PLAN instance of the kernel a build ran."""
    _fields_ = [("kind", C.c_int), ("culls", C.c_int), ("plan", C.c_int)]

    def name(self):
        plan = "true" if self.plan else "false"
        if self.kind == PYRAMID_KERNEL_SCALAR:
            return "k_pyramid<%s>" % plan
        if self.kind == PYRAMID_KERNEL_RAW4:
            return "k_pyramid_raw4<%d, %s>" % (self.culls, plan)
        if self.kind == PYRAMID_KERNEL_SPLIT:
            return "k_pyramid_raw4_coarse<%d> + k_pyramid_raw4_rest<%d>" % (self.culls, self.culls)
        if self.kind == PYRAMID_KERNEL_PHOTO_RAW4:
            return "k_pyramid_raw4_photo<%d, %s>" % (self.culls, plan)
        if self.kind == PYRAMID_KERNEL_PHOTO_SCALAR:
            return "k_pyramid_photo<%s, false>" % plan
        if self.kind == PYRAMID_KERNEL_PHOTO_REMAP:
            return "k_pyramid_photo<%s, true>" % plan
        if self.kind == PYRAMID_KERNEL_FILTER:   # plan = PLAN | WIDE << 1 | RAW << 2: <CULLS, RAW, PLAN, WIDE>
            b = lambda bit: "true" if self.plan & bit else "false"
            return "k_pyramid_filter_top<%d, %s, %s, %s>" % (self.culls, b(4), b(1), b(2))
        return "remap"


class PyramidFramesArgs(C.Structure):
    """dvo_pyramid_frames_args (include/dvo.h)."""
    _fields_ = [("struct_size", C.c_int), ("n_seq", C.c_int), ("w", C.c_int), ("h", C.c_int), ("levels", C.c_int), ("culls", C.c_int),
                ("flags", C.c_int), ("channels", C.c_int), ("depth_scale", C.c_float),
                ("gray", C.c_void_p), ("depth", C.c_void_p), ("sigma", C.c_void_p), ("rgb", C.c_void_p), ("depth16", C.c_void_p),
                ("seq_action", C.c_void_p), ("gray2", C.c_void_p), ("depth2", C.c_void_p), ("sigma2", C.c_void_p),
                ("rgb2", C.c_void_p), ("depth16_2", C.c_void_p)]


class DepthUpdateBatchArgs(C.Structure):
    """dvo_depth_update_batch_args (include/dvo.h)."""
    _fields_ = [("struct_size", C.c_int), ("n_seq", C.c_int), ("w", C.c_int), ("h", C.c_int), ("ring", C.c_int), ("per_camera", C.c_int),
                ("K", C.c_void_p), ("n_total", C.c_void_p), ("kf_gray", C.c_void_p), ("kf_xi", C.c_void_p), ("obj_gray", C.c_void_p),
                ("obj_xi", C.c_void_p), ("obj_rel_xi", C.c_void_p), ("need", C.c_void_p), ("frame_id", C.c_void_p)]


_lib = None


def lib():
    """Load lib/libdvo.so.  Raises (never falls back) when the HIP extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DvoError("libdvo.so not built: run `make -C direct-visual-odometry_amd` (or __graft_entry__.build()); "
                           "there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        L.dvo_version.restype = C.c_char_p
        L.dvo_status_string.restype = C.c_char_p
        L.dvo_last_error.restype = C.c_char_p
        _lib = L
    return _lib


def _check(st):
    if st != 0:
        L = lib()
        raise DvoError("%s: %s" % (L.dvo_status_string(st).decode(), L.dvo_last_error().decode()))


def default_config(**kw):
    c = Config()
    lib().dvo_config_default(C.byref(c))
    for k, v in kw.items():
        if not hasattr(c, k):
            raise AttributeError(k)
        setattr(c, k, v)
    return c


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def fp(a):
    return a.ctypes.data_as(FP)


def device_count():
    return lib().dvo_device_count()


# ------------------------------------------------------------------ math::se3 (device evaluated)
class se3:
    @staticmethod
    def exp(xi, dev=0):
        xi = f32(xi); T = np.zeros(16, np.float32)
        _check(lib().dvo_op_se3_exp(dev, fp(xi), fp(T)))
        return T.reshape(4, 4)

    @staticmethod
    def log(T, dev=0):
        T = f32(T).reshape(16); xi = np.zeros(6, np.float32)
        _check(lib().dvo_op_se3_log(dev, fp(T), fp(xi)))
        return xi

    @staticmethod
    def concatenate(a, b, dev=0):
        a = f32(a); b = f32(b); o = np.zeros(6, np.float32)
        _check(lib().dvo_op_se3_concatenate(dev, fp(a), fp(b), fp(o)))
        return o


# doubles per case (in, out) of pose_algebra's ops: include/dvo.h
POSE_ALGEBRA_ROWS = {0: (6, 12), 1: (12, 6), 2: (12, 6), 3: (12, 31), 4: (27, 7), 5: (21, 42)}


def pose_algebra(op, rows, dev=0):
    """dvo_op_pose_algebra: op on every row of rows (n x POSE_ALGEBRA_ROWS[op][0] float64) -> n x POSE_ALGEBRA_ROWS[op][1] float64"""
    ni, no = POSE_ALGEBRA_ROWS[op]
    rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, ni)
    out = np.zeros((rows.shape[0], no), np.float64)
    DP = C.POINTER(C.c_double)
    _check(lib().dvo_op_pose_algebra(dev, op, rows.shape[0], rows.ctypes.data_as(DP), out.ctypes.data_as(DP)))
    return out


# ------------------------------------------------------------------ Convert / Transform
class Convert:
    @staticmethod
    def cullImage(src, times, dev=0):
        src = f32(src); h, w = src.shape
        dst = np.zeros((h >> times, w >> times), np.float32)
        _check(lib().dvo_op_cull_image(dev, fp(src), w, h, times, fp(dst)))
        return dst

    @staticmethod
    def gradiate(img, x, dev=0):
        img = f32(img); h, w = img.shape
        out = np.zeros((h, w), np.float32)
        _check(lib().dvo_op_gradient(dev, fp(img), w, h, 1 if x else 0, fp(out)))
        return out


class Transform:
    @staticmethod
    def warpImage(xi, gray, depth, K, dev=0):
        xi = f32(xi); gray = f32(gray); depth = f32(depth); K = f32(K).reshape(9)
        h, w = gray.shape
        out = np.zeros((h, w), np.float32)
        _check(lib().dvo_op_warp_image(dev, fp(xi), fp(gray), fp(depth), w, h, fp(K), fp(out)))
        return out


def pyramid(gray, depth, sigma, levels, culls, dev=0):
    """Frame(gray, depth, sigma, K, levels, culls) pyramids (frame.cpp:16-37): lists of per-level arrays."""
    gray = f32(gray); h, w = gray.shape
    d = f32(depth) if depth is not None else None
    s = f32(sigma) if sigma is not None else None
    shapes = [((h >> culls) >> (levels - 1 - i), (w >> culls) >> (levels - 1 - i)) for i in range(levels)]
    go = [np.zeros(sh, np.float32) for sh in shapes]
    do = [np.zeros(sh, np.float32) for sh in shapes]
    so = [np.zeros(sh, np.float32) for sh in shapes]
    arr = lambda lst: (FP * levels)(*[fp(a) for a in lst])
    _check(lib().dvo_op_pyramid(dev, fp(gray), fp(d) if d is not None else None, fp(s) if s is not None else None,
                                w, h, levels, culls, arr(go), arr(do), arr(so)))
    return go, (do if d is not None else None), (so if s is not None else None)


def op_pyramid_frames_filtered(w, h, levels, culls, filter=PYRAMID_FILTER_BINOMIAL3, **kw):
    """dvo_op_pyramid_frames_filtered (include/dvo.h): op_pyramid_frames with the gray pyramid low-pass filtered before each
    halving; the same arguments and result.  filter = PYRAMID_FILTER_NONE is op_pyramid_frames."""
    return op_pyramid_frames(w, h, levels, culls, _filter=int(filter), **kw)


def op_pyramid_frames(w, h, levels, culls, gray=None, depth=None, sigma=None, rgb=None, depth16=None, depth_scale=0.0, flags=0,
                      seq_action=None, second=None, cfg=None, dev=0, _filter=None):
    """dvo_op_pyramid_frames (include/dvo.h): the batched pyramid build through the engine, once.  Float maps gray [+ depth + sigma]
    [n][rows][w], or raw frames rgb u8 [n][rows][w] / [n][rows][w][3 or 4] [+ depth16 u16]; rows = h, or h >> culls with
    PYRAMID_ROWS_DECIMATED.  seq_action [n] with second = dict(gray=, depth=, sigma=) / dict(rgb=, depth16=): the planned build.
    Returns dict(gray, depth, sigma, wgt: lists of [n][h_l][w_l] float32 per level, kernel: PyramidKernel)."""
    keep = []

    def ptr(a, dt):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        return a.ctypes.data

    first = rgb if rgb is not None else gray
    n = int(np.shape(first)[0])
    a = PyramidFramesArgs()
    a.struct_size = C.sizeof(PyramidFramesArgs)
    a.n_seq, a.w, a.h, a.levels, a.culls, a.flags = n, int(w), int(h), int(levels), int(culls), int(flags)
    a.depth_scale = float(depth_scale)
    if rgb is not None:
        a.channels = 1 if np.ndim(rgb) == 3 else int(np.shape(rgb)[3])
    a.gray, a.depth, a.sigma = ptr(gray, np.float32), ptr(depth, np.float32), ptr(sigma, np.float32)
    a.rgb, a.depth16 = ptr(rgb, np.uint8), ptr(depth16, np.uint16)
    a.seq_action = ptr(seq_action, np.uint8)
    if second is not None:
        a.gray2, a.depth2, a.sigma2 = (ptr(second.get(k), np.float32) for k in ("gray", "depth", "sigma"))
        a.rgb2, a.depth16_2 = ptr(second.get("rgb"), np.uint8), ptr(second.get("depth16"), np.uint16)
    shapes = [(n, (h >> culls) >> (levels - 1 - i), (w >> culls) >> (levels - 1 - i)) for i in range(levels)]
    out = {m: [np.zeros(sh, np.float32) for sh in shapes] for m in ("gray", "depth", "sigma", "wgt")}
    arr = lambda lst: (FP * levels)(*[fp(x) for x in lst])
    ran = PyramidKernel()
    outs = (arr(out["gray"]), arr(out["depth"]), arr(out["sigma"]), arr(out["wgt"]), C.byref(ran))
    if _filter is None:
        _check(lib().dvo_op_pyramid_frames(dev, C.byref(cfg) if cfg is not None else None, C.byref(a), *outs))
    else:
        _check(lib().dvo_op_pyramid_frames_filtered(dev, C.byref(cfg) if cfg is not None else None, C.byref(a), _filter, *outs))
    out["kernel"] = ran
    return out


# ------------------------------------------------------------------ Track
def optimize(obj_gray, ref_gray, ref_depth, ref_sigma, K, xi, level, cfg=None, want_mask=False, dev=0):
    """Track::optimize (src/track/optimize.cpp:10-99): one Gauss-Newton step on one level."""
    obj_gray = f32(obj_gray); ref_gray = f32(ref_gray); ref_depth = f32(ref_depth); ref_sigma = f32(ref_sigma)
    K = f32(K).reshape(9); xi = f32(xi)
    h, w = ref_gray.shape
    out = GnResult()
    mask = np.zeros((h, w), np.uint8) if want_mask else None
    _check(lib().dvo_op_gn_step(dev, C.byref(cfg) if cfg is not None else None, fp(obj_gray), fp(ref_gray),
                                fp(ref_depth), fp(ref_sigma), w, h, fp(K), fp(xi), level, C.byref(out),
                                mask.ctypes.data_as(C.c_void_p) if want_mask else None))
    res = dict(H=np.array(out.H[:]), g=np.array(out.g[:]), sum_r2=out.sum_r2, n_valid=out.n_valid,
               xi_update=np.array(out.xi_update[:], np.float32), residual=np.float32(out.residual),
               xi_next=np.array(out.xi_next[:], np.float32))
    if want_mask:
        res["mask"] = mask
    return res


def optimize_robust(obj_gray, ref_gray, ref_depth, ref_sigma, K, xi, level, kind, param, s2, cfg=None, dev=0):
    """optimize() with every contributing pixel weighted by rho of (kind, param, s2) (dvo_op_gn_step_robust, include/dvo.h)."""
    obj_gray = f32(obj_gray); ref_gray = f32(ref_gray); ref_depth = f32(ref_depth); ref_sigma = f32(ref_sigma)
    K = f32(K).reshape(9); xi = f32(xi)
    h, w = ref_gray.shape
    out = GnResult()
    _check(lib().dvo_op_gn_step_robust(dev, C.byref(cfg) if cfg is not None else None, fp(obj_gray), fp(ref_gray),
                                       fp(ref_depth), fp(ref_sigma), w, h, fp(K), fp(xi), level, int(kind), C.c_float(param),
                                       C.c_float(s2), C.byref(out)))
    return dict(H=np.array(out.H[:]), g=np.array(out.g[:]), sum_r2=out.sum_r2, n_valid=out.n_valid,
                xi_update=np.array(out.xi_update[:], np.float32), residual=np.float32(out.residual),
                xi_next=np.array(out.xi_next[:], np.float32))


def op_gn_step_robust_median(obj_gray, ref_gray, ref_depth, ref_sigma, K, xi, level, kind, param, s2, cfg=None, dev=0):
    """optimize_robust() through the median scale's kernel pair (dvo_op_gn_step_robust_median, include/dvo.h); adds `counts` (uint32
    [256], the bins of the contributing pixels' |r|), `median_bin` (-1: no pixel) and `next_s2` (the s2 of the entry the solve wrote)."""
    obj_gray = f32(obj_gray); ref_gray = f32(ref_gray); ref_depth = f32(ref_depth); ref_sigma = f32(ref_sigma)
    K = f32(K).reshape(9); xi = f32(xi)
    h, w = ref_gray.shape
    out = GnResult()
    counts = np.zeros(MEDIAN_BINS, np.uint32)
    m = C.c_int(0)
    nxt = C.c_float(0.0)
    _check(lib().dvo_op_gn_step_robust_median(dev, C.byref(cfg) if cfg is not None else None, fp(obj_gray), fp(ref_gray),
                                              fp(ref_depth), fp(ref_sigma), w, h, fp(K), fp(xi), level, int(kind), C.c_float(param),
                                              C.c_float(s2), C.byref(out), counts.ctypes.data_as(C.c_void_p), C.byref(m), C.byref(nxt)))
    return dict(H=np.array(out.H[:]), g=np.array(out.g[:]), sum_r2=out.sum_r2, n_valid=out.n_valid,
                xi_update=np.array(out.xi_update[:], np.float32), residual=np.float32(out.residual),
                xi_next=np.array(out.xi_next[:], np.float32), counts=counts, median_bin=int(m.value), next_s2=np.float32(nxt.value))


def op_gn_step_affine(obj_gray, ref_gray, ref_depth, ref_sigma, K, xi, level, a, b, kind=ROBUST_NONE, param=1.0, s2=0.0, cfg=None, dev=0):
    """optimize_robust() against the compensated brightness fmaf(a, I1, b) (dvo_op_gn_step_affine, include/dvo.h); adds `moments`
    (N, M1, M2, M11, M12 in float64) and `next_ab` (the entry the solve writes from them)."""
    obj_gray = f32(obj_gray); ref_gray = f32(ref_gray); ref_depth = f32(ref_depth); ref_sigma = f32(ref_sigma)
    K = f32(K).reshape(9); xi = f32(xi)
    h, w = ref_gray.shape
    out = GnResult()
    mom = np.zeros(5, np.float64); nxt = np.zeros(2, np.float32)
    _check(lib().dvo_op_gn_step_affine(dev, C.byref(cfg) if cfg is not None else None, fp(obj_gray), fp(ref_gray),
                                       fp(ref_depth), fp(ref_sigma), w, h, fp(K), fp(xi), level, int(kind), C.c_float(param),
                                       C.c_float(s2), C.c_float(a), C.c_float(b), C.byref(out),
                                       mom.ctypes.data_as(C.POINTER(C.c_double)), fp(nxt)))
    return dict(H=np.array(out.H[:]), g=np.array(out.g[:]), sum_r2=out.sum_r2, n_valid=out.n_valid,
                xi_update=np.array(out.xi_update[:], np.float32), residual=np.float32(out.residual),
                xi_next=np.array(out.xi_next[:], np.float32), moments=mom, next_ab=nxt)


def geometric_default_config():
    """dvo_geometric_config_default: ON, weight 10, max_diff 0.1 m"""
    c = GeometricConfig()
    lib().dvo_geometric_config_default(C.byref(c))
    return c


def op_gn_step_geometric(obj_gray, obj_depth, obj_sigma, ref_gray, ref_depth, K, xi, level, weight, max_diff, cfg=None, dev=0):
    """optimize() with the geometric term (dvo_op_gn_step_geometric, include/dvo.h): the tracked frame's gray, depth and sigma, the
    reference's gray and depth; adds `n_geo` and `sum_sq` (S29 in float64)."""
    obj_gray = f32(obj_gray); obj_depth = f32(obj_depth); obj_sigma = f32(obj_sigma); ref_gray = f32(ref_gray); ref_depth = f32(ref_depth)
    K = f32(K).reshape(9); xi = f32(xi)
    h, w = ref_gray.shape
    out = GnResult()
    sums = np.zeros(2, np.float64)
    _check(lib().dvo_op_gn_step_geometric(dev, C.byref(cfg) if cfg is not None else None, fp(obj_gray), fp(obj_depth), fp(obj_sigma),
                                          fp(ref_gray), fp(ref_depth), w, h, fp(K), fp(xi), level, C.c_float(weight),
                                          C.c_float(max_diff), C.byref(out), sums.ctypes.data_as(C.POINTER(C.c_double))))
    return dict(H=np.array(out.H[:]), g=np.array(out.g[:]), sum_r2=out.sum_r2, n_valid=out.n_valid,
                xi_update=np.array(out.xi_update[:], np.float32), residual=np.float32(out.residual),
                xi_next=np.array(out.xi_next[:], np.float32), n_geo=int(sums[0]), sum_sq=float(sums[1]))


def op_gn_step_geometric_affine(obj_gray, obj_depth, obj_sigma, ref_gray, ref_depth, K, xi, level, weight, max_diff, a, b, cfg=None, dev=0):
    """op_gn_step_geometric() against the compensated brightness fmaf(a, I1, b) (dvo_op_gn_step_geometric_affine, include/dvo.h): adds
    `n_geo`, `sum_sq`, `moments` (n_valid, M1, M2, M11, M12 in float64) and `next_ab`."""
    obj_gray = f32(obj_gray); obj_depth = f32(obj_depth); obj_sigma = f32(obj_sigma); ref_gray = f32(ref_gray); ref_depth = f32(ref_depth)
    K = f32(K).reshape(9); xi = f32(xi)
    h, w = ref_gray.shape
    out = GnResult()
    sums = np.zeros(2, np.float64); mom = np.zeros(5, np.float64); nxt = np.zeros(2, np.float32)
    DP = C.POINTER(C.c_double)
    _check(lib().dvo_op_gn_step_geometric_affine(dev, C.byref(cfg) if cfg is not None else None, fp(obj_gray), fp(obj_depth), fp(obj_sigma),
                                                 fp(ref_gray), fp(ref_depth), w, h, fp(K), fp(xi), level, C.c_float(weight),
                                                 C.c_float(max_diff), C.c_float(a), C.c_float(b), C.byref(out),
                                                 sums.ctypes.data_as(DP), mom.ctypes.data_as(DP), fp(nxt)))
    return dict(H=np.array(out.H[:]), g=np.array(out.g[:]), sum_r2=out.sum_r2, n_valid=out.n_valid,
                xi_update=np.array(out.xi_update[:], np.float32), residual=np.float32(out.residual),
                xi_next=np.array(out.xi_next[:], np.float32), n_geo=int(sums[0]), sum_sq=float(sums[1]), moments=mom, next_ab=nxt)


def lm_default_config():
    """dvo_lm_config_default: ON, lambda0 1, up 4, down 0.5, floor 1e-4, max 1e6, min_valid_fraction 0.5"""
    c = LmConfig()
    lib().dvo_lm_config_default(C.byref(c))
    return c


def op_lm_step(sums, xi_eval, entries, lm=None, level_first=False, it_prev=0, cfg=None, dev=0):
    """The serial tail of the step-control solve on given sums (dvo_op_lm_step, include/dvo.h): sums float64 [n][29], xi_eval float32
    [n][6], entries an array [n] of LM_ENTRY_DTYPE; lm an LmConfig (None: the defaults), cfg a Config for the stop constants.
    -> dict(entry [n] LM_ENTRY_DTYPE, update [n][6], xi_next [n][6], decision [n], active [n])"""
    sums = np.ascontiguousarray(sums, dtype=np.float64).reshape(-1, 29)
    n = sums.shape[0]
    xi_eval = f32(xi_eval).reshape(n, 6)
    entries = np.ascontiguousarray(entries, dtype=LM_ENTRY_DTYPE).reshape(n)
    lm = lm if lm is not None else lm_default_config()
    cfg = cfg if cfg is not None else default_config()
    out = np.zeros(n, LM_ENTRY_DTYPE)
    upd = np.zeros((n, 6), np.float32); nxt = np.zeros((n, 6), np.float32)
    dec = np.zeros(n, np.int32); act = np.zeros(n, np.int32)
    _check(lib().dvo_op_lm_step(dev, n, sums.ctypes.data_as(C.c_void_p), fp(xi_eval), entries.ctypes.data_as(C.c_void_p), C.byref(lm),
                                1 if level_first else 0, int(it_prev), int(cfg.max_iterations), int(cfg.fixed_iterations),
                                C.c_float(cfg.min_update), C.c_float(cfg.min_residual), out.ctypes.data_as(C.c_void_p), fp(upd), fp(nxt),
                                dec.ctypes.data_as(C.c_void_p), act.ctypes.data_as(C.c_void_p)))
    return dict(entry=out, update=upd, xi_next=nxt, decision=dec, active=act)


def track(obj_gray, ref_gray, ref_depth, ref_sigma, K, levels, culls, cfg=None, dev=0):
    """Tracker::track (src/track/tracker.cpp:22-85) on full-resolution frames."""
    obj_gray = f32(obj_gray); ref_gray = f32(ref_gray); ref_depth = f32(ref_depth); ref_sigma = f32(ref_sigma)
    K = f32(K).reshape(9)
    h, w = ref_gray.shape
    xi = np.zeros(6, np.float32); log = TrackLog()
    _check(lib().dvo_op_track(dev, C.byref(cfg) if cfg is not None else None, fp(obj_gray), fp(ref_gray),
                              fp(ref_depth), fp(ref_sigma), w, h, fp(K), levels, culls, fp(xi), C.byref(log)))
    return xi, log.to_dict()


# ------------------------------------------------------------------ Map::Implement
class Implement:
    @staticmethod
    def propagate(ref_depth, ref_sigma, ref_age, xi, K, dev=0):
        d = f32(ref_depth); s = f32(ref_sigma); a = f32(ref_age); xi = f32(xi); K = f32(K).reshape(9)
        h, w = d.shape
        od = np.zeros_like(d); os_ = np.zeros_like(d); oa = np.zeros_like(d)
        _check(lib().dvo_op_propagate(dev, fp(d), fp(s), fp(a), w, h, fp(xi), fp(K), fp(od), fp(os_), fp(oa)))
        return od, os_, oa

    @staticmethod
    def regularize(depth, sigma, dev=0):
        d = f32(depth); s = f32(sigma); h, w = d.shape
        out = np.zeros_like(d)
        _check(lib().dvo_op_regularize(dev, fp(d), fp(s), w, h, fp(out)))
        return out


def mapper_update(hist_gray, hist_xi, obj_gray, obj_xi, obj_rel_xi, obj_id, K, ref_depth, ref_sigma, ref_age,
                  cfg=None, dev=0):
    """Mapper::update (src/map/mapper.cpp:76-137).  Returns updated (depth, sigma, age, valid_updates)."""
    n = len(hist_gray)
    grays = [f32(g) for g in hist_gray]
    h, w = grays[0].shape
    garr = (FP * n)(*[fp(g) for g in grays])
    hx = f32(np.asarray(hist_xi).reshape(n, 6))
    og = f32(obj_gray); ox = f32(obj_xi); orx = f32(obj_rel_xi); K = f32(K).reshape(9)
    d = f32(ref_depth).copy(); s = f32(ref_sigma).copy(); a = f32(ref_age).copy()
    v = C.c_int(0)
    _check(lib().dvo_op_depth_update(dev, C.byref(cfg) if cfg is not None else None, n, garr, fp(hx), fp(og), fp(ox),
                                     fp(orx), int(obj_id), fp(K), w, h, fp(d), fp(s), fp(a), C.byref(v)))
    return d, s, a, v.value


def op_depth_update_batch(w, h, ring, K, n_total, kf_gray, kf_xi, obj_gray, obj_xi, obj_rel_xi, need, frame_id, depth, sigma, age,
                          cfg=None, dev=0):
    """dvo_op_depth_update_batch (include/dvo.h): the mapping update of one mono-batch call, on given per-sequence state.  w, h: the
    frame size (maps are (h >> 2) x (w >> 2)); K: [3][3] at full resolution for every sequence, or [n_seq][3][3]: one per sequence
    (the per-camera kernels); kf_gray [n_seq][ring][mh][mw] and kf_xi [n_seq][ring][6]: each sequence's retained keyframes, oldest
    first.  Returns (depth, sigma, age, valid_updates[n_seq], clamped[n_seq])."""
    d = f32(depth).copy(); s = f32(sigma).copy(); a = f32(age).copy()
    n = d.shape[0]
    K = f32(K)
    per_camera = K.ndim == 3
    arrs = dict(K=K.reshape(-1), n_total=np.ascontiguousarray(n_total, np.int32), kf_gray=f32(kf_gray), kf_xi=f32(kf_xi), obj_gray=f32(obj_gray),
                obj_xi=f32(obj_xi), obj_rel_xi=f32(obj_rel_xi), need=np.ascontiguousarray(need, np.int32),
                frame_id=np.ascontiguousarray(frame_id, np.int32))
    mh, mw = h >> 2, w >> 2
    assert d.shape == s.shape == a.shape == arrs["obj_gray"].shape == (n, mh, mw), (d.shape, (n, mh, mw))
    assert arrs["kf_gray"].shape == (n, ring, mh, mw) and arrs["kf_xi"].shape == (n, ring, 6) and K.size == (9 * n if per_camera else 9)
    assert arrs["obj_xi"].shape == arrs["obj_rel_xi"].shape == (n, 6) and all(arrs[k].shape == (n,) for k in ("n_total", "need", "frame_id"))
    args = DepthUpdateBatchArgs()
    args.struct_size = C.sizeof(DepthUpdateBatchArgs)
    args.n_seq, args.w, args.h, args.ring, args.per_camera = n, w, h, ring, 1 if per_camera else 0
    for k, v in arrs.items():
        setattr(args, k, v.ctypes.data)
    valid = np.full(n, -1, np.int32); clamped = np.full(n, -1, np.int32)
    _check(lib().dvo_op_depth_update_batch(dev, C.byref(cfg) if cfg is not None else None, C.byref(args), fp(d), fp(s), fp(a),
                                           valid.ctypes.data_as(C.POINTER(C.c_int)), clamped.ctypes.data_as(C.POINTER(C.c_int))))
    return d, s, a, valid, clamped


# ------------------------------------------------------------------ Core::Loader (dataset front-end) and evaluation
def imread(path):
    """cv::imread(path, IMREAD_UNCHANGED) for PNGs: uint8 / uint16 array [H, W] or [H, W, C] in file channel order (RGB)."""
    w = C.c_int(); h = C.c_int(); ch = C.c_int(); bd = C.c_int()
    _check(lib().dvo_png_info(path.encode(), C.byref(w), C.byref(h), C.byref(ch), C.byref(bd)))
    shape = (h.value, w.value) if ch.value == 1 else (h.value, w.value, ch.value)
    out = np.zeros(shape, np.uint8 if bd.value == 8 else np.uint16)
    _check(lib().dvo_png_read(path.encode(), out.ctypes.data_as(C.c_void_p), C.c_size_t(out.nbytes)))
    return out


class Dataset:
    """TUM RGB-D directory or one of the reference's list files (include/core/loader.hpp:28-52,77-105)."""

    def __init__(self, directory, list_file=None, tum=False, max_dt=0.02):
        self._p = C.c_void_p()
        if tum:
            _check(lib().dvo_dataset_open_tum(directory.encode(), C.c_double(max_dt), C.byref(self._p)))
        else:
            _check(lib().dvo_dataset_open_list(directory.encode(), list_file.encode() if list_file else None, C.byref(self._p)))

    def __len__(self):
        return lib().dvo_dataset_size(self._p)

    def entry(self, i):
        t = C.c_double(); a = C.create_string_buffer(1024); b = C.create_string_buffer(1024); gt = np.zeros(7, np.float32)
        _check(lib().dvo_dataset_entry(self._p, i, C.byref(t), a, b, 1024, fp(gt)))
        return dict(timestamp=t.value, rgb=a.value.decode(), depth=b.value.decode(), gt=gt)

    def close(self):
        if self._p:
            lib().dvo_dataset_close(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ingest(rgb, depth16=None, depth_scale=1.0 / 5000.0, sigma_valid=0.1, sigma_invalid=1.0, invalidate_gray=True, dev=0):
    """k_ingest: raw u8 gray/RGB(A) (+ u16 depth) -> float gray [0,1] (+ depth [m], sigma)."""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    h, w = rgb.shape[:2]
    ch = 1 if rgb.ndim == 2 else rgb.shape[2]
    gray = np.zeros((h, w), np.float32)
    if depth16 is None:
        _check(lib().dvo_op_ingest(dev, rgb.ctypes.data_as(C.c_void_p), ch, None, w, h, C.c_float(depth_scale), C.c_float(sigma_valid),
                                   C.c_float(sigma_invalid), 0, fp(gray), None, None))
        return gray
    d16 = np.ascontiguousarray(depth16, np.uint16)
    depth = np.zeros((h, w), np.float32); sigma = np.zeros((h, w), np.float32)
    _check(lib().dvo_op_ingest(dev, rgb.ctypes.data_as(C.c_void_p), ch, d16.ctypes.data_as(C.c_void_p), w, h, C.c_float(depth_scale),
                               C.c_float(sigma_valid), C.c_float(sigma_invalid), 1 if invalidate_gray else 0, fp(gray), fp(depth), fp(sigma)))
    return gray, depth, sigma


def undistort(src, K, D, dev=0):
    """Loader::getNormalizedUndistortedImages (src/core/loader.cpp:15-42)."""
    src = f32(src); K = f32(K).reshape(9); D = f32(D).reshape(5)
    h, w = src.shape
    out = np.zeros_like(src)
    _check(lib().dvo_op_undistort(dev, fp(src), w, h, fp(K), fp(D), fp(out)))
    return out


VIS_GRAY, VIS_DEPTH, VIS_SIGMA, VIS_AGE, VIS_GRADIENT = range(5)


def visualize(mode, a, b=None, dev=0):
    """Draw::visualize{Gray,Depth,Sigma,Age,Gradient} (src/core/draw.cpp:7-100) -> uint8 RGB [H, W, 3]."""
    a = f32(a); h, w = a.shape
    bb = f32(b) if b is not None else None
    out = np.zeros((h, w, 3), np.uint8)
    _check(lib().dvo_op_visualize(dev, int(mode), fp(a), fp(bb) if bb is not None else None, w, h, out.ctypes.data_as(C.c_void_p)))
    return out


def selftest_reciprocal(dev=0):
    """All 2^32 float patterns through the kernels' reciprocal vs the IEEE division: (fast-path inputs, mismatches, first bad bits)."""
    n = C.c_uint64(); bad = C.c_uint64(); first = C.c_uint32()
    _check(lib().dvo_selftest_reciprocal(dev, C.byref(n), C.byref(bad), C.byref(first)))
    return n.value, bad.value, first.value


def selftest_trig(dev=0):
    """The device's SE(3) sin / cos / atan2 kernels vs the math library on 2^24 arguments: largest relative differences (sin, cos, atan2)."""
    a = C.c_double(); b = C.c_double(); c = C.c_double(); n = C.c_uint64()
    _check(lib().dvo_selftest_trig(dev, C.byref(a), C.byref(b), C.byref(c), C.byref(n)))
    return a.value, b.value, c.value, n.value


def selftest_sqrt(dev=0):
    """Every float in [2^-100, 2^100] through the regularize kernels' short square root vs sqrtf: (inputs, mismatches, first bad bits)."""
    n = C.c_uint64(); bad = C.c_uint64(); first = C.c_uint32()
    _check(lib().dvo_selftest_sqrt(dev, C.byref(n), C.byref(bad), C.byref(first)))
    return n.value, bad.value, first.value


def selftest_division(b_first=0, b_stride=1, b_count=1 << 23, dev=0):
    """The regularize kernels' short division vs the IEEE quotient for b_count mantissas of b times all 2^23 of a: (pairs, mismatches, first bad pair)."""
    n = C.c_uint64(); bad = C.c_uint64(); first = C.c_uint64()
    _check(lib().dvo_selftest_division(dev, C.c_uint32(b_first), C.c_uint32(b_stride), C.c_uint32(b_count), C.byref(n), C.byref(bad), C.byref(first)))
    return n.value, bad.value, first.value


def write_ppm(path, rgb):
    rgb = np.ascontiguousarray(rgb, np.uint8)
    _check(lib().dvo_ppm_write(path.encode(), rgb.ctypes.data_as(C.c_void_p), rgb.shape[1], rgb.shape[0]))


def ate(est_xyz, gt_xyz, with_scale=False):
    """Absolute trajectory error (RMSE after Horn alignment).  Returns (rmse, R, t, scale)."""
    e = f32(est_xyz).reshape(-1, 3); g = f32(gt_xyz).reshape(-1, 3)
    rm = C.c_double(); R = np.zeros(9); t = np.zeros(3); s = C.c_double()
    _check(lib().dvo_eval_ate(e.shape[0], fp(e), fp(g), 1 if with_scale else 0, C.byref(rm), R.ctypes.data_as(C.POINTER(C.c_double)),
                              t.ctypes.data_as(C.POINTER(C.c_double)), C.byref(s)))
    return rm.value, R.reshape(3, 3), t, s.value


def rpe(est_T, gt_T, delta=1):
    e = f32(est_T).reshape(-1, 16); g = f32(gt_T).reshape(-1, 16)
    a = C.c_double(); b = C.c_double()
    _check(lib().dvo_eval_rpe(e.shape[0], fp(e), fp(g), delta, C.byref(a), C.byref(b)))
    return a.value, b.value


def pose_inverse(T):
    T = f32(T).reshape(16); o = np.zeros(16, np.float32)
    _check(lib().dvo_pose_inverse(fp(T), fp(o)))
    return o.reshape(4, 4)


def write_tum_trajectory(path, T, timestamps=None):
    T = f32(T).reshape(-1, 16)
    ts = np.ascontiguousarray(timestamps, np.float64) if timestamps is not None else None
    _check(lib().dvo_traj_write_tum(path.encode(), T.shape[0], ts.ctypes.data_as(C.POINTER(C.c_double)) if ts is not None else None, fp(T)))


# ------------------------------------------------------------------ System::VisualOdometry
class VisualOdometry:
    """System::VisualOdometry (include/system/system.hpp:12-104)."""

    def __init__(self, K, width, height, cfg=None):
        K = f32(K).reshape(9)
        self.width, self.height = width, height
        self._p = C.c_void_p()
        _check(lib().dvo_vo_create(fp(K), width, height, C.byref(cfg) if cfg is not None else None, C.byref(self._p)))

    def close(self):
        if self._p:
            lib().dvo_vo_destroy(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def setInitialDepth(self, depth, sigma):
        d = f32(depth); s = f32(sigma)
        _check(lib().dvo_vo_set_initial_depth(self._p, fp(d), fp(s)))

    def initKeyframe(self, gray, depth, sigma):
        g = f32(gray); d = f32(depth); s = f32(sigma)
        _check(lib().dvo_vo_init_keyframe(self._p, fp(g), fp(d), fp(s)))

    def setDistortion(self, D):
        """Undistort every mono frame (Loader::getNormalizedUndistortedImages) with the creation K and D = (k1, k2, p1, p2, k3);
        None clears.  Before the first frame (dvo_vo_set_distortion)."""
        if D is None:
            _check(lib().dvo_vo_set_distortion(self._p, None))
            return
        d = f32(D)
        if d.shape != (5,):
            raise ValueError("setDistortion: expected float[5], got shape %s" % (d.shape,))
        _check(lib().dvo_vo_set_distortion(self._p, fp(d)))

    def set_photometric(self, inv_response=None, vignette=None):
        """Photometric calibration of every raw mono frame: inv_response float [256] in gray units (None: i / 255) and vignette
        float [H, W] (None: 1); both None clears.  Before the first frame; from then on feed odometrizeRaw (dvo_vo_set_photometric)."""
        r, v = _photometric_arrays("set_photometric", 1, inv_response, vignette, self.height, self.width)
        _check(lib().dvo_vo_set_photometric(self._p, fp(r) if r is not None else None, fp(v) if v is not None else None))

    def odometrize(self, gray):
        g = f32(gray); T = np.zeros(16, np.float32); key = C.c_int(0)
        _check(lib().dvo_vo_odometrize(self._p, fp(g), fp(T), C.byref(key)))
        return T.reshape(4, 4), bool(key.value)

    def odometrizeRaw(self, rgb_u8):
        """odometrize() fed with a raw uint8 frame [H, W] or [H, W, C] (converted on the device)."""
        rgb = np.ascontiguousarray(rgb_u8, np.uint8)
        ch = 1 if rgb.ndim == 2 else rgb.shape[2]
        T = np.zeros(16, np.float32); key = C.c_int(0)
        _check(lib().dvo_vo_odometrize_raw(self._p, rgb.ctypes.data_as(C.c_void_p), ch, fp(T), C.byref(key)))
        return T.reshape(4, 4), bool(key.value)

    def odometrizeUsingDepth(self, gray, depth, sigma):
        g = f32(gray); d = f32(depth); s = f32(sigma); T = np.zeros(16, np.float32)
        _check(lib().dvo_vo_odometrize_depth(self._p, fp(g), fp(d), fp(s), fp(T)))
        return T.reshape(4, 4)

    def odometrizeUsingDepthRaw(self, rgb_u8, depth_u16, depth_scale=1.0 / 5000.0):
        rgb = np.ascontiguousarray(rgb_u8, np.uint8); d16 = np.ascontiguousarray(depth_u16, np.uint16)
        ch = 1 if rgb.ndim == 2 else rgb.shape[2]
        T = np.zeros(16, np.float32)
        _check(lib().dvo_vo_odometrize_depth_raw(self._p, rgb.ctypes.data_as(C.c_void_p), ch, d16.ctypes.data_as(C.c_void_p),
                                                 C.c_float(depth_scale), fp(T)))
        return T.reshape(4, 4)

    def save(self, path):
        _check(lib().dvo_vo_save(self._p, path.encode()))

    def load(self, path):
        _check(lib().dvo_vo_load(self._p, path.encode()))

    def setHistoryLimit(self, n):
        _check(lib().dvo_vo_set_history_limit(self._p, int(n)))

    def keyframeCount(self):
        return lib().dvo_vo_keyframe_count(self._p)

    def keyframeInfo(self, index):
        i = C.c_int(); l = C.c_int(); w = C.c_int(); h = C.c_int()
        xi = np.zeros(6, np.float32); rel = np.zeros(6, np.float32)
        _check(lib().dvo_vo_keyframe_info(self._p, index, C.byref(i), C.byref(l), C.byref(w), C.byref(h), fp(xi), fp(rel)))
        return dict(id=i.value, levels=l.value, width=w.value, height=h.value, xi=xi, rel_xi=rel)

    def keyframe(self, index, level=None):
        info = self.keyframeInfo(index)
        top = info["levels"] - 1
        if level is None:
            level = top
        sh = (info["height"] >> (top - level), info["width"] >> (top - level))
        g = np.zeros(sh, np.float32); d = np.zeros(sh, np.float32); s = np.zeros(sh, np.float32)
        a = np.zeros(sh, np.float32) if level == top else None
        K = np.zeros(9, np.float32)
        _check(lib().dvo_vo_keyframe_get(self._p, index, level, fp(g), fp(d), fp(s), fp(a) if a is not None else None, fp(K)))
        return dict(gray=g, depth=d, sigma=s, age=a, K=K.reshape(3, 3), **info)

    def lastFramePose(self):
        i = C.c_int(); xi = np.zeros(6, np.float32); rel = np.zeros(6, np.float32)
        _check(lib().dvo_vo_last_frame_pose(self._p, C.byref(i), fp(xi), fp(rel)))
        return i.value, xi, rel

    def lastValidUpdates(self):
        return lib().dvo_vo_last_valid_updates(self._p)

    def lastTrackLog(self):
        log = TrackLog()
        _check(lib().dvo_vo_last_track_log(self._p, C.byref(log)))
        return log.to_dict()


class _PoseGuess:
    """Start pose of the tracking, shared by Batch and MonoBatch (dvo_batch_set_pose_guess_mode, include/dvo.h)."""

    def set_pose_guess_mode(self, mode):
        """GUESS_NONE (zero twist, the default), GUESS_GIVEN (set_pose_guess rows) or GUESS_CONSTANT_VELOCITY, from the next push on."""
        _check(lib().dvo_batch_set_pose_guess_mode(self._p, int(mode)))

    def set_pose_guess(self, xi, on_device=False):
        """Rows of the NEXT push (GUESS_GIVEN): float32 [n_seq, 6] (copied now), an int device pointer to float32 [n_seq, 6] with
        on_device=True (read in stream order when the push runs), or None to clear.  Sensor depth: the relative twist of the frame,
        as last_poses returns it; mono: its world twist, as world_poses returns it."""
        if xi is None:
            _check(lib().dvo_batch_set_pose_guess(self._p, None, 0))
        elif on_device:
            _check(lib().dvo_batch_set_pose_guess(self._p, C.c_void_p(int(xi)), 1))
        else:
            x = f32(xi)
            if x.shape != (self.n_seq, 6):
                raise ValueError("set_pose_guess: expected float[%d, 6], got shape %s" % (self.n_seq, x.shape))
            _check(lib().dvo_batch_set_pose_guess(self._p, fp(x), 0))

    def last_start_poses(self):
        """float32 [n_seq, 6]: the twist each TRACKED sequence started from at the last push, zeros for the others (synchronises)."""
        xi = np.zeros((self.n_seq, 6), np.float32)
        _check(lib().dvo_batch_last_start_poses(self._p, fp(xi)))
        return xi


class _TrackQuality:
    """Per-sequence tracking quality of the last push / call, shared by Batch and MonoBatch (dvo_batch_set_track_quality, include/dvo.h)."""

    def set_track_quality(self, enable=True):
        """Keep the finest level's last Gauss-Newton sums of every sequence from the next push / call on (False: stop)."""
        _check(lib().dvo_batch_set_track_quality(self._p, 1 if enable else 0))

    def last_track_quality(self):
        """numpy structured array [n_seq] of TRACK_QUALITY_DTYPE (the fields of dvo_track_quality); synchronises."""
        out = np.zeros(self.n_seq, TRACK_QUALITY_DTYPE)
        _check(lib().dvo_batch_last_track_quality(self._p, out.ctypes.data_as(C.c_void_p)))
        return out

    def copy_track_quality_device(self, ptr):
        """Write the records [n_seq] (C.sizeof(TrackQuality) bytes each) to device memory at int `ptr`, in stream order."""
        _check(lib().dvo_batch_copy_track_quality_device(self._p, C.c_void_p(int(ptr))))


class _RobustWeights:
    """Robust residual weights of the tracking, shared by Batch and MonoBatch (dvo_batch_set_robust_weights, include/dvo.h)."""

    def set_robust_weights(self, kind=ROBUST_NONE, param=1.0, scale_mode=ROBUST_SCALE_ADAPTIVE, scale_floor=1e-3):
        """ROBUST_HUBER (param = k) or ROBUST_STUDENT_T (param = nu) from the next push / call on; ROBUST_NONE or None: off."""
        if kind is None:
            _check(lib().dvo_batch_set_robust_weights(self._p, None))
            return
        c = RobustConfig(C.sizeof(RobustConfig), int(kind), int(scale_mode), float(param), float(scale_floor))
        _check(lib().dvo_batch_set_robust_weights(self._p, C.byref(c)))

    def set_robust_scales(self, s, on_device=False):
        """Scales of every later push (ROBUST_SCALE_GIVEN): float32 [n_seq] (copied now), an int device pointer with on_device=True
        (read in stream order by every push), or None to clear.  A sequence whose s is not finite and > 0 runs unweighted."""
        if s is None:
            _check(lib().dvo_batch_set_robust_scales(self._p, None, 0))
        elif on_device:
            _check(lib().dvo_batch_set_robust_scales(self._p, C.c_void_p(int(s)), 1))
        else:
            x = f32(s)
            if x.shape != (self.n_seq,):
                raise ValueError("set_robust_scales: expected float[%d], got shape %s" % (self.n_seq, x.shape))
            _check(lib().dvo_batch_set_robust_scales(self._p, fp(x), 0))

    def last_robust_scales(self):
        """float32 [n_seq]: the s2 of the finest level's last iteration at the last push (+inf: unweighted, 0: not tracked); synchronises."""
        s2 = np.zeros(self.n_seq, np.float32)
        _check(lib().dvo_batch_last_robust_scales(self._p, fp(s2)))
        return s2

    def set_robust_median(self, kind=ROBUST_HUBER, param=1.0, scale_floor=1e-3):
        """Robust weights with the median (MAD) scale from the next push / call on (dvo_batch_set_robust_median): ROBUST_HUBER (param
        = k) or ROBUST_STUDENT_T (param = nu); None: off."""
        if kind is None:
            _check(lib().dvo_batch_set_robust_median(self._p, None))
            return
        c = RobustConfig(C.sizeof(RobustConfig), int(kind), ROBUST_SCALE_MEDIAN, float(param), float(scale_floor))
        _check(lib().dvo_batch_set_robust_median(self._p, C.byref(c)))

    def last_robust_log(self, seq):
        """dict of the median scale's record of `seq` at the last push (dvo_robust_log): per logged iteration the s2 it used and the
        median bin and count of its own pixels (the next entry's), and the priming pair's; synchronises."""
        lg = RobustLog()
        lg.struct_size = C.sizeof(RobustLog)
        _check(lib().dvo_batch_last_robust_log(self._p, int(seq), C.byref(lg)))
        rec = np.frombuffer(lg, ROBUST_LOG_DTYPE)[0]
        return dict(levels=int(rec["levels"]), n_iter=rec["n_iter"].copy(), s2=rec["s2"].copy(), median_bin=rec["median_bin"].copy(),
                    count=rec["count"].copy(), prime_bin=int(rec["prime_bin"]), prime_count=int(rec["prime_count"]))

    def last_robust_histogram(self, seq):
        """uint32 [256]: the bin counts of the finest level's last iteration of `seq` at the last push (zeros: not tracked); synchronises."""
        counts = np.zeros(MEDIAN_BINS, np.uint32)
        _check(lib().dvo_batch_last_robust_histogram(self._p, int(seq), counts.ctypes.data_as(C.c_void_p)))
        return counts


class _AffineBrightness:
    """Affine brightness compensation of the tracking, shared by Batch and MonoBatch (dvo_batch_set_affine_brightness, include/dvo.h)."""

    def set_affine_brightness(self, mode=AFFINE_OFF, min_pixels=64, min_contrast=1e-3, gain_min=0.25, gain_max=4.0):
        """AFFINE_ESTIMATE (alternating estimate of a gain and an offset per sequence) or AFFINE_GIVEN (rows of set_affine_rows) from
        the next push / call on; AFFINE_OFF or None: off."""
        if mode is None:
            _check(lib().dvo_batch_set_affine_brightness(self._p, None))
            return
        c = AffineConfig(C.sizeof(AffineConfig), int(mode), int(min_pixels), float(min_contrast), float(gain_min), float(gain_max))
        _check(lib().dvo_batch_set_affine_brightness(self._p, C.byref(c)))

    def set_affine_rows(self, ab, on_device=False):
        """(a, b) of every later push (AFFINE_GIVEN): float32 [n_seq][2] (copied now), an int device pointer with on_device=True (read
        in stream order by every push), or None to clear.  A row that is not finite or has a <= 0 is (1, 0)."""
        if ab is None:
            _check(lib().dvo_batch_set_affine_rows(self._p, None, 0))
        elif on_device:
            _check(lib().dvo_batch_set_affine_rows(self._p, C.c_void_p(int(ab)), 1))
        else:
            x = f32(ab)
            if x.shape != (self.n_seq, 2):
                raise ValueError("set_affine_rows: expected float[%d][2], got shape %s" % (self.n_seq, x.shape))
            _check(lib().dvo_batch_set_affine_rows(self._p, fp(x), 0))

    def last_affine(self):
        """float32 [n_seq][2]: the (a, b) the finest level's last iteration used at the last push ((0, 0): not tracked); synchronises."""
        ab = np.zeros((self.n_seq, 2), np.float32)
        _check(lib().dvo_batch_last_affine(self._p, fp(ab)))
        return ab

    def last_affine_log(self, seq):
        """dict of the (a, b) every logged iteration of `seq` used at the last push (dvo_affine_log); synchronises."""
        lg = AffineLog()
        lg.struct_size = C.sizeof(AffineLog)
        _check(lib().dvo_batch_last_affine_log(self._p, int(seq), C.byref(lg)))
        rec = np.frombuffer(lg, AFFINE_LOG_DTYPE)[0]
        return dict(levels=int(rec["levels"]), n_iter=rec["n_iter"].copy(), a=rec["a"].copy(), b=rec["b"].copy(),
                    prime_a=np.float32(rec["prime_a"]), prime_b=np.float32(rec["prime_b"]))


class _GeometricTerm:
    """The geometric (depth) term of a sensor-depth batch (dvo_batch_set_geometric, include/dvo.h)."""

    def set_geometric(self, mode=GEOMETRIC_ON, weight=10.0, max_diff=0.1):
        """GEOMETRIC_ON: every later push adds a depth-error row per pixel, on the tracked frame's own depth; GEOMETRIC_OFF or None: off."""
        if mode is None:
            _check(lib().dvo_batch_set_geometric(self._p, None))
            return
        c = GeometricConfig(C.sizeof(GeometricConfig), int(mode), float(weight), float(max_diff))
        _check(lib().dvo_batch_set_geometric(self._p, C.byref(c)))

    def set_geometric_affine(self, weight=10.0, max_diff=0.1, affine_mode=AFFINE_ESTIMATE, min_pixels=64, min_contrast=1e-3, gain_min=0.25,
                             gain_max=4.0):
        """The geometric term and affine brightness compensation together from the next push on (dvo_batch_set_geometric_affine,
        include/dvo.h); set_geometric(GEOMETRIC_OFF) / set_affine_brightness(AFFINE_OFF) turn either off again."""
        g = GeometricConfig(C.sizeof(GeometricConfig), GEOMETRIC_ON, float(weight), float(max_diff))
        a = AffineConfig(C.sizeof(AffineConfig), int(affine_mode), int(min_pixels), float(min_contrast), float(gain_min), float(gain_max))
        _check(lib().dvo_batch_set_geometric_affine(self._p, C.byref(g), C.byref(a)))

    def last_geometric(self):
        """record array [n_seq] (n_geo, mean_sq) of the finest level's last iteration at the last push (zeros: not tracked); synchronises."""
        rec = np.zeros(self.n_seq, GEOMETRIC_RECORD_DTYPE)
        _check(lib().dvo_batch_last_geometric(self._p, rec.ctypes.data_as(C.POINTER(GeometricRecord))))
        return rec

    def last_geometric_log(self, seq):
        """dict of n_geo and sum_sq of every logged iteration of `seq` at the last push (dvo_geometric_log); synchronises."""
        lg = GeometricLog()
        lg.struct_size = C.sizeof(GeometricLog)
        _check(lib().dvo_batch_last_geometric_log(self._p, int(seq), C.byref(lg)))
        rec = np.frombuffer(lg, GEOMETRIC_LOG_DTYPE)[0]
        return dict(levels=int(rec["levels"]), n_iter=rec["n_iter"].copy(), n_geo=rec["n_geo"].copy(), sum_sq=rec["sum_sq"].copy())


class _StepControl:
    """Step control of the tracking, shared by Batch and MonoBatch (dvo_batch_set_step_control, include/dvo.h)."""

    def set_step_control(self, mode=LM_ON, lambda0=1.0, lambda_up=4.0, lambda_down=0.5, lambda_floor=1e-4, lambda_max=1e6,
                         min_valid_fraction=0.5):
        """LM_ON: from the next push / call on every Gauss-Newton step is damped, compared with the pose it started from and taken
        only when it did not make the residual worse; LM_OFF or None: the plain iteration."""
        if mode is None:
            _check(lib().dvo_batch_set_step_control(self._p, None))
            return
        c = LmConfig(C.sizeof(LmConfig), int(mode), float(lambda0), float(lambda_up), float(lambda_down), float(lambda_floor),
                     float(lambda_max), float(min_valid_fraction))
        _check(lib().dvo_batch_set_step_control(self._p, C.byref(c)))

    def last_step_control(self):
        """record array [n_seq] (n_first, n_accepted, n_rejected, lambda, residual) of the last push (zeros: not tracked); synchronises."""
        rec = np.zeros(self.n_seq, LM_RECORD_DTYPE)
        _check(lib().dvo_batch_last_step_control(self._p, rec.ctypes.data_as(C.c_void_p)))
        return rec

    def last_step_control_log(self, seq):
        """dict of the lambda and the decision of every logged iteration of `seq` at the last push (dvo_lm_log); synchronises."""
        lg = LmLog()
        lg.struct_size = C.sizeof(LmLog)
        _check(lib().dvo_batch_last_step_control_log(self._p, int(seq), C.byref(lg)))
        rec = np.frombuffer(lg, LM_LOG_DTYPE)[0]
        return dict(levels=int(rec["levels"]), n_iter=rec["n_iter"].copy(), lambda_=rec["lambda"].copy(), decision=rec["decision"].copy())

    op_lm_step = staticmethod(op_lm_step)


class _KeyframeFusion:
    """Depth fusion into the keyframes of a sensor-depth batch with keyframe tracking (dvo_batch_set_keyframe_fusion, include/dvo.h)."""

    def set_keyframe_fusion(self, mode=KF_FUSION_ON, max_diff=0.05, max_count=16):
        """KF_FUSION_ON: every later push folds the tracked frame's depth into the keyframe it was tracked against (a running mean per
        pixel, gated by max_diff metres, at most max_count samples of memory); KF_FUSION_OFF or None: stop, the maps stay as they are."""
        if mode is None:
            _check(lib().dvo_batch_set_keyframe_fusion(self._p, None))
            return
        c = KfFusionConfig(int(mode), float(max_diff), int(max_count))
        _check(lib().dvo_batch_set_keyframe_fusion(self._p, C.byref(c)))

    def last_keyframe_fusion(self):
        """record array [n_seq] (n_candidates, n_fused, n_gated) of the last push (zeros: started, promoted or skipped); synchronises."""
        rec = np.zeros(self.n_seq, KF_FUSION_RECORD_DTYPE)
        _check(lib().dvo_batch_last_keyframe_fusion(self._p, rec.ctypes.data_as(C.POINTER(KfFusionRecord))))
        return rec

    def keyframe_fusion_counts(self, seq):
        """uint8 [h_top, w_top]: how many samples each pixel of sequence `seq`'s keyframe depth has fused (capped at max_count)."""
        shift = self.culls
        c = np.zeros((self.height >> shift, self.width >> shift), np.uint8)
        _check(lib().dvo_batch_keyframe_fusion_counts(self._p, int(seq), c.ctypes.data_as(C.c_void_p)))
        return c

    def set_keyframe_carry(self, mode=KF_CARRY_ON, max_diff=0.05):
        """KF_CARRY_ON (needs fusion on): every later promotion blends the old keyframe's fused depth, warped into the frame that becomes
        the keyframe, into that frame's depth and carries the counts along, so the map outlives its keyframe; KF_CARRY_OFF or None:
        stop, maps and counts stay as they are.  After a carrying push frame() returns the carried depth for the promoted sequences."""
        if mode is None:
            _check(lib().dvo_batch_set_keyframe_carry(self._p, None))
            return
        c = KfCarryConfig(int(mode), float(max_diff))
        _check(lib().dvo_batch_set_keyframe_carry(self._p, C.byref(c)))

    def last_keyframe_carry(self):
        """record array [n_seq] (n_candidates, n_carried, n_gated) of the last push (zeros: the sequence did not promote); synchronises."""
        rec = np.zeros(self.n_seq, KF_CARRY_RECORD_DTYPE)
        _check(lib().dvo_batch_last_keyframe_carry(self._p, rec.ctypes.data_as(C.POINTER(KfCarryRecord))))
        return rec


class PointsConfig(C.Structure):
    """dvo_points_config (include/dvo.h): which keyframe pixels dvo_batch_export_points exports."""
    _fields_ = [("struct_size", C.c_int), ("select", C.c_int), ("level", C.c_int), ("stride", C.c_int), ("min_depth", C.c_float),
                ("max_depth", C.c_float), ("max_sigma", C.c_float), ("min_age", C.c_float), ("min_count", C.c_int)]


# which sequences an export selects (PointsConfig.select): include/dvo.h
POINTS_ALL, POINTS_NEW = 0, 1


def points_config(**kw):
    """dvo_points_config_default (every started sequence, top level, stride 1, the handle's min_depth, no other gate) with `kw` set"""
    c = PointsConfig()
    lib().dvo_points_config_default(C.byref(c))
    for k, v in kw.items():
        if not hasattr(c, k):
            raise AttributeError(k)
        setattr(c, k, v)
    return c


class _PointsExport:
    """The keyframe maps as compacted world-frame point clouds, shared by MonoBatch and a Batch with keyframe tracking
    (dvo_batch_export_points, include/dvo.h)."""

    def export_points(self, cfg, capacity, xyzg_ptr, src_ptr, sigma_ptr, offsets_ptr):
        """Device pointers (ints): float32 [capacity, 4], uint32 [capacity] or 0, float32 [capacity] or 0 (mono only), uint32 [n_seq + 1].
        Asynchronous on the handle's stream; cfg None = points_config()."""
        c = cfg if cfg is not None else points_config()
        _check(lib().dvo_batch_export_points(self._p, C.byref(c), C.c_uint32(int(capacity)), C.c_void_p(xyzg_ptr or None),
                                             C.c_void_p(src_ptr or None), C.c_void_p(sigma_ptr or None), C.c_void_p(offsets_ptr or None)))

    def last_points(self):
        """uint32 [n_seq + 1]: the offsets of the last export_points (the last entry is the total); synchronises."""
        off = np.zeros(self.n_seq + 1, np.uint32)
        _check(lib().dvo_batch_last_points(self._p, off.ctypes.data_as(C.c_void_p)))
        return off

    def export_points_torch(self, cfg=None, capacity=None, want_src=True, want_sigma=False, device="cuda"):
        """Allocates torch tensors and exports into them: (xyzg float32 [n, 4], src int32 [n] or None, sigma float32 [n] or None,
        offsets int32 [n_seq + 1]), n = min(total, capacity).  capacity None: a counting call first, then exactly the total
        (two synchronisations); otherwise one call and one synchronisation."""
        import torch
        off = torch.empty(self.n_seq + 1, dtype=torch.int32, device=device)
        if capacity is None:
            self.export_points(cfg, 0, 0, 0, 0, off.data_ptr())
            capacity = int(self.last_points()[-1])
        cap = int(capacity)
        xyzg = torch.empty((max(cap, 1), 4), dtype=torch.float32, device=device)
        src = torch.empty(max(cap, 1), dtype=torch.int32, device=device) if want_src else None
        sig = torch.empty(max(cap, 1), dtype=torch.float32, device=device) if want_sigma else None
        torch.cuda.synchronize()   # (the handle works on its own stream: nothing of torch's may still be pending on these blocks)
        self.export_points(cfg, cap, xyzg.data_ptr(), src.data_ptr() if want_src else 0, sig.data_ptr() if want_sigma else 0, off.data_ptr())
        n = min(int(self.last_points()[-1]), cap)
        return xyzg[:n], (src[:n] if want_src else None), (sig[:n] if want_sigma else None), off


class _WorldPoses:
    """World poses of the last frame, shared by MonoBatch and a Batch with keyframe tracking (dvo_batch_world_poses, include/dvo.h)."""

    def world_poses(self):
        xi = np.zeros((self.n_seq, 6), np.float32); T = np.zeros((self.n_seq, 16), np.float32); key = np.zeros(self.n_seq, np.int32)
        _check(lib().dvo_batch_world_poses(self._p, fp(xi), fp(T), key.ctypes.data_as(C.c_void_p)))
        return xi, T.reshape(self.n_seq, 4, 4), key.astype(bool)

    def copy_world_poses_device(self, xi_ptr=0, T_ptr=0, key_ptr=0):
        _check(lib().dvo_batch_copy_world_poses_device(self._p, C.c_void_p(xi_ptr or None), C.c_void_p(T_ptr or None), C.c_void_p(key_ptr or None)))


# ------------------------------------------------------------------ batched tracking (n_seq sequences per GPU)
class Batch(_PoseGuess, _WorldPoses, _PointsExport, _TrackQuality, _RobustWeights, _AffineBrightness, _GeometricTerm, _KeyframeFusion, _StepControl):
    def __init__(self, n_seq, K, width, height, levels=4, culls=1, cfg=None):
        K = f32(K).reshape(9)
        self.n_seq, self.width, self.height, self.levels, self.culls = n_seq, width, height, levels, culls
        self._p = C.c_void_p()
        _check(lib().dvo_batch_create(n_seq, fp(K), width, height, levels, culls,
                                      C.byref(cfg) if cfg is not None else None, C.byref(self._p)))

    def close(self):
        if self._p:
            lib().dvo_batch_destroy(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def push_device(self, gray_ptr, depth_ptr, sigma_ptr):
        """Device pointers (ints, e.g. torch.Tensor.data_ptr()) to [n_seq, H, W] float32."""
        _check(lib().dvo_batch_push_device(self._p, C.c_void_p(gray_ptr), C.c_void_p(depth_ptr), C.c_void_p(sigma_ptr)))

    def prefetch_device(self, gray_ptr, depth_ptr, sigma_ptr):
        """Build the pyramids of the frame that the NEXT push_device will receive, on a side stream (the buffers must be complete)."""
        _check(lib().dvo_batch_prefetch_device(self._p, C.c_void_p(gray_ptr), C.c_void_p(depth_ptr), C.c_void_p(sigma_ptr)))

    def push_host(self, gray, depth, sigma):
        g = f32(gray); d = f32(depth); s = f32(sigma)
        assert g.shape == (self.n_seq, self.height, self.width)
        _check(lib().dvo_batch_push_host(self._p, fp(g), fp(d), fp(s)))

    def push_raw_device(self, rgb_ptr, channels, depth16_ptr, depth_scale=1.0 / 5000.0):
        """Device pointers to raw frames: [n_seq, H, W(, C)] uint8 and [n_seq, H, W] uint16 (converted inside the pyramid kernel)."""
        _check(lib().dvo_batch_push_raw_device(self._p, C.c_void_p(rgb_ptr), int(channels), C.c_void_p(depth16_ptr), C.c_float(depth_scale)))

    def prefetch_raw_device(self, rgb_ptr, channels, depth16_ptr, depth_scale=1.0 / 5000.0):
        _check(lib().dvo_batch_prefetch_raw_device(self._p, C.c_void_p(rgb_ptr), int(channels), C.c_void_p(depth16_ptr), C.c_float(depth_scale)))

    def push_raw_host(self, rgb_u8, depth_u16, depth_scale=1.0 / 5000.0):
        rgb = np.ascontiguousarray(rgb_u8, np.uint8); d16 = np.ascontiguousarray(depth_u16, np.uint16)
        ch = 1 if rgb.ndim == 3 else rgb.shape[3]
        assert rgb.shape[:3] == (self.n_seq, self.height, self.width) and d16.shape == (self.n_seq, self.height, self.width)
        _check(lib().dvo_batch_push_raw_host(self._p, rgb.ctypes.data_as(C.c_void_p), ch, d16.ctypes.data_as(C.c_void_p), C.c_float(depth_scale)))

    def last_poses(self):
        xi = np.zeros((self.n_seq, 6), np.float32); T = np.zeros((self.n_seq, 16), np.float32)
        _check(lib().dvo_batch_last_poses(self._p, fp(xi), fp(T)))
        return xi, T.reshape(self.n_seq, 4, 4)

    def copy_poses_device(self, xi_ptr, T_ptr=0):
        """Async D2D copy of the last poses into device memory (ints = device pointers, 0 = skip)."""
        _check(lib().dvo_batch_copy_poses_device(self._p, C.c_void_p(xi_ptr or None), C.c_void_p(T_ptr or None)))

    def last_track_log(self, seq):
        log = TrackLog()
        _check(lib().dvo_batch_last_track_log(self._p, seq, C.byref(log)))
        return log.to_dict()

    def level_plan(self, level):
        """Diagnostic: the kernel instance and tiles the next push / call runs on pyramid level `level` (0 = coarsest), with the
        opt-in terms as they are set now: dict(ppt, group, tiles_2d, tiles, schedule = PLAN_*).  Reads the plan only."""
        return _level_plan(self._p, level)

    def set_actions(self, actions, on_device=False):
        """Per-sequence action of the NEXT push (SEQ_SKIP / SEQ_TRACK / SEQ_RESTART): a numpy uint8 [n_seq] (copied now), an int device
        pointer to uint8 [n_seq] with on_device=True (read in stream order when the push runs), or None to clear."""
        if actions is None:
            _check(lib().dvo_batch_set_actions(self._p, None, 0))
        elif on_device:
            _check(lib().dvo_batch_set_actions(self._p, C.c_void_p(int(actions)), 1))
        else:
            a = np.ascontiguousarray(actions, np.uint8)
            if a.shape != (self.n_seq,):
                raise ValueError("set_actions: expected uint8[%d], got shape %s" % (self.n_seq, a.shape))
            _check(lib().dvo_batch_set_actions(self._p, a.ctypes.data_as(C.c_void_p), 0))

    def last_status(self):
        """int32 [n_seq]: SEQ_TRACKED / SEQ_SKIPPED / SEQ_STARTED / SEQ_BAD_ACTION of the last push (synchronises)."""
        st = np.zeros(self.n_seq, np.int32)
        _check(lib().dvo_batch_last_status(self._p, st.ctypes.data_as(C.c_void_p)))
        return st

    def set_intrinsics(self, K):
        """Per-sequence camera intrinsics from the NEXT push on: float [n_seq, 3, 3] or [n_seq, 9] (row-major, copied now), or None for
        the creation K of every sequence.  A sequence whose fx, fy, cx or cy change loses its reference at that push (include/dvo.h)."""
        if K is None:
            _check(lib().dvo_batch_set_intrinsics(self._p, None))
            return
        k = np.ascontiguousarray(K, np.float32)
        if k.shape not in ((self.n_seq, 3, 3), (self.n_seq, 9)):
            raise ValueError("set_intrinsics: expected float[%d, 3, 3] or float[%d, 9], got shape %s" % (self.n_seq, self.n_seq, k.shape))
        _check(lib().dvo_batch_set_intrinsics(self._p, k.ctypes.data_as(C.c_void_p)))

    def intrinsics(self):
        """float32 [n_seq, 3, 3]: the intrinsics the next push uses (the creation K until set_intrinsics)."""
        k = np.zeros((self.n_seq, 3, 3), np.float32)
        _check(lib().dvo_batch_get_intrinsics(self._p, k.ctypes.data_as(C.c_void_p)))
        return k

    def set_distortion(self, D):
        """Undistort every frame from the NEXT push on with each sequence's current K: D float [5] for every sequence or [n_seq, 5],
        OpenCV order (k1, k2, p1, p2, k3); None clears.  A sequence whose D changes loses its reference at that push
        (dvo_batch_set_sensor_distortion)."""
        if D is None:
            _check(lib().dvo_batch_set_sensor_distortion(self._p, None, 0))
            return
        d = f32(D)
        if d.shape not in ((5,), (self.n_seq, 5)):
            raise ValueError("set_distortion: expected float[5] or float[%d, 5], got shape %s" % (self.n_seq, d.shape))
        _check(lib().dvo_batch_set_sensor_distortion(self._p, fp(d), 1 if d.ndim == 2 else 0))

    def distortion(self):
        """(D float32 [n_seq, 5], enabled): the coefficients the next push uses (zeros when none)."""
        d = np.zeros((self.n_seq, 5), np.float32); en = C.c_int(0)
        _check(lib().dvo_batch_get_sensor_distortion(self._p, fp(d), C.byref(en)))
        return d, bool(en.value)

    def set_pyramid_filter(self, filter=PYRAMID_FILTER_BINOMIAL3):
        """Build the gray pyramid of every frame with a 3x3 binomial filter before each halving (PYRAMID_FILTER_BINOMIAL3) or by
        decimation (PYRAMID_FILTER_NONE, the default); before the first push or prefetch (dvo_batch_set_pyramid_filter)."""
        _check(lib().dvo_batch_set_pyramid_filter(self._p, int(filter)))

    def pyramid_filter(self):
        """The PYRAMID_FILTER_* in force (dvo_batch_pyramid_filter)."""
        f = C.c_int(-1)
        _check(lib().dvo_batch_pyramid_filter(self._p, C.byref(f)))
        return f.value

    def copy_status_device(self, ptr):
        """Async D2D copy of last_status() into device memory int32 [n_seq] (int = device pointer)."""
        _check(lib().dvo_batch_copy_status_device(self._p, C.c_void_p(int(ptr))))

    def set_keyframe_tracking(self, enable=True):
        """Track every frame against its sequence's keyframe (the mono rule decides when it is replaced) instead of the previous frame;
        before the first push (dvo_batch_set_keyframe_tracking).  world_poses(), copy_world_poses_device() and keyframe() then work."""
        _check(lib().dvo_batch_set_keyframe_tracking(self._p, 1 if enable else 0))

    def keyframe(self, seq, level=None):
        """The keyframe of sequence `seq` (keyframe tracking): gray and depth of `level` (default: the finest), its world twist, id and the
        number of keyframes the sequence has created."""
        level = self.levels - 1 if level is None else level
        if not 0 <= level < self.levels:
            raise ValueError("keyframe: level %d is outside [0, %d)" % (level, self.levels))
        shift = self.culls + (self.levels - 1 - level)
        sh = (self.height >> shift, self.width >> shift)
        g = np.zeros(sh, np.float32); d = np.zeros(sh, np.float32)
        xi = np.zeros(6, np.float32); i = C.c_int(); n = C.c_int(); v = C.c_int()
        _check(lib().dvo_batch_keyframe_get(self._p, seq, level, fp(g), fp(d), None, None, fp(xi), C.byref(i), C.byref(n), C.byref(v)))
        return dict(gray=g, depth=d, xi=xi, id=i.value, n_keyframes=n.value)

    def frame(self, seq, level=None):
        """Gray and depth of `level` (default: the finest) of the last pushed frame of sequence `seq`: the next push's reference (with
        keyframe tracking: the frame the last push tracked; the references are the keyframes)."""
        level = self.levels - 1 if level is None else level
        if not 0 <= level < self.levels:
            raise ValueError("frame: level %d is outside [0, %d)" % (level, self.levels))
        shift = self.culls + (self.levels - 1 - level)
        sh = (self.height >> shift, self.width >> shift)
        g = np.zeros(sh, np.float32); d = np.zeros(sh, np.float32)
        _check(lib().dvo_batch_frame_get(self._p, seq, level, fp(g), fp(d)))
        return g, d

    def synchronize(self):
        _check(lib().dvo_batch_synchronize(self._p))

    def profile(self, reset=False):
        p = GnProfile()
        _check(lib().dvo_batch_profile(self._p, C.byref(p), 1 if reset else 0))
        return dict(gn_ms=p.gn_ms, gn_launches=p.gn_launches, gn_pixels=p.gn_pixels, gn_iterations=p.gn_iterations)

    def probe_gn(self, level, n_launches):
        ms = C.c_float(); px = C.c_uint64()
        _check(lib().dvo_batch_probe_gn(self._p, level, n_launches, C.byref(ms), C.byref(px)))
        return ms.value, px.value


class MonoBatch(_PoseGuess, _WorldPoses, _PointsExport, _TrackQuality, _RobustWeights, _AffineBrightness, _StepControl):
    """n_seq mono sequences per GPU: System::VisualOdometry::odometrize (track + Mapper::estimate + regularize, system.hpp:44-74,
    src/map/mapper.cpp:16-144) for every sequence per call, keyframe decisions on the device (dvo_batch_create_mono)."""

    def __init__(self, n_seq, K, width, height, ring_keyframes=8, cfg=None, per_sequence_K=False):
        """K: one camera for every sequence, float [3, 3] or [9].  per_sequence_K=True: K is a table with one camera per sequence,
        float [n_seq, 3, 3] or [n_seq, 9], fixed for the life of the batch (dvo_batch_create_mono_cameras)."""
        self.n_seq, self.width, self.height = n_seq, width, height
        self._p = C.c_void_p()
        if per_sequence_K:
            k = np.ascontiguousarray(K, np.float32)
            if k.shape not in ((n_seq, 3, 3), (n_seq, 9)):
                raise ValueError("MonoBatch: per_sequence_K expects float[%d, 3, 3] or float[%d, 9], got shape %s" % (n_seq, n_seq, k.shape))
            _check(lib().dvo_batch_create_mono_cameras(n_seq, fp(k), width, height, ring_keyframes,
                                                       C.byref(cfg) if cfg is not None else None, C.byref(self._p)))
            return
        K = f32(K).reshape(9)
        _check(lib().dvo_batch_create_mono(n_seq, fp(K), width, height, ring_keyframes,
                                           C.byref(cfg) if cfg is not None else None, C.byref(self._p)))

    def close(self):
        if self._p:
            lib().dvo_batch_destroy(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def setInitialDepth(self, depth, sigma):
        d = f32(depth); s = f32(sigma)
        assert d.shape == (self.height // 4, self.width // 4)
        _check(lib().dvo_batch_set_initial_depth(self._p, fp(d), fp(s)))

    def set_distortion(self, D):
        """Undistort every frame (Loader::getNormalizedUndistortedImages) with each sequence's creation K: D float [5] for every
        sequence or [n_seq, 5], OpenCV order (k1, k2, p1, p2, k3); None clears.  Before the first frame (dvo_batch_set_distortion)."""
        if D is None:
            _check(lib().dvo_batch_set_distortion(self._p, None, 0))
            return
        d = f32(D)
        if d.shape not in ((5,), (self.n_seq, 5)):
            raise ValueError("set_distortion: expected float[5] or float[%d, 5], got shape %s" % (self.n_seq, d.shape))
        _check(lib().dvo_batch_set_distortion(self._p, fp(d), 1 if d.ndim == 2 else 0))

    def distortion(self):
        """(D float32 [n_seq, 5], enabled): the coefficients in use (zeros when none)."""
        d = np.zeros((self.n_seq, 5), np.float32); en = C.c_int(0)
        _check(lib().dvo_batch_get_distortion(self._p, fp(d), C.byref(en)))
        return d, bool(en.value)

    def set_photometric(self, inv_response=None, vignette=None, seq_cal=None):
        """Photometric calibration of every raw frame (dvo_batch_set_photometric): inv_response float [n_cal, 256] (or [256]) in gray
        units, None = i / 255; vignette float [n_cal, H, W] (or [H, W]), None = 1, an entry <= 0 or not finite masks the pixel; seq_cal
        int [n_seq] = the calibration of each sequence, None = 0 for all.  gray = inv_response[g8] * (1 / vignette), on the luma of a
        colour frame.  All None clears.  Before the first frame; from then on only raw frames are accepted."""
        if inv_response is None and vignette is None:
            _check(lib().dvo_batch_set_photometric(self._p, 0, None, None, None))
            return
        first = inv_response if inv_response is not None else vignette
        lead = np.ndim(first) - (1 if inv_response is not None else 2)
        n_cal = int(np.shape(first)[0]) if lead == 1 else 1
        r, v = _photometric_arrays("set_photometric", n_cal, inv_response, vignette, self.height, self.width)
        sc = None
        if seq_cal is not None:
            sc = np.ascontiguousarray(seq_cal, np.int32)
            if sc.shape != (self.n_seq,):
                raise ValueError("set_photometric: seq_cal must be int[%d], got shape %s" % (self.n_seq, sc.shape))
        _check(lib().dvo_batch_set_photometric(self._p, n_cal, fp(r) if r is not None else None, fp(v) if v is not None else None,
                                               sc.ctypes.data_as(C.c_void_p) if sc is not None else None))

    def get_photometric(self):
        """(n_cal, seq_cal int32 [n_seq]): the number of calibrations in use (0: none) and each sequence's."""
        n = C.c_int(0); sc = np.zeros(self.n_seq, np.int32)
        _check(lib().dvo_batch_get_photometric(self._p, C.byref(n), sc.ctypes.data_as(C.c_void_p)))
        return n.value, sc

    def photometric_gain(self, seq):
        """Diagnostic: the gain table sequence `seq` reads, float32 [H/4, W/4]: 1 / vignette at each kept pixel's source, -1 where the
        pixel is masked or outside the undistorted image (dvo_debug_batch_photometric_gain; synchronises)."""
        g = np.zeros((self.height // 4, self.width // 4), np.float32)
        _check(lib().dvo_debug_batch_photometric_gain(self._p, int(seq), fp(g)))
        return g

    def last_pyramid_kernel(self):
        """Diagnostic: the PyramidKernel (kind, culls, plan) the last frame build launched (dvo_debug_batch_last_pyramid_kernel)."""
        k = PyramidKernel()
        _check(lib().dvo_debug_batch_last_pyramid_kernel(self._p, C.byref(k)))
        return k

    def setInitialDepthDevice(self, depth_ptr, sigma_ptr):
        _check(lib().dvo_batch_set_initial_depth_device(self._p, C.c_void_p(depth_ptr), C.c_void_p(sigma_ptr)))

    def odometrize_device(self, gray_ptr):
        """Device pointer (int) to [n_seq, H, W] float32 gray frames."""
        _check(lib().dvo_batch_odometrize_device(self._p, C.c_void_p(gray_ptr)))

    def odometrize_raw_device(self, rgb_ptr, channels):
        """Device pointer (int) to [n_seq, H, W(, C)] uint8 frames (gray / RGB / RGBA)."""
        _check(lib().dvo_batch_odometrize_raw_device(self._p, C.c_void_p(rgb_ptr), int(channels)))

    def odometrize_host(self, frames):
        """Host frames [n_seq, H, W]: float32 gray, or uint8 gray / [n_seq, H, W, C] uint8 colour (raw, converted on the device)."""
        a = np.ascontiguousarray(frames)
        assert a.shape[:3] == (self.n_seq, self.height, self.width)
        if a.dtype == np.uint8:
            _check(lib().dvo_batch_odometrize_raw_host(self._p, a.ctypes.data_as(C.c_void_p), 1 if a.ndim == 3 else a.shape[3]))
        else:
            a = f32(a)
            _check(lib().dvo_batch_odometrize_host(self._p, fp(a)))

    def set_actions(self, actions, on_device=False):
        """Per-sequence action of the NEXT call (SEQ_SKIP / SEQ_TRACK / SEQ_RESTART): a numpy uint8 [n_seq] (copied now), an int device
        pointer to uint8 [n_seq] with on_device=True (read in stream order when the call runs), or None to clear
        (dvo_batch_set_mono_actions)."""
        if actions is None:
            _check(lib().dvo_batch_set_mono_actions(self._p, None, 0))
        elif on_device:
            _check(lib().dvo_batch_set_mono_actions(self._p, C.c_void_p(int(actions)), 1))
        else:
            a = np.ascontiguousarray(actions, np.uint8)
            assert a.shape == (self.n_seq,)
            _check(lib().dvo_batch_set_mono_actions(self._p, a.ctypes.data_as(C.c_void_p), 0))

    def last_status(self):
        """int32 [n_seq]: SEQ_TRACKED / SEQ_SKIPPED / SEQ_STARTED / SEQ_BAD_ACTION of the last call (synchronises)."""
        st = np.zeros(self.n_seq, np.int32)
        _check(lib().dvo_batch_mono_last_status(self._p, st.ctypes.data_as(C.c_void_p)))
        return st

    def copy_status_device(self, ptr):
        """Async D2D copy of last_status() into device memory int32 [n_seq] (int = device pointer)."""
        _check(lib().dvo_batch_copy_mono_status_device(self._p, C.c_void_p(int(ptr))))

    def set_start_depth_device(self, depth_ptr, sigma_ptr):
        """Start maps [n_seq, H/4, W/4] float32 (int device pointers) of the sequences that start in the NEXT call; 0, 0 (or None) clears
        (dvo_batch_set_mono_start_depth_device)."""
        _check(lib().dvo_batch_set_mono_start_depth_device(self._p, C.c_void_p(int(depth_ptr) if depth_ptr else None),
                                                            C.c_void_p(int(sigma_ptr) if sigma_ptr else None)))

    def keyframe(self, seq, level=2):
        sh = ((self.height // 4) >> (2 - level), (self.width // 4) >> (2 - level))
        g = np.zeros(sh, np.float32); d = np.zeros(sh, np.float32); s = np.zeros(sh, np.float32)
        a = np.zeros(sh, np.float32) if level == 2 else None
        xi = np.zeros(6, np.float32); i = C.c_int(); n = C.c_int(); v = C.c_int()
        _check(lib().dvo_batch_keyframe_get(self._p, seq, level, fp(g), fp(d), fp(s), fp(a) if a is not None else None, fp(xi),
                                            C.byref(i), C.byref(n), C.byref(v)))
        return dict(gray=g, depth=d, sigma=s, age=a, xi=xi, id=i.value, n_keyframes=n.value, valid_updates=v.value)

    def last_track_log(self, seq):
        log = TrackLog()
        _check(lib().dvo_batch_last_track_log(self._p, seq, C.byref(log)))
        return log.to_dict()

    def level_plan(self, level):
        """Diagnostic: the kernel instance and tiles the next push / call runs on pyramid level `level` (0 = coarsest), with the
        opt-in terms as they are set now: dict(ppt, group, tiles_2d, tiles, schedule = PLAN_*).  Reads the plan only."""
        return _level_plan(self._p, level)

    def synchronize(self):
        _check(lib().dvo_batch_synchronize(self._p))

    def stats(self, seq):
        """per-sequence counters (dvo_mono_stats): frames, keyframes created, ring size, valid updates of the last frame and the
        cumulative number of pixels whose birth keyframe had left the ring (searched against the oldest retained one instead)"""
        st = MonoStats()
        _check(lib().dvo_batch_mono_stats(self._p, seq, C.byref(st)))
        return {k: getattr(st, k) for k, _ in MonoStats._fields_}

    def profile_mapping(self, reset=False):
        p = MapProfile()
        _check(lib().dvo_batch_profile_mapping(self._p, C.byref(p), 1 if reset else 0))
        return {k: getattr(p, k) for k, _ in MapProfile._fields_}

    def profile(self, reset=False):
        p = GnProfile()
        _check(lib().dvo_batch_profile(self._p, C.byref(p), 1 if reset else 0))
        return dict(gn_ms=p.gn_ms, gn_launches=p.gn_launches, gn_pixels=p.gn_pixels, gn_iterations=p.gn_iterations)
