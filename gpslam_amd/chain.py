"""ctypes binding of libgpslam_hip.so: one ChainSolver = one gpslam_hip_handle = one GPU stream.

Mirrors the reference's usage pattern (NonlinearFactorGraph::add / Values::insert / optimizer.iterate(),
e.g. gpslam/gp/tests/testGaussianProcessPriorPose3.cpp:172-188) on arrays instead of per-factor objects.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

LINEAR2, LINEAR3, POSE2, POSE3, ROT3, ROT3_BIAS = 0, 1, 2, 3, 4, 5
CHART_EXPMAP, CHART_FIRST_ORDER = 0, 1
FP64, FP32 = 0, 1
# noiseModel::Robust: GPSLAM_ROBUST_* (mEstimator::Huber, Cauchy, Tukey, GemanMcClure, Welsh, Fair) and GPSLAM_MEAS_* of include/gpslam_hip.h
ROBUST_NONE, ROBUST_HUBER, ROBUST_CAUCHY, ROBUST_TUKEY, ROBUST_GEMAN_MCCLURE, ROBUST_WELSH, ROBUST_FAIR = 0, 1, 2, 3, 4, 5, 6
MEAS_INTERP_RANGE, MEAS_RANGE, MEAS_INTERP_ATTITUDE, MEAS_INTERP_GPS, MEAS_ODOMETRY2D, MEAS_BEARING_RANGE, MEAS_INTERP_PROJECTION, MEAS_AHRS = range(8)
# gpslam_hip_config_v2.plan: kernel families compile() is told to use instead of its default choice (include/gpslam_hip.h)
PLAN_UNFUSED_LEVEL0, PLAN_COLUMN_LEVEL0, PLAN_LEVELS_OF_FOUR, PLAN_FS_TWO_LAUNCHES, PLAN_GP_ROWS, PLAN_GENERIC_QC, PLAN_MEAS_ROWS, PLAN_SEPARATE_RETRACT = 1, 2, 4, 8, 16, 32, 64, 128
# Test harness hook of this PYTHON mirror (the library itself reads no environment): plan bits OR-ed into every ChainSolver a
# process creates, so that tests/test_gpu_switches.py can re-run whole parity suites on the fallback kernel families.
_DEFAULT_PLAN = int(os.environ.get("GPSLAM_PY_DEFAULT_PLAN", "0"))
POSE_DIM = {LINEAR2: 2, LINEAR3: 3, POSE2: 3, POSE3: 12, ROT3: 9, ROT3_BIAS: 12}
TANGENT_DIM = {LINEAR2: 2, LINEAR3: 3, POSE2: 3, POSE3: 6, ROT3: 3, ROT3_BIAS: 6}

# every symbol include/gpslam_hip.h declares
ABI_SYMBOLS = [
    "gpslam_hip_create", "gpslam_hip_destroy", "gpslam_hip_default_params", "gpslam_hip_last_error",
    "gpslam_hip_stream", "gpslam_hip_set_stream", "gpslam_hip_set_states", "gpslam_hip_get_states", "gpslam_hip_set_landmarks",
    "gpslam_hip_get_landmarks", "gpslam_hip_set_qc", "gpslam_hip_add_gp_priors", "gpslam_hip_add_pose_priors",
    "gpslam_hip_add_vel_priors", "gpslam_hip_add_between", "gpslam_hip_add_landmark_priors",
    "gpslam_hip_add_interp_range", "gpslam_hip_add_range", "gpslam_hip_add_interp_attitude",
    "gpslam_hip_add_interp_gps", "gpslam_hip_add_odometry2d", "gpslam_hip_add_bearing_range", "gpslam_hip_compile",
    "gpslam_hip_linearize_gp", "gpslam_hip_error", "gpslam_hip_iterate_gn", "gpslam_hip_iterate_lm",
    "gpslam_hip_optimize", "gpslam_hip_normal_equations", "gpslam_hip_get_rows", "gpslam_hip_block_tridiag_solve",
    "gpslam_hip_last_timing", "gpslam_hip_run_gn", "gpslam_hip_time_kernel", "gpslam_hip_interface_send", "gpslam_hip_interface_recv",
    "gpslam_hip_iterate_phase1", "gpslam_hip_iterate_phase2", "gpslam_hip_set_halo_state",
    "gpslam_hip_interpolate_poses", "gpslam_hip_add_interp_projection", "gpslam_hip_add_interp_projection_ds2", "gpslam_hip_iterate_phase2a",
    "gpslam_hip_iterate_phase2b", "gpslam_hip_landmark_reduce_buffer", "gpslam_hip_lm_begin",
    "gpslam_hip_lm_trial_phase1", "gpslam_hip_lm_trial_phase2", "gpslam_hip_lm_reject", "gpslam_hip_clear_factors", "gpslam_hip_segment_plan", "gpslam_hip_linearize_meas", "gpslam_hip_interpolate_poses_jac",
    "gpslam_hip_add_ahrs", "gpslam_hip_plan_info", "gpslam_hip_fs_set_split", "gpslam_hip_fs_split_info", "gpslam_hip_fs_set_top",
    "gpslam_hip_fs_interface", "gpslam_hip_fs_phase1", "gpslam_hip_fs_phase2", "gpslam_hip_fs_lm_trial_phase1",
    "gpslam_hip_fs_lm_trial_phase2", "gpslam_hip_add_gp_priors_qc", "gpslam_hip_set_meas_covariance",
    "gpslam_hip_interpolate_velocities", "gpslam_hip_body_centric_velocity", "gpslam_hip_last_level0_ms",
    "gpslam_hip_lm_decide", "gpslam_hip_set_collectives", "gpslam_hip_create_v2", "gpslam_hip_abi_version", "gpslam_hip_struct_size",
    "gpslam_hip_add_between_pairs", "gpslam_hip_set_level0_stamps",
    "gpslam_hip_marginals", "gpslam_hip_get_marginals", "gpslam_hip_interpolate_covariances",
    "gpslam_hip_launch_census",
    "gpslam_hip_set_meas_robust", "gpslam_hip_set_between_pairs_robust", "gpslam_hip_get_meas_weights",
    "gpslam_hip_get_between_pairs_weights", "gpslam_hip_robust_eval",
    "gpslam_hip_set_closure_passes", "gpslam_hip_closure_info",
    "gpslam_hip_marginals_keep_closure_columns",
    "gpslam_hip_marginals_on_segments", "gpslam_hip_get_landmark_marginals", "gpslam_hip_get_state_landmark_marginals",
    "gpslam_hip_get_landmark_pair_marginals",
    "gpslam_hip_add_state_gaussians", "gpslam_hip_get_state_gaussians", "gpslam_hip_marginalize_head", "gpslam_hip_get_head_prior",
    "gpslam_hip_append_states",
    "gpslam_hip_add_border_gaussians", "gpslam_hip_get_border_gaussians", "gpslam_hip_marginalize_head_onto_landmarks",
    "gpslam_hip_get_head_prior_border",
    "gpslam_hip_marginals_keep_pair_terms", "gpslam_hip_get_state_pair_marginals", "gpslam_hip_gate_between_pairs",
]
# every symbol include/gpslam_hip_dogleg.h declares (Powell's dogleg; a list of its own: the ABI stays 2.4 and these entry points are
# detected by presence)
DOGLEG_SYMBOLS = [
    "gpslam_hip_dogleg_point", "gpslam_hip_dogleg_decide", "gpslam_hip_iterate_dogleg", "gpslam_hip_optimize_dogleg",
    "gpslam_hip_dogleg_last",
]
DOGLEG_ONE_STEP_PER_ITERATION, DOGLEG_SEARCH_EACH_ITERATION, DOGLEG_SEARCH_REDUCE_ONLY = 0, 1, 2
# every symbol include/gpslam_hip_evidence.h declares (log det H, the Laplace log-evidence; a list of its own, as the dogleg's)
EVIDENCE_SYMBOLS = [
    "gpslam_hip_log_determinant", "gpslam_hip_log_noise_normaliser", "gpslam_hip_log_evidence",
    "gpslam_hip_gp_log_normaliser", "gpslam_hip_evidence_combine",
]
# every symbol include/gpslam_hip_qc.h declares (learning Qc: the statistic A, its gradient, the EM update; a list of its own again)
QC_SYMBOLS = [
    "gpslam_hip_qc_statistic", "gpslam_hip_qc_gradient", "gpslam_hip_qc_em_update", "gpslam_hip_qc_em_scale",
]
# every symbol include/gpslam_hip_sampling.h declares (draws from N(x^, H^-1) by perturbed solves; a list of its own again)
SAMPLING_SYMBOLS = [
    "gpslam_hip_posterior_noise_dim", "gpslam_hip_posterior_noise", "gpslam_hip_sample_posterior",
]
# every symbol include/gpslam_hip_sampling_at.h declares (the same draws at query times between the support states, with the GP's
# conditional noise; a list of its own again)
SAMPLING_AT_SYMBOLS = [
    "gpslam_hip_posterior_noise_dim_at", "gpslam_hip_posterior_noise_at", "gpslam_hip_sample_posterior_at",
]
# every symbol include/gpslam_hip_sampling_stats.h declares (those draws reduced on the device to moment sums, collision counts,
# clearances and path lengths; a list of its own again)
SAMPLING_STATS_SYMBOLS = [
    "gpslam_hip_sample_posterior_stats", "gpslam_hip_posterior_moments",
]
# every symbol include/gpslam_hip_noise.h declares (learning measurement noise: the per-kind statistic, the predicted covariances, the
# gradient, the EM updates; a list of its own again)
NOISE_SYMBOLS = [
    "gpslam_hip_meas_noise_statistic", "gpslam_hip_meas_predicted_covariances", "gpslam_hip_noise_gradient",
    "gpslam_hip_noise_em_update", "gpslam_hip_noise_em_scale",
]
# the version of include/gpslam_hip.h this binding's structs mirror (GPSLAM_HIP_ABI_MAJOR / _MINOR); load_library() checks the library's
ABI_MAJOR, ABI_MINOR = 2, 4
STRUCT_CONFIG, STRUCT_CONFIG_V2, STRUCT_STATS, STRUCT_PARAMS = 0, 1, 2, 3
# gpslam_hip_launch_census: the GPSLAM_CENSUS_* entries of include/gpslam_hip.h, in order
CENSUS_KEYS = (
    "l0_fused", "l0_rows", "l0_column", "l0_column_fast", "top_chunk",
    "sv", "dg", "block", "fp32", "gsave", "gp", "btw_rec", "lines", "odd_rows", "tail",
    "gsave_launches", "tail_launches",
    "upper_cr", "upper_chunk",
    "bwd_rows", "bwd_rows_fold", "bwd_chunk", "upper_bwd",
    "lin_rec", "lin_rec_vp", "lin_rows", "lin_rows_vp", "lin_vw", "lin_vw_vp", "lin_groups", "lin_pend", "flush",
    "gps_lines", "meas_rec", "meas_self",
    "retract",
)
CENSUS_GP_ROWS, CENSUS_GP_D3_RECORDS, CENSUS_GP_SE3_RECORDS = 0, 1, 2


class GpslamHipError(RuntimeError):
    pass


class Config(C.Structure):
    """gpslam_hip_config (v1: the eight knobs as anonymous words); kept for callers of gpslam_hip_create"""
    _fields_ = [("manifold", C.c_int32), ("precision", C.c_int32), ("device", C.c_int32), ("chart", C.c_int32),
                ("landmark_dim", C.c_int32), ("chunk", C.c_int32), ("rank", C.c_int32), ("nranks", C.c_int32),
                ("reserved", C.c_int32 * 8)]


class ConfigV2(C.Structure):
    """gpslam_hip_config_v2: struct_size first, every knob by name (include/gpslam_hip.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("manifold", C.c_int32), ("precision", C.c_int32), ("device", C.c_int32), ("chart", C.c_int32),
                ("landmark_dim", C.c_int32), ("chunk", C.c_int32), ("rank", C.c_int32), ("nranks", C.c_int32),
                ("force_sharded", C.c_int32), ("upper_chunk", C.c_int32), ("top_blocks", C.c_int32), ("velocity", C.c_int32),
                ("segment_length", C.c_int32), ("force_segmented", C.c_int32), ("plan", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("error_before", C.c_double), ("error_after", C.c_double), ("delta_inf_norm", C.c_double),
                ("lambda_", C.c_double), ("iterations", C.c_int32), ("status", C.c_int32),
                ("accepted", C.c_int32), ("trials", C.c_int32), ("last_trial_error", C.c_double)]


ALL_GATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
ALL_REDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)


class Params(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("relative_error_tol", C.c_double),
                ("absolute_error_tol", C.c_double), ("error_tol", C.c_double), ("delta_tol", C.c_double),
                ("lambda_initial", C.c_double), ("lambda_factor", C.c_double), ("lambda_upper_bound", C.c_double),
                ("lambda_lower_bound", C.c_double), ("min_model_fidelity", C.c_double), ("use_lm", C.c_int32),
                ("pad", C.c_int32)]


_lib = None


def load_library():
    """Load libgpslam_hip.so, building it with hipcc if needed.  Raises if that is impossible."""
    global _lib
    if _lib is None:
        path = os.environ.get("GPSLAM_LIB") or _build.build()     # GPSLAM_LIB: an alternative build (A/B timing of kernel variants)
        if not os.path.exists(path):
            raise GpslamHipError("libgpslam_hip.so is missing and could not be built; there is no CPU fallback")
        lib = C.CDLL(path)
        lib.gpslam_hip_last_error.restype = C.c_char_p
        lib.gpslam_hip_stream.restype = C.c_void_p
        check_abi(lib, path)
        _lib = lib
    return _lib


def check_abi(lib, path="libgpslam_hip.so"):
    """The structs below are written into by the library: a library built from another major version of the header, or one whose
    struct sizes differ from this file's, is refused at load time (gpslam_hip_stats grew by 8 bytes in round 5 with
    nothing to tell an old caller)."""
    if not hasattr(lib, "gpslam_hip_abi_version"):
        raise GpslamHipError("%s exports no gpslam_hip_abi_version: built from a header older than ABI 2.0" % path)
    lib.gpslam_hip_abi_version.restype = C.c_uint32
    lib.gpslam_hip_struct_size.restype = C.c_size_t
    v = lib.gpslam_hip_abi_version()
    if (v >> 16) != ABI_MAJOR or (v & 0xffff) < ABI_MINOR:
        raise GpslamHipError("%s speaks ABI %d.%d, this binding %d.%d" % (path, v >> 16, v & 0xffff, ABI_MAJOR, ABI_MINOR))
    for which, ty in ((STRUCT_CONFIG, Config), (STRUCT_CONFIG_V2, ConfigV2), (STRUCT_STATS, Stats), (STRUCT_PARAMS, Params)):
        n = lib.gpslam_hip_struct_size(which)
        if n != C.sizeof(ty):
            raise GpslamHipError("%s: sizeof(%s) is %d in the library, %d in this binding" % (path, ty.__name__, n, C.sizeof(ty)))


def lm_decide(s6, lam, lambda_factor=10.0, lambda_upper_bound=1e5, lambda_lower_bound=0.0, min_model_fidelity=1e-3,
              relative_error_tol=1e-5):
    """gpslam_hip_lm_decide (host arithmetic, no GPU): one tryLambda decision from the reduced scalars of a trial.
    Returns (accepted, done, new lambda)."""
    p = Params()
    load_library().gpslam_hip_default_params(C.byref(p))
    p.use_lm = 1
    p.lambda_factor, p.lambda_upper_bound, p.lambda_lower_bound = lambda_factor, lambda_upper_bound, lambda_lower_bound
    p.min_model_fidelity, p.relative_error_tol = min_model_fidelity, relative_error_tol
    s = (C.c_double * 6)(*[float(v) for v in s6])
    lam_c, acc, done = C.c_double(lam), C.c_int32(0), C.c_int32(0)
    rc = load_library().gpslam_hip_lm_decide(s, C.byref(p), C.byref(lam_c), C.byref(acc), C.byref(done))
    if rc:
        raise GpslamHipError("lm_decide: %d" % rc)
    return bool(acc.value), bool(done.value), lam_c.value


def _dogleg_lib():
    """The library with the argument types of include/gpslam_hip_dogleg.h set (doubles travel by value there)."""
    lib = load_library()
    if not hasattr(lib, "gpslam_hip_iterate_dogleg"):
        raise GpslamHipError("this libgpslam_hip.so has no dogleg entry points (include/gpslam_hip_dogleg.h)")
    if getattr(lib, "_dogleg_bound", False):
        return lib
    dp, ip, vp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_void_p
    lib.gpslam_hip_dogleg_point.argtypes = [dp, C.c_double, dp, dp, dp, ip]
    lib.gpslam_hip_dogleg_decide.argtypes = [dp, C.c_int32, dp, ip, ip, ip]
    lib.gpslam_hip_iterate_dogleg.argtypes = [vp, dp, C.c_int32, C.POINTER(Stats)]
    lib.gpslam_hip_optimize_dogleg.argtypes = [vp, C.POINTER(Params), C.c_double, C.c_int32, C.POINTER(Stats)]
    lib.gpslam_hip_dogleg_last.argtypes = [vp, dp]
    for name in DOGLEG_SYMBOLS:
        getattr(lib, name).restype = C.c_int
    lib._dogleg_bound = True
    return lib


def dogleg_point(s4, delta):
    """gpslam_hip_dogleg_point (host arithmetic, no GPU): the dogleg point of trust radius delta from s4 = (gg, gHg, gn, nn).
    Returns (alpha, beta, |delta_d|, predicted decrease, branch): delta_d = alpha g + beta delta_n."""
    s = (C.c_double * 4)(*[float(v) for v in s4])
    coef, norm, pred, br = (C.c_double * 2)(), C.c_double(0.0), C.c_double(0.0), C.c_int32(0)
    rc = _dogleg_lib().gpslam_hip_dogleg_point(s, float(delta), coef, C.byref(norm), C.byref(pred), C.byref(br))
    if rc:
        raise GpslamHipError("dogleg_point: %d" % rc)
    return coef[0], coef[1], norm.value, pred.value, br.value


def dogleg_decide(s4, mode, delta, last_action=0):
    """gpslam_hip_dogleg_decide (host arithmetic, no GPU): one trust-region decision from s4 = (f, f_new, predicted, |delta_d|).
    Returns (keep, stay, new delta, new last_action)."""
    s = (C.c_double * 4)(*[float(v) for v in s4])
    d, la, keep, stay = C.c_double(delta), C.c_int32(int(last_action)), C.c_int32(0), C.c_int32(0)
    rc = _dogleg_lib().gpslam_hip_dogleg_decide(s, int(mode), C.byref(d), C.byref(la), C.byref(keep), C.byref(stay))
    if rc:
        raise GpslamHipError("dogleg_decide: %d" % rc)
    return bool(keep.value), bool(stay.value), d.value, la.value


def _evidence_lib():
    """The library with the argument types of include/gpslam_hip_evidence.h set (doubles and 64-bit counts travel by value there)."""
    lib = load_library()
    if not hasattr(lib, "gpslam_hip_log_determinant"):
        raise GpslamHipError("this libgpslam_hip.so has no evidence entry points (include/gpslam_hip_evidence.h)")
    if getattr(lib, "_evidence_bound", False):
        return lib
    dp, lp, vp = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_void_p
    lib.gpslam_hip_log_determinant.argtypes = [vp, dp, dp]
    lib.gpslam_hip_log_noise_normaliser.argtypes = [vp, dp, lp, lp]
    lib.gpslam_hip_log_evidence.argtypes = [vp, dp]
    lib.gpslam_hip_gp_log_normaliser.argtypes = [C.c_int32, dp, C.c_double, dp]
    lib.gpslam_hip_evidence_combine.argtypes = [C.c_double, C.c_double, C.c_double, C.c_int64, C.c_int64, dp]
    for name in EVIDENCE_SYMBOLS:
        getattr(lib, name).restype = C.c_int
    lib._evidence_bound = True
    return lib


def gp_log_normaliser(Qc, dt):
    """gpslam_hip_gp_log_normaliser (host arithmetic, no GPU): log|det R| = -1/2 log det Q(dt) of one GP prior with the d x d Qc."""
    q = np.ascontiguousarray(Qc, dtype=np.float64)
    if q.ndim != 2 or q.shape[0] != q.shape[1]:
        raise GpslamHipError("gp_log_normaliser: Qc must be square")
    out = C.c_double(0.0)
    rc = _evidence_lib().gpslam_hip_gp_log_normaliser(int(q.shape[0]), q.ctypes.data_as(C.POINTER(C.c_double)), float(dt), C.byref(out))
    if rc:
        raise GpslamHipError("gp_log_normaliser: %d" % rc)
    return out.value


def evidence_combine(cost, logdet, lognorm, rows, nvars):
    """gpslam_hip_evidence_combine (host arithmetic, no GPU): log Z = -cost + lognorm - logdet / 2 - ((rows - nvars) / 2) log 2 pi."""
    out = C.c_double(0.0)
    rc = _evidence_lib().gpslam_hip_evidence_combine(float(cost), float(logdet), float(lognorm), int(rows), int(nvars), C.byref(out))
    if rc:
        raise GpslamHipError("evidence_combine: %d" % rc)
    return out.value


def _qc_lib():
    """The library with the argument types of include/gpslam_hip_qc.h set (64-bit counts travel by value there)."""
    lib = load_library()
    if not hasattr(lib, "gpslam_hip_qc_statistic"):
        raise GpslamHipError("this libgpslam_hip.so has no Qc-learning entry points (include/gpslam_hip_qc.h)")
    if getattr(lib, "_qc_bound", False):
        return lib
    dp, lp, vp = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_void_p
    lib.gpslam_hip_qc_statistic.argtypes = [vp, dp, lp]
    lib.gpslam_hip_qc_gradient.argtypes = [C.c_int32, dp, dp, C.c_int64, dp]
    lib.gpslam_hip_qc_em_update.argtypes = [C.c_int32, dp, C.c_int64, dp]
    lib.gpslam_hip_qc_em_scale.argtypes = [C.c_int32, dp, dp, C.c_int64, dp]
    for name in QC_SYMBOLS:
        getattr(lib, name).restype = C.c_int
    lib._qc_bound = True
    return lib


def _noise_lib():
    """The library with the argument types of include/gpslam_hip_noise.h set (64-bit counts travel by value there)."""
    lib = load_library()
    if not hasattr(lib, "gpslam_hip_meas_noise_statistic"):
        raise GpslamHipError("this libgpslam_hip.so has no noise-learning entry points (include/gpslam_hip_noise.h)")
    if getattr(lib, "_noise_bound", False):
        return lib
    dp, lp, vp = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_void_p
    lib.gpslam_hip_meas_noise_statistic.argtypes = [vp, C.c_int32, C.POINTER(C.c_uint8), dp, dp, lp]
    lib.gpslam_hip_meas_predicted_covariances.argtypes = [vp, C.c_int32, dp]
    lib.gpslam_hip_noise_gradient.argtypes = [C.c_int32, dp, dp, C.c_int64, dp]
    lib.gpslam_hip_noise_em_update.argtypes = [C.c_int32, dp, C.c_int64, dp]
    lib.gpslam_hip_noise_em_scale.argtypes = [C.c_int32, dp, C.c_int64, dp, dp]
    for name in NOISE_SYMBOLS:
        getattr(lib, name).restype = C.c_int
    lib._noise_bound = True
    return lib


def _sampling_lib():
    """The library with the argument types of include/gpslam_hip_sampling.h set (64-bit seeds and counters travel by value there)."""
    lib = load_library()
    if not hasattr(lib, "gpslam_hip_sample_posterior"):
        raise GpslamHipError("this libgpslam_hip.so has no sampling entry points (include/gpslam_hip_sampling.h)")
    if getattr(lib, "_sampling_bound", False):
        return lib
    dp, ip, vp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_void_p
    lib.gpslam_hip_posterior_noise_dim.argtypes = [vp, ip]
    lib.gpslam_hip_posterior_noise.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_int32, dp]
    lib.gpslam_hip_sample_posterior.argtypes = [vp, C.c_int32, C.c_uint64, C.c_uint64, dp, dp, dp, dp, dp]
    for name in SAMPLING_SYMBOLS:
        getattr(lib, name).restype = C.c_int
    lib._sampling_bound = True
    return lib


def _sampling_at_lib():
    """The library with the argument types of include/gpslam_hip_sampling_at.h set."""
    lib = _sampling_lib()
    if not hasattr(lib, "gpslam_hip_sample_posterior_at"):
        raise GpslamHipError("this libgpslam_hip.so has no dense sampling entry points (include/gpslam_hip_sampling_at.h)")
    if getattr(lib, "_sampling_at_bound", False):
        return lib
    dp, ip, vp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_void_p
    lib.gpslam_hip_posterior_noise_dim_at.argtypes = [vp, C.c_int32, ip]
    lib.gpslam_hip_posterior_noise_at.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_int32, C.c_int32, dp]
    lib.gpslam_hip_sample_posterior_at.argtypes = [vp, C.c_int32, C.c_uint64, C.c_uint64, dp, C.c_int32, ip, dp, dp, dp, dp, dp, dp, dp, dp]
    for name in SAMPLING_AT_SYMBOLS:
        getattr(lib, name).restype = C.c_int
    lib._sampling_at_bound = True
    return lib


def _sampling_stats_lib():
    """The library with the argument types of include/gpslam_hip_sampling_stats.h set."""
    lib = _sampling_at_lib()
    if not hasattr(lib, "gpslam_hip_sample_posterior_stats"):
        raise GpslamHipError("this libgpslam_hip.so has no sampling statistics entry points (include/gpslam_hip_sampling_stats.h)")
    if getattr(lib, "_sampling_stats_bound", False):
        return lib
    dp, ip, lp, vp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.c_void_p
    lib.gpslam_hip_sample_posterior_stats.argtypes = [vp, C.c_int32, C.c_uint64, C.c_uint64, dp, C.c_int32, ip, dp, dp,
                                                      C.c_int32, dp, C.c_double, C.c_int32, lp, dp, dp, lp, dp, dp]
    lib.gpslam_hip_posterior_moments.argtypes = [C.c_int32, C.c_int32, C.c_int64, dp, dp, dp, dp]
    for name in SAMPLING_STATS_SYMBOLS:
        getattr(lib, name).restype = C.c_int
    lib._sampling_stats_bound = True
    return lib


def _square(M, what):
    m = np.ascontiguousarray(M, dtype=np.float64)
    if m.ndim != 2 or m.shape[0] != m.shape[1]:
        raise GpslamHipError("%s: the matrices must be square" % what)
    return m


def qc_gradient(Qc, A, n_f):
    """gpslam_hip_qc_gradient (host arithmetic, no GPU): G = n_f Qc - A / 2, the derivative of the log-evidence in W = Qc^-1 at
    fixed states (dF = tr(G dW)), from the statistic (A, n_f) of ChainSolver.qc_statistic."""
    q, a = _square(Qc, "qc_gradient"), _square(A, "qc_gradient")
    if q.shape != a.shape:
        raise GpslamHipError("qc_gradient: Qc and A differ in size")
    dp = C.POINTER(C.c_double)
    G = np.zeros_like(q)
    rc = _qc_lib().gpslam_hip_qc_gradient(int(q.shape[0]), q.ctypes.data_as(dp), a.ctypes.data_as(dp), int(n_f), G.ctypes.data_as(dp))
    if rc:
        raise GpslamHipError("qc_gradient: %d" % rc)
    return G


def qc_em_update(A, n_f):
    """gpslam_hip_qc_em_update (host arithmetic, no GPU): the EM M-step Qc+ = A / (2 n_f)."""
    a = _square(A, "qc_em_update")
    dp = C.POINTER(C.c_double)
    out = np.zeros_like(a)
    rc = _qc_lib().gpslam_hip_qc_em_update(int(a.shape[0]), a.ctypes.data_as(dp), int(n_f), out.ctypes.data_as(dp))
    if rc:
        raise GpslamHipError("qc_em_update: %d" % rc)
    return out


def qc_em_scale(Qc0, A, n_f):
    """gpslam_hip_qc_em_scale (host arithmetic, no GPU): theta+ = tr(Qc0^-1 A) / (2 n_f d), the stationary scale of Qc = theta Qc0."""
    q, a = _square(Qc0, "qc_em_scale"), _square(A, "qc_em_scale")
    if q.shape != a.shape:
        raise GpslamHipError("qc_em_scale: Qc0 and A differ in size")
    dp = C.POINTER(C.c_double)
    out = C.c_double(0.0)
    rc = _qc_lib().gpslam_hip_qc_em_scale(int(q.shape[0]), q.ctypes.data_as(dp), a.ctypes.data_as(dp), int(n_f), C.byref(out))
    if rc:
        raise GpslamHipError("qc_em_scale: %d" % rc)
    return out.value


def noise_gradient(Cov, B, n):
    """gpslam_hip_noise_gradient (host arithmetic, no GPU): G = (n C - B) / 2, the derivative of the log-evidence in W = C^-1 at
    fixed states (dF = tr(G dW)) when the used factors share the covariance C, from ChainSolver.meas_noise_statistic's (B, n)."""
    c, b = _square(Cov, "noise_gradient"), _square(B, "noise_gradient")
    if c.shape != b.shape:
        raise GpslamHipError("noise_gradient: C and B differ in size")
    dp = C.POINTER(C.c_double)
    G = np.zeros_like(c)
    rc = _noise_lib().gpslam_hip_noise_gradient(int(c.shape[0]), c.ctypes.data_as(dp), b.ctypes.data_as(dp), int(n), G.ctypes.data_as(dp))
    if rc:
        raise GpslamHipError("noise_gradient: %d" % rc)
    return G


def noise_em_update(B, n):
    """gpslam_hip_noise_em_update (host arithmetic, no GPU): the EM M-step C+ = B / n of a covariance the used factors share."""
    b = _square(B, "noise_em_update")
    dp = C.POINTER(C.c_double)
    out = np.zeros_like(b)
    rc = _noise_lib().gpslam_hip_noise_em_update(int(b.shape[0]), b.ctypes.data_as(dp), int(n), out.ctypes.data_as(dp))
    if rc:
        raise GpslamHipError("noise_em_update: %d" % rc)
    return out


def noise_em_scale(Bw, n):
    """gpslam_hip_noise_em_scale (host arithmetic, no GPU): (theta+ / theta, per-row ratios) = (tr(Bw) / (n r), diag(Bw) / n), the
    stationary scales of C_m = theta C_m^0 relative to the ones Bw was whitened with."""
    b = _square(Bw, "noise_em_scale")
    dp = C.POINTER(C.c_double)
    ratio, rows = C.c_double(0.0), np.zeros(b.shape[0])
    rc = _noise_lib().gpslam_hip_noise_em_scale(int(b.shape[0]), b.ctypes.data_as(dp), int(n), C.byref(ratio), rows.ctypes.data_as(dp))
    if rc:
        raise GpslamHipError("noise_em_scale: %d" % rc)
    return ratio.value, rows


def robust_eval(loss, k, r):
    """gpslam_hip_robust_eval (host arithmetic, no GPU): (w(r), rho(r)) of one GPSLAM_ROBUST_* loss with parameter k."""
    w, rho = C.c_double(0.0), C.c_double(0.0)
    rc = load_library().gpslam_hip_robust_eval(C.c_int32(int(loss)), C.c_double(k), C.c_double(r), C.byref(w), C.byref(rho))
    if rc:
        raise GpslamHipError("robust_eval: %d" % rc)
    return w.value, rho.value


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32))


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


class ChainSolver:
    def __init__(self, kind, chart=CHART_EXPMAP, landmark_dim=0, device=0, chunk=0, rank=0, nranks=1,
                 force_sharded=False, upper_chunk=0, top_blocks=0, velocity_world=False, segment_length=0,
                 force_segmented=False, precision=0, plan=0):
        self.lib = load_library()
        self.kind, self.chart, self.ld = kind, chart, landmark_dim
        self.d, self.pd = TANGENT_DIM[kind], POSE_DIM[kind]
        self.b = 2 * self.d
        self.N = self.L = self.n_gp = 0
        self._gp_left = np.zeros(0, dtype=np.int64)     # left states of the GP priors, in the order added (marginalize_head drops those of the head)
        cfg = ConfigV2(struct_size=C.sizeof(ConfigV2), manifold=kind, precision=precision, device=device, chart=chart,
                       landmark_dim=landmark_dim, chunk=chunk, rank=rank, nranks=nranks,
                       force_sharded=1 if force_sharded else 0, upper_chunk=upper_chunk, top_blocks=top_blocks,
                       velocity=1 if velocity_world else 0,        # GPSLAM_VELOCITY_WORLD_VW: the *Pose3VW factor family
                       segment_length=segment_length,              # segmented landmark elimination: states per segment (0 = automatic)
                       force_segmented=1 if force_segmented else 0,   # ... for any landmark count (default: only beyond the dense border)
                       plan=plan | _DEFAULT_PLAN)                  # GPSLAM_PLAN_* bits
        self._h = C.c_void_p()
        rc = self.lib.gpslam_hip_create_v2(C.byref(cfg), C.byref(self._h))
        if rc != 0:
            self._h = None
            raise GpslamHipError("gpslam_hip_create_v2 failed (%d): no usable HIP device, and there is no CPU fallback" % rc)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.gpslam_hip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc < 0:
            msg = self.lib.gpslam_hip_last_error(self._h)
            raise GpslamHipError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else ""))
        return rc

    # ---- variables
    def set_qc(self, Qc):
        Qc = _f64(Qc)
        return self._chk(self.lib.gpslam_hip_set_qc(self._h, _p(Qc)), "set_qc")

    def set_states(self, pose, vel):
        pose, vel = _f64(pose).reshape(-1, self.pd), _f64(vel).reshape(-1, self.d)
        self.N = pose.shape[0]
        return self._chk(self.lib.gpslam_hip_set_states(self._h, self.N, _p(pose), _p(vel)), "set_states")

    def get_states(self):
        pose, vel = np.zeros((self.N, self.pd)), np.zeros((self.N, self.d))
        self._chk(self.lib.gpslam_hip_get_states(self._h, _p(pose), _p(vel)), "get_states")
        return pose, vel

    def set_landmarks(self, pts):
        pts = _f64(pts).reshape(-1, self.ld)
        self.L = pts.shape[0]
        return self._chk(self.lib.gpslam_hip_set_landmarks(self._h, self.L, _p(pts)), "set_landmarks")

    def get_landmarks(self):
        pts = np.zeros((self.L, self.ld))
        self._chk(self.lib.gpslam_hip_get_landmarks(self._h, _p(pts)), "get_landmarks")
        return pts

    # ---- factors
    def add_gp_priors(self, left, dt):
        left, dt = _i32(left), _f64(dt)
        self.n_gp += len(left)
        self._gp_left = np.concatenate([self._gp_left, left.astype(np.int64)])
        return self._chk(self.lib.gpslam_hip_add_gp_priors(self._h, len(left), _p(left), _p(dt)), "add_gp_priors")

    def add_gp_priors_qc(self, left, dt, Qc):
        """GP priors with one Qc_model per factor (count x d x d), as the reference's constructors take it."""
        left, dt, Qc = _i32(left), _f64(dt), _f64(Qc)
        self.n_gp += len(left)
        self._gp_left = np.concatenate([self._gp_left, left.astype(np.int64)])
        return self._chk(self.lib.gpslam_hip_add_gp_priors_qc(self._h, len(left), _p(left), _p(dt), _p(Qc)), "add_gp_priors_qc")

    def set_meas_covariance(self, kind, cov):
        """noiseModel::Gaussian::Covariance (count x rows x rows) on the most recently added factors of one MEAS_* kind."""
        cov = _f64(cov)
        return self._chk(self.lib.gpslam_hip_set_meas_covariance(self._h, int(kind), cov.shape[0], _p(cov)), "set_meas_covariance")

    def _losses(self, loss, k):
        loss = _i32(loss).reshape(-1)
        k = _f64(np.broadcast_to(np.asarray(k, dtype=np.float64), loss.shape))
        return loss, k

    def set_meas_robust(self, kind, loss, k):
        """noiseModel::Robust on the most recently added factors of one MEAS_* kind: loss = ROBUST_* per factor, k = its parameter
        (one per factor, or one for all)."""
        loss, k = self._losses(loss, k)
        return self._chk(self.lib.gpslam_hip_set_meas_robust(self._h, int(kind), len(loss), _p(loss), _p(k)), "set_meas_robust")

    def set_between_pairs_robust(self, loss, k):
        """... on the most recently added loop closures (the non-adjacent pairs of add_between_pairs)."""
        loss, k = self._losses(loss, k)
        return self._chk(self.lib.gpslam_hip_set_between_pairs_robust(self._h, len(loss), _p(loss), _p(k)), "set_between_pairs_robust")

    def meas_weights(self, kind, count):
        """The weights w(r) of the `count` factors of one MEAS_* kind at the current states (1 without a loss)."""
        w = np.zeros(count)
        n = self._chk(self.lib.gpslam_hip_get_meas_weights(self._h, int(kind), _p(w)), "get_meas_weights")
        assert n == count, (n, count)
        return w

    def between_pairs_weights(self, count):
        """The weights w(r) of the `count` loop closures at the current states."""
        w = np.zeros(count)
        n = self._chk(self.lib.gpslam_hip_get_between_pairs_weights(self._h, _p(w)), "get_between_pairs_weights")
        assert n == count, (n, count)
        return w

    def add_pose_priors(self, idx, prior, sigmas):
        idx, prior, sigmas = _i32(idx), _f64(prior), _f64(sigmas)
        return self._chk(self.lib.gpslam_hip_add_pose_priors(self._h, len(idx), _p(idx), _p(prior), _p(sigmas)),
                         "add_pose_priors")

    def add_vel_priors(self, idx, prior, sigmas):
        idx, prior, sigmas = _i32(idx), _f64(prior), _f64(sigmas)
        return self._chk(self.lib.gpslam_hip_add_vel_priors(self._h, len(idx), _p(idx), _p(prior), _p(sigmas)),
                         "add_vel_priors")

    def add_between(self, left, measured, sigmas):
        left, measured, sigmas = _i32(left), _f64(measured), _f64(sigmas)
        return self._chk(self.lib.gpslam_hip_add_between(self._h, len(left), _p(left), _p(measured), _p(sigmas)),
                         "add_between")

    def add_between_pairs(self, first, second, measured, sigmas):
        """gtsam::BetweenFactor<Pose>(x_first, x_second, measured) between any two states: loop closures (consecutive pairs are
        ordinary chain factors)"""
        first, second, measured, sigmas = _i32(first), _i32(second), _f64(measured), _f64(sigmas)
        if len(first) != len(second):
            raise ValueError("add_between_pairs: first and second differ in length")
        return self._chk(self.lib.gpslam_hip_add_between_pairs(self._h, len(first), _p(first), _p(second), _p(measured), _p(sigmas)),
                         "add_between_pairs")

    def set_closure_passes(self, max_passes, closures_per_pass=0):
        """Before compile(): allow more loop closures than one border holds, as up to max_passes column passes of closures_per_pass
        closures each (0: as many as fit).  max_passes <= 1 is the default: one pass, today's capacity."""
        return self._chk(self.lib.gpslam_hip_set_closure_passes(self._h, int(max_passes), int(closures_per_pass)), "set_closure_passes")

    def closure_info(self):
        """After compile(): dict(closures, per_pass, passes, solves) -- the closures, the w of them that share a pass, the column
        passes P, and the solves of the chain one linear system takes (P + 1 beyond one pass)."""
        out = (C.c_int32 * 4)()
        self._chk(self.lib.gpslam_hip_closure_info(self._h, out), "closure_info")
        return dict(zip(("closures", "per_pass", "passes", "solves"), (int(v) for v in out)))

    def add_landmark_priors(self, idx, prior, sigmas):
        idx, prior, sigmas = _i32(idx), _f64(prior), _f64(sigmas)
        return self._chk(self.lib.gpslam_hip_add_landmark_priors(self._h, len(idx), _p(idx), _p(prior), _p(sigmas)),
                         "add_landmark_priors")

    def add_interp_range(self, left, landmark, z, sigma, dt, tau, sensor=None):
        left, landmark = _i32(left), _i32(landmark)
        z, sigma, dt, tau = _f64(z), _f64(sigma), _f64(dt), _f64(tau)
        sensor = None if sensor is None else _f64(sensor)
        return self._chk(self.lib.gpslam_hip_add_interp_range(self._h, len(left), _p(left), _p(landmark), _p(z),
                                                              _p(sigma), _p(dt), _p(tau), _p(sensor)),
                         "add_interp_range")

    def add_range(self, idx, landmark, z, sigma):
        idx, landmark, z, sigma = _i32(idx), _i32(landmark), _f64(z), _f64(sigma)
        return self._chk(self.lib.gpslam_hip_add_range(self._h, len(idx), _p(idx), _p(landmark), _p(z), _p(sigma)),
                         "add_range")

    def add_interp_attitude(self, left, nZ, bRef, sigma, dt, tau):
        left = _i32(left)
        nZ, bRef, sigma, dt, tau = _f64(nZ), _f64(bRef), _f64(sigma), _f64(dt), _f64(tau)
        return self._chk(self.lib.gpslam_hip_add_interp_attitude(self._h, len(left), _p(left), _p(nZ), _p(bRef),
                                                                 _p(sigma), _p(dt), _p(tau)), "add_interp_attitude")

    def add_ahrs(self, left, delta_R, dR_dbias, bias_hat, delta_tij, cov, omega_coriolis=None):
        """gtsam::AHRSFactor(x_left, x_left+1, b_left, pim, omegaCoriolis) -- matlab/GPAHRSexample.m:131-137; the
        arrays are the PreintegratedAhrsMeasurements state per factor (gpslam_amd.ahrs.Preintegrated)."""
        left = _i32(left)
        delta_R, dR_dbias, bias_hat = _f64(delta_R), _f64(dR_dbias), _f64(bias_hat)
        delta_tij, cov = _f64(delta_tij), _f64(cov)
        cor = None if omega_coriolis is None else _f64(omega_coriolis)
        return self._chk(self.lib.gpslam_hip_add_ahrs(self._h, len(left), _p(left), _p(delta_R), _p(dR_dbias), _p(bias_hat),
                                                      _p(delta_tij), _p(cov), None if cor is None else _p(cor)), "add_ahrs")

    def add_interp_gps(self, left, measured, sigmas, dt, tau, sensor=None):
        left = _i32(left)
        measured, sigmas, dt, tau = _f64(measured), _f64(sigmas), _f64(dt), _f64(tau)
        sensor = None if sensor is None else _f64(sensor)
        return self._chk(self.lib.gpslam_hip_add_interp_gps(self._h, len(left), _p(left), _p(measured), _p(sigmas),
                                                            _p(dt), _p(tau), _p(sensor)), "add_interp_gps")

    def add_interp_projection(self, left, landmark, measured, sigmas, dt, tau, K, sensor=None):
        left, landmark = _i32(left), _i32(landmark)
        measured, sigmas, dt, tau, K = _f64(measured), _f64(sigmas), _f64(dt), _f64(tau), _f64(K)
        sensor = None if sensor is None else _f64(sensor)
        if K.size == 9:      # gtsam::Cal3DS2: fx, fy, s, u0, v0, k1, k2, p1, p2
            return self._chk(self.lib.gpslam_hip_add_interp_projection_ds2(
                self._h, len(left), _p(left), _p(landmark), _p(measured), _p(sigmas), _p(dt), _p(tau), _p(K),
                None if sensor is None else _p(sensor)), "add_interp_projection_ds2")
        return self._chk(self.lib.gpslam_hip_add_interp_projection(
            self._h, len(left), _p(left), _p(landmark), _p(measured), _p(sigmas), _p(dt), _p(tau), _p(K),
            None if sensor is None else _p(sensor)), "add_interp_projection")

    def add_odometry2d(self, left, measured, sigmas):
        left, measured, sigmas = _i32(left), _f64(measured), _f64(sigmas)
        return self._chk(self.lib.gpslam_hip_add_odometry2d(self._h, len(left), _p(left), _p(measured), _p(sigmas)),
                         "add_odometry2d")

    def add_bearing_range(self, idx, landmark, bearing, rng, sigmas):
        idx, landmark = _i32(idx), _i32(landmark)
        bearing, rng, sigmas = _f64(bearing), _f64(rng), _f64(sigmas)
        return self._chk(self.lib.gpslam_hip_add_bearing_range(self._h, len(idx), _p(idx), _p(landmark), _p(bearing),
                                                               _p(rng), _p(sigmas)), "add_bearing_range")

    # ---- fixed-lag smoothing (include/gpslam_hip.h "fixed-lag smoothing")
    def add_state_gaussians(self, idx, pose_lin, vel_lin, A, c):
        """gtsam::LinearContainerFactor over (x_i, v_i): r = A [Local(pose_lin, pose_i) ; vel_i - vel_lin] - c per factor, A (count, b, b)."""
        idx = _i32(idx).reshape(-1)
        n = len(idx)
        pose_lin, vel_lin = _f64(pose_lin).reshape(n, self.pd), _f64(vel_lin).reshape(n, self.d)
        A, c = _f64(A).reshape(n, self.b, self.b), _f64(c).reshape(n, self.b)
        return self._chk(self.lib.gpslam_hip_add_state_gaussians(self._h, n, _p(idx), _p(pose_lin), _p(vel_lin), _p(A), _p(c)),
                         "add_state_gaussians")

    def get_state_gaussians(self):
        """(idx, pose_lin, vel_lin, A, c) of the stored state Gaussians, in the order they stand."""
        n = self._chk(self.lib.gpslam_hip_get_state_gaussians(self._h, None, None, None, None, None), "get_state_gaussians")
        idx = np.zeros(n, dtype=np.int32)
        pose_lin, vel_lin = np.zeros((n, self.pd)), np.zeros((n, self.d))
        A, c = np.zeros((n, self.b, self.b)), np.zeros((n, self.b))
        self._chk(self.lib.gpslam_hip_get_state_gaussians(self._h, _p(idx), _p(pose_lin), _p(vel_lin), _p(A), _p(c)), "get_state_gaussians")
        return idx, pose_lin, vel_lin, A, c

    def marginalize_head(self, k):
        """Eliminates states 0 .. k - 1 and their factors into a state Gaussian on the new state 0; the handle then needs compile()."""
        rc = self._chk(self.lib.gpslam_hip_marginalize_head(self._h, int(k)), "marginalize_head")
        self.N -= int(k)
        self._gp_left = self._gp_left[self._gp_left >= int(k)] - int(k)
        self.n_gp = len(self._gp_left)
        return rc

    def get_head_prior(self):
        """(pose_lin, vel_lin, Lambda, gamma) of the last marginalize_head, as the device computed them."""
        pose_lin, vel_lin = np.zeros(self.pd), np.zeros(self.d)
        Lam, gam = np.zeros((self.b, self.b)), np.zeros(self.b)
        self._chk(self.lib.gpslam_hip_get_head_prior(self._h, _p(pose_lin), _p(vel_lin), _p(Lam), _p(gam)), "get_head_prior")
        return pose_lin, vel_lin, Lam, gam

    def add_border_gaussians(self, idx, pose_lin, vel_lin, lm_lin, A, c):
        """gtsam::LinearContainerFactor over (x_i, v_i, every landmark): r = A [Local(pose_lin, pose_i) ; vel_i - vel_lin ; l - lm_lin] - c
        per factor, A (count, n, n), n = b + L * landmark_dim."""
        idx = _i32(idx).reshape(-1)
        m, nl = len(idx), self.L * self.ld
        n = self.b + nl
        pose_lin, vel_lin, lm_lin = _f64(pose_lin).reshape(m, self.pd), _f64(vel_lin).reshape(m, self.d), _f64(lm_lin).reshape(m, nl)
        A, c = _f64(A).reshape(m, n, n), _f64(c).reshape(m, n)
        return self._chk(self.lib.gpslam_hip_add_border_gaussians(self._h, m, _p(idx), _p(pose_lin), _p(vel_lin), _p(lm_lin), _p(A), _p(c)),
                         "add_border_gaussians")

    def get_border_gaussians(self):
        """(idx, pose_lin, vel_lin, lm_lin, A, c) of the stored border Gaussians, in the order they stand."""
        m = self._chk(self.lib.gpslam_hip_get_border_gaussians(self._h, None, None, None, None, None, None), "get_border_gaussians")
        nl = self.L * self.ld
        n = self.b + nl
        idx = np.zeros(m, dtype=np.int32)
        pose_lin, vel_lin, lm_lin = np.zeros((m, self.pd)), np.zeros((m, self.d)), np.zeros((m, nl))
        A, c = np.zeros((m, n, n)), np.zeros((m, n))
        if m:
            self._chk(self.lib.gpslam_hip_get_border_gaussians(self._h, _p(idx), _p(pose_lin), _p(vel_lin), _p(lm_lin), _p(A), _p(c)),
                      "get_border_gaussians")
        return idx, pose_lin, vel_lin, lm_lin, A, c

    def marginalize_head_onto_landmarks(self, enable=True):
        """marginalize_head accepts head factors that name landmarks and leaves a border Gaussian on (state 0, landmarks)."""
        return self._chk(self.lib.gpslam_hip_marginalize_head_onto_landmarks(self._h, 1 if enable else 0), "marginalize_head_onto_landmarks")

    def get_head_prior_border(self):
        """(lm_lin, Lambda, gamma) over (state, landmarks) of the last marginalize_head onto the landmarks, as the device computed them."""
        nl = self.L * self.ld
        n = self.b + nl
        lm_lin, Lam, gam = np.zeros((self.L, self.ld)), np.zeros((n, n)), np.zeros(n)
        self._chk(self.lib.gpslam_hip_get_head_prior_border(self._h, _p(lm_lin), _p(Lam), _p(gam)), "get_head_prior_border")
        return lm_lin, Lam, gam

    def append_states(self, pose, vel):
        """n more states behind the last one; the factors stay, the handle needs compile()."""
        pose, vel = _f64(pose).reshape(-1, self.pd), _f64(vel).reshape(-1, self.d)
        rc = self._chk(self.lib.gpslam_hip_append_states(self._h, pose.shape[0], _p(pose), _p(vel)), "append_states")
        self.N += pose.shape[0]
        return rc

    def clear_factors(self):
        self.n_gp = 0
        self._gp_left = np.zeros(0, dtype=np.int64)
        return self._chk(self.lib.gpslam_hip_clear_factors(self._h), "clear_factors")

    def compile(self):
        return self._chk(self.lib.gpslam_hip_compile(self._h), "compile")

    # ---- hot path
    def linearize_gp(self, jac=True):
        e = np.zeros((self.n_gp, self.b))
        H = np.zeros((self.n_gp, 4, self.b, self.d)) if jac else None
        self._chk(self.lib.gpslam_hip_linearize_gp(self._h, _p(e), _p(H)), "linearize_gp")
        return e, H

    MEAS_ROWS = {0: 1, 1: 1, 2: 2, 3: 3, 4: 3, 5: 2, 6: 2, 7: 3}

    def linearize_meas(self, kind, count):
        """Unwhitened (e, J) of the `count` measurement factors of one kind (MEAS_* order of include/gpslam_hip.h):
        e (count, rows), J (count, rows, 4d + 3) = [H1 | H2 | H3 | H4 | H5 padded to 3]."""
        rows = self.MEAS_ROWS[kind]
        e = np.zeros((count, rows))
        J = np.zeros((count, rows, 2 * self.b + 3))
        n = self._chk(self.lib.gpslam_hip_linearize_meas(self._h, int(kind), _p(e), _p(J)), "linearize_meas")
        assert n == count, (n, count)
        return e, J

    def error(self):
        out = C.c_double(0.0)
        self._chk(self.lib.gpslam_hip_error(self._h, C.byref(out)), "error")
        return out.value

    def iterate_gn(self):
        st = Stats()
        rc = self.lib.gpslam_hip_iterate_gn(self._h, C.byref(st))
        self._chk(rc, "iterate_gn")
        return rc, st

    def iterate_lm(self, lam, params=None):
        st = Stats()
        p = params or self.default_params(use_lm=1)
        lam_c = C.c_double(lam)
        rc = self.lib.gpslam_hip_iterate_lm(self._h, C.byref(lam_c), C.byref(p), C.byref(st))
        self._chk(rc, "iterate_lm")
        return rc, st, lam_c.value

    def optimize(self, params=None):
        st = Stats()
        p = params or self.default_params()
        rc = self.lib.gpslam_hip_optimize(self._h, C.byref(p), C.byref(st))
        self._chk(rc, "optimize")
        return rc, st

    def iterate_dogleg(self, delta, mode=DOGLEG_ONE_STEP_PER_ITERATION):
        """One DoglegOptimizer::iterate() (include/gpslam_hip_dogleg.h): returns (stats, the trust radius after)."""
        st, d = Stats(), C.c_double(delta)
        self._chk(_dogleg_lib().gpslam_hip_iterate_dogleg(self._h, C.byref(d), int(mode), C.byref(st)), "iterate_dogleg")
        return st, d.value

    def optimize_dogleg(self, params=None, delta_initial=1.0, mode=DOGLEG_ONE_STEP_PER_ITERATION):
        st = Stats()
        p = params or self.default_params()
        rc = _dogleg_lib().gpslam_hip_optimize_dogleg(self._h, C.byref(p), float(delta_initial), int(mode), C.byref(st))
        self._chk(rc, "optimize_dogleg")
        return rc, st

    def dogleg_last(self):
        """(gg, gHg, gn, nn, alpha, beta, predicted, branch) of the last trial of the last iterate_dogleg"""
        out = (C.c_double * 8)()
        self._chk(_dogleg_lib().gpslam_hip_dogleg_last(self._h, out), "dogleg_last")
        return tuple(out)

    def log_determinant(self, parts=False):
        """log det H at the current states (include/gpslam_hip_evidence.h); parts=True: (logdet, (log det A, log det(I + U Z),
        log det S)).  The marginals are stale afterwards."""
        out, p3 = C.c_double(0.0), (C.c_double * 3)()
        self._chk(_evidence_lib().gpslam_hip_log_determinant(self._h, C.byref(out), p3), "log_determinant")
        return (out.value, tuple(p3)) if parts else out.value

    def log_noise_normaliser(self):
        """(sum_f log|det R_f|, residual rows m, variables n) of the stored graph: host arithmetic, nothing is launched"""
        out, m, n = C.c_double(0.0), C.c_int64(0), C.c_int64(0)
        self._chk(_evidence_lib().gpslam_hip_log_noise_normaliser(self._h, C.byref(out), C.byref(m), C.byref(n)), "log_noise_normaliser")
        return out.value, m.value, n.value

    def log_evidence(self):
        """(log Z, cost, log det H, lognorm, m - n) at the current states: the Laplace log-evidence (optimise first)"""
        out = (C.c_double * 5)()
        self._chk(_evidence_lib().gpslam_hip_log_evidence(self._h, out), "log_evidence")
        return tuple(out)

    def qc_statistic(self):
        """(A, n_f) over the GP priors that carry the handle's shared Qc, from the current marginals (include/gpslam_hip_qc.h):
        A = sum_i sum_k (e~_k e~_k^T + J~_k Sigma_J J~_k^T), d x d.  Call marginals() first; they stay valid."""
        A, n = np.zeros((self.d, self.d)), C.c_int64(0)
        self._chk(_qc_lib().gpslam_hip_qc_statistic(self._h, A.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n)), "qc_statistic")
        return A, n.value

    def meas_noise_statistic(self, kind, use=None):
        """(B, Bw, n) over the factors of one MEAS_* kind whose entry of `use` is true (None: all; one entry per factor in the order
        added), from the current marginals (include/gpslam_hip_noise.h): B = sum_m (e e^T + J Sigma_m J^T), Bw the same between the
        factors' base whitening R_m and R_m^T, r x r.  Call marginals() first; they stay valid."""
        r = self.MEAS_ROWS[int(kind)]
        B, Bw, n = np.zeros((r, r)), np.zeros((r, r)), C.c_int64(0)
        dp = C.POINTER(C.c_double)
        m = None if use is None else np.ascontiguousarray(np.asarray(use).reshape(-1) != 0, dtype=np.uint8)
        if m is not None:
            count = self.meas_count(kind)
            if count != len(m):
                raise GpslamHipError("meas_noise_statistic: `use` has %d entries, the kind has %d factors" % (len(m), count))
        self._chk(_noise_lib().gpslam_hip_meas_noise_statistic(self._h, int(kind), None if m is None else m.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                               B.ctypes.data_as(dp), Bw.ctypes.data_as(dp), C.byref(n)), "meas_noise_statistic")
        return B, Bw, n.value

    def meas_count(self, kind):
        """the number of factors of one MEAS_* kind the handle stores (gpslam_hip_meas_predicted_covariances without an output)"""
        return self._chk(_noise_lib().gpslam_hip_meas_predicted_covariances(self._h, int(kind), None), "meas_count")

    def meas_predicted_covariances(self, kind):
        """(count, r, r): P_m = J_m Sigma_m J_m^T of every factor of one MEAS_* kind in the order added, from the current marginals
        (include/gpslam_hip_noise.h); robust graphs are accepted.  Call marginals() first; they stay valid."""
        r = self.MEAS_ROWS[int(kind)]
        lib = _noise_lib()
        count = self.meas_count(kind)
        P = np.zeros((count, r, r))
        if count:
            self._chk(lib.gpslam_hip_meas_predicted_covariances(self._h, int(kind), P.ctypes.data_as(C.POINTER(C.c_double))), "meas_predicted_covariances")
        return P

    def posterior_noise_dim(self):
        """length of one noise vector of sample_posterior: the rows of get_rows(), then the landmark priors' coordinates"""
        n = C.c_int32(0)
        self._chk(_sampling_lib().gpslam_hip_posterior_noise_dim(self._h, C.byref(n)), "posterior_noise_dim")
        return n.value

    def posterior_noise(self, seed, first, count):
        """(count, n_noise): the generator's standard normals for samples first .. first + count - 1 (include/gpslam_hip_sampling.h:
        Philox4x32-10, one normal per (seed, sample, noise index)); nothing is solved"""
        out = np.zeros((max(int(count), 0), self.posterior_noise_dim()))
        rc = _sampling_lib().gpslam_hip_posterior_noise(self._h, int(seed), int(first), int(count), out.ctypes.data_as(C.POINTER(C.c_double)))
        self._chk(rc, "posterior_noise")
        return out

    def sample_posterior(self, count, seed=0, first=0, noise=None, want=("delta", "poses", "vels", "landmarks")):
        """count draws from N(x^, H^-1) at the current states: (delta, poses, vels, landmarks), each with a leading axis of count --
        delta the tangent draws (states, then landmarks), the rest x^ (+) delta in the layouts of get_states() and get_landmarks()
        (landmarks None on a handle without any).  noise: (count, n_noise) whitened residuals to solve for instead of the generator's
        -- the graph's own give the Gauss-Newton step.  want: the outputs asked for; the others return None and are neither written
        nor copied to the host (on long chains the copies cost more than the solve).  The estimate stays; the marginals are stale
        afterwards."""
        count = int(count)
        if not set(want) <= {"delta", "poses", "vels", "landmarks"}:
            raise GpslamHipError("sample_posterior: want names delta, poses, vels, landmarks")
        dp = C.POINTER(C.c_double)
        if noise is not None:
            noise = _f64(noise)
            if noise.shape != (count, self.posterior_noise_dim()):
                raise GpslamHipError("sample_posterior: noise must be count x posterior_noise_dim()")
        nl = self.L * self.ld
        n = max(count, 0)
        delta = np.zeros((n, self.N * self.b + nl)) if "delta" in want else None
        poses = np.zeros((n, self.N, self.pd)) if "poses" in want else None
        vels = np.zeros((n, self.N, self.d)) if "vels" in want else None
        lms = np.zeros((n, self.L, self.ld)) if (nl and "landmarks" in want) else None
        out = (delta, poses, vels, lms)
        rc = _sampling_lib().gpslam_hip_sample_posterior(self._h, count, int(seed), int(first), None if noise is None else noise.ctypes.data_as(dp),
                                                         *[None if a is None else a.ctypes.data_as(dp) for a in out])
        self._chk(rc, "sample_posterior")
        return out

    def posterior_noise_dim_at(self, n_queries):
        """length of one noise vector of sample_posterior_at: posterior_noise_dim() + 2 d n_queries (per query eps_p, then eps_v)"""
        n = C.c_int32(0)
        self._chk(_sampling_at_lib().gpslam_hip_posterior_noise_dim_at(self._h, int(n_queries), C.byref(n)), "posterior_noise_dim_at")
        return n.value

    def posterior_noise_at(self, seed, first, count, n_queries):
        """(count, n_noise_at): the generator's standard normals of a dense draw; the first posterior_noise_dim() columns are
        posterior_noise()'s"""
        out = np.zeros((max(int(count), 0), self.posterior_noise_dim_at(n_queries)))
        rc = _sampling_at_lib().gpslam_hip_posterior_noise_at(self._h, int(seed), int(first), int(count), int(n_queries), out.ctypes.data_as(C.POINTER(C.c_double)))
        self._chk(rc, "posterior_noise_at")
        return out

    def sample_posterior_at(self, left, dt, tau, count, seed=0, first=0, noise=None, want=("query_poses",)):
        """count draws of the support states AND of the trajectory at the query times (left, dt, tau as interpolate_poses takes them;
        include/gpslam_hip_sampling_at.h): each draw's queries are conditioned on that draw's own support states, with the GP's
        conditional noise, and the queries of one interval are correlated as the prior says.  Returns (query_poses (count, n, pose_dim),
        query_vels (count, n, d; LINEAR2 / LINEAR3 only), delta, poses, vels, landmarks) -- the last four as sample_posterior returns
        them, for the same draws; whatever `want` does not name is None and is not copied to the host.  left is non-decreasing; within
        an interval dt is one number and 0 < tau < dt increases strictly.  noise: (count, posterior_noise_dim_at(n))."""
        count = int(count)
        names = ("query_poses", "query_vels", "delta", "poses", "vels", "landmarks")
        if not set(want) <= set(names):
            raise GpslamHipError("sample_posterior_at: want names " + ", ".join(names))
        left, dt, tau = _i32(left), _f64(dt), _f64(tau)
        nq = len(left)
        if len(dt) != nq or len(tau) != nq:
            raise GpslamHipError("sample_posterior_at: left, dt and tau differ in length")
        dp = C.POINTER(C.c_double)
        if noise is not None:
            noise = _f64(noise)
            if noise.shape != (count, self.posterior_noise_dim_at(nq)):
                raise GpslamHipError("sample_posterior_at: noise must be count x posterior_noise_dim_at(n_queries)")
        nl = self.L * self.ld
        n = max(count, 0)
        shapes = dict(query_poses=(n, nq, self.pd), query_vels=(n, nq, self.d), delta=(n, self.N * self.b + nl), poses=(n, self.N, self.pd),
                      vels=(n, self.N, self.d), landmarks=(n, self.L, self.ld))
        out = tuple(np.zeros(shapes[k]) if (k in want and (k != "landmarks" or nl)) else None for k in names)
        rc = _sampling_at_lib().gpslam_hip_sample_posterior_at(self._h, count, int(seed), int(first), None if noise is None else noise.ctypes.data_as(dp),
                                                              nq, left.ctypes.data_as(C.POINTER(C.c_int32)), dt.ctypes.data_as(dp), tau.ctypes.data_as(dp), *[None if a is None else a.ctypes.data_as(dp) for a in out])
        self._chk(rc, "sample_posterior_at")
        return out

    def sample_posterior_stats(self, left, dt, tau, count, seed=0, first=0, noise=None, obstacles=None, margin=0.0, want=None, resume=None):
        """count draws at the query times as sample_posterior_at makes them, reduced on the device (include/gpslam_hip_sampling_stats.h):
        no query pose comes to the host.  Returns a dict:
          n                 the number of draws in the per-query sums
          s1, s2            (n_queries, d), (n_queries, d (d + 1) / 2): sums of the local coordinates eta of the draws' query poses
                            around interpolate_poses() of the estimate, under the handle's chart, and of the lower triangle of eta eta^T
          mean, cov         posterior_moments(n, s1, s2) (cov None with fewer than two draws)
          hits              (n_queries,) int64: draws with a clearance below zero at that query
          clearance, length (count,): min over the queries of (distance to the nearest obstacle's surface - margin), and the length of
                            the polyline through the query positions -- of THIS call's draws
        obstacles: (n, w + 1) rows of centre and radius, w = 3 on POSE3 and 2 elsewhere.  want: a subset of ("moments", "hits",
        "clearance", "length"); by default the moments, hits and clearance when obstacles are given, and the length where poses have a
        position (not ROT3).  What is not asked for is None.  resume: an earlier result over the same queries to continue -- its n,
        s1, s2 and hits are the starting values, and the result equals one call over all the draws to the bit."""
        count = int(count)
        names = ("moments", "hits", "clearance", "length")
        if obstacles is not None:
            obstacles = _f64(obstacles)
            if obstacles.ndim != 2 or obstacles.shape[1] != (4 if self.kind == POSE3 else 3):
                raise GpslamHipError("sample_posterior_stats: obstacles must be n x (w + 1): a centre, then a radius")
        n_obs = 0 if obstacles is None else len(obstacles)
        if want is None:
            want = ("moments",) + (("hits", "clearance") if n_obs else ()) + (("length",) if self.kind != ROT3 else ())
        if not set(want) <= set(names):
            raise GpslamHipError("sample_posterior_stats: want names " + ", ".join(names))
        left, dt, tau = _i32(left), _f64(dt), _f64(tau)
        nq = len(left)
        if len(dt) != nq or len(tau) != nq:
            raise GpslamHipError("sample_posterior_stats: left, dt and tau differ in length")
        dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_int64)
        if noise is not None:
            noise = _f64(noise)
            if noise.shape != (count, self.posterior_noise_dim_at(nq)):
                raise GpslamHipError("sample_posterior_stats: noise must be count x posterior_noise_dim_at(n_queries)")
        d, n = self.d, max(count, 0)
        tri = d * (d + 1) // 2
        mom, hit = "moments" in want, "hits" in want
        n_draws = C.c_int64(0)
        s1 = s2 = hits = None
        if resume is not None:
            if (mom and resume["s1"] is None) or (hit and resume["hits"] is None):
                raise GpslamHipError("sample_posterior_stats: resume lacks the sums this call asks for")
            n_draws = C.c_int64(int(resume["n"]))
            if mom:
                s1, s2 = _f64(resume["s1"]).copy(), _f64(resume["s2"]).copy()
                if s1.shape != (nq, d) or s2.shape != (nq, tri):
                    raise GpslamHipError("sample_posterior_stats: resume holds sums of other queries")
            if hit:
                hits = np.ascontiguousarray(np.asarray(resume["hits"], dtype=np.int64)).copy()
                if hits.shape != (nq,):
                    raise GpslamHipError("sample_posterior_stats: resume holds counts of other queries")
        else:
            if mom:
                s1, s2 = np.zeros((nq, d)), np.zeros((nq, tri))
            if hit:
                hits = np.zeros(nq, dtype=np.int64)
        clearance = np.zeros(n) if "clearance" in want else None
        length = np.zeros(n) if "length" in want else None
        opt = lambda a, t: None if a is None else a.ctypes.data_as(t)
        rc = _sampling_stats_lib().gpslam_hip_sample_posterior_stats(
            self._h, count, int(seed), int(first), opt(noise, dp), nq, left.ctypes.data_as(C.POINTER(C.c_int32)), dt.ctypes.data_as(dp), tau.ctypes.data_as(dp),
            n_obs, opt(obstacles, dp) if n_obs else None, float(margin), 0 if resume is None else 1, C.byref(n_draws),
            opt(s1, dp), opt(s2, dp), opt(hits, lp), opt(clearance, dp), opt(length, dp))
        self._chk(rc, "sample_posterior_stats")
        mean = cov = None
        if mom:
            mean, cov = self.posterior_moments(n_draws.value, s1, s2, cov=n_draws.value >= 2)
        return dict(n=n_draws.value, s1=s1, s2=s2, mean=mean, cov=cov, hits=hits, clearance=clearance, length=length)

    @staticmethod
    def posterior_moments(n, s1, s2, cov=True):
        """(mean (n_queries, d), cov (n_queries, d, d) or None) of n draws from the sums sample_posterior_stats returns: mean = s1 / n,
        cov = (S2 - n mean mean^T) / (n - 1).  Host arithmetic."""
        s1, s2 = _f64(s1), _f64(s2)
        nq, d = s1.shape
        if s2.shape != (nq, d * (d + 1) // 2):
            raise GpslamHipError("posterior_moments: s2 must be n_queries x d (d + 1) / 2")
        dp = C.POINTER(C.c_double)
        mean = np.zeros((nq, d))
        P = np.zeros((nq, d, d)) if cov else None
        rc = _sampling_stats_lib().gpslam_hip_posterior_moments(d, nq, int(n), s1.ctypes.data_as(dp), s2.ctypes.data_as(dp), mean.ctypes.data_as(dp),
                                                                 None if P is None else P.ctypes.data_as(dp))
        if rc < 0:
            raise GpslamHipError("posterior_moments failed (%d): n must be at least 1, and 2 for the covariance" % rc)
        return mean, P

    def run_gn(self, iters, timed=False):
        st = Stats()
        t = np.zeros(5) if timed else None
        self._chk(self.lib.gpslam_hip_run_gn(self._h, int(iters), C.byref(st), _p(t)), "run_gn")
        return st, t

    def default_params(self, **kw):
        p = Params()
        self.lib.gpslam_hip_default_params(C.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    # ---- inspection
    def normal_equations(self):
        N, b, nl = self.N, self.b, self.L * self.ld
        D, O, g = np.zeros((N, b, b)), np.zeros((N, b, b)), np.zeros((N, b))
        B = np.zeros((N, b, nl)) if nl else None
        self._chk(self.lib.gpslam_hip_normal_equations(self._h, _p(D), _p(O), _p(g), _p(B)), "normal_equations")
        return D, O, g, B

    def get_rows(self):
        """(rowLR, rowE, rowM, rowLm) of the current linearisation (whitened)."""
        n = C.c_int32(0)
        self._chk(self.lib.gpslam_hip_get_rows(self._h, C.byref(n), None, None, None, None), "get_rows")
        M = n.value
        LR, E = np.zeros((M, 2 * self.b)), np.zeros(M)
        Mm = np.zeros((M, self.ld)) if self.ld else None
        Lm = np.full(M, -1, dtype=np.int32) if self.ld else None
        self._chk(self.lib.gpslam_hip_get_rows(self._h, C.byref(n), _p(LR), _p(E), _p(Mm), _p(Lm)), "get_rows")
        return LR, E, Mm, Lm

    def block_tridiag_solve(self, D, O, g):
        D, O, g = _f64(D), _f64(O), _f64(g)
        x = np.zeros_like(g)
        self._chk(self.lib.gpslam_hip_block_tridiag_solve(self._h, g.shape[0], _p(D), _p(O), _p(g), _p(x)),
                  "block_tridiag_solve")
        return x

    def interpolate_poses(self, left, dt, tau):
        """Batched interpolatePose of the current estimate: (count, pose_dim)."""
        left, dt, tau = _i32(left), _f64(dt), _f64(tau)
        out = np.zeros((len(left), self.pd))
        self._chk(self.lib.gpslam_hip_interpolate_poses(self._h, len(left), _p(left), _p(dt), _p(tau), _p(out)),
                  "interpolate_poses")
        return out

    def interpolate_velocities(self, left, dt, tau, jac=False):
        """Batched GaussianProcessInterpolatorLinear::interpolateVelocity of the current estimate: (count, d) [, H (count, 4, d, d)]."""
        left, dt, tau = _i32(left), _f64(dt), _f64(tau)
        out = np.zeros((len(left), self.d))
        H = np.zeros((len(left), 4, self.d, self.d)) if jac else None
        self._chk(self.lib.gpslam_hip_interpolate_velocities(self._h, len(left), _p(left), _p(dt), _p(tau), _p(out), _p(H)),
                  "interpolate_velocities")
        return (out, H) if jac else out

    def body_centric_velocity(self, pose1, pose2, dt, spatial=False):
        """getBodyCentricVb (spatial=False) / getBodyCentricVs of pose pairs (count x 12 each): (count, 6)."""
        pose1, pose2 = _f64(pose1).reshape(-1, 12), _f64(pose2).reshape(-1, 12)
        dt = _f64(np.broadcast_to(np.asarray(dt, dtype=np.float64), (len(pose1),)))
        out = np.zeros((len(pose1), 6))
        self._chk(self.lib.gpslam_hip_body_centric_velocity(self._h, 1 if spatial else 0, len(pose1), _p(pose1), _p(pose2), _p(dt), _p(out)),
                  "body_centric_velocity")
        return out

    def plan_info(self):
        """What compile() chose: dict(levels, chunk0, chunk_upper, fused, structured_gp, rows_full, rows_compact, R)."""
        out = (C.c_int32 * 8)()
        self._chk(self.lib.gpslam_hip_plan_info(self._h, out), "plan_info")
        return dict(zip(("levels", "chunk0", "chunk_upper", "fused", "structured_gp", "rows_full", "rows_compact", "R"), list(out)))

    def launch_census(self, reset=True):
        """What this handle's launchers did since the last reset: dict of CENSUS_KEYS (GPSLAM_CENSUS_* of include/gpslam_hip.h).
        Launch counts, and for the last k_fused_level0 launch its instantiation (sv, dg, block, fp32) and inputs (gsave, gp, btw_rec,
        lines, odd_rows, tail), -1 where there was none.  Written by the launch statements themselves, not derived from plan_info()."""
        out = (C.c_int32 * len(CENSUS_KEYS))()
        n = self._chk(self.lib.gpslam_hip_launch_census(self._h, out, len(CENSUS_KEYS), 1 if reset else 0), "launch_census")
        if n != len(CENSUS_KEYS):
            raise GpslamHipError("launch_census: the library reports %d entries, this binding names %d" % (n, len(CENSUS_KEYS)))
        return dict(zip(CENSUS_KEYS, (int(v) for v in out)))

    def segment_plan(self):
        """dict of the segmented landmark elimination's plan (active, C, K, NB, NC, NCP, levels, links)."""
        out = np.zeros(8, dtype=np.int32)
        self._chk(self.lib.gpslam_hip_segment_plan(self._h, _p(out)), "segment_plan")
        return dict(zip(("active", "C", "K", "NB", "NC", "NCP", "levels", "links"), (int(v) for v in out)))

    def interpolate_poses_jac(self, left, dt, tau):
        """interpolatePose with H1..H4: (poses (count, pose_dim), H (count, 4, d, d))."""
        left, dt, tau = _i32(left), _f64(dt), _f64(tau)
        out = np.zeros((len(left), self.pd))
        H = np.zeros((len(left), 4, self.d, self.d))
        self._chk(self.lib.gpslam_hip_interpolate_poses_jac(self._h, len(left), _p(left), _p(dt), _p(tau), _p(out), _p(H)),
                  "interpolate_poses_jac")
        return out, H

    # ---- posterior covariances (gtsam::Marginals)
    def marginals(self):
        """gtsam::Marginals(graph, values) at the current states: computes Sigma = H^-1's blocks on the device (see get_marginals)."""
        return self._chk(self.lib.gpslam_hip_marginals(self._h), "marginals")

    def marginals_keep_closure_columns(self, enable=True):
        """Let marginals() run on a handle whose closures go in column passes (closure_info()["passes"] > 1): it then keeps the
        closures' columns at every state, one more device buffer of about N * closures * d * b doubles.  Any time after create;
        changes nothing on a handle within one pass.  enable=False restores the refusal and frees the buffer."""
        return self._chk(self.lib.gpslam_hip_marginals_keep_closure_columns(self._h, 1 if enable else 0), "marginals_keep_closure_columns")

    def marginals_on_segments(self, enable=True):
        """Let marginals() run on the segmented landmark path (segment_plan()["active"]): it then keeps G = A_s^-1 H[I_s, B_s] at every
        interior state, one more device buffer of about N * b * NCP doubles, and the fat blocks' covariances.  Fat blocks up to 64
        columns.  Any time after create; changes nothing on a handle that is not segmented.  enable=False restores the refusal and
        frees the buffers.  Landmark blocks then come from get_landmark_marginals / get_state_landmark_marginals /
        get_landmark_pair_marginals (get_marginals(cross=True) is refused there: S_lm and S_x_lm are too large to exist)."""
        return self._chk(self.lib.gpslam_hip_marginals_on_segments(self._h, 1 if enable else 0), "marginals_on_segments")

    def get_landmark_marginals(self, first=0, count=None):
        """Sigma_{l,l} (count, ld, ld) of the landmarks [first, first + count) after marginals(); any handle with landmarks."""
        count = self.L - first if count is None else count
        out = np.zeros((count, self.ld, self.ld))
        self._chk(self.lib.gpslam_hip_get_landmark_marginals(self._h, int(first), int(count), _p(out)), "get_landmark_marginals")
        return out

    def get_state_landmark_marginals(self, states, landmarks):
        """Sigma_{state, landmark} (count, b, ld) for pairs of a state and a landmark.  Segmented handles: the landmark must sit in a
        fat block next to the state's segment (every landmark the state observes does)."""
        states, landmarks = _i32(states), _i32(landmarks)
        if len(states) != len(landmarks):
            raise ValueError("get_state_landmark_marginals: states and landmarks differ in length")
        out = np.zeros((len(states), self.b, self.ld))
        self._chk(self.lib.gpslam_hip_get_state_landmark_marginals(self._h, len(states), _p(states), _p(landmarks), _p(out)),
                  "get_state_landmark_marginals")
        return out

    def get_landmark_pair_marginals(self, a, b):
        """Sigma_{a, b} (count, ld, ld) for pairs of landmarks.  Segmented handles: both in the same or in neighbouring fat blocks."""
        a, b = _i32(a), _i32(b)
        if len(a) != len(b):
            raise ValueError("get_landmark_pair_marginals: a and b differ in length")
        out = np.zeros((len(a), self.ld, self.ld))
        self._chk(self.lib.gpslam_hip_get_landmark_pair_marginals(self._h, len(a), _p(a), _p(b), _p(out)), "get_landmark_pair_marginals")
        return out

    def marginals_keep_pair_terms(self, enable=True):
        """Let get_state_pair_marginals / gate_between_pairs run on a handle with landmarks or closures: marginals() then copies
        their columns at every state, one more device buffer of N * b * (nl + closures * d) doubles (column passes: N * b * nl).
        Any time after create, before marginals(); a handle without landmarks and closures needs no call.  enable=False frees it."""
        return self._chk(self.lib.gpslam_hip_marginals_keep_pair_terms(self._h, 1 if enable else 0), "marginals_keep_pair_terms")

    def get_state_pair_marginals(self, a, b):
        """Sigma_{a, b} (count, b, b; rows: state a) for pairs of ANY two states after marginals().  a == b and adjacent pairs are
        get_marginals' blocks to the bit; Sigma_{b,a} is the transpose of Sigma_{a,b} to the bit."""
        a, b = _i32(a), _i32(b)
        if len(a) != len(b):
            raise ValueError("get_state_pair_marginals: a and b differ in length")
        out = np.zeros((len(a), self.b, self.b))
        self._chk(self.lib.gpslam_hip_get_state_pair_marginals(self._h, len(a), _p(a), _p(b), _p(out)), "get_state_pair_marginals")
        return out

    def gate_between_pairs(self, first, second, measured, sigmas):
        """The chi-square gate of loop-closure candidates that are not in the graph (arguments as add_between_pairs), at the current
        states and the held marginals.  Returns (chi2 (count,), err (count, d), innov_cov (count, d, d)): the unwhitened
        BetweenFactor error e, P = diag(sigma^2) + [H1 H2] Sigma [H1 H2]^T over the two states' pose blocks, and e^T P^-1 e."""
        first, second, measured, sigmas = _i32(first), _i32(second), _f64(measured), _f64(sigmas)
        if len(first) != len(second):
            raise ValueError("gate_between_pairs: first and second differ in length")
        n = len(first)
        if measured.size != n * self.pd or sigmas.size != n * self.d:
            raise ValueError("gate_between_pairs: measured must be count x %d and sigmas count x %d" % (self.pd, self.d))
        chi2, err, cov = np.zeros(n), np.zeros((n, self.d)), np.zeros((n, self.d, self.d))
        self._chk(self.lib.gpslam_hip_gate_between_pairs(self._h, n, _p(first), _p(second), _p(measured), _p(sigmas), _p(chi2), _p(err), _p(cov)),
                  "gate_between_pairs")
        return chi2, err, cov

    def get_marginals(self, first=0, count=None, cross=False):
        """Blocks of the last marginals() call for states [first, first + count): S (count, b, b) = Sigma_{i,i} and S_next
        (count, b, b) = Sigma_{i,i+1}; with landmarks also S_lm (nl, nl) and S_x_lm (count, b, nl).  Returns (S, S_next) or, with
        cross=True, (S, S_next, S_lm, S_x_lm) (None without landmarks)."""
        count = self.N - first if count is None else count
        b, nl = self.b, self.L * self.ld
        S, Sn = np.zeros((count, b, b)), np.zeros((count, b, b))
        Slm = np.zeros((nl, nl)) if (cross and nl) else None
        Sxl = np.zeros((count, b, nl)) if (cross and nl) else None
        self._chk(self.lib.gpslam_hip_get_marginals(self._h, int(first), int(count), _p(S), _p(Sn), _p(Slm), _p(Sxl)), "get_marginals")
        return (S, Sn, Slm, Sxl) if cross else (S, Sn)

    def interpolate_covariances(self, left, dt, tau, gp_term=True):
        """Posterior covariance (count, d, d) of the GP-interpolated pose at tau in (left, left + 1), after marginals()."""
        left, dt, tau = _i32(left), _f64(dt), _f64(tau)
        out = np.zeros((len(left), self.d, self.d))
        self._chk(self.lib.gpslam_hip_interpolate_covariances(self._h, len(left), _p(left), _p(dt), _p(tau), 1 if gp_term else 0, _p(out)),
                  "interpolate_covariances")
        return out

    def set_level0_stamps(self, on=True):
        """timed iterations stamp the fused level-0 launch with its own dispatch events (exact duration; perturbs the other phases)"""
        return self._chk(self.lib.gpslam_hip_set_level0_stamps(self._h, 1 if on else 0), "set_level0_stamps")

    def last_level0_ms(self):
        """device ms of the level-0 forward launch, summed over the iterations of the last timed run_gn / iterate_gn"""
        out = C.c_double(0.0)
        self._chk(self.lib.gpslam_hip_last_level0_ms(self._h, C.byref(out)), "last_level0_ms")
        return out.value

    def last_timing(self):
        t = np.zeros(5)
        self.lib.gpslam_hip_last_timing(self._h, _p(t))
        return t

    def time_kernel(self, which, reps=10):
        out = C.c_double(0.0)
        self._chk(self.lib.gpslam_hip_time_kernel(self._h, int(which), int(reps), C.byref(out)), "time_kernel")
        return out.value

    def stream(self):
        return self.lib.gpslam_hip_stream(self._h)

    def set_stream(self, hip_stream):
        return self._chk(self.lib.gpslam_hip_set_stream(self._h, C.c_void_p(hip_stream)), "set_stream")

    def set_collectives(self, all_gather, all_reduce_sum=None):
        """gpslam_hip_set_collectives: hand the library the host's collectives, after which iterate_gn / run_gn / iterate_lm /
        optimize / error work on this rank's handle (or split piece) and return the whole chain's statistics.
            all_gather(send_ptr, recv_ptr, bytes_per_rank, hip_stream)     all_reduce_sum(buf_ptr, n_doubles, hip_stream)
        are Python callables working on raw device pointers, on the handle's stream; an exception becomes GPSLAM_E_COMM."""
        def guard(fn):
            def run(_user, *args):
                try:
                    fn(*args)
                    return 0
                except Exception:       # noqa: BLE001 -- no exception may cross the C ABI
                    import traceback
                    traceback.print_exc()
                    return 1
            return run
        self._cb_gather = ALL_GATHER_FN(guard(all_gather)) if all_gather else ALL_GATHER_FN()
        self._cb_reduce = ALL_REDUCE_FN(guard(all_reduce_sum)) if all_reduce_sum else ALL_REDUCE_FN()
        return self._chk(self.lib.gpslam_hip_set_collectives(self._h, self._cb_gather, self._cb_reduce, None), "set_collectives")

    # ---- segment sharding (nranks > 1)
    def set_halo_state(self, pose, vel):
        pose, vel = _f64(pose), _f64(vel)
        return self._chk(self.lib.gpslam_hip_set_halo_state(self._h, _p(pose), _p(vel)), "set_halo_state")

    def interface_buffers(self):
        """(send_ptr, send_bytes, recv_ptr, recv_bytes): device pointers of this rank's interface record and of
        the gathered records of all ranks."""
        sp, rp = C.c_void_p(), C.c_void_p()
        sb, rb = C.c_size_t(), C.c_size_t()
        self._chk(self.lib.gpslam_hip_interface_send(self._h, C.byref(sp), C.byref(sb)), "interface_send")
        self._chk(self.lib.gpslam_hip_interface_recv(self._h, C.byref(rp), C.byref(rb)), "interface_recv")
        return sp.value, sb.value, rp.value, rb.value

    def iterate_phase1(self, lam=0.0):
        return self._chk(self.lib.gpslam_hip_iterate_phase1(self._h, C.c_double(lam)), "iterate_phase1")

    def iterate_phase2a(self):
        return self._chk(self.lib.gpslam_hip_iterate_phase2a(self._h), "iterate_phase2a")

    def iterate_phase2b(self, want_stats=True):
        st = Stats()
        self._chk(self.lib.gpslam_hip_iterate_phase2b(self._h, C.byref(st) if want_stats else None), "iterate_phase2b")
        return st

    def lm_begin(self):
        return self._chk(self.lib.gpslam_hip_lm_begin(self._h), "lm_begin")

    def lm_trial_phase1(self, lam):
        return self._chk(self.lib.gpslam_hip_lm_trial_phase1(self._h, C.c_double(lam)), "lm_trial_phase1")

    def lm_trial_phase2(self):
        """[error, trial error, |delta|_inf, delta.g, |delta|^2, indefinite flag] of this rank."""
        out = np.zeros(6)
        self._chk(self.lib.gpslam_hip_lm_trial_phase2(self._h, _p(out)), "lm_trial_phase2")
        return out

    def lm_reject(self):
        return self._chk(self.lib.gpslam_hip_lm_reject(self._h), "lm_reject")

    def landmark_reduce_buffer(self):
        """(device pointer, bytes) of this rank's landmark Schur complement [S | gL]; (None, 0) without landmarks."""
        ptr, nb = C.c_void_p(), C.c_size_t()
        self._chk(self.lib.gpslam_hip_landmark_reduce_buffer(self._h, C.byref(ptr), C.byref(nb)), "landmark_reduce_buffer")
        return ptr.value, nb.value

    # ---- config 4 across GPUs: pieces of a chain joined at shared cut states (include/gpslam_hip.h, fs_set_split)
    def fs_set_split(self, rank, nranks, first_lm=(), last_lm=()):
        f = np.ascontiguousarray(first_lm, dtype=np.int32)
        l = np.ascontiguousarray(last_lm, dtype=np.int32)
        return self._chk(self.lib.gpslam_hip_fs_set_split(self._h, C.c_int32(rank), C.c_int32(nranks), _p(f) if len(f) else None, C.c_int32(len(f)),
                                                          _p(l) if len(l) else None, C.c_int32(len(l))), "fs_set_split")

    def fs_split_info(self):
        out = (C.c_int32 * 4)()
        self._chk(self.lib.gpslam_hip_fs_split_info(self._h, out), "fs_split_info")
        return dict(fat_block=out[0], fat_blocks=out[1], segment_length=out[2], nb_top=out[3])

    def fs_set_top(self, nb_top):
        return self._chk(self.lib.gpslam_hip_fs_set_top(self._h, C.c_int32(nb_top)), "fs_set_top")

    def fs_interface(self):
        """(send pointer, bytes, recv pointer, bytes) of the interface record and of the gathered records."""
        sp, rp = C.c_void_p(), C.c_void_p()
        sb, rb = C.c_size_t(), C.c_size_t()
        self._chk(self.lib.gpslam_hip_fs_interface(self._h, C.byref(sp), C.byref(sb), C.byref(rp), C.byref(rb)), "fs_interface")
        return sp.value, sb.value, rp.value, rb.value

    def fs_phase1(self, lam=0.0):
        return self._chk(self.lib.gpslam_hip_fs_phase1(self._h, C.c_double(lam)), "fs_phase1")

    def fs_phase2(self, want_stats=True):
        st = Stats()
        self._chk(self.lib.gpslam_hip_fs_phase2(self._h, C.byref(st) if want_stats else None), "fs_phase2")
        return st

    def fs_lm_trial_phase1(self, lam):
        return self._chk(self.lib.gpslam_hip_fs_lm_trial_phase1(self._h, C.c_double(lam)), "fs_lm_trial_phase1")

    def fs_lm_trial_phase2(self):
        """[error, trial error, |delta|_inf, delta.g, |delta|^2, indefinite flag] of this piece."""
        out = np.zeros(6)
        self._chk(self.lib.gpslam_hip_fs_lm_trial_phase2(self._h, _p(out)), "fs_lm_trial_phase2")
        return out

    def iterate_phase2(self, want_stats=True):
        st = Stats()
        self._chk(self.lib.gpslam_hip_iterate_phase2(self._h, C.byref(st) if want_stats else None), "iterate_phase2")
        return st
