/*
 * gpslam_hip.h -- C ABI of the MI355X-native GP-SLAM Gauss-Newton / Levenberg-Marquardt inner loop.
 *
 * This is the drop-in boundary.  In the reference (gtrll/gpslam) the hot path
 * sits behind GTSAM's NonlinearFactor virtual interface: every factor overrides
 *     gtsam::Vector evaluateError(x1, ..., boost::optional<gtsam::Matrix&> H1, ...)
 * (e.g. gpslam/gp/GaussianProcessPriorPose3.h:60-64) and GTSAM's optimizers call it factor by
 * factor, whiten, eliminate and retract on the CPU
 * (call sites: gpslam/gp/tests/testGaussianProcessPriorPose3.cpp:185-188, matlab/PlazaPose2.m:208-228).
 * Here the whole chain-structured graph lives in HBM behind an opaque handle and each of those steps
 * is a batched HIP kernel.  The C++ host classes in gpslam_amd/host/ (same names and ctor signatures
 * as gpslam.h / GTSAM) and the Python mirror in gpslam_amd/ bind to exactly these entry points.
 *
 * Conventions
 *  - All functions return 0 on success, <0 on failure (GPSLAM_E_*); no exceptions cross the ABI.
 *  - The caller owns every host buffer; the library owns all device memory behind the handle.
 *  - One handle = one HIP stream; a handle is thread-compatible, not thread-safe.
 *  - Host arrays are row-major doubles.  Pose layouts (per state):
 *        LINEAR2/LINEAR3: D doubles;   POSE2: (x, y, theta);   ROT3: R row-major (9);
 *        POSE3: R row-major (9) then t (3).   Velocities: d doubles, d = tangent dimension
 *        (POSE3: (omega, v) rotation first; POSE2: (vx, vy, omega)).
 *  - State i is the pair (pose_i, vel_i); the variable ordering is the explicit chain order
 *    [x0, v0, x1, v1, ..., l0, l1, ...].  Factors that couple two states couple i and i+1 only
 *    (the GP Markov property, gpslam/gp/GaussianProcessPriorPose3.h:43-47).
 *  - Noise models: the GP prior uses Q(dt) built from Qc (gpslam/gp/GPutils.h:24-41) -- the handle's shared one or one per
 *    factor (add_gp_priors_qc); every other factor takes diagonal sigmas, or a full Gaussian covariance through
 *    gpslam_hip_set_meas_covariance; measurement factors and loop closures also a robust loss on top of either
 *    (noiseModel::Robust: gpslam_hip_set_meas_robust, gpslam_hip_set_between_pairs_robust).
 */
#ifndef GPSLAM_HIP_H
#define GPSLAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpslam_hip_handle gpslam_hip_handle;

enum { GPSLAM_LINEAR2 = 0, GPSLAM_LINEAR3 = 1, GPSLAM_POSE2 = 2, GPSLAM_POSE3 = 3, GPSLAM_ROT3 = 4, GPSLAM_ROT3_BIAS = 5 };
/* GPSLAM_ROT3_BIAS: the AHRS state of matlab/GPAHRSexample.m:69-202 (gtsam keys x_i Rot3, v_i Vector3, b_i Vector3):
 *   pose slot (12 doubles) = [R row-major (9) | gyroscope bias b_i (3)],  tangent (dtheta, db)
 *   velocity slot (6)      = [angular velocity v_i (3) | 0 0 0],           the three pads stay zero
 * set_qc takes the 3 x 3 Qc of GaussianProcessPriorRot3; add_gp_priors = GaussianProcessPriorRot3 on (x, v);
 * add_pose_priors = [PriorFactorRot3 ; PriorFactorVector(b)] and add_between = [BetweenFactorRot3 ; BetweenFactorVector(b)]
 * with 6 sigmas each, INFINITY switching a half off; add_vel_priors: 6 sigmas, the last three ignored;
 * add_interp_attitude = GPInterpolatedAttitudeFactorRot3; gpslam_hip_add_ahrs = gtsam::AHRSFactor. */
/* retract chart of the state update (and, for POSE2, of PriorFactor / BetweenFactor's Local):
 * EXPMAP       x Exp(delta) on every manifold (GTSAM >= 4.1 defaults; GTSAM_ROT3_EXPMAP / GTSAM_POSE3_EXPMAP /
 *              SLOW_BUT_CORRECT_EXPMAP builds of 4.0)
 * FIRST_ORDER  GTSAM 4.0's default charts: POSE2 x * Pose2(dx, dy, dtheta); ROT3 R * Cayley(w);
 *              POSE3 (R * Cayley(w), t + R v).  All charts agree to first order: the fixed point is the same. */
enum { GPSLAM_CHART_EXPMAP = 0, GPSLAM_CHART_FIRST_ORDER = 1 };
enum { GPSLAM_FP64 = 0, GPSLAM_FP32 = 1 };
/* velocity parameterisation of a POSE3 chain (config_v2.velocity; v1: config.reserved[3]):
 * BODY      6-vector body-frame velocity (w, v): GaussianProcessPriorPose3 / InterpolatorPose3 (gpslam.h:32-35, :72-77)
 * WORLD_VW  world-frame translational v and rotational w, stored as [v; w]: GaussianProcessPriorPose3VW,
 *           GaussianProcessInterpolatorPose3VW, GPInterpolatedGPSFactorPose3VW (gpslam.h:38-41, :65-70;
 *           gpslam/gp/GaussianProcessPriorPose3VW.h:62-117).  gtsam keys (x_i, v_i, w_i) map to one state. */
enum { GPSLAM_VELOCITY_BODY = 0, GPSLAM_VELOCITY_WORLD_VW = 1 };

enum {
  GPSLAM_OK = 0,
  GPSLAM_E_INVALID = -1,      /* bad argument / wrong manifold for this factor */
  GPSLAM_E_HIP = -2,          /* a HIP runtime call failed */
  GPSLAM_E_NOT_SPD = -3,      /* a pivot block was not positive definite (indeterminate system) */
  GPSLAM_E_NOT_COMPILED = -4, /* gpslam_hip_compile() has not been called since the last change */
  GPSLAM_E_UNSUPPORTED = -5,
  GPSLAM_E_NAN = -6,
  GPSLAM_E_COMM = -7          /* a collective supplied through gpslam_hip_set_collectives reported a failure */
};

/* ---- ABI version (round 6).  Everything a caller's struct layouts depend on is behind one number: the library reports the
 * version it was built from (gpslam_hip_abi_version) and the sizes of its structs (gpslam_hip_struct_size); a binding checks
 * both once at load time (gpslam_amd/chain.py: load_library; gpslam_amd/host/gpslam_host.hpp: check_abi) instead of finding out
 * through a corrupted stack.  History: 1.0 rounds 1-4 (gpslam_hip_stats 48 bytes); 1.1 round 5 (stats 56 bytes: trials,
 * last_trial_error; GPSLAM_E_COMM; plan bits 64, 128) -- shipped without a version symbol; 2.0 this header: gpslam_hip_config_v2 +
 * gpslam_hip_create_v2 (named fields, struct_size first), gpslam_hip_abi_version, gpslam_hip_struct_size.  The v1 config and
 * gpslam_hip_create stay, bit for bit; 2.1 gpslam_hip_add_between_pairs (loop closures); 2.2 gpslam_hip_set_level0_stamps; 2.3
 * gpslam_hip_marginals, gpslam_hip_get_marginals, gpslam_hip_interpolate_covariances; 2.4 gpslam_hip_launch_census (and, added since without a bump,
 * gpslam_hip_set_closure_passes / gpslam_hip_closure_info / gpslam_hip_marginals_keep_closure_columns / gpslam_hip_marginals_on_segments /
 * gpslam_hip_get_landmark_marginals / gpslam_hip_get_state_landmark_marginals / gpslam_hip_get_landmark_pair_marginals /
 * gpslam_hip_add_state_gaussians / gpslam_hip_get_state_gaussians / gpslam_hip_marginalize_head / gpslam_hip_get_head_prior / gpslam_hip_append_states /
 * gpslam_hip_add_border_gaussians / gpslam_hip_get_border_gaussians / gpslam_hip_marginalize_head_onto_landmarks / gpslam_hip_get_head_prior_border /
 * gpslam_hip_marginals_keep_pair_terms / gpslam_hip_get_state_pair_marginals / gpslam_hip_gate_between_pairs).  A MAJOR bump changes a struct or a
 * signature, a MINOR bump only adds. */
#define GPSLAM_HIP_ABI_MAJOR 2
#define GPSLAM_HIP_ABI_MINOR 4
#define GPSLAM_HIP_ABI_VERSION ((GPSLAM_HIP_ABI_MAJOR << 16) | GPSLAM_HIP_ABI_MINOR)
uint32_t gpslam_hip_abi_version(void);
enum { GPSLAM_STRUCT_CONFIG = 0, GPSLAM_STRUCT_CONFIG_V2 = 1, GPSLAM_STRUCT_STATS = 2, GPSLAM_STRUCT_PARAMS = 3 };
/* sizeof() of the named struct in the library's build (0: unknown struct) */
size_t gpslam_hip_struct_size(int32_t which);

/* What a binding written against gpslam.h's class list fills in (gpslam_hip_create_v2).  struct_size = sizeof(gpslam_hip_config_v2)
 * of the CALLER's header: a library that knows a longer struct reads the fields the caller has and takes defaults (0) for the rest;
 * a library that knows a shorter one accepts the call only if the bytes it does not know are zero (GPSLAM_E_UNSUPPORTED otherwise). */
typedef struct {
  uint32_t struct_size;     /* sizeof(gpslam_hip_config_v2) */
  int32_t manifold;         /* GPSLAM_LINEAR2 .. GPSLAM_ROT3_BIAS */
  int32_t precision;        /* GPSLAM_FP64 | GPSLAM_FP32 (a tolerance mode, see gpslam_hip_config.precision) */
  int32_t device;           /* HIP device ordinal */
  int32_t chart;            /* GPSLAM_CHART_* */
  int32_t landmark_dim;     /* 0 (no landmarks), 2 or 3 */
  int32_t chunk;            /* level-0 chunk length of the partitioned solver; 0 = default */
  int32_t rank, nranks;     /* contiguous-segment sharding: this handle owns segment `rank` of `nranks` */
  int32_t force_sharded;    /* 1: the sharded code path on a single segment (self-test of the exchange plumbing)      v1 reserved[0] */
  int32_t upper_chunk;      /* chunk length of the solver levels above level 0; 0 / 1 = default (LDS-resident groups)  v1 reserved[1] */
  int32_t top_blocks;       /* size of the sequential top level; 0 = default                                          v1 reserved[2] */
  int32_t velocity;         /* GPSLAM_VELOCITY_* (POSE3 only): body (w, v) or the *Pose3VW family's world [v; w]      v1 reserved[3] */
  int32_t segment_length;   /* segmented landmark elimination: states per segment; 0 = the smallest that fits         v1 reserved[4] */
  int32_t force_segmented;  /* 1: the segmented landmark elimination for any landmark count                           v1 reserved[5] */
  int32_t plan;             /* mask of GPSLAM_PLAN_* bits; 0 = the default plan                                       v1 reserved[6] */
} gpslam_hip_config_v2;

/* v1 (rounds 1-5): the same eight knobs as anonymous words.  Kept so that callers built against the old header keep working. */
typedef struct {
  int32_t manifold;      /* GPSLAM_LINEAR2 .. GPSLAM_ROT3 */
  int32_t precision;     /* GPSLAM_FP64, or GPSLAM_FP32: fp32 Jacobian rows (evaluated re-centred, with the exact derivative in place of the
                          * h = 1e-6 difference), fp64 residual, normal equations and solver.  A TOLERANCE mode
                          * (north_star's 1e-5-relative sweep, half the row-table footprint), not a throughput mode: the structured
                          * GP-prior records of the fp64 path are fp64-only, fp32 rows are slower per iteration on every measured mix */
  int32_t device;        /* HIP device ordinal */
  int32_t chart;         /* GPSLAM_CHART_* */
  int32_t landmark_dim;  /* 0 (no landmarks), 2 or 3 */
  int32_t chunk;         /* level-0 chunk length of the partitioned solver; 0 = default */
  int32_t rank, nranks;  /* contiguous-segment sharding: this handle owns segment `rank` of `nranks` */
  int32_t reserved[8];   /* [0] force the sharded code path, [1] upper-level chunk length, [2] sequential top size,
                          * [3] GPSLAM_VELOCITY_* (POSE3 only), [4] segment length of the segmented landmark elimination
                          * (0 = smallest that fits), [5] 1 = use the segmented landmark elimination for any landmark
                          * count (default: only when the landmarks do not fit the dense border), [6] mask of GPSLAM_PLAN_* bits
                          * (below; 0 = the default plan); [7] must be 0 */
} gpslam_hip_config;
/* config_v2.plan (v1: config.reserved[6]): kernel families compile() may be told to use instead of its default choice.  Every one of them is the
 * path some graphs take anyway (chains with landmark columns, pinned hierarchy shapes, wide landmark borders, graphs whose
 * full-width rows are not all GP priors); the bits exist so that tests run them on plain chains and so that a maintainer
 * can A/B them per handle (gpslam_hip_plan_info shows what a handle ended up with).  No reference counterpart. */
enum {
  GPSLAM_PLAN_UNFUSED_LEVEL0 = 1,     /* assembly and level-0 elimination as two launches (k_assemble_ghost + k_chunk_forward_rows) */
  GPSLAM_PLAN_COLUMN_LEVEL0 = 2,      /* column-layout level-0 elimination (k_chunk_forward; implies the two launches) */
  GPSLAM_PLAN_LEVELS_OF_FOUR = 4,     /* upper hierarchy as one launch per level of chunks of four instead of LDS-resident cyclic reduction */
  GPSLAM_PLAN_FS_TWO_LAUNCHES = 8,    /* segmented landmark elimination: border sweep and Schur complement as two launches through Y */
  GPSLAM_PLAN_GP_ROWS = 16,           /* GP priors as plain Jacobian rows instead of structured records */
  GPSLAM_PLAN_GENERIC_QC = 32,        /* SE(3) records: the general (upper-triangular) chol(Qc^-1) form even when Qc is diagonal */
  GPSLAM_PLAN_MEAS_ROWS = 64,         /* SE(3) records: interpolated GPS factors as plain 24-column rows (k_fused_level0<3>) instead of 16-double lines (<4>) */
  GPSLAM_PLAN_SEPARATE_RETRACT = 128  /* gpslam_hip_run_gn: every iteration ends with its own k_retract launch instead of leaving the retraction to the next K1 */
};

/* per-call statistics; mirrors what GTSAM's optimizers expose (error(), iterations(), lambda()) */
typedef struct {
  double error_before;    /* 0.5 * sum |R e|^2 at the linearisation point */
  double error_after;     /* after the accepted update */
  double delta_inf_norm;  /* max |delta| over all variables */
  double lambda;          /* LM damping after the step */
  int32_t iterations;
  int32_t status;
  int32_t accepted;
  int32_t trials;         /* iterate_lm: lambdas tried by this call (0 elsewhere) */
  double last_trial_error;/* iterate_lm: error at the last lambda tried, kept or not; lets a caller see how far the cost moved on a
                           * trial that was not kept (a change at rounding level makes the fidelity test a ratio of two rounding
                           * errors: tests compare lambda schedules only above it) */
} gpslam_hip_stats;

/* GaussNewtonParams / LevenbergMarquardtParams (GTSAM names; defaults = GTSAM 4.0 defaults) */
typedef struct {
  int32_t max_iterations;     /* 100 */
  double relative_error_tol;  /* 1e-5 */
  double absolute_error_tol;  /* 1e-5 */
  double error_tol;           /* 0 */
  double delta_tol;           /* if > 0 additionally stop when |delta|_inf < delta_tol */
  double lambda_initial;      /* 1e-5 */
  double lambda_factor;       /* 10 */
  double lambda_upper_bound;  /* 1e5 */
  double lambda_lower_bound;  /* 0 */
  double min_model_fidelity;  /* 1e-3 */
  int32_t use_lm;             /* 0 Gauss-Newton, 1 Levenberg-Marquardt */
  int32_t pad;
} gpslam_hip_params;

/* ---- life cycle ---- */
int gpslam_hip_create(const gpslam_hip_config *cfg, gpslam_hip_handle **out);
int gpslam_hip_create_v2(const gpslam_hip_config_v2 *cfg, gpslam_hip_handle **out);
int gpslam_hip_destroy(gpslam_hip_handle *h);
void gpslam_hip_default_params(gpslam_hip_params *p);
const char *gpslam_hip_last_error(const gpslam_hip_handle *h);
/* the HIP stream (hipStream_t) all kernels of this handle are launched on */
void *gpslam_hip_stream(gpslam_hip_handle *h);
/* run on a caller-owned stream instead (e.g. the stream RCCL collectives are ordered against) */
int gpslam_hip_set_stream(gpslam_hip_handle *h, void *hip_stream);

/* ---- variables (replaces gtsam::Values::insert / at, e.g. testGaussianProcessPriorPose3.cpp:179-183) ---- */
int gpslam_hip_set_states(gpslam_hip_handle *h, int32_t N, const double *pose, const double *vel);
int gpslam_hip_get_states(gpslam_hip_handle *h, double *pose, double *vel);
int gpslam_hip_set_landmarks(gpslam_hip_handle *h, int32_t L, const double *pts);
int gpslam_hip_get_landmarks(gpslam_hip_handle *h, double *pts);
/* power-spectral density Qc (d x d, SPD) shared by all GP priors/interpolators
 * (replaces the Qc_model ctor argument + getQc, gpslam/gp/GPutils.cpp:16-20) */
int gpslam_hip_set_qc(gpslam_hip_handle *h, const double *Qc);

/* ---- factors (replace NonlinearFactorGraph::add of the named class) ---- */
/* GaussianProcessPrior{Linear,Pose2,Pose3,Rot3}(key_i, vel_i, key_i+1, vel_i+1, dt, Qc_model)
 * gpslam/gp/GaussianProcessPriorPose3.h:43-49 and siblings */
int gpslam_hip_add_gp_priors(gpslam_hip_handle *h, int32_t count, const int32_t *left, const double *dt);
/* ... with ONE Qc_model PER FACTOR, as the reference's constructors take it (gpslam/gp/GaussianProcessPriorPose3.h:43-49,
 * GaussianProcessPriorLinear.h:45-52): Qc = count x d x d (GPSLAM_ROT3_BIAS: 3 x 3), each SPD.  Factors added through
 * gpslam_hip_add_gp_priors use the handle's shared Qc (set_qc).  A graph with several distinct Qc is linearised with one
 * launch per distinct Qc.  (The interpolated measurement factors do not need their Qc_model at all: in
 * Psi = Q(tau) Phi(dt - tau)^T Q^-1(dt) = (A(tau) Phi2^T A^-1(dt)) (x) (Qc Qc^-1) and Lambda = Phi(tau) - Psi Phi(dt)
 * -- gpslam/gp/GPutils.h:54-71 -- Qc cancels for every SPD Qc, so their constructors' Qc_model argument has no effect
 * on evaluateError; GPInterpolatedRangeFactorPose2.h:46-54.) */
int gpslam_hip_add_gp_priors_qc(gpslam_hip_handle *h, int32_t count, const int32_t *left, const double *dt, const double *Qc);
/* gtsam::PriorFactor<Pose> on x_idx, diagonal sigmas (count x d) */
int gpslam_hip_add_pose_priors(gpslam_hip_handle *h, int32_t count, const int32_t *idx, const double *prior,
                               const double *sigmas);
/* gtsam::PriorFactor<Vector> on v_idx */
int gpslam_hip_add_vel_priors(gpslam_hip_handle *h, int32_t count, const int32_t *idx, const double *prior,
                              const double *sigmas);
/* gtsam::BetweenFactor<Pose>(x_left, x_left+1, measured) (matlab/PlazaPose2.m:125) */
int gpslam_hip_add_between(gpslam_hip_handle *h, int32_t count, const int32_t *left, const double *measured,
                           const double *sigmas);
/* gtsam::BetweenFactor<Pose>(x_first, x_second, measured) between ANY two states of the chain -- a loop closure (round 6; ABI 2.1).
 * The reference's factors take arbitrary keys (gpslam/gp/GaussianProcessPriorPose3.h:43-47) and GTSAM eliminates whatever graph
 * they form; here everything but closures couples state i with i + 1, and a closure is applied to the chain solve as a low-rank
 * correction: its d whitened rows ride through the block-tridiagonal solver as d extra right-hand sides behind the landmark
 * columns (Sherman-Morrison-Woodbury; closures.hpp "loop closures").  Pairs with second == first + 1 are ordinary chain factors
 * (add_between).  Capacity of one pass: 1 + landmarks * landmark_dim + closures * d <= 28 right-hand sides (Pose2 / Rot3 / Linear3:
 * 9 closures without landmarks, Pose3: 4); compile() answers GPSLAM_E_UNSUPPORTED beyond that unless gpslam_hip_set_closure_passes
 * allowed column passes (then closures * d <= 120: 40 closures, Pose3: 20), and always on fp32 handles, on sharded handles and on
 * the segmented landmark path.  measured: count x pose_dim, sigmas: count x d.  Gauss-Newton, Levenberg-Marquardt, optimize and
 * error include the closures; gpslam_hip_normal_equations reports the chain part H0 (the closures' blocks are not in D / O / g). */
int gpslam_hip_add_between_pairs(gpslam_hip_handle *h, int32_t count, const int32_t *first, const int32_t *second,
                                 const double *measured, const double *sigmas);
/* Loop closures beyond one border: column passes.  Call before compile().  max_passes <= 1 (the default) leaves the capacity above
 * as it is.  With max_passes >= 2 compile() deals the closures, in the order they were added, into P = ceil(closures / w) slices of
 * w closures -- closures_per_pass if that is > 0, else the most that fit: 1 + landmarks * landmark_dim + w * d <= 28 -- and one linear
 * solve becomes P passes of the chain solver over the closures' columns, a dense (closures * d)-square solve, and one final pass
 * (closures.hpp CloPass); the linearisation still runs once.  A graph whose closures fit one pass (P == 1) keeps the single-pass path
 * bit for bit.  compile() answers GPSLAM_E_UNSUPPORTED when the landmark columns leave no room for a closure, when
 * closures_per_pass is larger than fits, when P > max_passes and when closures * d > 120; fp32, sharded and segmented handles
 * refuse closures as before.  gpslam_hip_marginals answers GPSLAM_E_UNSUPPORTED on a handle with P > 1 unless
 * gpslam_hip_marginals_keep_closure_columns was called on it. */
int gpslam_hip_set_closure_passes(gpslam_hip_handle *h, int32_t max_passes, int32_t closures_per_pass);
/* after compile(): {closures, closures per pass w, column passes P, solves of the chain per linear system (P + 1 beyond one pass)} */
int gpslam_hip_closure_info(gpslam_hip_handle *h, int32_t out4[4]);
/* gtsam::PriorFactor<Point> on landmark idx (matlab/PlazaPose2.m:63) */
int gpslam_hip_add_landmark_priors(gpslam_hip_handle *h, int32_t count, const int32_t *idx, const double *prior,
                                   const double *sigmas);
/* GPInterpolatedRangeFactor{Pose2,Pose3,2DLinear}(z, model, Qc, x_i, v_i, x_i+1, v_i+1, l, dt, tau[, body_P_sensor])
 * gpslam/slam/GPInterpolatedRangeFactorPose2.h:46-54; sensor: body_P_sensor of THIS call's `count` factors or NULL.
 * Every factor keeps its own body_P_sensor as in the reference (GPInterpolatedRangeFactorPose3.h:46-54): calls with
 * different sensor poses may be mixed freely on one handle. */
int gpslam_hip_add_interp_range(gpslam_hip_handle *h, int32_t count, const int32_t *left, const int32_t *landmark,
                                const double *z, const double *sigma, const double *dt, const double *tau,
                                const double *sensor);
/* RangeFactorPose2 / RangeFactor2DLinear (gpslam/slam/RangeFactor2DLinear.h:30-37) */
int gpslam_hip_add_range(gpslam_hip_handle *h, int32_t count, const int32_t *idx, const int32_t *landmark,
                         const double *z, const double *sigma);
/* GPInterpolatedAttitudeFactorRot3(keys, dt, tau, Qc, model, nZ, bRef) -- GPInterpolatedAttitudeFactorRot3.h:44-51 */
int gpslam_hip_add_interp_attitude(gpslam_hip_handle *h, int32_t count, const int32_t *left, const double *nZ,
                                   const double *bRef, const double *sigma, const double *dt, const double *tau);
/* gtsam::AHRSFactor(x_left, x_left+1, b_left, PreintegratedAhrsMeasurements, omegaCoriolis) -- GTSAM 4.0
 * gtsam/navigation/AHRSFactor.h (third party; call site matlab/GPAHRSexample.m:128-137).  GPSLAM_ROT3_BIAS handles only.
 * Per factor, the state of the pre-integration after its last integrateMeasurement():
 *   delta_R (9, deltaRij row-major), dR_dbias (9, delRdelBiasOmega), bias_hat (3), delta_tij (1),
 *   cov (9, preintMeasCov: the factor's Gaussian noise model, SPD)
 * omega_coriolis: 3 doubles shared by the call, or NULL (the recipe passes zeros).
 * gpslam_amd/host/gpslam_host.hpp and gpslam_amd/ahrs.py restate PreintegratedAhrsMeasurements::integrateMeasurement. */
int gpslam_hip_add_ahrs(gpslam_hip_handle *h, int32_t count, const int32_t *left, const double *delta_R,
                        const double *dR_dbias, const double *bias_hat, const double *delta_tij, const double *cov,
                        const double *omega_coriolis);
/* GPInterpolatedGPSFactorPose3 -- gpslam/slam/GPInterpolatedGPSFactorPose3.h:46-54 */
int gpslam_hip_add_interp_gps(gpslam_hip_handle *h, int32_t count, const int32_t *left, const double *measured,
                              const double *sigmas, const double *dt, const double *tau, const double *sensor);
/* GPInterpolatedProjectionFactorPose3<Cal3_S2>(measured, cam_model, Qc_model, x_i, v_i, x_i+1, v_i+1, l, delta_t, tau, K,
 * body_P_sensor) -- gpslam/slam/GPInterpolatedProjectionFactorPose3.h:64-139: reprojection error of 3-D landmark l
 * through a pinhole camera riding on the GP-interpolated pose.  measured: count x 2 pixels, sigmas: count x 2,
 * K = {fx, fy, s, u0, v0} (gtsam::Cal3_S2, kept per factor: calls may differ), sensor = body_P_sensor (12 doubles) or NULL.
 * throwCheirality = false semantics: a landmark behind the camera contributes error 2 fx and zero Jacobians. */
int gpslam_hip_add_interp_projection(gpslam_hip_handle *h, int32_t count, const int32_t *left, const int32_t *landmark,
                                     const double *measured, const double *sigmas, const double *dt, const double *tau,
                                     const double *K, const double *sensor);
/* The same factor with CALIBRATION = gtsam::Cal3DS2 (the reference class is a template over it,
 * GPInterpolatedProjectionFactorPose3.h:29): K9 = {fx, fy, s, u0, v0, k1, k2, p1, p2}, radial (k1, k2) and tangential
 * (p1, p2) distortion of the intrinsic point before the linear calibration (Cal3DS2_Base::uncalibrate).  Zero coefficients
 * give the Cal3_S2 factor bit for bit; both kinds may share a graph. */
int gpslam_hip_add_interp_projection_ds2(gpslam_hip_handle *h, int32_t count, const int32_t *left, const int32_t *landmark,
                                         const double *measured, const double *sigmas, const double *dt, const double *tau,
                                         const double *K9, const double *sensor);
/* OdometryFactor2DLinear(x_left, x_left+1, measured) -- gpslam/slam/OdometryFactor2DLinear.h:38-40 */
int gpslam_hip_add_odometry2d(gpslam_hip_handle *h, int32_t count, const int32_t *left, const double *measured,
                              const double *sigmas);
/* RangeBearingFactor2DLinear(x, l, range, bearing) -- gpslam/slam/RangeBearingFactor2DLinear.h:33-37 */
int gpslam_hip_add_bearing_range(gpslam_hip_handle *h, int32_t count, const int32_t *idx, const int32_t *landmark,
                                 const double *bearing, const double *range, const double *sigmas);

/* noiseModel::Gaussian::Covariance on measurement factors.  The reference's constructors take any gtsam::SharedNoiseModel
 * (gpslam/slam/GPInterpolatedGPSFactorPose3.h:46-54, GPInterpolatedRangeFactorPose3.h:46-54, OdometryFactor2DLinear.h:38-40);
 * the add_* calls above take diagonal sigmas.  This call replaces the noise model of the `count` most recently added factors
 * of `kind` (GPSLAM_MEAS_*, not AHRS: that one takes its covariance itself) by full covariances, cov = count x rows x rows
 * (rows = residual dimension of the kind), each SPD: the rows are whitened by R = chol_upper(cov^-1), R^T R = cov^-1, as
 * gtsam::noiseModel::Gaussian does. */
int gpslam_hip_set_meas_covariance(gpslam_hip_handle *h, int32_t kind, int32_t count, const double *cov);

/* noiseModel::Robust(mEstimator, base) on measurement factors and loop closures (gtsam/linear/NoiseModel.h, LossFunctions.h; added
 * without an ABI bump: a binding detects these entry points by their presence).  The base model is what the factor has -- sigmas, or
 * the square-root information of set_meas_covariance; the loss (kind, k) sits on top of it.  With e_w the factor's whitened error
 * over all of its rows and r = |e_w|_2:
 *   linearisation  every row of the factor and its error entry are multiplied by sqrt(w(r)), ONE weight per factor -- GTSAM's
 *                  Robust::WhitenSystem with Block reweighting: noise_->WhitenSystem(A, b); robust_->reweight(A, b);
 *   cost           gpslam_hip_error, error_before / error_after and every cost Levenberg-Marquardt compares take rho(r) for the
 *                  factor in place of r^2 / 2 -- Robust::loss of GTSAM >= 4.1 (4.0 reported w r^2 / 2, which for the redescending
 *                  losses falls to zero as a residual grows: DESIGN.md section 2).  The model-fidelity denominator stays the
 *                  weighted linear system's, as in GTSAM.
 * With u = r^2 / k^2 (mEstimator::Huber, Cauchy, Tukey, GemanMcClure, Welsh, Fair):
 *   HUBER          w = 1 (r <= k), k / r            rho = r^2 / 2 (r <= k), k (r - k / 2)
 *   CAUCHY         w = k^2 / (k^2 + r^2)            rho = (k^2 / 2) log(1 + u)
 *   TUKEY          w = (1 - u)^2 (r <= k), 0        rho = k^2 (1 - (1 - u)^3) / 6 (r <= k), k^2 / 6
 *   GEMAN_MCCLURE  w = k^4 / (k^2 + r^2)^2          rho = k^2 r^2 / (2 (k^2 + r^2))
 *   WELSH          w = exp(-u)                      rho = (k^2 / 2) (1 - exp(-u))
 *   FAIR           w = 1 / (1 + r / k)              rho = k^2 (r / k - log(1 + r / k))
 * each with rho'(r) = w(r) r, rho(0) = 0, w(0) = 1.  k <= 0 or not finite: GPSLAM_E_INVALID.  A factor whose loss is NONE, and a
 * handle on which every loss is NONE, run exactly as without these calls.
 * compile() answers GPSLAM_E_UNSUPPORTED on fp32 handles, sharded handles and split pieces that carry any loss.  A graph with a robust
 * interpolated GPS factor keeps those factors as 24-column rows (as GPSLAM_PLAN_MEAS_ROWS does): the weight needs all three rows.
 * gpslam_hip_marginals linearises through the same kernels and so inverts the reweighted H, as gtsam::Marginals does. */
enum { GPSLAM_ROBUST_NONE = 0, GPSLAM_ROBUST_HUBER = 1, GPSLAM_ROBUST_CAUCHY = 2, GPSLAM_ROBUST_TUKEY = 3, GPSLAM_ROBUST_GEMAN_MCCLURE = 4,
       GPSLAM_ROBUST_WELSH = 5, GPSLAM_ROBUST_FAIR = 6 };
/* replaces the loss of the `count` most recently added factors of `kind` (GPSLAM_MEAS_*; the calling convention of
 * set_meas_covariance, in either order with it): loss = count x GPSLAM_ROBUST_*, k = count parameters (ignored where the loss is
 * NONE).  GPSLAM_MEAS_AHRS is refused (GPSLAM_E_UNSUPPORTED).  The handle needs a new compile(); marginals held from before are stale. */
int gpslam_hip_set_meas_robust(gpslam_hip_handle *h, int32_t kind, int32_t count, const int32_t *loss, const double *k);
/* the same for the `count` most recently added loop closures (the non-adjacent pairs of add_between_pairs).  Adjacent pairs are chain
 * factors (add_between) and take no loss, like the GP priors and the pose / velocity priors. */
int gpslam_hip_set_between_pairs_robust(gpslam_hip_handle *h, int32_t count, const int32_t *loss, const double *k);
/* the weights w(r) at the current states, in the order the factors were added (1 for a factor without a loss): what a caller reads
 * after optimize() to see which measurements were rejected.  One error-only pass each.  w: count of the kind / of the closures.
 * Returns the count. */
int gpslam_hip_get_meas_weights(gpslam_hip_handle *h, int32_t kind, double *w);
int gpslam_hip_get_between_pairs_weights(gpslam_hip_handle *h, double *w);
/* w(r) and rho(r) of one loss, host arithmetic only, no handle: the inline functions the kernels include (gpslam_amd/csrc/robust.hpp).
 * r >= 0 and finite; NONE gives 1 and r^2 / 2. */
int gpslam_hip_robust_eval(int32_t loss, double k, double r, double *w, double *rho);

/* ---- fixed-lag smoothing (added without an ABI bump: a binding detects these entry points by their presence) ----
 * The reference's method is incremental GP regression; these calls let a handle slide along a live trajectory instead of growing for
 * ever: the old states are eliminated at the current linearisation and the Gaussian they leave on the oldest kept state stays in the
 * graph, as gtsam::BatchFixedLagSmoother does it with a gtsam::LinearContainerFactor (gtsam_unstable/nonlinear/BatchFixedLagSmoother.h,
 * gtsam/nonlinear/LinearContainerFactor.h; third party).  All of them want an fp64 handle that is single (not sharded, not a piece of
 * a split chain) and off the segmented landmark path: GPSLAM_E_UNSUPPORTED with a message otherwise.
 *
 * A joint Gaussian factor on ONE state -- gtsam::LinearContainerFactor over the keys (x_i, v_i).  Per factor: a linearisation point
 * (pose_lin in the layout of set_states, vel_lin d doubles), A (b x b row-major, b = 2d; any finite matrix, zero rows allowed) and
 * c (b); a value that is not finite in any of the four: GPSLAM_E_INVALID.  With xi = [Local(pose_lin, pose_i) ; vel_i - vel_lin] in the handle's chart (GPSLAM_VELOCITY_WORLD_VW: the plain
 * difference of the stored [v; w]) the whitened residual is r = A xi - c and the cost |r|^2 / 2.  The Jacobian is the CONSTANT A on
 * state i's columns [pose tangent | velocity] -- what LinearContainerFactor::linearize does: exact at xi = 0, first order away from
 * it (the derivative of Local is taken as the identity).  b full-width rows [A | 0] on left state i, behind the velocity priors'
 * (gpslam_hip_get_rows lists them there; a graph without such a factor keeps its order); i = N - 1 is allowed.  Gauss-Newton,
 * Levenberg-Marquardt, optimize, error, normal_equations and marginals include them; clear_factors drops them.  compile() answers
 * GPSLAM_E_UNSUPPORTED on a GPSLAM_ROT3_BIAS handle that carries one. */
int gpslam_hip_add_state_gaussians(gpslam_hip_handle *h, int32_t count, const int32_t *idx, const double *pose_lin, const double *vel_lin,
                                   const double *A, const double *c);
/* the stored factors in the order they stand (any pointer may be NULL); returns the count */
int gpslam_hip_get_state_gaussians(gpslam_hip_handle *h, int32_t *idx, double *pose_lin, double *vel_lin, double *A, double *c);
/* Marginalise the head: states 0 .. k - 1 (1 <= k <= N - 1) of a compiled handle.  The head is every stored factor that touches a
 * state < k: GP priors, between factors, odometry and two-state measurement factors with left < k; unary factors and single-state
 * measurements with idx < k; state Gaussians with idx < k (the previous head prior among them).  A factor on state k alone or on
 * the interval (k, k + 1) is not in it.  With q(delta_0 .. delta_k) = |J_h delta + r_h|^2 / 2 the head's whitened linearisation at
 * the current states (lambda = 0 and the robust weights, as gpslam_hip_marginals linearises),
 *     min over delta_0 .. delta_{k-1} of q  =  delta_k^T Lambda delta_k / 2 + gamma^T delta_k + const
 * is computed on the device (a pending update of run_gn is applied first).  Then the handle holds a state Gaussian on the new state 0
 * with the current (pose_k, vel_k) as linearisation point, A^T A = Lambda and A^T c = -gamma; states 0 .. k - 1 and every head
 * factor are gone, the remaining state indices are k lower (landmark indices stay), N is N - k, and the handle needs compile():
 * until then the iteration calls answer GPSLAM_E_NOT_COMPILED; marginals held from before are stale.  The constant of the minimum is
 * dropped, as GTSAM's elimination drops it: gpslam_hip_error is lower afterwards.  Lambda is symmetrised and factorised by Cholesky
 * with diagonal pivoting; pivots below b * eps * max|diag| of the head's own share of block k (before the subtraction) become zero
 * rows of A, so a head without absolute information (Lambda ~ 0) works.
 * Refusals, all before anything changes (the handle then iterates exactly as if the call had not been made): k out of range
 * GPSLAM_E_INVALID; not compiled GPSLAM_E_NOT_COMPILED; GPSLAM_E_UNSUPPORTED for a head factor that names a landmark (the message
 * names kind and factor), for a loop closure with first < k or second < k, and on fp32 / sharded / split / segmented /
 * GPSLAM_ROT3_BIAS handles.  GPSLAM_E_NOT_SPD when a pivot block of the head is not positive definite.
 * The refusal of head factors that name a landmark is the default; gpslam_hip_marginalize_head_onto_landmarks (below) lifts it: the
 * prior then spans the oldest kept state and the landmarks. */
int gpslam_hip_marginalize_head(gpslam_hip_handle *h, int32_t k);
/* linearisation point, Lambda (b x b) and gamma (b) of the last successful marginalize_head, as the device computed them (any
 * pointer may be NULL); GPSLAM_E_INVALID before the first one */
int gpslam_hip_get_head_prior(gpslam_hip_handle *h, double *pose_lin, double *vel_lin, double *Lambda, double *gamma);
/* n more states behind the last one (layouts of set_states), placed on the device; the factors stay; the handle needs compile() */
int gpslam_hip_append_states(gpslam_hip_handle *h, int32_t n, const double *pose, const double *vel);

/* ---- fixed-lag smoothing with landmarks: the head's prior over the oldest kept state AND the landmarks ----
 * What gtsam::BatchFixedLagSmoother leaves on a range / bearing-range / projection graph: a gtsam::LinearContainerFactor over the
 * keys (x_k, v_k, l_0 .. l_{L-1}).  fp64 only, one unsharded handle on the DENSE landmark border (nl = L * landmark_dim <= 27).
 *
 * A joint Gaussian factor on ONE state and ALL landmarks of the handle.  n = b + nl; per factor a linearisation point (pose_lin,
 * vel_lin as for the state Gaussians, lm_lin nl doubles: the landmarks in index order), A (n x n row-major; any finite matrix, zero
 * rows allowed) and c (n); lm_lin is count x nl.  With xi = [Local(pose_lin, pose_i) ; vel_i - vel_lin ; l - lm_lin] (the landmarks'
 * plain difference) the whitened residual is r = A xi - c, the cost |r|^2 / 2, the Jacobian the CONSTANT A: exact at xi = 0, first
 * order away from it, as documented for the state Gaussians.  A value that is not finite in any array: GPSLAM_E_INVALID; a handle
 * without landmarks: GPSLAM_E_INVALID.  compile() answers GPSLAM_E_INVALID when a stored factor's nl no longer matches the handle's
 * (set_landmarks changed L) and GPSLAM_E_UNSUPPORTED, each with a message, on fp32, sharded, split, segmented and GPSLAM_ROT3_BIAS
 * handles, and together with loop closures in column passes (gpslam_hip_set_closure_passes with more than one pass).  Gauss-Newton, Levenberg-Marquardt, optimize, error, normal_equations (the factor's share of D_i, g_i, B_i) and marginals
 * include it; clear_factors drops it.  The factor has NO rows in gpslam_hip_get_rows: a row of the tables names one landmark, this
 * factor names all of them -- its blocks A_x^T A_x, A_x^T (c - A xi), A_x^T A_L go into record i behind the assembly, and
 * A_L^T A_L, A_L^T (c - A xi) and the cross term with the chain's solution into the landmark system behind its reduction. */
int gpslam_hip_add_border_gaussians(gpslam_hip_handle *h, int32_t count, const int32_t *idx, const double *pose_lin, const double *vel_lin,
                                    const double *lm_lin, const double *A, const double *c);
/* the stored factors in the order they stand (any pointer may be NULL); returns the count.  The arrays hold n = b + nl of the STORED
 * factors: when set_landmarks has changed the handle's nl since, a call with lm_lin, A or c answers GPSLAM_E_INVALID and writes nothing */
int gpslam_hip_get_border_gaussians(gpslam_hip_handle *h, int32_t *idx, double *pose_lin, double *vel_lin, double *lm_lin, double *A, double *c);
/* enable != 0: gpslam_hip_marginalize_head accepts head factors that name landmarks, and border Gaussians with idx < k (the previous
 * head prior among them).  On a handle with landmarks it then leaves a BORDER Gaussian on the new state 0 -- linearisation point the
 * current (pose_k, vel_k, landmarks), A^T A = Lambda, A^T c = -gamma with Lambda, gamma over (delta_k, delta_l) from the recursion
 * of k_head_schur_border; pivots at or below n * eps * max|diag| of the head's own share of [D_k^left ; H_LL^head] become zero rows
 * of A (Lambda is rank-deficient as a rule: landmarks the head never saw have zero rows, a range-only head has a gauge).  On a handle
 * without landmarks it leaves the state Gaussian, exactly as with the option off.  The head is every stored factor that touches a
 * state < k; landmark priors touch no state and stay in the graph, landmark indices stay, and a landmark no tail factor sees stays
 * too, determined by the prior.  Every other refusal of gpslam_hip_marginalize_head stays, made before anything changes.  Default 0:
 * the refusal of such head factors, message unchanged (a border Gaussian with idx < k is then refused likewise).  Two more cases:
 * a handle whose closures go in column passes answers GPSLAM_E_UNSUPPORTED (compile() would refuse the factor it leaves); a handle of
 * block size 4 (GPSLAM_LINEAR2: no factor of that manifold names a landmark) keeps leaving the state Gaussian, which is the whole marginal. */
int gpslam_hip_marginalize_head_onto_landmarks(gpslam_hip_handle *h, int32_t enable);
/* lm_lin (nl), Lambda (n x n) and gamma (n), n = b + nl, of the last marginalize_head if it was one onto the landmarks, as the device
 * computed them (any pointer may be NULL); GPSLAM_E_INVALID otherwise, and when set_landmarks has changed the handle's nl since.  gpslam_hip_get_head_prior then returns the state block
 * Lambda_xx and gamma_x: its sizes never change. */
int gpslam_hip_get_head_prior_border(gpslam_hip_handle *h, double *lm_lin, double *Lambda, double *gamma);

/* drop every factor added so far (states, landmarks and Qc stay); the handle needs a new compile() */
int gpslam_hip_clear_factors(gpslam_hip_handle *h);

/* Graph compile: classify, sort by left state, pack SoA parameter arrays, size the solver hierarchy.
 * Must be called after the last add_* / set_states and before any of the calls below.  Every stored factor index is
 * re-validated against the CURRENT number of states / landmarks (GPSLAM_E_INVALID if set_states / set_landmarks
 * shrank the problem under factors that still refer to the removed variables). */
int gpslam_hip_compile(gpslam_hip_handle *h);

/* ---- the hot path ---- */
/* Batched evaluateError + H1..H4 of every GP prior, in the order they were added (unwhitened, exactly what
 * NoiseModelFactor::unwhitenedError returns): errors count x 2d; jacobians count x 4 x 2d x d row-major
 * (may be NULL).  Returns the factor count. */
int gpslam_hip_linearize_gp(gpslam_hip_handle *h, double *errors, double *jacobians);
/* The same for the measurement factors of one kind (kind = GPSLAM_MEAS_*), in the order they were added: errors
 * count x rows (unwhitened evaluateError), jacobians count x rows x (4d + 3) = per row [H1 (d) | H2 (d) | H3 (d) | H4 (d) |
 * H5 (landmark, zero padded to 3)] (may be NULL); single-state factors leave H3 / H4 zero, factors without a landmark H5
 * (e.g. gpslam/slam/GPInterpolatedRangeFactorPose3.h:64-98, GPInterpolatedAttitudeFactorRot3.h:61-83).  Returns the count. */
enum { GPSLAM_MEAS_INTERP_RANGE = 0, GPSLAM_MEAS_RANGE = 1, GPSLAM_MEAS_INTERP_ATTITUDE = 2, GPSLAM_MEAS_INTERP_GPS = 3,
       GPSLAM_MEAS_ODOMETRY2D = 4, GPSLAM_MEAS_BEARING_RANGE = 5, GPSLAM_MEAS_INTERP_PROJECTION = 6, GPSLAM_MEAS_AHRS = 7 };
int gpslam_hip_linearize_meas(gpslam_hip_handle *h, int32_t kind, double *errors, double *jacobians);
/* total graph error 0.5 * sum |R e|^2 (NonlinearFactorGraph::error) */
int gpslam_hip_error(gpslam_hip_handle *h, double *err);
/* one GaussNewtonOptimizer::iterate(): linearize, assemble, solve, retract, error */
int gpslam_hip_iterate_gn(gpslam_hip_handle *h, gpslam_hip_stats *st);
/* one LevenbergMarquardtOptimizer::iterate() */
int gpslam_hip_iterate_lm(gpslam_hip_handle *h, double *lambda, const gpslam_hip_params *p, gpslam_hip_stats *st);
/* The decision of ONE lambda trial of LevenbergMarquardtOptimizer::iterate() (GTSAM 4.0.x tryLambda, third party, as recalled --
 * parity unpinned; the reference's call sites: matlab/PlazaPose2.m:210-226, matlab/GPAHRSexample.m:259-264), host arithmetic
 * only, no handle.  s6 = {error at the linearisation point, error after the trial step, |delta|_inf, delta . g, |delta|^2,
 * indefinite flag} (lm_trial_phase2's out6 after the reduction over ranks; iterate_lm's own scalars).
 *   rho = (s6[0] - s6[1]) / (0.5 delta.g + 0.5 lambda |delta|^2) > minModelFidelity: *accepted = 1, lambda /= lambdaFactor
 *       (not below lambdaLowerBound), *done = 1;
 *   otherwise, |s6[0] - s6[1]| < relativeErrorTol * s6[0]:  *accepted = 0, *done = 1, lambda untouched ("relative cost
 *       reduction is small": the search for a lambda ends, the values stay);
 *   otherwise lambda *= lambdaFactor, *accepted = 0, *done = (lambda >= lambdaUpperBound).
 * A caller that owns the loop (sharded / split handles) calls lm_reject whenever *accepted == 0 and tries again while
 * *done == 0.  gpslam_hip_iterate_lm takes its branches here as well. */
int gpslam_hip_lm_decide(const double *s6, const gpslam_hip_params *p, double *lambda, int32_t *accepted, int32_t *done);
/* NonlinearOptimizer::optimize() with GTSAM's stop rules (+ optional |delta|_inf rule) */
int gpslam_hip_optimize(gpslam_hip_handle *h, const gpslam_hip_params *p, gpslam_hip_stats *st);

/* ---- inspection (parity tests, profiling) ---- */
/* normal equations of the current linearisation: D (N x b x b), O (N x b x b), g (N x b), b = 2d;
 * with landmarks also B (N x b x nl), nl = L * landmark_dim.  Any pointer may be NULL. */
int gpslam_hip_normal_equations(gpslam_hip_handle *h, double *D, double *O, double *g, double *B);
/* whitened Jacobian rows of the current linearisation (what NoiseModelFactor::linearize produces after
 * WhitenSystem): rowLR M x 4d = [d/dx_left | d/dx_right], rowE M, rowM M x landmark_dim, rowLm M (landmark id or -1).
 * Row order: first the rows with velocity columns, grouped by left state (inside a state: GP priors, velocity priors, state Gaussians,
 * then interpolated range, range, attitude, GPS, odometry2d, bearing-range, projection, each in the order they were
 * added); then the velocity-free rows (pose priors, between factors; the device keeps them in a half-width table),
 * again grouped by left state, expanded to full width.  Any output pointer may be NULL; n_rows receives M.  Border Gaussians
 * (gpslam_hip_add_border_gaussians) have no rows here: a row names one landmark, they name all of them. */
int gpslam_hip_get_rows(gpslam_hip_handle *h, int32_t *n_rows, double *rowLR, double *rowE, double *rowM,
                        int32_t *rowLm);
/* solve the block-tridiagonal SPD system D/O/g (host arrays as above, N x b) with the device solver; x: N x b */
int gpslam_hip_block_tridiag_solve(gpslam_hip_handle *h, int32_t N, const double *D, const double *O,
                                   const double *g, double *x);
/* Batched GaussianProcessInterpolator{Linear<D>,Pose2,Pose3,Rot3}::interpolatePose (gpslam.h:57-86; e.g.
 * gpslam/gp/GaussianProcessInterpolatorPose3.h:57-105 without the Jacobians): the pose of the current estimate at
 * time tau[q] after state left[q], inside the interval (left[q], left[q] + 1) of duration dt[q], with the handle's
 * Qc.  out_pose: count x pose_dim, rows in the layout of gpslam_hip_get_states.  Dense trajectory output after
 * an optimisation is the use the MATLAB wrapper exports the interpolators for. */
int gpslam_hip_interpolate_poses(gpslam_hip_handle *h, int32_t count, const int32_t *left, const double *dt,
                                 const double *tau, double *out_pose);
/* ... with the Jacobians of the interpolated pose with respect to (pose_left, vel_left, pose_right, vel_right):
 * out_H count x 4 x d x d = H1..H4 of interpolatePose (gpslam/gp/GaussianProcessInterpolatorPose3.h:82-98, gpslam.h:57-86) */
int gpslam_hip_interpolate_poses_jac(gpslam_hip_handle *h, int32_t count, const int32_t *left, const double *dt,
                                     const double *tau, double *out_pose, double *out_H);
/* ---- posterior covariances (ABI 2.3) ----
 * gtsam::Marginals(graph, values) at the current states and landmarks (GTSAM 4.0 gtsam/nonlinear/Marginals.h): H = J^T J of the whole
 * whitened graph -- chain factors, measurement factors, landmark priors, loop closures; no Levenberg-Marquardt damping -- in the
 * columns of gpslam_hip_normal_equations (state i: [pose tangent (d) | velocity (d)], b = 2d, in the handle's chart; then the
 * landmarks, landmark_dim each), and the blocks of Sigma = H^-1 that the chain's structure makes cheap:
 *   S[i]       b x b   Sigma_{i,i}                  (Marginals::marginalCovariance of x_i / v_i: its diagonal blocks)
 *   S_next[i]  b x b   Sigma_{i,i+1} (rows: state i; the last state's block is zero)   (jointMarginalCovariance({x_i, x_i+1}))
 *   S_lm       nl x nl Sigma_{L,L}, every landmark coordinate jointly, nl = L * landmark_dim
 *   S_x_lm[i]  b x nl  Sigma_{i,L}
 * The three pad coordinates of GPSLAM_ROT3_BIAS's velocity slot report zero rows and columns; the VW family reports its velocity
 * slot as stored, [v; w].  Computed on the device (selected inversion of the block-tridiagonal chain, landmarks and closures as a
 * low-rank term) and kept there.  GPSLAM_E_UNSUPPORTED on fp32 handles, sharded handles, split pieces and the segmented landmark
 * path (unless gpslam_hip_marginals_on_segments asks for it); GPSLAM_E_NOT_SPD when H is indeterminate (e.g. nothing anchors the chain), as iterate_gn. */
int gpslam_hip_marginals(gpslam_hip_handle *h);
/* Marginals on a handle whose closures go through the solver in column passes (gpslam_hip_set_closure_passes, P > 1).  There only
 * one slice of Z = A^-1 U^T (A the chain part of H, U the nc = closures * d whitened closure rows) exists at a time, and
 * gpslam_hip_marginals refuses.  enable != 0 lets it run: it then keeps Z at every state in one more device buffer of
 *     (ceil(N * b / 48) * 48 + 16) * (ceil(nc / 16) * 16) doubles  ~  N * nc * b * 8 bytes
 * (1.15 GB at 1e5 Pose3 states with 20 closures; allocated inside gpslam_hip_marginals, freed by enable == 0 and by destroy) and
 * forms Sigma_xx = A^-1 + W S^-1 W^T - Z M^-1 Z^T, M = I + 1/2 (U Z + (U Z)^T), with the closure term on the fp64 matrix cores
 * (marginals.hip: k_mg_clo_inverse, k_mg_clo_finish).  Callable any time after create, no new compile() is needed; marginals held
 * from before are stale.  enable == 0 (the default) restores the refusal.  On a handle with P <= 1 the call is accepted and
 * changes nothing.  GPSLAM_E_INVALID on a NULL handle.  The fp32, sharded, split and segmented refusals stay. */
int gpslam_hip_marginals_keep_closure_columns(gpslam_hip_handle *h, int32_t enable);
/* Marginals on the segmented landmark path (nested dissection with fat separators: the only path that holds more than 13 planar
 * landmarks).  gpslam_hip_marginals refuses there by default.  enable != 0 lets it run: a solve's forward half at lambda = 0, then the
 * selected inversion back through the fat chain and along every segment (marginals_fs.hip).  It keeps, until enable == 0 or destroy,
 *     G = A_s^-1 H[I_s, B_s] at every interior state:  (N * b + 64) * NCP doubles  ~  N * b * NCP * 8 bytes,  NCP = 2 NB + 1 rounded up to 16
 * (NB: the fat block size of gpslam_hip_segment_plan; about 3 GB at 1e6 SE(2) states with NB = 28) -- the state-landmark getter
 * needs it -- and Sigma_{k,k}, Sigma_{k,k+1} of the fat blocks (about 3 K NB^2 doubles).  Fat blocks up to NB = 64 columns; wider ones
 * answer GPSLAM_E_UNSUPPORTED (the message names NB and the limit).  Callable any time after create, no new compile() is needed;
 * marginals held from before are stale.  enable == 0 (the default) restores the refusal and frees the buffers.  On a handle that is
 * not segmented the call is accepted and changes nothing.  The fp32, sharded and split refusals stay.  Iterations after a
 * gpslam_hip_marginals call are bit-identical to those of a handle that never made it.  GPSLAM_E_INVALID on a NULL handle. */
int gpslam_hip_marginals_on_segments(gpslam_hip_handle *h, int32_t enable);
/* copies the window [first, first + count) of S / S_next / S_x_lm (count x b x b, count x b x b, count x b x nl), and S_lm; any pointer
 * may be NULL.  GPSLAM_E_INVALID ("stale") before gpslam_hip_marginals, or after any call that can change states, landmarks,
 * factors or Qc since: set_states, set_landmarks, set_qc, add_*, set_meas_covariance, set_*_robust, clear_factors, compile, iterate_gn, iterate_lm,
 * run_gn, optimize. */
int gpslam_hip_get_marginals(gpslam_hip_handle *h, int32_t first, int32_t count, double *S, double *S_next, double *S_lm,
                             double *S_x_lm);
/* On a segmented handle S_lm / S_x_lm do not exist (nl x nl and N b x nl: 80 GB at 1e5 landmark coordinates): a non-NULL S_lm or
 * S_x_lm answers GPSLAM_E_UNSUPPORTED there, S and S_next work as everywhere.  The landmark blocks come from three getters that
 * gather on the device what they are asked for; same refusals and staleness rule as gpslam_hip_get_marginals, and they serve dense-border
 * handles as well (from S_lm / S_x_lm):
 *   get_landmark_marginals        out count x ld x ld: Sigma_{l,l} of the landmarks first .. first + count - 1
 *   get_state_landmark_marginals  out count x b x ld:  Sigma_{state[t], landmark[t]}.  Segmented: the landmark must sit in a fat block
 *                                 next to the state's segment (for a cut state: its own block or a neighbouring one) -- by the
 *                                 attachment rule that covers every landmark the state observes; dense border: any pair
 *   get_landmark_pair_marginals   out count x ld x ld: Sigma_{a[t], b[t]}.  Segmented: both in the same or in neighbouring fat blocks
 * GPSLAM_E_INVALID (the message names the first such item) for a pair that cannot be served or an index out of range. */
int gpslam_hip_get_landmark_marginals(gpslam_hip_handle *h, int32_t first, int32_t count, double *out);
int gpslam_hip_get_state_landmark_marginals(gpslam_hip_handle *h, int32_t count, const int32_t *state, const int32_t *landmark, double *out);
int gpslam_hip_get_landmark_pair_marginals(gpslam_hip_handle *h, int32_t count, const int32_t *a, const int32_t *b, double *out);
/* Sigma_{a,b} of ANY two states (Marginals::jointMarginalCovariance over states that are far apart on the chain; the covariance a
 * chi-square gate of a loop-closure candidate needs).  Sigma_xx = A^-1 + (low-rank term), A the block-tridiagonal chain part: A^-1_{a,b}
 * comes from the factorisation the selected inversion leaves on the device (marginals_pairs.hip: k_mg_pair, a few hundred b x b
 * products per pair at 1e6 states, whatever |a - b|), the low-rank term from Y = [W | Z] of the two states.  Y lives in a solver buffer
 * that later calls (normal_equations, get_rows, error, linearize_*, interpolate_*) rewrite, so on a handle with landmarks or closures
 * the pair getters need enable != 0 BEFORE gpslam_hip_marginals, which then copies it into one more device buffer of
 *     N * b * m doubles,  m = nl + closures * d  (column passes: m = nl; Z is what gpslam_hip_marginals_keep_closure_columns keeps)
 * (259 MB at 1e5 Pose3 states with 7 landmarks of dimension 3 and one closure, m = 27, the widest border; allocated
 * inside gpslam_hip_marginals, freed by enable == 0 and by destroy).  A handle with m = 0 needs no copy: there the getters work
 * without this call.  Callable any time after create, no new compile() is needed; marginals held from before are stale.
 * Iterations and every output of gpslam_hip_get_marginals are bit-identical with and without it.  GPSLAM_E_INVALID on a NULL handle. */
int gpslam_hip_marginals_keep_pair_terms(gpslam_hip_handle *h, int32_t enable);
/* out: count x b x b, block t = Sigma_{a[t], b[t]} (rows: state a[t]) in the columns of gpslam_hip_normal_equations; the pad
 * coordinates of GPSLAM_ROT3_BIAS report zero rows and columns.  a == b is S[a] and |a - b| == 1 is S_next (transposed when a > b)
 * of gpslam_hip_get_marginals, to the bit; every other pair is computed for (min, max) and transposed on output, so that
 * Sigma_{b,a} = Sigma_{a,b}^T to the bit.  No atomics, fixed order: reruns are bit-identical.  Same refusals and staleness rule as
 * gpslam_hip_get_marginals; in addition GPSLAM_E_UNSUPPORTED on the segmented landmark path (even with
 * gpslam_hip_marginals_on_segments), GPSLAM_E_INVALID on a handle with landmarks or closures whose last gpslam_hip_marginals ran
 * without gpslam_hip_marginals_keep_pair_terms, and for an index out of range (the message names the first such item). */
int gpslam_hip_get_state_pair_marginals(gpslam_hip_handle *h, int32_t count, const int32_t *a, const int32_t *b, double *out);
/* The chi-square gate of loop-closure candidates that are NOT in the graph, in the argument layout of gpslam_hip_add_between_pairs
 * (measured count x pose_dim, sigmas count x d), at the current states and the held marginals:
 *   err        count x d      (may be NULL) the unwhitened BetweenFactor error e
 *   innov_cov  count x d x d  (may be NULL) P = diag(sigma^2) + [H1 H2] Sigma^{pp}_{(first, second)} [H1 H2]^T, pp: the pose-tangent blocks
 *   chi2       count          e^T P^-1 e by a d x d Cholesky; GPSLAM_E_NOT_SPD on a non-positive pivot
 * first == second answers GPSLAM_E_INVALID; adjacent states are allowed.  Refusals and staleness as gpslam_hip_get_state_pair_marginals. */
int gpslam_hip_gate_between_pairs(gpslam_hip_handle *h, int32_t count, const int32_t *first, const int32_t *second,
                                  const double *measured, const double *sigmas, double *chi2, double *err, double *innov_cov);
/* Posterior covariance (count x d x d) of the GP-interpolated pose at tau[q] in (left[q], left[q] + 1), batched like
 * interpolate_poses -- the covariance half of the sparse-GP interpolation (Barfoot, Tong & Sarkka, RSS 2014), which GTSAM has no
 * call for:  P(tau) = H_J Sigma_J H_J^T + gp_term * c(dt, tau) * Qc,  H_J = [H1 H2 H3 H4] of interpolate_poses_jac,
 * Sigma_J = [[S[i], S_next[i]], [S_next[i]^T, S[i+1]]],  c = tau^3 (dt - tau)^3 / (3 dt^3): c Qc is the pose block of the GP's
 * conditional covariance Q(tau) - Psi Phi(dt - tau) Q(tau) (gpslam/gp/GPutils.h:24-71) for the handle's Qc (GPSLAM_ROT3_BIAS: on
 * the rotation; the bias is held over the interval).  Exact on GPSLAM_LINEAR2 / GPSLAM_LINEAR3 with gp_term = 1; on the Lie groups
 * first order in the local variable.  Same refusals and staleness rule as gpslam_hip_get_marginals. */
int gpslam_hip_interpolate_covariances(gpslam_hip_handle *h, int32_t count, const int32_t *left, const double *dt,
                                       const double *tau, int32_t gp_term, double *out_cov);
/* GaussianProcessInterpolatorLinear<D>::interpolateVelocity (gpslam.h:193, gpslam/gp/GaussianProcessInterpolatorLinear.h:106-126)
 * of the current estimate, batched like interpolate_poses: out_vel count x d; out_H (may be NULL) count x 4 x d x d = H1..H4
 * (:117-120, the lower blocks of Lambda and Psi).  GPSLAM_LINEAR2 / GPSLAM_LINEAR3 handles; the reference declares the method
 * for its Lie-group interpolators without implementing it (GaussianProcessInterpolatorPose3.h:118-123): GPSLAM_E_UNSUPPORTED. */
int gpslam_hip_interpolate_velocities(gpslam_hip_handle *h, int32_t count, const int32_t *left, const double *dt,
                                      const double *tau, double *out_vel, double *out_H);
/* getBodyCentricVb / getBodyCentricVs (gpslam.h:161-164, gpslam/gp/Pose3utils.cpp:17-24), batched: the MATLAB scripts
 * initialise the velocity of every state with them.  which = 0: Vb = Logmap(pose1^-1 pose2) / dt, 1: Vs = Logmap(pose2
 * pose1^-1) / dt;  pose1, pose2: count x 12 (R row-major, t), dt: count, out: count x 6 (omega, v).  Any handle: its device
 * and stream are used, its graph is not touched. */
int gpslam_hip_body_centric_velocity(gpslam_hip_handle *h, int32_t which, int32_t count, const double *pose1,
                                     const double *pose2, const double *dt, double *out);
/* What compile() chose for the chain solver (introspection for tests and tuning; no reference counterpart):
 * out8 = {levels of the hierarchy, level-0 chunk length, upper chunk length, assembly fused into the level-0 elimination
 * (k_fused_level0) 0/1, GP priors handed to the assembly as structured records instead of Jacobian rows 0/1 (SE(3): inside the fused
 * kernel; SE(2) / SO(3) / 3-D linear: where k_assemble_ghost runs; 2: SE(3) records AND the interpolated GPS factors' rows as
 * 16-double lines whose right halves the assembly wave forms from the interval's record -- round 5), rows in the
 * full-width table, rows in the compact table, right-hand-side columns R}. */
int gpslam_hip_plan_info(gpslam_hip_handle *h, int32_t out8[8]);
/* What the launchers of this handle DID since the last reset (introspection for tests; no reference counterpart).  plan_info above
 * is computed from the plan; these are host-side integers the launchers write at their launch statements, each from the branch it
 * took, so a handle that quietly takes another form than the plan promises shows here.  Recording costs a few integer stores per
 * launch: no device work, no synchronisation, no allocation.  out receives min(n, GPSLAM_CENSUS_N) entries, indexed by
 * GPSLAM_CENSUS_*; reset != 0 clears the counts (and the "last launch" entries to -1) after reading.  Returns GPSLAM_CENSUS_N of
 * the library, or an error code.  Counts cover the iteration launchers (linearisation, level 0, the levels above, back-substitution,
 * retraction) from whichever call reached them. */
enum {
  /* level-0 forward elimination, launches per family */
  GPSLAM_CENSUS_L0_FUSED = 0,       /* k_fused_level0 */
  GPSLAM_CENSUS_L0_ROWS,            /* k_chunk_forward_rows */
  GPSLAM_CENSUS_L0_COLUMN,          /* k_chunk_forward on a level without addends that keeps its separators ... */
  GPSLAM_CENSUS_L0_COLUMN_FAST,     /* ... of which the variant with the separator sums in spare lanes */
  GPSLAM_CENSUS_TOP_CHUNK,          /* k_chunk_forward as the sequential top solve of blocks without addends (a chain of a single level,
                                     * the reduced system of a sharded solve, gpslam_hip_block_tridiag_solve) */
  /* the LAST k_fused_level0 launch (-1: none since the reset): its instantiation <SV, TR, B, DG> ... */
  GPSLAM_CENSUS_FUSED_SV,
  GPSLAM_CENSUS_FUSED_DG,
  GPSLAM_CENSUS_FUSED_B,
  GPSLAM_CENSUS_FUSED_FP32,         /* TR: 0 double, 1 float */
  GPSLAM_CENSUS_FUSED_GSAVE,        /* the gradient was stored (a Levenberg-Marquardt trial) */
  /* ... and its inputs as passed */
  GPSLAM_CENSUS_FUSED_GP,           /* GP priors consumed as 0 rows, 1 d = 3 records, 2 SE(3) records */
  GPSLAM_CENSUS_FUSED_BTW_REC,      /* between records attached */
  GPSLAM_CENSUS_FUSED_LINES,        /* interpolated GPS lines attached */
  GPSLAM_CENSUS_FUSED_ODD_ROWS,     /* FusedArgs::odd_rows */
  GPSLAM_CENSUS_FUSED_TAIL,         /* level 1 reduced in the kernel's tail (FwdArgs::tail) */
  GPSLAM_CENSUS_FUSED_GSAVE_LAUNCHES,   /* k_fused_level0 launches that stored the gradient */
  GPSLAM_CENSUS_FUSED_TAIL_LAUNCHES,    /* k_fused_level0 launches with the tail on */
  /* levels above level 0, forward */
  GPSLAM_CENSUS_UPPER_CR,           /* upper_forward launches (LDS-resident cyclic reduction) */
  GPSLAM_CENSUS_UPPER_CHUNK,        /* k_chunk_forward launches on a level with addends */
  /* back-substitution */
  GPSLAM_CENSUS_BWD_ROWS,           /* k_chunk_backward_rows launches ... */
  GPSLAM_CENSUS_BWD_ROWS_FOLD,      /* ... of which solved their group of four of level 1 themselves (BwdArgs::l1_blk) */
  GPSLAM_CENSUS_BWD_CHUNK,          /* k_chunk_backward launches */
  GPSLAM_CENSUS_UPPER_BWD,          /* upper_backward launches */
  /* K1, Jacobian pass: one counter per k_lin statement */
  GPSLAM_CENSUS_LIN_REC,            /* merged k_lin writing records, no velocity priors */
  GPSLAM_CENSUS_LIN_REC_VP,         /* ... with velocity priors */
  GPSLAM_CENSUS_LIN_ROWS,           /* merged k_lin writing rows, body velocities, no velocity priors */
  GPSLAM_CENSUS_LIN_ROWS_VP,
  GPSLAM_CENSUS_LIN_VW,             /* merged k_lin writing rows, world velocities */
  GPSLAM_CENSUS_LIN_VW_VP,
  GPSLAM_CENSUS_LIN_GROUPS,         /* k_gp launches of the Jacobian pass, one per Qc group */
  GPSLAM_CENSUS_LIN_PEND,           /* k_lin launches that applied a pending update (run_gn's folded retraction) */
  GPSLAM_CENSUS_FLUSH,              /* a pending update met a launch that could not apply it: retracted on the spot */
  /* interpolated GPS, Jacobian pass */
  GPSLAM_CENSUS_GPS_LINES,          /* k_gps_lines launches */
  GPSLAM_CENSUS_MEAS_REC,           /* k_meas launches with the intervals' GP records attached (a factor whose interval has none forms
                                     * its blocks itself inside the kernel: not visible to the host) */
  GPSLAM_CENSUS_MEAS_SELF,          /* k_meas launches without records: every factor forms its blocks itself */
  GPSLAM_CENSUS_RETRACT,            /* k_retract launches over the local states */
  GPSLAM_CENSUS_N
};
int gpslam_hip_launch_census(gpslam_hip_handle *h, int32_t *out, int32_t n, int32_t reset);
/* the plan of the segmented landmark elimination chosen by compile(): out = {active (0 / 1), segment length C, fat
 * blocks K, fat block size NB, border columns NC per segment, NC rounded up to MFMA tiles, cyclic-reduction levels,
 * link blocks} */
int gpslam_hip_segment_plan(gpslam_hip_handle *h, int32_t out8[8]);
/* time (ms) of the last iterate call's phases measured with hipEvents on the handle's stream:
 * out[0] linearize, out[1] assemble, out[2] solve, out[3] retract+error, out[4] total */
int gpslam_hip_last_timing(gpslam_hip_handle *h, double *out5);
/* device time (ms) of the LEVEL-0 FORWARD launch -- on Pose3 chains k_fused_level0, the dominant kernel -- summed over the
 * iterations of the last timed run_gn / iterate_gn: the kernel as it runs INSIDE an iteration (behind the linearisation,
 * caches as an iteration leaves them), which is what bench.py's roofline fraction is computed from (time_kernel's isolated
 * launches are faster).  The fused launch carries its own start / stop events (the dispatch's time stamps, what a profiler's
 * kernel trace reports); the two-launch level 0 is bracketed by events on the stream.  0 on the segmented landmark path. */
int gpslam_hip_last_level0_ms(gpslam_hip_handle *h, double *ms);
/* on = 1: the fused level-0 launch of a TIMED iteration carries its own start / stop events (hipExtLaunchKernelGGL: the dispatch's
 * time stamps -- gpslam_hip_last_level0_ms then reports what a profiler's kernel trace reports, where events recorded around the
 * launch add their marker packets: 149 us for 142).  A stamped dispatch costs the iteration ~10 us elsewhere, so the other phase
 * times of such a run are not to be quoted; off (the default) nothing changes.  ABI 2.2. */
int gpslam_hip_set_level0_stamps(gpslam_hip_handle *h, int32_t on);
/* run `iters` Gauss-Newton iterations back to back with no host synchronisation in between (the benchmark
 * loop); per-phase device time is accumulated in out5 (ms, summed over iters) when out5 != NULL.
 * The error of the state an iteration produces is the error the next iteration's linearisation evaluates, so
 * inside the run it is computed once (by that linearisation) and only the last iteration is followed by an
 * error-only pass; st->error_before / error_after refer to the last iteration. */
int gpslam_hip_run_gn(gpslam_hip_handle *h, int32_t iters, gpslam_hip_stats *st, double *out5);

/* average device time (ms, hipEvents on the handle's stream) of ONE launch of a hot kernel over `reps` launches:
 * which = 0 GP-prior linearisation (K1), 1 normal-equation assembly (K3), 2 level-0 forward elimination (K4),
 * 3 level-0 back-substitution, 4 retract (K6).  Inputs are re-created (untimed) before every timed launch.
 * Pose3 chains without landmarks run the assembly INSIDE the level-0 elimination (k_fused_level0): there
 * which = 1 reports 0.0 (no such launch in an iteration) and which = 2 times the fused kernel. */
int gpslam_hip_time_kernel(gpslam_hip_handle *h, int32_t which, int32_t reps, double *avg_ms);

/* ---- segment sharding (nranks > 1): one exchange per iteration, performed by the host via RCCL ---- */
/* device pointer + size (bytes) of this rank's interface record (written by phase 1) */
int gpslam_hip_interface_send(gpslam_hip_handle *h, void **dev_ptr, size_t *bytes);
/* device pointer + size of the gathered records of all ranks (nranks * bytes; filled by the host's all-gather) */
int gpslam_hip_interface_recv(gpslam_hip_handle *h, void **dev_ptr, size_t *bytes);
/* phase 1: linearize + assemble + local elimination down to the rank separator -> interface record */
int gpslam_hip_iterate_phase1(gpslam_hip_handle *h, double lambda);
/* phase 2 (after the all-gather): reduced solve, back-substitution, retract, local error (st may be NULL: no error
 * pass, no host synchronisation).  Chains with landmarks on more than one rank run it in two halves with one
 * all-reduce (sum) of the landmark buffer in between -- SURVEY.md section 8(e) collective (3):
 *   phase2a: reduced solve + back-substitution + this rank's share of the landmark Schur complement [S | gL]
 *   all-reduce of gpslam_hip_landmark_reduce_buffer (doubles)
 *   phase2b: landmark solve (redundant on every rank), chain correction, retract of states / halo / landmarks */
int gpslam_hip_iterate_phase2(gpslam_hip_handle *h, gpslam_hip_stats *st);
int gpslam_hip_iterate_phase2a(gpslam_hip_handle *h);
int gpslam_hip_iterate_phase2b(gpslam_hip_handle *h, gpslam_hip_stats *st);
int gpslam_hip_landmark_reduce_buffer(gpslam_hip_handle *h, void **dev_ptr, size_t *bytes);
/* LevenbergMarquardtOptimizer::iterate on a sharded chain: the accept / reject decisions need global sums, so the
 * loop is the caller's (gpslam_amd/sharded.py: ShardedSolver.iterate_lm mirrors gpslam_hip_iterate_lm line by line):
 *   lm_begin;  repeat { lm_trial_phase1(lambda); all-gather records; iterate_phase2a; [all-reduce landmark buffer];
 *   lm_trial_phase2(out6); all-reduce out6 (sum of [0], [1], [3], [4]; max of [2], [5]); accept, or lm_reject and a
 *   larger lambda }.  out6 = {error, trial error, |delta|_inf, delta . g, |delta|^2, indefinite flag} of this rank. */
int gpslam_hip_lm_begin(gpslam_hip_handle *h);
int gpslam_hip_lm_trial_phase1(gpslam_hip_handle *h, double lambda);
int gpslam_hip_lm_trial_phase2(gpslam_hip_handle *h, double *out6);
int gpslam_hip_lm_reject(gpslam_hip_handle *h);
/* ---- chains with many locally visible landmarks (the segmented landmark elimination, BASELINE config 4) across GPUs ----
 * The chain is split into P pieces that OVERLAP in one state: piece r holds the states [s_r, s_(r+1)] (both ends included),
 * every factor whose left / only state lies in [s_r, s_(r+1)) (the last piece also those of the final state), and the
 * landmarks its factors touch, in its own numbering.  A landmark seen from both sides of s_(r+1) is listed -- in the same
 * order -- as a `last` landmark of piece r and a `first` landmark of piece r + 1 (its prior, if any, is given to ONE of the
 * two); the shared state and these landmarks form a fat separator both pieces hold, and both apply the same update to it.
 * Handles are created with nranks = 1 (no halo); before compile():  fs_set_split;  after compile(): fs_split_info ->
 * out4 = {this piece's fat block size NB, fat blocks, segment length, nb_top}, then fs_set_top(max of NB over the pieces).
 * One Gauss-Newton iteration:  fs_phase1(lambda)  -> interface record [Dff | H | Dll | g_first | g_last] in `send`
 * (3 nb_top^2 + 2 nb_top doubles);  ONE all-gather of the records into `recv` (piece order);  fs_phase2: every piece solves
 * the (P + 1)-block system of the shared separators redundantly, back-substitutes, retracts its states and landmarks
 * (st: THIS piece's error terms and |delta|_inf; NULL skips the error pass).  GPInterpolatedRangeFactorPose2.h:64-98 over
 * matlab/PlazaPose2.m:147-178's graph, at BASELINE config 4's size on more than one GPU. */
int gpslam_hip_fs_set_split(gpslam_hip_handle *h, int32_t rank, int32_t nranks, const int32_t *first_lm, int32_t n_first,
                            const int32_t *last_lm, int32_t n_last);
int gpslam_hip_fs_split_info(gpslam_hip_handle *h, int32_t out4[4]);
int gpslam_hip_fs_set_top(gpslam_hip_handle *h, int32_t nb_top);
int gpslam_hip_fs_interface(gpslam_hip_handle *h, void **send, size_t *send_bytes, void **recv, size_t *recv_bytes);
int gpslam_hip_fs_phase1(gpslam_hip_handle *h, double lambda);
int gpslam_hip_fs_phase2(gpslam_hip_handle *h, gpslam_hip_stats *st);
/* LevenbergMarquardtOptimizer::iterate on a split chain (matlab/PlazaPose2.m:217-229 optimises this graph with it): the
 * caller's loop, as for nranks > 1 below --  gpslam_hip_lm_begin;  repeat { fs_lm_trial_phase1(lambda); all-gather of the
 * records; fs_lm_trial_phase2(out6); all-reduce of out6 (sum of [0], [1], [3], [4]; max of [2], [5]); accept, or
 * gpslam_hip_lm_reject and a larger lambda }.  out6 as for gpslam_hip_lm_trial_phase2; a shared state / landmark enters
 * |delta|^2 on the piece to its right only, delta . g adds up over the pieces as it is. */
int gpslam_hip_fs_lm_trial_phase1(gpslam_hip_handle *h, double lambda);
int gpslam_hip_fs_lm_trial_phase2(gpslam_hip_handle *h, double *out6);
/* ---- the whole optimiser loop on a sharded handle or a split piece (round 5) ----
 * The library does not link a communication library: the ONE data-path collective of an iteration is the
 * host's to perform.  With the two callbacks below registered, gpslam_hip_iterate_gn / _run_gn / _iterate_lm / _optimize /
 * _error accept handles with nranks > 1 and pieces of a split chain: they run the phases above in order and call
 *   all_gather(user, send_dev, recv_dev, bytes_per_rank, hip_stream)  -- every rank's `bytes_per_rank` bytes at send_dev into
 *       recv_dev, rank order, enqueued on hip_stream (the handle's stream): ncclAllGather(send, recv, bytes, ncclChar, comm, stream)
 *   all_reduce_sum(user, buf_dev, n_doubles, hip_stream)              -- in-place sum of doubles (the landmark Schur complement
 *       of a chain with a dense landmark border; may be NULL for chains without landmarks and for split pieces)
 * and return the statistics of the WHOLE chain (errors summed, |delta|_inf maximised over the ranks), identical on every rank.
 * A callback returns 0, anything else ends the call with GPSLAM_E_COMM.  Collectives per call:
 *   iterate_gn      1 all-gather of the interface records (+ 1 all-reduce with a landmark border) + 1 all-gather of 64 B of scalars
 *                   (with or without statistics: it is also how a rank learns that another one failed);
 *   run_gn(K)       K x (the record all-gather (+ the all-reduce)) + ONE all-gather of 64 B at the end: the statistics of the last
 *                   iteration, the non-positive-pivot flag of ANY iteration (sticky through the run) and the first failure of any rank;
 *   iterate_lm      per lambda trial: the record all-gather (+ the all-reduce) and ONE all-gather of 64 B carrying the trial's six
 *                   scalars {error, trial error, |delta|_inf, delta . g, |delta|^2, indefinite flag} -- the scalars of a trial
 *                   exist only after its back-substitution, which needs the gathered records, so they cannot ride the record;
 *                   every rank then takes the branch of gpslam_hip_lm_decide on identical reduced numbers;
 *   optimize        GTSAM's loop (NonlinearOptimizer::defaultOptimize) over the two above.
 * Every rank must make the same calls in the same order (they are collective).
 * FAILURES ON ONE RANK (round 6).  A rank whose local work fails inside one of these calls -- a HIP error, a phase's status, its own
 * all_reduce_sum callback -- does NOT leave the collective sequence: it records the code, skips its remaining local work, goes on making
 * every collective call of the iteration, and the code travels in a spare slot of the 64-byte scalar gather; EVERY rank then returns
 * that code (a non-positive pivot anywhere: GPSLAM_E_NOT_SPD everywhere, as before).  What can still leave ranks out of step, and is
 * the caller's to prevent or to time out: a rank that never enters the call (GPSLAM_E_NOT_COMPILED, no callbacks registered, a
 * split piece without gpslam_hip_fs_set_top: checked before the first collective), an all_gather callback that fails or hangs on
 * one rank only, and a HIP failure inside the scalar gather's own two 64-byte copies.
 * A single-rank handle that was forced onto the sharded code path (config_v2.force_sharded) needs no callbacks.  LevenbergMarquardtOptimizer::iterate on the reference's
 * landmark graph: matlab/PlazaPose2.m:210-226. */
typedef int (*gpslam_hip_all_gather_fn)(void *user, const void *send_dev, void *recv_dev, size_t bytes_per_rank, void *hip_stream);
typedef int (*gpslam_hip_all_reduce_sum_fn)(void *user, void *buf_dev, size_t n_doubles, void *hip_stream);
int gpslam_hip_set_collectives(gpslam_hip_handle *h, gpslam_hip_all_gather_fn all_gather, gpslam_hip_all_reduce_sum_fn all_reduce_sum,
                               void *user);
/* halo: the first state of the right neighbour (pose_dim + d doubles), kept in sync by the library after init */
int gpslam_hip_set_halo_state(gpslam_hip_handle *h, const double *pose, const double *vel);

#ifdef __cplusplus
}
#endif
#endif /* GPSLAM_HIP_H */
