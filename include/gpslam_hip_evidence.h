/* gpslam_hip_evidence.h -- log det H and the Laplace log-evidence of a gpslam_hip_handle, for choosing Qc.
 *
 * An addition to include/gpslam_hip.h, which it includes; the ABI stays 2.4 and a binding detects these entry points by
 * presence (dlsym), as it does for the dogleg calls.
 *
 * The mathematics.  At the optimum x^ of the nonlinear least-squares problem the Laplace approximation of the marginal
 * likelihood of the data is
 *     log Z = -cost(x^) + sum_f log|det R_f| - 1/2 log det H - ((m - n) / 2) log 2 pi,
 * R_f the whitening matrix of factor f (R_f^T R_f = its inverse covariance), m the number of residual rows, n the number of
 * variables, H = J^T J the whitened system at x^ -- the matrix gpslam_hip_marginals inverts.  On a graph whose factors are all
 * linear the approximation is exact.  GTSAM's GaussianBayesNet::logDeterminant() returns log det R = HALF of log det H.
 *
 * log det H = log det A + log det(I + U Z) + log det S:  A the block-tridiagonal chain part (everything but loop closures and
 * landmark columns), U the closures' whitened rows and Z = A^-1 U^T, S = H_LL - B^T H_xx^-1 B the landmarks' Schur complement.
 * log det A comes from a forward-only chunked block elimination that adds up the logarithms of its Cholesky pivots and keeps
 * nothing per state; the other two from the solver's own right-hand sides, as in gpslam_hip_marginals.
 *
 * Supported by the handle calls: fp64, unsharded handles, without landmarks or with the dense landmark border, loop closures in
 * one pass and in column passes (gpslam_hip_marginals_keep_closure_columns is not needed).  GPSLAM_E_UNSUPPORTED, with a message and
 * before anything is launched: fp32 handles, sharded handles and split pieces, the segmented landmark path, GPSLAM_ROT3_BIAS.
 */
#ifndef GPSLAM_HIP_EVIDENCE_H
#define GPSLAM_HIP_EVIDENCE_H

#include "gpslam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* log det H at the current states and landmarks: lambda = 0, the robust weights as linearised, state and border Gaussians
 * included, a pending run_gn update applied first.  parts3 (may be NULL) = {log det A, log det(I + U Z), log det S}; they sum to
 * *logdet.  GPSLAM_E_NOT_SPD on a non-positive pivot, and on a pivot of the chain's elimination below 2^-36 of the diagonal entry
 * its coordinate has in H (nothing of it is significant; the message says which of the two it was).  The floor also refuses a
 * well-posed graph whose Jacobi-scaled condition number is beyond about 7e10 (2^36), which Gauss-Newton and gpslam_hip_marginals
 * would still take.  The closures' and landmarks' small systems keep the plain test.  Rewrites the solver's buffers: the marginals
 * are stale afterwards; the iterations that follow are what they would have been.  No atomics, fixed summation order: two calls
 * return the same bits. */
int gpslam_hip_log_determinant(gpslam_hip_handle *h, double *logdet, double *parts3);
/* sum_f log|det R_f|, m and n of the stored graph: host arithmetic, nothing is launched.  GP priors -1/2 log det Q(dt) with the
 * factor's own Qc (gpslam_hip_add_gp_priors_qc) or the handle's; diagonal sigmas -sum log sigma; gpslam_hip_set_meas_covariance
 * -1/2 log det cov.  GPSLAM_E_UNSUPPORTED, naming the first offending factor: robust losses, state or border Gaussians, AHRS
 * factors, GPSLAM_ROT3_BIAS.  rows, vars may be NULL */
int gpslam_hip_log_noise_normaliser(gpslam_hip_handle *h, double *lognorm, int64_t *rows, int64_t *vars);
/* out5 = {log Z, cost, log det H, lognorm, m - n} at the current states (optimise first).  The refusals of the two calls above and
 * of gpslam_hip_error, every one made before any device work */
int gpslam_hip_log_evidence(gpslam_hip_handle *h, double *out5);
/* host arithmetic only, no handle: log|det R| of ONE GP prior, -1/2 (d log(dt^4 / 12) + 2 log det Qc); Qc d x d row-major,
 * 1 <= d <= 6.  GPSLAM_E_INVALID on a Qc that is not symmetric positive definite and on dt <= 0 */
int gpslam_hip_gp_log_normaliser(int32_t d, const double *Qc, double dt, double *out);
/* host arithmetic only: *logZ = -cost + lognorm - logdet / 2 - ((rows - vars) / 2) log 2 pi */
int gpslam_hip_evidence_combine(double cost, double logdet, double lognorm, int64_t rows, int64_t vars, double *logZ);

#ifdef __cplusplus
}
#endif
#endif
