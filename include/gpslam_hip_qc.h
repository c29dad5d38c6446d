/* gpslam_hip_qc.h -- learning Qc from data: the statistic the log-evidence's derivative in Qc^-1 needs, that derivative, and the
 * EM update it implies.
 *
 * An addition to include/gpslam_hip.h, which it includes; the ABI stays 2.4 and a binding detects these entry points by
 * presence (dlsym), as it does for the dogleg and the evidence calls.
 *
 * The mathematics.  Write W = Qc^-1.  A GP prior over an interval dt whitens with Q^-1(dt) = T(dt) (x) W,
 *     T = [[12 / dt^3, -6 / dt^2], [-6 / dt^2, 4 / dt]] = K^T K,   K = [[sa, sb], [0, sc]]
 * (sa = sqrt(12 / dt^3), sb = -sqrt(3 / dt), sc = 1 / sqrt(dt): the scalars of the solver's own whitening).  For prior i with the
 * unwhitened error e = [e_t; e_b] and Jacobian J = [J_t; J_b] (each d x 4d, columns [x_i, v_i, x_i+1, v_i+1] in the handle's chart:
 * what gpslam_hip_linearize_gp returns) the time-whitened halves are
 *     e~_1 = sa e_t + sb e_b,  e~_2 = sc e_b,      J~_1 = sa J_t + sb J_b,  J~_2 = sc J_b,
 * and with Sigma_J = [[S[i], S_next[i]], [S_next[i]^T, S[i+1]]] of gpslam_hip_get_marginals the statistic is
 *     A = sum_i sum_{k = 1, 2} ( e~_k e~_k^T + J~_k Sigma_J J~_k^T )        (d x d, symmetric),     n_f = the number of priors summed.
 * Let F(x, W) = -cost + sum_f log|det R_f| - 1/2 log det H at FIXED states x.  Then dF = tr(G dW) for symmetric dW with
 *     G = n_f Qc - 1/2 A:
 * the cost gives -1/2 sum e~ e~^T, -1/2 tr(H^-1 dH/dW) gives -1/2 sum J~ Sigma_J J~^T, the normaliser n_f log det W gives n_f Qc.
 * On a graph of linear factors at its optimum G is the total derivative of the log-evidence log Z (the states' own dependence on W
 * drops out at a stationary point of the cost, and H does not depend on the states); on a nonlinear graph it leaves out the
 * implicit term -1/2 tr(H^-1 dH/dx^ dx^/dW).  G = 0 is the M-step of expectation-maximisation for the GP's power spectral density
 * (Barfoot, State Estimation for Robotics; Wong, Yoon, Schoellig, Barfoot, RA-L 2020):
 *     Qc+ = A / (2 n_f),          and for the one-parameter family Qc = theta Qc0:    theta+ = tr(Qc0^-1 A) / (2 n_f d).
 * The interpolated measurement factors do not depend on Qc (gpslam_hip.h, the note at gpslam_hip_add_gp_priors_qc): the GP priors
 * are the only factors that enter.
 */
#ifndef GPSLAM_HIP_QC_H
#define GPSLAM_HIP_QC_H

#include "gpslam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A (d x d, row-major, symmetric to the bit) and n_f over the GP priors that carry the handle's shared Qc (gpslam_hip_add_gp_priors);
 * priors added through gpslam_hip_add_gp_priors_qc keep their own Qc, are constants here, and are neither summed nor counted.
 * n_f = 0 and A = 0 when no prior carries the shared Qc.  A does not depend on the value of Qc except through the states and the
 * marginals.  Needs current marginals: the refusals and the staleness rule of gpslam_hip_get_marginals apply (GPSLAM_E_INVALID,
 * "stale"), so it works wherever S / S_next exist -- the dense landmark border, closures in one pass, column passes with
 * gpslam_hip_marginals_keep_closure_columns, the segmented path with gpslam_hip_marginals_on_segments.  GPSLAM_E_UNSUPPORTED, with a
 * message and before anything is launched: GPSLAM_ROT3_BIAS, fp32 handles, sharded handles and split pieces.  One streaming pass over
 * the priors and one reduction; it writes none of the solver's buffers: the marginals stay valid and the iterations that follow are
 * what they would have been.  No atomics, fixed summation order: two calls return the same bits.  n_f may be NULL. */
int gpslam_hip_qc_statistic(gpslam_hip_handle *h, double *A, int64_t *n_f);
/* host arithmetic only, no handle; d x d row-major matrices, 1 <= d <= 6.  GPSLAM_E_INVALID on a NULL pointer, on n_f <= 0, and
 * on an input that must be symmetric positive definite and is not (Qc, Qc0; A in the two updates, where the answer must be one). */
/* G = n_f Qc - A / 2 */
int gpslam_hip_qc_gradient(int32_t d, const double *Qc, const double *A, int64_t n_f, double *G);
/* Qc_next = A / (2 n_f), symmetric to the bit */
int gpslam_hip_qc_em_update(int32_t d, const double *A, int64_t n_f, double *Qc_next);
/* *theta = tr(Qc0^-1 A) / (2 n_f d): the stationary scale of Qc = theta Qc0 */
int gpslam_hip_qc_em_scale(int32_t d, const double *Qc0, const double *A, int64_t n_f, double *theta);

#ifdef __cplusplus
}
#endif
#endif
