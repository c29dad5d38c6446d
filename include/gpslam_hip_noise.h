/* gpslam_hip_noise.h -- learning measurement noise from data: per measurement kind the statistic the log-evidence's derivative in
 * the kind's covariance needs, the per-factor predicted covariances J Sigma J^T behind it (innovation / NIS diagnostics), that
 * derivative, and the EM updates it implies.
 *
 * An addition to include/gpslam_hip.h, which it includes; the ABI stays 2.4 and a binding detects these entry points by
 * presence (dlsym), as it does for the dogleg, the evidence and the Qc calls.
 *
 * The mathematics.  Factor m of kind k (GPSLAM_MEAS_*, residual dimension r <= 3) touches state i (and i + 1 for the two-state
 * kinds) and landmark l (for the kinds that name one).  e_m (r) and J_m = [H1 H2 | H3 H4 | H5[:ld]] (r x (2b + ld)) are exactly what
 * gpslam_hip_linearize_meas returns: the handle's chart, the VW slot as stored.  Sigma_m is the joint posterior covariance of the
 * variables the factor touches, from what gpslam_hip_get_marginals returns (S, S_next, S_x_lm, S_lm):
 *     Sigma_m = [[S[i],        S_next[i],  S_x_lm[i][:, l]    ],
 *                [S_next[i]^T, S[i+1],     S_x_lm[i+1][:, l]  ],
 *                [   .       ,    .      , S_lm[l, l]         ]]
 * The single-state kinds (RANGE, BEARING_RANGE) have the i and l parts only and never read state i + 1 (i may be N - 1, and S_next
 * of the last state is a zero block, not a covariance); kinds without a landmark have no landmark parts.  P_m = J_m Sigma_m J_m^T
 * (r x r), and R_m is the factor's base whitening: diag(1 / sigma), or the upper square-root information of
 * gpslam_hip_set_meas_covariance.  Over the used factors
 *     B = sum_m (e_m e_m^T + P_m),     Bw = sum_m R_m (e_m e_m^T + P_m) R_m^T,     n = the number of factors summed.
 * Let F(x, .) = -cost + sum_f log|det R_f| - 1/2 log det H at FIXED states x.
 *   - The used factors share one covariance C, W = C^-1: dF = tr(G dW) for symmetric dW with G = 1/2 (n C - B) -- the cost gives
 *     -1/2 sum e e^T, -1/2 tr(H^-1 dH/dW) gives -1/2 sum P, the normaliser n/2 log det W gives 1/2 n C.  G = 0 is the M-step of
 *     expectation-maximisation, C+ = B / n.
 *   - The scale family: factor m has C_m = theta C_m^0, every factor keeps its own shape.  dF/d log theta = 1/2 (tr Bw - n r) with Bw
 *     whitened at the current theta, so the stationary ratio is theta+ / theta = tr(Bw) / (n r); for diagonal models with one scale
 *     per row, theta_q+ / theta_q = Bw[q, q] / n.
 * On a graph of linear factors at its optimum these are total derivatives of the log-evidence; on a nonlinear graph they leave out the
 * implicit term -1/2 tr(H^-1 dH/dx^ dx^/d.), as gpslam_hip_qc.h's G does.
 */
#ifndef GPSLAM_HIP_NOISE_H
#define GPSLAM_HIP_NOISE_H

#include "gpslam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* B and Bw (r x r, row-major, symmetric to the bit) and n over the factors of one kind whose byte in `use` is not zero; `use` has one
 * byte per factor of the kind in the order the factors were added, NULL: all of them (two sensors of one kind: two calls, two masks).
 * B, Bw and n may each be NULL.  With no factor used n = 0, the matrices are zero and nothing is launched.  Needs current marginals:
 * the refusals and the staleness rule of gpslam_hip_get_marginals apply (GPSLAM_E_INVALID, "stale").  GPSLAM_E_UNSUPPORTED, with a
 * message and before anything is launched: fp32 handles, sharded handles, split pieces, GPSLAM_ROT3_BIAS, GPSLAM_MEAS_AHRS; a kind
 * that names a landmark on the segmented landmark path (S_lm and S_x_lm do not exist there; the kinds without a landmark work there
 * with gpslam_hip_marginals_on_segments); a used factor that carries a robust loss (the Gaussian M-step does not apply to it).
 * The factors are evaluated by the launch of gpslam_hip_linearize_meas in chunks of a fixed size, each followed by one contraction
 * pass and one reduction; what is written is what gpslam_hip_linearize_meas writes and the call's own buffers: the marginals stay
 * valid and the iterations that follow are what they would have been.  No atomics, fixed summation order: two calls return the same
 * bits. */
int gpslam_hip_meas_noise_statistic(gpslam_hip_handle *h, int32_t kind, const uint8_t *use, double *B, double *Bw, int64_t *n);
/* P_m = J_m Sigma_m J_m^T of every factor of the kind, count x r x r in the order the factors were added (each symmetric to the bit);
 * returns the count; P == NULL: the count alone, from the stored graph (no marginals needed, nothing launched).  The refusals of
 * the statistic except the last: a robust graph is accepted -- J is the unweighted Jacobian,
 * Sigma the inverse of the reweighted H as the marginals give it.  A projection factor whose landmark is behind its camera enters
 * with the error and the zero Jacobians gpslam_hip_linearize_meas reports for it (P_m = 0; in the statistic it adds e e^T): leave
 * such factors out with `use`. */
int gpslam_hip_meas_predicted_covariances(gpslam_hip_handle *h, int32_t kind, double *P);
/* host arithmetic only, no handle; r x r row-major matrices, 1 <= r <= 3.  GPSLAM_E_INVALID on a NULL pointer (ratio_rows may be
 * NULL), on n <= 0, on a non-finite input, on a C that is not symmetric positive definite, and on a B / Bw that is not where the
 * answer must be one (the two updates). */
/* G = 1/2 (n C - B) */
int gpslam_hip_noise_gradient(int32_t r, const double *C, const double *B, int64_t n, double *G);
/* C_next = B / n, symmetric to the bit */
int gpslam_hip_noise_em_update(int32_t r, const double *B, int64_t n, double *C_next);
/* *ratio = tr(Bw) / (n r), ratio_rows[q] = Bw[q, q] / n: the stationary scales relative to the current ones */
int gpslam_hip_noise_em_scale(int32_t r, const double *Bw, int64_t n, double *ratio, double *ratio_rows);

#ifdef __cplusplus
}
#endif
#endif
