/* gpslam_hip_sampling_at.h -- draws from the Laplace posterior in continuous time: the support states of
 * include/gpslam_hip_sampling.h AND the trajectory at any number of query times between them, each draw's queries conditioned on that
 * draw's own support states, with the GP's conditional noise and the correlation of the queries that share an interval.
 *
 * An addition to include/gpslam_hip_sampling.h, which it includes; the ABI stays 2.4 and a binding detects these entry points by
 * presence (dlsym).  DESIGN.md section 4n.
 *
 * The local variable.  Inside interval i the interpolators work in the local variable of the left state,
 *     gamma(t) = [xi(t); xi'(t)],  xi(t) = Log(T_i^-1 T(t)):   gamma(t_i) = [0; v_i],  gamma(t_i+1) = [xi_i,i+1; J v_i+1]
 * with J = Jr^-1(xi_i,i+1) on GPSLAM_POSE3 and J = I elsewhere (on the vector spaces xi = p - p_i) -- the arithmetic of
 * gpslam_hip_interpolate_poses.  In that variable the prior is the linear white-noise-on-acceleration process, so for times
 * a < tau < b, u = tau - a, s = b - tau, T = u + s:
 *     gamma(tau) | gamma(a), gamma(b)  ~  N(Lambda gamma(a) + Psi gamma(b),  K (x) Qc)
 *     Psi = Q(u) Phi(s)^T Q(T)^-1 = 1/T^3 [[u^2 (u + 3 s), -u^2 s T], [6 u s, u (u - 2 s) T]]  (x) I
 *     Lambda = Phi(u) - Psi Phi(T) = 1/T^3 [[s^2 (3 u + s), u s^2 T], [-6 u s, s (s - 2 u) T]]  (x) I
 *     K = 1/T^3 [[u^3 s^3 / 3, u^2 s^2 (s - u) / 2], [u^2 s^2 (s - u) / 2, u s (s^2 - s u + u^2)]]
 * and K = l l^T with  l00 = (u s)^(3/2) / sqrt(3 T^3),  l10 = sqrt(3) (s - u) sqrt(u s) / (2 T^(3/2)),  l11 = sqrt(u s / T) / 2.
 * K[0][0] at a = 0, b = dt is the c(dt, tau) of gpslam_hip_interpolate_covariances.
 *
 * The walk (interface: signs and the order of eps_p / eps_v included).  The process is Markov: the queries tau_1 < ... < tau_m of
 * an interval are drawn in order, L_q the lower Cholesky factor of the handle's Qc (gpslam_hip_set_qc),
 *     gamma_0 = gamma(t_i),
 *     gamma_k = Lambda_k gamma_k-1 + Psi_k gamma(t_i+1) + [l00 L_q eps_p; l10 L_q eps_p + l11 L_q eps_v],   (a, tau, b) = (tau_k-1, tau_k, dt),
 * tau_0 = 0, and the pose of the draw at tau_k is T_i (+) Exp(xi_k) -- the exponential map whatever the handle's chart, as in
 * gpslam_hip_interpolate_poses.  T_i, v_i, T_i+1, v_i+1 are THIS DRAW'S support states.  With eps_p = eps_v = 0 the queries are
 * gpslam_hip_interpolate_poses of the drawn support states.
 *
 * The noise vector (n_noise_at = n_noise + 2 d n_queries entries).  The first n_noise entries are those of
 * gpslam_hip_sample_posterior; behind them every query q, in the call's order, has 2 d entries: eps_p (d), then eps_v (d).  The
 * generator is gpslam_hip_sampling.h's with noise index j = n_noise + 2 d q + c.  The bridge's normals are staged with the support
 * states' by the same kernel, so a draw from the generator and a draw from the numbers gpslam_hip_posterior_noise_at returns run the
 * same arithmetic on the same bits.
 *
 * The queries.  left is non-decreasing; within a run of equal left, dt is one number and tau increases strictly with
 * 0 < tau < dt.  Anything else -- left > N - 2, n_queries <= 0, no output asked for -- is GPSLAM_E_INVALID, and the message names the
 * first offending query.  Extrapolation and tau in {0, dt} are not sampled here (K is singular or the bridge is not defined).
 *
 * GPSLAM_E_UNSUPPORTED, with a message and before anything is launched: everything gpslam_hip_sample_posterior refuses;
 * GPSLAM_ROT3_BIAS handles; world-frame velocities (velocity_world: the local variable differs); handles that carry GP priors with a
 * Qc of their own (gpslam_hip_add_gp_priors_qc); query_vels on a Lie group (as gpslam_hip_interpolate_velocities).
 */
#ifndef GPSLAM_HIP_SAMPLING_AT_H
#define GPSLAM_HIP_SAMPLING_AT_H

#include "gpslam_hip_sampling.h"

#ifdef __cplusplus
extern "C" {
#endif

/* length of one noise vector of a dense draw: posterior_noise_dim + 2 d n_queries.  Nothing is launched */
int gpslam_hip_posterior_noise_dim_at(gpslam_hip_handle *h, int32_t n_queries, int32_t *n_noise_at);
/* the generator's numbers, count x n_noise_at (row-major), without solving anything; the first n_noise columns are
 * gpslam_hip_posterior_noise's */
int gpslam_hip_posterior_noise_at(gpslam_hip_handle *h, uint64_t seed, uint64_t first, int32_t count,
                                  int32_t n_queries, double *noise);
/* count draws of the support states AND of the n_queries query times.  noise: count x n_noise_at given by the caller, or NULL: the
 * generator with (seed, first).
 *   left, dt, tau   n_queries, as gpslam_hip_interpolate_poses takes them
 *   query_poses     count x n_queries x pose_dim   (rows in the layout of gpslam_hip_get_states)
 *   query_vels      count x n_queries x d          GPSLAM_LINEAR2 / LINEAR3 only (the xi' part); elsewhere non-NULL is
 *                                                  GPSLAM_E_UNSUPPORTED, as gpslam_hip_interpolate_velocities
 *   delta, poses, vels, landmarks                  the same draw's support outputs, as gpslam_hip_sample_posterior
 * Any of the outputs may be NULL (not all of them).  With the same (seed, first), or the same leading n_noise columns of noise, the
 * support outputs are gpslam_hip_sample_posterior's to the bit; sample k of a call equals sample 0 of a call with first + k, query
 * outputs included; the same arguments return the same bits.  The handle is left as gpslam_hip_sample_posterior leaves it. */
int gpslam_hip_sample_posterior_at(gpslam_hip_handle *h, int32_t count, uint64_t seed, uint64_t first, const double *noise,
                                   int32_t n_queries, const int32_t *left, const double *dt, const double *tau,
                                   double *query_poses, double *query_vels,
                                   double *delta, double *poses, double *vels, double *landmarks);

#ifdef __cplusplus
}
#endif
#endif
