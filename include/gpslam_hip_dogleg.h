/* gpslam_hip_dogleg.h -- Powell's dogleg optimiser (gtsam::DoglegOptimizer) on a gpslam_hip_handle.
 *
 * An addition to include/gpslam_hip.h, which it includes; the ABI stays 2.4 and a binding detects these entry points by
 * presence (dlsym), as it does for the fixed-lag calls.
 *
 * The mathematics.  At the linearisation point the undamped system is H dn = g, g = -gradient (the library's sign: the
 * Levenberg-Marquardt trials solve (H + lambda I) d = g); unknowns are the states, then the landmarks.  The device forms four
 * scalars per linearisation,
 *     gg = g . g,   gHg = g^T H g,   gn = g . dn,   nn = dn . dn,
 * and everything else is host arithmetic on them.  With s = gg / gHg the steepest-descent (Cauchy) step is du = s g,
 * |du|^2 = s^2 gg, du . dn = s gn.  The dogleg point of trust radius Delta (DoglegOptimizerImpl::ComputeDoglegPoint):
 *     Delta < |du|         dd = (Delta / |du|) du                                       branch 0
 *     Delta < |dn|         dd = du + tau (dn - du), tau in [0, 1], |dd| = Delta         branch 1 (ComputeBlend)
 *     otherwise            dd = dn                                                      branch 2
 * so that always dd = alpha g + beta dn.  Degenerate (gg == 0 or gHg <= 0): the Gauss-Newton step clipped to Delta, alpha = 0,
 * beta = min(1, Delta / |dn|), beta = 0 when nn == 0; reported as branch 2.  The decrease the quadratic model predicts, by H dn = g:
 *     M(0) - M(dd) = (alpha gg + beta gn) - 0.5 (alpha^2 gHg + 2 alpha beta gg + beta^2 gn).
 *
 * The trust-region update follows GTSAM 4.0 DoglegOptimizerImpl::Iterate AS RECALLED: PARITY UNPINNED (the status
 * gpslam_hip.h gives gpslam_hip_lm_decide).  rho = (f - f_new) / predicted if both |f - f_new| and |predicted| exceed 1e-15,
 * else 0.5.  last_action: 0 none, 1 Delta was increased, 2 Delta was decreased (inside one iterate() call; starts at 0).
 *
 *     rho >= 0.75          newDelta = max(Delta, 3 |dd|); keep = 1
 *                            ONE_STEP_PER_ITERATION, SEARCH_REDUCE_ONLY:  stay = 0
 *                            SEARCH_EACH_ITERATION:  stay = 0 if |newDelta - Delta| < 1e-15 or last_action == 2,
 *                                                    else stay = 1 and last_action = 1
 *                          Delta = newDelta
 *     0.25 <= rho < 0.75   keep = 1, stay = 0, Delta stays
 *     0 <= rho < 0.25      keep = 1; Delta > 1e-5: newDelta = Delta / 2, else newDelta = Delta (the floor is hit)
 *                            ONE_STEP_PER_ITERATION, or last_action == 1, or the floor is hit:  stay = 0
 *                            SEARCH_EACH_ITERATION, SEARCH_REDUCE_ONLY otherwise:  stay = 1 and last_action = 2
 *                          Delta = newDelta
 *     rho < 0, not finite  keep = 0 (every mode); Delta > 1e-5: Delta /= 2, stay = 1, last_action = 2; else stay = 0
 *
 * One stated deviation from GTSAM: a loop that ends with f_new > f (Delta at its floor) restores the linearisation point and
 * reports accepted = 0.
 *
 * f is the cost Levenberg-Marquardt compares: with robust losses the sum of rho, the model built on the reweighted H.
 *
 * Supported: fp64, unsharded handles; every manifold, chain and measurement factor, state Gaussians, robust losses on
 * measurement factors, the dense landmark border.  GPSLAM_E_UNSUPPORTED, before anything is launched: fp32 handles, sharded handles
 * and split pieces, the segmented landmark path, loop closures, border Gaussians.
 */
#ifndef GPSLAM_HIP_DOGLEG_H
#define GPSLAM_HIP_DOGLEG_H

#include "gpslam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { GPSLAM_DOGLEG_ONE_STEP_PER_ITERATION = 0, GPSLAM_DOGLEG_SEARCH_EACH_ITERATION = 1, GPSLAM_DOGLEG_SEARCH_REDUCE_ONLY = 2 };

/* host arithmetic only, no handle.  s4 = {gg, gHg, gn, nn}; coef2 = {alpha, beta}; branch 0 scaled steepest descent, 1 blend,
 * 2 Gauss-Newton.  step_norm, predicted, branch may be NULL */
int gpslam_hip_dogleg_point(const double *s4, double delta, double *coef2, double *step_norm, double *predicted, int32_t *branch);
/* host arithmetic only.  s4 = {f, f_new, predicted, |delta_d|}; updates *delta and *last_action; *keep: the trial's values are the
 * result so far; *stay: try again */
int gpslam_hip_dogleg_decide(const double *s4, int32_t mode, double *delta, int32_t *last_action, int32_t *keep, int32_t *stay);
/* one DoglegOptimizer::iterate(): linearise, ONE solve, then trials until stay == 0.  *delta in/out (GTSAM's deltaInitial is 1.0).
 * st: error_before, error_after, delta_inf_norm of the kept step, lambda = the trust radius after, trials, accepted,
 * last_trial_error */
int gpslam_hip_iterate_dogleg(gpslam_hip_handle *h, double *delta, int32_t mode, gpslam_hip_stats *st);
/* NonlinearOptimizer::defaultOptimize over iterate_dogleg with the stop rules of p (max_iterations, the three error tolerances,
 * delta_tol).  st: error_before / error_after of the whole run, iterations, lambda = the trust radius at the end, status = the return
 * code; delta_inf_norm, accepted, trials and last_trial_error are those of the LAST iteration (accepted = 0, trials = 0 and
 * last_trial_error = error_before when none ran because error_before <= error_tol; accepted = 0 when the last one failed) */
int gpslam_hip_optimize_dogleg(gpslam_hip_handle *h, const gpslam_hip_params *p, double delta_initial, int32_t mode, gpslam_hip_stats *st);
/* what the last iterate_dogleg computed: out8 = {gg, gHg, gn, nn, alpha, beta, predicted, branch} of its LAST trial (tests, tuning) */
int gpslam_hip_dogleg_last(gpslam_hip_handle *h, double *out8);

#ifdef __cplusplus
}
#endif
#endif
