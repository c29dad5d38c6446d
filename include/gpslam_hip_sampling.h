/* gpslam_hip_sampling.h -- draws from the Laplace posterior N(x^, H^-1) of a gpslam_hip_handle: whole trajectories, landmarks
 * included.
 *
 * An addition to include/gpslam_hip.h, which it includes; the ABI stays 2.4 and a binding detects these entry points by
 * presence (dlsym), as it does for the dogleg, the evidence and the Qc calls.
 *
 * The method.  J is the whitened Jacobian of the current linearisation (robust factors at their current weights), H = J^T J the
 * matrix gpslam_hip_marginals inverts.  For eps ~ N(0, I), one entry per whitened row,
 *     delta(eps) = -H^-1 J^T eps            has covariance H^-1 J^T J H^-1 = H^-1:
 * delta(eps) is THE GAUSS-NEWTON STEP THE GRAPH WOULD TAKE IF EVERY WHITENED RESIDUAL WERE eps.  A draw is one assembly and one solve
 * at lambda = 0 over the linearisation the call made once; x^ (+) delta is the sample.  Sign and order are part of the interface:
 * with eps set to the graph's own whitened residuals the draw is the Gauss-Newton step.
 *
 * The noise vector (n_noise entries).  First the n_rows entries of the row tables in the order gpslam_hip_get_rows documents (the M
 * full-width rows, then the Mc compact rows: entry k belongs to the row whose whitened error get_rows returns in rowE[k]); behind
 * them the landmark priors in the order they were added, landmark_dim coordinates each (whitened residual (l - prior) / sigma).
 *
 * The generator (counter-based: a number depends on (seed, sample index s, noise index j) alone -- not on count, on how a call is
 * cut into chunks, or on the launch shape).  Philox4x32-10 (Salmon et al., SC'11; Random123), multipliers 0xD2511F53 and 0xCD9E8D57,
 * Weyl constants 0x9E3779B9 and 0xBB67AE85, the key bumped before every round but the first.  Key (seed & 0xffffffff, seed >> 32),
 * counter (j lo, j hi, s lo, s hi), s = first + k for sample k of a call.  From the four output words w0 .. w3, in double:
 *     u1 = (w0 + (w1 + 0.5) 2^-32) 2^-32,   u2 = (w2 + w3 2^-32) 2^-32,   eps = sqrt(-2 ln u1) cos(2 pi u2)
 * -- one normal per counter (the second Box-Muller value is not used).
 *
 * Supported: fp64, unsharded handles, without landmarks or with the dense landmark border, every manifold (GPSLAM_ROT3_BIAS: the pad
 * coordinates of a draw are exact zeros), every factor kind, robust losses.  GPSLAM_E_UNSUPPORTED, with a message and before
 * anything is launched: fp32 handles, sharded handles, split pieces, the segmented landmark path, and handles with loop closures,
 * state Gaussians or border Gaussians (closures and border Gaussians have no rows in the tables to perturb: their noise would need
 * square roots of its own; the factors a marginalised head leaves are refused together).
 */
#ifndef GPSLAM_HIP_SAMPLING_H
#define GPSLAM_HIP_SAMPLING_H

#include "gpslam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* length of one noise vector: rows of the row tables + landmark-prior coordinates.  Nothing is launched */
int gpslam_hip_posterior_noise_dim(gpslam_hip_handle *h, int32_t *n_noise);
/* the generator's numbers for samples first .. first+count-1 (count x n_noise, row-major), without solving anything */
int gpslam_hip_posterior_noise(gpslam_hip_handle *h, uint64_t seed, uint64_t first, int32_t count, double *noise);
/* count draws.  noise: count x n_noise given by the caller, or NULL: the generator with (seed, first).
 * Any of the outputs may be NULL (not all of them: GPSLAM_E_INVALID, as for count <= 0):
 *   delta      count x (N*b + L*landmark_dim)  the tangent draws, states then landmarks
 *   poses      count x N x pose_dim            } x^ (+) delta in the layout of gpslam_hip_get_states
 *   vels       count x N x d                   }
 *   landmarks  count x L x landmark_dim        the layout of gpslam_hip_get_landmarks
 * Linearises once, at the current states (a pending run_gn update applied first); per draw an assembly and a solve.  The estimate,
 * the landmarks and the factor set are left bit for bit as they were; the solver's buffers are rewritten, so the marginals are
 * stale afterwards.  GPSLAM_E_NOT_SPD on a non-positive pivot (nothing is written to the outputs of that chunk of draws).  No
 * atomics, fixed summation order: the same arguments return the same bits, and sample k of a call equals sample 0 of a call with
 * first + k. */
int gpslam_hip_sample_posterior(gpslam_hip_handle *h, int32_t count, uint64_t seed, uint64_t first,
                                const double *noise, double *delta, double *poses, double *vels, double *landmarks);

#ifdef __cplusplus
}
#endif
#endif
