/* gpslam_hip_sampling_stats.h -- statistics of the posterior draws in continuous time, reduced on the device: the draws of
 * include/gpslam_hip_sampling_at.h at the query times, returned as per-query moment sums and collision counts and as per-draw
 * clearances and path lengths instead of count x n_queries poses.  No support or query slab goes to the host.
 *
 * An addition to include/gpslam_hip_sampling_at.h, which it includes; the ABI stays 2.4 and a binding detects these entry points by
 * presence (dlsym).  DESIGN.md section 4o.
 *
 * The draws.  Queries, noise vector (n_noise_at entries, no new normals), generator and staging are those of the dense call: with
 * the same (seed, first) or the same noise, draw k's query poses q_kq are the query_poses of that call to the bit.
 *
 * The reference pose.  q^_q is the interpolated estimate at query q, what the interpolators return for (left, dt, tau).
 *
 * Moments.  eta_kq in R^d are the local coordinates of q_kq around q^_q under the handle's chart -- the unwhitened error of a pose
 * prior at q^_q: q - q^ on the vector spaces, Log(q^^-1 q) on SO(3) and SE(3), chart-dependent on SE(2) -- the tangent the
 * interpolated covariances speak in.
 *     s1   n_queries x d                 sum_k eta_kq
 *     s2   n_queries x d (d + 1) / 2     the lower triangle of sum_k eta_kq eta_kq^T, rows packed: entry (r, c), c <= r, at r (r + 1) / 2 + c
 * s1 and s2 come together or not at all.
 *
 * Obstacles.  obstacles is n_obstacles x (w + 1): a centre, then a radius >= 0; w = 3 on GPSLAM_POSE3, otherwise 2.  A pose's
 * position p is its first two coordinates on GPSLAM_LINEAR2 / LINEAR3 / POSE2 and the translation (entries 9 .. 11 of its row) on
 * GPSLAM_POSE3.
 *     g_kq = min_o (|p_kq - c_o| - r_o) - margin
 *     hits[q]       the number of draws with g_kq < 0 (strictly)
 *     clearance[k]  min_q g_kq;   mean(clearance < 0) estimates the probability that the path collides
 * 0 <= n_obstacles <= 1024.
 *
 * Length.  length[k] = sum_{q = 0}^{n_queries - 2} |p_k,q+1 - p_kq|, the polyline through the query positions in the call's order;
 * exactly 0.0 for one query.
 *
 * Accumulating.  With accumulate == 0 the per-query sums start at zero and *n_draws = count on return.  Otherwise s1, s2, hits and
 * *n_draws are read as starting values and continued: the caller owns them, nothing is kept on the handle.  clearance and length
 * always describe this call's count draws.  Every per-query sum adds its draws in the order k = 0, 1, ...: a continued call returns
 * the bits of one call over all the draws, and clearance[k], length[k] are functions of draw k and the queries alone.
 *
 * GPSLAM_E_INVALID: every output NULL; s1 without s2 or s2 without s1; hits or clearance with n_obstacles == 0; n_obstacles > 0 with
 * neither; a negative radius or margin; n_draws NULL while s1 or hits is asked for; count <= 0; and whatever the dense call says
 * about the queries.
 * GPSLAM_E_UNSUPPORTED, with a message and before anything is launched: everything the dense call refuses; hits, clearance or
 * length on GPSLAM_ROT3, which has no position.
 */
#ifndef GPSLAM_HIP_SAMPLING_STATS_H
#define GPSLAM_HIP_SAMPLING_STATS_H

#include "gpslam_hip_sampling_at.h"

#ifdef __cplusplus
extern "C" {
#endif

/* count draws at the n_queries query times, reduced on the device.  noise: count x n_noise_at given by the caller, or NULL: the
 * generator with (seed, first).  Any of s1 / s2, hits, clearance, length may be NULL (not all of them).  The handle is left as the
 * dense call leaves it. */
int gpslam_hip_sample_posterior_stats(gpslam_hip_handle *h, int32_t count, uint64_t seed, uint64_t first, const double *noise,
                                      int32_t n_queries, const int32_t *left, const double *dt, const double *tau,
                                      int32_t n_obstacles, const double *obstacles, double margin,
                                      int32_t accumulate, int64_t *n_draws,
                                      double *s1, double *s2, int64_t *hits,          /* per query, accumulated over draws */
                                      double *clearance, double *length);              /* per draw of THIS call */
/* mean = s1 / n and cov = (S2 - n mean mean^T) / (n - 1), full symmetric d x d per query (cov may be NULL).  Host arithmetic, no
 * device.  n < 1, or n < 2 with cov, is GPSLAM_E_INVALID. */
int gpslam_hip_posterior_moments(int32_t d, int32_t n_queries, int64_t n_draws, const double *s1, const double *s2,
                                 double *mean, double *cov);

#ifdef __cplusplus
}
#endif
#endif
