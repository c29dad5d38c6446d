// samplePosteriorStats of gpslam_amd/host/gpslam_host.hpp (include/gpslam_hip_sampling_stats.h).  Without a device: the answers of
// gpslam_hip_sample_posterior_stats to a NULL handle and to arguments that are refused before the handle is looked at, and
// gpslam_hip_posterior_moments, which is host arithmetic, on numbers worked out by hand.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../gpslam_amd/host/gpslam_host.hpp"

using namespace gtsam;
using namespace gpslam;

static int failures = 0;
#define EXPECT(cond)                                                                  \
  do {                                                                                \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
  } while (0)

static void test_null_handle_and_arguments() {
  int32_t left[1] = {0};
  int64_t n = 7, hits[1] = {0};
  double x[4] = {0, 0, 0, 0}, dt[1] = {1.0}, tau[1] = {0.5}, ob[3] = {0.0, 0.0, 1.0};
  EXPECT(gpslam_hip_sample_posterior_stats(nullptr, 1, 1, 0, nullptr, 1, left, dt, tau, 1, ob, 0.0, 0, &n, x, x, hits, x, x) == GPSLAM_E_INVALID && n == 7);
  EXPECT(gpslam_hip_sample_posterior_stats(nullptr, 0, 1, 0, nullptr, 1, left, dt, tau, 1, ob, 0.0, 0, &n, x, x, hits, x, x) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_sample_posterior_stats(nullptr, 1, 1, 0, nullptr, 0, left, dt, tau, 1, ob, 0.0, 0, &n, x, x, hits, x, x) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_sample_posterior_stats(nullptr, 1, 1, 0, nullptr, 1, left, dt, tau, 0, nullptr, 0.0, 0, &n, nullptr, nullptr, nullptr, nullptr, nullptr) == GPSLAM_E_INVALID);
  bool thrown = false;
  try { samplePosteriorStats(NonlinearFactorGraph(), Values(), {Symbol('x', 0)}, {1.0}, {0.5}, 0); } catch (const std::invalid_argument &) { thrown = true; }
  EXPECT(thrown);
  thrown = false;
  try { samplePosteriorStats(NonlinearFactorGraph(), Values(), {Symbol('x', 0)}, {1.0, 1.0}, {0.5}, 1); } catch (const std::invalid_argument &) { thrown = true; }
  EXPECT(thrown);
}

static void test_moments_by_hand() {
  // two queries in the plane, draws (1, 2), (3, 6), (5, 1) at the first and (0, 0), (2, 2), (4, 4) at the second
  const double s1[4] = {9.0, 9.0, 6.0, 6.0};
  const double s2[6] = {35.0, 25.0, 41.0, 20.0, 20.0, 20.0};      // (0, 0), (1, 0), (1, 1) per query
  double mean[4], cov[8];
  EXPECT(gpslam_hip_posterior_moments(2, 2, 3, s1, s2, mean, cov) == 0);
  const double want_mean[4] = {3.0, 3.0, 2.0, 2.0}, want_cov[8] = {4.0, -1.0, -1.0, 7.0, 4.0, 4.0, 4.0, 4.0};
  for (int i = 0; i < 4; i++) EXPECT(std::fabs(mean[i] - want_mean[i]) <= 1e-14);
  for (int i = 0; i < 8; i++) EXPECT(std::fabs(cov[i] - want_cov[i]) <= 1e-13);
  EXPECT(gpslam_hip_posterior_moments(2, 2, 1, s1, s2, mean, nullptr) == 0 && mean[0] == 9.0);
  EXPECT(gpslam_hip_posterior_moments(2, 2, 1, s1, s2, mean, cov) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_posterior_moments(2, 2, 0, s1, s2, mean, nullptr) == GPSLAM_E_INVALID);
  PosteriorStats st;
  EXPECT(st.draws == 0 && st.mean.empty() && st.hits.empty());
}

int main() {
  test_null_handle_and_arguments();
  test_moments_by_hand();
  if (failures) { std::printf("sampling_stats_host_tests: %d FAILED\n", failures); return 1; }
  std::printf("sampling_stats_host_tests: all tests passed\n");
  return 0;
}
