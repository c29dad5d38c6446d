// samplePosteriorAt of gpslam_amd/host/gpslam_host.hpp (include/gpslam_hip_sampling_at.h).  Without an argument: the answers of the
// three entry points to a NULL handle and to arguments that are refused before the handle is looked at -- no device call.  With one,
// on the GPU: dense draws of the small Pose2 chain of posterior_host_tests.cpp, one query of one of them printed for
// tests/test_sampling_at_host.py, which builds the same graph through the Python binding.
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
  int32_t n = 7, left[1] = {0};
  double x[4] = {0, 0, 0, 0}, dt[1] = {1.0}, tau[1] = {0.5};
  EXPECT(gpslam_hip_posterior_noise_dim_at(nullptr, 1, &n) == GPSLAM_E_INVALID && n == 7);
  EXPECT(gpslam_hip_posterior_noise_at(nullptr, 1, 0, 1, 1, x) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_sample_posterior_at(nullptr, 1, 1, 0, nullptr, 1, left, dt, tau, x, nullptr, nullptr, nullptr, nullptr, nullptr) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_sample_posterior_at(nullptr, 0, 1, 0, nullptr, 1, left, dt, tau, x, nullptr, nullptr, nullptr, nullptr, nullptr) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_sample_posterior_at(nullptr, 1, 1, 0, nullptr, 0, left, dt, tau, x, nullptr, nullptr, nullptr, nullptr, nullptr) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_sample_posterior_at(nullptr, 1, 1, 0, nullptr, 1, left, dt, tau, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == GPSLAM_E_INVALID);
  bool thrown = false;
  try { samplePosteriorAt<Pose2>(NonlinearFactorGraph(), Values(), {Symbol('x', 0)}, {1.0}, {0.5}, 0); } catch (const std::invalid_argument &) { thrown = true; }
  EXPECT(thrown);
  thrown = false;
  try { samplePosteriorAt<Pose2>(NonlinearFactorGraph(), Values(), {Symbol('x', 0)}, {1.0, 1.0}, {0.5}, 1); } catch (const std::invalid_argument &) { thrown = true; }
  EXPECT(thrown);
}

// N = 12, dt = 0.25, Qc = 0.5 I; tests/test_evidence_cpp.py's _python_twin builds the same numbers
static void test_dense_draws_of_a_pose2_chain() {
  const int N = 12;
  const double dt = 0.25, w = 0.6, v = 1.0;
  const double th = dt * w;
  const Pose2 step(v * dt * std::sin(th) / th, v * dt * (1 - std::cos(th)) / th, th);
  auto compose = [](const Pose2 &a, const Pose2 &c) {
    return Pose2(a.x + std::cos(a.theta) * c.x - std::sin(a.theta) * c.y, a.y + std::sin(a.theta) * c.x + std::cos(a.theta) * c.y, a.theta + c.theta);
  };
  std::vector<Pose2> truth(N);
  for (int k = 0; k + 1 < N; k++) truth[k + 1] = compose(truth[k], step);
  auto Qc_model = noiseModel::Gaussian::Covariance(0.5 * Matrix::Identity(3));
  NonlinearFactorGraph graph;
  graph.add(PriorFactor<Pose2>(Symbol('x', 0), truth[0], noiseModel::Isotropic::Sigma(3, 1e-2)));
  for (int k = 0; k + 1 < N; k++) {
    graph.add(GaussianProcessPriorPose2(Symbol('x', k), Symbol('v', k), Symbol('x', k + 1), Symbol('v', k + 1), dt, Qc_model));
    graph.add(BetweenFactor<Pose2>(Symbol('x', k), Symbol('x', k + 1), step, noiseModel::Isotropic::Sigma(3, 2e-2)));
  }
  Values init;
  for (int k = 0; k < N; k++) {
    init.insert(Symbol('x', k), Pose2(truth[k].x + 0.03 * std::sin(0.7 * k), truth[k].y - 0.02 * std::cos(0.4 * k), truth[k].theta + 0.04 * std::sin(0.3 * k)));
    init.insert(Symbol('v', k), Vector3{v, 0, w});
  }
  // a run of one on interval 0, a run of two on interval 4, a run of one on the last interval
  const std::vector<Key> left = {Symbol('x', 0), Symbol('x', 4), Symbol('x', 4), Symbol('x', N - 2)};
  const std::vector<double> dts(4, dt), tau = {0.1, 0.05, 0.2, 0.125};
  const uint64_t seed = (uint64_t(9) << 40) + 77, first = 5;
  const PosteriorDrawsAt<Pose2> three = samplePosteriorAt<Pose2>(graph, init, left, dts, tau, 3, seed, first);
  EXPECT(three.support.size() == 3 && three.queries.size() == 3);
  for (const auto &q : three.queries) EXPECT(q.size() == left.size());
  // the support states are samplePosterior's for the same (seed, first), to the bit
  const std::vector<Values> plain = samplePosterior(graph, init, 3, seed, first);
  bool same = true;
  for (int k = 0; k < N; k++) {
    const Pose2 a = three.support[1].at<Pose2>(Symbol('x', k)), c = plain[1].at<Pose2>(Symbol('x', k));
    same = same && a.x == c.x && a.y == c.y && a.theta == c.theta;
  }
  EXPECT(same);
  // draw k of a call is draw 0 of a call that starts at first + k: to the bit, queries included
  const PosteriorDrawsAt<Pose2> one = samplePosteriorAt<Pose2>(graph, init, left, dts, tau, 1, seed, first + 2);
  same = true;
  for (size_t q = 0; q < left.size(); q++) {
    const Pose2 a = three.queries[2][q], c = one.queries[0][q];
    same = same && a.x == c.x && a.y == c.y && a.theta == c.theta;
    EXPECT(std::isfinite(a.x) && std::isfinite(a.y) && std::isfinite(a.theta));
  }
  EXPECT(same);
  // a query between two states is not the draw's left state
  EXPECT(three.queries[1][2].x != three.support[1].at<Pose2>(Symbol('x', 4)).x);
  const Pose2 p = three.queries[1][2];
  std::printf("samplePosteriorAt draw 1 query 2: %.17g %.17g %.17g\n", p.x, p.y, p.theta);
  // a second Qc_model in the graph: the bridge has one Qc, the call is refused
  NonlinearFactorGraph two;
  two.add(PriorFactor<Pose2>(Symbol('x', 0), truth[0], noiseModel::Isotropic::Sigma(3, 1e-2)));
  for (int k = 0; k + 1 < N; k++) {
    auto Qk = k + 2 < N ? Qc_model : noiseModel::Gaussian::Covariance(0.7 * Matrix::Identity(3));
    two.add(GaussianProcessPriorPose2(Symbol('x', k), Symbol('v', k), Symbol('x', k + 1), Symbol('v', k + 1), dt, Qk));
    two.add(BetweenFactor<Pose2>(Symbol('x', k), Symbol('x', k + 1), step, noiseModel::Isotropic::Sigma(3, 2e-2)));
  }
  EXPECT(samplePosterior(two, init, 1, seed, first).size() == 1);      // (the graph itself is fine)
  bool thrown = false;
  try { samplePosteriorAt<Pose2>(two, init, left, dts, tau, 1, seed, first); } catch (const std::exception &) { thrown = true; }
  EXPECT(thrown);
}

int main(int argc, char **) {
  test_null_handle_and_arguments();
  if (argc > 1) test_dense_draws_of_a_pose2_chain();
  if (failures) { std::printf("sampling_at_host_tests: %d FAILED\n", failures); return 1; }
  std::printf("sampling_at_host_tests: all tests passed\n");
  return 0;
}
