// samplePosterior of gpslam_amd/host/gpslam_host.hpp (include/gpslam_hip_sampling.h).  Without an argument: the answers of the three
// entry points to a NULL handle and to arguments that are refused before the handle is looked at -- no device call.  With one, on
// the GPU: draws of a small Pose2 chain (a prior, GP priors, odometry; the graph of evidence_host_tests.cpp), one of them printed for
// tests/test_posterior_host.py, which builds the same graph through the Python binding.
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
  int32_t n = 7;
  double x[4] = {0, 0, 0, 0};
  EXPECT(gpslam_hip_posterior_noise_dim(nullptr, &n) == GPSLAM_E_INVALID && n == 7);
  EXPECT(gpslam_hip_posterior_noise(nullptr, 1, 0, 1, x) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_sample_posterior(nullptr, 1, 1, 0, nullptr, x, nullptr, nullptr, nullptr) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_sample_posterior(nullptr, 0, 1, 0, nullptr, x, nullptr, nullptr, nullptr) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_sample_posterior(nullptr, 1, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == GPSLAM_E_INVALID);
  bool thrown = false;
  try { samplePosterior(NonlinearFactorGraph(), Values(), 0); } catch (const std::invalid_argument &) { thrown = true; }
  EXPECT(thrown);
}

// N = 12, dt = 0.25, Qc = 0.5 I; tests/test_evidence_cpp.py's _python_twin builds the same numbers
static void test_draws_of_a_pose2_chain() {
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
  const uint64_t seed = (uint64_t(9) << 40) + 77, first = 5;
  const std::vector<Values> three = samplePosterior(graph, init, 3, seed, first);
  EXPECT(three.size() == 3);
  for (const Values &s : three) EXPECT(s.size() == init.size());
  // draw k of a call is draw 0 of a call that starts at first + k: to the bit
  const std::vector<Values> one = samplePosterior(graph, init, 1, seed, first + 2);
  bool same = true, moved = false;
  for (int k = 0; k < N; k++) {
    const Pose2 a = three[2].at<Pose2>(Symbol('x', k)), c = one[0].at<Pose2>(Symbol('x', k)), x0 = init.at<Pose2>(Symbol('x', k));
    const Vector3 va = three[2].at<Vector3>(Symbol('v', k)), vc = one[0].at<Vector3>(Symbol('v', k));
    same = same && a.x == c.x && a.y == c.y && a.theta == c.theta && va[0] == vc[0] && va[1] == vc[1] && va[2] == vc[2];
    moved = moved || a.x != x0.x;
    EXPECT(std::isfinite(a.x) && std::isfinite(a.y) && std::isfinite(a.theta));
  }
  EXPECT(same);
  EXPECT(moved);
  const Pose2 p = three[1].at<Pose2>(Symbol('x', 3));
  const Vector3 q = three[1].at<Vector3>(Symbol('v', 3));
  std::printf("samplePosterior draw 1 state 3: %.17g %.17g %.17g %.17g %.17g %.17g\n", p.x, p.y, p.theta, q[0], q[1], q[2]);
}

int main(int argc, char **) {
  test_null_handle_and_arguments();
  if (argc > 1) test_draws_of_a_pose2_chain();
  if (failures) { std::printf("posterior_host_tests: %d FAILED\n", failures); return 1; }
  std::printf("posterior_host_tests: all tests passed\n");
  return 0;
}
