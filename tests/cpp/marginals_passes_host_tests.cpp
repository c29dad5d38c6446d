// gtsam::Marginals on a graph whose loop closures go through the solver in column passes (gpslam_amd/host/gpslam_host.hpp): 12
// non-adjacent BetweenFactor<Pose2> are two passes, and the Marginals constructor asks its own session to keep the closures'
// columns at every state (gpslam_hip_marginals_keep_closure_columns) before gpslam_hip_marginals.  The blocks the class hands out
// are compared with gpslam_hip_get_marginals on its handle, as tests/cpp/marginals_host_tests.cpp does.  Without an argument the
// program only proves that it links (no device call); with one it runs on the GPU.
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "../../gpslam_amd/host/gpslam_host.hpp"

using namespace gtsam;
using namespace gpslam;

static int failures = 0;
#define EXPECT(cond)                                                                  \
  do {                                                                                \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
  } while (0)

static Pose2 compose(const Pose2 &a, const Pose2 &b) {
  return Pose2(a.x + std::cos(a.theta) * b.x - std::sin(a.theta) * b.y, a.y + std::sin(a.theta) * b.x + std::cos(a.theta) * b.y, a.theta + b.theta);
}
static Pose2 between(const Pose2 &a, const Pose2 &b) {   // a^-1 b
  const double dx = b.x - a.x, dy = b.y - a.y, c = std::cos(a.theta), s = std::sin(a.theta);
  return Pose2(c * dx + s * dy, -s * dx + c * dy, b.theta - a.theta);
}

// m(r, c) == f(r, c) exactly for an rows x cols block (the host class copies numbers, it computes none)
template <typename F> static bool same(const Matrix &m, int rows, int cols, F f) {
  if (m.rows != rows || m.cols != cols) return false;
  for (int r = 0; r < rows; r++)
    for (int c = 0; c < cols; c++)
      if (m(r, c) != f(r, c)) return false;
  return true;
}

// the circle of closure_passes_host_tests: constant velocity, exact odometry, 12 exact closures in both key orders
static void test_marginals_with_12_closures() {
  const int N = 64, b = 6;
  const double dt = 0.25, w = 2 * M_PI / ((N - 1) * dt), v = 1.0, th = dt * w;
  const Pose2 step(v * dt * std::sin(th) / th, v * dt * (1 - std::cos(th)) / th, th);
  std::vector<Pose2> truth(N);
  for (int k = 0; k + 1 < N; k++) truth[k + 1] = compose(truth[k], step);
  auto Qc_model = noiseModel::Gaussian::Covariance(1.0 * Matrix::Identity(3));
  NonlinearFactorGraph graph;
  graph.add(PriorFactor<Pose2>(Symbol('x', 0), truth[0], noiseModel::Isotropic::Sigma(3, 1e-3)));
  for (int k = 0; k + 1 < N; k++) {
    graph.add(GaussianProcessPriorPose2(Symbol('x', k), Symbol('v', k), Symbol('x', k + 1), Symbol('v', k + 1), dt, Qc_model));
    graph.add(BetweenFactor<Pose2>(Symbol('x', k), Symbol('x', k + 1), step, noiseModel::Isotropic::Sigma(3, 2e-2)));
  }
  for (int k = 0; k < 12; k++) {
    const int i = k % 2 ? 5 * k + 1 : (5 * k + 33) % N, j = k % 2 ? (5 * k + 30) % N : 5 * k;
    graph.add(BetweenFactor<Pose2>(Symbol('x', i), Symbol('x', j), between(truth[i], truth[j]), noiseModel::Isotropic::Sigma(3, 1e-2)));
  }
  Values values;
  for (int k = 0; k < N; k++) { values.insert(Symbol('x', k), truth[k]); values.insert(Symbol('v', k), Vector3{v, 0, w}); }

  Marginals m(graph, values);
  int32_t info[4] = {0, 0, 0, 0};
  EXPECT(gpslam_hip_closure_info(m.handle(), info) == 0);
  EXPECT(info[0] == 12 && info[1] == 9 && info[2] == 2 && info[3] == 3);
  std::vector<double> S((size_t)N * b * b), Sn(S.size());
  EXPECT(gpslam_hip_get_marginals(m.handle(), 0, N, S.data(), Sn.data(), nullptr, nullptr) == 0);
  auto s = [&](int i, int r, int c) { return S[((size_t)i * b + r) * b + c]; };
  auto sn = [&](int i, int r, int c) { return Sn[((size_t)i * b + r) * b + c]; };
  for (int i : {0, 31, N - 1}) {
    EXPECT(same(m.marginalCovariance(Symbol('x', i)), 3, 3, [&](int r, int c) { return s(i, r, c); }));
    EXPECT(same(m.marginalCovariance(Symbol('v', i)), 3, 3, [&](int r, int c) { return s(i, 3 + r, 3 + c); }));
    for (int r = 0; r < b; r++) EXPECT(s(i, r, r) > 0.0 && std::isfinite(s(i, r, r)));
  }
  const int i = 40;
  const JointMarginal j = m.jointMarginalCovariance(KeyVector{Symbol('x', i + 1), Symbol('v', i), Symbol('x', i)});
  EXPECT(same(j(Symbol('x', i), Symbol('x', i + 1)), 3, 3, [&](int r, int c) { return sn(i, r, c); }));
  EXPECT(same(j(Symbol('x', i + 1), Symbol('x', i)), 3, 3, [&](int r, int c) { return sn(i, c, r); }));
  EXPECT(same(j(Symbol('v', i), Symbol('x', i + 1)), 3, 3, [&](int r, int c) { return sn(i, 3 + r, c); }));
  EXPECT(same(j(Symbol('v', i), Symbol('x', i)), 3, 3, [&](int r, int c) { return s(i, 3 + r, c); }));
  // the opt-in belongs to this session alone: switched off, the handle refuses again
  EXPECT(gpslam_hip_marginals_keep_closure_columns(m.handle(), 0) == 0);
  EXPECT(gpslam_hip_marginals(m.handle()) == GPSLAM_E_UNSUPPORTED);
  std::printf("12 closures, P %d: Sigma(x31) diag %.3e %.3e %.3e\n", (int)info[2], s(31, 0, 0), s(31, 1, 1), s(31, 2, 2));
}

int main(int argc, char **) {
  if (argc < 2) return gpslam_hip_marginals_keep_closure_columns(nullptr, 1) == GPSLAM_E_INVALID ? 0 : 1;   // (no device call)
  test_marginals_with_12_closures();
  if (failures) { std::printf("marginals_passes_host_tests: %d FAILED\n", failures); return 1; }
  std::printf("marginals_passes_host_tests: all tests passed\n");
  return 0;
}
