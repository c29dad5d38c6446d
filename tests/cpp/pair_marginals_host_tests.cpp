// gtsam::Marginals over ANY states (gpslam_amd/host/gpslam_host.hpp: Marginals::serveAnyStates, Marginals::betweenChiSquared) on the
// Pose2 circle of marginals_host_tests.cpp (GP priors, odometry, one loop closure, two range landmarks).  By default a joint set
// over non-adjacent states still throws; after the opt-in its blocks are compared, number by number, with
// gpslam_hip_get_state_pair_marginals and the landmark getters on the class's handle, and the gate with gpslam_hip_gate_between_pairs.
// Without an argument the program only proves that it links (no device call); with one it runs on the GPU.
#include <cmath>
#include <cstdio>
#include <functional>
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

template <typename F> static bool same(const Matrix &m, int rows, int cols, F f) {
  if (m.rows != rows || m.cols != cols) return false;
  for (int r = 0; r < rows; r++)
    for (int c = 0; c < cols; c++)
      if (m(r, c) != f(r, c)) return false;
  return true;
}
static bool throws_invalid(const std::function<void()> &f) {
  try { f(); } catch (const std::invalid_argument &) { return true; } catch (...) { return false; }
  return false;
}

static void test_any_states_and_the_gate() {
  const int N = 48, b = 6, ld = 2;
  const double dt = 0.25, w = 2 * M_PI / ((N - 1) * dt), v = 1.0;
  auto step = [&](double bias) {
    const double th = dt * (w + bias);
    return Pose2(v * dt * std::sin(th) / th, v * dt * (1 - std::cos(th)) / th, th);
  };
  auto compose = [](const Pose2 &a, const Pose2 &c) {
    return Pose2(a.x + std::cos(a.theta) * c.x - std::sin(a.theta) * c.y, a.y + std::sin(a.theta) * c.x + std::cos(a.theta) * c.y, a.theta + c.theta);
  };
  std::vector<Pose2> truth(N);
  for (int k = 0; k + 1 < N; k++) truth[k + 1] = compose(truth[k], step(0.0));
  const Point2 land[2] = {Point2(0.5, 2.5), Point2(-1.0, 1.0)};
  auto Qc_model = noiseModel::Gaussian::Covariance(1.0 * Matrix::Identity(3));
  NonlinearFactorGraph graph;
  graph.add(PriorFactor<Pose2>(Symbol('x', 0), truth[0], noiseModel::Isotropic::Sigma(3, 1e-3)));
  for (int k = 0; k + 1 < N; k++) {
    graph.add(GaussianProcessPriorPose2(Symbol('x', k), Symbol('v', k), Symbol('x', k + 1), Symbol('v', k + 1), dt, Qc_model));
    graph.add(BetweenFactor<Pose2>(Symbol('x', k), Symbol('x', k + 1), step(0.02), noiseModel::Isotropic::Sigma(3, 2e-2)));
  }
  graph.add(BetweenFactor<Pose2>(Symbol('x', N - 1), Symbol('x', 0), Pose2(0, 0, -2 * M_PI), noiseModel::Isotropic::Sigma(3, 1e-3)));
  for (int k = 0; k < N; k += 2)
    for (int l = 0; l < 2; l++)
      graph.add(RangeFactorPose2(Symbol('x', k), Symbol('l', l), std::hypot(truth[k].x - land[l].x, truth[k].y - land[l].y),
                                 noiseModel::Isotropic::Sigma(1, 0.05)));
  Values init;
  for (int k = 0; k < N; k++) { init.insert(Symbol('x', k), truth[k]); init.insert(Symbol('v', k), Vector3{v, 0, w}); }
  for (int l = 0; l < 2; l++) init.insert(Symbol('l', l), Point2(land[l].x + 0.05, land[l].y - 0.05));
  Values opt = GaussNewtonOptimizer(graph, init).optimize();

  Marginals m(graph, opt);
  // the default: non-adjacent states are refused, by the class and (landmarks and a closure, no opt-in) by the C getter
  EXPECT(throws_invalid([&] { m.jointMarginalCovariance(KeyVector{Symbol('x', 0), Symbol('x', 2)}); }));
  const int32_t i0 = 0, i2 = 2;
  std::vector<double> blk((size_t)b * b);
  EXPECT(gpslam_hip_get_state_pair_marginals(m.handle(), 1, &i0, &i2, blk.data()) == GPSLAM_E_INVALID);
  EXPECT(throws_invalid([&] { m.betweenChiSquared(Symbol('x', 3), Symbol('x', 40), Pose2(0, 0, 0), Vector{0.1, 0.1, 0.1}); }));

  m.serveAnyStates();
  const int32_t st[3] = {0, 7, 31};
  std::vector<int32_t> sa, sb;
  for (int u = 0; u < 3; u++)
    for (int q = 0; q < 3; q++) { sa.push_back(st[u]); sb.push_back(st[q]); }
  std::vector<double> SS((size_t)9 * b * b), XL((size_t)3 * b * ld), LL((size_t)ld * ld);
  EXPECT(gpslam_hip_get_state_pair_marginals(m.handle(), 9, sa.data(), sb.data(), SS.data()) == 0);
  const int32_t l1[3] = {1, 1, 1};
  EXPECT(gpslam_hip_get_state_landmark_marginals(m.handle(), 3, st, l1, XL.data()) == 0);
  EXPECT(gpslam_hip_get_landmark_pair_marginals(m.handle(), 1, l1, l1, LL.data()) == 0);
  auto ss = [&](int u, int q, int r, int c) { return SS[(((size_t)u * 3 + q) * b + r) * b + c]; };
  auto xl = [&](int u, int r, int c) { return XL[((size_t)u * b + r) * ld + c]; };

  const Key x0 = Symbol('x', 0), v7 = Symbol('v', 7), x31 = Symbol('x', 31), lm = Symbol('l', 1);
  const JointMarginal j = m.jointMarginalCovariance(KeyVector{x0, v7, x31, lm});
  EXPECT(j.fullMatrix().rows == 11 && j.fullMatrix().cols == 11);
  EXPECT(same(j(x0, x0), 3, 3, [&](int r, int c) { return ss(0, 0, r, c); }));
  EXPECT(same(j(x0, v7), 3, 3, [&](int r, int c) { return ss(0, 1, r, 3 + c); }));
  EXPECT(same(j(v7, x0), 3, 3, [&](int r, int c) { return ss(1, 0, 3 + r, c); }));
  EXPECT(same(j(x0, x31), 3, 3, [&](int r, int c) { return ss(0, 2, r, c); }));
  EXPECT(same(j(x31, x0), 3, 3, [&](int r, int c) { return ss(2, 0, r, c); }));
  EXPECT(same(j(x31, x0), 3, 3, [&](int r, int c) { return ss(0, 2, c, r); }));     // the transpose, to the bit
  EXPECT(same(j(v7, x31), 3, 3, [&](int r, int c) { return ss(1, 2, 3 + r, c); }));
  EXPECT(same(j(v7, v7), 3, 3, [&](int r, int c) { return ss(1, 1, 3 + r, 3 + c); }));
  EXPECT(same(j(x31, lm), 3, 2, [&](int r, int c) { return xl(2, r, c); }));
  EXPECT(same(j(lm, v7), 2, 3, [&](int r, int c) { return xl(1, 3 + c, r); }));
  EXPECT(same(j(lm, lm), 2, 2, [&](int r, int c) { return LL[(size_t)r * ld + c]; }));
  bool nonzero = false;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) nonzero = nonzero || j(x0, x31)(r, c) != 0.0;
  EXPECT(nonzero);
  // sets the default serves are what they were
  EXPECT(same(m.marginalCovariance(x31), 3, 3, [&](int r, int c) { return ss(2, 2, r, c); }));

  // the gate: a candidate between x3 and x40
  const int32_t f = 3, s = 40;
  const Pose2 measured(0.1, -0.2, 0.05);
  const Vector sig{0.05, 0.05, 0.02};
  const double meas[3] = {measured.x, measured.y, measured.theta};
  double chi2 = -1.0;
  EXPECT(gpslam_hip_gate_between_pairs(m.handle(), 1, &f, &s, meas, sig.data(), &chi2, nullptr, nullptr) == 0);
  const double got = m.betweenChiSquared(Symbol('x', 3), Symbol('x', 40), measured, sig);
  EXPECT(got == chi2 && chi2 > 0.0 && std::isfinite(chi2));
  EXPECT(throws_invalid([&] { m.betweenChiSquared(Symbol('x', 3), Symbol('x', 3), measured, sig); }));
  EXPECT(throws_invalid([&] { m.betweenChiSquared(Symbol('x', 3), Symbol('x', 40), measured, Vector{0.1, 0.1}); }));
  std::printf("Sigma(x0, x31)[0][0] %.3e, chi2 of the candidate (3, 40) %.3e\n", ss(0, 2, 0, 0), chi2);
}

// the straight SE(2) chain with 24 locally visible landmarks of segmented_marginals_host_tests.cpp: the session takes the segmented
// landmark path, where serveAnyStates() throws and the set over non-adjacent states stays refused
static void test_segmented_session_refuses() {
  const int N = 240, L = 24, span = 20;
  const double dt = 0.1, v = 1.0;
  std::vector<Pose2> truth(N);
  for (int k = 0; k < N; k++) truth[k] = Pose2(v * dt * k, 0.0, 0.0);
  std::vector<Point2> land(L);
  std::vector<int> centre(L);
  for (int l = 0; l < L; l++) {
    centre[l] = (int)((l + 0.5) * N / L);
    land[l] = Point2(truth[centre[l]].x, (l % 2 ? -1.0 : 1.0) * (3.0 + 0.25 * (l % 5)));
  }
  auto Qc_model = noiseModel::Gaussian::Covariance(1.0 * Matrix::Identity(3));
  NonlinearFactorGraph graph;
  graph.add(PriorFactor<Pose2>(Symbol('x', 0), truth[0], noiseModel::Isotropic::Sigma(3, 1e-2)));
  for (int k = 0; k + 1 < N; k++) {
    graph.add(GaussianProcessPriorPose2(Symbol('x', k), Symbol('v', k), Symbol('x', k + 1), Symbol('v', k + 1), dt, Qc_model));
    graph.add(BetweenFactor<Pose2>(Symbol('x', k), Symbol('x', k + 1), Pose2(v * dt, 0, 0), noiseModel::Isotropic::Sigma(3, 5e-2)));
  }
  for (int l = 0; l < L; l++)
    for (int k = std::max(centre[l] - span, 0); k <= std::min(centre[l] + span, N - 1); k += 2)
      graph.add(RangeFactorPose2(Symbol('x', k), Symbol('l', l), std::hypot(truth[k].x - land[l].x, truth[k].y - land[l].y),
                                 noiseModel::Isotropic::Sigma(1, 0.05)));
  Values values;
  for (int k = 0; k < N; k++) { values.insert(Symbol('x', k), truth[k]); values.insert(Symbol('v', k), Vector3{v, 0, 0}); }
  for (int l = 0; l < L; l++) values.insert(Symbol('l', l), land[l]);

  Marginals m(graph, values);
  int32_t plan[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  EXPECT(gpslam_hip_segment_plan(m.handle(), plan) == 0);
  EXPECT(plan[0] == 1);
  EXPECT(throws_invalid([&] { m.serveAnyStates(); }));
  EXPECT(throws_invalid([&] { m.jointMarginalCovariance(KeyVector{Symbol('x', 0), Symbol('x', 2)}); }));
  EXPECT(m.marginalCovariance(Symbol('x', 5)).rows == 3);      // what was served stays served
  const int32_t i0 = 0, i2 = 2;
  std::vector<double> blk(36);
  EXPECT(gpslam_hip_get_state_pair_marginals(m.handle(), 1, &i0, &i2, blk.data()) == GPSLAM_E_UNSUPPORTED);
}

int main(int argc, char **) {
  if (argc < 2) {      // (no device call)
    return gpslam_hip_marginals_keep_pair_terms(nullptr, 1) == GPSLAM_E_INVALID &&
           gpslam_hip_get_state_pair_marginals(nullptr, 0, nullptr, nullptr, nullptr) == GPSLAM_E_INVALID &&
           gpslam_hip_gate_between_pairs(nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == GPSLAM_E_INVALID ? 0 : 1;
  }
  test_any_states_and_the_gate();
  test_segmented_session_refuses();
  if (failures) { std::printf("pair_marginals_host_tests: %d FAILED\n", failures); return 1; }
  std::printf("pair_marginals_host_tests: all tests passed\n");
  return 0;
}
