// gtsam::Marginals of gpslam_amd/host/gpslam_host.hpp against the C ABI it sits on (gpslam_hip_get_marginals /
// gpslam_hip_interpolate_covariances on the same handle): the key-to-slot mapping (x, v, w, b, landmark keys; the VW family's
// [v; w] slot, the AHRS state's (rotation, bias | omega, pad)), the joint blocks of two adjacent states and landmarks, fullMatrix,
// marginalInformation, interpolatePoseCovariances, and the std::invalid_argument of a non-adjacent joint set.  Needs a GPU.
#include <cmath>
#include <cstdio>
#include <cstring>
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

struct Abi {   // the blocks as the C ABI reports them, for states [0, N)
  int N, b, nl;
  std::vector<double> S, Sn, Slm, Sxl;
  Abi(gpslam_hip_handle *h, int N_, int d, int nl_) : N(N_), b(2 * d), nl(nl_), S((size_t)N_ * 4 * d * d), Sn(S.size()),
      Slm((size_t)std::max(nl_ * nl_, 1)), Sxl((size_t)std::max(N_ * 2 * d * nl_, 1)) {
    const int rc = gpslam_hip_get_marginals(h, 0, N, S.data(), Sn.data(), nl ? Slm.data() : nullptr, nl ? Sxl.data() : nullptr);
    if (rc != 0) throw std::runtime_error("gpslam_hip_get_marginals failed");
  }
  double s(int i, int r, int c) const { return S[((size_t)i * b + r) * b + c]; }
  double sn(int i, int r, int c) const { return Sn[((size_t)i * b + r) * b + c]; }
  double sxl(int i, int r, int c) const { return Sxl[((size_t)i * b + r) * nl + c]; }
  double slm(int r, int c) const { return Slm[(size_t)r * nl + c]; }
};

// m(r, c) == f(r, c) exactly for an rows x cols block (the host class copies numbers, it computes none)
template <typename F> static bool same(const Matrix &m, int rows, int cols, F f) {
  if (m.rows != rows || m.cols != cols) return false;
  for (int r = 0; r < rows; r++)
    for (int c = 0; c < cols; c++)
      if (m(r, c) != f(r, c)) return false;
  return true;
}

static bool inverse_of(const Matrix &info, const Matrix &cov, double tol) {
  const int n = cov.rows;
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) {
      double acc = 0.0;
      for (int k = 0; k < n; k++) acc += info(i, k) * cov(k, j);
      if (std::fabs(acc - (i == j ? 1.0 : 0.0)) > tol) return false;
    }
  return true;
}

static bool throws_invalid(const std::function<void()> &f) {
  try { f(); } catch (const std::invalid_argument &) { return true; } catch (...) { return false; }
  return false;
}

// the loop-closure circle of host_api_tests (Pose2, GP priors, odometry, one closure) with two range landmarks
static void test_pose2_circle_with_closure_and_landmarks() {
  const int N = 48;
  const double dt = 0.25, w = 2 * M_PI / ((N - 1) * dt), v = 1.0;
  auto step = [&](double bias) {
    const double th = dt * (w + bias);
    return Pose2(v * dt * std::sin(th) / th, v * dt * (1 - std::cos(th)) / th, th);
  };
  auto compose = [](const Pose2 &a, const Pose2 &b) {
    return Pose2(a.x + std::cos(a.theta) * b.x - std::sin(a.theta) * b.y, a.y + std::sin(a.theta) * b.x + std::cos(a.theta) * b.y, a.theta + b.theta);
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
  const Abi a(m.handle(), N, 3, 4);
  const int i = 17;
  EXPECT(same(m.marginalCovariance(Symbol('x', i)), 3, 3, [&](int r, int c) { return a.s(i, r, c); }));
  EXPECT(same(m.marginalCovariance(Symbol('v', i)), 3, 3, [&](int r, int c) { return a.s(i, 3 + r, 3 + c); }));
  EXPECT(same(m.marginalCovariance(Symbol('l', 1)), 2, 2, [&](int r, int c) { return a.slm(2 + r, 2 + c); }));
  EXPECT(inverse_of(m.marginalInformation(Symbol('x', i)), m.marginalCovariance(Symbol('x', i)), 1e-8));
  // two adjacent states and a landmark, keys in a mixed order
  const KeyVector keys{Symbol('x', i + 1), Symbol('l', 0), Symbol('v', i), Symbol('x', i)};
  const JointMarginal j = m.jointMarginalCovariance(keys);
  EXPECT(same(j(Symbol('x', i), Symbol('x', i + 1)), 3, 3, [&](int r, int c) { return a.sn(i, r, c); }));
  EXPECT(same(j(Symbol('x', i + 1), Symbol('x', i)), 3, 3, [&](int r, int c) { return a.sn(i, c, r); }));
  EXPECT(same(j(Symbol('v', i), Symbol('x', i + 1)), 3, 3, [&](int r, int c) { return a.sn(i, 3 + r, c); }));
  EXPECT(same(j(Symbol('v', i), Symbol('x', i)), 3, 3, [&](int r, int c) { return a.s(i, 3 + r, c); }));
  EXPECT(same(j(Symbol('x', i), Symbol('l', 0)), 3, 2, [&](int r, int c) { return a.sxl(i, r, c); }));
  EXPECT(same(j(Symbol('l', 0), Symbol('x', i + 1)), 2, 3, [&](int r, int c) { return a.sxl(i + 1, c, r); }));
  EXPECT(same(j(Symbol('l', 0), Symbol('l', 0)), 2, 2, [&](int r, int c) { return a.slm(r, c); }));
  const int dims[4] = {3, 2, 3, 3};
  int off[4] = {0, 3, 5, 8};
  const Matrix &F = j.fullMatrix();
  EXPECT(F.rows == 11 && F.cols == 11);
  for (int p = 0; p < 4; p++)
    for (int q = 0; q < 4; q++)
      EXPECT(same(j(keys[p], keys[q]), dims[p], dims[q], [&](int r, int c) { return F(off[p] + r, off[q] + c); }));
  // the last state's joint with its predecessor, and the landmarks alone
  EXPECT(same(m.jointMarginalCovariance(KeyVector{Symbol('x', N - 2), Symbol('x', N - 1)})(Symbol('x', N - 2), Symbol('x', N - 1)), 3, 3,
              [&](int r, int c) { return a.sn(N - 2, r, c); }));
  EXPECT(same(m.jointMarginalCovariance(KeyVector{Symbol('l', 0), Symbol('l', 1)}).fullMatrix(), 4, 4, [&](int r, int c) { return a.slm(r, c); }));
  // non-adjacent states, unknown keys
  EXPECT(throws_invalid([&] { m.jointMarginalCovariance(KeyVector{Symbol('x', 0), Symbol('x', 2)}); }));
  EXPECT(throws_invalid([&] { m.jointMarginalCovariance(KeyVector{Symbol('x', 3), Symbol('l', 1), Symbol('v', 5)}); }));
  EXPECT(throws_invalid([&] { m.marginalCovariance(Symbol('x', N + 3)); }));
  EXPECT(throws_invalid([&] { m.jointMarginalCovariance(KeyVector{}); }));
  // interpolatePoseCovariances: what gpslam_hip_interpolate_covariances returns for the same queries (gp term on)
  const KeyVector left{Symbol('x', 3), Symbol('x', N - 2)};
  const std::vector<double> dts{dt, dt}, taus{0.1, 0.2};
  const std::vector<Matrix> P = m.interpolatePoseCovariances(left, dts, taus);
  std::vector<double> ref(2 * 9);
  const int32_t idx[2] = {3, N - 2};
  EXPECT(gpslam_hip_interpolate_covariances(m.handle(), 2, idx, dts.data(), taus.data(), 1, ref.data()) == 0);
  EXPECT(P.size() == 2);
  for (int q = 0; q < 2 && P.size() == 2; q++) EXPECT(same(P[q], 3, 3, [&](int r, int c) { return ref[q * 9 + r * 3 + c]; }));
  std::printf("pose2 circle: Sigma(x%d) diag %.3e %.3e %.3e\n", i, a.s(i, 0, 0), a.s(i, 1, 1), a.s(i, 2, 2));
}

// Pose3VW: 'v' keys are the first three coordinates of the velocity slot, 'w' keys the last three ([v; w] as stored)
static void test_pose3vw_slots() {
  const int N = 5;
  auto Qc_model = noiseModel::Gaussian::Covariance(0.01 * Matrix::Identity(6));
  NonlinearFactorGraph graph;
  Values init;
  for (int k = 1; k <= N; k++) {
    const Pose3 p(Rot3(), Point3(k - 1.0, 0, 0));
    graph.add(PriorFactor<Pose3>(Symbol('x', k), p, noiseModel::Isotropic::Sigma(6, 0.01)));
    init.insert(Symbol('x', k), p);
    init.insert(Symbol('v', k), Vector3{1, 0, 0});
    init.insert(Symbol('w', k), Vector3{0, 0, 0});
    if (k < N)
      graph.add(GaussianProcessPriorPose3VW(Symbol('x', k), Symbol('v', k), Symbol('w', k), Symbol('x', k + 1), Symbol('v', k + 1),
                                            Symbol('w', k + 1), 1.0, Qc_model));
  }
  Marginals m(graph, init);
  const Abi a(m.handle(), N, 6, 0);
  const int i = 2;   // state index of key 3
  EXPECT(same(m.marginalCovariance(Symbol('x', 3)), 6, 6, [&](int r, int c) { return a.s(i, r, c); }));
  EXPECT(same(m.marginalCovariance(Symbol('v', 3)), 3, 3, [&](int r, int c) { return a.s(i, 6 + r, 6 + c); }));
  EXPECT(same(m.marginalCovariance(Symbol('w', 3)), 3, 3, [&](int r, int c) { return a.s(i, 9 + r, 9 + c); }));
  const JointMarginal j = m.jointMarginalCovariance(KeyVector{Symbol('w', 3), Symbol('v', 4)});
  EXPECT(same(j(Symbol('w', 3), Symbol('v', 4)), 3, 3, [&](int r, int c) { return a.sn(i, 9 + r, 6 + c); }));
  EXPECT(same(j(Symbol('v', 4), Symbol('w', 3)), 3, 3, [&](int r, int c) { return a.sn(i, 9 + c, 6 + r); }));
  EXPECT(throws_invalid([&] { m.jointMarginalCovariance(KeyVector{Symbol('w', 1), Symbol('v', 3)}); }));
}

// the AHRS state (GPSLAM_ROT3_BIAS): x -> rotation (0..2), b -> bias (3..5), v -> angular velocity (6..8); the pads are no key
static void test_ahrs_bias_slots() {
  const int N = 12;
  const double dt = 0.01;
  auto Qc_model = noiseModel::Gaussian::Covariance(1e4 * Matrix::Identity(3));
  Matrix gyro_cov = 1e-3 * Matrix::Identity(3);
  NonlinearFactorGraph graph;
  Values init;
  graph.add(PriorFactor<Rot3>(Symbol('x', 1), Rot3(), noiseModel::Isotropic::Sigma(3, 0.1)));
  graph.add(PriorFactor<Vector3>(Symbol('b', 1), Vector3{0, 0, 0}, noiseModel::Isotropic::Sigma(3, 1e-2)));
  graph.add(PriorFactor<Vector3>(Symbol('v', 1), Vector3{0.3, -0.2, 0.5}, noiseModel::Isotropic::Sigma(3, 1.0)));
  for (int k = 1; k < N; k++) {
    PreintegratedAhrsMeasurements pim(Vector3{0, 0, 0}, gyro_cov);
    for (int q = 0; q < 2; q++) pim.integrateMeasurement(Vector3{0.3, -0.2, 0.5}, dt / 2);
    graph.add(AHRSFactor(Symbol('x', k), Symbol('x', k + 1), Symbol('b', k), pim));
    graph.add(BetweenFactor<Vector3>(Symbol('b', k), Symbol('b', k + 1), Vector3{0, 0, 0}, noiseModel::Isotropic::Sigma(3, 1e-4)));
    graph.add(GaussianProcessPriorRot3(Symbol('x', k), Symbol('v', k), Symbol('x', k + 1), Symbol('v', k + 1), dt, Qc_model));
  }
  for (int k = 1; k <= N; k++) {
    init.insert(Symbol('x', k), Rot3());
    init.insert(Symbol('b', k), Vector3{0, 0, 0});
    init.insert(Symbol('v', k), Vector3{0.3, -0.2, 0.5});
  }
  Marginals m(graph, init);
  const Abi a(m.handle(), N, 6, 0);
  const int i = 4;   // key 5
  EXPECT(same(m.marginalCovariance(Symbol('x', 5)), 3, 3, [&](int r, int c) { return a.s(i, r, c); }));
  EXPECT(same(m.marginalCovariance(Symbol('b', 5)), 3, 3, [&](int r, int c) { return a.s(i, 3 + r, 3 + c); }));
  EXPECT(same(m.marginalCovariance(Symbol('v', 5)), 3, 3, [&](int r, int c) { return a.s(i, 6 + r, 6 + c); }));
  const JointMarginal j = m.jointMarginalCovariance(KeyVector{Symbol('b', 5), Symbol('x', 6), Symbol('v', 5)});
  EXPECT(same(j(Symbol('b', 5), Symbol('x', 6)), 3, 3, [&](int r, int c) { return a.sn(i, 3 + r, c); }));
  EXPECT(same(j(Symbol('x', 6), Symbol('v', 5)), 3, 3, [&](int r, int c) { return a.sn(i, 6 + c, r); }));
  EXPECT(same(j(Symbol('v', 5), Symbol('b', 5)), 3, 3, [&](int r, int c) { return a.s(i, 6 + r, 3 + c); }));
  for (int r = 9; r < 12; r++)      // the pads: zero rows in the ABI's blocks
    for (int c = 0; c < 12; c++) EXPECT(a.s(i, r, c) == 0.0 && a.s(i, c, r) == 0.0 && a.sn(i, r, c) == 0.0 && a.sn(i, c, r) == 0.0);
  EXPECT(inverse_of(m.marginalInformation(Symbol('b', 5)), m.marginalCovariance(Symbol('b', 5)), 1e-8));
  EXPECT(throws_invalid([&] { m.jointMarginalCovariance(KeyVector{Symbol('x', 1), Symbol('b', 3)}); }));
}

int main() {
  test_pose2_circle_with_closure_and_landmarks();
  test_pose3vw_slots();
  test_ahrs_bias_slots();
  if (failures == 0) std::printf("marginals_host_tests: all tests passed\n");
  return failures == 0 ? 0 : 1;
}
