// gtsam::LinearContainerFactor over (x, v) and gtsam::BatchFixedLagSmoother of gpslam_amd/host/gpslam_host.hpp.  A GaussianProcessPriorLinear<3>
// chain with position fixes: (1) a block-diagonal LinearContainerFactor is the PriorFactor pair it restates (same graph error, same
// Levenberg-Marquardt result); (2) the smoother, fed four states per update with a lag of eight intervals, ends with the batch
// optimum's last states -- the problem is linear, so the marginal it carries is exact; (3) a key that is older than the lag without
// being at the head of the chain throws, and so do states that do not continue the chain; (4) a refusal of the ABI -- a head factor
// that ranges a landmark -- throws with the ABI's message.  Without an argument the program only proves that it links (NULL-handle
// checks, no device call); with one it runs on the GPU.
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../gpslam_amd/host/gpslam_host.hpp"

using namespace gtsam;
using namespace gpslam;

static int failures = 0;
#define EXPECT(cond)                                                                  \
  do {                                                                                \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
  } while (0)

static const int N = 28;
static const double dt = 0.1;
static Vector3 truth_x(int k) { return Vector3{0.5 * k * dt, std::sin(0.3 * k * dt), 0.1 * k * dt * k * dt}; }
static Vector3 init_x(int k) { const Vector3 t = truth_x(k); return Vector3{t[0] + 0.05 * std::sin(1.7 * k), t[1] - 0.04 * std::cos(0.9 * k), t[2] + 0.03 * std::sin(2.3 * k + 1)}; }
static Vector3 init_v(int k) { return Vector3{0.5 + 0.02 * std::cos(1.1 * k), 0.3 * std::cos(0.3 * k * dt), 0.2 * k * dt}; }

// the factors that touch only states lo .. hi - 1 and at least one state >= from
static NonlinearFactorGraph factors(int lo, int hi, int from) {
  auto Qc_model = noiseModel::Gaussian::Covariance(0.5 * Matrix::Identity(3));
  NonlinearFactorGraph g;
  for (int k = lo; k < hi; k++) {
    if (k >= from && k % 3 == 0) g.add(PriorFactor<Vector3>(Symbol('x', k), truth_x(k), noiseModel::Isotropic::Sigma(3, k == 0 ? 1e-2 : 5e-2)));
    if (k >= from && k == 0) g.add(PriorFactor<Vector3>(Symbol('v', 0), init_v(0), noiseModel::Isotropic::Sigma(3, 1e-1)));
    if (k + 1 < hi && k + 1 >= from)
      g.add(GaussianProcessPriorLinear<3>(Symbol('x', k), Symbol('v', k), Symbol('x', k + 1), Symbol('v', k + 1), dt, Qc_model));
  }
  return g;
}
static Values initial(int lo, int hi) {
  Values v;
  for (int k = lo; k < hi; k++) { v.insert(Symbol('x', k), init_x(k)); v.insert(Symbol('v', k), init_v(k)); }
  return v;
}
static LevenbergMarquardtParams tight() {
  LevenbergMarquardtParams p;
  p.maxIterations = 40; p.relativeErrorTol = 1e-15; p.absoluteErrorTol = 1e-15; p.lambdaInitial = 1e-9;
  return p;
}
template <typename F> static bool throws_invalid(F f) {
  try { f(); } catch (const std::invalid_argument &e) { std::printf("  (thrown: %s)\n", e.what()); return true; } catch (...) { return false; }
  return false;
}

static void test_container_factor_is_the_prior_pair() {
  NonlinearFactorGraph a = factors(0, 8, 0), b = factors(0, 8, 0);
  const Vector3 mx{0.3, -0.2, 0.1}, mv{0.4, 0.1, -0.3};
  const double sx = 0.07, sv = 0.2;
  a.add(PriorFactor<Vector3>(Symbol('x', 5), mx, noiseModel::Isotropic::Sigma(3, sx)));
  a.add(PriorFactor<Vector3>(Symbol('v', 5), mv, noiseModel::Isotropic::Sigma(3, sv)));
  Matrix A(6, 6);
  for (int i = 0; i < 3; i++) { A(i, i) = 1.0 / sx; A(3 + i, 3 + i) = 1.0 / sv; }
  b.add(LinearContainerFactor(Symbol('x', 5), Symbol('v', 5), A, Vector(6, 0.0), mx, mv));
  const Values v0 = initial(0, 8);
  const double ea = a.error(v0), eb = b.error(v0);
  EXPECT(std::fabs(ea - eb) <= 1e-12 * ea);
  LevenbergMarquardtOptimizer oa(a, v0, tight()), ob(b, v0, tight());
  const Values ra = oa.optimize(), rb = ob.optimize();
  double worst = 0.0;
  for (int k = 0; k < 8; k++)
    for (int c = 0; c < 3; c++) {
      worst = std::max(worst, std::fabs(ra.at<Vector3>(Symbol('x', k))[c] - rb.at<Vector3>(Symbol('x', k))[c]));
      worst = std::max(worst, std::fabs(ra.at<Vector3>(Symbol('v', k))[c] - rb.at<Vector3>(Symbol('v', k))[c]));
    }
  std::printf("container factor against the prior pair: error %.6e / %.6e, states differ by %.3e\n", ea, eb, worst);
  EXPECT(worst <= 1e-9);
  EXPECT(throws_invalid([&] { LinearContainerFactor(Symbol('x', 1), Symbol('v', 1), Matrix(6, 5), Vector(6, 0.0), mx, mv); }));
}

static void test_smoother_ends_at_the_batch_optimum() {
  LevenbergMarquardtOptimizer batch(factors(0, N, 0), initial(0, N), tight());
  const Values want = batch.optimize();
  BatchFixedLagSmoother smoother(8 * dt + 0.5 * dt, tight());
  int hi = 0, dropped = 0;
  for (int step = 0; hi < N; step++) {
    const int lo = hi;
    hi = std::min(N, hi + (step == 0 ? 12 : 4));
    BatchFixedLagSmoother::KeyTimestampMap stamps;
    for (int k = lo; k < hi; k++) { stamps[Symbol('x', k)] = k * dt; stamps[Symbol('v', k)] = k * dt; }
    const BatchFixedLagSmoother::Result r = smoother.update(factors(0, hi, lo), initial(lo, hi), stamps);
    dropped += r.marginalized;
    EXPECT(std::isfinite(r.error));
  }
  const Values got = smoother.calculateEstimate();
  EXPECT(dropped == N - 9);
  EXPECT(!got.exists(Symbol('x', N - 10)) && got.exists(Symbol('x', N - 9)) && got.size() == 18);
  double worst = 0.0;
  for (int k = N - 9; k < N; k++)
    for (int c = 0; c < 3; c++) {
      worst = std::max(worst, std::fabs(got.at<Vector3>(Symbol('x', k))[c] - want.at<Vector3>(Symbol('x', k))[c]));
      worst = std::max(worst, std::fabs(got.at<Vector3>(Symbol('v', k))[c] - want.at<Vector3>(Symbol('v', k))[c]));
    }
  std::printf("smoother against batch over the last 9 states: %.3e\n", worst);
  EXPECT(worst <= 1e-8);
  double Lam[36], gam[6];
  EXPECT(gpslam_hip_get_head_prior(smoother.handle(), nullptr, nullptr, Lam, gam) == 0);
  EXPECT(Lam[0] > 0.0 && std::fabs(Lam[1] - Lam[6]) <= 1e-9 * Lam[0]);
}

static void test_a_key_that_is_not_at_the_head_throws() {
  BatchFixedLagSmoother smoother(4 * dt, tight());
  BatchFixedLagSmoother::KeyTimestampMap stamps;
  for (int k = 0; k < 8; k++) stamps[Symbol('x', k)] = k * dt;
  stamps[Symbol('x', 5)] = 0.0;       // older than the lag, behind younger states
  EXPECT(throws_invalid([&] { smoother.update(factors(0, 8, 0), initial(0, 8), stamps); }));
  // new states that do not continue the chain
  BatchFixedLagSmoother s2(100.0, tight());
  s2.update(factors(4, 8, 4), initial(4, 8), BatchFixedLagSmoother::KeyTimestampMap());
  EXPECT(throws_invalid([&] { s2.update(NonlinearFactorGraph(), initial(2, 3), BatchFixedLagSmoother::KeyTimestampMap()); }));
}

// a refusal of the ABI reaches the caller as std::invalid_argument with the ABI's own text: a Pose2 chain whose state 1 ranges a
// landmark, and a lag that sends states 0 .. 2 into the head (gpslam_hip_marginalize_head: GPSLAM_E_UNSUPPORTED, names the factor)
static void test_a_refusal_of_the_abi_throws_with_its_message() {
  const int n = 8;
  auto Qc_model = noiseModel::Gaussian::Covariance(1.0 * Matrix::Identity(3));
  const Point2 land(1.0, 2.0);
  NonlinearFactorGraph g;
  Values v;
  BatchFixedLagSmoother::KeyTimestampMap stamps;
  g.add(PriorFactor<Pose2>(Symbol('x', 0), Pose2(0, 0, 0), noiseModel::Isotropic::Sigma(3, 1e-2)));
  for (int k = 0; k < n; k++) {
    const Pose2 x(0.1 * k, 0.0, 0.0);
    v.insert(Symbol('x', k), x);
    v.insert(Symbol('v', k), Vector3{1.0, 0.0, 0.0});
    stamps[Symbol('x', k)] = k * dt;
    if (k + 1 < n) g.add(GaussianProcessPriorPose2(Symbol('x', k), Symbol('v', k), Symbol('x', k + 1), Symbol('v', k + 1), dt, Qc_model));
    if (k % 2 == 1) g.add(RangeFactorPose2(Symbol('x', k), Symbol('l', 0), std::hypot(x.x - land.x, x.y - land.y), noiseModel::Isotropic::Sigma(1, 0.05)));
  }
  v.insert(Symbol('l', 0), Point2(1.1, 1.9));
  BatchFixedLagSmoother smoother(4 * dt + 0.5 * dt, tight());
  std::string text;
  try { smoother.update(g, v, stamps); } catch (const std::invalid_argument &e) { text = e.what(); }
  std::printf("  (thrown: %s)\n", text.c_str());
  EXPECT(text.find("marginalize_head failed (-5)") != std::string::npos);
  EXPECT(text.find("factor 0 (state 1) is in the head and names landmark 0") != std::string::npos);
  EXPECT(text.find(gpslam_hip_last_error(smoother.handle())) != std::string::npos);
}

int main(int argc, char **) {
  if (argc < 2)   // (no device call: the NULL-handle checks)
    return (gpslam_hip_marginalize_head(nullptr, 1) == GPSLAM_E_INVALID && gpslam_hip_get_head_prior(nullptr, nullptr, nullptr, nullptr, nullptr) == GPSLAM_E_INVALID &&
            gpslam_hip_append_states(nullptr, 0, nullptr, nullptr) == GPSLAM_E_INVALID &&
            gpslam_hip_add_state_gaussians(nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == GPSLAM_E_INVALID &&
            gpslam_hip_get_state_gaussians(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == GPSLAM_E_INVALID && BatchFixedLagSmoother(1.0).smootherLag() == 1.0) ? 0 : 1;
  test_container_factor_is_the_prior_pair();
  test_smoother_ends_at_the_batch_optimum();
  test_a_key_that_is_not_at_the_head_throws();
  test_a_refusal_of_the_abi_throws_with_its_message();
  if (failures) { std::printf("fixed_lag_host_tests: %d FAILED\n", failures); return 1; }
  std::printf("fixed_lag_host_tests: all tests passed\n");
  return 0;
}
