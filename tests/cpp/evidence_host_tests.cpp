// logDeterminant / logEvidence of gpslam_amd/host/gpslam_host.hpp (include/gpslam_hip_evidence.h).  Without an argument: the two
// host-arithmetic entry points and the NULL-handle answers -- no device call.  With one, on the GPU: a small Pose2 chain (a prior, GP
// priors, odometry), its logEvidence printed for tests/test_evidence_cpp.py, which builds the same graph through the Python binding.
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

static void test_host_arithmetic_and_null_handle() {
  // Qc = diag(4, 9), dt = 2: det Q = (dt^4 / 12)^2 det(Qc)^2 = (16 / 12)^2 * 36^2, log|det R| = -1/2 log det Q
  const double Qc[4] = {4.0, 0.0, 0.0, 9.0};
  double out = 0.0;
  EXPECT(gpslam_hip_gp_log_normaliser(2, Qc, 2.0, &out) == 0);
  EXPECT(std::fabs(out - (-0.5 * std::log((16.0 / 12.0) * (16.0 / 12.0) * 36.0 * 36.0))) < 1e-14);
  const double full[4] = {2.0, 1.0, 1.0, 2.0};      // det 3
  EXPECT(gpslam_hip_gp_log_normaliser(2, full, 1.0, &out) == 0 && std::fabs(out - (-0.5 * (2.0 * std::log(1.0 / 12.0) + 2.0 * std::log(3.0)))) < 1e-14);
  const double indefinite[4] = {1.0, 2.0, 2.0, 1.0};
  EXPECT(gpslam_hip_gp_log_normaliser(2, indefinite, 1.0, &out) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_gp_log_normaliser(2, Qc, 0.0, &out) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_gp_log_normaliser(2, Qc, -1.0, &out) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_gp_log_normaliser(2, nullptr, 1.0, &out) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_gp_log_normaliser(2, Qc, 1.0, nullptr) == GPSLAM_E_INVALID);
  double z = 0.0;
  EXPECT(gpslam_hip_evidence_combine(1.5, 4.0, 0.25, 12, 10, &z) == 0 && std::fabs(z - (-1.5 + 0.25 - 2.0 - std::log(2.0 * M_PI))) < 1e-15);
  EXPECT(gpslam_hip_evidence_combine(0.0, 0.0, 0.0, 7, 7, &z) == 0 && z == 0.0);
  EXPECT(gpslam_hip_evidence_combine(0.0, 0.0, 0.0, 7, 7, nullptr) == GPSLAM_E_INVALID);
  double p3[3], o5[5];
  int64_t m = 0, n = 0;
  EXPECT(gpslam_hip_log_determinant(nullptr, &out, p3) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_log_noise_normaliser(nullptr, &out, &m, &n) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_log_evidence(nullptr, o5) == GPSLAM_E_INVALID);
}

// N = 12, dt = 0.25, Qc = 0.5 I; tests/test_evidence_cpp.py builds the same numbers
static void test_log_evidence_of_a_pose2_chain() {
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
  LevenbergMarquardtParams lp;
  lp.setRelativeErrorTol(1e-14);
  lp.setAbsoluteErrorTol(1e-14);
  LevenbergMarquardtOptimizer lm(graph, init, lp);
  const Values best = lm.optimize();
  const LogEvidence e = logEvidence(graph, best);
  const double ld = logDeterminant(graph, best);
  EXPECT(ld == e.logDeterminant);
  EXPECT(e.rowsMinusVariables == 3 + (N - 1) * 9 - N * 6);
  EXPECT(std::fabs(e.cost - lm.error()) <= 1e-11 * (1.0 + lm.error()));
  double z = 0.0;
  EXPECT(gpslam_hip_evidence_combine(e.cost, e.logDeterminant, e.logNoiseNormaliser, e.rowsMinusVariables, 0, &z) == 0 && z == e.logZ);
  const double at_start = logEvidence(graph, init).logZ;
  EXPECT(at_start < e.logZ);
  std::printf("logEvidence at_start %.17g\n", at_start);
  std::printf("logEvidence optimum %.17g %.17g %.17g %.17g %lld\n", e.logZ, e.cost, e.logDeterminant, e.logNoiseNormaliser, e.rowsMinusVariables);
}

int main(int argc, char **) {
  test_host_arithmetic_and_null_handle();
  if (argc > 1) test_log_evidence_of_a_pose2_chain();
  if (failures) { std::printf("evidence_host_tests: %d FAILED\n", failures); return 1; }
  std::printf("evidence_host_tests: all tests passed\n");
  return 0;
}
