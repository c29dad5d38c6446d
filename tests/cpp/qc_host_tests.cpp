// qcStatistic of gpslam_amd/host/gpslam_host.hpp (include/gpslam_hip_qc.h).  Without an argument: the three host-arithmetic entry
// points and the NULL-handle answer -- no device call.  With one, on the GPU: the Pose2 chain of evidence_host_tests.cpp, its statistic
// at the start printed for tests/test_qc_learning_cpp.py, which builds the same graph through the Python binding; and the same chain
// with every other GP prior on a Qc_model of its own, which the statistic must leave out.
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
  const double Qc[4] = {2.0, 1.0, 1.0, 2.0}, A[4] = {40.0, 4.0, 4.0, 10.0};
  double G[4], Q1[4], theta = 0.0;
  EXPECT(gpslam_hip_qc_gradient(2, Qc, A, 5, G) == 0);
  EXPECT(G[0] == 10.0 - 20.0 && G[1] == 5.0 - 2.0 && G[2] == G[1] && G[3] == 10.0 - 5.0);
  EXPECT(gpslam_hip_qc_em_update(2, A, 5, Q1) == 0);
  EXPECT(Q1[0] == 4.0 && Q1[1] == 0.4 && Q1[2] == 0.4 && Q1[3] == 1.0);
  EXPECT(gpslam_hip_qc_gradient(2, Q1, A, 5, G) == 0 && std::fabs(G[0]) + std::fabs(G[1]) + std::fabs(G[2]) + std::fabs(G[3]) < 1e-14);
  // Qc^-1 = [[2, -1], [-1, 2]] / 3: tr(Qc^-1 A) = (80 - 4 - 4 + 20) / 3
  EXPECT(gpslam_hip_qc_em_scale(2, Qc, A, 5, &theta) == 0 && std::fabs(theta - (92.0 / 3.0) / 20.0) < 1e-14);
  const double indefinite[4] = {1.0, 2.0, 2.0, 1.0};
  EXPECT(gpslam_hip_qc_gradient(2, indefinite, A, 5, G) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_qc_em_update(2, indefinite, 5, Q1) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_qc_em_scale(2, indefinite, A, 5, &theta) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_qc_em_scale(2, Qc, indefinite, 5, &theta) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_qc_gradient(2, Qc, A, 0, G) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_qc_em_update(2, A, -1, Q1) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_qc_em_scale(2, Qc, A, 0, &theta) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_qc_gradient(2, nullptr, A, 5, G) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_qc_em_update(2, A, 5, nullptr) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_qc_em_scale(7, Qc, A, 5, &theta) == GPSLAM_E_INVALID);
  int64_t n = 0;
  EXPECT(gpslam_hip_qc_statistic(nullptr, G, &n) == GPSLAM_E_INVALID);
  QcStatistic empty;
  empty.A = Matrix(2, 2);
  bool threw = false;
  try { empty.emUpdate(); } catch (const std::invalid_argument &) { threw = true; }
  EXPECT(threw);
}

// N = 12, dt = 0.25, Qc = 0.5 I; tests/test_qc_learning_cpp.py builds the same numbers
static void test_qc_statistic_of_a_pose2_chain() {
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
  auto other_model = noiseModel::Gaussian::Covariance(2.0 * Matrix::Identity(3));
  NonlinearFactorGraph graph, mixed;
  for (NonlinearFactorGraph *g : {&graph, &mixed}) {
    g->add(PriorFactor<Pose2>(Symbol('x', 0), truth[0], noiseModel::Isotropic::Sigma(3, 1e-2)));
    for (int k = 0; k + 1 < N; k++) {
      g->add(GaussianProcessPriorPose2(Symbol('x', k), Symbol('v', k), Symbol('x', k + 1), Symbol('v', k + 1), dt, (g == &mixed && k % 2) ? other_model : Qc_model));
      g->add(BetweenFactor<Pose2>(Symbol('x', k), Symbol('x', k + 1), step, noiseModel::Isotropic::Sigma(3, 2e-2)));
    }
  }
  Values init;
  for (int k = 0; k < N; k++) {
    init.insert(Symbol('x', k), Pose2(truth[k].x + 0.03 * std::sin(0.7 * k), truth[k].y - 0.02 * std::cos(0.4 * k), truth[k].theta + 0.04 * std::sin(0.3 * k)));
    init.insert(Symbol('v', k), Vector3{v, 0, w});
  }
  const QcStatistic q = qcStatistic(graph, init);
  EXPECT(q.priors == N - 1 && q.A.rows == 3 && q.A.cols == 3);
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) EXPECT(q.A(r, c) == q.A(c, r));
  const Matrix Q1 = q.emUpdate(), G = q.gradient(Q1);
  for (int r = 0; r < 3; r++) {
    EXPECT(Q1(r, r) > 0.0);
    for (int c = 0; c < 3; c++) EXPECT(std::fabs(G(r, c)) <= 1e-12 * std::fabs(q.A(r, r)) + 1e-12 * std::fabs(q.A(c, c)));
  }
  EXPECT(std::fabs(q.emScale(Q1) - 1.0) < 1e-12);
  const QcStatistic h = qcStatistic(mixed, init);
  EXPECT(h.priors == N / 2);          // k = 0, 2, .., 10
  std::printf("qcStatistic at_start %lld", q.priors);
  for (int i = 0; i < 9; i++) std::printf(" %.17g", q.A.a[i]);
  std::printf("\n");
}

int main(int argc, char **) {
  test_host_arithmetic_and_null_handle();
  if (argc > 1) test_qc_statistic_of_a_pose2_chain();
  if (failures) { std::printf("qc_host_tests: %d FAILED\n", failures); return 1; }
  std::printf("qc_host_tests: all tests passed\n");
  return 0;
}
