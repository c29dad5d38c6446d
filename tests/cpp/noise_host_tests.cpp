// measNoiseStatistic of gpslam_amd/host/gpslam_host.hpp (include/gpslam_hip_noise.h).  Without an argument: the three host-arithmetic
// entry points and the NULL-handle answers -- no device call.  With one, on the GPU: a 2-D linear chain with odometry factors, its
// statistic at the start printed for tests/test_noise_learning_cpp.py, which builds the same graph through the Python binding.
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
  const double C[4] = {2.0, 1.0, 1.0, 2.0}, B[4] = {40.0, 4.0, 4.0, 10.0};
  double G[4], C1[4], ratio = 0.0, rows[2];
  EXPECT(gpslam_hip_noise_gradient(2, C, B, 5, G) == 0);
  EXPECT(G[0] == 0.5 * (10.0 - 40.0) && G[1] == 0.5 * (5.0 - 4.0) && G[2] == G[1] && G[3] == 0.5 * (10.0 - 10.0));
  EXPECT(gpslam_hip_noise_em_update(2, B, 5, C1) == 0);
  EXPECT(C1[0] == 8.0 && C1[1] == 0.8 && C1[2] == 0.8 && C1[3] == 2.0);
  EXPECT(gpslam_hip_noise_gradient(2, C1, B, 5, G) == 0 && std::fabs(G[0]) + std::fabs(G[1]) + std::fabs(G[2]) + std::fabs(G[3]) < 1e-14);
  EXPECT(gpslam_hip_noise_em_scale(2, B, 5, &ratio, rows) == 0 && ratio == 5.0 && rows[0] == 8.0 && rows[1] == 2.0);
  EXPECT(gpslam_hip_noise_em_scale(2, B, 5, &ratio, nullptr) == 0);
  const double indefinite[4] = {1.0, 2.0, 2.0, 1.0};
  EXPECT(gpslam_hip_noise_gradient(2, indefinite, B, 5, G) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_noise_em_update(2, indefinite, 5, C1) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_noise_em_scale(2, indefinite, 5, &ratio, rows) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_noise_gradient(2, C, B, 0, G) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_noise_em_update(2, B, -1, C1) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_noise_em_scale(2, B, 0, &ratio, rows) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_noise_gradient(2, nullptr, B, 5, G) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_noise_em_update(2, B, 5, nullptr) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_noise_em_scale(4, B, 5, &ratio, rows) == GPSLAM_E_INVALID);
  int64_t n = 0;
  EXPECT(gpslam_hip_meas_noise_statistic(nullptr, GPSLAM_MEAS_ODOMETRY2D, nullptr, G, C1, &n) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_meas_predicted_covariances(nullptr, GPSLAM_MEAS_ODOMETRY2D, G) == GPSLAM_E_INVALID);
  MeasNoiseStatistic empty;
  empty.B = Matrix(2, 2);
  empty.Bw = Matrix(2, 2);
  bool threw = false;
  try { empty.emUpdate(); } catch (const std::invalid_argument &) { threw = true; }
  EXPECT(threw);
}

// N = 12, dt = 0.25, Qc = 0.5 I; tests/test_noise_learning_cpp.py builds the same numbers
static void test_statistic_of_a_linear_chain_with_odometry() {
  const int N = 12;
  const double dt = 0.25;
  auto Qc_model = noiseModel::Gaussian::Covariance(0.5 * Matrix::Identity(3));
  NonlinearFactorGraph graph;
  Values init;
  graph.add(PriorFactor<Vector3>(Symbol('x', 0), Vector3{0, 0, 0}, noiseModel::Isotropic::Sigma(3, 1e-2)));
  for (int k = 0; k < N; k++) {
    init.insert(Symbol('x', k), Vector3{0.25 * k + 0.03 * std::sin(0.7 * k), 0.1 * k - 0.02 * std::cos(0.4 * k), 0.05 * k + 0.04 * std::sin(0.3 * k)});
    init.insert(Symbol('v', k), Vector3{1.0, 0.4, 0.2});
  }
  for (int k = 0; k + 1 < N; k++) {
    graph.add(GaussianProcessPriorLinear<3>(Symbol('x', k), Symbol('v', k), Symbol('x', k + 1), Symbol('v', k + 1), dt, Qc_model));
    Vector sig(3);
    sig[0] = 0.05 + 0.01 * k; sig[1] = 0.08; sig[2] = 0.02 + 0.005 * k;
    graph.add(OdometryFactor2DLinear(Symbol('x', k), Symbol('x', k + 1), Vector3{0.26, 0.02 * k, 0.05}, noiseModel::Diagonal::Sigmas(sig)));
  }
  const MeasNoiseStatistic q = measNoiseStatistic(graph, init, GPSLAM_MEAS_ODOMETRY2D);
  EXPECT(q.factors == N - 1 && q.B.rows == 3 && q.B.cols == 3);
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) EXPECT(q.B(r, c) == q.B(c, r) && q.Bw(r, c) == q.Bw(c, r));
  const Matrix C1 = q.emUpdate(), G = q.gradient(C1);
  for (int r = 0; r < 3; r++) {
    EXPECT(C1(r, r) > 0.0);
    for (int c = 0; c < 3; c++) EXPECT(std::fabs(G(r, c)) <= 1e-12 * std::fabs(q.B(r, r)) + 1e-12 * std::fabs(q.B(c, c)));
  }
  std::vector<double> rows;
  const double ratio = q.emScale(&rows);
  EXPECT(rows.size() == 3 && std::fabs(ratio - (rows[0] + rows[1] + rows[2]) / 3.0) <= 1e-14 * ratio);
  EXPECT(measNoiseStatistic(graph, init, GPSLAM_MEAS_RANGE).factors == 0);
  std::printf("measNoiseStatistic at_start %lld", q.factors);
  for (int i = 0; i < 9; i++) std::printf(" %.17g", q.B.a[i]);
  for (int i = 0; i < 9; i++) std::printf(" %.17g", q.Bw.a[i]);
  std::printf("\n");
}

int main(int argc, char **) {
  test_host_arithmetic_and_null_handle();
  if (argc > 1) test_statistic_of_a_linear_chain_with_odometry();
  if (failures) { std::printf("noise_host_tests: %d FAILED\n", failures); return 1; }
  std::printf("noise_host_tests: all tests passed\n");
  return 0;
}
