// gtsam::DoglegOptimizer of gpslam_amd/host/gpslam_host.hpp (include/gpslam_hip_dogleg.h).  Without an argument: the parameter mapping,
// the two host-arithmetic entry points and the NULL-handle answers -- no device call.  With one, on the GPU: a Pose2 chain with range
// landmarks from a start a quarter turn off, DoglegOptimizer against LevenbergMarquardtOptimizer.
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

static void test_parameter_mapping() {
  DoglegParams p;
  EXPECT(p.deltaInitial == 1.0 && p.getDeltaInitial() == 1.0);
  EXPECT(p.adaptationMode == DoglegParams::ONE_STEP_PER_ITERATION);
  EXPECT(p.maxIterations == 100 && p.relativeErrorTol == 1e-5 && p.absoluteErrorTol == 1e-5 && p.errorTol == 0.0);
  EXPECT(DoglegOptimizer::abiArguments(p).first == 1.0 && DoglegOptimizer::abiArguments(p).second == GPSLAM_DOGLEG_ONE_STEP_PER_ITERATION);
  p.setDeltaInitial(0.25);
  p.adaptationMode = DoglegParams::SEARCH_EACH_ITERATION;
  EXPECT(DoglegOptimizer::abiArguments(p).first == 0.25 && DoglegOptimizer::abiArguments(p).second == GPSLAM_DOGLEG_SEARCH_EACH_ITERATION);
  p.adaptationMode = DoglegParams::SEARCH_REDUCE_ONLY;
  EXPECT(DoglegOptimizer::abiArguments(p).second == GPSLAM_DOGLEG_SEARCH_REDUCE_ONLY);
  NonlinearOptimizerParams &base = p;      // DoglegParams IS a NonlinearOptimizerParams
  base.setMaxIterations(7);
  EXPECT(p.maxIterations == 7);
}

static void test_host_arithmetic_and_null_handle() {
  // H = diag(1, 4), g = (1, 2): gg = 5, gHg = 17, dn = (1, 0.5), gn = 2, nn = 1.25; |du| = (5 / 17) sqrt(5) = 0.6577, |dn| = 1.118
  const double s4[4] = {5.0, 17.0, 2.0, 1.25};
  double coef[2], norm, pred;
  int32_t branch;
  EXPECT(gpslam_hip_dogleg_point(s4, 0.5, coef, &norm, &pred, &branch) == 0 && branch == 0 && coef[1] == 0.0 && std::fabs(norm - 0.5) < 1e-15);
  EXPECT(gpslam_hip_dogleg_point(s4, 1.0, coef, &norm, &pred, &branch) == 0 && branch == 1 && std::fabs(norm - 1.0) < 1e-14);
  EXPECT(gpslam_hip_dogleg_point(s4, 2.0, coef, &norm, &pred, &branch) == 0 && branch == 2 && coef[0] == 0.0 && coef[1] == 1.0 && pred == 1.0);
  EXPECT(gpslam_hip_dogleg_point(s4, 0.0, coef, &norm, &pred, &branch) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_dogleg_point(nullptr, 1.0, coef, &norm, &pred, &branch) == GPSLAM_E_INVALID);
  double delta = 1.0;
  int32_t last = 0, keep = -1, stay = -1;
  const double good[4] = {10.0, 1.0, 10.0, 0.5};      // rho = 0.9
  EXPECT(gpslam_hip_dogleg_decide(good, GPSLAM_DOGLEG_ONE_STEP_PER_ITERATION, &delta, &last, &keep, &stay) == 0 && keep == 1 && stay == 0 && delta == 1.5);
  const double bad[4] = {10.0, 11.0, 10.0, 0.5};      // rho < 0
  EXPECT(gpslam_hip_dogleg_decide(bad, GPSLAM_DOGLEG_ONE_STEP_PER_ITERATION, &delta, &last, &keep, &stay) == 0 && keep == 0 && stay == 1 && delta == 0.75 && last == 2);
  EXPECT(gpslam_hip_dogleg_decide(bad, 3, &delta, &last, &keep, &stay) == GPSLAM_E_INVALID);
  gpslam_hip_stats st;
  double out8[8];
  gpslam_hip_params prm;
  gpslam_hip_default_params(&prm);
  EXPECT(gpslam_hip_iterate_dogleg(nullptr, &delta, 0, &st) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_optimize_dogleg(nullptr, &prm, 1.0, 0, &st) == GPSLAM_E_INVALID);
  EXPECT(gpslam_hip_dogleg_last(nullptr, out8) == GPSLAM_E_INVALID);
}

static void test_dogleg_against_levenberg_marquardt() {
  const int N = 24;
  const double dt = 0.25, w = 0.6, v = 1.0;
  auto step = [&]() {
    const double th = dt * w;
    return Pose2(v * dt * std::sin(th) / th, v * dt * (1 - std::cos(th)) / th, th);
  };
  auto compose = [](const Pose2 &a, const Pose2 &c) {
    return Pose2(a.x + std::cos(a.theta) * c.x - std::sin(a.theta) * c.y, a.y + std::sin(a.theta) * c.x + std::cos(a.theta) * c.y, a.theta + c.theta);
  };
  std::vector<Pose2> truth(N);
  for (int k = 0; k + 1 < N; k++) truth[k + 1] = compose(truth[k], step());
  const Point2 land[2] = {Point2(0.5, 2.5), Point2(-1.0, 1.0)};
  auto Qc_model = noiseModel::Gaussian::Covariance(1.0 * Matrix::Identity(3));
  NonlinearFactorGraph graph;
  graph.add(PriorFactor<Pose2>(Symbol('x', 0), truth[0], noiseModel::Isotropic::Sigma(3, 1e-3)));
  for (int k = 0; k + 1 < N; k++) {
    graph.add(GaussianProcessPriorPose2(Symbol('x', k), Symbol('v', k), Symbol('x', k + 1), Symbol('v', k + 1), dt, Qc_model));
    graph.add(BetweenFactor<Pose2>(Symbol('x', k), Symbol('x', k + 1), step(), noiseModel::Isotropic::Sigma(3, 2e-2)));
  }
  for (int k = 0; k < N; k += 2)
    for (int l = 0; l < 2; l++)
      graph.add(RangeFactorPose2(Symbol('x', k), Symbol('l', l), std::hypot(truth[k].x - land[l].x, truth[k].y - land[l].y),
                                 noiseModel::Isotropic::Sigma(1, 0.05)));
  graph.add(PriorFactor<Point2>(Symbol('l', 0), land[0], noiseModel::Isotropic::Sigma(2, 0.5)));
  graph.add(PriorFactor<Point2>(Symbol('l', 1), land[1], noiseModel::Isotropic::Sigma(2, 0.5)));
  Values init;
  for (int k = 0; k < N; k++) {
    init.insert(Symbol('x', k), Pose2(truth[k].x + 0.3 * std::sin(0.7 * k), truth[k].y - 0.2 * std::cos(0.4 * k), truth[k].theta + 0.4 * std::sin(0.3 * k)));
    init.insert(Symbol('v', k), Vector3{v, 0, w});
  }
  init.insert(Symbol('l', 0), Point2(land[0].x + 0.2, land[0].y - 0.1));
  init.insert(Symbol('l', 1), Point2(land[1].x - 0.1, land[1].y + 0.2));
  DoglegParams dp;
  dp.setRelativeErrorTol(1e-12);
  dp.setAbsoluteErrorTol(1e-12);
  DoglegOptimizer dog(graph, init, dp);
  const double e0 = dog.error();
  EXPECT(dog.getDelta() == 1.0);
  double prev = e0;
  dog.iterate();
  EXPECT(dog.error() <= prev && dog.iterations() == 1);
  dog.optimize();
  LevenbergMarquardtParams lp;
  lp.setRelativeErrorTol(1e-12);
  lp.setAbsoluteErrorTol(1e-12);
  LevenbergMarquardtOptimizer lm(graph, init, lp);
  lm.optimize();
  std::printf("dogleg: error %.12g -> %.12g in %d iterations, delta %.3g; Levenberg-Marquardt %.12g in %d\n", e0, dog.error(), dog.iterations(),
              dog.getDelta(), lm.error(), lm.iterations());
  EXPECT(dog.error() < e0);
  EXPECT(std::fabs(dog.error() - lm.error()) <= 1e-8 * (1.0 + lm.error()));
  const Pose2 a = dog.values().at<Pose2>(Symbol('x', N - 1)), b = lm.values().at<Pose2>(Symbol('x', N - 1));
  EXPECT(std::fabs(a.x - b.x) < 1e-6 && std::fabs(a.y - b.y) < 1e-6 && std::fabs(a.theta - b.theta) < 1e-6);
}

int main(int argc, char **) {
  test_parameter_mapping();
  test_host_arithmetic_and_null_handle();
  if (argc > 1) test_dogleg_against_levenberg_marquardt();
  if (failures) { std::printf("dogleg_host_tests: %d FAILED\n", failures); return 1; }
  std::printf("dogleg_host_tests: all tests passed\n");
  return 0;
}
