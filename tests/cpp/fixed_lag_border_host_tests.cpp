// gtsam::LinearContainerFactor over (x, v, landmarks) and gtsam::BatchFixedLagSmoother on a graph with landmarks
// (gpslam_amd/host/gpslam_host.hpp; gpslam_hip_add_border_gaussians, gpslam_hip_marginalize_head_onto_landmarks).  A Pose2 GP chain
// whose odd states range two landmarks: (1) a block-diagonal container factor over (x_5, v_5, l_0, l_1) is the velocity prior and the
// two landmark priors it restates (same graph error, same Levenberg-Marquardt result); (2) the smoother, asked to marginalise onto the
// landmarks, slides where it otherwise refuses, and leaves one border Gaussian on the oldest kept state; (3) a container factor that
// does not name every landmark, or names them out of order, throws.  Without an argument the program only proves that it links
// (NULL-handle checks, no device call); with one it runs on the GPU.
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

static const int N = 10;
static const double dt = 0.1;
static const Point2 land[2] = {Point2(1.0, 2.0), Point2(-0.5, 1.5)};

static NonlinearFactorGraph chain(Values &v, BatchFixedLagSmoother::KeyTimestampMap &stamps) {
  auto Qc_model = noiseModel::Gaussian::Covariance(1.0 * Matrix::Identity(3));
  NonlinearFactorGraph g;
  g.add(PriorFactor<Pose2>(Symbol('x', 0), Pose2(0, 0, 0), noiseModel::Isotropic::Sigma(3, 1e-2)));
  g.add(PriorFactor<Vector3>(Symbol('v', 0), Vector3{1.0, 0.0, 0.0}, noiseModel::Isotropic::Sigma(3, 1e-1)));
  for (int k = 0; k < N; k++) {
    const Pose2 x(0.1 * k, 0.0, 0.0);
    v.insert(Symbol('x', k), Pose2(0.1 * k + 0.01 * std::sin(1.3 * k), 0.01 * std::cos(0.7 * k), 0.0));
    v.insert(Symbol('v', k), Vector3{1.0, 0.0, 0.0});
    stamps[Symbol('x', k)] = k * dt;
    if (k + 1 < N) g.add(GaussianProcessPriorPose2(Symbol('x', k), Symbol('v', k), Symbol('x', k + 1), Symbol('v', k + 1), dt, Qc_model));
    if (k % 2 == 1)
      for (int l = 0; l < 2; l++)
        g.add(RangeFactorPose2(Symbol('x', k), Symbol('l', l), std::hypot(x.x - land[l].x, x.y - land[l].y), noiseModel::Isotropic::Sigma(1, 0.05)));
  }
  for (int l = 0; l < 2; l++) {
    v.insert(Symbol('l', l), Point2(land[l].x + 0.1, land[l].y - 0.1));
    g.add(PriorFactor<Point2>(Symbol('l', l), land[l], noiseModel::Isotropic::Sigma(2, 0.5)));
  }
  return g;
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

static void test_container_factor_is_the_priors_it_restates() {
  Values v0;
  BatchFixedLagSmoother::KeyTimestampMap stamps;
  NonlinearFactorGraph a = chain(v0, stamps), b = a;
  const Vector3 mv{0.9, 0.1, -0.05};
  const Point2 ml[2] = {Point2(1.2, 1.9), Point2(-0.4, 1.4)};
  const double sv = 0.2, sl = 0.3;
  a.add(PriorFactor<Vector3>(Symbol('v', 5), mv, noiseModel::Isotropic::Sigma(3, sv)));
  for (int l = 0; l < 2; l++) a.add(PriorFactor<Point2>(Symbol('l', l), ml[l], noiseModel::Isotropic::Sigma(2, sl)));
  Matrix A(10, 10);
  for (int i = 0; i < 3; i++) A(3 + i, 3 + i) = 1.0 / sv;      // (the pose rows stay zero)
  for (int i = 0; i < 4; i++) A(6 + i, 6 + i) = 1.0 / sl;
  const std::vector<Key> lk = {Symbol('l', 0), Symbol('l', 1)};
  b.add(LinearContainerFactor(Symbol('x', 5), Symbol('v', 5), lk, A, Vector(10, 0.0), Pose2(0.5, 0.0, 0.0), mv, std::vector<Point2>{ml[0], ml[1]}));
  const double ea = a.error(v0), eb = b.error(v0);
  EXPECT(std::fabs(ea - eb) <= 1e-12 * ea);
  LevenbergMarquardtOptimizer oa(a, v0, tight()), ob(b, v0, tight());
  const Values ra = oa.optimize(), rb = ob.optimize();
  double worst = 0.0;
  for (int k = 0; k < N; k++) {
    const Pose2 pa = ra.at<Pose2>(Symbol('x', k)), pb = rb.at<Pose2>(Symbol('x', k));
    worst = std::max(worst, std::max(std::fabs(pa.x - pb.x), std::max(std::fabs(pa.y - pb.y), std::fabs(pa.theta - pb.theta))));
    for (int c = 0; c < 3; c++) worst = std::max(worst, std::fabs(ra.at<Vector3>(Symbol('v', k))[c] - rb.at<Vector3>(Symbol('v', k))[c]));
  }
  for (int l = 0; l < 2; l++) {
    const Point2 qa = ra.at<Point2>(Symbol('l', l)), qb = rb.at<Point2>(Symbol('l', l));
    worst = std::max(worst, std::max(std::fabs(qa.x - qb.x), std::fabs(qa.y - qb.y)));
  }
  std::printf("container factor over the landmarks against the priors: error %.6e / %.6e, variables differ by %.3e\n", ea, eb, worst);
  EXPECT(worst <= 1e-9);
  // not every landmark / out of order / sizes
  NonlinearFactorGraph c1 = chain(v0 = Values(), stamps), c2 = c1;
  c1.add(LinearContainerFactor(Symbol('x', 5), Symbol('v', 5), std::vector<Key>{Symbol('l', 0)}, Matrix(8, 8), Vector(8, 0.0), Pose2(0, 0, 0), mv, std::vector<Point2>{ml[0]}));
  EXPECT(throws_invalid([&] { c1.error(v0); }));
  c2.add(LinearContainerFactor(Symbol('x', 5), Symbol('v', 5), std::vector<Key>{Symbol('l', 1), Symbol('l', 0)}, A, Vector(10, 0.0), Pose2(0, 0, 0), mv, std::vector<Point2>{ml[1], ml[0]}));
  EXPECT(throws_invalid([&] { c2.error(v0); }));
  EXPECT(throws_invalid([&] { LinearContainerFactor(Symbol('x', 1), Symbol('v', 1), lk, A, Vector(10, 0.0), Pose2(0, 0, 0), mv, std::vector<Point2>{ml[0]}); }));
}

static void test_smoother_slides_over_a_graph_with_landmarks() {
  Values v;
  BatchFixedLagSmoother::KeyTimestampMap stamps;
  const NonlinearFactorGraph g = chain(v, stamps);
  BatchFixedLagSmoother refuses(4 * dt + 0.5 * dt, tight());
  EXPECT(throws_invalid([&] { refuses.update(g, v, stamps); }));       // the default: as before
  BatchFixedLagSmoother smoother(4 * dt + 0.5 * dt, tight());
  smoother.marginalizeOntoLandmarks();
  const BatchFixedLagSmoother::Result r = smoother.update(g, v, stamps);
  EXPECT(r.marginalized == N - 5 && std::isfinite(r.error));
  const Values got = smoother.calculateEstimate();
  EXPECT(!got.exists(Symbol('x', N - 6)) && got.exists(Symbol('x', N - 5)) && got.exists(Symbol('l', 1)));
  EXPECT(gpslam_hip_get_border_gaussians(smoother.handle(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 1);
  EXPECT(gpslam_hip_get_state_gaussians(smoother.handle(), nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
  double lm[4], Lam[100], gam[10];
  EXPECT(gpslam_hip_get_head_prior_border(smoother.handle(), lm, Lam, gam) == 0);
  EXPECT(Lam[0] > 0.0 && Lam[6 * 10 + 6] > 0.0 && std::fabs(Lam[6] - Lam[60]) <= 1e-12 * Lam[0]);
  std::printf("smoother with landmarks: %d states marginalised, error %.6e\n", r.marginalized, r.error);
}

int main(int argc, char **) {
  if (argc < 2)   // (no device call: the NULL-handle checks)
    return (gpslam_hip_add_border_gaussians(nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == GPSLAM_E_INVALID &&
            gpslam_hip_get_border_gaussians(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == GPSLAM_E_INVALID &&
            gpslam_hip_marginalize_head_onto_landmarks(nullptr, 1) == GPSLAM_E_INVALID &&
            gpslam_hip_get_head_prior_border(nullptr, nullptr, nullptr, nullptr) == GPSLAM_E_INVALID) ? 0 : 1;
  test_container_factor_is_the_priors_it_restates();
  test_smoother_slides_over_a_graph_with_landmarks();
  if (failures) { std::printf("fixed_lag_border_host_tests: %d FAILED\n", failures); return 1; }
  std::printf("fixed_lag_border_host_tests: all tests passed\n");
  return 0;
}
