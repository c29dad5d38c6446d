// Loop closures past one border through the C++ host classes (gpslam_amd/host/gpslam_host.hpp): a graph with 12 non-adjacent
// BetweenFactor<Pose2> is what GTSAM would simply solve, so the host session switches the column passes on by itself
// (gpslam_hip_set_closure_passes(h, 32, 0)); a graph whose closures fit one pass creates its handle as before.  Without an
// argument the program only proves that it links (no device call); with one it runs on the GPU.
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

static Pose2 compose(const Pose2 &a, const Pose2 &b) {
  return Pose2(a.x + std::cos(a.theta) * b.x - std::sin(a.theta) * b.y, a.y + std::sin(a.theta) * b.x + std::cos(a.theta) * b.y, a.theta + b.theta);
}
static Pose2 between(const Pose2 &a, const Pose2 &b) {   // a^-1 b
  const double dx = b.x - a.x, dy = b.y - a.y, c = std::cos(a.theta), s = std::sin(a.theta);
  return Pose2(c * dx + s * dy, -s * dx + c * dy, b.theta - a.theta);
}

// a circle driven at constant velocity: exact odometry, exact closures, a start that is 2 cm / 0.01 rad off everywhere
static void circle(int N, const std::vector<std::pair<int, int>> &closures, NonlinearFactorGraph &graph, Values &init, std::vector<Pose2> &truth) {
  const double dt = 0.25, w = 2 * M_PI / ((N - 1) * dt), v = 1.0, th = dt * w;
  const Pose2 step(v * dt * std::sin(th) / th, v * dt * (1 - std::cos(th)) / th, th);
  truth.assign(N, Pose2());
  for (int k = 0; k + 1 < N; k++) truth[k + 1] = compose(truth[k], step);
  auto Qc_model = noiseModel::Gaussian::Covariance(1.0 * Matrix::Identity(3));
  graph.add(PriorFactor<Pose2>(Symbol('x', 0), truth[0], noiseModel::Isotropic::Sigma(3, 1e-3)));
  for (int k = 0; k + 1 < N; k++) {
    graph.add(GaussianProcessPriorPose2(Symbol('x', k), Symbol('v', k), Symbol('x', k + 1), Symbol('v', k + 1), dt, Qc_model));
    graph.add(BetweenFactor<Pose2>(Symbol('x', k), Symbol('x', k + 1), step, noiseModel::Isotropic::Sigma(3, 2e-2)));
  }
  for (const auto &c : closures)
    graph.add(BetweenFactor<Pose2>(Symbol('x', c.first), Symbol('x', c.second), between(truth[c.first], truth[c.second]), noiseModel::Isotropic::Sigma(3, 1e-2)));
  for (int k = 0; k < N; k++) {
    const double s = (k % 2) ? 1.0 : -1.0;
    init.insert(Symbol('x', k), k == 0 ? truth[0] : Pose2(truth[k].x + 0.02 * s, truth[k].y - 0.02 * s, truth[k].theta + 0.01 * s));
    init.insert(Symbol('v', k), Vector3{v, 0, w});
  }
}

static void run(int nclosures, int want_w, int want_P) {
  const int N = 64;
  std::vector<std::pair<int, int>> closures;
  for (int k = 0; k < nclosures; k++) closures.push_back(k % 2 ? std::make_pair(5 * k + 1, (5 * k + 30) % N) : std::make_pair((5 * k + 33) % N, 5 * k));
  NonlinearFactorGraph graph;
  Values init;
  std::vector<Pose2> truth;
  circle(N, closures, graph, init, truth);
  GaussNewtonOptimizer optimizer(graph, init);
  int32_t info[4] = {0, 0, 0, 0};
  EXPECT(gpslam_hip_closure_info(optimizer.handle(), info) == 0);
  EXPECT(info[0] == nclosures && info[1] == want_w && info[2] == want_P && info[3] == (want_P > 1 ? want_P + 1 : 1));
  Values values = optimizer.optimize();
  EXPECT(std::fabs(graph.error(values)) < 1e-6);
  double worst = 0.0;
  for (int k = 0; k < N; k++) {
    const Pose2 p = values.at<Pose2>(Symbol('x', k));
    worst = std::fmax(worst, std::fmax(std::fabs(p.x - truth[k].x), std::fmax(std::fabs(p.y - truth[k].y), std::fabs(p.theta - truth[k].theta))));
  }
  EXPECT(worst < 1e-6);
  EXPECT(optimizer.iterations() > 0 && optimizer.iterations() < 100);
  std::printf("%d closures: w %d, P %d, %d iterations, error %.3e, worst pose coordinate %.3e\n", nclosures, (int)info[1], (int)info[2],
              (int)optimizer.iterations(), graph.error(values), worst);
}

int main(int argc, char **) {
  if (argc < 2) return 0;   // (link check only: running it needs a device)
  run(12, 9, 2);            // two column passes, switched on by the host session
  run(3, 3, 1);             // within one pass: the handle as before
  if (failures) { std::printf("closure_passes_host_tests: %d FAILED\n", failures); return 1; }
  std::printf("closure_passes_host_tests: all tests passed\n");
  return 0;
}
