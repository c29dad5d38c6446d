// gtsam::Marginals on a graph that takes the segmented landmark path (gpslam_amd/host/gpslam_host.hpp): 24 planar range landmarks,
// each seen from a window of a 240-state drive -- more than the dense landmark border holds.  The Marginals constructor asks its own
// session for gpslam_hip_marginals_on_segments; jointMarginalCovariance is served through the landmark getters, and the blocks the
// class hands out are compared with those getters on its handle (the class copies numbers, it computes none).  Sets the getters
// cannot serve -- landmarks further apart than neighbouring fat blocks -- throw std::invalid_argument.  Without an argument the
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

template <typename F> static bool same(const Matrix &m, int rows, int cols, F f) {
  if (m.rows != rows || m.cols != cols) return false;
  for (int r = 0; r < rows; r++)
    for (int c = 0; c < cols; c++)
      if (m(r, c) != f(r, c)) return false;
  return true;
}
template <typename F> static bool throws_invalid(F f) {
  try { f(); } catch (const std::invalid_argument &) { return true; } catch (...) { return false; }
  return false;
}

static void test_marginals_on_the_segmented_path() {
  const int N = 240, L = 24, b = 6, ld = 2, span = 20;
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
  EXPECT(plan[0] == 1 && plan[2] >= 3);          // segmented, at least two segments
  std::vector<double> S((size_t)N * b * b), Sn(S.size()), big(4);
  EXPECT(gpslam_hip_get_marginals(m.handle(), 0, N, S.data(), Sn.data(), nullptr, nullptr) == 0);
  EXPECT(gpslam_hip_get_marginals(m.handle(), 0, 1, nullptr, nullptr, big.data(), nullptr) == GPSLAM_E_UNSUPPORTED);
  auto s = [&](int i, int r, int c) { return S[((size_t)i * b + r) * b + c]; };
  auto sn = [&](int i, int r, int c) { return Sn[((size_t)i * b + r) * b + c]; };
  for (int i : {0, 57, N - 1}) {
    EXPECT(same(m.marginalCovariance(Symbol('x', i)), 3, 3, [&](int r, int c) { return s(i, r, c); }));
    EXPECT(same(m.marginalCovariance(Symbol('v', i)), 3, 3, [&](int r, int c) { return s(i, 3 + r, 3 + c); }));
    for (int r = 0; r < b; r++) EXPECT(s(i, r, r) > 0.0 && std::isfinite(s(i, r, r)));
  }
  // a landmark, two adjacent states that observe it, and its neighbour landmark
  const int l = 7, l2 = 8, i = centre[l];
  std::vector<double> Ll(ld * ld), Lp(ld * ld), X(2 * b * ld);
  const int32_t la[1] = {l}, lb[1] = {l2}, st[2] = {i, i + 1}, ll[2] = {l, l};
  EXPECT(gpslam_hip_get_landmark_marginals(m.handle(), l, 1, Ll.data()) == 0);
  EXPECT(gpslam_hip_get_landmark_pair_marginals(m.handle(), 1, la, lb, Lp.data()) == 0);
  EXPECT(gpslam_hip_get_state_landmark_marginals(m.handle(), 2, st, ll, X.data()) == 0);
  EXPECT(same(m.marginalCovariance(Symbol('l', l)), 2, 2, [&](int r, int c) { return Ll[r * ld + c]; }));
  EXPECT(Ll[0] > 0.0 && Ll[3] > 0.0 && Ll[1] == Ll[2]);
  const JointMarginal j = m.jointMarginalCovariance(KeyVector{Symbol('x', i + 1), Symbol('l', l), Symbol('v', i), Symbol('x', i), Symbol('l', l2)});
  EXPECT(same(j(Symbol('x', i), Symbol('x', i + 1)), 3, 3, [&](int r, int c) { return sn(i, r, c); }));
  EXPECT(same(j(Symbol('x', i), Symbol('l', l)), 3, 2, [&](int r, int c) { return X[r * ld + c]; }));
  EXPECT(same(j(Symbol('v', i), Symbol('l', l)), 3, 2, [&](int r, int c) { return X[(3 + r) * ld + c]; }));
  EXPECT(same(j(Symbol('l', l), Symbol('x', i + 1)), 2, 3, [&](int r, int c) { return X[(b + c) * ld + r]; }));
  EXPECT(same(j(Symbol('l', l), Symbol('l', l2)), 2, 2, [&](int r, int c) { return Lp[r * ld + c]; }));
  EXPECT(same(j(Symbol('l', l2), Symbol('l', l)), 2, 2, [&](int r, int c) { return Lp[c * ld + r]; }));
  EXPECT(j.fullMatrix().rows == 13);
  // sets the getters cannot serve: landmarks at the two ends of the drive, a state with a landmark from the other end
  EXPECT(throws_invalid([&] { m.jointMarginalCovariance(KeyVector{Symbol('l', 0), Symbol('l', L - 1)}); }));
  EXPECT(throws_invalid([&] { m.jointMarginalCovariance(KeyVector{Symbol('x', 2), Symbol('l', L - 1)}); }));
  EXPECT(throws_invalid([&] { m.jointMarginalCovariance(KeyVector{Symbol('x', 0), Symbol('x', 2)}); }));
  const std::vector<Matrix> P = m.interpolatePoseCovariances(KeyVector{Symbol('x', 3)}, {dt}, {0.04});
  EXPECT(P.size() == 1 && P[0](0, 0) > 0.0);
  // the opt-in belongs to this session alone: switched off, the handle refuses again
  EXPECT(gpslam_hip_marginals_on_segments(m.handle(), 0) == 0);
  EXPECT(gpslam_hip_marginals(m.handle()) == GPSLAM_E_UNSUPPORTED);
  std::printf("segmented: K %d NB %d, Sigma(l%d) %.3e %.3e\n", (int)plan[2], (int)plan[3], l, Ll[0], Ll[3]);
}

int main(int argc, char **) {
  if (argc < 2)   // (no device call: the NULL-handle checks)
    return (gpslam_hip_marginals_on_segments(nullptr, 1) == GPSLAM_E_INVALID && gpslam_hip_get_landmark_marginals(nullptr, 0, 0, nullptr) == GPSLAM_E_INVALID &&
            gpslam_hip_get_state_landmark_marginals(nullptr, 0, nullptr, nullptr, nullptr) == GPSLAM_E_INVALID &&
            gpslam_hip_get_landmark_pair_marginals(nullptr, 0, nullptr, nullptr, nullptr) == GPSLAM_E_INVALID) ? 0 : 1;
  test_marginals_on_the_segmented_path();
  if (failures) { std::printf("segmented_marginals_host_tests: %d FAILED\n", failures); return 1; }
  std::printf("segmented_marginals_host_tests: all tests passed\n");
  return 0;
}
