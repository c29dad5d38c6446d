// gpslam_host.hpp -- C++ host classes with the gpslam / GTSAM names, constructor signatures and call pattern,
// implemented on top of the C ABI (include/gpslam_hip.h).  Header-only, C++17, no Eigen/Boost/GTSAM needed.
//
// What a user of gtrll/gpslam writes (gpslam/gp/tests/testGaussianProcessPriorPose3.cpp:162-194):
//     NonlinearFactorGraph graph;
//     graph.add(PriorFactor<Pose3>(Symbol('x', 1), pose1, model_prior));
//     graph.add(GaussianProcessPriorPose3(Symbol('x', 1), Symbol('v', 1), Symbol('x', 2), Symbol('v', 2), delta_t, Qc_model));
//     Values init_values;  init_values.insert(Symbol('x', 1), pose1); ...
//     GaussNewtonOptimizer optimizer(graph, init_values, parameters);  optimizer.optimize();
//     Values values = optimizer.values();
// compiles against this header unchanged; the optimizer's constructor is the "graph compile" pass (classify the
// factors, map keys to chain positions, pack SoA arrays, upload) and every iterate() is HIP kernels.
//
// Key convention (the one every gpslam test and script uses): pose i = Symbol('x', i), velocity i = Symbol('v', i),
// landmark j = Symbol('l', j).  States are ordered by index; factors may couple a state only with its successor
// (the GP Markov structure, GaussianProcessPriorPose3.h:43-47).  Anything else throws std::invalid_argument,
// the analogue of GTSAM's exceptions; HIP failures throw std::runtime_error.
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <iostream>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/gpslam_hip.h"
#include "../../include/gpslam_hip_dogleg.h"
#include "../../include/gpslam_hip_evidence.h"
#include "../../include/gpslam_hip_qc.h"
#include "../../include/gpslam_hip_noise.h"
#include "../../include/gpslam_hip_sampling.h"
#include "../../include/gpslam_hip_sampling_at.h"
#include "../../include/gpslam_hip_sampling_stats.h"

// boost::optional<Matrix&> -- the type of the reference's Jacobian arguments (gpslam/gp/GaussianProcessPriorPose3.h:60-64:
// `boost::optional<gtsam::Matrix&> H1 = boost::none`).  Where Boost is installed its header is used; where it is not (this image), the
// two names a call site of evaluateError / interpolatePose can spell -- boost::none and boost::optional<T&> -- are provided here, so
// that `f.evaluateError(p1, v1, p2, v2, H1, boost::none, H3)` compiles unchanged (round 6; rounds 2-5 took `Matrix*`, which still works).
#if defined(__has_include) && __has_include(<boost/optional.hpp>)
#include <boost/optional.hpp>
#else
namespace boost {
struct none_t { struct init_tag {}; explicit constexpr none_t(init_tag) {} };
inline constexpr none_t none{none_t::init_tag{}};
template <class T> class optional;
template <class T> class optional<T &> {
 public:
  optional() : p_(nullptr) {}
  optional(none_t) : p_(nullptr) {}
  optional(T &r) : p_(&r) {}
  explicit operator bool() const { return p_ != nullptr; }
  bool is_initialized() const { return p_ != nullptr; }
  T &operator*() const { return *p_; }
  T *operator->() const { return p_; }
  T &get() const { return *p_; }
  T *get_ptr() const { return p_; }
  void reset() { p_ = nullptr; }
 private:
  T *p_;
};
}  // namespace boost
#endif

namespace gtsam {

typedef uint64_t Key;
/// gtsam::Symbol(c, j) -> Key = (c << 56) | j
inline Key Symbol(unsigned char c, uint64_t j) { return (Key(c) << 56) | j; }
inline unsigned char symbolChr(Key k) { return (unsigned char)(k >> 56); }
inline uint64_t symbolIndex(Key k) { return k & ((Key(1) << 56) - 1); }
/// gtsam::KeyFormatter / DefaultKeyFormatter: "x12" for Symbol('x', 12), the plain number for keys without a character
typedef std::function<std::string(Key)> KeyFormatter;
inline std::string DefaultKeyFormatter(Key k) {
  const unsigned char c = symbolChr(k);
  return (c ? std::string(1, (char)c) : std::string()) + std::to_string(c ? symbolIndex(k) : k);
}

template <int N> struct VectorN : std::array<double, N> {
  VectorN() { this->fill(0.0); }
  VectorN(std::initializer_list<double> l) { this->fill(0.0); int i = 0; for (double v : l) if (i < N) (*this)[i++] = v; }
};
typedef VectorN<2> Vector2;
typedef VectorN<3> Vector3;
typedef VectorN<6> Vector6;
typedef std::vector<double> Vector;

struct Matrix {  // dynamic, row-major
  int rows = 0, cols = 0;
  std::vector<double> a;
  Matrix() {}
  Matrix(int r, int c) : rows(r), cols(c), a((size_t)r * c, 0.0) {}
  double &operator()(int i, int j) { return a[(size_t)i * cols + j]; }
  double operator()(int i, int j) const { return a[(size_t)i * cols + j]; }
  static Matrix Identity(int n) { Matrix m(n, n); for (int i = 0; i < n; i++) m(i, i) = 1.0; return m; }
  Matrix operator*(double s) const { Matrix m = *this; for (double &v : m.a) v *= s; return m; }
};
inline Matrix operator*(double s, const Matrix &m) { return m * s; }

/// What a Jacobian argument of evaluateError / interpolatePose accepts: everything a call site of the reference can pass to a
/// `boost::optional<gtsam::Matrix&>` parameter -- a Matrix lvalue, boost::none, a boost::optional<Matrix&> -- and, as in rounds 2-5 of
/// this header, a `Matrix*` (nullptr = not wanted).  Converts to `Matrix*` for the implementation.
class OptionalMatrix {
 public:
  OptionalMatrix() {}
  OptionalMatrix(boost::none_t) {}
  OptionalMatrix(std::nullptr_t) {}
  OptionalMatrix(Matrix &m) : p_(&m) {}
  OptionalMatrix(Matrix *m) : p_(m) {}
  OptionalMatrix(const boost::optional<Matrix &> &o) : p_(o ? &*o : nullptr) {}
  operator Matrix *() const { return p_; }
 private:
  Matrix *p_ = nullptr;
};

struct Point2 { double x = 0, y = 0; Point2() {} Point2(double x_, double y_) : x(x_), y(y_) {} };
struct Point3 { double x = 0, y = 0, z = 0; Point3() {} Point3(double x_, double y_, double z_) : x(x_), y(y_), z(z_) {} };

struct Rot3 {
  double R[9];
  Rot3() { std::memset(R, 0, sizeof(R)); R[0] = R[4] = R[8] = 1.0; }
  /// Rot3::Ypr(y, p, r) = Rz(y) Ry(p) Rx(r)
  static Rot3 Ypr(double y, double p, double r) {
    const double cy = std::cos(y), sy = std::sin(y), cp = std::cos(p), sp = std::sin(p), cr = std::cos(r), sr = std::sin(r);
    Rot3 o;
    o.R[0] = cy * cp; o.R[1] = cy * sp * sr - sy * cr; o.R[2] = cy * sp * cr + sy * sr;
    o.R[3] = sy * cp; o.R[4] = sy * sp * sr + cy * cr; o.R[5] = sy * sp * cr - cy * sr;
    o.R[6] = -sp;     o.R[7] = cp * sr;                o.R[8] = cp * cr;
    return o;
  }
};
struct Pose2 {
  double x = 0, y = 0, theta = 0;
  Pose2() {}
  Pose2(double x_, double y_, double th) : x(x_), y(y_), theta(th) {}
  double range(const Point2 &p) const { return std::hypot(p.x - x, p.y - y); }
};
struct Pose3 {
  Rot3 R;
  Point3 t;
  Pose3() {}
  Pose3(const Rot3 &r, const Point3 &p) : R(r), t(p) {}
  const Rot3 &rotation() const { return R; }
  const Point3 &translation() const { return t; }
  Pose3 compose(const Pose3 &o) const {
    Pose3 c;
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) c.R.R[3 * i + j] = R.R[3 * i] * o.R.R[j] + R.R[3 * i + 1] * o.R.R[3 + j] + R.R[3 * i + 2] * o.R.R[6 + j];
    c.t.x = t.x + R.R[0] * o.t.x + R.R[1] * o.t.y + R.R[2] * o.t.z;
    c.t.y = t.y + R.R[3] * o.t.x + R.R[4] * o.t.y + R.R[5] * o.t.z;
    c.t.z = t.z + R.R[6] * o.t.x + R.R[7] * o.t.y + R.R[8] * o.t.z;
    return c;
  }
  double range(const Point3 &p) const {
    const double dx = p.x - t.x, dy = p.y - t.y, dz = p.z - t.z;
    return std::sqrt(dx * dx + dy * dy + dz * dz);
  }
};
struct Unit3 {
  double p[3];
  Unit3(double x = 0, double y = 0, double z = 1) { const double n = std::sqrt(x * x + y * y + z * z); p[0] = x / n; p[1] = y / n; p[2] = z / n; }
};

// ---------------------------------------------------------------- noise models
/// gtsam::Cal3_S2: fx, fy, skew, principal point (default = identity calibration)
class Cal3_S2 {
 public:
  Cal3_S2() {}
  Cal3_S2(double fx, double fy, double s, double u0, double v0) : fx_(fx), fy_(fy), s_(s), u0_(u0), v0_(v0) {}
  double fx() const { return fx_; }
  double fy() const { return fy_; }
  double skew() const { return s_; }
  double px() const { return u0_; }
  double py() const { return v0_; }
 private:
  double fx_ = 1, fy_ = 1, s_ = 0, u0_ = 0, v0_ = 0;
};

/// gtsam::Cal3DS2: Cal3_S2 plus radial (k1, k2) and tangential (p1, p2) distortion -- the second CALIBRATION the projection
/// factor template is instantiated for here (GPInterpolatedProjectionFactorPose3.h:29; round 4)
class Cal3DS2 {
 public:
  Cal3DS2() {}
  Cal3DS2(double fx, double fy, double s, double u0, double v0, double k1, double k2, double p1 = 0.0, double p2 = 0.0)
      : fx_(fx), fy_(fy), s_(s), u0_(u0), v0_(v0), k1_(k1), k2_(k2), p1_(p1), p2_(p2) {}
  double fx() const { return fx_; }
  double fy() const { return fy_; }
  double skew() const { return s_; }
  double px() const { return u0_; }
  double py() const { return v0_; }
  double k1() const { return k1_; }
  double k2() const { return k2_; }
  double p1() const { return p1_; }
  double p2() const { return p2_; }
 private:
  double fx_ = 1, fy_ = 1, s_ = 0, u0_ = 0, v0_ = 0, k1_ = 0, k2_ = 0, p1_ = 0, p2_ = 0;
};
namespace detail {
// what a calibration hands to the device: {fx, fy, s, u0, v0} for a linear one, + {k1, k2, p1, p2} for Cal3DS2.  A user-defined
// CALIBRATION with the Cal3_S2 accessors works through the first overload (the documented hook: anything that is linear in the
// intrinsic point); anything else needs its uncalibrate() in k_meas.
template <class CAL> inline std::vector<double> calibration_vector(const CAL &K) { return {K.fx(), K.fy(), K.skew(), K.px(), K.py()}; }
inline std::vector<double> calibration_vector(const Cal3DS2 &K) { return {K.fx(), K.fy(), K.skew(), K.px(), K.py(), K.k1(), K.k2(), K.p1(), K.p2()}; }
inline Point2 uncalibrate(const std::vector<double> &K, double x, double y) {
  if (K.size() == 9) {
    const double rr = x * x + y * y, g = 1.0 + K[5] * rr + K[6] * rr * rr;
    const double dx = 2.0 * K[7] * x * y + K[8] * (rr + 2.0 * x * x), dy = 2.0 * K[8] * x * y + K[7] * (rr + 2.0 * y * y);
    x = g * x + dx; y = g * y + dy;
  }
  return Point2(K[0] * x + K[2] * y + K[3], K[1] * y + K[4]);
}
}  // namespace detail

/// gtsam::PinholeCamera<CALIBRATION>::project -- host-side helper for building measurements (as the reference's
/// tests do with cam.project(land), testGPInterpolatedProjectionFactorPose3.cpp:131-134); not part of the device path.
template <class CALIBRATION> class PinholeCamera {
 public:
  PinholeCamera(const Pose3 &pose, const CALIBRATION &K) : pose_(pose), K_(K) {}
  Point2 project(const Point3 &p) const {
    const double dx = p.x - pose_.t.x, dy = p.y - pose_.t.y, dz = p.z - pose_.t.z;
    const double *R = pose_.R.R;
    const double qx = R[0] * dx + R[3] * dy + R[6] * dz, qy = R[1] * dx + R[4] * dy + R[7] * dz, qz = R[2] * dx + R[5] * dy + R[8] * dz;
    if (!(qz > 0.0)) throw std::domain_error("CheiralityException: point behind the camera");
    return detail::uncalibrate(detail::calibration_vector(K_), qx / qz, qy / qz);
  }
 private:
  Pose3 pose_;
  CALIBRATION K_;
};

namespace noiseModel {
struct Base {
  int dim_ = 0;
  std::vector<double> sigmas_;   // diagonal models
  Matrix cov_;                   // full Gaussian (used for Qc)
  bool diagonal_ = true;
  int robust_ = 0;               // noiseModel::Robust: GPSLAM_ROBUST_* of the mEstimator on top of this model (0: none) and its k
  double robust_k_ = 0.0;
  int dim() const { return dim_; }
  Matrix covariance() const {
    if (!diagonal_) return cov_;
    Matrix m(dim_, dim_);
    for (int i = 0; i < dim_; i++) m(i, i) = sigmas_[i] * sigmas_[i];
    return m;
  }
};
typedef std::shared_ptr<Base> shared_ptr_base;
struct Isotropic { typedef std::shared_ptr<Base> shared_ptr;
  static shared_ptr Sigma(int dim, double sigma) { auto b = std::make_shared<Base>(); b->dim_ = dim; b->sigmas_.assign(dim, sigma); return b; } };
struct Diagonal { typedef std::shared_ptr<Base> shared_ptr;
  static shared_ptr Sigmas(const Vector &s) { auto b = std::make_shared<Base>(); b->dim_ = (int)s.size(); b->sigmas_ = s; return b; } };
struct Gaussian { typedef std::shared_ptr<Base> shared_ptr;
  static shared_ptr Covariance(const Matrix &c) {
    auto b = std::make_shared<Base>(); b->dim_ = c.rows; b->cov_ = c; b->diagonal_ = true;
    for (int i = 0; i < c.rows; i++) for (int j = 0; j < c.cols; j++) if (i != j && c(i, j) != 0.0) b->diagonal_ = false;
    if (b->diagonal_) { b->sigmas_.resize(c.rows); for (int i = 0; i < c.rows; i++) b->sigmas_[i] = std::sqrt(c(i, i)); }
    return b;
  } };
// gtsam/linear/LossFunctions.h: mEstimator::Huber / Cauchy / Tukey / GemanMcClure / Welsh / Fair, each Create(k); w(r) and rho(r) are
// those of include/gpslam_hip.h (gpslam_hip_robust_eval), Block reweighting (one weight per factor)
namespace mEstimator {
struct Base {
  typedef std::shared_ptr<Base> shared_ptr;
  int kind_ = 0;
  double k_ = 0.0;
  double weight(double r) const { double w = 1.0, rho = 0.0; (void)gpslam_hip_robust_eval(kind_, k_, r, &w, &rho); return w; }
  double loss(double r) const { double w = 1.0, rho = 0.0; (void)gpslam_hip_robust_eval(kind_, k_, r, &w, &rho); return rho; }
};
inline Base::shared_ptr make(int kind, double k) {
  if (!(k > 0.0) || !std::isfinite(k)) throw std::invalid_argument("mEstimator: the parameter k must be positive and finite");
  auto b = std::make_shared<Base>(); b->kind_ = kind; b->k_ = k; return b;
}
struct Huber { typedef Base::shared_ptr shared_ptr; static shared_ptr Create(double k = 1.345) { return make(GPSLAM_ROBUST_HUBER, k); } };
struct Cauchy { typedef Base::shared_ptr shared_ptr; static shared_ptr Create(double k = 0.1) { return make(GPSLAM_ROBUST_CAUCHY, k); } };
struct Tukey { typedef Base::shared_ptr shared_ptr; static shared_ptr Create(double k = 4.6851) { return make(GPSLAM_ROBUST_TUKEY, k); } };
struct GemanMcClure { typedef Base::shared_ptr shared_ptr; static shared_ptr Create(double k = 1.0) { return make(GPSLAM_ROBUST_GEMAN_MCCLURE, k); } };
struct Welsh { typedef Base::shared_ptr shared_ptr; static shared_ptr Create(double k = 2.9846) { return make(GPSLAM_ROBUST_WELSH, k); } };
struct Fair { typedef Base::shared_ptr shared_ptr; static shared_ptr Create(double k = 1.3998) { return make(GPSLAM_ROBUST_FAIR, k); } };
}  // namespace mEstimator
// noiseModel::Robust::Create(mEstimator, base model): measurement factors and loop closures (non-adjacent BetweenFactor) take it; the
// chain's own factors -- GP priors, PriorFactor, BetweenFactor(x_i, x_i+1) -- do not (they throw, naming the limitation)
struct Robust { typedef std::shared_ptr<Base> shared_ptr;
  static shared_ptr Create(const mEstimator::Base::shared_ptr &robust, const std::shared_ptr<Base> &noise) {
    if (!robust || !noise) throw std::invalid_argument("noiseModel::Robust::Create: null argument");
    auto b = std::make_shared<Base>(*noise); b->robust_ = robust->kind_; b->robust_k_ = robust->k_; return b;
  } };
}  // namespace noiseModel
typedef std::shared_ptr<noiseModel::Base> SharedNoiseModel;

// ---------------------------------------------------------------- Values
namespace detail {
enum VType { T_NONE, T_VEC2, T_VEC3, T_VEC6, T_POSE2, T_POSE3, T_ROT3, T_POINT2, T_POINT3 };
template <typename T> struct VT;
template <> struct VT<Vector2> { static constexpr VType t = T_VEC2; static std::vector<double> pack(const Vector2 &v) { return {v[0], v[1]}; } static Vector2 un(const std::vector<double> &d) { return {d[0], d[1]}; } };
template <> struct VT<Vector3> { static constexpr VType t = T_VEC3; static std::vector<double> pack(const Vector3 &v) { return {v[0], v[1], v[2]}; } static Vector3 un(const std::vector<double> &d) { return {d[0], d[1], d[2]}; } };
template <> struct VT<Vector6> { static constexpr VType t = T_VEC6; static std::vector<double> pack(const Vector6 &v) { return std::vector<double>(v.begin(), v.end()); } static Vector6 un(const std::vector<double> &d) { return {d[0], d[1], d[2], d[3], d[4], d[5]}; } };
template <> struct VT<Pose2> { static constexpr VType t = T_POSE2; static std::vector<double> pack(const Pose2 &p) { return {p.x, p.y, p.theta}; } static Pose2 un(const std::vector<double> &d) { return Pose2(d[0], d[1], d[2]); } };
template <> struct VT<Rot3> { static constexpr VType t = T_ROT3; static std::vector<double> pack(const Rot3 &r) { return std::vector<double>(r.R, r.R + 9); } static Rot3 un(const std::vector<double> &d) { Rot3 r; for (int i = 0; i < 9; i++) r.R[i] = d[i]; return r; } };
template <> struct VT<Pose3> { static constexpr VType t = T_POSE3;
  static std::vector<double> pack(const Pose3 &p) { std::vector<double> d(p.R.R, p.R.R + 9); d.push_back(p.t.x); d.push_back(p.t.y); d.push_back(p.t.z); return d; }
  static Pose3 un(const std::vector<double> &d) { Pose3 p; for (int i = 0; i < 9; i++) p.R.R[i] = d[i]; p.t = Point3(d[9], d[10], d[11]); return p; } };
template <> struct VT<Point2> { static constexpr VType t = T_POINT2; static std::vector<double> pack(const Point2 &p) { return {p.x, p.y}; } static Point2 un(const std::vector<double> &d) { return Point2(d[0], d[1]); } };
template <> struct VT<Point3> { static constexpr VType t = T_POINT3; static std::vector<double> pack(const Point3 &p) { return {p.x, p.y, p.z}; } static Point3 un(const std::vector<double> &d) { return Point3(d[0], d[1], d[2]); } };
struct Value { VType type = T_NONE; std::vector<double> d; };
}  // namespace detail

class Values {
 public:
  template <typename T> void insert(Key k, const T &v) {
    if (m_.count(k)) throw std::invalid_argument("Values::insert: key already exists");
    detail::Value val; val.type = detail::VT<T>::t; val.d = detail::VT<T>::pack(v); m_[k] = val;
  }
  template <typename T> T at(Key k) const {
    auto it = m_.find(k);
    if (it == m_.end()) throw std::out_of_range("Values::at: key does not exist");   // ValuesKeyDoesNotExist
    if (it->second.type != detail::VT<T>::t) throw std::invalid_argument("Values::at: wrong type");
    return detail::VT<T>::un(it->second.d);
  }
  bool exists(Key k) const { return m_.count(k) != 0; }
  size_t size() const { return m_.size(); }
  const std::map<Key, detail::Value> &raw() const { return m_; }
  std::map<Key, detail::Value> &raw() { return m_; }
 private:
  std::map<Key, detail::Value> m_;
};

// ---------------------------------------------------------------- factors
namespace detail {
enum FType { F_GP, F_POSE_PRIOR, F_VEL_PRIOR, F_LM_PRIOR, F_BETWEEN, F_INTERP_RANGE, F_RANGE, F_INTERP_ATT, F_INTERP_GPS, F_ODOM2D, F_BEARING_RANGE, F_INTERP_PROJ,
             F_BIAS_PRIOR, F_BIAS_BETWEEN, F_AHRS, F_ATTITUDE, F_STATE_GAUSS, F_BORDER_GAUSS };
struct Desc {   // what a factor hands to the graph compiler
  FType type;
  int manifold = -1;                 // GPSLAM_* the factor requires, -1 = any
  Key k[5] = {0, 0, 0, 0, 0};        // pose1, vel1, pose2, vel2, landmark (as applicable)
  Key kw[2] = {0, 0};                // omega1, omega2 of the *Pose3VW factors
  std::vector<Key> lmk;              // F_BORDER_GAUSS: the landmark keys, in the order of the factor's columns
  bool vw = false;                   // world-frame (v, w) velocity family
  std::vector<double> meas, sig, sensor, aux;
  std::vector<double> cov;           // measurement factors with a noiseModel::Gaussian (full covariance): rows x rows, else empty
  int32_t robust = 0;                // noiseModel::Robust: GPSLAM_ROBUST_* and its parameter (measurement factors, loop closures)
  double robust_k = 0.0;
  double dt = 0, tau = 0;
  Matrix Qc;
};
inline bool close(const std::vector<double> &a, const std::vector<double> &b, double tol) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); i++) if (!(std::fabs(a[i] - b[i]) < tol) && a[i] != b[i]) return false;
  return true;
}
// NoiseModelFactor::equals of the reference's factors (e.g. GaussianProcessPriorPose3.h:106-109): keys and noise model through
// Base::equals, then the members the class compares itself -- measurement, sensor pose / calibration, and the GP base
// (delta_t, tau, Qc) unless the class leaves it out (gp = false: GPInterpolatedRangeFactor2DLinear.h:96-100)
inline bool desc_equals(const Desc &a, const Desc &b, double tol, bool gp) {
  if (a.type != b.type || a.manifold != b.manifold || a.vw != b.vw) return false;
  for (int i = 0; i < 5; i++) if (a.k[i] != b.k[i]) return false;
  for (int i = 0; i < 2; i++) if (a.kw[i] != b.kw[i]) return false;
  if (a.lmk != b.lmk) return false;
  if (!close(a.meas, b.meas, tol) || !close(a.sig, b.sig, tol) || !close(a.cov, b.cov, tol)) return false;
  if (!close(a.sensor, b.sensor, tol) || !close(a.aux, b.aux, tol)) return false;
  if (a.robust != b.robust || !(std::fabs(a.robust_k - b.robust_k) < tol || a.robust_k == b.robust_k)) return false;
  if (a.type == F_GP) return std::fabs(a.dt - b.dt) < tol && close(a.Qc.a, b.Qc.a, tol);   // (the prior's noise model IS Q(Qc, delta_t))
  if (!gp) return true;
  return std::fabs(a.dt - b.dt) < tol && std::fabs(a.tau - b.tau) < tol && close(a.Qc.a, b.Qc.a, tol);
}
inline void desc_print(const Desc &d, const std::string &s, const char *name, int nkeys, const KeyFormatter &kf) {
  std::cout << s << name << std::endl;
  std::cout << "  keys = {";
  // which key slots this kind of factor fills, in the order of its constructor's key arguments (slots 0..4 = k[], 5 / 6 = kw[]).
  // The VALUE of a key says nothing: plain integer keys are legal and 0 is one of them (a zero key used to be dropped).
  int slots[7], ns = 0;
  auto put = [&](std::initializer_list<int> l) { for (int v : l) slots[ns++] = v; };
  const bool lm2 = d.type == F_RANGE || d.type == F_BEARING_RANGE;
  switch (nkeys) {
    case 1: put({0}); break;
    case 2: if (lm2) put({0, 4}); else put({0, 2}); break;
    case 3: put({0, 2, 4}); break;                                   // AHRSFactor(rot_i, rot_j, bias)
    case 4: put({0, 1, 2, 3}); break;
    case 5: put({0, 1, 2, 3, 4}); break;
    case 6: put({0, 1, 5, 2, 3, 6}); break;                          // *Pose3VW: (pose1, vel1, omega1, pose2, vel2, omega2)
    default: put({0, 1, 5, 2, 3, 6, 4}); break;                      // ... with a landmark
  }
  for (int i = 0; i < ns && i < nkeys; i++) std::cout << " " << kf(slots[i] < 5 ? d.k[slots[i]] : d.kw[slots[i] - 5]);
  std::cout << " }" << std::endl;
  auto vec = [](const char *label, const std::vector<double> &v) {
    if (v.empty()) return;
    std::cout << "  " << label << " = [";
    for (size_t i = 0; i < v.size(); i++) std::cout << (i ? ", " : "") << v[i];
    std::cout << "]" << std::endl;
  };
  vec("measured", d.meas);
  if (d.cov.empty()) vec("noise model: diagonal sigmas", d.sig); else vec("noise model: Gaussian covariance", d.cov);
  if (d.robust) std::cout << "  robust: mEstimator " << d.robust << ", k = " << d.robust_k << std::endl;
  vec("body_P_sensor", d.sensor);
  vec("calibration", d.aux);
  if (d.dt != 0) std::cout << "  delta_t = " << d.dt << (d.type == F_GP ? "" : ", tau = " + std::to_string(d.tau)) << std::endl;
  if (!d.Qc.a.empty()) vec("Qc", d.Qc.a);
}
}  // namespace detail

class NonlinearFactor {
 public:
  typedef std::shared_ptr<NonlinearFactor> shared_ptr;
  virtual ~NonlinearFactor() {}
  virtual detail::Desc describe() const = 0;
  virtual size_t size() const = 0;
  virtual shared_ptr clone() const = 0;
  /// gtsam::NonlinearFactor::equals / print (every factor class overrides both, as in the reference: e.g.
  /// gpslam/gp/GaussianProcessPriorPose3.h:104-115)
  virtual bool equals(const NonlinearFactor &expected, double tol = 1e-9) const = 0;
  virtual void print(const std::string &s = "", const KeyFormatter &keyFormatter = DefaultKeyFormatter) const = 0;
};

inline std::vector<double> sigmas_of(const SharedNoiseModel &m, bool robust_ok = false) {
  if (m && m->robust_ && !robust_ok)
    throw std::invalid_argument("noiseModel::Robust is supported on measurement factors and loop closures only, not on the chain's own factors (GP priors, PriorFactor, BetweenFactor of consecutive states)");
  if (!m || !m->diagonal_) throw std::invalid_argument("the noise model of PriorFactor / BetweenFactor must be diagonal (Isotropic / Diagonal)");
  return m->sigmas_;
}
// the measurement factors take any Gaussian model, as the reference's constructors do (GPInterpolatedGPSFactorPose3.h:46-54):
// a full covariance travels in Desc::cov and reaches the device through gpslam_hip_set_meas_covariance
inline void noise_of(const SharedNoiseModel &m, detail::Desc &d) {
  if (!m) throw std::invalid_argument("null noise model");
  d.robust = m->robust_; d.robust_k = m->robust_k_;      // noiseModel::Robust: the loss rides on top of the base model below
  if (m->diagonal_) { d.sig = m->sigmas_; d.cov.clear(); return; }
  d.cov = m->cov_.a;
  d.sig.resize(m->dim_);
  for (int i = 0; i < m->dim_; i++) d.sig[i] = std::sqrt(m->cov_(i, i));
}

// NAME: the first line print() writes (the reference's own strings); EQ_GP: equals() compares the GP base (delta_t, tau, Qc)
#define GPSLAM_FACTOR_BOILERPLATE_NAMED(CLS, NKEYS, NAME, EQ_GP)                                        \
  size_t size() const override { return NKEYS; }                                                        \
  gtsam::NonlinearFactor::shared_ptr clone() const override { return std::make_shared<CLS>(*this); }    \
  gtsam::detail::Desc describe() const override { return d_; }                                          \
  bool equals(const gtsam::NonlinearFactor &expected, double tol = 1e-9) const override {               \
    const CLS *e = dynamic_cast<const CLS *>(&expected);                                                \
    return e != nullptr && gtsam::detail::desc_equals(d_, e->d_, tol, EQ_GP);                           \
  }                                                                                                     \
  void print(const std::string &s = "", const gtsam::KeyFormatter &keyFormatter = gtsam::DefaultKeyFormatter) const override { \
    gtsam::detail::desc_print(d_, s, NAME, NKEYS, keyFormatter);                                        \
  }                                                                                                     \
 protected:                                                                                             \
  gtsam::detail::Desc d_;                                                                               \
 public:
#define GPSLAM_FACTOR_BOILERPLATE(CLS, NKEYS) GPSLAM_FACTOR_BOILERPLATE_NAMED(CLS, NKEYS, #CLS, true)

template <typename T> class PriorFactor : public NonlinearFactor {
 public:
  PriorFactor(Key key, const T &prior, const SharedNoiseModel &model) {
    constexpr detail::VType vt = detail::VT<T>::t;
    const unsigned char c = symbolChr(key);
    if (vt == detail::T_POINT2 || vt == detail::T_POINT3) d_.type = detail::F_LM_PRIOR;
    else if (c == 'v') d_.type = detail::F_VEL_PRIOR;
    else if (c == 'b' && vt == detail::T_VEC3) d_.type = detail::F_BIAS_PRIOR;   // PriorFactorVector(b_1) of the AHRS recipe
    else d_.type = detail::F_POSE_PRIOR;
    d_.k[0] = key; d_.meas = detail::VT<T>::pack(prior); d_.sig = sigmas_of(model);
  }
  GPSLAM_FACTOR_BOILERPLATE(PriorFactor<T>, 1)
};

template <typename T> class BetweenFactor : public NonlinearFactor {
 public:
  BetweenFactor(Key key1, Key key2, const T &measured, const SharedNoiseModel &model) {
    d_.type = (symbolChr(key1) == 'b' && detail::VT<T>::t == detail::T_VEC3) ? detail::F_BIAS_BETWEEN : detail::F_BETWEEN;
    d_.k[0] = key1; d_.k[2] = key2; d_.meas = detail::VT<T>::pack(measured); d_.sig = sigmas_of(model, true);
    d_.robust = model->robust_; d_.robust_k = model->robust_k_;   // (a loop closure may carry a loss; a chain factor throws at compile)
  }
  GPSLAM_FACTOR_BOILERPLATE(BetweenFactor<T>, 2)
};

// ---------------------------------------------------------------- optimizer parameters (GTSAM names and defaults)
struct NonlinearOptimizerParams {
  int maxIterations = 100;
  double relativeErrorTol = 1e-5, absoluteErrorTol = 1e-5, errorTol = 0.0;
  std::string verbosity = "SILENT";
  void setVerbosity(const std::string &v) { verbosity = v; }
  void setMaxIterations(int v) { maxIterations = v; }
  void setRelativeErrorTol(double v) { relativeErrorTol = v; }
  void setAbsoluteErrorTol(double v) { absoluteErrorTol = v; }
};
struct GaussNewtonParams : NonlinearOptimizerParams {};
struct LevenbergMarquardtParams : NonlinearOptimizerParams {
  double lambdaInitial = 1e-5, lambdaFactor = 10.0, lambdaUpperBound = 1e5, lambdaLowerBound = 0.0, minModelFidelity = 1e-3;
  void setlambdaInitial(double v) { lambdaInitial = v; }
  void setlambdaFactor(double v) { lambdaFactor = v; }
  void setlambdaUpperBound(double v) { lambdaUpperBound = v; }
};
/// gtsam::DoglegParams: deltaInitial is the first trust radius.  adaptationMode is DoglegOptimizerImpl::TrustRegionAdaptationMode
/// (DoglegOptimizer itself always iterates ONE_STEP_PER_ITERATION; the other two are what ISAM2DoglegParams may choose)
struct DoglegParams : NonlinearOptimizerParams {
  enum TrustRegionAdaptationMode { ONE_STEP_PER_ITERATION = GPSLAM_DOGLEG_ONE_STEP_PER_ITERATION,
                                   SEARCH_EACH_ITERATION = GPSLAM_DOGLEG_SEARCH_EACH_ITERATION,
                                   SEARCH_REDUCE_ONLY = GPSLAM_DOGLEG_SEARCH_REDUCE_ONLY };
  double deltaInitial = 1.0;
  TrustRegionAdaptationMode adaptationMode = ONE_STEP_PER_ITERATION;
  void setDeltaInitial(double v) { deltaInitial = v; }
  double getDeltaInitial() const { return deltaInitial; }
};

class NonlinearFactorGraph {
 public:
  template <typename F> void add(const F &f) { f_.push_back(std::make_shared<F>(f)); }
  void push_back(const NonlinearFactor::shared_ptr &f) { f_.push_back(f); }
  size_t size() const { return f_.size(); }
  const std::vector<NonlinearFactor::shared_ptr> &factors() const { return f_; }
  inline double error(const Values &values) const;   // 0.5 * sum |R e|^2, evaluated on the GPU
 private:
  std::vector<NonlinearFactor::shared_ptr> f_;
};

// ---------------------------------------------------------------- graph compile + device session
namespace detail {

// The structs of include/gpslam_hip.h are written into by the library: before the first handle is created, the library this process
// loaded must report the header's major version and the header's struct sizes (gpslam_hip_stats grew in round 5 with
// nothing to tell an old caller).  Throws; checked once.
inline void check_abi() {
  static const bool ok = [] {
    const uint32_t v = gpslam_hip_abi_version();
    if ((v >> 16) != (uint32_t)GPSLAM_HIP_ABI_MAJOR || (v & 0xffffu) < (uint32_t)GPSLAM_HIP_ABI_MINOR)
      throw std::runtime_error("libgpslam_hip.so speaks ABI " + std::to_string(v >> 16) + "." + std::to_string(v & 0xffffu) + ", this header " +
                               std::to_string(GPSLAM_HIP_ABI_MAJOR) + "." + std::to_string(GPSLAM_HIP_ABI_MINOR));
    if (gpslam_hip_struct_size(GPSLAM_STRUCT_CONFIG_V2) != sizeof(gpslam_hip_config_v2) || gpslam_hip_struct_size(GPSLAM_STRUCT_STATS) != sizeof(gpslam_hip_stats) ||
        gpslam_hip_struct_size(GPSLAM_STRUCT_PARAMS) != sizeof(gpslam_hip_params) || gpslam_hip_struct_size(GPSLAM_STRUCT_CONFIG) != sizeof(gpslam_hip_config))
      throw std::runtime_error("libgpslam_hip.so was built from another include/gpslam_hip.h: struct sizes differ");
    return true;
  }();
  (void)ok;
}
// a zeroed gpslam_hip_config_v2 with its size filled in (every knob by name; one segment)
inline gpslam_hip_config_v2 make_config(int manifold, int device = 0) {
  check_abi();
  gpslam_hip_config_v2 cfg;
  std::memset(&cfg, 0, sizeof(cfg));
  cfg.struct_size = (uint32_t)sizeof(cfg);
  cfg.manifold = manifold; cfg.precision = GPSLAM_FP64; cfg.device = device; cfg.nranks = 1;
  cfg.chart = (manifold == GPSLAM_POSE2) ? GPSLAM_CHART_FIRST_ORDER : GPSLAM_CHART_EXPMAP;   // GTSAM's default charts
  return cfg;
}

inline void check(int rc, gpslam_hip_handle *h, const char *what) {
  if (rc < 0) {
    std::string msg = std::string(what) + " failed (" + std::to_string(rc) + "): " + (h ? gpslam_hip_last_error(h) : "");
    if (rc == GPSLAM_E_INVALID || rc == GPSLAM_E_UNSUPPORTED) throw std::invalid_argument(msg);
    throw std::runtime_error(msg);   // GPSLAM_E_NOT_SPD ~ IndeterminantLinearSystemException, GPSLAM_E_HIP
  }
}

struct Session {
  gpslam_hip_handle *h = nullptr;
  int manifold = -1, d = 0, pd = 0, ld = 0, N = 0, L = 0;
  std::vector<uint64_t> state_index;        // sorted symbol indices of the states
  std::vector<uint64_t> lm_index;
  std::vector<bool> has_vel;                // velocity key present in the user's Values
  bool vw = false;                          // Pose3VW family: 'v' and 'w' keys hold world-frame 3-vectors
  bool bias = false;                        // AHRS graph: 'b' keys (gyroscope bias) ride in the pose slot of a GPSLAM_ROT3_BIAS chain
  Values values;
  ~Session() { if (h) gpslam_hip_destroy(h); }

  static int manifold_of(VType t) {
    switch (t) { case T_VEC2: return GPSLAM_LINEAR2; case T_VEC3: return GPSLAM_LINEAR3; case T_POSE2: return GPSLAM_POSE2;
      case T_POSE3: return GPSLAM_POSE3; case T_ROT3: return GPSLAM_ROT3; default: return -1; }
  }
  int state_of(Key k) const {
    const uint64_t idx = symbolIndex(k);
    for (size_t i = 0; i < state_index.size(); i++) if (state_index[i] == idx) return (int)i;
    throw std::invalid_argument("factor refers to a state that is not in the Values");
  }
  int lm_of(Key k) const {
    const uint64_t idx = symbolIndex(k);
    for (size_t i = 0; i < lm_index.size(); i++) if (lm_index[i] == idx) return (int)i;
    throw std::invalid_argument("factor refers to a landmark that is not in the Values");
  }

  // classify the variables, map keys to chain positions, create the handle, upload states
  void build(const NonlinearFactorGraph &graph, const Values &init, int device = 0) {
    values = init;
    std::map<uint64_t, const Value *> poses, vels, omegas, lms, biases;
    bool any_vw = false, any_body = false;
    for (auto &fp : graph.factors()) {
      const Desc f = fp->describe();
      if (f.vw) any_vw = true;
      else if (f.type == F_GP || f.type == F_INTERP_RANGE || f.type == F_INTERP_GPS || f.type == F_INTERP_PROJ || f.type == F_INTERP_ATT) any_body = true;
    }
    if (any_vw && any_body) throw std::invalid_argument("Pose3VW factors cannot be mixed with body-velocity GP factors in one graph");
    vw = any_vw;
    for (auto &kv : init.raw()) {
      const unsigned char c = symbolChr(kv.first);
      if (kv.second.type == T_POINT2 || kv.second.type == T_POINT3) lms[symbolIndex(kv.first)] = &kv.second;
      else if (c == 'v') vels[symbolIndex(kv.first)] = &kv.second;
      else if (vw && c == 'w') omegas[symbolIndex(kv.first)] = &kv.second;
      else if (c == 'b' && kv.second.type == T_VEC3) biases[symbolIndex(kv.first)] = &kv.second;
      else poses[symbolIndex(kv.first)] = &kv.second;
    }
    if (poses.empty()) throw std::invalid_argument("no pose variables (keys other than 'v' / landmarks) in the Values");
    manifold = manifold_of(poses.begin()->second->type);
    if (manifold < 0) throw std::invalid_argument("unsupported pose type");
    if (!biases.empty()) {   // matlab/GPAHRSexample.m: x_i Rot3, v_i Vector3, b_i Vector3 -> one (rotation, bias | omega, pad) state
      if (manifold != GPSLAM_ROT3) throw std::invalid_argument("bias variables ('b' keys) need Rot3 states");
      manifold = GPSLAM_ROT3_BIAS;
      bias = true;
    }
    static const int dd[6] = {2, 3, 3, 6, 3, 6}, pdd[6] = {2, 3, 3, 12, 9, 12};
    d = dd[manifold]; pd = pdd[manifold];
    ld = lms.empty() ? 0 : (lms.begin()->second->type == T_POINT2 ? 2 : 3);
    N = (int)poses.size(); L = (int)lms.size();
    std::vector<double> P((size_t)N * pd), V((size_t)N * d, 0.0), LM((size_t)L * (ld ? ld : 1));
    int i = 0;
    for (auto &kv : poses) {
      if (manifold_of(kv.second->type) != (bias ? (int)GPSLAM_ROT3 : manifold)) throw std::invalid_argument("mixed pose types");
      state_index.push_back(kv.first);
      std::memcpy(&P[(size_t)i * pd], kv.second->d.data(), sizeof(double) * (bias ? 9 : pd));
      if (bias) {
        auto bi = biases.find(kv.first);
        if (bi != biases.end()) std::memcpy(&P[(size_t)i * pd + 9], bi->second->d.data(), sizeof(double) * 3);
        else std::memset(&P[(size_t)i * pd + 9], 0, sizeof(double) * 3);
      }
      auto vi = vels.find(kv.first);
      has_vel.push_back(vi != vels.end());
      if (vi != vels.end()) {
        const int want = (vw || bias) ? 3 : d;
        if ((int)vi->second->d.size() != want) throw std::invalid_argument("velocity dimension does not match the pose manifold");
        std::memcpy(&V[(size_t)i * d], vi->second->d.data(), sizeof(double) * want);
      }
      if (vw) {   // state velocity slot = [v; w] (include/gpslam_hip.h, GPSLAM_VELOCITY_WORLD_VW)
        auto wi = omegas.find(kv.first);
        if (wi != omegas.end()) {
          if (wi->second->d.size() != 3) throw std::invalid_argument("omega variables are Vector3");
          std::memcpy(&V[(size_t)i * d + 3], wi->second->d.data(), sizeof(double) * 3);
        }
      }
      i++;
    }
    i = 0;
    for (auto &kv : lms) { lm_index.push_back(kv.first); std::memcpy(&LM[(size_t)i * ld], kv.second->d.data(), sizeof(double) * ld); i++; }
    gpslam_hip_config_v2 cfg = make_config(manifold, device);
    cfg.landmark_dim = ld;
    if (vw) {
      if (manifold != GPSLAM_POSE3) throw std::invalid_argument("Pose3VW factors need Pose3 states");
      cfg.velocity = GPSLAM_VELOCITY_WORLD_VW;
    }
    int rc = gpslam_hip_create_v2(&cfg, &h);
    if (rc < 0) throw std::runtime_error("gpslam_hip_create_v2 failed: no usable HIP device (there is no CPU fallback)");
    check(gpslam_hip_set_states(h, N, P.data(), V.data()), h, "set_states");
    if (L > 0) check(gpslam_hip_set_landmarks(h, L, LM.data()), h, "set_landmarks");
    add_factors(graph);
    finish(0);
  }

  bool qc_set = false;
  // qcStatistic: GP priors whose Qc_model is the handle's shared Qc (the first one seen) go in as sharing it, not with a copy of
  // their own -- the statistic sums the priors that share it (include/gpslam_hip_qc.h); everything else builds as it always did
  bool share_qc = false;
  std::vector<double> qc_shared;
  int closures = 0;                 // BetweenFactors between non-adjacent states
  // the factors of `graph` onto the handle: build(), and BatchFixedLagSmoother::update for the factors that arrive later
  void add_factors(const NonlinearFactorGraph &graph) {
    std::vector<double> qc_used;
    for (auto &fp : graph.factors()) {
      const Desc f = fp->describe();
      if (f.manifold >= 0 && f.manifold != manifold && !(bias && f.manifold == GPSLAM_ROT3))
        throw std::invalid_argument("factor type does not match the pose type in the Values");
      auto set_qc = [&](const Matrix &Qc) {
        if (Qc.rows != (bias ? 3 : d)) throw std::invalid_argument("Qc_model dimension does not match the manifold");
        // (the handle's shared Qc serves the interpolation queries; GP priors carry their own Qc_model -- below --, and
        //  the interpolated measurement factors do not depend on theirs: Qc cancels in Lambda and Psi)
        if (!qc_set) { check(gpslam_hip_set_qc(h, Qc.a.data()), h, "set_qc"); qc_set = true; qc_used = Qc.a; qc_shared = Qc.a; }
      };
      auto gaussian = [&](int kind) {   // noiseModel::Gaussian::Covariance / noiseModel::Robust on the factor just added
        if (!f.cov.empty()) check(gpslam_hip_set_meas_covariance(h, kind, 1, f.cov.data()), h, "set_meas_covariance");
        if (f.robust) check(gpslam_hip_set_meas_robust(h, kind, 1, &f.robust, &f.robust_k), h, "set_meas_robust");
      };
      auto adjacent = [&](Key k1, Key k2) {
        const int s1 = state_of(k1), s2 = state_of(k2);
        if (s2 != s1 + 1) throw std::invalid_argument("factors may couple a state only with its successor (chain structure)");
        return s1;
      };
      const double *sens = f.sensor.empty() ? nullptr : f.sensor.data();
      switch (f.type) {
        case F_GP: {
          set_qc(f.Qc);
          if (symbolIndex(f.k[0]) != symbolIndex(f.k[1]) || symbolIndex(f.k[2]) != symbolIndex(f.k[3]) ||
              (f.vw && (symbolIndex(f.kw[0]) != symbolIndex(f.k[0]) || symbolIndex(f.kw[1]) != symbolIndex(f.k[2]))))
            throw std::invalid_argument("GP prior: pose and velocity keys of a state must share their index");
          int32_t l = adjacent(f.k[0], f.k[2]);
          if (share_qc && f.Qc.a == qc_shared) check(gpslam_hip_add_gp_priors(h, 1, &l, &f.dt), h, "add_gp_priors");
          else check(gpslam_hip_add_gp_priors_qc(h, 1, &l, &f.dt, f.Qc.a.data()), h, "add_gp_priors_qc");   // one Qc_model per factor
        } break;
        case F_POSE_PRIOR: {
          int32_t s = state_of(f.k[0]);
          if (bias) {   // PriorFactorRot3 on the rotation half of the (rotation, bias) state; the bias half is switched off
            std::vector<double> m(12, 0.0), sg(6, INFINITY);
            std::memcpy(m.data(), f.meas.data(), sizeof(double) * 9);
            std::memcpy(sg.data(), f.sig.data(), sizeof(double) * 3);
            check(gpslam_hip_add_pose_priors(h, 1, &s, m.data(), sg.data()), h, "add_pose_priors");
          } else {
            check(gpslam_hip_add_pose_priors(h, 1, &s, f.meas.data(), f.sig.data()), h, "add_pose_priors");
          }
        } break;
        case F_BIAS_PRIOR: {
          if (!bias) throw std::invalid_argument("PriorFactor on a 'b' key needs bias variables in the Values");
          int32_t s = state_of(f.k[0]);
          std::vector<double> m = {1, 0, 0, 0, 1, 0, 0, 0, 1, f.meas[0], f.meas[1], f.meas[2]};
          std::vector<double> sg = {INFINITY, INFINITY, INFINITY, f.sig[0], f.sig[1], f.sig[2]};
          check(gpslam_hip_add_pose_priors(h, 1, &s, m.data(), sg.data()), h, "add_pose_priors");
        } break;
        case F_BIAS_BETWEEN: {
          if (!bias) throw std::invalid_argument("BetweenFactor on 'b' keys needs bias variables in the Values");
          if (f.robust) throw std::invalid_argument("noiseModel::Robust on a BetweenFactor of consecutive states: the chain's own factors take no loss");
          int32_t l = adjacent(f.k[0], f.k[2]);
          std::vector<double> m = {1, 0, 0, 0, 1, 0, 0, 0, 1, f.meas[0], f.meas[1], f.meas[2]};
          std::vector<double> sg = {INFINITY, INFINITY, INFINITY, f.sig[0], f.sig[1], f.sig[2]};
          check(gpslam_hip_add_between(h, 1, &l, m.data(), sg.data()), h, "add_between");
        } break;
        case F_AHRS: {   // gtsam::AHRSFactor(x_i, x_j, b_i, pim, omegaCoriolis): meas = deltaRij | delRdelBiasOmega | biasHat | deltaTij | cov
          if (!bias) throw std::invalid_argument("AHRSFactor needs bias variables ('b' keys) in the Values");
          int32_t l = adjacent(f.k[0], f.k[2]);
          if (symbolIndex(f.k[4]) != symbolIndex(f.k[0])) throw std::invalid_argument("AHRSFactor: the bias key must belong to the first rotation's state");
          check(gpslam_hip_add_ahrs(h, 1, &l, &f.meas[0], &f.meas[9], &f.meas[18], &f.meas[21], &f.meas[22], f.aux.empty() ? nullptr : f.aux.data()), h, "add_ahrs");
        } break;
        case F_ATTITUDE: {   // gtsam::Rot3AttitudeFactor(x_s): the interpolated factor at tau = delta_t sits exactly on the right state
          if (manifold != GPSLAM_ROT3 && manifold != GPSLAM_ROT3_BIAS) throw std::invalid_argument("Rot3AttitudeFactor needs Rot3 states");
          const int st = state_of(f.k[0]);
          int32_t l = st > 0 ? st - 1 : 0;
          const double one = 1.0, tau = st > 0 ? 1.0 : 0.0;
          if (N < 2) throw std::invalid_argument("Rot3AttitudeFactor needs a chain of at least two states");
          check(gpslam_hip_add_interp_attitude(h, 1, &l, f.aux.data(), f.aux.data() + 3, f.sig.data(), &one, &tau), h, "add_interp_attitude");
          gaussian(GPSLAM_MEAS_INTERP_ATTITUDE);
        } break;
        case F_VEL_PRIOR: { if (vw) throw std::invalid_argument("PriorFactor<Vector3> on a 'v' / 'w' key of a Pose3VW graph is not supported yet");
          int32_t s = state_of(f.k[0]);
          std::vector<double> m = f.meas, sg = f.sig;
          if (bias) { m.resize(6, 0.0); sg.resize(6, 1.0); }     // the three pad components of the velocity slot
          check(gpslam_hip_add_vel_priors(h, 1, &s, m.data(), sg.data()), h, "add_vel_priors"); } break;
        case F_LM_PRIOR: { int32_t s = lm_of(f.k[0]); check(gpslam_hip_add_landmark_priors(h, 1, &s, f.meas.data(), f.sig.data()), h, "add_landmark_priors"); } break;
        case F_BETWEEN: {   // any two states: consecutive ones are a chain factor, anything else a loop closure (round 6)
          int32_t s1 = state_of(f.k[0]), s2 = state_of(f.k[2]);
          if (f.robust && (s2 == s1 + 1 || f.type == F_BIAS_BETWEEN))
            throw std::invalid_argument("noiseModel::Robust on a BetweenFactor of consecutive states: the chain's own factors take no loss (loop closures do)");
          if (bias) {   // BetweenFactorRot3 on the rotation half
            std::vector<double> m(12, 0.0), sg(6, INFINITY);
            std::memcpy(m.data(), f.meas.data(), sizeof(double) * 9);
            std::memcpy(sg.data(), f.sig.data(), sizeof(double) * 3);
            check(gpslam_hip_add_between_pairs(h, 1, &s1, &s2, m.data(), sg.data()), h, "add_between_pairs");
          } else {
            check(gpslam_hip_add_between_pairs(h, 1, &s1, &s2, f.meas.data(), f.sig.data()), h, "add_between_pairs");
          }
          if (f.robust) check(gpslam_hip_set_between_pairs_robust(h, 1, &f.robust, &f.robust_k), h, "set_between_pairs_robust");
          if (s2 != s1 + 1) closures++;
        } break;
        case F_INTERP_RANGE: { set_qc(f.Qc); int32_t l = adjacent(f.k[0], f.k[2]), m = lm_of(f.k[4]);
          check(gpslam_hip_add_interp_range(h, 1, &l, &m, f.meas.data(), f.sig.data(), &f.dt, &f.tau, sens), h, "add_interp_range"); gaussian(GPSLAM_MEAS_INTERP_RANGE); } break;
        case F_RANGE: { int32_t s = state_of(f.k[0]), m = lm_of(f.k[4]); check(gpslam_hip_add_range(h, 1, &s, &m, f.meas.data(), f.sig.data()), h, "add_range"); gaussian(GPSLAM_MEAS_RANGE); } break;
        case F_INTERP_ATT: { set_qc(f.Qc); int32_t l = adjacent(f.k[0], f.k[2]);
          check(gpslam_hip_add_interp_attitude(h, 1, &l, f.aux.data(), f.aux.data() + 3, f.sig.data(), &f.dt, &f.tau), h, "add_interp_attitude"); gaussian(GPSLAM_MEAS_INTERP_ATTITUDE); } break;
        case F_INTERP_GPS: { set_qc(f.Qc); int32_t l = adjacent(f.k[0], f.k[2]);
          check(gpslam_hip_add_interp_gps(h, 1, &l, f.meas.data(), f.sig.data(), &f.dt, &f.tau, sens), h, "add_interp_gps"); gaussian(GPSLAM_MEAS_INTERP_GPS); } break;
        case F_ODOM2D: { int32_t l = adjacent(f.k[0], f.k[2]); check(gpslam_hip_add_odometry2d(h, 1, &l, f.meas.data(), f.sig.data()), h, "add_odometry2d"); gaussian(GPSLAM_MEAS_ODOMETRY2D); } break;
        case F_BEARING_RANGE: { int32_t s = state_of(f.k[0]), m = lm_of(f.k[4]);
          check(gpslam_hip_add_bearing_range(h, 1, &s, &m, &f.meas[0], &f.meas[1], f.sig.data()), h, "add_bearing_range"); gaussian(GPSLAM_MEAS_BEARING_RANGE); } break;
        case F_INTERP_PROJ: { set_qc(f.Qc); int32_t l = adjacent(f.k[0], f.k[2]), m = lm_of(f.k[4]);
          check((f.aux.size() == 9 ? gpslam_hip_add_interp_projection_ds2 : gpslam_hip_add_interp_projection)(h, 1, &l, &m, f.meas.data(), f.sig.data(), &f.dt, &f.tau, f.aux.data(), sens), h,
                "add_interp_projection"); gaussian(GPSLAM_MEAS_INTERP_PROJECTION); } break;
        case F_STATE_GAUSS: {   // gtsam::LinearContainerFactor over (x_s, v_s): meas = [pose_lin | vel_lin], aux = A, sig = c
          if (vw || bias) throw std::invalid_argument("LinearContainerFactor: not on Pose3VW or AHRS graphs");
          if (symbolIndex(f.k[0]) != symbolIndex(f.k[1])) throw std::invalid_argument("LinearContainerFactor: pose and velocity keys of a state must share their index");
          if ((int)f.meas.size() != pd + d || (int)f.aux.size() != 4 * d * d || (int)f.sig.size() != 2 * d)
            throw std::invalid_argument("LinearContainerFactor: A must be 2d x 2d and b 2d for the manifold of the Values");
          int32_t st = state_of(f.k[0]);
          check(gpslam_hip_add_state_gaussians(h, 1, &st, f.meas.data(), f.meas.data() + pd, f.aux.data(), f.sig.data()), h, "add_state_gaussians");
        } break;
        case F_BORDER_GAUSS: {   // gtsam::LinearContainerFactor over (x_s, v_s, l_0 .. l_{L-1}): meas = [pose_lin | vel_lin | lm_lin], aux = A, sig = c
          if (vw || bias) throw std::invalid_argument("LinearContainerFactor: not on Pose3VW or AHRS graphs");
          if (symbolIndex(f.k[0]) != symbolIndex(f.k[1])) throw std::invalid_argument("LinearContainerFactor: pose and velocity keys of a state must share their index");
          if ((int)f.lmk.size() != L) throw std::invalid_argument("LinearContainerFactor: a factor over a state and landmarks names every landmark of the Values");
          for (int i = 0; i < L; i++)
            if (lm_of(f.lmk[i]) != i) throw std::invalid_argument("LinearContainerFactor: the landmark keys must stand in the order of their indices");
          const int n = 2 * d + L * ld;
          if ((int)f.meas.size() != pd + d + L * ld || (int)f.aux.size() != n * n || (int)f.sig.size() != n)
            throw std::invalid_argument("LinearContainerFactor: A must be n x n and b n, n = 2d + the landmarks' coordinates");
          int32_t st = state_of(f.k[0]);
          check(gpslam_hip_add_border_gaussians(h, 1, &st, f.meas.data(), f.meas.data() + pd, f.meas.data() + pd + d, f.aux.data(), f.sig.data()), h, "add_border_gaussians");
        } break;
      }
    }
  }
  // states from `first` on whose velocity is not a variable of the user's graph: pin a zero velocity (decoupled, zero error); compile
  void finish(int first) {
    for (int s = first; s < N; s++) {
      if (has_vel[s]) continue;
      std::vector<double> z(d, 0.0), one(d, 1.0);
      int32_t idx = s;
      check(gpslam_hip_add_vel_priors(h, 1, &idx, z.data(), one.data()), h, "add_vel_priors");
    }
    // more closures than one border of 28 right-hand sides holds: GTSAM would simply solve such a graph, so the column passes are
    // switched on here (gpslam_hip_set_closure_passes); graphs within one pass create their handle exactly as before
    if (closures > 0 && 1 + L * ld + closures * d > 28) check(gpslam_hip_set_closure_passes(h, 32, 0), h, "set_closure_passes");
    check(gpslam_hip_compile(h), h, "compile");
  }

  // copy the device state back into `values`
  void pull() {
    std::vector<double> P((size_t)N * pd), V((size_t)N * d), LM((size_t)L * (ld ? ld : 1));
    check(gpslam_hip_get_states(h, P.data(), V.data()), h, "get_states");
    if (L > 0) check(gpslam_hip_get_landmarks(h, LM.data()), h, "get_landmarks");
    scatter(values, P.data(), V.data(), LM.data());
  }
  // states (N x pd, N x d) and landmarks (L x ld) in the layouts of gpslam_hip_get_states / gpslam_hip_get_landmarks into the
  // variables of `out` (the keys of this session's Values)
  void scatter(Values &out, const double *P, const double *V, const double *LM) const {
    for (auto &kv : out.raw()) {
      const unsigned char c = symbolChr(kv.first);
      if (kv.second.type == T_POINT2 || kv.second.type == T_POINT3) {
        const int j = lm_of(kv.first);
        kv.second.d.assign(LM + (size_t)j * ld, LM + (size_t)(j + 1) * ld);
      } else if (c == 'v') {
        const int s = state_of(kv.first);
        kv.second.d.assign(V + (size_t)s * d, V + (size_t)s * d + ((vw || bias) ? 3 : d));
      } else if (bias && c == 'b' && kv.second.type == T_VEC3) {
        const int s = state_of(kv.first);
        kv.second.d.assign(P + (size_t)s * pd + 9, P + (size_t)(s + 1) * pd);
      } else if (vw && c == 'w') {
        const int s = state_of(kv.first);
        kv.second.d.assign(V + (size_t)s * d + 3, V + (size_t)(s + 1) * d);
      } else {
        const int s = state_of(kv.first);
        kv.second.d.assign(P + (size_t)s * pd, P + (size_t)s * pd + (bias ? 9 : pd));
      }
    }
  }
};
}  // namespace detail

inline double NonlinearFactorGraph::error(const Values &values) const {
  detail::Session s;
  s.build(*this, values);
  double e = 0.0;
  detail::check(gpslam_hip_error(s.h, &e), s.h, "error");
  return e;
}

class NonlinearOptimizer {
 public:
  const Values &values() { if (dirty_) { s_.pull(); dirty_ = false; } return s_.values; }
  double error() const { return error_; }
  int iterations() const { return iterations_; }
  const Values &optimize() {
    // NonlinearOptimizer::defaultOptimize: do { cur = error(); iterate(); } while (iters < max && !converged)
    if (error_ <= params_.errorTol) return values();
    for (;;) {
      const double cur = error_;
      iterate();
      if (iterations_ >= params_.maxIterations) break;
      if (error_ <= params_.errorTol) break;
      const double abs_dec = cur - error_, rel_dec = abs_dec / cur;
      if (rel_dec <= params_.relativeErrorTol || abs_dec <= params_.absoluteErrorTol) break;
      if (stop_) break;
    }
    return values();
  }
  virtual void iterate() = 0;
  virtual ~NonlinearOptimizer() {}
  /// Dense trajectory output: GaussianProcessInterpolator*::interpolatePose (gpslam.h:57-86) of the current estimate
  /// at time tau[q] after the state with pose key left[q] (interval length dt[q]), all queries in one launch.
  template <typename POSE> std::vector<POSE> interpolatePoses(const std::vector<Key> &left, const std::vector<double> &dt,
                                                              const std::vector<double> &tau) {
    if (left.size() != dt.size() || left.size() != tau.size()) throw std::invalid_argument("interpolatePoses: size mismatch");
    std::vector<int32_t> idx(left.size());
    for (size_t q = 0; q < left.size(); q++) idx[q] = s_.state_of(left[q]);
    std::vector<double> out(left.size() * (size_t)s_.pd);
    detail::check(gpslam_hip_interpolate_poses(s_.h, (int32_t)left.size(), idx.data(), dt.data(), tau.data(), out.data()), s_.h,
                  "interpolate_poses");
    std::vector<POSE> r;
    for (size_t q = 0; q < left.size(); q++)
      r.push_back(detail::VT<POSE>::un(std::vector<double>(out.begin() + q * s_.pd, out.begin() + (q + 1) * s_.pd)));
    return r;
  }
  /// the C-ABI handle behind this optimizer (no GTSAM counterpart: for gpslam_hip_plan_info and the other introspection calls)
  gpslam_hip_handle *handle() const { return s_.h; }
 protected:
  NonlinearOptimizer(const NonlinearFactorGraph &g, const Values &v, const NonlinearOptimizerParams &p) : params_(p) {
    s_.build(g, v);
    detail::check(gpslam_hip_error(s_.h, &error_), s_.h, "error");
  }
  detail::Session s_;
  NonlinearOptimizerParams params_;
  double error_ = 0.0;
  int iterations_ = 0;
  bool dirty_ = false, stop_ = false;
};

class GaussNewtonOptimizer : public NonlinearOptimizer {
 public:
  GaussNewtonOptimizer(const NonlinearFactorGraph &graph, const Values &initial, const GaussNewtonParams &params = GaussNewtonParams())
      : NonlinearOptimizer(graph, initial, params) {}
  void iterate() override {
    gpslam_hip_stats st;
    detail::check(gpslam_hip_iterate_gn(s_.h, &st), s_.h, "iterate_gn");
    error_ = st.error_after; iterations_++; dirty_ = true;
  }
};

class LevenbergMarquardtOptimizer : public NonlinearOptimizer {
 public:
  LevenbergMarquardtOptimizer(const NonlinearFactorGraph &graph, const Values &initial,
                              const LevenbergMarquardtParams &params = LevenbergMarquardtParams())
      : NonlinearOptimizer(graph, initial, params), lm_(params), lambda_(params.lambdaInitial) {}
  double lambda() const { return lambda_; }
  void iterate() override {
    gpslam_hip_params p;
    gpslam_hip_default_params(&p);
    p.use_lm = 1; p.lambda_factor = lm_.lambdaFactor; p.lambda_upper_bound = lm_.lambdaUpperBound;
    p.lambda_lower_bound = lm_.lambdaLowerBound; p.min_model_fidelity = lm_.minModelFidelity;
    p.relative_error_tol = lm_.relativeErrorTol;       // tryLambda's small-cost-change stop uses the optimiser's relativeErrorTol
    gpslam_hip_stats st;
    detail::check(gpslam_hip_iterate_lm(s_.h, &lambda_, &p, &st), s_.h, "iterate_lm");
    error_ = st.error_after; iterations_++; dirty_ = true; stop_ = !st.accepted;
  }
 private:
  LevenbergMarquardtParams lm_;
  double lambda_;
};

/// gtsam::DoglegOptimizer (Powell's dogleg; include/gpslam_hip_dogleg.h): one solve per iteration, every trial of a trust radius a
/// blend of the Gauss-Newton and the steepest-descent step.  fp64 unsharded handles without loop closures (the library refuses others)
class DoglegOptimizer : public NonlinearOptimizer {
 public:
  DoglegOptimizer(const NonlinearFactorGraph &graph, const Values &initial, const DoglegParams &params = DoglegParams())
      : NonlinearOptimizer(graph, initial, params), dl_(params), delta_(params.deltaInitial) {}
  double getDelta() const { return delta_; }
  /// the library's arguments for these parameters: (trust radius, mode)
  static std::pair<double, int32_t> abiArguments(const DoglegParams &p) { return {p.deltaInitial, (int32_t)p.adaptationMode}; }
  void iterate() override {
    gpslam_hip_stats st;
    detail::check(gpslam_hip_iterate_dogleg(s_.h, &delta_, abiArguments(dl_).second, &st), s_.h, "iterate_dogleg");
    error_ = st.error_after; iterations_++; dirty_ = true;
  }
 private:
  DoglegParams dl_;
  double delta_;
};

// ---------------------------------------------------------------- fixed-lag smoothing
/// gtsam::LinearContainerFactor (gtsam/nonlinear/LinearContainerFactor.h) over the two keys of one state: a Gaussian |A xi - b|^2 / 2
/// on xi = [Local(lin_x, x) ; v - lin_v], linearised with the constant Jacobian A as LinearContainerFactor::linearize does (exact at
/// the linearisation point, first order away from it).  A is 2d x 2d, b 2d; maps to gpslam_hip_add_state_gaussians.
class LinearContainerFactor : public NonlinearFactor {
 public:
  template <typename POSE, typename VEL>
  LinearContainerFactor(Key poseKey, Key velKey, const Matrix &A, const Vector &b, const POSE &lin_pose, const VEL &lin_vel) {
    if (A.rows != A.cols || (size_t)A.rows != b.size()) throw std::invalid_argument("LinearContainerFactor: A must be square and b of its size");
    d_.type = detail::F_STATE_GAUSS; d_.k[0] = poseKey; d_.k[1] = velKey;
    d_.meas = detail::VT<POSE>::pack(lin_pose);
    const std::vector<double> lv = detail::VT<VEL>::pack(lin_vel);
    d_.meas.insert(d_.meas.end(), lv.begin(), lv.end());
    d_.aux = A.a; d_.sig = b;
  }
  /// ... over (x, v, l_0 .. l_{L-1}): xi = [Local(lin_x, x) ; v - lin_v ; l - lin_l], A n x n, b n, n = 2d + the landmarks' coordinates.  The
  /// landmark keys are every landmark of the graph, in the order of their indices; maps to gpslam_hip_add_border_gaussians -- what
  /// BatchFixedLagSmoother leaves behind on a graph with landmarks.
  template <typename POSE, typename VEL, typename POINT>
  LinearContainerFactor(Key poseKey, Key velKey, const std::vector<Key> &landmarkKeys, const Matrix &A, const Vector &b, const POSE &lin_pose,
                        const VEL &lin_vel, const std::vector<POINT> &lin_landmarks) {
    if (A.rows != A.cols || (size_t)A.rows != b.size()) throw std::invalid_argument("LinearContainerFactor: A must be square and b of its size");
    if (landmarkKeys.size() != lin_landmarks.size()) throw std::invalid_argument("LinearContainerFactor: one linearisation point per landmark key");
    d_.type = detail::F_BORDER_GAUSS; d_.k[0] = poseKey; d_.k[1] = velKey; d_.lmk = landmarkKeys;
    d_.meas = detail::VT<POSE>::pack(lin_pose);
    const std::vector<double> lv = detail::VT<VEL>::pack(lin_vel);
    d_.meas.insert(d_.meas.end(), lv.begin(), lv.end());
    for (const POINT &pt : lin_landmarks) {
      const std::vector<double> lp = detail::VT<POINT>::pack(pt);
      d_.meas.insert(d_.meas.end(), lp.begin(), lp.end());
    }
    d_.aux = A.a; d_.sig = b;
  }
  size_t size() const override { return 2 + d_.lmk.size(); }
  NonlinearFactor::shared_ptr clone() const override { return std::make_shared<LinearContainerFactor>(*this); }
  detail::Desc describe() const override { return d_; }
  bool equals(const NonlinearFactor &expected, double tol = 1e-9) const override {
    const LinearContainerFactor *e = dynamic_cast<const LinearContainerFactor *>(&expected);
    return e != nullptr && detail::desc_equals(d_, e->d_, tol, false);
  }
  void print(const std::string &s = "", const KeyFormatter &kf = DefaultKeyFormatter) const override {
    std::cout << s << "LinearContainerFactor" << std::endl << "  keys = { " << kf(d_.k[0]) << " " << kf(d_.k[1]) << " }" << std::endl;
  }
 protected:
  detail::Desc d_;
};

/// gtsam::BatchFixedLagSmoother (gtsam_unstable/nonlinear/BatchFixedLagSmoother.h) on a chain: update() adds the new factors and
/// values, marginalises the leading states whose time stamp is older than (latest - lag) into a Gaussian on the oldest kept state
/// (gpslam_hip_marginalize_head: elimination at the current linearisation, as GTSAM's) -- on a graph with landmarks into a Gaussian on
/// that state and the landmarks where marginalizeOntoLandmarks() asked for it (gpslam_hip_marginalize_head_onto_landmarks) --, re-compiles and optimises with the
/// Levenberg-Marquardt parameters.  New states continue the chain: their pose keys carry larger indices than every key seen so far.
class BatchFixedLagSmoother {
 public:
  typedef std::map<Key, double> KeyTimestampMap;
  struct Result { int iterations = 0; double error = 0.0; int marginalized = 0; };
  explicit BatchFixedLagSmoother(double smootherLag = 0.0, const LevenbergMarquardtParams &params = LevenbergMarquardtParams())
      : lag_(smootherLag), params_(params) {}
  double smootherLag() const { return lag_; }
  /// On a graph with landmarks (range, bearing-range, projection factors) the head's prior must span the oldest kept state AND the
  /// landmarks, as GTSAM's does: gpslam_hip_marginalize_head_onto_landmarks.  Off by default, as in the C ABI: a smoother that was not
  /// asked keeps refusing a head factor that names a landmark, with the ABI's message.  Any time; a graph without landmarks is unaffected.
  void marginalizeOntoLandmarks(bool on = true) {
    onto_landmarks_ = on;
    if (s_) detail::check(gpslam_hip_marginalize_head_onto_landmarks(s_->h, on ? 1 : 0), s_->h, "marginalize_head_onto_landmarks");
  }
  const KeyTimestampMap &timestamps() const { return stamps_; }
  gpslam_hip_handle *handle() const { return s_ ? s_->h : nullptr; }

  Result update(const NonlinearFactorGraph &newFactors = NonlinearFactorGraph(), const Values &newTheta = Values(),
                const KeyTimestampMap &timestamps = KeyTimestampMap()) {
    for (auto &kv : timestamps) stamps_[kv.first] = kv.second;
    std::map<uint64_t, Key> pose_keys;                      // of the new values, in chain order
    for (auto &kv : newTheta.raw()) {
      const unsigned char c = symbolChr(kv.first);
      const bool point = kv.second.type == detail::T_POINT2 || kv.second.type == detail::T_POINT3;
      if (!point && c != 'v' && c != 'w' && c != 'b') pose_keys[symbolIndex(kv.first)] = kv.first;
    }
    if (!s_) {
      s_.reset(new detail::Session());
      s_->build(newFactors, newTheta);
      if (onto_landmarks_) detail::check(gpslam_hip_marginalize_head_onto_landmarks(s_->h, 1), s_->h, "marginalize_head_onto_landmarks");
    } else {
      extend(newFactors, newTheta, pose_keys);
    }
    for (auto &kv : pose_keys) keys_.push_back(kv.second);
    // the leading states that fell out of the lag
    Result r;
    double latest = -INFINITY;
    for (Key k : keys_) { auto it = stamps_.find(k); if (it != stamps_.end()) latest = std::max(latest, it->second); }
    auto old = [&](Key k) { auto it = stamps_.find(k); return it != stamps_.end() && it->second < latest - lag_; };
    int k = 0;
    while (k < (int)keys_.size() && old(keys_[k])) k++;
    for (size_t i = k; i < keys_.size(); i++)
      if (old(keys_[i])) throw std::invalid_argument("BatchFixedLagSmoother: key " + DefaultKeyFormatter(keys_[i]) + " is older than the lag but not at the head of the chain");
    k = std::min(k, (int)keys_.size() - 1);
    if (k >= 1) {
      detail::check(gpslam_hip_marginalize_head(s_->h, k), s_->h, "marginalize_head");
      for (int i = 0; i < k; i++) {
        const uint64_t idx = s_->state_index[i];
        for (auto it = s_->values.raw().begin(); it != s_->values.raw().end();) {
          const bool point = it->second.type == detail::T_POINT2 || it->second.type == detail::T_POINT3;
          if (!point && symbolIndex(it->first) == idx) { stamps_.erase(it->first); it = s_->values.raw().erase(it); } else ++it;
        }
      }
      s_->state_index.erase(s_->state_index.begin(), s_->state_index.begin() + k);
      s_->has_vel.erase(s_->has_vel.begin(), s_->has_vel.begin() + k);
      keys_.erase(keys_.begin(), keys_.begin() + k);
      s_->N -= k;
      detail::check(gpslam_hip_compile(s_->h), s_->h, "compile");
      r.marginalized = k;
    }
    gpslam_hip_params p;
    gpslam_hip_default_params(&p);
    p.use_lm = 1; p.max_iterations = params_.maxIterations; p.relative_error_tol = params_.relativeErrorTol;
    p.absolute_error_tol = params_.absoluteErrorTol; p.error_tol = params_.errorTol; p.lambda_initial = params_.lambdaInitial;
    p.lambda_factor = params_.lambdaFactor; p.lambda_upper_bound = params_.lambdaUpperBound; p.lambda_lower_bound = params_.lambdaLowerBound;
    p.min_model_fidelity = params_.minModelFidelity;
    gpslam_hip_stats st;
    detail::check(gpslam_hip_optimize(s_->h, &p, &st), s_->h, "optimize");
    r.iterations = st.iterations; r.error = st.error_after;
    return r;
  }
  /// the current estimate of every variable still in the window (and of the landmarks)
  Values calculateEstimate() {
    if (!s_) return Values();
    s_->pull();
    return s_->values;
  }

 private:
  void extend(const NonlinearFactorGraph &newFactors, const Values &newTheta, const std::map<uint64_t, Key> &pose_keys) {
    detail::Session &s = *s_;
    if (s.vw || s.bias) throw std::invalid_argument("BatchFixedLagSmoother: Pose3VW and AHRS graphs cannot be extended");
    const int n = (int)pose_keys.size(), first = s.N;
    std::vector<double> P((size_t)n * s.pd), V((size_t)n * s.d, 0.0);
    int i = 0;
    for (auto &kv : pose_keys) {
      if (kv.first <= s.state_index.back()) throw std::invalid_argument("BatchFixedLagSmoother: new states must continue the chain (larger key indices)");
      const detail::Value &val = newTheta.raw().at(kv.second);
      if (detail::Session::manifold_of(val.type) != s.manifold) throw std::invalid_argument("mixed pose types");
      std::memcpy(&P[(size_t)i * s.pd], val.d.data(), sizeof(double) * s.pd);
      const auto vi = newTheta.raw().find(Symbol('v', kv.first));
      const bool hv = vi != newTheta.raw().end();
      if (hv) {
        if ((int)vi->second.d.size() != s.d) throw std::invalid_argument("velocity dimension does not match the pose manifold");
        std::memcpy(&V[(size_t)i * s.d], vi->second.d.data(), sizeof(double) * s.d);
      }
      s.state_index.push_back(kv.first);
      s.has_vel.push_back(hv);
      i++;
    }
    for (auto &kv : newTheta.raw()) {
      if (kv.second.type == detail::T_POINT2 || kv.second.type == detail::T_POINT3) throw std::invalid_argument("BatchFixedLagSmoother: landmarks arrive with the first update");
      if (s.values.exists(kv.first)) throw std::invalid_argument("BatchFixedLagSmoother: key already exists");
      s.values.raw()[kv.first] = kv.second;
    }
    if (n > 0) detail::check(gpslam_hip_append_states(s.h, n, P.data(), V.data()), s.h, "append_states");
    s.N += n;
    s.add_factors(newFactors);
    s.finish(first);
  }
  double lag_;
  LevenbergMarquardtParams params_;
  bool onto_landmarks_ = false;
  std::unique_ptr<detail::Session> s_;
  std::vector<Key> keys_;          // pose keys of the states in the window, in chain order
  KeyTimestampMap stamps_;
};

// ---------------------------------------------------------------- gtsam::Marginals (gtsam/nonlinear/Marginals.h, GTSAM 4.0)
typedef std::vector<Key> KeyVector;

/// gtsam::JointMarginal: the joint covariance of a key set, block (k1, k2) or the whole matrix in the order of the keys given
class JointMarginal {
 public:
  Matrix operator()(Key k1, Key k2) const {
    const size_t i = at(k1), j = at(k2);
    Matrix m(dim_[i], dim_[j]);
    for (int r = 0; r < dim_[i]; r++)
      for (int c = 0; c < dim_[j]; c++) m(r, c) = full_(off_[i] + r, off_[j] + c);
    return m;
  }
  const Matrix &fullMatrix() const { return full_; }
 private:
  friend class Marginals;
  size_t at(Key k) const {
    for (size_t i = 0; i < keys_.size(); i++) if (keys_[i] == k) return i;
    throw std::invalid_argument("JointMarginal: key not in this joint marginal");
  }
  KeyVector keys_;
  std::vector<int> off_, dim_;
  Matrix full_;
};

/// gtsam::Marginals(graph, values): the Gauss-Newton Hessian of the whole graph at `values`, inverted on the device
/// (gpslam_hip_marginals).  Served: single keys (x, v, w, b and landmark keys), joint sets whose state keys belong to one
/// state or to two adjacent states, with any landmarks; other sets throw std::invalid_argument unless serveAnyStates() was called
/// (then: any states; betweenChiSquared() gates a loop-closure candidate over the same covariances).  On a graph that takes the segmented
/// landmark path (more than 13 planar landmarks) the landmarks of a set must sit in the same or in neighbouring fat blocks, and next to
/// the segment of the set's states -- every landmark a state observes does; sets beyond that throw std::invalid_argument as well.
class Marginals {
 public:
  Marginals(const NonlinearFactorGraph &graph, const Values &values) {
    s_.build(graph, values);
    // (closures in column passes: who constructs Marginals has asked for the closures' columns to be kept at every state)
    detail::check(gpslam_hip_marginals_keep_closure_columns(s_.h, 1), s_.h, "marginals_keep_closure_columns");
    // (... and on the segmented landmark path, for G at every interior state: the landmark blocks are gathered from it)
    detail::check(gpslam_hip_marginals_on_segments(s_.h, 1), s_.h, "marginals_on_segments");
    detail::check(gpslam_hip_marginals(s_.h), s_.h, "marginals");
  }
  /// Marginals::marginalCovariance(variable)
  Matrix marginalCovariance(Key k) const { return jointMarginalCovariance(KeyVector{k}).fullMatrix(); }
  /// Marginals::marginalInformation(variable): the inverse of the marginal covariance
  Matrix marginalInformation(Key k) const { return inverse(marginalCovariance(k)); }
  /// Marginals::jointMarginalCovariance(variables)
  JointMarginal jointMarginalCovariance(const KeyVector &keys) const {
    if (keys.empty()) throw std::invalid_argument("jointMarginalCovariance: no keys");
    std::vector<Var> vars;
    int lo = -1, hi = -1;
    for (Key k : keys) {
      const Var v = var_of(k);
      if (v.state >= 0) { lo = lo < 0 ? v.state : std::min(lo, v.state); hi = std::max(hi, v.state); }
      vars.push_back(v);
    }
    if (lo >= 0 && hi - lo > 1 && any_states_) return joint_any_states(keys, vars);
    if (lo >= 0 && hi - lo > 1)
      throw std::invalid_argument("jointMarginalCovariance: the keys span non-adjacent states; only one state or two adjacent states (with any landmarks) are served");
    const int b = 2 * s_.d, ld = s_.ld, first = lo < 0 ? 0 : lo, count = lo < 0 ? 0 : hi - lo + 1;
    std::vector<double> S((size_t)std::max(count, 1) * b * b), Sn(S.size());
    detail::check(gpslam_hip_get_marginals(s_.h, first, count, count ? S.data() : nullptr, count ? Sn.data() : nullptr, nullptr, nullptr),
                  s_.h, "get_marginals");
    // the landmarks of the set, through the getters that gather on the device what they are asked for (the only ones a session on
    // the segmented landmark path has: S_lm and S_x_lm do not exist there): every pair of them, and each with every state of the set
    std::vector<int32_t> lms;
    for (const Var &v : vars)
      if (v.state < 0 && std::find(lms.begin(), lms.end(), v.off / ld) == lms.end()) lms.push_back(v.off / ld);
    const int nL = (int)lms.size();
    auto pos = [&](int lm) { return (int)(std::find(lms.begin(), lms.end(), lm) - lms.begin()); };
    std::vector<int32_t> pa, pb, xs, xl;
    for (int u = 0; u < nL; u++)
      for (int v = 0; v < nL; v++) { pa.push_back(lms[u]); pb.push_back(lms[v]); }
    for (int t = 0; t < count; t++)
      for (int v = 0; v < nL; v++) { xs.push_back(first + t); xl.push_back(lms[v]); }
    std::vector<double> LL(std::max<size_t>(pa.size() * ld * ld, 1)), XL(std::max<size_t>(xs.size() * b * ld, 1));
    served(gpslam_hip_get_landmark_pair_marginals(s_.h, (int32_t)pa.size(), pa.data(), pb.data(), LL.data()), "get_landmark_pair_marginals");
    served(gpslam_hip_get_state_landmark_marginals(s_.h, (int32_t)xs.size(), xs.data(), xl.data(), XL.data()), "get_state_landmark_marginals");
    // one coordinate of the set: (state - first) * b + c for a state, or -1 - c for landmark coordinate c
    auto cov = [&](int p, int q) -> double {
      if (p >= 0 && q >= 0) {
        const int sp = p / b, sq = q / b, cp = p % b, cq = q % b;
        if (sp == sq) return S[(size_t)sp * b * b + cp * b + cq];
        return sp < sq ? Sn[(size_t)sp * b * b + cp * b + cq] : Sn[(size_t)sq * b * b + cq * b + cp];
      }
      if (p < 0 && q < 0) {
        const int cp = -1 - p, cq = -1 - q;
        return LL[(((size_t)pos(cp / ld) * nL + pos(cq / ld)) * ld + cp % ld) * ld + cq % ld];
      }
      const int st = p >= 0 ? p : q, cl = -1 - (p >= 0 ? q : p);
      return XL[(((size_t)(st / b) * nL + pos(cl / ld)) * b + st % b) * ld + cl % ld];
    };
    JointMarginal jm;
    jm.keys_ = keys;
    std::vector<int> coord;
    for (const Var &v : vars) {
      jm.off_.push_back((int)coord.size());
      jm.dim_.push_back(v.dim);
      for (int c = 0; c < v.dim; c++) coord.push_back(v.state >= 0 ? (v.state - first) * b + v.off + c : -1 - (v.off + c));
    }
    const int n = (int)coord.size();
    jm.full_ = Matrix(n, n);
    for (int i = 0; i < n; i++)
      for (int j = 0; j < n; j++) jm.full_(i, j) = cov(coord[i], coord[j]);
    return jm;
  }
  /// Posterior covariance (d x d) of the GP-interpolated pose at tau[q] after the state with pose key left[q] (interval dt[q]):
  /// gpslam_hip_interpolate_covariances, the covariance half of NonlinearOptimizer::interpolatePoses
  std::vector<Matrix> interpolatePoseCovariances(const KeyVector &left, const std::vector<double> &dt, const std::vector<double> &tau) const {
    if (left.size() != dt.size() || left.size() != tau.size()) throw std::invalid_argument("interpolatePoseCovariances: size mismatch");
    std::vector<int32_t> idx(left.size());
    for (size_t q = 0; q < left.size(); q++) idx[q] = s_.state_of(left[q]);
    const int d = s_.d;
    std::vector<double> out(left.size() * (size_t)d * d);
    detail::check(gpslam_hip_interpolate_covariances(s_.h, (int32_t)left.size(), idx.data(), dt.data(), tau.data(), 1, out.data()), s_.h,
                  "interpolate_covariances");
    std::vector<Matrix> r;
    for (size_t q = 0; q < left.size(); q++) {
      Matrix m(d, d);
      std::copy(out.begin() + q * d * d, out.begin() + (q + 1) * d * d, m.a.begin());
      r.push_back(m);
    }
    return r;
  }
  /// Opt-in: serve joint sets over ANY states (gtsam::Marginals does; here the default throws beyond two adjacent states).  Keeps
  /// one more device buffer (gpslam_hip_marginals_keep_pair_terms) and recomputes the marginals; afterwards a set's state blocks come
  /// from gpslam_hip_get_state_pair_marginals.  Dense-border and landmark-free sessions; a session on the segmented landmark path
  /// throws std::invalid_argument.
  void serveAnyStates() {
    int32_t plan[8] = {0};
    detail::check(gpslam_hip_segment_plan(s_.h, plan), s_.h, "segment_plan");
    if (plan[0]) throw std::invalid_argument("serveAnyStates: joint marginals over any states are not served on the segmented landmark path");
    detail::check(gpslam_hip_marginals_keep_pair_terms(s_.h, 1), s_.h, "marginals_keep_pair_terms");
    detail::check(gpslam_hip_marginals(s_.h), s_.h, "marginals");
    any_states_ = true;
  }
  /// The chi-square gate of a loop-closure candidate BetweenFactor<Pose>(a, b, measured, Diagonal::Sigmas(sigmas)) that is not in
  /// the graph: e^T (R + [H1 H2] Sigma [H1 H2]^T)^-1 e at the values and the marginals held (gpslam_hip_gate_between_pairs).
  /// Needs serveAnyStates() on a graph with landmarks or loop closures.
  template <typename Pose> double betweenChiSquared(Key a, Key b, const Pose &measured, const Vector &sigmas) const {
    if (s_.bias) throw std::invalid_argument("betweenChiSquared: not served on AHRS graphs (rotation and bias states)");
    if ((int)sigmas.size() != s_.d) throw std::invalid_argument("betweenChiSquared: sigmas must have the pose's tangent dimension");
    const int32_t s1 = s_.state_of(a), s2 = s_.state_of(b);
    const std::vector<double> m = detail::VT<Pose>::pack(measured);
    double chi2 = 0.0;
    const int rc = gpslam_hip_gate_between_pairs(s_.h, 1, &s1, &s2, m.data(), sigmas.data(), &chi2, nullptr, nullptr);
    if (rc == GPSLAM_E_INVALID) throw std::invalid_argument(std::string("betweenChiSquared: ") + gpslam_hip_last_error(s_.h));
    detail::check(rc, s_.h, "gate_between_pairs");
    return chi2;
  }
  /// the C-ABI handle behind these marginals
  gpslam_hip_handle *handle() const { return s_.h; }

 private:
  struct Var { int state, off, dim; };   // state -1: landmark coordinates off .. off + dim
  // serveAnyStates(): a set over any states, every state pair from one gpslam_hip_get_state_pair_marginals call, the landmarks from
  // the getters the default path uses
  JointMarginal joint_any_states(const KeyVector &keys, const std::vector<Var> &vars) const {
    const int b = 2 * s_.d, ld = s_.ld;
    std::vector<int32_t> sts, lms;
    for (const Var &v : vars) {
      if (v.state >= 0 && std::find(sts.begin(), sts.end(), v.state) == sts.end()) sts.push_back(v.state);
      if (v.state < 0 && std::find(lms.begin(), lms.end(), v.off / ld) == lms.end()) lms.push_back(v.off / ld);
    }
    const int nS = (int)sts.size(), nL = (int)lms.size();
    auto spos = [&](int st) { return (int)(std::find(sts.begin(), sts.end(), st) - sts.begin()); };
    auto lpos = [&](int lm) { return (int)(std::find(lms.begin(), lms.end(), lm) - lms.begin()); };
    std::vector<int32_t> sa, sb, pa, pb, xs, xl;
    for (int u = 0; u < nS; u++)
      for (int v = 0; v < nS; v++) { sa.push_back(sts[u]); sb.push_back(sts[v]); }
    for (int u = 0; u < nL; u++)
      for (int v = 0; v < nL; v++) { pa.push_back(lms[u]); pb.push_back(lms[v]); }
    for (int u = 0; u < nS; u++)
      for (int v = 0; v < nL; v++) { xs.push_back(sts[u]); xl.push_back(lms[v]); }
    std::vector<double> SS(std::max<size_t>(sa.size() * b * b, 1)), LL(std::max<size_t>(pa.size() * ld * ld, 1)), XL(std::max<size_t>(xs.size() * b * ld, 1));
    served(gpslam_hip_get_state_pair_marginals(s_.h, (int32_t)sa.size(), sa.data(), sb.data(), SS.data()), "get_state_pair_marginals");
    served(gpslam_hip_get_landmark_pair_marginals(s_.h, (int32_t)pa.size(), pa.data(), pb.data(), LL.data()), "get_landmark_pair_marginals");
    served(gpslam_hip_get_state_landmark_marginals(s_.h, (int32_t)xs.size(), xs.data(), xl.data(), XL.data()), "get_state_landmark_marginals");
    // one coordinate of the set: (position of its state) * b + c, or -1 - c for landmark coordinate c
    auto cov = [&](int p, int q) -> double {
      if (p >= 0 && q >= 0) return SS[(((size_t)(p / b) * nS + q / b) * b + p % b) * b + q % b];
      if (p < 0 && q < 0) {
        const int cp = -1 - p, cq = -1 - q;
        return LL[(((size_t)lpos(cp / ld) * nL + lpos(cq / ld)) * ld + cp % ld) * ld + cq % ld];
      }
      const int st = p >= 0 ? p : q, cl = -1 - (p >= 0 ? q : p);
      return XL[(((size_t)(st / b) * nL + lpos(cl / ld)) * b + st % b) * ld + cl % ld];
    };
    JointMarginal jm;
    jm.keys_ = keys;
    std::vector<int> coord;
    for (const Var &v : vars) {
      jm.off_.push_back((int)coord.size());
      jm.dim_.push_back(v.dim);
      for (int c = 0; c < v.dim; c++) coord.push_back(v.state >= 0 ? spos(v.state) * b + v.off + c : -1 - (v.off + c));
    }
    const int n = (int)coord.size();
    jm.full_ = Matrix(n, n);
    for (int i = 0; i < n; i++)
      for (int j = 0; j < n; j++) jm.full_(i, j) = cov(coord[i], coord[j]);
    return jm;
  }
  bool any_states_ = false;
  // a set the getters cannot serve (segmented sessions: landmarks beyond the neighbouring fat blocks) is the caller's error
  void served(int rc, const char *what) const {
    if (rc == GPSLAM_E_INVALID) throw std::invalid_argument(std::string("jointMarginalCovariance: ") + gpslam_hip_last_error(s_.h));
    detail::check(rc, s_.h, what);
  }
  Var var_of(Key k) const {
    auto it = s_.values.raw().find(k);
    if (it == s_.values.raw().end()) throw std::invalid_argument("Marginals: key not in the Values");
    const unsigned char c = symbolChr(k);
    const int d = s_.d;
    if (it->second.type == detail::T_POINT2 || it->second.type == detail::T_POINT3) return {-1, s_.lm_of(k) * s_.ld, s_.ld};
    if (c == 'v') return {s_.state_of(k), d, (s_.vw || s_.bias) ? 3 : d};
    if (s_.vw && c == 'w') return {s_.state_of(k), d + 3, 3};
    if (s_.bias && c == 'b') return {s_.state_of(k), 3, 3};
    return {s_.state_of(k), 0, s_.bias ? 3 : d};
  }
  static Matrix inverse(Matrix m) {   // Gauss-Jordan with partial pivoting
    const int n = m.rows;
    Matrix r = Matrix::Identity(n);
    for (int k = 0; k < n; k++) {
      int p = k;
      for (int i = k + 1; i < n; i++) if (std::fabs(m(i, k)) > std::fabs(m(p, k))) p = i;
      if (m(p, k) == 0.0) throw std::runtime_error("marginalInformation: singular marginal covariance");
      for (int j = 0; j < n; j++) { std::swap(m(k, j), m(p, j)); std::swap(r(k, j), r(p, j)); }
      const double piv = 1.0 / m(k, k);
      for (int j = 0; j < n; j++) { m(k, j) *= piv; r(k, j) *= piv; }
      for (int i = 0; i < n; i++) {
        if (i == k) continue;
        const double f = m(i, k);
        for (int j = 0; j < n; j++) { m(i, j) -= f * m(k, j); r(i, j) -= f * r(k, j); }
      }
    }
    return r;
  }
  detail::Session s_;
};

/// log det H of the whole graph at `values`, H = J^T J the Gauss-Newton Hessian Marginals inverts (gpslam_hip_log_determinant; include/
/// gpslam_hip_evidence.h), on a session of its own.  GTSAM's GaussianBayesNet::logDeterminant() of the eliminated linearised graph is
/// log det R with R^T R = H: HALF of this number.
inline double logDeterminant(const NonlinearFactorGraph &graph, const Values &values) {
  detail::Session s;
  s.build(graph, values);
  double out = 0.0;
  detail::check(gpslam_hip_log_determinant(s.h, &out, nullptr), s.h, "log_determinant");
  return out;
}

/// The Laplace log-evidence of the graph at `values` (the caller's optimum): log Z = -cost + sum_f log|det R_f| - 1/2 log det H -
/// ((m - n) / 2) log 2 pi (gpslam_hip_log_evidence), the number a hyperparameter such as Qc is chosen by.  Graphs with robust noise
/// models or AHRS factors have none: std::invalid_argument.
struct LogEvidence {
  double logZ = 0.0, cost = 0.0, logDeterminant = 0.0, logNoiseNormaliser = 0.0;
  long long rowsMinusVariables = 0;
};
inline LogEvidence logEvidence(const NonlinearFactorGraph &graph, const Values &values) {
  detail::Session s;
  s.build(graph, values);
  double out5[5] = {0, 0, 0, 0, 0};
  detail::check(gpslam_hip_log_evidence(s.h, out5), s.h, "log_evidence");
  LogEvidence e;
  e.logZ = out5[0]; e.cost = out5[1]; e.logDeterminant = out5[2]; e.logNoiseNormaliser = out5[3]; e.rowsMinusVariables = (long long)out5[4];
  return e;
}

/// The statistic Qc is learned from (gpslam_hip_qc_statistic; include/gpslam_hip_qc.h), at `values` (the caller's optimum), on a session
/// of its own: A = sum over the GP priors whose Qc_model is the first one the graph names of e~ e~^T + J~ Sigma_J J~^T, and their
/// number.  GP priors with another Qc_model are constants: neither summed nor counted.  gradient(Qc) is the derivative of the
/// log-evidence in Qc^-1 at fixed states, emUpdate() the Qc that makes it zero, emScale(Qc0) the stationary theta of theta Qc0.
struct QcStatistic {
  Matrix A;
  long long priors = 0;
  Matrix gradient(const Matrix &Qc) const {
    Matrix G(A.rows, A.cols);
    if (Qc.rows != A.rows || Qc.cols != A.cols || gpslam_hip_qc_gradient(A.rows, Qc.a.data(), A.a.data(), priors, G.a.data()))
      throw std::invalid_argument("QcStatistic::gradient: Qc must be symmetric positive definite, of the statistic's size, and the statistic must count a prior");
    return G;
  }
  Matrix emUpdate() const {
    Matrix Q(A.rows, A.cols);
    if (gpslam_hip_qc_em_update(A.rows, A.a.data(), priors, Q.a.data())) throw std::invalid_argument("QcStatistic::emUpdate: the statistic counts no prior, or A is not positive definite");
    return Q;
  }
  double emScale(const Matrix &Qc0) const {
    double theta = 0.0;
    if (Qc0.rows != A.rows || Qc0.cols != A.cols || gpslam_hip_qc_em_scale(A.rows, Qc0.a.data(), A.a.data(), priors, &theta))
      throw std::invalid_argument("QcStatistic::emScale: Qc0 must be symmetric positive definite, of the statistic's size, and the statistic must count a prior");
    return theta;
  }
};
inline QcStatistic qcStatistic(const NonlinearFactorGraph &graph, const Values &values) {
  detail::Session s;
  s.share_qc = true;
  s.build(graph, values);
  // (as Marginals: the closures' columns kept in column passes, G kept on the segmented landmark path)
  detail::check(gpslam_hip_marginals_keep_closure_columns(s.h, 1), s.h, "marginals_keep_closure_columns");
  detail::check(gpslam_hip_marginals_on_segments(s.h, 1), s.h, "marginals_on_segments");
  detail::check(gpslam_hip_marginals(s.h), s.h, "marginals");
  QcStatistic q;
  q.A = Matrix(s.d, s.d);
  int64_t n = 0;
  detail::check(gpslam_hip_qc_statistic(s.h, q.A.a.data(), &n), s.h, "qc_statistic");
  q.priors = (long long)n;
  return q;
}

/// The statistic the measurement noise of one kind of factor is learned from (gpslam_hip_meas_noise_statistic;
/// include/gpslam_hip_noise.h), at `values` (the caller's optimum), on a session of its own: over the graph's factors of `kind`
/// (GPSLAM_MEAS_*), B = sum (e e^T + J Sigma J^T), Bw the same between each factor's base whitening R and R^T, and their number.
/// gradient(C) is the derivative of the log-evidence in C^-1 at fixed states when the factors share the covariance C, emUpdate() the
/// C that makes it zero, emScale() the stationary theta+ / theta of C_m = theta C_m^0 (rows: one ratio per row of diagonal models).
struct MeasNoiseStatistic {
  Matrix B, Bw;
  long long factors = 0;
  Matrix gradient(const Matrix &C) const {
    Matrix G(B.rows, B.cols);
    if (C.rows != B.rows || C.cols != B.cols || gpslam_hip_noise_gradient(B.rows, C.a.data(), B.a.data(), factors, G.a.data()))
      throw std::invalid_argument("MeasNoiseStatistic::gradient: C must be symmetric positive definite, of the statistic's size, and the statistic must count a factor");
    return G;
  }
  Matrix emUpdate() const {
    Matrix C(B.rows, B.cols);
    if (gpslam_hip_noise_em_update(B.rows, B.a.data(), factors, C.a.data())) throw std::invalid_argument("MeasNoiseStatistic::emUpdate: the statistic counts no factor, or B is not positive definite");
    return C;
  }
  double emScale(std::vector<double> *rows = nullptr) const {
    double ratio = 0.0;
    if (rows) rows->assign((size_t)Bw.rows, 0.0);
    if (gpslam_hip_noise_em_scale(Bw.rows, Bw.a.data(), factors, &ratio, rows ? rows->data() : nullptr))
      throw std::invalid_argument("MeasNoiseStatistic::emScale: the statistic counts no factor, or Bw is not positive definite");
    return ratio;
  }
};
inline MeasNoiseStatistic measNoiseStatistic(const NonlinearFactorGraph &graph, const Values &values, int kind) {
  static const int rows_of[8] = {1, 1, 2, 3, 3, 2, 2, 3};
  if (kind < 0 || kind >= 8) throw std::invalid_argument("measNoiseStatistic: kind must be one of GPSLAM_MEAS_*");
  detail::Session s;
  s.build(graph, values);
  // (as qcStatistic: the closures' columns kept in column passes, G kept on the segmented landmark path)
  detail::check(gpslam_hip_marginals_keep_closure_columns(s.h, 1), s.h, "marginals_keep_closure_columns");
  detail::check(gpslam_hip_marginals_on_segments(s.h, 1), s.h, "marginals_on_segments");
  detail::check(gpslam_hip_marginals(s.h), s.h, "marginals");
  MeasNoiseStatistic q;
  q.B = Matrix(rows_of[kind], rows_of[kind]);
  q.Bw = Matrix(rows_of[kind], rows_of[kind]);
  int64_t n = 0;
  detail::check(gpslam_hip_meas_noise_statistic(s.h, kind, nullptr, q.B.a.data(), q.Bw.a.data(), &n), s.h, "meas_noise_statistic");
  q.factors = (long long)n;
  return q;
}

/// `count` draws from the Laplace posterior N(values, H^-1) of the graph at `values` (the caller's optimum), H = J^T J the matrix
/// Marginals inverts (gpslam_hip_sample_posterior; include/gpslam_hip_sampling.h), on a session of its own: each draw a Values with
/// the keys of `values` -- whole trajectories, landmarks included, from the JOINT over all variables.  Draw k depends on (seed,
/// first + k) alone, so a run can be extended or cut into batches.  A velocity that is no variable of the graph is pinned by a
/// unit prior (as every optimiser here does) and returns as it was given.  Graphs with loop closures or LinearContainerFactors:
/// std::invalid_argument.
inline std::vector<Values> samplePosterior(const NonlinearFactorGraph &graph, const Values &values, int count, uint64_t seed = 0, uint64_t first = 0) {
  if (count <= 0) throw std::invalid_argument("samplePosterior: count must be positive");
  detail::Session s;
  s.build(graph, values);
  const size_t wp = (size_t)s.N * s.pd, wv = (size_t)s.N * s.d, wl = (size_t)s.L * s.ld;
  std::vector<double> P(count * wp), V(count * wv), LM(std::max<size_t>(count * wl, 1));
  detail::check(gpslam_hip_sample_posterior(s.h, count, seed, first, nullptr, nullptr, P.data(), V.data(), wl ? LM.data() : nullptr), s.h, "sample_posterior");
  std::vector<Values> out((size_t)count, s.values);
  for (int k = 0; k < count; k++) s.scatter(out[k], P.data() + k * wp, V.data() + k * wv, LM.data() + k * wl);
  return out;
}

/// The same draws in continuous time (gpslam_hip_sample_posterior_at; include/gpslam_hip_sampling_at.h): per draw the support
/// states as samplePosterior returns them AND the pose at time tau[q] after the state with pose key left[q] (interval length dt[q]),
/// conditioned on that draw's own support states, with the GP's conditional noise and the correlation of the queries that share an
/// interval.  Queries are ordered along the chain; within an interval dt is one number and 0 < tau < dt increases strictly.  The
/// bridge's noise is the Qc_model the graph's GP priors share: a graph whose GP priors differ in Qc_model, GPSLAM_ROT3_BIAS chains and
/// world-frame velocities are refused (std::invalid_argument).
template <typename POSE> struct PosteriorDrawsAt {
  std::vector<Values> support;               // count draws, the keys of `values`
  std::vector<std::vector<POSE>> queries;    // count x the queries
};
template <typename POSE>
inline PosteriorDrawsAt<POSE> samplePosteriorAt(const NonlinearFactorGraph &graph, const Values &values, const std::vector<Key> &left,
                                                const std::vector<double> &dt, const std::vector<double> &tau, int count, uint64_t seed = 0,
                                                uint64_t first = 0) {
  if (count <= 0) throw std::invalid_argument("samplePosteriorAt: count must be positive");
  if (left.empty() || left.size() != dt.size() || left.size() != tau.size()) throw std::invalid_argument("samplePosteriorAt: size mismatch");
  detail::Session s;
  s.share_qc = true;          // (GP priors of the graph's first Qc_model use the handle's Qc: the one the bridge draws with)
  s.build(graph, values);
  const size_t nq = left.size();
  std::vector<int32_t> idx(nq);
  for (size_t q = 0; q < nq; q++) idx[q] = s.state_of(left[q]);
  const size_t wp = (size_t)s.N * s.pd, wv = (size_t)s.N * s.d, wl = (size_t)s.L * s.ld, wq = nq * (size_t)s.pd;
  std::vector<double> P(count * wp), V(count * wv), LM(std::max<size_t>(count * wl, 1)), Q(count * wq);
  detail::check(gpslam_hip_sample_posterior_at(s.h, count, seed, first, nullptr, (int32_t)nq, idx.data(), dt.data(), tau.data(), Q.data(), nullptr,
                                               nullptr, P.data(), V.data(), wl ? LM.data() : nullptr), s.h, "sample_posterior_at");
  PosteriorDrawsAt<POSE> out;
  out.support.assign((size_t)count, s.values);
  out.queries.resize((size_t)count);
  for (int k = 0; k < count; k++) {
    s.scatter(out.support[k], P.data() + k * wp, V.data() + k * wv, LM.data() + k * wl);
    for (size_t q = 0; q < nq; q++) {
      const double *r = Q.data() + k * wq + q * s.pd;
      out.queries[k].push_back(detail::VT<POSE>::un(std::vector<double>(r, r + s.pd)));
    }
  }
  return out;
}

/// Statistics of those draws, reduced on the device (gpslam_hip_sample_posterior_stats; include/gpslam_hip_sampling_stats.h): no
/// draw comes to the host.  Per query the mean and covariance of the draws' local coordinates around the interpolated estimate (the
/// tangent Marginals::interpolatedCovariance speaks in) and the number of draws closer than `margin` to a spherical obstacle; per
/// draw the smallest clearance over the queries and the length of the polyline through the query positions.  obstacles: rows of
/// (centre, radius), the centre in 3-D for Pose3 and in the plane otherwise; may be empty.  Rot3 has no position: moments only.
struct PosteriorStats {
  int d = 0;
  long long draws = 0;
  std::vector<double> s1, s2;            // queries x d, queries x d (d + 1) / 2: the sums the moments come from
  std::vector<double> mean, cov;         // queries x d, queries x d x d (cov empty with fewer than two draws)
  std::vector<long long> hits;           // per query (empty without obstacles)
  std::vector<double> clearance, length; // per draw (clearance empty without obstacles, length empty on Rot3); the share of
                                         // clearance < 0 estimates the probability that the path collides
};
inline PosteriorStats samplePosteriorStats(const NonlinearFactorGraph &graph, const Values &values, const std::vector<Key> &left,
                                           const std::vector<double> &dt, const std::vector<double> &tau, int count,
                                           const std::vector<std::vector<double>> &obstacles = {}, double margin = 0.0, uint64_t seed = 0,
                                           uint64_t first = 0) {
  if (count <= 0) throw std::invalid_argument("samplePosteriorStats: count must be positive");
  if (left.empty() || left.size() != dt.size() || left.size() != tau.size()) throw std::invalid_argument("samplePosteriorStats: size mismatch");
  detail::Session s;
  s.share_qc = true;          // (as samplePosteriorAt)
  s.build(graph, values);
  const size_t nq = left.size(), d = (size_t)s.d, w = s.manifold == GPSLAM_POSE3 ? 3 : 2;
  std::vector<int32_t> idx(nq);
  for (size_t q = 0; q < nq; q++) idx[q] = s.state_of(left[q]);
  std::vector<double> obs;
  for (const auto &o : obstacles) {
    if (o.size() != w + 1) throw std::invalid_argument("samplePosteriorStats: an obstacle is a centre and a radius");
    obs.insert(obs.end(), o.begin(), o.end());
  }
  const bool position = s.manifold != GPSLAM_ROT3, obst = !obstacles.empty();
  PosteriorStats out;
  out.d = s.d;
  out.s1.assign(nq * d, 0.0);
  out.s2.assign(nq * (d * (d + 1) / 2), 0.0);
  std::vector<int64_t> hits(obst ? nq : 0);
  if (obst) out.clearance.assign((size_t)count, 0.0);
  if (position) out.length.assign((size_t)count, 0.0);
  int64_t n = 0;
  detail::check(gpslam_hip_sample_posterior_stats(s.h, count, seed, first, nullptr, (int32_t)nq, idx.data(), dt.data(), tau.data(),
                                                  (int32_t)obstacles.size(), obst ? obs.data() : nullptr, margin, 0, &n, out.s1.data(), out.s2.data(),
                                                  obst ? hits.data() : nullptr, obst ? out.clearance.data() : nullptr,
                                                  position ? out.length.data() : nullptr), s.h, "sample_posterior_stats");
  out.draws = (long long)n;
  out.hits.assign(hits.begin(), hits.end());
  out.mean.assign(nq * d, 0.0);
  if (n >= 2) out.cov.assign(nq * d * d, 0.0);
  if (gpslam_hip_posterior_moments(s.d, (int32_t)nq, n, out.s1.data(), out.s2.data(), out.mean.data(), n >= 2 ? out.cov.data() : nullptr) != 0)
    throw std::runtime_error("samplePosteriorStats: posterior_moments failed");
  return out;
}

// ---------------------------------------------------------------- AHRS (gtsam/navigation/AHRSFactor.h, GTSAM 4.0; third party)
/// gtsam::PreintegratedAhrsMeasurements(biasHat, measuredOmegaCovariance): the constructor matlab/GPAHRSexample.m:188 uses.
/// integrateMeasurement restates PreintegratedRotation::integrateMeasurement + the covariance propagation of AHRSFactor.cpp:
///   incrR = Expmap((omega - biasHat) dt), D = ExpmapDerivative(.);  deltaTij += dt;  deltaRij = deltaRij incrR;
///   delRdelBiasOmega = incrR^T delRdelBiasOmega - D dt;  preintMeasCov = incrR^T preintMeasCov incrR + gyroCov dt
class PreintegratedAhrsMeasurements {
 public:
  PreintegratedAhrsMeasurements(const Vector3 &biasHat, const Matrix &measuredOmegaCovariance) : bias_hat_(biasHat), gyro_cov_(measuredOmegaCovariance) {
    if (gyro_cov_.rows != 3 || gyro_cov_.cols != 3) throw std::invalid_argument("measuredOmegaCovariance must be 3 x 3");
    resetIntegration();
  }
  void resetIntegration() {
    std::memset(st_, 0, sizeof(st_));
    st_[0] = st_[4] = st_[8] = 1.0;
    dtij_ = 0.0;
  }
  void integrateMeasurement(const Vector3 &measuredOmega, double deltaT) {
    double th[3], incr[9], D[9];
    for (int i = 0; i < 3; i++) th[i] = (measuredOmega[i] - bias_hat_[i]) * deltaT;
    expmap(th, incr, D);
    dtij_ += deltaT;
    double t[9], u[9];
    mm(st_, incr, t, false);
    std::memcpy(st_, t, sizeof(t));                                   // deltaRij
    mm(incr, st_ + 9, t, true);
    for (int i = 0; i < 9; i++) st_[9 + i] = t[i] - D[i] * deltaT;     // delRdelBiasOmega
    mm(incr, st_ + 18, t, true);
    mm(t, incr, u, false);
    for (int i = 0; i < 9; i++) st_[18 + i] = u[i] + gyro_cov_.a[i] * deltaT;   // preintMeasCov
  }
  double deltaTij() const { return dtij_; }
  Rot3 deltaRij() const { Rot3 r; std::memcpy(r.R, st_, sizeof(r.R)); return r; }
  Matrix delRdelBiasOmega() const { return mat(st_ + 9); }
  Matrix preintMeasCov() const { return mat(st_ + 18); }
  const Vector3 &biasHat() const { return bias_hat_; }
  /// [deltaRij (9) | delRdelBiasOmega (9) | biasHat (3) | deltaTij | preintMeasCov (9)]: the arguments of gpslam_hip_add_ahrs
  std::vector<double> packed() const {
    std::vector<double> m(st_, st_ + 18);
    m.insert(m.end(), bias_hat_.begin(), bias_hat_.end());
    m.push_back(dtij_);
    m.insert(m.end(), st_ + 18, st_ + 27);
    return m;
  }
 private:
  static Matrix mat(const double *p) { Matrix m(3, 3); std::memcpy(m.a.data(), p, 9 * sizeof(double)); return m; }
  static void mm(const double *A, const double *B, double *C, bool transA) {
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        double s = 0.0;
        for (int k = 0; k < 3; k++) s += (transA ? A[3 * k + i] : A[3 * i + k]) * B[3 * k + j];
        C[3 * i + j] = s;
      }
  }
  /// Rot3::Expmap (Rodrigues) + SO3::ExpmapDerivative with GTSAM's theta^2 <= epsilon branches
  static void expmap(const double *w, double *R, double *J) {
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    const double W[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (th2 <= 2.220446049250313e-16) {
      for (int i = 0; i < 9; i++) { R[i] = I[i] + W[i]; J[i] = I[i]; }
      return;
    }
    const double th = std::sqrt(th2);
    double K[9], KK[9];
    for (int i = 0; i < 9; i++) K[i] = W[i] / th;
    mm(K, K, KK, false);
    const double sh = std::sin(th / 2.0), a = std::sin(th), b = 2.0 * sh * sh;
    for (int i = 0; i < 9; i++) {
      R[i] = I[i] + a * K[i] + b * KK[i];
      J[i] = I[i] - ((1.0 - std::cos(th)) / th) * K[i] + (1.0 - std::sin(th) / th) * KK[i];
    }
  }
  Vector3 bias_hat_;
  Matrix gyro_cov_;
  double st_[27];
  double dtij_ = 0.0;
};

/// gtsam::AHRSFactor(rot_i, rot_j, bias, preintegratedMeasurements, omegaCoriolis) -- matlab/GPAHRSexample.m:131-137.
/// Evaluated on the device (gpslam_hip_add_ahrs); the bias key must carry the index of rot_i (b_{k-1} with x_{k-1}).
class AHRSFactor : public NonlinearFactor {
 public:
  AHRSFactor(Key rot_i, Key rot_j, Key bias, const PreintegratedAhrsMeasurements &pim, const Vector3 &omegaCoriolis = Vector3()) {
    d_.type = detail::F_AHRS; d_.manifold = GPSLAM_ROT3_BIAS;
    d_.k[0] = rot_i; d_.k[2] = rot_j; d_.k[4] = bias;
    d_.meas = pim.packed();
    if (omegaCoriolis[0] != 0.0 || omegaCoriolis[1] != 0.0 || omegaCoriolis[2] != 0.0) d_.aux = {omegaCoriolis[0], omegaCoriolis[1], omegaCoriolis[2]};
  }
  GPSLAM_FACTOR_BOILERPLATE(AHRSFactor, 3)
};

/// gtsam::Rot3AttitudeFactor(key, nZ, model, bRef) -- matlab/GPAHRSexample.m:160-163
class Rot3AttitudeFactor : public NonlinearFactor {
 public:
  Rot3AttitudeFactor(Key key, const Unit3 &nZ, const SharedNoiseModel &model, const Unit3 &bRef = Unit3(0, 0, 1)) {
    d_.type = detail::F_ATTITUDE; d_.k[0] = key;
    d_.aux = {nZ.p[0], nZ.p[1], nZ.p[2], bRef.p[0], bRef.p[1], bRef.p[2]};
    noise_of(model, d_);
  }
  GPSLAM_FACTOR_BOILERPLATE(Rot3AttitudeFactor, 1)
};

}  // namespace gtsam

// =====================================================================================================
// gpslam factor classes: same names and constructor argument order as the reference headers / gpslam.h
// =====================================================================================================
namespace gpslam {

namespace detail_g {
inline gtsam::detail::Desc gp(int manifold, gtsam::Key p1, gtsam::Key v1, gtsam::Key p2, gtsam::Key v2, double dt,
                              const gtsam::SharedNoiseModel &Qc) {
  gtsam::detail::Desc d;
  d.type = gtsam::detail::F_GP; d.manifold = manifold; d.k[0] = p1; d.k[1] = v1; d.k[2] = p2; d.k[3] = v2; d.dt = dt;
  if (Qc && Qc->robust_) throw std::invalid_argument("noiseModel::Robust on a GP prior: the chain's own factors take no loss (measurement factors and loop closures do)");
  d.Qc = Qc->covariance();      // getQc(Qc_model), gpslam/gp/GPutils.cpp:16-20
  return d;
}

// ---- evaluateError / interpolatePose of ONE factor (what the reference's unit tests call, e.g.
// gpslam/gp/tests/testGaussianProcessPriorPose3.cpp:43-60).  There is no CPU implementation of the factor maths in this
// library: a two-state device session is built around the arguments and the batched kernels evaluate the single
// factor (gpslam_hip_linearize_gp / gpslam_hip_linearize_meas / gpslam_hip_interpolate_poses_jac).
struct Single {
  gpslam_hip_handle *h = nullptr;
  int d = 0, pd = 0, ld = 0;
  Single(int manifold, int landmark_dim, const std::vector<double> &p1, const std::vector<double> &v1, const std::vector<double> &p2,
         const std::vector<double> &v2, const gtsam::Matrix *Qc, const std::vector<double> *lm) {
    static const int dd[5] = {2, 3, 3, 6, 3}, pdd[5] = {2, 3, 3, 12, 9};
    d = dd[manifold]; pd = pdd[manifold]; ld = landmark_dim;
    if ((int)p1.size() != pd || (int)p2.size() != pd || (int)v1.size() != d || (int)v2.size() != d)
      throw std::invalid_argument("evaluateError: argument types do not match the factor's manifold");
    gpslam_hip_config_v2 cfg = gtsam::detail::make_config(manifold);
    cfg.landmark_dim = ld;
    if (gpslam_hip_create_v2(&cfg, &h) < 0) throw std::runtime_error("gpslam_hip_create_v2 failed: no usable HIP device (there is no CPU fallback)");
    std::vector<double> P(p1), V(v1);
    P.insert(P.end(), p2.begin(), p2.end());
    V.insert(V.end(), v2.begin(), v2.end());
    gtsam::detail::check(gpslam_hip_set_states(h, 2, P.data(), V.data()), h, "set_states");
    if (Qc) {
      if (Qc->rows != d) throw std::invalid_argument("Qc_model dimension does not match the manifold");
      gtsam::detail::check(gpslam_hip_set_qc(h, Qc->a.data()), h, "set_qc");
    }
    if (lm) gtsam::detail::check(gpslam_hip_set_landmarks(h, 1, lm->data()), h, "set_landmarks");
  }
  ~Single() { if (h) gpslam_hip_destroy(h); }
  Single(const Single &) = delete;
  Single &operator=(const Single &) = delete;
};
inline void fill(gtsam::Matrix *H, int rows, int cols, const double *src, int src_ld) {
  if (!H) return;
  *H = gtsam::Matrix(rows, cols);
  for (int r = 0; r < rows; r++)
    for (int c = 0; c < cols; c++) (*H)(r, c) = src[(size_t)r * src_ld + c];
}
// GaussianProcessPrior*::evaluateError: e (2d) and H1..H4 (2d x d each)
inline gtsam::Vector gp_evaluate(const gtsam::detail::Desc &f, const std::vector<double> &p1, const std::vector<double> &v1,
                                 const std::vector<double> &p2, const std::vector<double> &v2, gtsam::Matrix *H1, gtsam::Matrix *H2,
                                 gtsam::Matrix *H3, gtsam::Matrix *H4) {
  Single s(f.manifold, 0, p1, v1, p2, v2, &f.Qc, nullptr);
  const int32_t left = 0;
  gtsam::detail::check(gpslam_hip_add_gp_priors(s.h, 1, &left, &f.dt), s.h, "add_gp_priors");
  gtsam::detail::check(gpslam_hip_compile(s.h), s.h, "compile");
  const int d = s.d, b = 2 * d;
  gtsam::Vector e(b);
  std::vector<double> J((size_t)4 * b * d);
  gtsam::detail::check(gpslam_hip_linearize_gp(s.h, e.data(), J.data()), s.h, "linearize_gp");
  gtsam::Matrix *H[4] = {H1, H2, H3, H4};
  for (int m = 0; m < 4; m++) fill(H[m], b, d, J.data() + (size_t)m * b * d, d);
  return e;
}
// measurement factors: e (rows) and H1..H4 (rows x d), H5 (rows x landmark_dim)
inline gtsam::Vector meas_evaluate(const gtsam::detail::Desc &f, const std::vector<double> &p1, const std::vector<double> &v1,
                                   const std::vector<double> &p2, const std::vector<double> &v2, const std::vector<double> *lm,
                                   gtsam::Matrix *H1, gtsam::Matrix *H2, gtsam::Matrix *H3, gtsam::Matrix *H4, gtsam::Matrix *H5) {
  const int ld = lm ? (int)lm->size() : 0;
  Single s(f.manifold, ld, p1, v1, p2, v2, f.Qc.rows ? &f.Qc : nullptr, lm);
  const int32_t zero = 0;
  const double *sens = f.sensor.empty() ? nullptr : f.sensor.data();
  int kind = -1, rows = 1;
  switch (f.type) {
    case gtsam::detail::F_INTERP_RANGE:
      kind = GPSLAM_MEAS_INTERP_RANGE; rows = 1;
      gtsam::detail::check(gpslam_hip_add_interp_range(s.h, 1, &zero, &zero, f.meas.data(), f.sig.data(), &f.dt, &f.tau, sens), s.h, "add_interp_range");
      break;
    case gtsam::detail::F_RANGE:
      kind = GPSLAM_MEAS_RANGE; rows = 1;
      gtsam::detail::check(gpslam_hip_add_range(s.h, 1, &zero, &zero, f.meas.data(), f.sig.data()), s.h, "add_range");
      break;
    case gtsam::detail::F_INTERP_ATT:
      kind = GPSLAM_MEAS_INTERP_ATTITUDE; rows = 2;
      gtsam::detail::check(gpslam_hip_add_interp_attitude(s.h, 1, &zero, f.aux.data(), f.aux.data() + 3, f.sig.data(), &f.dt, &f.tau), s.h, "add_interp_attitude");
      break;
    case gtsam::detail::F_INTERP_GPS:
      kind = GPSLAM_MEAS_INTERP_GPS; rows = 3;
      gtsam::detail::check(gpslam_hip_add_interp_gps(s.h, 1, &zero, f.meas.data(), f.sig.data(), &f.dt, &f.tau, sens), s.h, "add_interp_gps");
      break;
    case gtsam::detail::F_ODOM2D:
      kind = GPSLAM_MEAS_ODOMETRY2D; rows = 3;
      gtsam::detail::check(gpslam_hip_add_odometry2d(s.h, 1, &zero, f.meas.data(), f.sig.data()), s.h, "add_odometry2d");
      break;
    case gtsam::detail::F_BEARING_RANGE:
      kind = GPSLAM_MEAS_BEARING_RANGE; rows = 2;
      gtsam::detail::check(gpslam_hip_add_bearing_range(s.h, 1, &zero, &zero, &f.meas[0], &f.meas[1], f.sig.data()), s.h, "add_bearing_range");
      break;
    case gtsam::detail::F_INTERP_PROJ:
      kind = GPSLAM_MEAS_INTERP_PROJECTION; rows = 2;
      gtsam::detail::check((f.aux.size() == 9 ? gpslam_hip_add_interp_projection_ds2 : gpslam_hip_add_interp_projection)(s.h, 1, &zero, &zero, f.meas.data(), f.sig.data(), &f.dt, &f.tau, f.aux.data(), sens), s.h, "add_interp_projection");
      break;
    default: throw std::invalid_argument("evaluateError: not a measurement factor");
  }
  gtsam::detail::check(gpslam_hip_compile(s.h), s.h, "compile");
  const int d = s.d, W = 4 * d + 3;
  gtsam::Vector e(rows);
  std::vector<double> J((size_t)rows * W);
  gtsam::detail::check(gpslam_hip_linearize_meas(s.h, kind, e.data(), J.data()), s.h, "linearize_meas");
  gtsam::Matrix *H[4] = {H1, H2, H3, H4};
  for (int m = 0; m < 4; m++) fill(H[m], rows, d, J.data() + (size_t)m * d, W);
  if (ld) fill(H5, rows, ld, J.data() + (size_t)4 * d, W);
  return e;
}
template <typename POSE, typename VEL>
inline POSE interpolate_one(int manifold, const gtsam::Matrix &Qc, double delta_t, double tau, const POSE &p1, const VEL &v1,
                            const POSE &p2, const VEL &v2, gtsam::Matrix *H1, gtsam::Matrix *H2, gtsam::Matrix *H3, gtsam::Matrix *H4) {
  Single s(manifold, 0, gtsam::detail::VT<POSE>::pack(p1), gtsam::detail::VT<VEL>::pack(v1), gtsam::detail::VT<POSE>::pack(p2),
           gtsam::detail::VT<VEL>::pack(v2), &Qc, nullptr);
  const int32_t left = 0;
  const int d = s.d;
  std::vector<double> out(s.pd), H((size_t)4 * d * d);
  gtsam::detail::check(gpslam_hip_interpolate_poses_jac(s.h, 1, &left, &delta_t, &tau, out.data(), H.data()), s.h, "interpolate_poses_jac");
  gtsam::Matrix *Hs[4] = {H1, H2, H3, H4};
  for (int m = 0; m < 4; m++) fill(Hs[m], d, d, H.data() + (size_t)m * d * d, d);
  return gtsam::detail::VT<POSE>::un(out);
}
}  // namespace detail_g

#define GPSLAM_GP_PRIOR(CLS, MANIFOLD, POSE, VEL, NAME)                                                                          \
  class CLS : public gtsam::NonlinearFactor {                                                                   \
   public:                                                                                                      \
    CLS(gtsam::Key poseKey1, gtsam::Key velKey1, gtsam::Key poseKey2, gtsam::Key velKey2, double delta_t,      \
        const gtsam::SharedNoiseModel &Qc_model) { d_ = detail_g::gp(MANIFOLD, poseKey1, velKey1, poseKey2, velKey2, delta_t, Qc_model); } \
    /** evaluateError(pose1, vel1, pose2, vel2, H1..H4): the reference's signature with pointers for boost::optional */ \
    gtsam::Vector evaluateError(const POSE &pose1, const VEL &vel1, const POSE &pose2, const VEL &vel2, gtsam::OptionalMatrix H1 = boost::none, \
                                gtsam::OptionalMatrix H2 = boost::none, gtsam::OptionalMatrix H3 = boost::none, gtsam::OptionalMatrix H4 = boost::none) const { \
      return detail_g::gp_evaluate(d_, gtsam::detail::VT<POSE>::pack(pose1), gtsam::detail::VT<VEL>::pack(vel1),      \
                                   gtsam::detail::VT<POSE>::pack(pose2), gtsam::detail::VT<VEL>::pack(vel2), H1, H2, H3, H4); \
    }                                                                                                           \
    GPSLAM_FACTOR_BOILERPLATE_NAMED(CLS, 4, NAME, true)                                                         \
  };
/// gpslam/gp/GaussianProcessPriorPose3.h:43-49
GPSLAM_GP_PRIOR(GaussianProcessPriorPose3, GPSLAM_POSE3, gtsam::Pose3, gtsam::Vector6, "4-way Gaussian Process Factor Pose3")
/// gpslam/gp/GaussianProcessPriorPose2.h:41-47
GPSLAM_GP_PRIOR(GaussianProcessPriorPose2, GPSLAM_POSE2, gtsam::Pose2, gtsam::Vector3, "4-way Gaussian Process Factor Pose2")
/// gpslam/gp/GaussianProcessPriorRot3.h:41-47
GPSLAM_GP_PRIOR(GaussianProcessPriorRot3, GPSLAM_ROT3, gtsam::Rot3, gtsam::Vector3, "4-way Gaussian Process Factor Rot3")

/// gpslam/gp/GaussianProcessPriorLinear.h:47-53 (Dim = 2 or 3, gpslam.h:177-181)
template <int Dim> class GaussianProcessPriorLinear : public gtsam::NonlinearFactor {
 public:
  GaussianProcessPriorLinear(gtsam::Key poseKey1, gtsam::Key velKey1, gtsam::Key poseKey2, gtsam::Key velKey2, double delta_t,
                             const gtsam::SharedNoiseModel &Qc_model) {
    static_assert(Dim == 2 || Dim == 3, "GaussianProcessPriorLinear<DOF = {2, 3}>");
    d_ = detail_g::gp(Dim == 2 ? GPSLAM_LINEAR2 : GPSLAM_LINEAR3, poseKey1, velKey1, poseKey2, velKey2, delta_t, Qc_model);
  }
  /// gpslam/gp/GaussianProcessPriorLinear.h:63-83
  gtsam::Vector evaluateError(const gtsam::VectorN<Dim> &pose1, const gtsam::VectorN<Dim> &vel1, const gtsam::VectorN<Dim> &pose2,
                              const gtsam::VectorN<Dim> &vel2, gtsam::OptionalMatrix H1 = boost::none, gtsam::OptionalMatrix H2 = boost::none,
                              gtsam::OptionalMatrix H3 = boost::none, gtsam::OptionalMatrix H4 = boost::none) const {
    typedef gtsam::detail::VT<gtsam::VectorN<Dim>> P;
    return detail_g::gp_evaluate(d_, P::pack(pose1), P::pack(vel1), P::pack(pose2), P::pack(vel2), H1, H2, H3, H4);
  }
  GPSLAM_FACTOR_BOILERPLATE_NAMED(GaussianProcessPriorLinear<Dim>, 4, (Dim == 2 ? "4-way Gaussian Process Factor Linear<2>" : "4-way Gaussian Process Factor Linear<3>"), true)
};

/// gpslam/slam/GPInterpolatedRangeFactorPose2.h:46-54
class GPInterpolatedRangeFactorPose2 : public gtsam::NonlinearFactor {
 public:
  GPInterpolatedRangeFactorPose2(double measured, const gtsam::SharedNoiseModel &meas_model, const gtsam::SharedNoiseModel &Qc_model,
                                 gtsam::Key poseKey1, gtsam::Key velKey1, gtsam::Key poseKey2, gtsam::Key velKey2, gtsam::Key pointKey,
                                 double delta_t, double tau, const gtsam::Pose2 *body_P_sensor = nullptr) {
    d_.type = gtsam::detail::F_INTERP_RANGE; d_.manifold = GPSLAM_POSE2;
    d_.k[0] = poseKey1; d_.k[1] = velKey1; d_.k[2] = poseKey2; d_.k[3] = velKey2; d_.k[4] = pointKey;
    d_.meas = {measured}; gtsam::noise_of(meas_model, d_); d_.Qc = Qc_model->covariance(); d_.dt = delta_t; d_.tau = tau;
    if (body_P_sensor) d_.sensor = {body_P_sensor->x, body_P_sensor->y, body_P_sensor->theta};
  }
  /// gpslam/slam/GPInterpolatedRangeFactorPose2.h:64-98
  gtsam::Vector evaluateError(const gtsam::Pose2 &pose1, const gtsam::Vector3 &vel1, const gtsam::Pose2 &pose2, const gtsam::Vector3 &vel2, const gtsam::Point2 &point,
                              gtsam::OptionalMatrix H1 = boost::none, gtsam::OptionalMatrix H2 = boost::none, gtsam::OptionalMatrix H3 = boost::none, gtsam::OptionalMatrix H4 = boost::none, gtsam::OptionalMatrix H5 = boost::none) const {
    const std::vector<double> lm = {point.x, point.y};
    return detail_g::meas_evaluate(d_, gtsam::detail::VT<gtsam::Pose2>::pack(pose1), gtsam::detail::VT<gtsam::Vector3>::pack(vel1), gtsam::detail::VT<gtsam::Pose2>::pack(pose2),
                                   gtsam::detail::VT<gtsam::Vector3>::pack(vel2), &lm, H1, H2, H3, H4, H5);
  }
  GPSLAM_FACTOR_BOILERPLATE_NAMED(GPInterpolatedRangeFactorPose2, 5, "RangeFactor (GP interpolated, Pose2)", true)
};

/// gpslam/slam/GPInterpolatedRangeFactorPose3.h:46-54
class GPInterpolatedRangeFactorPose3 : public gtsam::NonlinearFactor {
 public:
  GPInterpolatedRangeFactorPose3(double measured, const gtsam::SharedNoiseModel &meas_model, const gtsam::SharedNoiseModel &Qc_model,
                                 gtsam::Key poseKey1, gtsam::Key velKey1, gtsam::Key poseKey2, gtsam::Key velKey2, gtsam::Key pointKey,
                                 double delta_t, double tau, const gtsam::Pose3 *body_P_sensor = nullptr) {
    d_.type = gtsam::detail::F_INTERP_RANGE; d_.manifold = GPSLAM_POSE3;
    d_.k[0] = poseKey1; d_.k[1] = velKey1; d_.k[2] = poseKey2; d_.k[3] = velKey2; d_.k[4] = pointKey;
    d_.meas = {measured}; gtsam::noise_of(meas_model, d_); d_.Qc = Qc_model->covariance(); d_.dt = delta_t; d_.tau = tau;
    if (body_P_sensor) d_.sensor = gtsam::detail::VT<gtsam::Pose3>::pack(*body_P_sensor);
  }
  /// gpslam/slam/GPInterpolatedRangeFactorPose3.h:64-98
  gtsam::Vector evaluateError(const gtsam::Pose3 &pose1, const gtsam::Vector6 &vel1, const gtsam::Pose3 &pose2, const gtsam::Vector6 &vel2, const gtsam::Point3 &point,
                              gtsam::OptionalMatrix H1 = boost::none, gtsam::OptionalMatrix H2 = boost::none, gtsam::OptionalMatrix H3 = boost::none, gtsam::OptionalMatrix H4 = boost::none, gtsam::OptionalMatrix H5 = boost::none) const {
    const std::vector<double> lm = {point.x, point.y, point.z};
    return detail_g::meas_evaluate(d_, gtsam::detail::VT<gtsam::Pose3>::pack(pose1), gtsam::detail::VT<gtsam::Vector6>::pack(vel1), gtsam::detail::VT<gtsam::Pose3>::pack(pose2),
                                   gtsam::detail::VT<gtsam::Vector6>::pack(vel2), &lm, H1, H2, H3, H4, H5);
  }
  GPSLAM_FACTOR_BOILERPLATE_NAMED(GPInterpolatedRangeFactorPose3, 5, "RangeFactor (GP interpolated, Pose3)", true)
};

/// gpslam/slam/GPInterpolatedRangeFactor2DLinear.h:42-50 -- NOTE: keys come before the noise models here
class GPInterpolatedRangeFactor2DLinear : public gtsam::NonlinearFactor {
 public:
  GPInterpolatedRangeFactor2DLinear(double measured, gtsam::Key pose1Key, gtsam::Key vel1Key, gtsam::Key pose2Key, gtsam::Key vel2Key,
                                    gtsam::Key pointKey, const gtsam::SharedNoiseModel &meas_model,
                                    const gtsam::SharedNoiseModel &Qc_model, double delta_t, double tau) {
    d_.type = gtsam::detail::F_INTERP_RANGE; d_.manifold = GPSLAM_LINEAR3;
    d_.k[0] = pose1Key; d_.k[1] = vel1Key; d_.k[2] = pose2Key; d_.k[3] = vel2Key; d_.k[4] = pointKey;
    d_.meas = {measured}; gtsam::noise_of(meas_model, d_); d_.Qc = Qc_model->covariance(); d_.dt = delta_t; d_.tau = tau;
  }
  /// gpslam/slam/GPInterpolatedRangeFactor2DLinear.h:60-88
  gtsam::Vector evaluateError(const gtsam::Vector3 &pose1, const gtsam::Vector3 &vel1, const gtsam::Vector3 &pose2, const gtsam::Vector3 &vel2, const gtsam::Point2 &point,
                              gtsam::OptionalMatrix H1 = boost::none, gtsam::OptionalMatrix H2 = boost::none, gtsam::OptionalMatrix H3 = boost::none, gtsam::OptionalMatrix H4 = boost::none, gtsam::OptionalMatrix H5 = boost::none) const {
    typedef gtsam::detail::VT<gtsam::Vector3> P;
    const std::vector<double> lm = {point.x, point.y};
    return detail_g::meas_evaluate(d_, P::pack(pose1), P::pack(vel1), P::pack(pose2), P::pack(vel2), &lm, H1, H2, H3, H4, H5);
  }
  GPSLAM_FACTOR_BOILERPLATE_NAMED(GPInterpolatedRangeFactor2DLinear, 5, "RangeFactor (GP interpolated, 2D linear)", false)
};

/// gpslam/slam/GPInterpolatedAttitudeFactorRot3.h:44-51
class GPInterpolatedAttitudeFactorRot3 : public gtsam::NonlinearFactor {
 public:
  GPInterpolatedAttitudeFactorRot3(gtsam::Key poseKey1, gtsam::Key velKey1, gtsam::Key poseKey2, gtsam::Key velKey2, double delta_t,
                                   double tau, const gtsam::SharedNoiseModel &Qc_model, const gtsam::SharedNoiseModel &meas_model,
                                   const gtsam::Unit3 &nZ, const gtsam::Unit3 &bRef = gtsam::Unit3(0, 0, 1)) {
    d_.type = gtsam::detail::F_INTERP_ATT; d_.manifold = GPSLAM_ROT3;
    d_.k[0] = poseKey1; d_.k[1] = velKey1; d_.k[2] = poseKey2; d_.k[3] = velKey2;
    d_.aux = {nZ.p[0], nZ.p[1], nZ.p[2], bRef.p[0], bRef.p[1], bRef.p[2]};
    gtsam::noise_of(meas_model, d_); d_.Qc = Qc_model->covariance(); d_.dt = delta_t; d_.tau = tau;
  }
  /// gpslam/slam/GPInterpolatedAttitudeFactorRot3.h:61-83
  gtsam::Vector evaluateError(const gtsam::Rot3 &pose1, const gtsam::Vector3 &vel1, const gtsam::Rot3 &pose2, const gtsam::Vector3 &vel2,
                              gtsam::OptionalMatrix H1 = boost::none, gtsam::OptionalMatrix H2 = boost::none, gtsam::OptionalMatrix H3 = boost::none, gtsam::OptionalMatrix H4 = boost::none) const {
    return detail_g::meas_evaluate(d_, gtsam::detail::VT<gtsam::Rot3>::pack(pose1), gtsam::detail::VT<gtsam::Vector3>::pack(vel1), gtsam::detail::VT<gtsam::Rot3>::pack(pose2),
                                   gtsam::detail::VT<gtsam::Vector3>::pack(vel2), nullptr, H1, H2, H3, H4, nullptr);
  }
  GPSLAM_FACTOR_BOILERPLATE_NAMED(GPInterpolatedAttitudeFactorRot3, 4, "GP Interpolated AttitudeFactor", true)
};

/// gpslam/slam/GPInterpolatedGPSFactorPose3.h:46-54
class GPInterpolatedGPSFactorPose3 : public gtsam::NonlinearFactor {
 public:
  GPInterpolatedGPSFactorPose3(const gtsam::Point3 &measured, const gtsam::SharedNoiseModel &meas_model, const gtsam::SharedNoiseModel &Qc_model,
                               gtsam::Key poseKey1, gtsam::Key velKey1, gtsam::Key poseKey2, gtsam::Key velKey2, double delta_t, double tau,
                               const gtsam::Pose3 *body_P_sensor = nullptr) {
    d_.type = gtsam::detail::F_INTERP_GPS; d_.manifold = GPSLAM_POSE3;
    d_.k[0] = poseKey1; d_.k[1] = velKey1; d_.k[2] = poseKey2; d_.k[3] = velKey2;
    d_.meas = {measured.x, measured.y, measured.z}; gtsam::noise_of(meas_model, d_); d_.Qc = Qc_model->covariance();
    d_.dt = delta_t; d_.tau = tau;
    if (body_P_sensor) d_.sensor = gtsam::detail::VT<gtsam::Pose3>::pack(*body_P_sensor);
  }
  /// gpslam/slam/GPInterpolatedGPSFactorPose3.h:66-95
  gtsam::Vector evaluateError(const gtsam::Pose3 &pose1, const gtsam::Vector6 &vel1, const gtsam::Pose3 &pose2, const gtsam::Vector6 &vel2,
                              gtsam::OptionalMatrix H1 = boost::none, gtsam::OptionalMatrix H2 = boost::none, gtsam::OptionalMatrix H3 = boost::none, gtsam::OptionalMatrix H4 = boost::none) const {
    return detail_g::meas_evaluate(d_, gtsam::detail::VT<gtsam::Pose3>::pack(pose1), gtsam::detail::VT<gtsam::Vector6>::pack(vel1), gtsam::detail::VT<gtsam::Pose3>::pack(pose2),
                                   gtsam::detail::VT<gtsam::Vector6>::pack(vel2), nullptr, H1, H2, H3, H4, nullptr);
  }
  GPSLAM_FACTOR_BOILERPLATE_NAMED(GPInterpolatedGPSFactorPose3, 4, "GPSFactor (GP interpolated)", true)
};

/// gpslam/gp/GaussianProcessPriorPose3VW.h:43-51 -- world-frame translational (v) and rotational (w) velocity keys
class GaussianProcessPriorPose3VW : public gtsam::NonlinearFactor {
 public:
  GaussianProcessPriorPose3VW(gtsam::Key poseKey1, gtsam::Key velKey1, gtsam::Key omegaKey1, gtsam::Key poseKey2,
                              gtsam::Key velKey2, gtsam::Key omegaKey2, double delta_t, const gtsam::SharedNoiseModel &Qc_model) {
    d_ = detail_g::gp(GPSLAM_POSE3, poseKey1, velKey1, poseKey2, velKey2, delta_t, Qc_model);
    d_.kw[0] = omegaKey1; d_.kw[1] = omegaKey2; d_.vw = true;
  }
  GPSLAM_FACTOR_BOILERPLATE_NAMED(GaussianProcessPriorPose3VW, 6, "4-way Gaussian Process Factor Pose3 VW", true)
};

/// gpslam/slam/GPInterpolatedGPSFactorPose3VW.h:50-60
class GPInterpolatedGPSFactorPose3VW : public gtsam::NonlinearFactor {
 public:
  GPInterpolatedGPSFactorPose3VW(const gtsam::Point3 &measured, const gtsam::SharedNoiseModel &meas_model,
                                 const gtsam::SharedNoiseModel &Qc_model, gtsam::Key poseKey1, gtsam::Key velKey1, gtsam::Key omegaKey1,
                                 gtsam::Key poseKey2, gtsam::Key velKey2, gtsam::Key omegaKey2, double delta_t, double tau,
                                 const gtsam::Pose3 *body_P_sensor = nullptr) {
    d_.type = gtsam::detail::F_INTERP_GPS; d_.manifold = GPSLAM_POSE3; d_.vw = true;
    d_.k[0] = poseKey1; d_.k[1] = velKey1; d_.k[2] = poseKey2; d_.k[3] = velKey2; d_.kw[0] = omegaKey1; d_.kw[1] = omegaKey2;
    d_.meas = {measured.x, measured.y, measured.z}; gtsam::noise_of(meas_model, d_); d_.Qc = Qc_model->covariance();
    d_.dt = delta_t; d_.tau = tau;
    if (body_P_sensor) d_.sensor = gtsam::detail::VT<gtsam::Pose3>::pack(*body_P_sensor);
  }
  GPSLAM_FACTOR_BOILERPLATE_NAMED(GPInterpolatedGPSFactorPose3VW, 6, "GPSFactor (GP interpolated, VW)", true)
};

/// gpslam/slam/GPInterpolatedProjectionFactorPose3.h:64-76 (CALIBRATION = gtsam::Cal3_S2).  throwCheirality /
/// verboseCheirality keep their defaults (false): a landmark behind the camera is masked on the device.
template <class CALIBRATION = gtsam::Cal3_S2>
class GPInterpolatedProjectionFactorPose3 : public gtsam::NonlinearFactor {
 public:
  GPInterpolatedProjectionFactorPose3(const gtsam::Point2 &measured, const gtsam::SharedNoiseModel &cam_model,
                                      const gtsam::SharedNoiseModel &Qc_model, gtsam::Key poseKey1, gtsam::Key velKey1,
                                      gtsam::Key poseKey2, gtsam::Key velKey2, gtsam::Key pointKey, double delta_t, double tau,
                                      const std::shared_ptr<CALIBRATION> &K, const gtsam::Pose3 *body_P_sensor = nullptr) {
    d_.type = gtsam::detail::F_INTERP_PROJ; d_.manifold = GPSLAM_POSE3;
    d_.k[0] = poseKey1; d_.k[1] = velKey1; d_.k[2] = poseKey2; d_.k[3] = velKey2; d_.k[4] = pointKey;
    d_.meas = {measured.x, measured.y}; gtsam::noise_of(cam_model, d_); d_.Qc = Qc_model->covariance();
    d_.dt = delta_t; d_.tau = tau; d_.aux = gtsam::detail::calibration_vector(*K);
    if (body_P_sensor) d_.sensor = gtsam::detail::VT<gtsam::Pose3>::pack(*body_P_sensor);
  }
  GPSLAM_FACTOR_BOILERPLATE_NAMED(GPInterpolatedProjectionFactorPose3<CALIBRATION>, 5, "GPInterpolatedProjectionFactor", true)
};

/// gpslam/slam/RangeFactor2DLinear.h:30-37
class RangeFactor2DLinear : public gtsam::NonlinearFactor {
 public:
  RangeFactor2DLinear(gtsam::Key poseKey, gtsam::Key pointKey, double measured, const gtsam::SharedNoiseModel &model) {
    d_.type = gtsam::detail::F_RANGE; d_.manifold = GPSLAM_LINEAR3; d_.k[0] = poseKey; d_.k[4] = pointKey;
    d_.meas = {measured}; gtsam::noise_of(model, d_);
  }
  GPSLAM_FACTOR_BOILERPLATE_NAMED(RangeFactor2DLinear, 2, "RangeFactor (2D linear)", true)
};
/// gpslam/slam/RangeFactorPose2.h:15 (typedef gtsam::RangeFactor<Pose2, Point2>)
class RangeFactorPose2 : public gtsam::NonlinearFactor {
 public:
  RangeFactorPose2(gtsam::Key poseKey, gtsam::Key pointKey, double measured, const gtsam::SharedNoiseModel &model) {
    d_.type = gtsam::detail::F_RANGE; d_.manifold = GPSLAM_POSE2; d_.k[0] = poseKey; d_.k[4] = pointKey;
    d_.meas = {measured}; gtsam::noise_of(model, d_);
  }
  GPSLAM_FACTOR_BOILERPLATE(RangeFactorPose2, 2)
};
/// gpslam/slam/RangeBearingFactor2DLinear.h:33-37 (range first, then bearing)
class RangeBearingFactor2DLinear : public gtsam::NonlinearFactor {
 public:
  RangeBearingFactor2DLinear(gtsam::Key poseKey, gtsam::Key pointKey, double range, double bearing, const gtsam::SharedNoiseModel &model) {
    d_.type = gtsam::detail::F_BEARING_RANGE; d_.manifold = GPSLAM_LINEAR3; d_.k[0] = poseKey; d_.k[4] = pointKey;
    d_.meas = {bearing, range}; gtsam::noise_of(model, d_);
  }
  GPSLAM_FACTOR_BOILERPLATE_NAMED(RangeBearingFactor2DLinear, 2, "RangeBearingFactor", true)
};
/// gpslam/slam/OdometryFactor2DLinear.h:38-40
class OdometryFactor2DLinear : public gtsam::NonlinearFactor {
 public:
  OdometryFactor2DLinear(gtsam::Key pose1Key, gtsam::Key pose2Key, const gtsam::Vector3 &betweenMeasured, const gtsam::SharedNoiseModel &model) {
    d_.type = gtsam::detail::F_ODOM2D; d_.manifold = GPSLAM_LINEAR3; d_.k[0] = pose1Key; d_.k[2] = pose2Key;
    d_.meas = {betweenMeasured[0], betweenMeasured[1], betweenMeasured[2]}; gtsam::noise_of(model, d_);
  }
  GPSLAM_FACTOR_BOILERPLATE_NAMED(OdometryFactor2DLinear, 2, "2-way projected odometry factor", true)
};

// ---- GaussianProcessInterpolator{Linear, Pose2, Pose3, Rot3}: the public query use of the interpolators (gpslam.h:57-86):
// ctor (Qc_model, delta_t, tau), interpolatePose(pose1, vel1, pose2, vel2, H1..H4)
#define GPSLAM_INTERPOLATOR(CLS, MANIFOLD, POSE, VEL)                                                            \
  class CLS {                                                                                                    \
   public:                                                                                                       \
    CLS(const gtsam::SharedNoiseModel &Qc_model, double delta_t, double tau)                                     \
        : Qc_(Qc_model->covariance()), delta_t_(delta_t), tau_(tau) {}                                           \
    POSE interpolatePose(const POSE &pose1, const VEL &vel1, const POSE &pose2, const VEL &vel2, gtsam::OptionalMatrix H1 = boost::none, \
                         gtsam::OptionalMatrix H2 = boost::none, gtsam::OptionalMatrix H3 = boost::none, gtsam::OptionalMatrix H4 = boost::none) const { \
      return detail_g::interpolate_one<POSE, VEL>(MANIFOLD, Qc_, delta_t_, tau_, pose1, vel1, pose2, vel2, H1, H2, H3, H4); \
    }                                                                                                            \
   private:                                                                                                      \
    gtsam::Matrix Qc_;                                                                                           \
    double delta_t_, tau_;                                                                                       \
  };
/// gpslam/gp/GaussianProcessInterpolatorPose3.h:43-105
GPSLAM_INTERPOLATOR(GaussianProcessInterpolatorPose3, GPSLAM_POSE3, gtsam::Pose3, gtsam::Vector6)
/// gpslam/gp/GaussianProcessInterpolatorPose2.h:42-89
GPSLAM_INTERPOLATOR(GaussianProcessInterpolatorPose2, GPSLAM_POSE2, gtsam::Pose2, gtsam::Vector3)
/// gpslam/gp/GaussianProcessInterpolatorRot3.h:42-86
GPSLAM_INTERPOLATOR(GaussianProcessInterpolatorRot3, GPSLAM_ROT3, gtsam::Rot3, gtsam::Vector3)
/// gpslam/gp/GaussianProcessInterpolatorLinear.h:52-90 (Dim = 2 or 3)
template <int Dim> class GaussianProcessInterpolatorLinear {
 public:
  GaussianProcessInterpolatorLinear(const gtsam::SharedNoiseModel &Qc_model, double delta_t, double tau)
      : Qc_(Qc_model->covariance()), delta_t_(delta_t), tau_(tau) { static_assert(Dim == 2 || Dim == 3, "DOF = {2, 3}"); }
  gtsam::VectorN<Dim> interpolatePose(const gtsam::VectorN<Dim> &pose1, const gtsam::VectorN<Dim> &vel1, const gtsam::VectorN<Dim> &pose2,
                                      const gtsam::VectorN<Dim> &vel2, gtsam::OptionalMatrix H1 = boost::none, gtsam::OptionalMatrix H2 = boost::none,
                                      gtsam::OptionalMatrix H3 = boost::none, gtsam::OptionalMatrix H4 = boost::none) const {
    return detail_g::interpolate_one<gtsam::VectorN<Dim>, gtsam::VectorN<Dim>>(Dim == 2 ? GPSLAM_LINEAR2 : GPSLAM_LINEAR3, Qc_, delta_t_, tau_,
                                                                               pose1, vel1, pose2, vel2, H1, H2, H3, H4);
  }
  /// interpolate velocity with Jacobians -- gpslam/gp/GaussianProcessInterpolatorLinear.h:106-126 (gpslam.h:193); evaluated on the
  /// device like interpolatePose (gpslam_hip_interpolate_velocities on a two-state session)
  gtsam::VectorN<Dim> interpolateVelocity(const gtsam::VectorN<Dim> &pose1, const gtsam::VectorN<Dim> &vel1, const gtsam::VectorN<Dim> &pose2,
                                          const gtsam::VectorN<Dim> &vel2, gtsam::OptionalMatrix H1 = boost::none, gtsam::OptionalMatrix H2 = boost::none,
                                          gtsam::OptionalMatrix H3 = boost::none, gtsam::OptionalMatrix H4 = boost::none) const {
    typedef gtsam::VectorN<Dim> V;
    detail_g::Single s(Dim == 2 ? GPSLAM_LINEAR2 : GPSLAM_LINEAR3, 0, gtsam::detail::VT<V>::pack(pose1), gtsam::detail::VT<V>::pack(vel1),
                       gtsam::detail::VT<V>::pack(pose2), gtsam::detail::VT<V>::pack(vel2), &Qc_, nullptr);
    const int32_t left = 0;
    std::vector<double> out(Dim), H((size_t)4 * Dim * Dim);
    gtsam::detail::check(gpslam_hip_interpolate_velocities(s.h, 1, &left, &delta_t_, &tau_, out.data(), H.data()), s.h, "interpolate_velocities");
    gtsam::Matrix *Hs[4] = {H1, H2, H3, H4};
    for (int m = 0; m < 4; m++) detail_g::fill(Hs[m], Dim, Dim, H.data() + (size_t)m * Dim * Dim, Dim);
    return gtsam::detail::VT<V>::un(out);
  }
 private:
  gtsam::Matrix Qc_;
  double delta_t_, tau_;
};

// ---- getBodyCentricVb / getBodyCentricVs (gpslam.h:161-164, gpslam/gp/Pose3utils.cpp:17-24; Barfoot14tro eq. 25): the MATLAB
// scripts initialise every velocity with them.  Evaluated on the device (gpslam_hip_body_centric_velocity); the batched
// overloads take all pose pairs of a trajectory in one call.
namespace detail_g {
inline std::vector<gtsam::Vector6> body_centric(int which, const std::vector<gtsam::Pose3> &pose1, const std::vector<gtsam::Pose3> &pose2,
                                                const std::vector<double> &delta_t) {
  if (pose1.size() != pose2.size() || pose1.size() != delta_t.size()) throw std::invalid_argument("getBodyCentricV*: argument lengths differ");
  const size_t n = pose1.size();
  std::vector<gtsam::Vector6> out(n);
  if (n == 0) return out;
  gpslam_hip_config_v2 cfg = gtsam::detail::make_config(GPSLAM_POSE3);
  gpslam_hip_handle *h = nullptr;
  if (gpslam_hip_create_v2(&cfg, &h) < 0) throw std::runtime_error("gpslam_hip_create_v2 failed: no usable HIP device (there is no CPU fallback)");
  std::vector<double> p1(n * 12), p2(n * 12), o(n * 6);
  for (size_t i = 0; i < n; i++) {
    const std::vector<double> a = gtsam::detail::VT<gtsam::Pose3>::pack(pose1[i]), b = gtsam::detail::VT<gtsam::Pose3>::pack(pose2[i]);
    std::memcpy(&p1[i * 12], a.data(), sizeof(double) * 12);
    std::memcpy(&p2[i * 12], b.data(), sizeof(double) * 12);
  }
  const int rc = gpslam_hip_body_centric_velocity(h, which, (int32_t)n, p1.data(), p2.data(), delta_t.data(), o.data());
  const std::string msg = rc < 0 ? gpslam_hip_last_error(h) : "";
  gpslam_hip_destroy(h);
  if (rc < 0) throw std::invalid_argument("getBodyCentricV*: " + msg);
  for (size_t i = 0; i < n; i++) for (int k = 0; k < 6; k++) out[i][k] = o[i * 6 + k];
  return out;
}
}  // namespace detail_g
inline gtsam::Vector6 getBodyCentricVb(const gtsam::Pose3 &pose1, const gtsam::Pose3 &pose2, double delta_t) {
  return detail_g::body_centric(0, {pose1}, {pose2}, {delta_t})[0];
}
inline gtsam::Vector6 getBodyCentricVs(const gtsam::Pose3 &pose1, const gtsam::Pose3 &pose2, double delta_t) {
  return detail_g::body_centric(1, {pose1}, {pose2}, {delta_t})[0];
}
inline std::vector<gtsam::Vector6> getBodyCentricVb(const std::vector<gtsam::Pose3> &pose1, const std::vector<gtsam::Pose3> &pose2, const std::vector<double> &delta_t) {
  return detail_g::body_centric(0, pose1, pose2, delta_t);
}
inline std::vector<gtsam::Vector6> getBodyCentricVs(const std::vector<gtsam::Pose3> &pose1, const std::vector<gtsam::Pose3> &pose2, const std::vector<double> &delta_t) {
  return detail_g::body_centric(1, pose1, pose2, delta_t);
}

}  // namespace gpslam
