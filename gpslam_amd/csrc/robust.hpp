// robust.hpp -- the M-estimators of gtsam::noiseModel::mEstimator (gtsam/linear/LossFunctions.h, GTSAM >= 4.1: weight() and loss()),
// one definition for the factor kernels (k_meas, k_clo_eval) and for the host (gpslam_hip_robust_eval).
//   r = |whitened error of the factor|_2,  u = r^2 / k^2
//   w(r)   multiplies the factor's rows and error as sqrt(w): noiseModel::Robust::WhitenSystem with Block reweighting,
//          noise_->WhitenSystem(A, b); robust_->reweight(A, b)
//   rho(r) is the factor's cost (Robust::loss), rho'(r) = w(r) r, rho(0) = 0, w(0) = 1
// The forms below are the table of include/gpslam_hip.h arranged so that no difference of nearly equal numbers is taken.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GPS_ROBUST_HD __host__ __device__
#else
#define GPS_ROBUST_HD
#endif

namespace gps {

enum RobustKind : int { ROBUST_NONE = 0, ROBUST_HUBER = 1, ROBUST_CAUCHY = 2, ROBUST_TUKEY = 3, ROBUST_GEMAN_MCCLURE = 4, ROBUST_WELSH = 5, ROBUST_FAIR = 6 };
constexpr int kNumRobustKinds = 7;

// x - log(1 + x), x >= 0: below 1 through log(1 + x) = 2 atanh(s), s = x / (2 + x), where x - 2 s = x^2 / (2 + x) exactly
GPS_ROBUST_HD inline double robust_x_minus_log1p(double x) {
  if (x >= 1.0) return x - log1p(x);
  const double s = x / (2.0 + x), s2 = s * s;
  double acc = 0.0;      // 1/3 + s^2 / 5 + s^4 / 7 + ...: s^2 <= 1/9, 18 terms reach 1e-18
#pragma unroll
  for (int n = 37; n >= 3; n -= 2) acc = acc * s2 + 1.0 / n;
  return x * x / (2.0 + x) - 2.0 * s * s2 * acc;
}

// w(r) and rho(r) of loss `kind` with parameter k > 0 at r >= 0 (ROBUST_NONE: 1 and r^2 / 2)
GPS_ROBUST_HD inline void robust_eval(int kind, double k, double r, double &w, double &rho) {
  const double k2 = k * k, r2 = r * r;
  switch (kind) {
    case ROBUST_HUBER:
      if (r <= k) { w = 1.0; rho = 0.5 * r2; }
      else { w = k / r; rho = k * (r - 0.5 * k); }
      return;
    case ROBUST_CAUCHY: {
      const double u = r2 / k2;
      w = 1.0 / (1.0 + u); rho = 0.5 * k2 * log1p(u);
      return;
    }
    case ROBUST_TUKEY: {
      if (r > k) { w = 0.0; rho = k2 / 6.0; return; }
      const double t = (k - r) * (k + r) / k2, u = r2 / k2;     // t = 1 - u, exact near r = k
      w = t * t;
      rho = k2 * (u < 0.5 ? u * (3.0 - 3.0 * u + u * u) : 1.0 - t * t * t) / 6.0;
      return;
    }
    case ROBUST_GEMAN_MCCLURE: {
      const double c = 1.0 / (1.0 + r2 / k2);
      w = c * c; rho = 0.5 * r2 * c;
      return;
    }
    case ROBUST_WELSH: {
      // exp(-u) carries u's relative error u-fold: u = (r / k)^2 as hi + lo (the division's and the square's remainders by fma)
      const double x = r / k, xr = fma(-x, k, r) / k;
      const double hi = x * x, lo = fma(x, x, -hi) + 2.0 * x * xr;
      w = exp(-hi) * (1.0 - lo); rho = -0.5 * k2 * expm1(-(hi + lo));
      return;
    }
    case ROBUST_FAIR: {
      const double x = r / k;
      w = 1.0 / (1.0 + x); rho = k2 * robust_x_minus_log1p(x);
      return;
    }
    default: w = 1.0; rho = 0.5 * r2;
  }
}

}  // namespace gps
